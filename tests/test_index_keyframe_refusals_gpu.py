"""Every argument refusal of jsp_index_key_frame (include/jsplayer_amd.h, ERRORS): each is raised before anything is queued, leaves
`out` as it was, *len 0, the index as large as it was and the codec where it stood, and jsp_last_error() starts with
"index_key_frame:" — but for the wrong kind of codec, which keeps the text of the other index calls.  Then the order of the checks, as
tests/test_index_refusal_order_gpu.py pins it for the other calls that only borrow the codec: adjacent checks are violated together
and the earlier one must name itself."""
import ctypes as C

import numpy as np
import pytest

from jsplayer_amd import ScreenPressor
from jsplayer_amd import _native as N
from jsplayer_amd import streamgen as sg
from msv1_range_clips import make_gpu

pytestmark = pytest.mark.gpu

W, H = 40, 24
FILL = 0xA5
IN_FLIGHT = "index_key_frame: an asynchronous frame is in flight (jsp_wait for it first)"


def test_every_refusal_and_their_order():
    import torch
    frames, keys, _ = sg.msv1_clip(41, W, H, 6, bits=16, p_mix=sg.msv1_p_mix(0.6, 3.0))
    codec, other = make_gpu(16, W, H), make_gpu(16, W, H)
    idx, foreign = codec.BuildIndex(frames, keys), other.BuildIndex(frames, keys)
    wrong = ScreenPressor(W, H, 24)
    tiny = make_gpu(16, 3, 8)                                    # a picture without a 4x4 block
    tiny_idx = tiny.BuildIndex([b"\x01\x02\x03\x04", b""], [True, False])
    lib = N.lib()
    fn, n = lib.jsp_index_key_frame, idx.frames
    bound = idx.KeyFrameBound()
    assert n == 6 and bound == (W // 4) * (H // 4) * 18
    first = idx.KeyFrame(0)                                      # (the scratch is allocated here: from now on nothing may grow)
    out = np.full(bound, FILL, dtype=np.uint8)
    stands = {"prev": codec.PreviousFrame()}   # where the codec stands: moved by the test's own asynchronous frame only

    def info():
        k, d, h = C.c_int(0), C.c_uint64(0), C.c_uint64(0)
        assert lib.jsp_index_info(idx._h, C.byref(k), C.byref(d), C.byref(h)) == 0
        return k.value, d.value, h.value

    before = info()

    def refused(what, message, c=codec._h, i=idx._h, t=0, dst=out.ctypes.data, cap=bound, length=True):
        size = C.c_size_t(777)
        rc = fn(c, i, t, C.c_void_p(dst) if dst else None, cap, C.byref(size) if length else None)
        err = N.last_error()
        print(f"jsp_index_key_frame: {what}: {err}")
        assert rc != 0 and err == message, (what, err)
        assert size.value == (0 if length else 777) and np.all(out == FILL), what
        assert info() == before and codec.PreviousFrame() is stands["prev"], what

    def kf(what):
        return "index_key_frame: " + what

    # ---- each refusal alone --------------------------------------------------------------------------------------------------
    refused("null codec", kf("null argument"), c=None)
    refused("null index", kf("null argument"), i=None)
    refused("null out with a cap", kf("null argument"), dst=None)
    refused("null len", kf("null argument"), length=False)
    refused("wrong codec kind", "index: MSVideo1 only", c=wrong._h)
    refused("foreign index", kf("the index was built by another codec"), i=foreign._h)
    for bad in (-1, n, 0x7FFFFFFF):
        refused(f"t = {bad}", kf("t is outside the index"), t=bad)
    refused("no block", kf("the picture has no 4x4 block"), c=tiny._h, i=tiny_idx._h)
    size = C.c_size_t(7)
    assert lib.jsp_index_key_frame_bound(None, C.byref(size)) != 0 and N.last_error() == kf("null argument") and size.value == 7
    assert lib.jsp_index_key_frame_bound(idx._h, None) != 0 and N.last_error() == kf("null argument")

    # ---- the earlier refusal wins ---------------------------------------------------------------------------------------------
    refused("wrong codec kind + foreign index + bad t", "index: MSVideo1 only", c=wrong._h, i=foreign._h, t=-1)
    refused("foreign index + bad t", kf("the index was built by another codec"), i=foreign._h, t=n)
    refused("foreign index + no block", kf("the index was built by another codec"), c=codec._h, i=tiny_idx._h)
    refused("bad t + no block", kf("t is outside the index"), c=tiny._h, i=tiny_idx._h, t=2)
    frame_buf = torch.zeros(W * H, dtype=torch.int32, device="cuda")
    ticket = codec.DecompressI_async(frames[0], frame_buf)
    stands["prev"] = codec.PreviousFrame()
    refused("bad t + in flight", kf("t is outside the index"), t=n)
    refused("foreign index + in flight", kf("the index was built by another codec"), i=foreign._h)
    refused("in flight", IN_FLIGHT)
    refused("in flight + too-small cap", IN_FLIGHT, cap=1)
    codec.wait(ticket)

    # ---- and the call that is not refused works after all that --------------------------------------------------------------------
    size = C.c_size_t(0)
    assert fn(codec._h, idx._h, 0, C.c_void_p(out.ctypes.data), bound, C.byref(size)) == 0, N.last_error()
    assert out[:size.value].tobytes() == first and np.all(out[size.value:] == FILL)
    for x in (idx, foreign, tiny_idx):
        x.close()
    for c in (codec, other, wrong, tiny):
        c.StopAndClean()
