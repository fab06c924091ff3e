"""Which refusal wins when a call that only borrows the codec — Thumbs, Present, Tensor of an MSVideo1 seek index — is wrong on two
counts: the order of the checks in jsp_index_thumbs / jsp_index_present / jsp_index_tensor (msv1_seek.cpp), which the per-call
refusal tests do not pin because each of their inputs is wrong in one way only.

Every adjacent pair of a call's checks is violated together, in source order, and the earlier one must name itself: the whole text
of the CodecError is asserted, `out` keeps its poison and jsp_index_info says what it said before.  The order, per call:

  kind of codec ("index_thumbs: ..." for Thumbs, "index: ..." for the other two) -> the index is this codec's -> n and, for Present
  and Tensor, the window / the size of out -> the frame numbers -> for Thumbs scale, cols and the size of out -> nothing in flight
  -> out is device memory."""
import ctypes as C

import numpy as np
import pytest

from jsplayer_amd import CodecError, ScreenPressor
from jsplayer_amd import _native as N
from jsplayer_amd import streamgen as sg
from msv1_range_clips import POISON, dev_buf, make_gpu

pytestmark = pytest.mark.gpu

W = H = 8
FOREIGN = "the index was built by another codec"
BAD_FRAME = "a frame number is outside the index"
IN_FLIGHT = "an asynchronous frame is in flight (jsp_wait for it first)"
WINDOW = "window size outside 1..16384"


def thumbs_cases():
    """The call, the name its kind check gives itself, and (what is wrong, the message, arguments of the call; small: room for one cell)."""
    return "index_thumbs", "index_thumbs", [
        ("bad frame number + bad scale", BAD_FRAME, dict(frames=[0, 3], scale=5)),
        ("bad cols + in flight", "cols must be at least 1", dict(frames=[0, 1], cols=0)),
        ("too-small out + in flight", "out_pixels is smaller than the sheet", dict(frames=[0, 1], small=True)),
    ]


def present_cases():
    return "index_present", "index", [
        ("bad window + bad frame number", WINDOW, dict(frames=[0, 3], win_w=0)),
        ("too-small out + bad frame number", "out_ints is smaller than the sheet", dict(frames=[0, 3], small=True)),
        ("bad cols + in flight", "cols must be at least 1", dict(frames=[0, 1], cols=0)),
        ("too-small out + in flight", "out_ints is smaller than the sheet", dict(frames=[0, 1], small=True)),
    ]


def tensor_cases():
    return "index_tensor", "index", [
        ("bad window + bad frame number", WINDOW, dict(frames=[0, 3], win_w=0)),
        ("too-small out + bad frame number", "out_bytes is smaller than the tensor", dict(frames=[0, 3], small=True)),
        ("too-small out + in flight", "out_bytes is smaller than the tensor", dict(frames=[0, 1], small=True)),
    ]


@pytest.mark.parametrize("cases", [thumbs_cases, present_cases, tensor_cases], ids=["thumbs", "present", "tensor"])
def test_the_earlier_refusal_wins(cases):
    import torch
    who, kind_who, own = cases()
    frames, keys, _ = sg.msv1_clip(41, W, H, 3, bits=16, p_mix=sg.msv1_p_mix(0.6, 3.0))
    a, other, sp = make_gpu(16, W, H), make_gpu(16, W, H), ScreenPressor(64, 48, 24)
    idx = a.BuildIndex(frames, keys)
    assert idx.frames == 3
    lib = N.lib()
    tensor = who == "index_tensor"
    # room for two cells: Thumbs at scale 4 gives 2 x 2 pixels a frame, Present an 8 x 8 window, Tensor 3 x 8 x 8 floats
    cell = {"index_thumbs": 2 * 2, "index_present": W * H, "index_tensor": 3 * W * H}[who]
    out = torch.full((2 * cell,), -7.0, dtype=torch.float32, device="cuda") if tensor else dev_buf(2 * cell)
    host = np.full(2 * cell, -7.0, dtype=np.float32) if tensor else np.full(2 * cell, POISON, dtype=np.uint32).view(np.int32)
    host_out = torch.from_numpy(host) if tensor else host

    def info():
        n, dev, hostb = C.c_int(0), C.c_uint64(0), C.c_uint64(0)
        assert lib.jsp_index_info(idx._h, C.byref(n), C.byref(dev), C.byref(hostb)) == 0
        return n.value, dev.value, hostb.value

    def call(frames, scale=4, cols=1, win_w=W, small=False, to=None):
        to = (out[:cell] if small else out) if to is None else to
        if who == "index_thumbs":
            idx.Thumbs(frames, scale=scale, cols=cols, out=to)
        elif who == "index_present":
            idx.Present(frames, win_w, H, 1.0, 0.0, 0.0, cols=cols, out=to)
        else:
            idx.Tensor(frames, win_w, H, 1.0, 0.0, 0.0, out=to)

    before = info()

    def refused(what, message, **kw):
        with pytest.raises(CodecError) as e:
            call(**kw)
        print(f"{who}: {what}: {e.value}")
        assert str(e.value) == message, what
        assert info() == before, what
        if tensor:
            assert bool(torch.all(out == -7.0)) and np.all(host == -7.0), what
        else:
            assert np.all(out.cpu().numpy().view(np.uint32) == POISON) and np.all(host.view(np.uint32) == POISON), what

    if who == "index_thumbs":
        assert idx.ThumbSize(4) == (2, 2)

    # ---- nothing in flight ----
    idx._codec = sp   # ScreenPressor, and not the codec that built the index either
    refused("wrong codec kind + foreign index", f"{kind_who}: MSVideo1 only", frames=[0])
    idx._codec = other
    refused("foreign index + n out of range", f"{who}: {FOREIGN}", frames=[])
    refused("foreign index + n out of range", f"{who}: {FOREIGN}", frames=[0] * 4097)
    idx._codec = a
    for what, message, kw in own:
        if "in flight" not in what:
            refused(what, f"{who}: {message}", **kw)

    # ---- an asynchronous frame in flight ----
    assert keys[0]
    frame_buf = dev_buf(W * H)
    ticket = a.DecompressI_async(frames[0], frame_buf)
    for what, message, kw in own:
        if "in flight" in what:
            refused(what, f"{who}: {message}", **kw)
    refused("bad frame number + in flight", f"{who}: {BAD_FRAME}", frames=[0, 3])
    refused("in flight + host out", f"{who}: {IN_FLIGHT}", frames=[0], to=host_out)
    a.wait(ticket)

    # alone, the later one of the last pair; and the call still works
    refused("host out", f"{who}: out must be a device buffer", frames=[0], to=host_out)
    call(frames=[0, 1])
    idx.close()
    for c in (a, other, sp):
        c.StopAndClean()
