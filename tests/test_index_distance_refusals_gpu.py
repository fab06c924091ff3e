"""Every refusal of jsp_index_distance and jsp_sp_index_distance (include/jsplayer_amd.h, ERRORS): the activity call's, and three more
— a ref_frame outside its range, ref_frame and ref_picture that disagree, a ref_picture that is a host pointer or misaligned.  Each is
raised before anything is queued, leaves `out` and the reference picture as they were, the index as large as it was and the codec
where it stood, and jsp_last_error() starts with "index_distance:" — but for the wrong kind of codec, which keeps the text of the
other index calls."""
import ctypes as C

import numpy as np
import pytest

from jsplayer_amd import _native as N
from test_index_activity_refusals_gpu import CELLS, H, SENTINEL, W, Msv1, Sp

pytestmark = pytest.mark.gpu

REF_PICTURE = -2
CALLS = {Msv1: "jsp_index_distance", Sp: "jsp_sp_index_distance"}
IN_FLIGHT = "index_distance: an asynchronous frame is in flight (jsp_wait for it first)"
DISAGREE = "index_distance: ref_frame and ref_picture disagree (JSP_REF_PICTURE goes with a picture, a frame with none)"


@pytest.mark.parametrize("make", [Msv1, Sp], ids=["msvideo1", "screenpressor"])
def test_every_refusal(make):
    import torch
    s = make()
    lib = N.lib()
    fn, n = getattr(lib, CALLS[make]), s.idx.frames
    assert n == 6 and s.idx.ActivitySize() == (3, 2)
    s.idx.Distance(0)   # (a ScreenPressor index gets its per-frame table here: from now on nothing may grow)
    raw = torch.full((n * CELLS + 8,), SENTINEL, dtype=torch.int16, device="cuda")
    host = np.full(n * CELLS, SENTINEL, dtype=np.int16)
    dev, odd, hst = raw.data_ptr(), raw.data_ptr() + 1, host.ctypes.data
    pic = torch.full((W * H + 4,), 0x00ABCDEF, dtype=torch.int32, device="cuda")
    host_pic = np.full(W * H + 4, 0x00ABCDEF, dtype=np.int32)
    stands = {"prev": s.codec.PreviousFrame()}   # where the codec stands: moved by the test's own asynchronous frame only

    def info():
        k, d, h = C.c_int(0), C.c_uint64(0), C.c_uint64(0)
        assert getattr(lib, s.info_call)(s.idx._h, C.byref(k), C.byref(d), C.byref(h)) == 0
        return k.value, d.value, h.value

    before = info()

    def refused(what, message, c=s.codec._h, i=s.idx._h, ref=0, picture=None, first=0, count=n, out=dev, elems=n * CELLS):
        rc = fn(c, i, ref, C.c_void_p(picture) if picture else None, first, count, C.c_void_p(out) if out else None, elems)
        err = N.last_error()
        print(f"{CALLS[make]}: {what}: {err}")
        assert rc != 0 and err == message, (what, err)
        assert bool(torch.all(raw == SENTINEL)) and np.all(host == SENTINEL), what
        assert bool(torch.all(pic == 0x00ABCDEF)) and np.all(host_pic == 0x00ABCDEF), what
        assert info() == before and s.codec.PreviousFrame() is stands["prev"], what

    def dist(what):
        return "index_distance: " + what

    # ---- the activity call's refusals, with a frame and with a picture as the reference ---------------------------------------
    for kw in (dict(ref=0), dict(ref=REF_PICTURE, picture=pic.data_ptr())):
        refused("null codec", dist("null argument"), c=None, **kw)
        refused("null index", dist("null argument"), i=None, **kw)
        refused("null out", dist("null argument"), out=None, **kw)
        refused("wrong codec kind", s.wrong_kind, c=s.wrong._h, **kw)
        refused("foreign index", dist("the index was built by another codec"), i=s.foreign._h, **kw)
        for bad in (0, -1, 4097):
            refused(f"n = {bad}", dist("n is outside 1..4096"), count=bad, elems=1 << 20, **kw)
        refused("first < 0", dist("the run is outside the index"), first=-1, count=1, **kw)
        refused("first + n past the end", dist("the run is outside the index"), first=n - 2, count=3, **kw)
        refused("first = nframes", dist("the run is outside the index"), first=n, count=1, **kw)
        refused("first + n wraps in 32 bits", dist("the run is outside the index"), first=0x7FFFFFFF, count=4096, elems=1 << 20, **kw)
        refused("out_elems too small", dist("out_elems is smaller than the map"), elems=n * CELLS - 1, **kw)
        refused("misaligned out", dist("out is not aligned to 2 bytes"), out=odd, **kw)
        refused("host out", dist("out must be a device buffer"), out=hst, **kw)

    # ---- the three of its own ---------------------------------------------------------------------------------------------------
    for bad in (n, n + 1, -3, 0x7FFFFFFF, -0x80000000):
        refused(f"ref_frame = {bad}", dist("ref_frame is outside -1..nframes-1"), ref=bad)
    refused("JSP_REF_PICTURE without a picture", DISAGREE, ref=REF_PICTURE)
    for bad in (0, -1, n - 1, n):
        refused(f"a picture with ref_frame = {bad}", DISAGREE, ref=bad, picture=pic.data_ptr())
    for off in (1, 2, 3):
        refused(f"ref_picture {off} bytes off", dist("ref_picture is not aligned to 4 bytes"), ref=REF_PICTURE, picture=pic.data_ptr() + off)
    refused("host ref_picture", dist("ref_picture must be a device frame buffer"), ref=REF_PICTURE, picture=host_pic.ctypes.data)

    # ---- in flight ----------------------------------------------------------------------------------------------------------------
    frame_buf = torch.zeros(W * H, dtype=torch.int32, device="cuda")
    ticket = s.in_flight(frame_buf)
    stands["prev"] = s.codec.PreviousFrame()
    refused("in flight", IN_FLIGHT)
    refused("in flight, a picture", IN_FLIGHT, ref=REF_PICTURE, picture=pic.data_ptr())
    refused("in flight + host ref_picture", IN_FLIGHT, ref=REF_PICTURE, picture=host_pic.ctypes.data)
    s.codec.wait(ticket)

    # ---- and the calls that are not refused work after all that: a frame, a picture 4 bytes off a 16-byte boundary ---------------------
    assert fn(s.codec._h, s.idx._h, n - 1, None, 1, n - 1, C.c_void_p(dev), (n - 1) * CELLS) == 0, N.last_error()
    got = raw.cpu().numpy()
    assert np.array_equal(got[:(n - 1) * CELLS], s.idx.Distance(n - 1, 1, n - 1).cpu().numpy().reshape(-1))
    assert np.all(got[(n - 1) * CELLS:] == SENTINEL) and not got[(n - 2) * CELLS:(n - 1) * CELLS].any()
    assert fn(s.codec._h, s.idx._h, REF_PICTURE, C.c_void_p(pic.data_ptr() + 4), 0, n, C.c_void_p(dev), n * CELLS) == 0, N.last_error()
    got = raw.cpu().numpy()
    assert np.array_equal(got[:n * CELLS], s.idx.Distance(pic[1:1 + W * H]).cpu().numpy().reshape(-1)) and got[:n * CELLS].any()
    assert np.all(got[n * CELLS:] == SENTINEL)
    s.idx.close()
    s.foreign.close()
    for c in (s.codec, s.other, s.wrong):
        c.StopAndClean()
