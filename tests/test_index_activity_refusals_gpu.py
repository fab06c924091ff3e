"""Every refusal of jsp_index_activity and jsp_sp_index_activity (include/jsplayer_amd.h, ERRORS): each is raised before anything is
queued, leaves `out` as it was, the index as large as it was and the codec where it stood, and jsp_last_error() starts with
"index_activity:" — but for the wrong kind of codec, which keeps the text of the other index calls.  Then the order of the checks,
as tests/test_index_refusal_order_gpu.py pins it for the other calls that only borrow the codec: adjacent checks are violated
together and the earlier one must name itself."""
import ctypes as C

import numpy as np
import pytest

from jsplayer_amd import ScreenPressor
from jsplayer_amd import _native as N
from jsplayer_amd import streamgen as sg
from msv1_range_clips import make_gpu

pytestmark = pytest.mark.gpu

W, H = 40, 24            # 3 x 2 cells of either codec
CELLS = 6
SENTINEL = 0x7BCD
IN_FLIGHT = "index_activity: an asynchronous frame is in flight (jsp_wait for it first)"


class Msv1:
    call, size_call, info_call, wrong_kind = "jsp_index_activity", "jsp_index_activity_size", "jsp_index_info", "index: MSVideo1 only"

    def __init__(self):
        self.frames, self.keys, _ = sg.msv1_clip(41, W, H, 6, bits=16, p_mix=sg.msv1_p_mix(0.6, 3.0))
        self.codec, self.other = make_gpu(16, W, H), make_gpu(16, W, H)
        self.idx, self.foreign = self.codec.BuildIndex(self.frames, self.keys), self.other.BuildIndex(self.frames, self.keys)
        self.wrong = ScreenPressor(W, H, 24)

    def in_flight(self, buf):
        return self.codec.DecompressI_async(self.frames[0], buf)


class Sp:
    call, size_call, info_call, wrong_kind = "jsp_sp_index_activity", "jsp_sp_index_activity_size", "jsp_sp_index_info", "sp_index: ScreenPressor only"

    def __init__(self):
        self.frames, self.keys, _ = sg.sp_clip(71, W, H, 6, bpp=24, version=4)
        self.codec, self.other = ScreenPressor(W, H, 24), ScreenPressor(W, H, 24)
        self.idx = self.codec.BuildScrubIndex(self.frames, self.keys, key_row=5)
        self.foreign = self.other.BuildScrubIndex(self.frames, self.keys, key_row=5)
        self.wrong = make_gpu(16, W, H)

    def in_flight(self, buf):
        return self.codec.DecompressI_async(self.frames[0], buf)


@pytest.mark.parametrize("make", [Msv1, Sp], ids=["msvideo1", "screenpressor"])
def test_every_refusal_and_their_order(make):
    import torch
    s = make()
    lib = N.lib()
    fn, n = getattr(lib, s.call), s.idx.frames
    assert n == 6 and s.idx.ActivitySize() == (3, 2)
    s.idx.Activity()   # (a ScreenPressor index gets its per-frame table here: from now on nothing may grow)
    raw = torch.full((n * CELLS + 8,), SENTINEL, dtype=torch.int16, device="cuda")
    host = np.full(n * CELLS, SENTINEL, dtype=np.int16)
    dev, odd, hst = raw.data_ptr(), raw.data_ptr() + 1, host.ctypes.data
    stands = {"prev": s.codec.PreviousFrame()}   # where the codec stands: moved by the test's own asynchronous frame only

    def info():
        k, d, h = C.c_int(0), C.c_uint64(0), C.c_uint64(0)
        assert getattr(lib, s.info_call)(s.idx._h, C.byref(k), C.byref(d), C.byref(h)) == 0
        return k.value, d.value, h.value

    before = info()

    def refused(what, message, c=s.codec._h, i=s.idx._h, first=0, count=n, out=dev, elems=n * CELLS):
        rc = fn(c, i, first, count, C.c_void_p(out) if out else None, elems)
        err = N.last_error()
        print(f"{s.call}: {what}: {err}")
        assert rc != 0 and err == message, (what, err)
        assert bool(torch.all(raw == SENTINEL)) and np.all(host == SENTINEL), what
        assert info() == before and s.codec.PreviousFrame() is stands["prev"], what

    def act(what):
        return "index_activity: " + what

    # ---- each refusal alone --------------------------------------------------------------------------------------------------
    refused("null codec", act("null argument"), c=None)
    refused("null index", act("null argument"), i=None)
    refused("null out", act("null argument"), out=None)
    refused("wrong codec kind", s.wrong_kind, c=s.wrong._h)
    refused("foreign index", act("the index was built by another codec"), i=s.foreign._h)
    for bad in (0, -1, 4097):
        refused(f"n = {bad}", act("n is outside 1..4096"), count=bad, elems=1 << 20)
    refused("first < 0", act("the run is outside the index"), first=-1, count=1)
    refused("first + n past the end", act("the run is outside the index"), first=n - 2, count=3)
    refused("first = nframes", act("the run is outside the index"), first=n, count=1)
    refused("first + n wraps in 32 bits", act("the run is outside the index"), first=0x7FFFFFFF, count=4096, elems=1 << 20)
    refused("out_elems too small", act("out_elems is smaller than the map"), elems=n * CELLS - 1)
    refused("misaligned out", act("out is not aligned to 2 bytes"), out=odd)
    refused("host out", act("out must be a device buffer"), out=hst)
    cols, rows = C.c_int(7), C.c_int(7)
    assert getattr(lib, s.size_call)(None, C.byref(cols), C.byref(rows)) != 0 and N.last_error() == act("null argument")
    assert getattr(lib, s.size_call)(s.idx._h, None, C.byref(rows)) != 0 and (cols.value, rows.value) == (7, 7)

    # ---- the earlier refusal wins ---------------------------------------------------------------------------------------------
    refused("wrong codec kind + foreign index + bad n", s.wrong_kind, c=s.wrong._h, i=s.foreign._h, count=0)
    refused("foreign index + bad n", act("the index was built by another codec"), i=s.foreign._h, count=0)
    refused("bad n + bad first", act("n is outside 1..4096"), first=-1, count=0)
    refused("bad run + too-small out", act("the run is outside the index"), first=n - 1, count=2, elems=1)
    refused("too-small out + misaligned", act("out_elems is smaller than the map"), out=odd, elems=1)
    refused("misaligned + host out", act("out is not aligned to 2 bytes"), out=hst + 1)
    frame_buf = torch.zeros(W * H, dtype=torch.int32, device="cuda")
    ticket = s.in_flight(frame_buf)
    stands["prev"] = s.codec.PreviousFrame()
    refused("too-small out + in flight", act("out_elems is smaller than the map"), elems=1)
    refused("misaligned + in flight", act("out is not aligned to 2 bytes"), out=odd)
    refused("in flight + host out", IN_FLIGHT, out=hst)
    refused("in flight", IN_FLIGHT)
    s.codec.wait(ticket)

    # ---- and the call that is not refused works after all that --------------------------------------------------------------------
    assert fn(s.codec._h, s.idx._h, 1, n - 1, C.c_void_p(dev), (n - 1) * CELLS) == 0, N.last_error()
    got = raw.cpu().numpy()
    assert np.array_equal(got[:(n - 1) * CELLS], s.idx.Activity(1, n - 1).cpu().numpy().reshape(-1))
    assert np.all(got[(n - 1) * CELLS:] == SENTINEL)
    s.idx.close()
    s.foreign.close()
    for c in (s.codec, s.other, s.wrong):
        c.StopAndClean()
