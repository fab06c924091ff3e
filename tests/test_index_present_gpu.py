"""Frames of an MSVideo1 seek index straight into a window (jsp_index_present, SeekIndex.Present, jsp_play --index-present) on an
MI355X.

Truth is the oracle, not the library: the clip decoded frame by frame with OracleMSVideo1 into buffers that start as zeros
(test_index_thumbs_gpu.oracle_pictures' rule, restated here), then the contract in numpy (tests/index_present_ref.py over view_ref /
view_area_ref).  The cross-check on the device is Show into a zeroed buffer followed by display_present / display_present_area.  Every
comparison is exact.

Sizes (the kernel's constants are in tests/index_present_cases.py): the picture, 134 x 98, is larger than one 64 x 64 source tile in
both axes with X % 4 = Y % 4 = 2; the range has 72 frames, so last writers sit in three bitmap words, and about a tenth of the blocks
have no writer at all; every window but the tiny ones is larger than one output rectangle in both axes."""
import ctypes as C
import os
import subprocess
import zlib

import numpy as np
import pytest

import index_present_cases as ic
import index_present_ref as ipr
import msv1_range_clips as rc
import view_ref as vr
from jsplayer_amd import CodecError, ScreenPressor
from jsplayer_amd.codec import display_present, display_present_area
from jsplayer_amd import _native as N
from jsplayer_amd import streamgen as sg
from oracle_binding import OracleMSVideo1

pytestmark = pytest.mark.gpu

FN = "index_present"
POISON = ic.POISON
W, H = 134, 98
START, NF = 3, 72                              # frames decoded before the range; frames of the range
PICKS = [71, 0, 33, 64, 33, 5, 31]             # unordered, one twice; frames of all three bitmap words
PARSE = "host"


@pytest.fixture(autouse=True, params=["host", "gpu"])
def parse_mode(request):
    """Every test runs with the block tables of the host parser and of the on-GPU parse."""
    global PARSE
    PARSE = request.param
    yield request.param
    PARSE = "host"


def make_gpu(bits, w=W, h=H, pal=None):
    return rc.make_gpu(bits, w, h, pal, parse=PARSE)


def oracle_pictures(bits, w, h, pal, frames, keys, lines=36):
    """The picture after every frame, buffers starting as zeros, each destination first copied from the picture before it."""
    o = OracleMSVideo1(bits, w, h, pal)
    o.Preinit(lines)
    bufs = [np.zeros(w * h, dtype=np.int32) for _ in range(3)]
    out = []
    for src, key in zip(frames, keys):
        prev = o.PreviousFrame()
        dst = next(b for b in bufs if b is not prev)
        if prev is not None:
            np.copyto(dst, prev)
        else:
            dst.fill(0)
        if key:
            assert o.DecompressI(src, dst) == 0
        else:
            o.DecompressP(src, dst)
        pic = o.PreviousFrame()
        out.append(np.zeros(w * h, dtype=np.int32) if pic is None else pic.copy())
    o.close()
    return out


_CLIPS = {}


def clip(bits, before):
    """(frames, keys, palette, the oracle's pictures, frames in front of the range).  before: the range starts behind START decoded
    frames and its 72 inter frames skip 97 % of their blocks; else it is the whole clip from its key frame on a fresh codec — for 8-bit
    a key frame that stops at an end marker part-way, so that blocks no frame coded show 0 with nothing before them."""
    if (bits, before) in _CLIPS:
        return _CLIPS[(bits, before)]
    frames, keys, pal = sg.msv1_clip(940 + bits, W, H, START + NF, bits=bits, p_mix=sg.msv1_p_mix(0.97, 30.0), key_every=1000)
    frames, keys = list(frames), list(keys)
    start = START
    if not before:
        start = 0
        frames, keys = frames[:1] + frames[START + 1:], keys[:1] + keys[START + 1:]      # 72 frames again
        if bits == 8:
            gen = rc.Idle(8, W, H, 5)
            at = 9 * gen.nbx + 7                                                          # part-way through a block row
            frames[0] = gen.key()[: 2 * at] + b"\x00\x00"                                 # (solid 8-bit codes: two bytes a block)
    assert len(frames) - start == NF
    pictures = oracle_pictures(bits, W, H, pal, frames, keys)
    # the structure the sizes are chosen for: last writers of the range's last frame in three bitmap words, blocks with none
    nbx, nby = W // 4, H // 4
    last = np.full(nbx * nby, -1)
    for t in range(NF):
        coded = rc.coded_blocks(bits, nbx, nby, frames[start + t], have_prev=start + t > 0)[0]
        last[coded] = t
    assert {0, 1, 2} <= set(int(v) >> 5 for v in last if v >= 0)
    if before or bits == 8:
        assert 20 <= int((last < 0).sum()) < nbx * nby // 2
    _CLIPS[(bits, before)] = (frames, keys, pal, pictures, start)
    return _CLIPS[(bits, before)]


class Session:
    """A codec with the frames in front of the range decoded, and the index over the range."""

    def __init__(self, bits, before):
        self.frames, self.keys, self.pal, pictures, self.start = clip(bits, before)
        self.pictures = pictures[self.start:]
        self.gpu = make_gpu(bits, pal=self.pal)
        self.pool = [ic.dev_buf(W * H, 0) for _ in range(3)]
        for i in range(self.start):
            prev = self.gpu.PreviousFrame()
            dst = next(b for b in self.pool if b is not prev)
            if prev is not None:
                dst.copy_(prev)
            if self.keys[i]:
                assert self.gpu.DecompressI(self.frames[i], dst) == 0
            else:
                self.gpu.DecompressP(self.frames[i], dst)
        self.idx = self.gpu.BuildIndex(self.frames[self.start:], self.keys[self.start:])
        assert self.idx.frames == NF

    def close(self):
        self.idx.close()
        self.gpu.StopAndClean()


@pytest.mark.parametrize("before", [True, False], ids=["before", "fresh"])
@pytest.mark.parametrize("bits", [16, 8])
def test_the_windows_match_the_oracle_and_show_plus_present(bits, before):
    s = Session(bits, before)
    what = f"{bits}-bit {'behind a picture' if before else 'fresh codec'} ({PARSE} parse)"
    scratch, win = ic.dev_buf(W * H, 0), None
    for name, ww, wh, k, dx, dy, filters in ic.windows(W, H):
        sheets = {}
        for f in filters:
            sheets[f] = ic.check(FN, s.gpu, s.idx, s.pictures, PICKS, W, H, ww, wh, k, dx, dy, vr.CANVAS, f, cols=3, what=f"{what} {name}")
        if name == "crop100":                                             # the three filters agree on a plain crop
            assert np.array_equal(sheets[0], sheets[1]) and np.array_equal(sheets[0], sheets[2])
        if name == "quirk200":                                            # background at the left of every cell
            pitch = 3 * ww
            assert np.all(sheets[1][:pitch].reshape(3, ww)[:, :33] == ic.BG) and sheets[1][33] != ic.BG
        # the cross-check on the device: Show into a zeroed buffer, then the present call of the filter
        for i in (0, 2, 5):                                               # frames 71, 33 and 5: one of every bitmap word
            scratch.zero_()
            r = s.idx.Show(PICKS[i], scratch, adopt=False)
            shown = scratch if r.data_pnt is scratch else r.data_pnt
            for f in filters:
                win = ic.dev_buf(ww * wh)
                if f == ipr.AREA:
                    display_present_area(shown, W, H, win, ww, wh, k, dx, dy, background=ic.BG)
                else:
                    display_present(shown, W, H, win, ww, wh, k, dx, dy, filter=f, background=ic.BG)
                cell = ic.cell_of(sheets[f], i, 3, ww, wh)
                assert np.array_equal(win.cpu().numpy().view(np.uint32).reshape(wh, ww), cell), f"{what} {name} frame {PICKS[i]} filter {f}: not Show + present"
    s.close()


@pytest.mark.parametrize("bits", [16, 8])
def test_modes_pitch_padding_alignment_and_the_cells_past_n(bits):
    s = Session(bits, True)
    what = f"{bits}-bit ({PARSE} parse)"
    k, dx, dy = vr.view_matrix(W, H, 101, 73, 0, 0.5, 0.5)
    picks5 = PICKS[:5]
    for mode in ic.MODES:
        for f in ipr.FILTERS:
            # n = 5, cols = 2: the sixth cell, 7 ints of padding a row, the words behind the sheet all keep the poison; width 101 is no
            # multiple of 4 (scalar stores at every row's end, no cell row but the first on a 16-byte boundary)
            ic.check(FN, s.gpu, s.idx, s.pictures, picks5, W, H, 101, 73, k, dx, dy, mode, f, cols=2, pad=7, what=what)
    for f in ipr.FILTERS:
        ic.check(FN, s.gpu, s.idx, s.pictures, picks5, W, H, 100, 37, k, dx, dy, vr.CANVAS, f, cols=2, pad=4, what=what)            # 16-byte stores throughout
        ic.check(FN, s.gpu, s.idx, s.pictures, picks5, W, H, 100, 37, k, dx, dy, vr.CANVAS, f, cols=2, pad=4, offset=1, what=what)  # `out` one int off
        ic.check(FN, s.gpu, s.idx, s.pictures, [40], W, H, 100, 73, k, dx, dy, vr.CANVAS, f, what=what)                             # n = 1, cols = 1: the plain window
    # Present: the sheet as a tensor, new (zero-filled) or the caller's
    got = s.idx.Present(picks5, 50, 36, 0.37, 1.5, 2.5, filter=ipr.AREA, cols=2)
    want = ipr.sheet([s.pictures[t] for t in picks5], W, H, 50, 36, 0.37, 1.5, 2.5, filter=ipr.AREA, cols=2, fill=0)
    assert tuple(got.shape) == (3 * 36, 100) and np.array_equal(got.cpu().numpy().view(np.uint32).reshape(-1), want)
    out = ic.dev_buf(3 * 36 * 100 + 5)
    got = s.idx.Present(picks5, 50, 36, 0.37, 1.5, 2.5, mode=vr.SETPIXELS, filter=ipr.NEAREST, background=0x01020304, cols=2, out=out)
    want = ipr.sheet([s.pictures[t] for t in picks5], W, H, 50, 36, 0.37, 1.5, 2.5, mode=vr.SETPIXELS, filter=ipr.NEAREST, background=0x01020304, cols=2,
                     fill=POISON, total=3 * 36 * 100 + 5)
    assert got.data_ptr() == out.data_ptr() and np.array_equal(out.cpu().numpy().view(np.uint32), want)
    s.close()


def info(idx):
    n, dev, host = C.c_int(0), C.c_uint64(0), C.c_uint64(0)
    assert idx._lib.jsp_index_info(idx._h, C.byref(n), C.byref(dev), C.byref(host)) == 0
    return dev.value, host.value


@pytest.mark.parametrize("bits", [16, 8])
def test_the_codec_is_only_lent(bits):
    """A session that presents and one that does not: the previous frame, the block-change counter and the next inter frame come out
    the same; poisoned pool buffers stay poisoned; the index grows by the frame list, not by a picture."""
    runs = []
    for present in (True, False):
        s = Session(bits, True)
        prev = s.gpu.PreviousFrame()
        prev_pixels = prev.cpu().numpy().copy()
        free = [b for b in s.pool if b is not prev]
        for b in free:
            b.fill_(POISON)
        dev0, _ = info(s.idx)
        if present:
            k, dx, dy = vr.view_matrix(W, H, 100, 73, 0, 0.5, 0.5)
            for f in ipr.FILTERS:
                s.idx.Present(PICKS, 100, 73, k, dx, dy, filter=f, cols=4)
            s.idx.Present(list(range(NF)) * 3, 9, 7, 0.05, 0.0, 0.0, filter=ipr.AREA, cols=16)
            dev1, _ = info(s.idx)
            assert 4 * 3 * NF <= dev1 - dev0 < W * H * 4
        assert s.gpu.PreviousFrame() is prev and np.array_equal(prev.cpu().numpy(), prev_pixels)
        for b in free:
            assert bool((b == POISON).all()), "Present wrote a frame buffer"
        changes = s.gpu.counter("msv1_block_changes")
        nxt = free[0]
        nxt.copy_(prev)
        r = s.gpu.DecompressP(s.frames[s.start], nxt)
        runs.append((changes, s.gpu.counter("msv1_block_changes"), r.significant_changes, r.data_pnt is nxt, s.gpu.PreviousFrame().cpu().numpy().copy()))
        assert np.array_equal(runs[-1][4], s.pictures[0])
        s.close()
    a, b = runs
    assert a[:4] == b[:4] and np.array_equal(a[4], b[4])


def test_every_refusal_leaves_out_untouched_and_names_the_call():
    s = Session(16, True)
    a, idx = s.gpu, s.idx
    ww, wh = 20, 10
    out = ic.dev_buf(4 * ww * wh)
    good = dict(frames=[0], out=out, win_w=ww, win_h=wh, pitch=ww, cols=1, k=0.5, dx=0.0, dy=0.0, mode=vr.CANVAS, filter=ipr.BILINEAR)

    def refused(match, codec=None, prefix="index_present:", **kw):
        args = dict(good, **kw)
        with pytest.raises(CodecError, match=match) as e:
            ic.call(FN, codec or a, idx, **args)
        assert str(e.value).startswith(prefix), str(e.value)
        assert bool((out == POISON).all()), match + ": out was written"

    refused("1..4096", frames=[])
    refused("1..4096", frames=[0] * 4097)
    for bad in (0, -1, 16385):
        refused("window size", win_w=bad, pitch=max(bad, 1))
        refused("window size", win_h=bad)
    for bad in (1.0 / 65, 64.5, 0.0, -1.0):
        refused("k outside", k=bad)
    for name in ("k", "dx", "dy"):
        for bad in (float("nan"), float("inf"), -float("inf")):
            refused("finite", **{name: bad})
    for bad in (-1, 4, 99):
        refused("unknown mode", mode=bad)
    for bad in (-1, 3):
        refused("unknown filter", filter=bad)
    for bad in (0, -2):
        refused("cols", frames=[0, 1], cols=bad)
    for bad in (-1, NF, 1 << 20):
        refused("outside the index", frames=[0, bad], pitch=ww)
    refused("out_pitch", pitch=ww - 1)
    refused("out_pitch", frames=[0, 1], cols=2, pitch=2 * ww - 1)
    refused("smaller than the sheet", frames=[0, 1, 2, 3, 4])                              # five cells, room for four
    refused("smaller than the sheet", frames=[0, 1, 2], cols=2, pitch=2 * ww, out_ints=4 * ww * wh - 1)   # two sheet rows of two cells
    refused("smaller than the sheet", pitch=ww + 1, out_ints=(wh - 1) * (ww + 1) + ww - 1)
    host = np.full(4 * ww * wh, POISON, dtype=np.uint32).view(np.int32)
    refused("device buffer", out=host)
    assert np.all(host.view(np.uint32) == POISON)
    prev = a.PreviousFrame()
    ticket = a.DecompressP_async(s.frames[s.start], next(b for b in s.pool if b is not prev))
    refused("in flight")
    a.wait(ticket)
    # null arguments (the C ABI itself)
    lib = N.lib()
    one = (C.c_int * 1)(0)
    tail = (out.numel(), ww, wh, ww, 1, 0.5, 0.0, 0.0, 0, 1, 0)
    for args in ((None, idx._h, 1, one, C.c_void_p(out.data_ptr())), (a._h, None, 1, one, C.c_void_p(out.data_ptr())),
                 (a._h, idx._h, 1, None, C.c_void_p(out.data_ptr())), (a._h, idx._h, 1, one, None)):
        assert lib.jsp_index_present(*args, *tail) != 0 and N.last_error().startswith("index_present: null argument")
    # an index of another codec; ScreenPressor
    other = make_gpu(16)
    refused("another codec", codec=other)
    sp = ScreenPressor(W, H, 24)
    refused("MSVideo1 only", codec=sp, prefix="index: MSVideo1 only")
    sp.StopAndClean()
    other.StopAndClean()
    assert bool((out == POISON).all())
    # and the call still works; a closed index / codec raise as Thumbs does
    ic.check(FN, a, idx, s.pictures, [1, 0], W, H, ww, wh, 0.5, 0.0, 0.0, vr.CANVAS, ipr.BILINEAR, cols=2)
    idx.close()
    with pytest.raises(CodecError, match="index is closed"):
        idx.Present([0], ww, wh, 0.5, 0, 0)
    idx2 = a.BuildIndex(s.frames[s.start:], s.keys[s.start:])
    a.StopAndClean()
    with pytest.raises(CodecError, match="codec is closed"):
        idx2.Present([0], ww, wh, 0.5, 0, 0)
    idx2.close()


def test_jsp_play_index_present_prints_the_crcs_of_show_plus_present(tmp_path):
    from jsplayer_amd import avi
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "examples", "jsp_play")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-s", "-C", os.path.join(root, "examples")])
    w, h, n = 320, 240, 40
    frames, keys, _ = sg.msv1_clip(97, w, h, n, p_mix=sg.msv1_p_mix(0.7, 6.0), key_every=16)
    path = tmp_path / "clip.avi"
    path.write_bytes(avi.write_avi(w, h, frames, fourcc=b"CRAM", bpp=16, fps=15.0, key_flags=keys))
    picks = [(i * n) // 9 for i in range(9)]
    for spec, zoom, hpos, vpos, filter in (("90x50", 0, 0.5, 0.5, 1), ("160x90:2:0.3:0.8", 2, 0.3, 0.8, 0), ("90x50", 0, 0.5, 0.5, 2)):
        ww, wh = (int(v) for v in spec.split(":")[0].split("x"))
        res = subprocess.run([exe, str(path), "--index-present", spec, "9" if filter == 1 else f"9:{filter}"], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                             timeout=120)
        assert res.returncode == 0, res.stderr.decode()
        lines = [l.split() for l in res.stdout.decode().splitlines() if l and l[0].isdigit()]
        assert [int(l[0]) for l in lines] == picks
        k, dx, dy = vr.view_matrix(w, h, ww, wh, zoom, hpos, vpos)
        g = make_gpu(16, w, h)
        crcs = []
        with g.BuildIndex(frames, keys) as idx:
            dst, win = ic.dev_buf(w * h, 0), ic.dev_buf(ww * wh)
            for t in picks:
                dst.zero_()
                assert idx.Show(t, dst, adopt=False).data_pnt is dst
                if filter == 2:
                    display_present_area(dst, w, h, win, ww, wh, k, dx, dy)
                else:
                    display_present(dst, w, h, win, ww, wh, k, dx, dy, filter=filter)
                crcs.append("%08x" % (zlib.crc32(win.cpu().numpy().tobytes()) & 0xFFFFFFFF))
        g.StopAndClean()
        assert [l[1] for l in lines] == crcs, spec
    # the option goes alone and checks its arguments
    for extra in (["--index-present", "90x50", "0"], ["--index-present", "90x50", "4:3"], ["--index-present", "0x50", "4"],
                  ["--index-present", "90x50", "4", "--step-back"]):
        assert subprocess.run([exe, str(path)] + extra, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120).returncode == 2
