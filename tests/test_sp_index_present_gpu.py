"""Frames of a ScreenPressor seek index straight into a window (jsp_sp_index_present, SpScrubIndex.Present, jsp_play
--index-present) on an MI355X.

Truth: tests/index_present_ref.py (the contract in numpy, over view_ref / view_area_ref) applied to the oracle's pictures of
tests/sp_index_ref.oracle_run, which are also the encoder's.  The cross-check on the device is Show followed by display_present /
display_present_area.  Everything is bit-exact.

Sizes (the kernel's constants are in tests/index_present_cases.py): 150 x 106 is no multiple of 16 or 4 and larger than one 64 x 64
source tile in both axes (148 wide: the 16-byte key-picture loads); 41 frames with a key frame every 13 give several key pictures and
walks across a bitmap word (frames 32 .. 38 behind key frame 27); every window but the tiny ones is larger than one output rectangle in both axes."""
import ctypes as C
import os
import subprocess
import zlib

import numpy as np
import pytest

import index_present_cases as ic
import index_present_ref as ipr
import sp_index_ref as ref
import view_ref as vr
from jsplayer_amd import CodecError, MSVideo1_16bit, ScreenPressor
from jsplayer_amd import _native as N
from jsplayer_amd import streamgen as sg
from jsplayer_amd.codec import display_present, display_present_area

pytestmark = pytest.mark.gpu

FN = "sp_index_present"
POISON = ic.POISON
H = 106
# (config, width, frames, bpp, version): one clip per entropy version the index tests cover, 16 bpp twice
CLIPS = [(71, 150, 41, 24, 4), (72, 150, 41, 16, 3), (73, 150, 41, 24, 2), (74, 148, 45, 16, 4)]
PICKS = [40, 0, 35, 27, 13, 12, 31, 32, 13]    # unordered, one twice; key frames, the frame before one; 35 and 32 lie in bitmap word 1
CROSS = (2, 7)                                 # ... behind the key frame 27 of word 0: positions in PICKS whose walk steps down a word


def make_sp(clip, lines=36):
    c = ScreenPressor(clip.w, clip.h, clip.bpp)
    c.Preinit(lines)
    return c


def picture(buf):
    return buf.cpu().numpy().view(np.uint32)


_CLIPS = {}


def get_clip(case):
    if case not in _CLIPS:
        cfg, w, n, bpp, version = case
        clip = ref.make_clip(cfg, w, H, n, bpp, version, 13, 7)
        pictures, _ = ref.oracle_run(clip)
        for t in range(n):
            assert np.array_equal(pictures[t], clip.frames[t])
        for i in CROSS:                                                   # the walk of index_compose goes from word t / 32 down to (k + 1) / 32
            t = PICKS[i]
            k = max(j for j in range(t + 1) if clip.keys[j])
            assert (t >> 5) > ((k + 1) >> 5), f"frame {t} (key {k}) does not cross a bitmap word"
        _CLIPS[case] = (clip, pictures)
    return _CLIPS[case]


@pytest.mark.parametrize("case", CLIPS, ids=lambda c: "cfg%d_w%d_n%d_%dbpp_v%d" % c)
def test_the_windows_match_the_oracle_and_show_plus_present(case):
    clip, pictures = get_clip(case)
    w = clip.w
    gpu = make_sp(clip)
    idx = gpu.BuildScrubIndex(clip.chunks, clip.keys, key_row=7)
    mode = vr.CANVAS_RGB15 if clip.bpp == 16 else vr.CANVAS
    scratch = ic.dev_buf(w * H)
    for name, ww, wh, k, dx, dy, filters in ic.windows(w, H):
        sheets = {}
        for f in filters:
            sheets[f] = ic.check(FN, gpu, idx, pictures, PICKS, w, H, ww, wh, k, dx, dy, mode, f, cols=3, what=f"{clip.name} {name}")
        if name == "crop100":                                             # the three filters agree on a plain crop
            assert np.array_equal(sheets[0], sheets[1]) and np.array_equal(sheets[0], sheets[2])
        if name == "quirk200":                                            # background at the left of every cell
            assert np.all(sheets[1][:3 * ww].reshape(3, ww)[:, :33] == ic.BG) and sheets[1][33] != ic.BG
        for i in (0,) + CROSS:                                            # the cross-check on the device: Show, then the present call of the filter
            idx.Show(PICKS[i], scratch)
            for f in filters:
                win = ic.dev_buf(ww * wh)
                if f == ipr.AREA:
                    display_present_area(scratch, w, H, win, ww, wh, k, dx, dy, mode=mode, background=ic.BG)
                else:
                    display_present(scratch, w, H, win, ww, wh, k, dx, dy, mode=mode, filter=f, background=ic.BG)
                cell = ic.cell_of(sheets[f], i, 3, ww, wh)
                assert np.array_equal(picture(win).reshape(wh, ww), cell), f"{clip.name} {name} frame {PICKS[i]} filter {f}: not Show + present"
    assert gpu.PreviousFrame() is None
    idx.close()
    gpu.StopAndClean()


@pytest.mark.parametrize("case", [CLIPS[0], CLIPS[3]], ids=["150wide", "148wide"])
def test_modes_pitch_padding_alignment_and_the_cells_past_n(case):
    clip, pictures = get_clip(case)
    w = clip.w
    gpu = make_sp(clip)
    idx = gpu.BuildScrubIndex(clip.chunks, clip.keys, key_row=7)
    k, dx, dy = vr.view_matrix(w, H, 101, 73, 0, 0.5, 0.5)
    picks5 = PICKS[:5]                                                    # (35: a walk across a bitmap word)
    assert PICKS[CROSS[0]] in picks5
    for mode in ic.MODES:
        for f in ipr.FILTERS:
            ic.check(FN, gpu, idx, pictures, picks5, w, H, 101, 73, k, dx, dy, mode, f, cols=2, pad=7, what=clip.name)      # width no multiple of 4
    for f in ipr.FILTERS:
        ic.check(FN, gpu, idx, pictures, picks5, w, H, 100, 37, k, dx, dy, vr.CANVAS, f, cols=2, pad=4, what=clip.name)           # 16-byte stores throughout
        ic.check(FN, gpu, idx, pictures, picks5, w, H, 100, 37, k, dx, dy, vr.CANVAS, f, cols=2, pad=4, offset=1, what=clip.name) # `out` one int off
        ic.check(FN, gpu, idx, pictures, [20], w, H, 100, 73, k, dx, dy, vr.CANVAS, f, what=clip.name)                            # n = 1, cols = 1: the plain window
    # Present: `mode` defaults to the conversion that gives canvas pixels — RGB15 for 16 bpp
    mode = vr.CANVAS_RGB15 if clip.bpp == 16 else vr.CANVAS
    got = idx.Present(picks5, 50, 36, 0.37, 1.5, 2.5, filter=ipr.AREA, cols=2)
    want = ipr.sheet([pictures[t] for t in picks5], w, H, 50, 36, 0.37, 1.5, 2.5, mode=mode, filter=ipr.AREA, cols=2, fill=0)
    assert tuple(got.shape) == (3 * 36, 100) and np.array_equal(picture(got).reshape(-1), want)
    out = ic.dev_buf(3 * 36 * 100 + 5)
    got = idx.Present(picks5, 50, 36, 0.37, 1.5, 2.5, mode=vr.SETPIXELS, filter=ipr.NEAREST, background=0x01020304, cols=2, out=out)
    want = ipr.sheet([pictures[t] for t in picks5], w, H, 50, 36, 0.37, 1.5, 2.5, mode=vr.SETPIXELS, filter=ipr.NEAREST, background=0x01020304, cols=2,
                     fill=POISON, total=3 * 36 * 100 + 5)
    assert got.data_ptr() == out.data_ptr() and np.array_equal(picture(out), want)
    idx.close()
    gpu.StopAndClean()


def sequential(gpu, chunks, keys, lo, hi, pool):
    out = []
    for i in range(lo, hi):
        prev = gpu.PreviousFrame()
        dst = next(b for b in pool if b is not prev)
        if keys[i]:
            assert gpu.DecompressI(chunks[i], dst) == 0
            out.append((picture(gpu.PreviousFrame()).copy(), None, next(k for k, b in enumerate(pool) if b is gpu.PreviousFrame())))
        else:
            r = gpu.DecompressP(chunks[i], dst)
            out.append((picture(r.data_pnt).copy(), r.significant_changes, next(k for k, b in enumerate(pool) if b is r.data_pnt)))
    return out


def info(idx):
    n, dev, host = C.c_int(0), C.c_uint64(0), C.c_uint64(0)
    assert idx._lib.jsp_sp_index_info(idx._h, C.byref(n), C.byref(dev), C.byref(host)) == 0
    return dev.value, host.value


def test_the_codec_is_only_lent():
    """A codec half-way through ANOTHER clip builds an index and calls Present between its decodes: no frame buffer is written, and
    every later picture, verdict and data_pnt equals a twin's that never saw an index — nothing the codec remembered of its buffers
    (their last columns) was forgotten or spoilt.  The index grows by the per-cell records, not by a picture."""
    w, h = 100, 52
    own = ref.make_clip(81, w, h, 30, 24, 4, 9, 7)
    other = ref.make_clip(82, w, h, 41, 24, 4, 13, 7)
    gpu, twin = make_sp(own), make_sp(own)
    pool, tpool = [ic.dev_buf(w * h) for _ in range(3)], [ic.dev_buf(w * h) for _ in range(3)]
    a = sequential(gpu, own.chunks, own.keys, 0, 14, pool)
    b = sequential(twin, own.chunks, own.keys, 0, 14, tpool)
    idx = gpu.BuildScrubIndex(other.chunks, other.keys, key_row=7)
    dev0, _ = info(idx)
    k, dx, dy = vr.view_matrix(w, h, 64, 30, 0, 0.5, 0.5)
    for lo, hi in ((14, 15), (15, 22), (22, 30)):
        prev = gpu.PreviousFrame()
        pool_pics = [picture(p).copy() for p in pool]
        for f in ipr.FILTERS:
            idx.Present([40, 17, 3, 25, 0, 13], 64, 30, k, dx, dy, filter=f, cols=4)
        idx.Present(list(range(idx.frames)) * 2, 9, 5, 0.05, 0.0, 0.0, filter=ipr.AREA, cols=16)
        assert gpu.PreviousFrame() is prev
        for p, pic in zip(pool, pool_pics):
            assert np.array_equal(picture(p), pic), "Present wrote a frame buffer"
        a += sequential(gpu, own.chunks, own.keys, lo, hi, pool)
        b += sequential(twin, own.chunks, own.keys, lo, hi, tpool)
    dev1, _ = info(idx)
    assert 24 * 82 <= dev1 - dev0 < w * h * 4
    for i, (x, y) in enumerate(zip(a, b)):
        assert np.array_equal(x[0], y[0]) and x[1] == y[1] and x[2] == y[2], f"frame {i} after Present differs from the twin's"
        assert np.array_equal(x[0], own.frames[i]), f"frame {i}: not the encoder's picture"
    idx.close()
    gpu.StopAndClean()
    twin.StopAndClean()


def test_every_refusal_leaves_out_untouched_and_names_the_call():
    w, h = 64, 48
    clip = ref.make_clip(85, w, h, 41, 24, 4, 13, 36)
    pictures, _ = ref.oracle_run(clip)
    gpu = make_sp(clip)
    pool = [ic.dev_buf(w * h) for _ in range(3)]
    sequential(gpu, clip.chunks, clip.keys, 0, 5, pool)
    idx = gpu.BuildScrubIndex(clip.chunks, clip.keys)
    ww, wh = 20, 10
    out = ic.dev_buf(4 * ww * wh)
    good = dict(frames=[0], out=out, win_w=ww, win_h=wh, pitch=ww, cols=1, k=0.5, dx=0.0, dy=0.0, mode=vr.CANVAS, filter=ipr.BILINEAR)

    def refused(match, codec=None, prefix="sp_index_present:", **kw):
        args = dict(good, **kw)
        with pytest.raises(CodecError, match=match) as e:
            ic.call(FN, codec or gpu, idx, **args)
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
    for bad in (-1, idx.frames, 1 << 20):
        refused("outside the index", frames=[0, bad])
    refused("out_pitch", pitch=ww - 1)
    refused("out_pitch", frames=[0, 1], cols=2, pitch=2 * ww - 1)
    refused("smaller than the sheet", frames=[0, 1, 2, 3, 4])                              # five cells, room for four
    refused("smaller than the sheet", frames=[0, 1, 2], cols=2, pitch=2 * ww, out_ints=4 * ww * wh - 1)   # two sheet rows of two cells
    refused("smaller than the sheet", pitch=ww + 1, out_ints=(wh - 1) * (ww + 1) + ww - 1)
    host = np.full(4 * ww * wh, POISON, dtype=np.uint32).view(np.int32)
    refused("device buffer", out=host)
    assert np.all(host.view(np.uint32) == POISON)
    prev = gpu.PreviousFrame()
    ticket = gpu.DecompressP_async(clip.chunks[5], next(b for b in pool if b is not prev))
    refused("in flight")
    gpu.wait(ticket)
    # null arguments (the C ABI itself)
    lib = N.lib()
    one = (C.c_int * 1)(0)
    tail = (out.numel(), ww, wh, ww, 1, 0.5, 0.0, 0.0, 0, 1, 0)
    for args in ((None, idx._h, 1, one, C.c_void_p(out.data_ptr())), (gpu._h, None, 1, one, C.c_void_p(out.data_ptr())),
                 (gpu._h, idx._h, 1, None, C.c_void_p(out.data_ptr())), (gpu._h, idx._h, 1, one, None)):
        assert lib.jsp_sp_index_present(*args, *tail) != 0 and N.last_error().startswith("sp_index_present: null argument")
    # an index of another codec; an MSVideo1 codec
    other = make_sp(clip)
    refused("another codec", codec=other)
    msv = MSVideo1_16bit(w, h)
    refused("ScreenPressor only", codec=msv, prefix="sp_index: ScreenPressor only")
    msv.StopAndClean()
    other.StopAndClean()
    assert bool((out == POISON).all())
    # and the call still works, the codec's stream goes on; a closed index / codec raise as Thumbs does
    ic.check(FN, gpu, idx, pictures, [1, 0], w, h, ww, wh, 0.5, 0.0, 0.0, vr.CANVAS, ipr.BILINEAR, cols=2)
    after = sequential(gpu, clip.chunks, clip.keys, 6, 12, pool)
    for i, got in enumerate(after, start=6):
        assert np.array_equal(got[0], pictures[i]), f"frame {i} after the refusals"
    idx.close()
    with pytest.raises(CodecError, match="index is closed"):
        idx.Present([0], ww, wh, 0.5, 0, 0)
    idx2 = gpu.BuildScrubIndex(clip.chunks, clip.keys)
    gpu.StopAndClean()
    with pytest.raises(CodecError, match="codec is closed"):
        idx2.Present([0], ww, wh, 0.5, 0, 0)
    idx2.close()


def test_jsp_play_index_present_on_a_screenpressor_avi(tmp_path):
    from jsplayer_amd import avi
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "examples", "jsp_play")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-s", "-C", os.path.join(root, "examples")])
    w, h, n = 320, 240, 40
    chunks, keys, frames = sg.sp_clip(97, w, h, n, bpp=16, version=4, key_every=12, unchanged_at=(5,))
    assert [i for i, key in enumerate(keys) if key] == [0, 12, 24, 36]         # frame 35 of the picks walks from bitmap word 1 down to word 0
    path = tmp_path / "clip.avi"
    path.write_bytes(avi.write_avi(w, h, chunks, fourcc=b"SCPR", bpp=16, fps=15.0, key_flags=keys))
    picks = [(i * n) // 9 for i in range(9)]
    gpu = ScreenPressor(w, h, 16)
    gpu.Preinit(36)
    idx = gpu.BuildScrubIndex(chunks, keys)
    dst = ic.dev_buf(w * h)
    for spec, zoom, hpos, vpos, filter in (("90x50", 0, 0.5, 0.5, 1), ("160x90:2:0.3:0.8", 2, 0.3, 0.8, 0), ("90x50", 0, 0.5, 0.5, 2)):
        ww, wh = (int(v) for v in spec.split(":")[0].split("x"))
        res = subprocess.run([exe, str(path), "--index-present", spec, "9" if filter == 1 else f"9:{filter}"], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                             timeout=120)
        assert res.returncode == 0, res.stderr.decode()
        lines = [l.split() for l in res.stdout.decode().splitlines() if l and l[0].isdigit()]
        assert [int(l[0]) for l in lines] == picks
        k, dx, dy = vr.view_matrix(w, h, ww, wh, zoom, hpos, vpos)
        win, crcs = ic.dev_buf(ww * wh), []
        for t in picks:                                                   # 16 bpp: the RGB15 conversion, as for a frame
            idx.Show(t, dst)
            if filter == 2:
                display_present_area(dst, w, h, win, ww, wh, k, dx, dy, mode=vr.CANVAS_RGB15)
            else:
                display_present(dst, w, h, win, ww, wh, k, dx, dy, mode=vr.CANVAS_RGB15, filter=filter)
            crcs.append("%08x" % (zlib.crc32(win.cpu().numpy().tobytes()) & 0xFFFFFFFF))
        assert [l[1] for l in lines] == crcs, spec
    idx.close()
    gpu.StopAndClean()
