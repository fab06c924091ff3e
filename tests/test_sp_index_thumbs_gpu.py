"""Thumbnails of a ScreenPressor seek index (jsp_sp_index_thumb_size / jsp_sp_index_thumbs, SpScrubIndex.ThumbSize / Thumbs,
Manager.preview / filmstrip, jsp_play --filmstrip) on an MI355X.

Truth: tests/thumbs_ref.py (the box mean and the sheet layout of include/jsplayer_amd.h) applied to the oracle's pictures of
tests/sp_index_ref.oracle_run, which are also the encoder's.  Everything is bit-exact."""
import ctypes as C
import os
import subprocess
import zlib

import numpy as np
import pytest

import sp_index_ref as ref
import thumbs_ref as tr
from jsplayer_amd import CodecError, MSVideo1_16bit, ScreenPressor, _native as N, player
from jsplayer_amd import streamgen as sg

pytestmark = pytest.mark.gpu

POISON = 0x5A5A5A5A


def dev_buf(n, fill=POISON):
    import torch
    return torch.full((n,), fill, dtype=torch.int32, device="cuda")


def make_sp(clip_or_w, h=None, bpp=None, lines=36):
    if h is None:
        clip_or_w, h, bpp = clip_or_w.w, clip_or_w.h, clip_or_w.bpp
    c = ScreenPressor(clip_or_w, h, bpp)
    c.Preinit(lines)
    return c


def picture(buf):
    return buf.cpu().numpy().view(np.uint32)


def want_sheet(pictures, picks, w, h, s, cols, fill=POISON):
    return tr.sheet([tr.thumbnail(pictures[t], w, h, s) for t in picks], cols, fill=fill)


def check(idx, pictures, picks, w, h, s, cols, what):
    """One Thumbs call into a poisoned `out` one cell longer than the sheet: the sheet is the reference's, the cells of the last
    row past n and the ints behind the sheet keep the poison."""
    tw, th = idx.ThumbSize(s)
    assert (tw, th) == tr.thumb_size(w, h, s) == (w // s, h // s), what
    rows = -(-len(picks) // cols)
    out = dev_buf(rows * th * cols * tw + tw * th)
    got = idx.Thumbs(picks, scale=s, cols=cols, out=out)
    assert tuple(got.shape) == (rows * th, cols * tw) and got.data_ptr() == out.data_ptr(), what
    want = want_sheet(pictures, picks, w, h, s, cols)
    bad = np.argwhere(got.cpu().numpy() != want)
    assert len(bad) == 0, f"{what}: {len(bad)} sheet pixels differ, first at {tuple(bad[0])}"
    assert np.all(picture(out)[rows * th * cols * tw:] == POISON), what + ": written behind the sheet"


# (config, width, height, frames, bpp, version, key_every, key_row): the clips of test_sp_index_gpu.CLIPS — flat key frames, a key
# frame behind a key frame, unchanged frames and frames that move half their blocks are in every one (sp_index_ref.make_clip)
CLIPS = [
    (51, 64, 48, 41, 24, 4, 13, 36),
    (52, 100, 52, 41, 24, 3, 13, 7),        # neither dimension a multiple of 16
    (53, 37, 23, 41, 24, 2, 13, 5),         # X % 4 != 0: the scalar path; 2 x 1 thumbnails at scale 16
    (54, 320, 240, 41, 24, 4, 13, 36),
    (55, 320, 240, 41, 16, 2, 13, 36),
    (56, 64, 48, 41, 16, 3, 13, 36),
    (57, 100, 52, 41, 16, 4, 13, 7),
    (58, 320, 240, 90, 24, 4, 0, 36),       # one key frame, 89 frames behind it: three bitmap words
    (59, 100, 52, 75, 16, 3, 0, 7),
]


def clip_id(c):
    return "cfg%d_%dx%d_n%d_%dbpp_v%d_k%d" % c[:7]


@pytest.mark.parametrize("case", CLIPS, ids=clip_id)
def test_every_frame_every_scale_shuffled_with_repeats(case):
    cfg, w, h, n, bpp, version, key_every, key_row = case
    clip = ref.make_clip(cfg, w, h, n, bpp, version, key_every, key_row)
    pictures, _ = ref.oracle_run(clip)
    for t in range(n):
        assert np.array_equal(pictures[t], clip.frames[t])
    gpu = make_sp(clip)
    idx = gpu.BuildScrubIndex(clip.chunks, clip.keys, key_row=key_row)
    rng = np.random.default_rng(cfg)
    picks = [int(t) for t in rng.permutation(n)] + [int(t) for t in rng.integers(0, n, 7)]   # every frame, seven of them twice
    for s in tr.SCALES:
        for cols in (1, 3, len(picks)):
            check(idx, pictures, picks, w, h, s, cols, f"{clip.name} s={s} cols={cols}")
        # a byte's mean never exceeds the bytes it is the mean of; 16 bpp without a flat key frame (which the reference fills with
        # components already shifted left by 3, ScreenPressor.hx:134-139): one 5-bit component per byte, and so is its mean
        top = int(idx.Thumbs(picks, scale=s).cpu().numpy().view(np.uint8).max())
        assert top <= max(int(p.view(np.uint8).max()) for p in pictures)
        if bpp == 16 and key_every == 0:
            assert top <= 31
    assert gpu.PreviousFrame() is None
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


def test_equals_the_formula_on_show_and_leaves_no_trace():
    """A codec half-way through ANOTHER clip builds an index and calls Thumbs between its decodes: each thumbnail is the formula
    applied to the picture Show(t) wrote, and every later picture, verdict and data_pnt equals a twin's that never saw an index."""
    w, h = 100, 52
    own = ref.make_clip(61, w, h, 30, 24, 4, 9, 7)
    other = ref.make_clip(62, w, h, 41, 24, 4, 13, 7)
    gpu, twin = make_sp(own), make_sp(own)
    pool, tpool = [dev_buf(w * h) for _ in range(3)], [dev_buf(w * h) for _ in range(3)]
    a = sequential(gpu, own.chunks, own.keys, 0, 14, pool)
    b = sequential(twin, own.chunks, own.keys, 0, 14, tpool)
    idx = gpu.BuildScrubIndex(other.chunks, other.keys, key_row=7)
    shown = dev_buf(w * h)
    for lo, hi in ((14, 15), (15, 22), (22, 30)):
        prev = gpu.PreviousFrame()
        prev_pic = picture(prev).copy()
        pool_pics = [picture(p).copy() for p in pool]
        for t in (40, 17, 3, 25, 0, 13):
            shown.fill_(POISON)
            idx.Show(t, shown)
            for s in tr.SCALES:
                got = idx.Thumbs([t], scale=s).cpu().numpy()
                assert np.array_equal(got, tr.thumbnail(picture(shown), w, h, s)), f"t={t} s={s}"
        idx.Thumbs(list(range(idx.frames)), scale=8, cols=5)
        assert gpu.PreviousFrame() is prev and np.array_equal(picture(prev), prev_pic)
        for p, pic in zip(pool, pool_pics):
            assert np.array_equal(picture(p), pic), "Thumbs wrote a frame buffer"
        a += sequential(gpu, own.chunks, own.keys, lo, hi, pool)
        b += sequential(twin, own.chunks, own.keys, lo, hi, tpool)
    for i, (x, y) in enumerate(zip(a, b)):
        assert np.array_equal(x[0], y[0]) and x[1] == y[1] and x[2] == y[2], f"frame {i} after Thumbs differs from the twin's"
        assert np.array_equal(x[0], own.frames[i]), f"frame {i}: not the encoder's picture"
    idx.close()
    gpu.StopAndClean()
    twin.StopAndClean()


def test_the_record_array_is_counted_and_absent_until_asked_for():
    clip = ref.make_clip(64, 100, 52, 41, 24, 4, 13, 7)
    gpu = make_sp(clip)
    idx = gpu.BuildScrubIndex(clip.chunks, clip.keys, key_row=7)

    def info():
        n, dev, host = C.c_int(0), C.c_uint64(0), C.c_uint64(0)
        assert idx._lib.jsp_sp_index_info(idx._h, C.byref(n), C.byref(dev), C.byref(host)) == 0
        return dev.value, host.value

    dev0, host0 = info()
    assert (dev0, host0) == (idx.device_bytes, idx.host_bytes)
    dst = dev_buf(clip.w * clip.h)
    idx.Show(7, dst)
    assert info() == (dev0, host0)                         # Show holds nothing more
    idx.Thumbs([3], scale=4)
    dev1, host1 = info()
    assert 24 <= dev1 - dev0 <= 4096 and 24 <= host1 - host0 <= 4096
    idx.Thumbs([3, 4], scale=16)
    assert info() == (dev1, host1)                         # (room for two was there)
    idx.Thumbs([t % 41 for t in range(4096)], scale=16, cols=64)
    dev2, host2 = info()
    assert 4096 * 24 <= dev2 - dev0 <= 2 * 4096 * 24 and 4096 * 24 <= host2 - host0 <= 2 * 4096 * 24
    idx.close()
    gpu.StopAndClean()


class _Rebound:
    """SpScrubIndex.Thumbs of `index` called through ANOTHER codec (what the C ABI allows a caller to get wrong)."""

    def __init__(self, index, codec):
        self.index, self.codec = index, codec

    def Thumbs(self, frames, scale, out):
        arr = (C.c_int * len(frames))(*frames)
        if self.index._lib.jsp_sp_index_thumbs(self.codec._h, self.index._h, len(frames), arr, scale, 1, C.c_void_p(out.data_ptr()), out.numel()) != 0:
            raise CodecError(N.last_error())


def test_every_refusal_leaves_out_untouched_and_names_the_call():
    import torch
    w, h = 64, 48
    clip = ref.make_clip(65, w, h, 41, 24, 4, 13, 36)
    pictures, _ = ref.oracle_run(clip)
    gpu = make_sp(clip)
    pool = [dev_buf(w * h) for _ in range(3)]
    sequential(gpu, clip.chunks, clip.keys, 0, 5, pool)
    idx = gpu.BuildScrubIndex(clip.chunks, clip.keys)
    tw, th = idx.ThumbSize(8)
    assert (tw, th) == (8, 6)
    out = dev_buf(4 * tw * th)

    def refused(match, *args, **kw):
        with pytest.raises(CodecError, match=match) as e:
            idx.Thumbs(*args, **kw)
        assert "sp_index_thumbs:" in str(e.value), str(e.value)
        assert bool((out == POISON).all()), match + ": out was written"

    refused("1..4096", [], scale=8, out=out)
    refused("1..4096", [0] * 4097, scale=8, out=out)
    for bad in (-1, idx.frames, 1 << 20):
        refused("outside the index", [0, bad], scale=8, out=out)
    for bad in (0, 1, 2, 5, 12, 32, -8):
        refused("scale must be 4, 8 or 16", [0], scale=bad, out=out)
    refused("cols", [0, 1], scale=8, cols=0, out=out)
    refused("cols", [0, 1], scale=8, cols=-3, out=out)
    refused("smaller than the sheet", [0, 1, 2, 3, 4], scale=8, out=out)                        # five thumbnails, room for four
    refused("smaller than the sheet", [0, 1, 2], scale=8, cols=2, out=out[: 4 * tw * th - 1])   # two sheet rows of two cells
    host = np.full(4 * tw * th, POISON, dtype=np.uint32).view(np.int32)
    refused("device buffer", [0], scale=8, out=host)
    assert np.all(host.view(np.uint32) == POISON)
    prev = gpu.PreviousFrame()
    ticket = gpu.DecompressP_async(clip.chunks[5], next(b for b in pool if b is not prev))
    refused("in flight", [0], scale=8, out=out)
    gpu.wait(ticket)
    # null arguments (the C ABI itself)
    lib = N.lib()
    one = (C.c_int * 1)(0)
    for args in ((None, idx._h, 1, one, 8, 1, C.c_void_p(out.data_ptr()), out.numel()),
                 (gpu._h, None, 1, one, 8, 1, C.c_void_p(out.data_ptr()), out.numel()),
                 (gpu._h, idx._h, 1, None, 8, 1, C.c_void_p(out.data_ptr()), out.numel()),
                 (gpu._h, idx._h, 1, one, 8, 1, None, out.numel())):
        assert lib.jsp_sp_index_thumbs(*args) != 0 and "sp_index_thumbs: null argument" in N.last_error()
    wv, hv = C.c_int(-1), C.c_int(-1)
    assert lib.jsp_sp_index_thumb_size(None, 8, C.byref(wv), C.byref(hv)) != 0 and "sp_index_thumb_size: null argument" in N.last_error()
    assert lib.jsp_sp_index_thumb_size(idx._h, 8, None, C.byref(hv)) != 0 and "sp_index_thumb_size: null argument" in N.last_error()
    assert lib.jsp_sp_index_thumb_size(idx._h, 8, C.byref(wv), None) != 0
    assert lib.jsp_sp_index_thumb_size(idx._h, 3, C.byref(wv), C.byref(hv)) != 0 and (wv.value, hv.value) == (-1, -1)
    assert "sp_index_thumb_size: scale" in N.last_error()
    with pytest.raises(CodecError, match="sp_index_thumb_size: scale"):
        idx.ThumbSize(7)
    # an index of another codec; an MSVideo1 codec
    other = make_sp(clip)
    with pytest.raises(CodecError, match="sp_index_thumbs: the index was built by another codec"):
        _Rebound(idx, other).Thumbs([0], 8, out)
    msv = MSVideo1_16bit(w, h)
    with pytest.raises(CodecError, match="sp_index: ScreenPressor only"):
        _Rebound(idx, msv).Thumbs([0], 8, out)
    msv.StopAndClean()
    other.StopAndClean()
    # a picture too small for one thumbnail pixel at this scale
    tiny_clip = ref.make_clip(68, 12, 4, 9, 24, 4, 4, 1)
    t = make_sp(tiny_clip)
    tiny = t.BuildScrubIndex(tiny_clip.chunks, tiny_clip.keys, key_row=1)
    assert tiny.ThumbSize(4) == (3, 1)
    tiny_pictures, _ = ref.oracle_run(tiny_clip)
    for f in range(9):
        assert np.array_equal(tiny.Thumbs([f], scale=4).cpu().numpy(), tr.thumbnail(tiny_pictures[f], 12, 4, 4))
    for s in (8, 16):
        with pytest.raises(CodecError, match="too small") as e:
            tiny.Thumbs([0], scale=s, out=out)
        assert "sp_index_thumbs:" in str(e.value)
        with pytest.raises(CodecError, match="sp_index_thumb_size: the picture is too small"):
            tiny.ThumbSize(s)
    tiny.close()
    t.StopAndClean()
    assert np.all(picture(out) == POISON)
    # and the call still works, the codec's stream goes on; a closed index / codec raise as Show does
    got = idx.Thumbs([1, 0], scale=8, cols=2, out=out)
    assert tuple(got.shape) == (th, 2 * tw) and got.data_ptr() == out.data_ptr()
    assert np.array_equal(got.cpu().numpy(), want_sheet(pictures, [1, 0], w, h, 8, 2))
    after = sequential(gpu, clip.chunks, clip.keys, 6, 12, pool)
    for i, got in enumerate(after, start=6):
        assert np.array_equal(got[0], pictures[i]), f"frame {i} after the refusals"
    idx.close()
    with pytest.raises(CodecError, match="index is closed"):
        idx.Thumbs([0])
    with pytest.raises(CodecError, match="index is closed"):
        idx.ThumbSize(8)
    idx2 = gpu.BuildScrubIndex(clip.chunks, clip.keys)
    gpu.StopAndClean()
    with pytest.raises(CodecError, match="codec is closed"):
        idx2.Thumbs([0])
    idx2.close()        # after the codec is gone
    idx2.close()
    torch.cuda.synchronize()


def test_full_size_pclip300_sixteen_frames_every_scale():
    from jsplayer_amd import workloads as wl
    name = "screenpressor_v4_1080p_pclip300"
    c = wl.build_clips(name)[0]
    golden = wl.golden_digests(name, 0)
    if golden is None:
        pytest.fail("tests/golden/bench_digests.json has no digests for " + name)
    want = list(golden[0])
    assert len(want) == len(c.frames) == 300
    for t in range(1, 300):          # "-": the oracle adopted nothing (an unchanged frame) — the picture before it stays
        if want[t] == "-":
            want[t] = want[t - 1]
    codec = wl.make_codec(name)
    idx = codec.BuildScrubIndex(c.frames, c.keys)
    picks = [(k * 300) // 16 for k in range(16)]
    dst = dev_buf(wl.W * wl.H)
    pics = {}
    for t in picks:
        dst.fill_(POISON)
        idx.Show(t, dst)
        pics[t] = dst.cpu().numpy().copy()
        assert wl.digest(pics[t]) == want[t], f"Show({t}): not the golden picture"
    order = picks[::-1]
    for s in tr.SCALES:
        tw, th = idx.ThumbSize(s)
        assert (tw, th) == (wl.W // s, wl.H // s)
        got = idx.Thumbs(order, scale=s, cols=4).cpu().numpy()
        wanted = tr.sheet([tr.thumbnail(pics[t], wl.W, wl.H, s) for t in order], 4)
        assert got.shape == (4 * th, 4 * tw)
        bad = np.argwhere(got != wanted)
        assert len(bad) == 0, f"scale {s}: {len(bad)} pixels differ, first at {tuple(bad[0])}"
    idx.close()
    codec.StopAndClean()


class _Spy:
    """A decoder that forwards everything and logs the decoding calls."""

    def __init__(self, d):
        self.d, self.calls = d, []

    def __getattr__(self, k):
        v = getattr(self.d, k)
        if k in ("DecompressI", "DecompressP"):
            def logged(*a, **kw):
                self.calls.append(k)
                return v(*a, **kw)
            return logged
        return v


def test_manager_preview_and_filmstrip_are_pure_reads():
    from jsplayer_amd.avi import CODEC_SCREENPRESSOR, VideoInfo
    w, h = 100, 52
    chunks, keys, frames = sg.sp_clip(67, w, h, 41, bpp=24, version=4, key_every=13, unchanged_at=(3, 4, 30),
                                      p_mix_at={6: dict(unchanged=0.3, motion=0.6), 20: dict(unchanged=0.35, motion=0.45)})
    clip = ref.Clip("manager", w, h, 24, 4, player.INSIGNIFICANT_LINES, chunks, keys, [f.astype(np.uint32) for f in frames])
    pictures, _ = ref.oracle_run(clip, preinit=player.INSIGNIFICANT_LINES)
    first, n = 13, 41                                     # the index covers clip frames 13 .. 40 (13 is a coded key frame)
    vi = VideoInfo(X=w, Y=h, bpp=24, fps=15.0, nframes=n, codec=CODEC_SCREENPRESSOR, palette=None, riff_size=0)
    dec = make_sp(clip)
    spy = _Spy(dec)
    mgr = player.Manager(vi, spy, lambda k: dev_buf(k))
    mgr.play(clip.chunks[:5], key_flags=clip.keys[:5])    # the decoder stands behind frame 4
    idx = dec.BuildScrubIndex(clip.chunks[first:], clip.keys[first:], key_row=player.INSIGNIFICANT_LINES)
    mgr.attach_index(idx, first)
    spy.calls.clear()
    state = (mgr.next_frame_to_decode, list(mgr.holds), len(mgr.log), dec.PreviousFrame())
    held = [picture(b).copy() for b in mgr.buffers]
    for s in tr.SCALES:
        for i in (first, 20, n - 1):
            got = mgr.preview(i, scale=s).cpu().numpy()
            assert np.array_equal(got, tr.thumbnail(pictures[i], w, h, s)), f"preview({i}) s={s}"
        for count, cols in ((5, None), (7, 3), (28, 28)):
            numbers, sheet = mgr.filmstrip(count, scale=s, cols=cols)
            picks = [first + (k * idx.frames) // count for k in range(count)]
            assert numbers == picks
            assert np.array_equal(sheet.cpu().numpy(), want_sheet(pictures, picks, w, h, s, count if cols is None else cols, fill=0))
    with pytest.raises(ValueError):
        mgr.preview(first - 1)
    assert spy.calls == [], spy.calls
    assert (mgr.next_frame_to_decode, list(mgr.holds), len(mgr.log), dec.PreviousFrame()) == state
    for b, pic in zip(mgr.buffers, held):
        assert np.array_equal(picture(b), pic)
    # ... and play goes on from where the decoder stands
    d = mgr.seek(clip.chunks, 9, clip.keys)
    assert np.array_equal(picture(mgr.buffers[d.buffer_index]), pictures[9])
    idx.close()
    dec.StopAndClean()


def test_jsp_play_filmstrip_on_a_screenpressor_avi(tmp_path):
    from jsplayer_amd import avi
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "examples", "jsp_play")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-s", "-C", os.path.join(root, "examples")])
    w, h, n = 320, 240, 40
    chunks, keys, frames = sg.sp_clip(97, w, h, n, bpp=24, version=4, key_every=16, unchanged_at=(5,))
    path = tmp_path / "clip.avi"
    path.write_bytes(avi.write_avi(w, h, chunks, fourcc=b"SCPR", bpp=24, fps=15.0, key_flags=keys))
    for arg, count, s in (("9:8", 9, 8), ("5:16", 5, 16), ("40:4", 40, 4)):
        res = subprocess.run([exe, str(path), "--filmstrip", arg], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
        assert res.returncode == 0, res.stderr.decode()
        lines = [l.split() for l in res.stdout.decode().splitlines() if l and l[0].isdigit()]
        picks = [(k * n) // count for k in range(count)]
        assert [int(l[0]) for l in lines] == picks
        want = ["%08x" % (zlib.crc32(tr.thumbnail(frames[t].astype(np.uint32), w, h, s).tobytes()) & 0xFFFFFFFF) for t in picks]
        assert [l[1] for l in lines] == want, arg
    for extra in (["--filmstrip", "0"], ["--filmstrip", "4", "--step-back"]):
        assert subprocess.run([exe, str(path)] + extra, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120).returncode == 2
