"""ScreenPressor seek index (jsp_sp_index_* / ScreenPressor.BuildScrubIndex / SpScrubIndex.Show / Manager.attach_index) on an MI355X.

Truth: the encoder's pictures and the oracle's sequential run with every destination first filled with the picture before it
(tests/sp_index_ref.py) — the contract of jsp_sp_index_show (include/jsplayer_amd.h).  Everything is bit-exact, and every t of
every clip is compared."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import sp_index_ref as ref
from jsplayer_amd import CodecError, MSVideo1_16bit, ScreenPressor, _native as N, player
from jsplayer_amd import streamgen as sg
from oracle_binding import OracleScreenPressor

pytestmark = pytest.mark.gpu

POISON = 0x5A5A5A5A


def dev_buf(n, fill=POISON, misalign=False):
    """A device frame buffer; `misalign`: a view that starts 4 bytes into its allocation (not 16-byte aligned)."""
    import torch
    if misalign:
        return torch.full((n + 4,), fill, dtype=torch.int32, device="cuda")[1:1 + n]
    return torch.full((n,), fill, dtype=torch.int32, device="cuda")


def make_sp(clip_or_w, h=None, bpp=None, lines=36):
    if h is None:
        clip_or_w, h, bpp = clip_or_w.w, clip_or_w.h, clip_or_w.bpp
    c = ScreenPressor(clip_or_w, h, bpp)
    c.Preinit(lines)
    return c


def picture(buf):
    return buf.cpu().numpy().view(np.uint32)


def sequential(gpu, chunks, keys, lo, hi, pool):
    """Frames [lo, hi) through DecompressI / DecompressP into `pool` (the first buffer that is not the previous frame);
    [(picture, verdict, which buffer data_pnt is)] of each."""
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


# (config, width, height, frames, bpp, version, key_every, key_row, destination 4 bytes off 16-byte alignment)
CLIPS = [
    (51, 64, 48, 41, 24, 4, 13, 36, False),
    (52, 100, 52, 41, 24, 3, 13, 7, False),
    (53, 37, 23, 41, 24, 2, 13, 5, False),       # X % 4 != 0: the scalar path
    (54, 320, 240, 41, 24, 4, 13, 36, False),
    (55, 320, 240, 41, 16, 2, 13, 36, True),
    (56, 64, 48, 41, 16, 3, 13, 36, True),
    (57, 100, 52, 41, 16, 4, 13, 7, False),
    (58, 320, 240, 90, 24, 4, 0, 36, False),     # one key frame, 89 frames behind it: three bitmap words, two host waves
    (59, 100, 52, 75, 16, 3, 0, 7, True),
]


def clip_id(c):
    return "cfg%d_%dx%d_n%d_%dbpp_v%d_k%d%s" % (c[0], c[1], c[2], c[3], c[4], c[5], c[6], "_misaligned" if c[8] else "")


@pytest.mark.parametrize("case", CLIPS, ids=clip_id)
def test_every_frame_descending_then_random(case):
    cfg, w, h, n, bpp, version, key_every, key_row, misalign = case
    clip = ref.make_clip(cfg, w, h, n, bpp, version, key_every, key_row)
    pictures, verdicts = ref.oracle_run(clip)
    gpu = make_sp(clip)
    idx = gpu.BuildScrubIndex(clip.chunks, clip.keys, key_row=key_row)
    assert idx.frames == n and idx.significance == verdicts
    dsts = [dev_buf(w * h, misalign=misalign) for _ in range(2)]
    order = list(range(n - 1, -1, -1)) + [int(t) for t in np.random.default_rng(cfg).permutation(n)]
    for k, t in enumerate(order):
        dst = dsts[k & 1]
        dst.fill_(POISON)
        r = idx.Show(t, dst)
        got = picture(dst)
        assert r.data_pnt is dst
        assert np.array_equal(got, clip.frames[t]), f"{clip.name} t={t}: not the encoder's picture"
        assert np.array_equal(got, pictures[t]), f"{clip.name} t={t}: not the oracle's picture"
        assert r.significant_changes == verdicts[t], f"{clip.name} t={t}: verdict"
    assert gpu.PreviousFrame() is None
    idx.close()
    gpu.StopAndClean()


def test_the_codec_is_only_lent():
    """A codec half-way through ANOTHER clip builds an index, shows frames into its pool's free buffers, then goes on decoding
    its own clip: every picture, verdict and data_pnt equals a twin codec's that never saw an index."""
    w, h = 100, 52
    own = ref.make_clip(61, w, h, 30, 24, 4, 9, 7)
    other = ref.make_clip(62, w, h, 41, 24, 4, 13, 7)
    pictures, verdicts = ref.oracle_run(other)
    gpu, twin = make_sp(own), make_sp(own)
    pool, tpool = [dev_buf(w * h) for _ in range(3)], [dev_buf(w * h) for _ in range(3)]
    a = sequential(gpu, own.chunks, own.keys, 0, 14, pool)
    b = sequential(twin, own.chunks, own.keys, 0, 14, tpool)
    idx = gpu.BuildScrubIndex(other.chunks, other.keys, key_row=7)
    for lo, hi in ((14, 15), (15, 22), (22, 30)):
        prev = gpu.PreviousFrame()
        prev_pic = picture(prev).copy()
        for t in (40, 17, 3, 25):
            for free in (b_ for b_ in pool if b_ is not prev):
                r = idx.Show(t, free)
                assert np.array_equal(picture(free), pictures[t]) and r.significant_changes == verdicts[t]
        assert gpu.PreviousFrame() is prev and np.array_equal(picture(prev), prev_pic)
        a += sequential(gpu, own.chunks, own.keys, lo, hi, pool)
        b += sequential(twin, own.chunks, own.keys, lo, hi, tpool)
    for i, (x, y) in enumerate(zip(a, b)):
        assert np.array_equal(x[0], y[0]) and x[1] == y[1] and x[2] == y[2], f"frame {i} after an index differs from the twin's"
        assert np.array_equal(x[0], own.frames[i]), f"frame {i}: not the encoder's picture"
    idx.close()
    gpu.StopAndClean()
    twin.StopAndClean()


def test_show_makes_the_codec_forget_the_buffers_last_column():
    """The one read an inter frame makes of its destination ("left of column 0").  The crafted clip's last frame is decoded into a
    buffer the codec has decoded into before (it remembers that buffer's last column) — after a Show has written another picture
    there.  The result is what the oracle gives for a destination holding the SHOWN picture."""
    from test_screenpressor_cpu import column0_clip
    w, h, y0, chunks, _ = column0_clip(4)
    other = ref.make_clip(63, w, h, 20, 24, 4, 0, 36)
    gpu = make_sp(w, h, 24)
    idx = gpu.BuildScrubIndex(other.chunks, other.keys)
    a, b = dev_buf(w * h), dev_buf(w * h)
    assert gpu.DecompressI(chunks[0], a) == 0
    assert gpu.DecompressP(chunks[1], b).data_pnt is b
    f0 = picture(a).copy()
    t = next(t for t in range(19, -1, -1) if int(other.frames[t].reshape(h, w)[y0 - 1, w - 1]) != int(f0.reshape(h, w)[y0 - 1, w - 1]))
    idx.Show(t, a)
    shown = picture(a).copy()
    assert np.array_equal(shown, other.frames[t])
    assert gpu.DecompressP(chunks[2], a).data_pnt is a

    def oracle_with(a_holds):
        o = OracleScreenPressor(w, h, 24)
        o.Preinit(36)
        oa, ob = np.zeros(w * h, np.int32), np.zeros(w * h, np.int32)
        o.DecompressI(chunks[0], oa)
        o.DecompressP(chunks[1], ob)
        oa[:] = a_holds.view(np.int32)
        o.DecompressP(chunks[2], oa)
        out = o.PreviousFrame().view(np.uint32).copy()
        o.close()
        return out

    want, remembered = oracle_with(shown), oracle_with(f0)
    assert not np.array_equal(want, remembered), "the clip does not tell the two destinations apart"
    assert np.array_equal(picture(a), want)
    idx.close()
    gpu.StopAndClean()


def test_the_index_holds_everything():
    clip = ref.make_clip(64, 100, 52, 41, 24, 4, 13, 7)
    pictures, verdicts = ref.oracle_run(clip)
    gpu = make_sp(clip)
    srcs = [np.frombuffer(c, dtype=np.uint8).copy() for c in clip.chunks]
    idx = gpu.BuildScrubIndex(srcs, clip.keys, key_row=7)
    for s in srcs:
        s[:] = 0xA5
    assert idx.frames == 41
    assert idx.device_bytes >= sum(clip.keys) * clip.w * clip.h * 4 > 0
    assert idx.host_bytes > 0
    dst = dev_buf(clip.w * clip.h)
    for t in range(40, -1, -1):
        dst.fill_(POISON)
        r = idx.Show(t, dst)
        assert np.array_equal(picture(dst), pictures[t]) and r.significant_changes == verdicts[t], f"t={t}"
    gpu.StopAndClean()
    with pytest.raises(CodecError):
        idx.Show(0, dst)
    idx.close()        # after the codec is gone
    idx.close()


def _raw_build(lib, handle, chunks, keys, key_row=36, n=None, null_srcs=False):
    n = len(chunks) if n is None else n
    keep = [bytes(c) for c in chunks]
    ptrs = (C.c_void_p * max(len(keep), 1))(*[C.cast(C.c_char_p(k), C.c_void_p).value for k in keep])
    lens = (C.c_size_t * max(len(keep), 1))(*[len(k) for k in keep])
    kb = bytes(bytearray(1 if k else 0 for k in keys))
    return lib.jsp_sp_index_build(handle, n, None if null_srcs else ptrs, lens, kb, key_row)


def test_refusals_change_nothing():
    w, h = 64, 48
    clip = ref.make_clip(65, w, h, 41, 24, 4, 13, 36)
    clip2 = ref.make_clip(66, w, h, 41, 24, 2, 13, 36)
    pictures, _ = ref.oracle_run(clip)
    lib = N.lib()
    gpu = make_sp(clip)
    pool = [dev_buf(w * h) for _ in range(3)]
    done = sequential(gpu, clip.chunks, clip.keys, 0, 20, pool)
    prev = gpu.PreviousFrame()
    prev_pic = picture(prev).copy()
    poisoned = dev_buf(w * h)
    idx = gpu.BuildScrubIndex(clip.chunks, clip.keys)

    def unchanged(what):
        assert gpu.PreviousFrame() is prev, what
        assert np.array_equal(picture(prev), prev_pic), what
        assert bool((poisoned == POISON).all()), what + ": dst was written"

    def refused_build(what, needle, *a, **kw):
        assert not _raw_build(lib, gpu._h, *a, **kw), what
        assert needle in N.last_error(), (what, N.last_error())
        unchanged(what)

    # ---- build ----
    msv = MSVideo1_16bit(w, h)
    assert not _raw_build(lib, msv._h, clip.chunks, clip.keys)
    assert "sp_index: ScreenPressor only" in N.last_error()
    refused_build("starts at an inter frame", "coded key frame", clip.chunks[1:], clip.keys[1:])
    flat = next(t for t, (c, k) in enumerate(zip(clip.chunks, clip.keys)) if k and (c[0] & 0xF) == 1)
    refused_build("starts at a flat key frame", "coded key frame", clip.chunks[flat:], clip.keys[flat:])
    bad = list(clip.chunks)
    bad[13] = bytes([0x13, 0, 0, 0])                          # an unknown frame header: JSP_ERROR_OCCURED
    refused_build("invalid key frame", "frame 13", bad, clip.keys)
    cut = list(clip2.chunks)
    cut[26] = cut[26][: len(cut[26]) // 2]                    # version 2: the cut poisons the range coder, the previous frame is cleared
    refused_build("truncated key frame", "frame 26", cut, clip2.keys)
    refused_build("empty range", "sp_index", clip.chunks, clip.keys, n=0)
    refused_build("null srcs", "null argument", clip.chunks, clip.keys, null_srcs=True)
    refused_build("negative key_row", "key_row", clip.chunks, clip.keys, key_row=-1)
    assert not lib.jsp_sp_index_build(None, 1, None, None, None, 0) and "null argument" in N.last_error()

    # ---- show ----
    def refused_show(what, needle, codec, index, t, dst):
        with pytest.raises(CodecError) as e:
            (index if codec is None else _Rebound(index, codec)).Show(t, dst)
        assert needle in str(e.value), (what, str(e.value))
        unchanged(what)

    refused_show("t too large", "outside the index", None, idx, 41, poisoned)
    refused_show("t negative", "outside the index", None, idx, -1, poisoned)
    refused_show("dst is the previous frame", "previous frame", None, idx, 3, prev)
    host = np.full(w * h, POISON, dtype=np.int32)
    refused_show("host dst", "device frame buffer", None, idx, 3, host)
    assert (host == np.int32(POISON)).all()
    other = make_sp(clip)
    refused_show("another codec's index", "another codec", other, idx, 3, poisoned)
    refused_show("an MSVideo1 codec", "ScreenPressor only", msv, idx, 3, poisoned)
    sig = C.c_int(7)
    assert lib.jsp_sp_index_show(gpu._h, None, 0, C.c_void_p(poisoned.data_ptr()), C.byref(sig)) != 0 and sig.value == 7
    assert lib.jsp_sp_index_show(gpu._h, idx._h, 0, None, C.byref(sig)) != 0 and sig.value == 7
    unchanged("null arguments")
    # an asynchronous frame in flight
    free = next(b for b in pool if b is not prev)
    ticket = gpu.DecompressI_async(clip.chunks[0], free)
    with pytest.raises(CodecError) as e:
        idx.Show(3, poisoned)
    assert "in flight" in str(e.value)
    assert bool((poisoned == POISON).all())
    gpu.wait(ticket)

    # ---- and the stream goes on: the frame in flight restarted the clip, the following frames are exact ----
    after = sequential(gpu, clip.chunks, clip.keys, 1, 20, pool)
    for i, got in enumerate(after, start=1):
        assert np.array_equal(got[0], pictures[i]) and np.array_equal(got[0], done[i][0]) and got[1] == done[i][1], f"frame {i} after the refusals"
    idx.close()
    other.StopAndClean()
    msv.StopAndClean()
    gpu.StopAndClean()


class _Rebound:
    """SpScrubIndex.Show of `index` called through ANOTHER codec (what the C ABI allows a caller to get wrong)."""

    def __init__(self, index, codec):
        self.index, self.codec = index, codec

    def Show(self, t, dst):
        signif = C.c_int(0)
        addr = dst.data_ptr() if hasattr(dst, "data_ptr") else dst.ctypes.data
        if self.index._lib.jsp_sp_index_show(self.codec._h, self.index._h, int(t), C.c_void_p(addr), C.byref(signif)) != 0:
            raise CodecError(N.last_error())


def test_full_size_pclip300_every_frame():
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
    assert idx.frames == 300 and idx.device_bytes > sum(c.keys) * wl.W * wl.H * 4
    bufs = [dev_buf(wl.W * wl.H) for _ in range(2)]
    # (ordinary encoder output never reads its destination, so the committed digests of the plain sequential run apply)
    wrong = []
    for t in range(299, -1, -1):
        dst = bufs[t & 1]
        dst.fill_(POISON)
        idx.Show(t, dst)
        if wl.digest(dst.cpu().numpy()) != want[t]:
            wrong.append(t)
    assert not wrong, f"frames whose digest differs from the golden one: {wrong}"
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


def test_manager_step_back_and_skip_stills_equal_a_manager_without_an_index():
    from jsplayer_amd.avi import CODEC_SCREENPRESSOR, VideoInfo
    w, h = 100, 52
    # (coded key frames only: a Manager that seeks lands on the nearest key frame, and a flat one renews no entropy state)
    chunks, keys, frames = sg.sp_clip(67, w, h, 41, bpp=24, version=4, key_every=13, unchanged_at=(3, 4, 30),
                                      p_mix_at={6: dict(unchanged=0.3, motion=0.6), 20: dict(unchanged=0.35, motion=0.45)})
    clip = ref.Clip("manager", w, h, 24, 4, player.INSIGNIFICANT_LINES, chunks, keys, [f.astype(np.uint32) for f in frames])
    n, inside = 41, 33                                    # the index covers frames 0 .. 32; play goes on past its end
    vi = VideoInfo(X=w, Y=h, bpp=24, fps=15.0, nframes=n, codec=CODEC_SCREENPRESSOR, palette=None, riff_size=0)
    dec, plain_dec = make_sp(clip), make_sp(clip)
    spy = _Spy(dec)
    mgr = player.Manager(vi, spy, lambda k: dev_buf(k))
    plain = player.Manager(vi, plain_dec, lambda k: dev_buf(k))
    idx = dec.BuildScrubIndex(clip.chunks[:inside], clip.keys[:inside], key_row=player.INSIGNIFICANT_LINES)
    mgr.attach_index(idx, 0)
    # the plain Manager plays the clip once: its log is the significance record the reference's loader keeps
    plain.play(clip.chunks, key_flags=clip.keys)
    known = {d.index: d.significant_changes for d in plain.log}
    assert [idx.significance[t] for t in range(inside)] == [bool(known[t]) for t in range(inside)]

    def same(a, b, what):
        assert a.index == b.index, what
        assert np.array_equal(picture(mgr.buffers[a.buffer_index]), picture(plain.buffers[b.buffer_index])), what
        assert np.array_equal(picture(mgr.buffers[a.buffer_index]), clip.frames[a.index]), what

    same(mgr.seek(clip.chunks, inside - 1, clip.keys), plain.seek(clip.chunks, inside - 1, clip.keys), "seek to the index's last frame")
    for t in range(inside - 2, -1, -1):
        a, b = mgr.prev_frame(clip.chunks, clip.keys), plain.prev_frame(clip.chunks, clip.keys)
        same(a, b, f"step back to {t}")
        assert a.index == t and bool(a.significant_changes) == bool(known[t])
    assert spy.calls == [], spy.calls
    a = b = None
    while a is None or a.index < inside - 1:
        a, b = mgr.skip_stills(clip.chunks[:inside], clip.keys[:inside]), plain.skip_stills(clip.chunks[:inside], clip.keys[:inside])
        same(a, b, f"skip to {a.index}")
    assert spy.calls == [], spy.calls
    assert mgr.next_frame_to_decode == 0 and dec.PreviousFrame() is None
    # playing on past the index's end: the decoder really stands at frame 0, and every frame up to the clip's end is exact
    for t in (inside, inside + 1, n - 1):
        same(mgr.seek(clip.chunks, t, clip.keys), plain.seek(clip.chunks, t, clip.keys), f"seek past the index to {t}")
    idx.close()
    dec.StopAndClean()
    plain_dec.StopAndClean()


def test_jsp_play_step_back_matches_the_plain_run(tmp_path):
    from jsplayer_amd import avi
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "examples", "jsp_play")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-s", "-C", os.path.join(root, "examples")])
    w, h = 320, 240
    chunks, keys, _ = sg.sp_clip(97, w, h, 40, bpp=24, version=4, key_every=16, unchanged_at=(5,))
    path = tmp_path / "clip.avi"
    path.write_bytes(avi.write_avi(w, h, chunks, fourcc=b"SCPR", bpp=24, fps=15.0, key_flags=keys))

    def run(extra):
        res = subprocess.run([exe, str(path)] + extra, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
        assert res.returncode == 0, res.stderr.decode()
        return [l.split() for l in res.stdout.decode().splitlines() if l and l[0].isdigit()]

    plain = sorted((int(l[0]), l[1], int(l[3]), l[-1]) for l in run([]))
    back = run(["--step-back"])
    assert [int(l[0]) for l in back] == list(range(39, -1, -1))
    assert sorted((int(l[0]), l[1], int(l[2]), l[-1]) for l in back) == plain
