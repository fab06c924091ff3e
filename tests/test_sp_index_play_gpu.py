"""Playback from the ScreenPressor seek index (jsp_sp_index_play / SpScrubIndex.Play / Manager.play_from_index /
jsp_play --play-index) on an MI355X.

Truth: the encoder's pictures, the oracle's sequential run with every destination first filled with the picture before it
(tests/sp_index_ref.py), and what jsp_sp_index_show writes — the contract of jsp_sp_index_play (include/jsplayer_amd.h): dsts[k]
receives exactly the picture Show(first + k * stride) writes.  Everything is bit-exact.  Every destination is filled with a poison
word before each call, and one more poisoned buffer that is NOT listed must stay poisoned."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import sp_index_ref as ref
from jsplayer_amd import CodecError, FramePool, MSVideo1_16bit, _native as N, player
from jsplayer_amd import streamgen as sg
from oracle_binding import OracleScreenPressor
from test_sp_index_gpu import POISON, _Spy, dev_buf, make_sp, picture, sequential

pytestmark = pytest.mark.gpu

# test_sp_index_gpu.CLIPS, restated: (config, width, height, frames, bpp, version, key_every, key_row, destinations 4 bytes off
# 16-byte alignment)
CLIPS = [
    (51, 64, 48, 41, 24, 4, 13, 36, False),
    (52, 100, 52, 41, 24, 3, 13, 7, False),
    (53, 37, 23, 41, 24, 2, 13, 5, False),       # X % 4 != 0: the scalar path
    (54, 320, 240, 41, 24, 4, 13, 36, False),
    (55, 320, 240, 41, 16, 2, 13, 36, True),
    (56, 64, 48, 41, 16, 3, 13, 36, True),
    (57, 100, 52, 41, 16, 4, 13, 7, False),
    (58, 320, 240, 90, 24, 4, 0, 36, False),     # one key frame, 89 frames behind it: three bitmap words
    (59, 100, 52, 75, 16, 3, 0, 7, True),
]


def clip_id(c):
    return "cfg%d_%dx%d_n%d_%dbpp_v%d_k%d%s" % (c[0], c[1], c[2], c[3], c[4], c[5], c[6], "_misaligned" if c[8] else "")


def test_the_clips_are_those_of_the_show_tests():
    import test_sp_index_gpu
    assert CLIPS == test_sp_index_gpu.CLIPS


def poisoned(buf):
    return bool((buf == POISON).all())


class Played:
    """A clip, its index and a pool of poisoned buffers; `check` plays a run and compares every picture and verdict."""

    def __init__(self, clip, gpu, idx, pictures, verdicts, misalign=False, nbuf=None):
        self.clip, self.gpu, self.idx, self.pictures, self.verdicts = clip, gpu, idx, pictures, verdicts
        n = len(clip.keys)
        self.bufs = [dev_buf(clip.w * clip.h, misalign=misalign) for _ in range(nbuf or n)]
        self.extra = dev_buf(clip.w * clip.h, misalign=misalign)     # never listed: must stay poisoned
        scratch = dev_buf(clip.w * clip.h, misalign=misalign)
        self.shown = []
        for t in range(n):
            scratch.fill_(POISON)
            idx.Show(t, scratch)
            self.shown.append(picture(scratch).copy())

    def check(self, first, count, stride=1, reverse=False):
        what = f"{self.clip.name} Play({first}, {count}, stride {stride}{', buffers reversed' if reverse else ''})"
        dsts = self.bufs[:count][::-1] if reverse else self.bufs[:count]
        for b in dsts:
            b.fill_(POISON)
        res = self.idx.Play(first, dsts, stride)
        assert len(res) == count, what
        for k, (r, dst) in enumerate(zip(res, dsts)):
            t = first + k * stride
            got = picture(dst)
            assert r.data_pnt is dst, what
            assert np.array_equal(got, self.clip.frames[t]), f"{what} frame {t}: not the encoder's picture"
            assert np.array_equal(got, self.pictures[t]), f"{what} frame {t}: not the oracle's picture"
            assert np.array_equal(got, self.shown[t]), f"{what} frame {t}: not what Show writes"
            assert r.significant_changes == self.verdicts[t] == self.idx.significance[t], f"{what} frame {t}: verdict"
        assert poisoned(self.extra), what + ": a buffer that was not listed was written"


@pytest.mark.parametrize("case", CLIPS, ids=clip_id)
def test_play_equals_show_encoder_and_oracle(case):
    cfg, w, h, n, bpp, version, key_every, key_row, misalign = case
    clip = ref.make_clip(cfg, w, h, n, bpp, version, key_every, key_row)
    pictures, verdicts = ref.oracle_run(clip)
    gpu = make_sp(clip)
    idx = gpu.BuildScrubIndex(clip.chunks, clip.keys, key_row=key_row)
    assert idx.frames == n and idx.significance == verdicts
    p = Played(clip, gpu, idx, pictures, verdicts, misalign)
    for b in p.bufs:
        b.fill_(POISON)
    p.check(0, n)                                           # all frames: every key frame inside, every bitmap word
    p.check(0, n, reverse=True)
    for first in range(n):                                  # from every first frame
        p.check(first, min(5, n - first))
    for stride in (2, 7):
        for first in (0, 1, 6):
            p.check(first, (n - 1 - first) // stride + 1, stride)
        p.check(3, (n - 4) // stride + 1, stride, reverse=True)
    for k in [t for t, key in enumerate(clip.keys) if key and t > 0]:
        for first in (k - 1, k, k + 1):                     # just before, on and just after a key frame
            if first < n:
                p.check(first, min(9, n - first))
                p.check(first, (n - 1 - first) // 2 + 1, 2)
    if n > 64:                                              # runs that span three bitmap words, from an inter frame
        p.check(30, 36)
        p.check(31, 34)
        p.check(17, (n - 1 - 17) // 7 + 1, 7)
        p.check(31, 2, 33)
    p.check(n - 1, 1)
    p.check(0, 1, 5)
    assert gpu.PreviousFrame() is None
    idx.close()
    gpu.StopAndClean()


def test_one_misaligned_destination_among_aligned_ones():
    """X % 4 == 0, every destination 16-byte aligned but one: the call takes the scalar instantiation and is still exact."""
    clip = ref.make_clip(71, 64, 48, 41, 24, 4, 13, 36)
    pictures, verdicts = ref.oracle_run(clip)
    gpu = make_sp(clip)
    idx = gpu.BuildScrubIndex(clip.chunks, clip.keys)
    p = Played(clip, gpu, idx, pictures, verdicts, nbuf=12)
    for odd in (0, 5, 11):
        p.bufs[odd] = dev_buf(clip.w * clip.h, misalign=True)
        assert p.bufs[odd].data_ptr() % 16 != 0 and all(b.data_ptr() % 16 == 0 for k, b in enumerate(p.bufs) if k != odd)
        p.check(9, 12)
        p.check(2, 12, 3)
        p.bufs[odd] = dev_buf(clip.w * clip.h)
    idx.close()
    gpu.StopAndClean()


def test_the_codec_is_only_lent():
    """A sequential decode interrupted by Play calls between any two frames (into the pool's buffers that are not the previous
    frame) produces the pictures, verdicts and data_pnt of a twin codec's uninterrupted one; PreviousFrame() is unchanged."""
    w, h = 100, 52
    own = ref.make_clip(72, w, h, 30, 24, 4, 9, 7)
    other = ref.make_clip(73, w, h, 41, 24, 4, 13, 7)
    pictures, verdicts = ref.oracle_run(other)
    gpu, twin = make_sp(own), make_sp(own)
    pool, tpool = [dev_buf(w * h) for _ in range(4)], [dev_buf(w * h) for _ in range(4)]
    idx = gpu.BuildScrubIndex(other.chunks, other.keys, key_row=7)
    a, b = [], []
    for i in range(30):
        prev = gpu.PreviousFrame()
        prev_pic = picture(prev).copy() if prev is not None else None
        free = [buf for buf in pool if buf is not prev]
        first, stride = (7 * i) % 28, 1 + i % 4
        res = idx.Play(first, free, stride)
        for k, (r, buf) in enumerate(zip(res, free)):
            t = first + k * stride
            assert np.array_equal(picture(buf), pictures[t]) and r.significant_changes == verdicts[t], f"before frame {i}: Play frame {t}"
        assert gpu.PreviousFrame() is prev
        if prev is not None:
            assert np.array_equal(picture(prev), prev_pic)
        a += sequential(gpu, own.chunks, own.keys, i, i + 1, pool)
        b += sequential(twin, own.chunks, own.keys, i, i + 1, tpool)
    for i, (x, y) in enumerate(zip(a, b)):
        assert np.array_equal(x[0], y[0]) and x[1] == y[1] and x[2] == y[2], f"frame {i} between Plays differs from the twin's"
        assert np.array_equal(x[0], own.frames[i]), f"frame {i}: not the encoder's picture"
    idx.close()
    gpu.StopAndClean()
    twin.StopAndClean()


@pytest.mark.parametrize("which", [0, 1])
def test_play_makes_the_codec_forget_the_last_column_of_every_destination(which):
    """test_show_makes_the_codec_forget_the_buffers_last_column, for two destinations: the crafted clip's last frame reads its
    destination left of column 0.  It is decoded into a buffer the codec has decoded into before — after a Play has written other
    pictures into two such buffers — and the result is what the oracle gives for a destination holding the PLAYED picture,
    whichever of the two destinations it is."""
    from test_screenpressor_cpu import column0_clip
    w, h, y0, chunks, _ = column0_clip(4)
    other = ref.make_clip(63, w, h, 20, 24, 4, 0, 36)
    gpu = make_sp(w, h, 24)
    idx = gpu.BuildScrubIndex(other.chunks, other.keys)
    a, b, c = dev_buf(w * h), dev_buf(w * h), dev_buf(w * h)
    assert gpu.DecompressI(chunks[0], c) == 0               # the codec remembers the last column of c ...
    assert gpu.DecompressI(chunks[0], a) == 0               # ... and of a: both hold frame 0
    assert gpu.DecompressP(chunks[1], b).data_pnt is b
    f0 = picture(a).copy()
    assert np.array_equal(picture(c), f0)
    differ = [t for t in range(20) if int(other.frames[t].reshape(h, w)[y0 - 1, w - 1]) != int(f0.reshape(h, w)[y0 - 1, w - 1])]
    assert len(differ) >= 2
    t1, t2 = differ[0], differ[-1]
    idx.Play(t1, [a, c], t2 - t1)
    dst = (a, c)[which]
    shown = picture(dst).copy()
    assert np.array_equal(shown, other.frames[(t1, t2)[which]])
    assert gpu.DecompressP(chunks[2], dst).data_pnt is dst

    def oracle_with(dst_holds):
        o = OracleScreenPressor(w, h, 24)
        o.Preinit(36)
        oa, ob = np.zeros(w * h, np.int32), np.zeros(w * h, np.int32)
        o.DecompressI(chunks[0], oa)
        o.DecompressP(chunks[1], ob)
        oa[:] = dst_holds.view(np.int32)
        o.DecompressP(chunks[2], oa)
        out = o.PreviousFrame().view(np.uint32).copy()
        o.close()
        return out

    want, remembered = oracle_with(shown), oracle_with(f0)
    assert not np.array_equal(want, remembered), "the clip does not tell the two destinations apart"
    assert np.array_equal(picture(dst), want)
    idx.close()
    gpu.StopAndClean()


def _raw_play(lib, codec_h, index_h, first, ptrs, stride=1, n=None, sig=None):
    n = len(ptrs) if n is None else n
    arr = (C.c_void_p * max(len(ptrs), 1))(*ptrs) if ptrs is not None else None
    return lib.jsp_sp_index_play(codec_h, index_h, first, n, stride, arr, sig)


def test_refusals_change_nothing():
    w, h = 64, 48
    clip = ref.make_clip(65, w, h, 41, 24, 4, 13, 36)
    pictures, _ = ref.oracle_run(clip)
    lib = N.lib()
    gpu = make_sp(clip)
    pool = [dev_buf(w * h) for _ in range(3)]
    done = sequential(gpu, clip.chunks, clip.keys, 0, 20, pool)
    prev = gpu.PreviousFrame()
    prev_pic = picture(prev).copy()
    x, y, z = dev_buf(w * h), dev_buf(w * h), dev_buf(w * h)
    idx = gpu.BuildScrubIndex(clip.chunks, clip.keys)
    bytes_before = idx.device_bytes

    def unchanged(what):
        assert gpu.PreviousFrame() is prev, what
        assert np.array_equal(picture(prev), prev_pic), what
        assert poisoned(x) and poisoned(y) and poisoned(z), what + ": a buffer was written"

    def refused(what, needle, first, dsts, stride=1, codec=None, n=None, prefix="sp_index_play:"):
        sig = (C.c_int * 8)(*([7] * 8))
        ptrs = [d.data_ptr() if hasattr(d, "data_ptr") else (d.ctypes.data if d is not None else None) for d in dsts]
        assert _raw_play(lib, (codec or gpu)._h, idx._h, first, ptrs, stride, n, sig) != 0, what
        err = N.last_error()
        assert err.startswith(prefix) and needle in err, (what, err)
        assert list(sig) == [7] * 8, what + ": a verdict was written"
        unchanged(what)

    msv, other = MSVideo1_16bit(w, h), make_sp(clip)
    refused("an MSVideo1 codec", "ScreenPressor only", 3, [x, y], codec=msv, prefix="sp_index: ScreenPressor only")
    refused("another codec's index", "another codec", 3, [x, y], codec=other)
    refused("n = 0", "1..4096", 3, [x, y], n=0)
    refused("n = 4097", "1..4096", 0, [x] * 4097, n=4097)
    refused("n negative", "1..4096", 3, [x, y], n=-1)
    refused("stride 0", "stride", 3, [x, y], 0)
    refused("stride negative", "stride", 3, [x, y], -2)
    refused("first negative", "outside the index", -1, [x, y])
    refused("first past the end", "outside the index", 41, [x])
    refused("the run's last frame past the end", "outside the index", 39, [x, y, z])
    refused("the run's last frame past the end, strided", "outside the index", 1, [x, y, z], 20)
    refused("a last frame that overflows 32 bits", "outside the index", 1, [x, y, z], 1 << 30)
    refused("a last frame that wraps round 32 bits to frame 0", "outside the index", 2, [x, y, z], (1 << 31) - 1)
    refused("a null entry of dsts", "null", 3, [x, None, z])
    refused("the same buffer twice", "twice", 3, [x, y, x])
    refused("a buffer that is the previous frame", "previous frame", 3, [x, prev, z])
    host = np.full(w * h, POISON, dtype=np.int32)
    refused("a host-pointer buffer", "device frame buffer", 3, [x, host, z])
    assert (host == np.int32(POISON)).all()
    sig = (C.c_int * 2)(7, 7)
    two = [x.data_ptr(), y.data_ptr()]
    assert _raw_play(lib, None, idx._h, 3, two, sig=sig) != 0 and N.last_error().startswith("sp_index_play:")
    assert _raw_play(lib, gpu._h, None, 3, two, sig=sig) != 0 and N.last_error().startswith("sp_index_play:")
    assert _raw_play(lib, gpu._h, idx._h, 3, None, n=2, sig=sig) != 0 and N.last_error().startswith("sp_index_play:")
    assert list(sig) == [7, 7]
    unchanged("null arguments")
    # through Python: CodecError with the library's message
    with pytest.raises(CodecError) as e:
        idx.Play(39, [x, y, z])
    assert str(e.value).startswith("sp_index_play:") and "outside the index" in str(e.value)
    with pytest.raises(CodecError) as e:
        idx.Play(3, [])
    assert "1..4096" in str(e.value)
    unchanged("refused through Python")
    # an asynchronous frame in flight
    free = next(b for b in pool if b is not prev)
    ticket = gpu.DecompressI_async(clip.chunks[0], free)
    with pytest.raises(CodecError) as e:
        idx.Play(3, [x, y])
    assert str(e.value).startswith("sp_index_play:") and "in flight" in str(e.value)
    assert poisoned(x) and poisoned(y) and poisoned(z)
    gpu.wait(ticket)
    assert idx.device_bytes == bytes_before, "a refused Play left memory behind"
    n_, dev, hostb = C.c_int(0), C.c_uint64(0), C.c_uint64(0)
    lib.jsp_sp_index_info(idx._h, C.byref(n_), C.byref(dev), C.byref(hostb))
    assert dev.value == bytes_before, "a refused Play left memory behind"

    # ---- and the stream goes on: the frame in flight restarted the clip, the following frames are exact ----
    after = sequential(gpu, clip.chunks, clip.keys, 1, 20, pool)
    for i, got in enumerate(after, start=1):
        assert np.array_equal(got[0], pictures[i]) and np.array_equal(got[0], done[i][0]) and got[1] == done[i][1], f"frame {i} after the refusals"
    # a closed index, a closed codec
    ok = idx.Play(3, [x, y])
    assert np.array_equal(picture(x), pictures[3]) and np.array_equal(picture(y), pictures[4]) and len(ok) == 2
    x.fill_(POISON)
    other_idx = other.BuildScrubIndex(clip.chunks, clip.keys)
    other.StopAndClean()
    with pytest.raises(CodecError) as e:
        other_idx.Play(3, [x])
    assert "closed" in str(e.value)
    other_idx.close()
    idx.close()
    with pytest.raises(CodecError) as e:
        idx.Play(3, [x])
    assert "closed" in str(e.value)
    assert poisoned(x)
    msv.StopAndClean()
    gpu.StopAndClean()


def test_index_info_counts_what_play_adds_and_nothing_before():
    clip = ref.make_clip(74, 100, 52, 41, 24, 4, 13, 7)
    gpu = make_sp(clip)
    idx = gpu.BuildScrubIndex(clip.chunks, clip.keys, key_row=7)
    lib = N.lib()

    def device_bytes():
        n, dev, host = C.c_int(0), C.c_uint64(0), C.c_uint64(0)
        assert lib.jsp_sp_index_info(idx._h, C.byref(n), C.byref(dev), C.byref(host)) == 0
        return dev.value

    def reserve(nbytes):                                    # what a grown-on-demand array of nbytes holds (DeviceBuffer::reserve)
        return nbytes + nbytes // 4 + 256

    built = device_bytes()
    assert built == idx.device_bytes
    bufs = [dev_buf(clip.w * clip.h) for _ in range(41)]
    idx.Show(17, bufs[0])
    assert device_bytes() == built, "Show changed what the index holds"
    idx.Thumbs([0, 5, 9], scale=4)
    thumbs = device_bytes()
    assert thumbs == built + reserve(3 * 24), "Thumbs holds something other than its three 24-byte records"
    idx.Play(4, bufs[:5])
    first = device_bytes()
    table = 41 * 16 + 2 * 4                                 # a 16-byte record per frame and a key-frame bit per frame, 32 to a word
    assert first == thumbs + table + reserve(5 * 8), "the first Play adds the per-frame table and five destination pointers"
    assert idx.device_bytes == first
    idx.Play(20, bufs[:5], 3)
    idx.Play(0, bufs[:2])
    assert device_bytes() == first, "a second Play of the same size grew the index"
    idx.Play(0, bufs[:12])                                  # (still within what the first call reserved)
    assert device_bytes() == first
    idx.Play(0, bufs)                                       # a longer destination list grows, the table does not
    assert device_bytes() == thumbs + table + reserve(41 * 8)
    idx.close()
    gpu.StopAndClean()


def test_full_size_pclip300():
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
    pool = FramePool(wl.W, wl.H, 300)
    extra = dev_buf(wl.W * wl.H)
    for b in pool.frames:
        b.fill_(POISON)
    res = idx.Play(0, pool.frames)
    assert [r.significant_changes for r in res] == idx.significance
    wrong = [t for t in range(300) if wl.digest(pool.frames[t].cpu().numpy()) != want[t]]
    assert not wrong, f"Play(0, 300): frames whose digest differs from the golden one: {wrong}"
    assert poisoned(extra)
    for b in pool.frames[:20]:      # the 19 destinations, and the buffer behind them, which is not listed and must stay poisoned
        b.fill_(POISON)
    res = idx.Play(150, pool.frames[:19], 8)
    frames = [150 + 8 * k for k in range(19)]
    assert [r.significant_changes for r in res] == [idx.significance[t] for t in frames]
    wrong = [t for k, t in enumerate(frames) if wl.digest(pool.frames[k].cpu().numpy()) != want[t]]
    assert not wrong, f"Play(150, 19, stride 8): frames whose digest differs from the golden one: {wrong}"
    assert poisoned(extra) and poisoned(pool.frames[19])
    idx.close()
    pool.close()
    codec.StopAndClean()


def test_manager_play_from_index_equals_a_manager_that_seeks_frame_by_frame():
    from jsplayer_amd.avi import CODEC_SCREENPRESSOR, VideoInfo
    w, h = 100, 52
    # (coded key frames only: a Manager that seeks lands on the nearest key frame, and a flat one renews no entropy state)
    chunks, keys, frames = sg.sp_clip(75, w, h, 41, bpp=24, version=4, key_every=13, unchanged_at=(3, 4, 30),
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
    plain.play(clip.chunks, key_flags=clip.keys)          # the significance record of a plain sequential run
    known = {d.index: d.significant_changes for d in plain.log}

    def run(start, count, stride):
        got = []
        mgr.play_from_index(start, count, stride, on_frame=lambda d, buf: got.append((d, picture(buf).copy())), key_flags=clip.keys)
        want = range(start, inside, stride) if count is None else range(start, start + count * stride, stride)
        assert [d.index for d, _ in got] == list(want)
        for d, pic in got:
            s = plain.seek(clip.chunks, d.index, clip.keys)
            assert np.array_equal(pic, picture(plain.buffers[s.buffer_index])), f"frame {d.index}: not the seeking Manager's picture"
            assert np.array_equal(pic, clip.frames[d.index]), f"frame {d.index}: not the encoder's picture"
            assert bool(d.significant_changes) == bool(known[d.index]), f"frame {d.index}: verdict"
            assert d.key == clip.keys[d.index] and mgr.log[-len(got):] == [g for g, _ in got]
        last = got[-1][0]
        assert np.array_equal(picture(mgr.buffers[last.buffer_index]), clip.frames[last.index])
        assert mgr.holds[last.buffer_index] == range(last.index, last.index + 1) and mgr.frame_of_interest == last.index

    run(5, None, 1)                                        # play on from a shown frame to the end of the index: 28 frames, 4 batches
    run(0, 11, 3)                                          # fast-forward
    run(12, 9, 1)                                          # from just before a key frame, one batch
    assert spy.calls == [] and mgr.next_frame_to_decode == 0 and dec.PreviousFrame() is None
    # play goes on past the index: seek() to the next clip frame, then frame by frame
    for t in (inside, inside + 1, n - 1):
        a, b = mgr.seek(clip.chunks, t, clip.keys), plain.seek(clip.chunks, t, clip.keys)
        assert np.array_equal(picture(mgr.buffers[a.buffer_index]), picture(plain.buffers[b.buffer_index])), f"seek past the index to {t}"
        assert np.array_equal(picture(mgr.buffers[a.buffer_index]), clip.frames[t])
    # ... and with the decoder standing somewhere, its previous buffer is never a destination
    prev = dec.PreviousFrame()
    prev_pic = picture(prev).copy()
    run(2, 20, 1)
    assert dec.PreviousFrame() is prev and np.array_equal(picture(prev), prev_pic)
    idx.close()
    dec.StopAndClean()
    plain_dec.StopAndClean()


def test_jsp_play_play_index_matches_the_plain_run(tmp_path):
    from jsplayer_amd import avi
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "examples", "jsp_play")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-s", "-C", os.path.join(root, "examples")])
    w, h = 320, 240
    chunks, keys, _ = sg.sp_clip(98, w, h, 40, bpp=24, version=4, key_every=16, unchanged_at=(5,))
    path = tmp_path / "clip.avi"
    path.write_bytes(avi.write_avi(w, h, chunks, fourcc=b"SCPR", bpp=24, fps=15.0, key_flags=keys))

    def run(extra, target=path):
        res = subprocess.run([exe, str(target)] + extra, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
        return res.returncode, [l.split() for l in res.stdout.decode().splitlines() if l and l[0].isdigit()], res.stderr.decode()

    rc, lines, err = run([])
    assert rc == 0, err
    plain = {int(l[0]): (l[1], int(l[3]), l[-1]) for l in lines}
    assert len(plain) == 40
    for arg, want in (("0", list(range(40))), ("3:20", list(range(3, 23))), ("1:6:7", list(range(1, 40, 7))), ("39", [39]), ("15:4:2", [15, 17, 19, 21])):
        rc, lines, err = run(["--play-index", arg])
        assert rc == 0, (arg, err)
        assert [int(l[0]) for l in lines] == want, arg
        assert [(l[1], int(l[2]), l[-1]) for l in lines] == [plain[t] for t in want], arg
    assert run(["--play-index", "40"])[0] != 0 and run(["--play-index", "30:11"])[0] != 0
    assert run(["--play-index", "3", "--step-back"])[0] != 0          # it goes alone
    # an MSVideo1 file: ScreenPressor only, non-zero
    frames, mkeys, _ = sg.msv1_clip(5, w, h, 6, p_mix=sg.msv1_p_mix(0.7, 40.0))
    mpath = tmp_path / "msv1.avi"
    mpath.write_bytes(avi.write_avi(w, h, frames, fourcc=b"CRAM", bpp=16, fps=15.0, key_flags=mkeys))
    rc, lines, err = run(["--play-index", "0"], mpath)
    assert rc != 0 and "ScreenPressor only" in err and not lines
