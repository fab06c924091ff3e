"""Playback from the MSVideo1 seek index (jsp_index_play / SeekIndex.Play / Manager.run_from_index / jsp_play --index-run) on an
MI355X.

Truth: what jsp_index_show writes into an identically poisoned buffer — the contract of jsp_index_play (include/jsplayer_amd.h):
dsts[k] ends exactly as Show(first + k * stride, adopt = 0) leaves it, data_pnt and verdict included — and, here and there, the twin
codec's Seek that Show itself is pinned to.  Everything is bit-exact.  Every destination is filled with a poison first, and one more
poisoned buffer that is not listed must stay poisoned."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import msv1_index_play_ref as ref
from jsplayer_amd import CodecError, MSVideo1_16bit, MSVideo1_8bit, ScreenPressor, player
from jsplayer_amd import _native as N
from jsplayer_amd import streamgen as sg
from msv1_range_clips import long_clip
from oracle_binding import OracleMSVideo1

pytestmark = pytest.mark.gpu

POISON = 0x5A5A5A5A
PARSE = "host"


@pytest.fixture(autouse=True, params=["host", "gpu"])
def parse_mode(request):
    """Every test runs with the block tables of the host parser and of the on-GPU parse."""
    global PARSE
    PARSE = request.param
    yield request.param
    PARSE = "host"


def dev_buf(n, fill=POISON):
    import torch
    return torch.full((n,), fill, dtype=torch.int32, device="cuda")


class Pool:
    """count + 1 poisoned buffers of npix ints cut from one allocation, each 16-byte aligned (`misalign`: that buffer starts one int
    later); the last one is never handed out."""

    def __init__(self, npix, count, misalign=()):
        self.npix, self.count = npix, count
        self.pitch = (npix + 4 + 3) // 4 * 4
        self.all = dev_buf(self.pitch * (count + 1))
        assert self.all.data_ptr() % 16 == 0
        self.off = [k * self.pitch + (1 if k in misalign else 0) for k in range(count + 1)]
        self.bufs = [self.all[o:o + npix] for o in self.off]

    def pictures(self):
        """(the buffers' content, everything else still poisoned)"""
        host = self.all.cpu().numpy()
        pics = [host[o:o + self.npix] for o in self.off[:self.count]]
        rest = np.ones(host.size, dtype=bool)
        for o in self.off[:self.count]:
            rest[o:o + self.npix] = False
        return pics, bool(np.all(host[rest] == np.int32(POISON)))


def make_gpu(bits, w, h, pal=None, lines=36, chunk=None):
    c = MSVideo1_16bit(w, h) if bits == 16 else MSVideo1_8bit(w, h, pal or b"")
    c.set_option("msv1_parse", PARSE)
    if chunk:
        c.set_option("msv1_seek_chunk_frames", str(chunk))
    c.Preinit(lines)
    return c


def sequential(gpu, frames, keys, lo, hi, pool):
    """Frames [lo, hi) through DecompressI / DecompressP into `pool`; [(adopted, significance)] of each."""
    out = []
    for i in range(lo, hi):
        prev = gpu.PreviousFrame()
        dst = next(b for b in pool if b is not prev)
        if keys[i]:
            assert gpu.DecompressI(frames[i], dst) == 0
            out.append((gpu.PreviousFrame() is dst, None))
        else:
            r = gpu.DecompressP(frames[i], dst)
            out.append((r.data_pnt is dst, r.significant_changes))
    return out


def mixed_clip(bits, w, h, seed=0):
    """A key frame, inter frames with skips, all-skip frames, early-outs, an 8-bit end marker, a truncated frame, key frames
    mid-range (the clip of test_seek_index_gpu)."""
    frames, keys, pal = sg.msv1_clip(600 + seed + bits, w, h, 14, bits=bits, p_mix=sg.msv1_p_mix(0.6, 5.0), key_every=6)
    nb = (w // 4) * (h // 4)
    allskip = b"".join(bytes([min(nb - k, 255), 0x84]) for k in range(0, nb, 255))
    out, ks = list(frames[:4]), list(keys[:4])
    out += [allskip, bytes([0x10, 0x84]), frames[4]]                 # all-skip; 16-bit early-out (short); a real frame
    ks += [False, False, keys[4]]
    full = frames[5] if not keys[5] else frames[4]
    out.append(full[: max(2, len(full) // 2)])                          # truncated
    ks.append(False)
    if bits == 8:
        out.append(full[:10] + b"\x00\x00" + full[12:])                 # end marker part-way
    else:
        out.append(full + b"\x07")                                      # odd trailing byte
    ks.append(False)
    out += list(frames[5:])
    ks += list(keys[5:])
    out.append(allskip)
    ks.append(False)
    return out, ks, pal


class Built:
    """A codec brought to frame `start` of a clip frame by frame, its index over the frames from there on, and what Show leaves of
    every frame in a poisoned buffer (worked out once per frame)."""

    def __init__(self, bits, w, h, pal, frames, keys, start=0, lines=36, chunk=None):
        self.bits, self.w, self.h, self.start = bits, w, h, start
        self.frames, self.keys, self.pal, self.lines, self.chunk = frames, keys, pal, lines, chunk
        self.gpu = make_gpu(bits, w, h, pal, lines, chunk)
        self.pool = [dev_buf(w * h) for _ in range(3)]
        sequential(self.gpu, frames, keys, 0, start, self.pool)
        self.prev = self.gpu.PreviousFrame()
        self.idx = self.gpu.BuildIndex(frames[start:], keys[start:])
        self.n = self.idx.frames
        self._shown = {}
        self._dst = dev_buf(w * h)

    def show(self, t):
        """(picture, data_pnt is dst, data_pnt is the previous frame of the build's time, verdict) of Show(t) into a poisoned buffer."""
        if t not in self._shown:
            self._dst.fill_(POISON)
            r = self.idx.Show(t, self._dst, adopt=False)
            self._shown[t] = (self._dst.cpu().numpy().copy(), r.data_pnt is self._dst,
                              self.prev is not None and r.data_pnt is self.prev, r.significant_changes)
        return self._shown[t]

    def check(self, first, n, stride=1, reverse=False, misalign=(), what=""):
        """One Play against n Shows; returns the pictures."""
        pool = Pool(self.w * self.h, n, misalign)
        bufs = pool.bufs[:n][::-1] if reverse else pool.bufs[:n]
        res = self.idx.Play(first, bufs, stride)
        pics, rest_poisoned = pool.pictures()
        pics = pics[::-1] if reverse else pics
        where = f"{self.bits}-bit {self.w}x{self.h} start={self.start} first={first} n={n} stride={stride} {what}({PARSE} parse)"
        assert rest_poisoned, where + ": something outside the listed buffers was written"
        for k in range(n):
            want = self.show(first + k * stride)
            assert np.array_equal(pics[k], want[0]), where + f": picture {k}"
            got = (res[k].data_pnt is bufs[k], self.prev is not None and res[k].data_pnt is self.prev, res[k].significant_changes)
            assert got == want[1:], where + f": data_pnt / verdict {k}"
        return pics

    def close(self):
        self.idx.close()
        self.gpu.StopAndClean()


def twin_seek(b, t):
    """The picture Seek(range[0..t]) writes on a fresh codec brought to the build-time state."""
    g = make_gpu(b.bits, b.w, b.h, b.pal, b.lines, b.chunk)
    sequential(g, b.frames, b.keys, 0, b.start, [dev_buf(b.w * b.h) for _ in range(3)])
    dst = dev_buf(b.w * b.h)
    s = b.start
    g.Seek(b.frames[s:s + t + 1], dst, b.keys[s:s + t + 1])
    out = dst.cpu().numpy()
    g.StopAndClean()
    return out


# ---- 1. every run against Show ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [16, 8])
@pytest.mark.parametrize("size", [(4, 4), (13, 9), (64, 48), (256, 144), (262, 26)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_every_run_matches_show(bits, size):
    w, h = size
    frames, keys, pal = mixed_clip(bits, w, h)
    for start in (0, 3):   # without and with a picture before the index
        b = Built(bits, w, h, pal, frames, keys, start)
        n = b.n
        for first in range(n):
            b.check(first, min(6, n - first))
        pics = b.check(0, n, what="all frames ")
        for t in range(0, n, 3):
            assert np.array_equal(pics[t], twin_seek(b, t)), f"{bits}-bit {w}x{h} start={start}: frame {t} against the twin's Seek"
        for stride in (2, 5, 13):
            for first in (0, 1):
                b.check(first, (n - 1 - first) // stride + 1, stride)
        b.check(1, min(7, n - 1), reverse=True, what="reversed ")
        b.check(0, (n + 1) // 2, 2, reverse=True, what="reversed ")
        b.check(2, min(6, n - 2), misalign=(3,), what="one misaligned ")
        b.check(0, n, misalign=(0,), what="one misaligned ")
        b.close()


# ---- 2. spans of several bitmap words ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [16, 8])
@pytest.mark.parametrize("chunk", [7, 50])
def test_multi_word_spans(bits, chunk):
    w, h = 64, 48
    frames, keys, pal, plan = long_clip(bits, w, h, seed=5, n=300)
    assert not plan["raises"]
    b = Built(bits, w, h, pal, frames, keys, 0, lines=plan["lines"], chunk=chunk)
    assert b.n == 300
    firsts = sorted({0} | {e + d for e in range(32, 300, 32) for d in (-1, 0, 1)})
    for stride in (31, 32, 33, 64, 100, 170):   # (170: a span passes SCAN = 4 words)
        for first in firsts:
            b.check(first, (299 - first) // stride + 1, stride)
    b.check(0, 300)                             # across the 8-bit end markers and the 16-bit truncated frames, every frame
    b.check(25, 120, 2)
    b.close()


def test_a_range_that_begins_with_frames_that_code_nothing():
    w, h = 64, 48
    frames, keys, pal, plan = long_clip(16, w, h, seed=5, n=300)
    start = 133   # the long idle stretch begins with an all-skip frame: Show writes nothing there, and the kernel gets a null entry
    b = Built(16, w, h, pal, frames, keys, start, lines=plan["lines"])
    assert ref.first_adopted(plan["coded"][start:]) > 0 and not b.show(0)[1] and b.show(0)[2]
    assert np.all(b.show(0)[0] == np.int32(POISON))
    b.check(0, 12)
    b.check(0, 5, 33)
    b.check(0, 1)
    b.close()


# ---- 3. the key frame cut short ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [16, 8])
@pytest.mark.parametrize("size", [(24, 16), (64, 48)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_the_key_frame_cut_short(bits, size):
    w, h = size
    frames, keys, pal, at = ref.cut_short_clip(bits, w, h)
    b = Built(bits, w, h, pal, frames, keys, 0)
    for first in range(b.n):
        for stride in (1, 2, 3):
            b.check(first, (b.n - 1 - first) // stride + 1, stride)
    pics = b.check(0, b.n)
    if bits == 8:   # the blocks the end marker cut off stay poisoned in the early destinations and are defined in the later ones
        assert np.all(ref.to_blocks(pics[0], w, h)[at:] == np.int32(POISON))
        assert np.any(ref.to_blocks(pics[4], w, h)[at:] == np.int32(POISON)) and np.any(ref.to_blocks(pics[4], w, h)[at:] != np.int32(POISON))
        assert not np.any(ref.to_blocks(pics[-1], w, h) == np.int32(POISON))
    else:           # (a 16-bit stream that ends early paints the blocks whose codes are missing)
        assert not np.any(ref.to_blocks(pics[0], w, h) == np.int32(POISON))
    b.close()


# ---- 4. segments --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [16, 8])
def test_segments_do_not_change_the_pictures(bits):
    w, h = 64, 48
    frames, keys, pal = mixed_clip(bits, w, h, seed=1)
    lframes, lkeys, lpal, plan = long_clip(bits, w, h, seed=5, n=300)
    for b, runs in ((Built(bits, w, h, pal, frames, keys, 3), [(0, None, 1), (1, 6, 2)]),
                    (Built(bits, w, h, lpal, lframes, lkeys, 0, lines=plan["lines"], chunk=50), [(31, 9, 31), (100, 64, 1), (3, 2, 170)])):
        for first, n, stride in runs:
            n = b.n - first if n is None else n
            b.gpu.set_option("msv1_index_play_segments", "auto")
            want = b.check(first, n, stride, what="segments=auto ")
            for segs in (1, 2, 3, n):
                b.gpu.set_option("msv1_index_play_segments", str(segs))
                got = b.check(first, n, stride, what=f"segments={segs} ")
                assert all(np.array_equal(g, x) for g, x in zip(got, want))
        for bad in ("0", "65", "-1", "many", ""):
            with pytest.raises(CodecError):
                b.gpu.set_option("msv1_index_play_segments", bad)
        b.close()


# ---- 5. adopt -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [16, 8])
def test_adopt_leaves_the_codec_as_show_with_adopt_does(bits):
    w, h = 64, 48
    frames, keys, pal = mixed_clip(bits, w, h, seed=2)
    total = len(frames)
    cx, cy = (w // 4) * 4, (h // 4) * 4
    for first, n, stride in ((0, 7, 1), (3, 5, 2), (4, 4, 1)):   # (frames 4 and 5 code nothing: an all-skip and an early-out)
        for k in (0, n // 2, n - 1, None):
            t = first + (k or 0) * stride
            a = Built(bits, w, h, pal, frames, keys, 0)
            tw = Built(bits, w, h, pal, frames, keys, 0)
            pool = Pool(w * h, n)
            res = a.idx.Play(first, pool.bufs[:n], stride, adopt=k)
            where = f"{bits}-bit first={first} n={n} stride={stride} adopt={k} ({PARSE} parse)"
            if k is None:   # the codec is untouched: sequential decoding continues where it stood (nothing decoded yet)
                assert a.gpu.PreviousFrame() is None
                assert a.gpu.counter("msv1_block_changes") == tw.gpu.counter("msv1_block_changes")
                lo = 0
            else:
                dst = dev_buf(w * h)
                rt = tw.idx.Show(t, dst, adopt=True)
                assert (a.gpu.PreviousFrame() is pool.bufs[k]) == (tw.gpu.PreviousFrame() is dst), where
                assert (a.gpu.PreviousFrame() is None) == (tw.gpu.PreviousFrame() is None), where
                assert (res[k].data_pnt is pool.bufs[k]) == (rt.data_pnt is dst) and res[k].significant_changes == rt.significant_changes
                if a.gpu.PreviousFrame() is not None:
                    assert np.array_equal(a.gpu.PreviousFrame().cpu().numpy(), tw.gpu.PreviousFrame().cpu().numpy()), where
                assert a.gpu.counter("msv1_block_changes") == tw.gpu.counter("msv1_block_changes"), where
                assert a.gpu.KeyFrameDiffers() is None
                tw.pool.append(dst)
                lo = t + 1
            apool = a.pool + [dev_buf(w * h)] + ([pool.bufs[k]] if k is not None else [])
            for i in range(lo, min(lo + 3, total)):
                ra, rb = sequential(a.gpu, frames, keys, i, i + 1, apool), sequential(tw.gpu, frames, keys, i, i + 1, tw.pool)
                assert ra == rb, where + f": frame {i}"
                assert a.gpu.counter("msv1_block_changes") == tw.gpu.counter("msv1_block_changes"), where + f": frame {i}"
                if a.gpu.PreviousFrame() is not None:
                    pa = a.gpu.PreviousFrame().cpu().numpy().reshape(h, w)[:cy, :cx]
                    pb = tw.gpu.PreviousFrame().cpu().numpy().reshape(h, w)[:cy, :cx]
                    assert np.array_equal(pa, pb), where + f": frame {i}"
            a.close()
            tw.close()


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals_change_nothing():
    w, h = 64, 48
    frames, keys, _ = sg.msv1_clip(660, w, h, 8, p_mix=sg.msv1_p_mix(0.7, 5.0), key_every=8)
    lib = N.lib()
    b = Built(16, w, h, None, frames, keys, 2)
    a, idx, prev = b.gpu, b.idx, b.prev
    prev_pic = prev.cpu().numpy().copy()
    rows = a.counter("msv1_block_changes")
    pool = Pool(w * h, 4)
    host = np.full(w * h, POISON, dtype=np.int32)
    sp = ScreenPressor(w, h, 24)
    other = make_gpu(16, w, h)
    foreign = other.BuildIndex(frames, keys)
    outs, sig = (C.c_void_p * 8)(), (C.c_int * 8)(*([7] * 8))

    def ptrs(*bufs):
        return (C.c_void_p * max(len(bufs), 1))(*[None if x is None else x.ctypes.data if isinstance(x, np.ndarray) else x.data_ptr() for x in bufs])

    def refused(c, i, first, n, stride, dsts, adopt_k, starts="index_play:"):
        rc = lib.jsp_index_play(c, i, first, n, stride, dsts, adopt_k, outs, sig)
        err = N.last_error()
        assert rc != 0 and err.startswith(starts), (err, first, n, stride, adopt_k)
        assert list(sig) == [7] * 8 and not any(outs), "a refused call wrote its results"
        assert a.PreviousFrame() is prev and lib.jsp_previous_frame(a._h) == prev.data_ptr()
        assert a.counter("msv1_block_changes") == rows

    p = pool.bufs
    four = ptrs(p[0], p[1], p[2], p[3])
    refused(None, idx._h, 0, 4, 1, four, -1)
    refused(a._h, None, 0, 4, 1, four, -1)
    refused(a._h, idx._h, 0, 4, 1, None, -1)
    refused(a._h, idx._h, 0, 4, 1, ptrs(p[0], None, p[2], p[3]), -1)
    refused(sp._h, idx._h, 0, 4, 1, four, -1, starts="index: MSVideo1 only")
    refused(a._h, foreign._h, 0, 4, 1, four, -1)
    for n in (0, -1, 4097):
        refused(a._h, idx._h, 0, n, 1, four, -1)
    for stride in (0, -3):
        refused(a._h, idx._h, 0, 4, stride, four, -1)
    refused(a._h, idx._h, -1, 4, 1, four, -1)
    refused(a._h, idx._h, idx.frames - 3, 4, 1, four, -1)
    refused(a._h, idx._h, idx.frames, 1, 1, four, -1)
    refused(a._h, idx._h, 2, 3, 0x7FFFFFFF, four, -1)        # (2 + 2 * (2^31 - 1) wraps to 0 in 32 bits)
    refused(a._h, idx._h, 0, 4096, 0x7FFFFFFF, four, -1)     # (refused before dsts is read past its four entries)
    for adopt_k in (-2, 4, 100):
        refused(a._h, idx._h, 0, 4, 1, four, adopt_k)
    refused(a._h, idx._h, 0, 4, 1, ptrs(p[0], host, p[2], p[3]), -1)
    refused(a._h, idx._h, 0, 4, 1, ptrs(p[0], p[1], prev, p[3]), 1)
    refused(a._h, idx._h, 0, 4, 1, ptrs(p[0], p[1], p[2], p[0]), -1)
    spare = next(x for x in b.pool if x is not prev)
    spare_pic = spare.cpu().numpy().copy()
    ticket = a.DecompressP_async(frames[2], spare)
    rc = lib.jsp_index_play(a._h, idx._h, 0, 4, 1, four, -1, outs, sig)
    assert rc != 0 and N.last_error().startswith("index_play:") and "in flight" in N.last_error()
    a.wait(ticket)
    del spare_pic
    # a codec in host-pointer mode (its index was built before it decoded into host memory)
    hostc = make_gpu(16, w, h)
    hidx = hostc.BuildIndex(frames, keys)
    assert hostc.DecompressI(frames[0], np.zeros(w * h, dtype=np.int32)) == 0
    rc = lib.jsp_index_play(hostc._h, hidx._h, 0, 4, 1, four, -1, outs, sig)
    assert rc != 0 and N.last_error().startswith("index_play:") and "host-pointer" in N.last_error()
    pics, rest = pool.pictures()
    assert rest and all(np.all(x == np.int32(POISON)) for x in pics) and np.all(host == np.int32(POISON))
    assert list(sig) == [7] * 8 and not any(outs)
    # ... and the call that is not refused works after all that
    b.check(0, 4)
    hidx.close()
    hostc.StopAndClean()
    foreign.close()
    other.StopAndClean()
    sp.StopAndClean()
    b.close()
    assert np.array_equal(prev_pic, prev.cpu().numpy())


# ---- 7. jsp_index_info ------------------------------------------------------------------------------------------------------------------
def test_index_info_grows_only_at_the_first_play_by_the_table_bytes():
    w, h = 64, 48
    frames, keys, pal = mixed_clip(16, w, h)
    b = Built(16, w, h, pal, frames, keys, 0)
    lib = N.lib()

    def info():
        n, dev, host = C.c_int(0), C.c_uint64(0), C.c_uint64(0)
        assert lib.jsp_index_info(b.idx._h, C.byref(n), C.byref(dev), C.byref(host)) == 0
        return dev.value, host.value

    d0, h0 = info()
    b.show(3)
    assert info() == (d0, h0), "Show holds nothing"
    b.check(0, 6)
    d1, h1 = info()
    table = 6 * C.sizeof(C.c_void_p)
    for grown in (d1 - d0, h1 - h0):        # (a grown buffer takes a quarter more than asked and 256 bytes)
        assert table <= grown <= table + table // 4 + 256
    assert (b.idx.device_bytes, b.idx.host_bytes) == (d1, h1)
    b.check(2, 6, 2)
    b.check(5, 1)
    assert info() == (d1, h1), "a run no longer than the first grows nothing"
    b.check(0, b.n)
    d2, h2 = info()
    assert d2 >= d1 and h2 >= h1
    b.close()


# ---- 8. Manager end to end ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [16, 8])
def test_manager_run_from_index(bits):
    from jsplayer_amd.avi import CODEC_MSVC16, CODEC_MSVC8, VideoInfo
    w, h = 64, 48
    frames, keys, pal = sg.msv1_clip(670 + bits, w, h, 30, bits=bits, p_mix=sg.msv1_p_mix(0.4, 4.0), key_every=10)
    o = OracleMSVideo1(bits, w, h, pal)
    o.Preinit(player.INSIGNIFICANT_LINES)
    pics, buf = [], [np.zeros(w * h, dtype=np.int32) for _ in range(3)]
    for i, f in enumerate(frames):
        dst = next(x for x in buf if x is not o.PreviousFrame())
        if keys[i]:
            o.DecompressI(f, dst)
        else:
            o.DecompressP(f, dst)
        pics.append(o.PreviousFrame().copy())
    vi = VideoInfo(X=w, Y=h, bpp=bits, fps=15.0, nframes=len(frames), codec=CODEC_MSVC16 if bits == 16 else CODEC_MSVC8,
                   palette=pal, riff_size=0)
    dec = make_gpu(bits, w, h, pal)
    mgr = player.Manager(vi, dec, lambda n: dev_buf(n, 0))
    idx = dec.BuildIndex(frames, keys)
    mgr.attach_index(idx, 0)
    last = len(frames) - 1
    seen = []

    def on_frame(d, buffer):
        seen.append(d.index)
        assert np.array_equal(buffer.cpu().numpy(), pics[d.index]), f"frame {d.index}"

    out = mgr.run_from_index(2, 20, on_frame=on_frame, key_flags=keys)            # forward: three batches
    assert seen == list(range(2, 22)) and mgr.next_frame_to_decode == 22
    assert [d.significant_changes for d in out] == [None if keys[d.index] else idx.significance[d.index] for d in out]
    seen.clear()
    mgr.run_from_index(last, None, reverse=True, on_frame=on_frame, key_flags=keys)   # reverse play to frame 0
    assert seen == list(range(last, -1, -1)) and mgr.next_frame_to_decode == 1
    assert np.array_equal(dec.PreviousFrame().cpu().numpy(), pics[0])
    seen.clear()
    mgr.run_from_index(1, None, 4, on_frame=on_frame, key_flags=keys)              # fast-forward
    assert seen == list(range(1, len(frames), 4))
    seen.clear()
    mgr.run_from_index(17, 5, 3, reverse=True, on_frame=on_frame, key_flags=keys)
    assert seen == [17, 14, 11, 8, 5] and mgr.next_frame_to_decode == 6 and mgr.frame_of_interest == 5
    # and the play goes on from the frame adopted as after a sequential decode
    for i in range(6, 12):
        d = mgr.worker(frames[i], i, None, keys[i])
        assert np.array_equal(mgr.buffers[d.buffer_index].cpu().numpy(), pics[i]), f"frame {i} after the run"
    idx.close()
    dec.StopAndClean()


# ---- 9. jsp_play --index-run -----------------------------------------------------------------------------------------------------------
def test_jsp_play_index_run_matches_the_plain_run(tmp_path, parse_mode):
    if parse_mode != "host":
        return   # (the example takes the codec's default parse; one run of it is enough)
    from jsplayer_amd import avi
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "examples", "jsp_play")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-s", "-C", os.path.join(root, "examples")])
    w, h = 320, 240
    frames, keys, _ = sg.msv1_clip(97, w, h, 40, p_mix=sg.msv1_p_mix(0.7, 6.0), key_every=16)
    path = tmp_path / "clip.avi"
    path.write_bytes(avi.write_avi(w, h, frames, fourcc=b"CRAM", bpp=16, fps=15.0, key_flags=keys))

    def run(extra, target=path):
        res = subprocess.run([exe, str(target)] + extra, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
        return res.returncode, [l.split() for l in res.stdout.decode().splitlines() if l and l[0].isdigit()], res.stderr.decode()

    rc, lines, err = run([])
    assert rc == 0, err
    plain = {int(l[0]): (int(l[0]), l[1], int(l[3]), l[-1]) for l in lines}
    assert len(plain) == 40
    for arg, want in (("0", range(40)), ("3:20", range(3, 23)), ("1:6:7", range(1, 40, 7)), ("39", [39])):
        rc, lines, err = run(["--index-run", arg])
        assert rc == 0, err
        assert [(int(l[0]), l[1], int(l[2]), l[-1]) for l in lines] == [plain[t] for t in want], arg
    for arg in ("40", "0:41", "3:10:5", "-1"):                       # past the end
        rc, lines, err = run(["--index-run", arg])
        assert rc != 0 and not lines, arg
    assert run(["--index-run", "3", "--step-back"])[0] != 0          # it goes alone
    assert run(["--index-run", "3", "--seek", "5"])[0] != 0
    chunks, skeys, _ = sg.sp_clip(98, w, h, 6, bpp=24, version=4, key_every=16)
    spath = tmp_path / "sp.avi"
    spath.write_bytes(avi.write_avi(w, h, chunks, fourcc=b"SCPR", bpp=24, fps=15.0, key_flags=skeys))
    rc, lines, err = run(["--index-run", "0"], spath)
    assert rc != 0 and "MSVideo1 only" in err and not lines
