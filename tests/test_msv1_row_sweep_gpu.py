"""The MSVideo1 range calls (BuildIndex / SeekIndex.Show / Play / Present, Seek, FindChange) on the row sweeps of
tests/msv1_row_sweep_clips.py, against the oracle, on an MI355X: pictures wider than a wave, a workgroup and a row word, rows cut by
every wave seam, and the pixels no block covers told apart from each other.

Truth in every case: OracleMSVideo1 stepped frame by frame with its buffers painted (painted_truth) — the WHOLE picture, data_pnt,
significance, the per-row block_changes a sequential decode leaves.  Destinations are filled with the poison; the pool buffers —
and so the picture before a range — carry the paint on the pixels no block covers: a range call with a picture before it must bring
exactly that paint over, and one without must leave the destination's poison there.  Everything is bit-exact."""
import functools

import numpy as np
import pytest

import msv1_range_clips as R
import msv1_row_sweep_clips as S
from oracle_binding import orc_display_convert

pytestmark = pytest.mark.gpu

POISON = R.POISON
PARSE = "host"
IDS = lambda s: f"{s[0]}x{s[1]}"
CHUNKS = [None, 5]


@pytest.fixture(autouse=True, params=["host", "gpu"])
def parse_mode(request):
    """Every test runs with the block tables of the host parser and of the on-GPU parse."""
    global PARSE
    PARSE = request.param
    yield request.param
    PARSE = "host"


@functools.lru_cache(maxsize=None)
def clip(bits, w, h):
    frames, keys, marks, stops = S.sweep(bits, w, h)
    pal, lines = R.palette(bits), R.straddle_lines(h)
    truth = S.painted_truth(bits, w, h, pal, frames, keys, lines)
    S.check_census(truth, marks, stops, w // 4, h // 4, bits)
    plan = R.make_plan(bits, w, h, frames, keys, lines)
    return frames, keys, marks, stops, pal, lines, truth, plan


def mid(frames):
    """An inter frame inside the clip: a range that starts there has a painted picture before it."""
    return min(2, len(frames) - 1)


def targets(marks, stops):
    return sorted([f for f, _ in marks] + [f for f, _, _ in stops])


def painted_pool(w, h, count=3, misalign=False):
    import torch
    out = []
    for k in range(count):
        buf = R.dev_buf(w * h, misalign=misalign)
        buf.copy_(torch.from_numpy(S.paint(w, h, k)))
        out.append(buf)
    return out


def want_picture(truth, i, w, h, painted):
    return truth[i][0] if painted else S.unpainted(truth[i][0], w, h)


def same(got, want, w, h, where):
    got = got.cpu().numpy() if hasattr(got, "cpu") else got
    assert np.array_equal(got, want), f"{where}: {S.first_difference(got, want, w, h)}"


def play(gpu, frames, keys, lo, hi, pool, truth=None, painted=True, where=""):
    """Frames [lo, hi) through DecompressI / DecompressP into `pool`, each destination first copied from the picture before it (as
    truth_run does); with truth: each one's significance, WHOLE picture and block_changes against the oracle."""
    w, h = gpu.X, gpu.Y
    for i in range(lo, hi):
        prev = gpu.PreviousFrame()
        dst = next(b for b in pool if b is not prev)
        if prev is not None:
            dst.copy_(prev)
        if keys[i]:
            assert gpu.DecompressI(frames[i], dst) == 0
        else:
            r = gpu.DecompressP(frames[i], dst)
            if truth is not None:
                assert r.significant_changes == truth[i][1], f"{where}: frame {i} played on: significance"
        if truth is not None:
            same(gpu.PreviousFrame(), want_picture(truth, i, w, h, painted), w, h, f"{where}: frame {i} played on: picture")
            got = gpu.counter("msv1_block_changes")
            assert got == truth[i][2], f"{where}: frame {i} played on: block_changes {got:#x}, the oracle's {truth[i][2]:#x}"


def started(bits, w, h, frames, keys, pal, lines, chunk, start, misalign=False):
    """A codec brought to frame `start` frame by frame in a painted pool."""
    gpu = R.make_gpu(bits, w, h, pal, lines, chunk, PARSE)
    pool = painted_pool(w, h, misalign=misalign)
    play(gpu, frames, keys, 0, start, pool)
    return gpu, pool


# ---- index: every t ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chunk", CHUNKS, ids=lambda c: f"chunk{c}")
@pytest.mark.parametrize("size", S.SIZES, ids=IDS)
@pytest.mark.parametrize("bits", [16, 8])
def test_index_every_t_whole_buffer(bits, size, chunk):
    w, h = size
    frames, keys, marks, stops, pal, lines, truth, plan = clip(bits, w, h)
    n = len(frames)
    unc = S.uncovered(w, h)
    dst = R.dev_buf(w * h)
    for start in (0, mid(frames)):
        gpu, pool = started(bits, w, h, frames, keys, pal, lines, chunk, start)
        old = gpu.PreviousFrame()
        idx = gpu.BuildIndex(frames[start:], keys[start:], key_row=lines)
        where = f"{bits}-bit {w}x{h} chunk={chunk} index from {start} ({PARSE} parse)"
        assert idx.frames == n - start, where
        assert idx.significance == [truth[k][1] for k in range(start, n)], where + ": significance"
        for t in range(n - start):
            dst.fill_(POISON)
            r = idx.Show(t, dst, adopt=False)
            assert r.data_pnt is dst, f"{where} t={t}: data_pnt"     # (every frame of a sweep codes a block)
            assert r.significant_changes == (False if keys[start + t] else truth[start + t][1]), f"{where} t={t}: verdict"
            got = dst.cpu().numpy()
            same(got, want_picture(truth, start + t, w, h, start > 0), w, h, f"{where} t={t} (frame {start + t})")
            if start > 0:   # (said once more, on its own: the picture before the range, pixel for pixel)
                assert np.array_equal(got[unc], S.paint(w, h, 0)[unc]), f"{where} t={t}: the paint of the picture before the range"
            else:
                assert np.all(got[unc] == np.int32(POISON)), f"{where} t={t}: no picture before the range, yet an uncovered pixel was written"
        assert gpu.PreviousFrame() is old, where
        idx.close()
        gpu.StopAndClean()


# ---- index: adopt, then play on ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chunk", CHUNKS, ids=lambda c: f"chunk{c}")
@pytest.mark.parametrize("size", S.SIZES, ids=IDS)
@pytest.mark.parametrize("bits", [16, 8])
def test_adopt_every_mark_and_stop_then_play_on(bits, size, chunk):
    """Show(t, adopt=True) at every MARK and STOP frame — of the index from frame 0 (the MARK of block 0 among them) and of the one
    from inside the clip: the per-row block_changes built from rows[] / stop[] of msv1_coded_bitmap_kernel are the oracle's, and the
    next two frames decode as after a sequential decode."""
    w, h = size
    frames, keys, marks, stops, pal, lines, truth, plan = clip(bits, w, h)
    n = len(frames)
    assert targets(marks, stops)[0] == 1 and marks[0] == (1, 0)
    for start in (0, mid(frames)):
        gpu, pool = started(bits, w, h, frames, keys, pal, lines, chunk, start)
        old = gpu.PreviousFrame()
        idx = gpu.BuildIndex(frames[start:], keys[start:], key_row=lines)
        pool = [b for b in pool if b is not old] + painted_pool(w, h, 2)   # (the index reads the picture before it where it lies)
        for f in targets(marks, stops):
            if f < start:
                continue
            where = f"{bits}-bit {w}x{h} chunk={chunk} index from {start}, show({f - start}) = frame {f}, adopted ({PARSE} parse)"
            dst = next(b for b in pool if b is not gpu.PreviousFrame())
            dst.fill_(POISON)
            r = idx.Show(f - start, dst, adopt=True)
            assert r.data_pnt is dst and gpu.PreviousFrame() is dst, where
            same(dst, want_picture(truth, f, w, h, start > 0), w, h, where)
            got = gpu.counter("msv1_block_changes")
            assert got == truth[f][2], f"{where}: block_changes {got:#x}, the oracle's {truth[f][2]:#x}"
            play(gpu, frames, keys, f + 1, min(n, f + 3), pool, truth, start > 0, where)
        idx.close()
        gpu.StopAndClean()


# ---- seek ----------------------------------------------------------------------------------------------------------------------
def check_seek(bits, w, h, chunk, start, target, misalign=False):
    frames, keys, marks, stops, pal, lines, truth, plan = clip(bits, w, h)
    gpu, pool = started(bits, w, h, frames, keys, pal, lines, chunk, start, misalign)
    dst = R.dev_buf(w * h, misalign=misalign)
    res = gpu.Seek(frames[start:target + 1], dst, keys[start:target + 1])
    where = f"{bits}-bit {w}x{h} chunk={chunk} seek {start}..{target} misalign={misalign} ({PARSE} parse)"
    assert res.data_pnt is dst and gpu.PreviousFrame() is dst, where
    same(dst, want_picture(truth, target, w, h, start > 0), w, h, where)
    assert res.significant_changes == (False if keys[target] else truth[target][1]), where + ": significant_changes"
    got = gpu.counter("msv1_block_changes")
    assert got == truth[target][2], f"{where}: block_changes {got:#x}, the oracle's {truth[target][2]:#x}"
    pool = [p for p in pool if p is not gpu.PreviousFrame()] + [dst]
    play(gpu, frames, keys, target + 1, min(len(frames), target + 3), pool, truth, start > 0, where)
    gpu.StopAndClean()


@pytest.mark.parametrize("chunk", CHUNKS, ids=lambda c: f"chunk{c}")
@pytest.mark.parametrize("size", S.SIZES, ids=IDS)
@pytest.mark.parametrize("bits", [16, 8])
def test_seek_to_every_mark_and_stop(bits, size, chunk):
    w, h = size
    frames, keys, marks, stops, pal, lines, truth, plan = clip(bits, w, h)
    ts = targets(marks, stops)
    for start in (0, mid(frames)):   # (frame 0 is the nearest key frame of every frame)
        for t in ts:
            if t >= start:
                check_seek(bits, w, h, chunk, start, t)
    if chunk is None:               # once into a destination that is not 16-byte aligned, from a picture that is not either
        check_seek(bits, w, h, chunk, mid(frames), ts[-1], misalign=True)


# ---- find change ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chunk", CHUNKS, ids=lambda c: f"chunk{c}")
@pytest.mark.parametrize("size", S.SIZES, ids=IDS)
@pytest.mark.parametrize("bits", [16, 8])
def test_find_change_walk(bits, size, chunk):
    """walk(): every frame changes one block (or all), so where FindChange lands depends on the row of that one block against the
    straddled `lines`.  (walk() decodes into poisoned buffers, so on this path the pixels no block covers are poison on both sides: what
    FindChange copies onto them is not told apart here — Seek, Show and Play above are the painted paths.)"""
    w, h = size
    frames, keys, marks, stops, pal, lines, truth, plan = clip(bits, w, h)
    assert lines == R.straddle_lines(h)
    tr = [(S.unpainted(p, w, h), s) for p, s, _ in truth]
    for step in (False, True):
        R.walk(bits, w, h, pal, frames, keys, lines=lines, chunk=chunk, step=step, parse=PARSE, truth=tr)


# ---- play ----------------------------------------------------------------------------------------------------------------------
class Sheet:
    """count + 1 poisoned buffers of npix ints cut from one allocation, each 16-byte aligned; the last one is never handed out."""

    def __init__(self, npix, count):
        self.npix, self.count = npix, count
        self.pitch = (npix + 4 + 3) // 4 * 4
        self.all = R.dev_buf(self.pitch * (count + 1))
        self.bufs = [self.all[k * self.pitch:k * self.pitch + npix] for k in range(count)]

    def pictures(self):
        """(the buffers' content, everything else still poisoned)"""
        host = self.all.cpu().numpy()
        rest = np.ones(host.size, dtype=bool)
        for k in range(self.count):
            rest[k * self.pitch:k * self.pitch + self.npix] = False
        return [host[k * self.pitch:k * self.pitch + self.npix] for k in range(self.count)], bool(np.all(host[rest] == np.int32(POISON)))


@pytest.mark.parametrize("chunk", CHUNKS, ids=lambda c: f"chunk{c}")
@pytest.mark.parametrize("size", S.SIZES, ids=IDS)
@pytest.mark.parametrize("bits", [16, 8])
def test_play_whole_index_and_stride_3(bits, size, chunk):
    """One Play over the whole index and one with stride 3, segments auto and 2: every destination is the oracle's whole picture.
    The index from inside the clip begins with an all-skip frame put there: Show and Play write nothing for it."""
    w, h = size
    frames, keys, marks, stops, pal, lines, truth, plan = clip(bits, w, h)
    for start in (0, mid(frames)):
        fr, ks, tr = frames, keys, truth
        if start:
            fr, ks = S.with_idle_frame(bits, w, h, frames, keys, start)
            tr = S.painted_truth(bits, w, h, pal, fr, ks, lines)
            assert not R.coded_blocks(bits, w // 4, h // 4, fr[start])[0].any() and not tr[start][1]
        n = len(fr) - start
        gpu, pool = started(bits, w, h, fr, ks, pal, lines, chunk, start)
        old = gpu.PreviousFrame()
        idx = gpu.BuildIndex(fr[start:], ks[start:], key_row=lines)
        first_adopted = 1 if start else 0
        for segs in ("auto", "2"):
            gpu.set_option("msv1_index_play_segments", segs)
            for first, stride in ((0, 1), (0, 3), (1, 3)):
                if first >= n:
                    continue
                count = (n - 1 - first) // stride + 1
                sheet = Sheet(w * h, count)
                res = idx.Play(first, sheet.bufs, stride)
                pics, rest_poisoned = sheet.pictures()
                where = f"{bits}-bit {w}x{h} chunk={chunk} index from {start}, play first={first} stride={stride} segments={segs} ({PARSE} parse)"
                assert rest_poisoned, where + ": something outside the listed buffers was written"
                for k in range(count):
                    t = first + k * stride
                    if t < first_adopted:
                        assert res[k].data_pnt is old and np.all(pics[k] == np.int32(POISON)), f"{where}: t={t} codes nothing, its buffer stays untouched"
                    else:
                        assert res[k].data_pnt is sheet.bufs[k], f"{where} t={t}: data_pnt"
                        same(pics[k], want_picture(tr, start + t, w, h, start > 0), w, h, f"{where} t={t} (buffer {k})")
                    assert res[k].significant_changes == (False if ks[start + t] else tr[start + t][1]), f"{where} t={t}: verdict"
        assert gpu.PreviousFrame() is old
        idx.close()
        gpu.StopAndClean()


# ---- present -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [16, 8])
def test_present_shows_the_whole_picture(bits):
    """IndexPresent at k = 1 with integral offsets is display_convert of the frame's WHOLE picture, flipped: the 572 pixels no block
    covers of 262x26 come from the painted picture before the index."""
    w, h = 262, 26
    frames, keys, marks, stops, pal, lines, truth, plan = clip(bits, w, h)
    start = mid(frames)
    gpu, pool = started(bits, w, h, frames, keys, pal, lines, None, start)
    idx = gpu.BuildIndex(frames[start:], keys[start:], key_row=lines)
    for f in (stops[0][0], stops[len(stops) // 2][0], marks[-1][0]):
        for mode in (0, 1):
            where = f"{bits}-bit {w}x{h} present of frame {f} mode {mode} ({PARSE} parse)"
            got = idx.Present([f - start], w, h, 1.0, 0.0, 0.0, mode=mode).cpu().numpy().reshape(-1)
            want = orc_display_convert(truth[f][0], w, h, mode, True)
            flipped = lambda a: a.reshape(h, w)[::-1].reshape(-1)   # (failure messages name the pixel of the picture, not of the window)
            same(flipped(got), flipped(want), w, h, where)
    idx.close()
    gpu.StopAndClean()


# ---- the flags behind an end marker, frames in flight ---------------------------------------------------------------------------
@pytest.mark.parametrize("depth", [1, 2, 4])
def test_block_changes_behind_end_markers_with_frames_in_flight(depth):
    """8-bit 68x16: the rows past an end marker keep the flags of the frame before, and with the on-GPU parse that frame's bytes, where
    its staging left them, are all the codec keeps of them.  Frame 1 ends on the first block of row 3 (the host parser's last word on
    the flags: row 3 is 0); then every block changes and four frames end on a marker in rows 2, 1, 0 and 2 — submitted with `depth`
    frames in flight, the oldest waited for when the ring is full.  Every marker frame is vetoed by the GPU and re-run by the host
    parser, which must rebuild the flags from the frame before it: at depth 1 that frame's staging object is the one being staged, at
    depth 4 it has a new tenant before the veto is read.  Row 3 is never walked again, so it must hold the every-block frame's 1 to
    the end."""
    bits, w, h = 8, 68, 16
    frames, keys, marks, stops, pal, lines, truth, plan = clip(bits, w, h)
    cut = {m: frames[f] for f, m, _ in stops}
    every = frames[stops[0][0] - 1]
    seq = [frames[0], cut[51], every, cut[50], cut[33], cut[16], cut[50], every]
    ks = [True] + [False] * (len(seq) - 1)
    tr = S.painted_truth(bits, w, h, pal, seq, ks, lines)
    assert [t[2] for t in tr] == [0xF, 0x2, 0xF, 0xC, 0xE, 0xF, 0xC, 0xF]
    gpu = R.make_gpu(bits, w, h, pal, lines, None, PARSE)
    gpu.set_option("async_depth", str(depth))
    where = f"8-bit 68x16, {depth} frames in flight ({PARSE} parse)"
    pool = painted_pool(w, h, 8)
    play(gpu, seq, ks, 0, 2, pool[:3])
    got = gpu.counter("msv1_block_changes")
    assert got == tr[1][2], f"{where}: frame 1: block_changes {got:#x}, the oracle's {tr[1][2]:#x}"
    free = [b for b in pool if b is not gpu.PreviousFrame()]
    inflight = []

    def collect():
        k, ticket = inflight.pop(0)
        assert gpu.wait(ticket).significant_changes == tr[k][1], f"{where}: frame {k}"

    for k in range(2, 7):
        if len(inflight) == depth:
            collect()
        inflight.append((k, gpu.DecompressP_async(seq[k], free[k - 2])))
    while inflight:
        collect()
    assert gpu.PreviousFrame() is free[4], where
    got = gpu.counter("msv1_block_changes")
    assert got == tr[6][2], f"{where}: block_changes {got:#x}, the oracle's {tr[6][2]:#x}"
    play(gpu, seq, ks, 7, 8, free[5:7], tr, True, where)
    gpu.StopAndClean()
