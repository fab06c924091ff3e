"""The MSVideo1 range calls (Seek, FindChange, BuildIndex / SeekIndex.Show) on long clips, against the oracle, on an MI355X.

The clips (msv1_range_clips.long_clip) reach what only a long clip reaches in msv1_seek_kernels.hip: the show kernel's backward
walk over bitmap words, coded-bitmap words shared by two chunks, change-scan walk lists of many segments, last writers hundreds
of frames back.  Truth in every case: OracleMSVideo1 stepped frame by frame (truth_run) — picture, data_pnt, significance,
the per-row block_changes a sequential decode leaves."""
import functools

import numpy as np
import pytest

import msv1_range_clips as R
from jsplayer_amd import player

pytestmark = pytest.mark.gpu

POISON = R.POISON
PARSE = "host"
SIZES = [(4, 4), (13, 9), (37, 23), (64, 48)]
MID = R.LATE_FROM   # an inter frame mid-clip: an index / seek range that starts there has a picture before it


@pytest.fixture(autouse=True, params=["host", "gpu"])
def parse_mode(request):
    """Every test runs with the block tables of the host parser and of the on-GPU parse."""
    global PARSE
    PARSE = request.param
    yield request.param
    PARSE = "host"


@functools.lru_cache(maxsize=None)
def clip(bits, w, h):
    frames, keys, pal, plan = R.long_clip(bits, w, h, seed=w * h + bits)
    truth = R.truth_run(bits, w, h, pal, frames, keys, plan["lines"], key_row=plan["lines"], rows=True)
    assert all(x is not None for x in truth)
    return frames, keys, pal, plan, truth


def make(bits, w, h, pal, lines, chunk=None):
    return R.make_gpu(bits, w, h, pal, lines, chunk, PARSE)


def play(gpu, frames, keys, lo, hi, pool, truth=None, where=""):
    """Frames [lo, hi) through DecompressI / DecompressP into `pool`, each destination first copied from the picture before it
    (as truth_run does: what an 8-bit end marker leaves alone is the picture before); with truth: each one's significance,
    picture (block-covered part) and block_changes against the oracle."""
    w, h = gpu.X, gpu.Y
    cx, cy = (w // 4) * 4, (h // 4) * 4
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
                assert r.significant_changes == truth[i][1], f"{where}: frame {i} significance"
        if truth is not None:
            pic = gpu.PreviousFrame().cpu().numpy().reshape(h, w)[:cy, :cx]
            assert np.array_equal(pic, truth[i][0].reshape(h, w)[:cy, :cx]), f"{where}: frame {i} picture"
            assert gpu.counter("msv1_block_changes") == truth[i][2], f"{where}: frame {i} block_changes"


# ---- index: every t ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chunk", [None, 5, 31, 33], ids=lambda c: f"chunk{c}")
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("bits", [16, 8])
def test_index_every_t_against_the_oracle(bits, size, chunk):
    w, h = size
    frames, keys, pal, plan, truth = clip(bits, w, h)
    n, lines = plan["n"], plan["lines"]
    ad = R.adopted(plan)
    dst = R.dev_buf(w * h)
    for start in (0, MID):
        gpu = make(bits, w, h, pal, lines, chunk)
        pool = [R.dev_buf(w * h) for _ in range(3)]
        play(gpu, frames, keys, 0, start, pool)
        old = gpu.PreviousFrame()
        idx = gpu.BuildIndex(frames[start:], keys[start:], key_row=lines)
        where = f"{bits}-bit {w}x{h} chunk={chunk} start={start} ({PARSE} parse)"
        assert idx.frames == n - start
        assert idx.significance == [truth[k][1] for k in range(start, n)], where
        first_adopted = next(k for k in range(start, n) if ad[k]) - start
        for t in range(n - start):
            dst.fill_(POISON)
            r = idx.Show(t, dst, adopt=False)
            if t >= first_adopted:
                assert r.data_pnt is dst, f"{where} t={t}"
                assert np.array_equal(dst.cpu().numpy(), truth[start + t][0]), f"{where} t={t}: picture"
            else:
                assert r.data_pnt is old, f"{where} t={t}"
            assert r.significant_changes == (False if keys[start + t] else truth[start + t][1]), f"{where} t={t}"
        assert gpu.PreviousFrame() is old
        idx.close()
        gpu.StopAndClean()


# ---- index: adopt, then play on -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chunk", [None, 33], ids=lambda c: f"chunk{c}")
@pytest.mark.parametrize("size", [(37, 23), (64, 48), (262, 26)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("bits", [16, 8])
def test_index_adopt_then_play_on(bits, size, chunk):
    """Show(t, adopt=True), then the next 3 frames through DecompressP / DecompressI: the codec state the show leaves —
    previous frame and the per-row block_changes built from the coded-row words and the first untouched block of each frame
    (rows[] / stop[] of msv1_coded_bitmap_kernel, words 1 and up) — is the sequential one."""
    w, h = size
    frames, keys, pal, plan, truth = clip(bits, w, h)
    n = plan["n"]
    gpu = make(bits, w, h, pal, plan["lines"], chunk)
    idx = gpu.BuildIndex(frames, keys, key_row=plan["lines"])
    pool = [R.dev_buf(w * h) for _ in range(4)]
    for t in sorted({31, 32, 33, 127, 128, 129, n - 1} | set(plan["markers"])):
        where = f"{bits}-bit {w}x{h} chunk={chunk} show({t}) ({PARSE} parse)"
        dst = next(b for b in pool if b is not gpu.PreviousFrame())
        r = idx.Show(t, dst, adopt=True)
        assert r.data_pnt is dst and gpu.PreviousFrame() is dst, where
        assert np.array_equal(dst.cpu().numpy(), truth[t][0]), where + ": picture"
        assert gpu.counter("msv1_block_changes") == truth[t][2], where + ": block_changes"
        play(gpu, frames, keys, t + 1, min(n, t + 4), pool, truth, where)
    idx.close()
    gpu.StopAndClean()


# ---- seek --------------------------------------------------------------------------------------------------------------------
def seek_targets(plan, keys, chunk):
    """Targets whose range (from the nearest key frame) has a block last coded more than 128 frames back, and targets whose last
    frame codes a block whose previous writer lies in an earlier chunk of the range (the stage-2 compare's second writer)."""
    n, far, cross = plan["n"], [], []
    for t in range(1, n):
        s = player.nearest_key_frame(keys, t)
        lw = R.last_writers(plan, s, t)
        if (lw >= 0).any() and t - lw[lw >= 0].min() > 128:
            far.append(t)
        if chunk and not keys[t]:
            for b in np.nonzero(plan["coded"][t])[0]:
                p = R.last_writer(plan, s, t - 1, int(b))
                if p >= 0 and (p - s) // chunk < (t - s) // chunk:
                    cross.append(t)
                    break
    pick = lambda xs: sorted({xs[0], xs[len(xs) // 2], xs[-1]}) if xs else []
    return pick(far), pick([t for t in cross if t - player.nearest_key_frame(keys, t) > 64])


def check_seek(bits, w, h, frames, keys, pal, plan, truth, start, target, chunk=None, misalign=False, play_on=3):
    gpu = make(bits, w, h, pal, plan["lines"], chunk)
    pool = [R.dev_buf(w * h) for _ in range(3)]
    play(gpu, frames, keys, 0, start, pool)
    old = gpu.PreviousFrame()
    dst = R.dev_buf(w * h, misalign=misalign)
    res = gpu.Seek(frames[start:target + 1], dst, keys[start:target + 1])
    where = f"{bits}-bit {w}x{h} seek {start}..{target} chunk={chunk} misalign={misalign} ({PARSE} parse)"
    if R.adopted(plan)[start:target + 1].any():
        assert res.data_pnt is dst and gpu.PreviousFrame() is dst, where
        assert np.array_equal(dst.cpu().numpy(), truth[target][0]), where + ": picture"
    else:
        assert res.data_pnt is old and np.all(dst.cpu().numpy() == POISON), where
    assert res.significant_changes == (False if keys[target] else truth[target][1]), where
    assert gpu.counter("msv1_block_changes") == truth[target][2], where + ": block_changes"
    pool = [p for p in pool if p is not gpu.PreviousFrame()] + [dst]
    play(gpu, frames, keys, target + 1, min(plan["n"], target + 1 + play_on), pool, truth, where)
    gpu.StopAndClean()


@pytest.mark.parametrize("chunk", [None, 5, 33], ids=lambda c: f"chunk{c}")
@pytest.mark.parametrize("size", [(13, 9), (37, 23), (64, 48), (262, 26)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("bits", [16, 8])
def test_seek_from_the_nearest_key_frame(bits, size, chunk):
    w, h = size
    frames, keys, pal, plan, truth = clip(bits, w, h)
    far, cross = seek_targets(plan, keys, chunk)
    assert far and (cross or not chunk)
    for t in far + cross:
        check_seek(bits, w, h, frames, keys, pal, plan, truth, player.nearest_key_frame(keys, t), t, chunk)
    if chunk is None:   # and from an inter frame, into a destination that is not 16-byte aligned
        check_seek(bits, w, h, frames, keys, pal, plan, truth, MID, far[-1], misalign=True)


# ---- find change -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chunk", [None, 7, 33], ids=lambda c: f"chunk{c}")
@pytest.mark.parametrize("size", [(37, 23), (64, 48), (262, 26)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("bits", [16, 8])
def test_find_change_walk(bits, size, chunk):
    """walk(): FindChange from the frame after the one shown to the end, with and without stepping a frame after each landing —
    the landing, every entry of the significance list and the picture against the oracle."""
    w, h = size
    frames, keys, pal, plan, truth = clip(bits, w, h)
    tr = [(p, s) for p, s, _ in truth]
    for step in (False, True):
        R.walk(bits, w, h, pal, frames, keys, lines=plan["lines"], chunk=chunk, step=step, parse=PARSE, truth=tr)


# ---- one full-size case ------------------------------------------------------------------------------------------------------
def test_full_hd_8bit_index_and_step_back():
    """1920x1080 8-bit: an index over 96 frames of a long clip, 20 values of t where blocks were last coded 64+ frames before
    (or never since the key frame), then the step back over them adopting as the Manager does."""
    import torch
    bits, w, h, n = 8, 1920, 1080, 96
    frames, keys, pal, plan = R.long_clip(bits, w, h, seed=11, n=n)
    far = [t for t in range(n) if (t - R.last_writers(plan, 0, t) >= 64).any()]
    rest = [t for t in range(n) if t not in far]
    far = [far[int(i)] for i in np.linspace(0, len(far) - 1, min(12, len(far)))]
    ts = sorted(set(far) | {rest[int(i)] for i in np.linspace(0, len(rest) - 1, 20 - len(far))})
    assert len(ts) == 20 and far
    truth = R.truth_run(bits, w, h, pal, frames, keys, plan["lines"], key_row=plan["lines"], keep=set(ts))
    gpu = make(bits, w, h, pal, plan["lines"])
    idx = gpu.BuildIndex(frames, keys, key_row=plan["lines"])
    assert idx.significance == [truth[k][1] for k in range(n)]
    bufs = [R.dev_buf(w * h) for _ in range(2)]
    for k, t in enumerate(ts):
        r = idx.Show(t, bufs[k & 1], adopt=False)
        assert r.data_pnt is bufs[k & 1]
        assert np.array_equal(bufs[k & 1].cpu().numpy(), truth[t][0]), f"frame {t}"
    for k, t in enumerate(reversed(ts)):   # the step back, adopting
        dst = next(b for b in bufs if b is not gpu.PreviousFrame())
        idx.Show(t, dst, adopt=True)
        torch.cuda.synchronize()
        assert gpu.PreviousFrame() is dst
        assert np.array_equal(dst.cpu().numpy(), truth[t][0]), f"step back: frame {t}"
    idx.close()
    gpu.StopAndClean()
