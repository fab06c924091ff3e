"""The long clips of test_range_calls_long_gpu.py reach the edges of the range kernels (msv1_seek_kernels.hip) — checked from
their plan and the oracle, without a GPU, so that a change to the clip builder cannot quietly take an edge away."""
import numpy as np
import pytest

import msv1_range_clips as R
from oracle_binding import OracleAbort, OracleMSVideo1

# what test_range_calls_long_gpu.py uses: sizes, the mid-clip index start, chunk options of the index and FindChange tests
SIZES = [(4, 4), (13, 9), (37, 23), (64, 48)]
MID = R.LATE_FROM
INDEX_CHUNKS = (5, 31, 33)
FIND_CHUNKS = (7, 33)


def clip(bits, w, h):
    return R.long_clip(bits, w, h, seed=w * h + bits)


def group_words(plan, start, t, b):
    """msv1_index_show_kernel's walk for block b at t of an index from `start`: the non-zero bitmap words of the SCAN group
    (4 words) in which the walk stops, nearest first ([]: it does not walk or finds nothing)."""
    col = plan["coded"][start:start + t + 1, b]
    w = t // 32
    if col[32 * w:].any():
        return []
    while w > 0:
        group = [v for v in range(w - 1, w - 5, -1) if v >= 0 and col[32 * v:32 * v + 32].any()]
        if group:
            return group
        w -= 4
    return []


@pytest.mark.parametrize("bits", [16, 8])
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_schedule_and_oracle(bits, size):
    """The parse codes what the schedule meant to code, and the oracle raises on no frame the plan does not mark."""
    w, h = size
    frames, keys, pal, plan = clip(bits, w, h)
    assert 200 <= len(frames) <= 300 and plan["raises"] == []
    for i, want in enumerate(plan["intent"]):
        if want is not None:
            assert sorted(np.nonzero(plan["coded"][i])[0].tolist()) == want, f"frame {i}"
    assert [i for i, k in enumerate(keys) if k] == [0] + list(R.KEYS_AT)
    assert all(k % 32 for k in R.KEYS_AT) and frames[R.KEYS_AT[2]] == frames[R.KEYS_AT[1]]
    o = OracleMSVideo1(bits, w, h, pal)
    o.Preinit(plan["lines"])
    bufs = [np.zeros(w * h, dtype=np.int32) for _ in range(3)]
    for i, (f, k) in enumerate(zip(frames, keys)):
        dst = next(b for b in bufs if b is not o.PreviousFrame())
        try:
            if k:
                if o.DecompressI(f, dst) != 0:
                    raise OracleAbort()
            else:
                o.DecompressP(f, dst)
        except OracleAbort:
            assert i in plan["raises"], f"frame {i} raises"
            break


@pytest.mark.parametrize("bits", [16, 8])
@pytest.mark.parametrize("size", SIZES[1:], ids=lambda s: f"{s[0]}x{s[1]}")
def test_index_edges(bits, size):
    w, h = size
    frames, keys, pal, plan = clip(bits, w, h)
    n = plan["n"]
    # a block's last writer 5 or more bitmap words below t (the index from frame 0 shows every t)
    far = 0
    for t in range(n):
        lw = R.last_writers(plan, 0, t)
        far = max(far, max(t // 32 - int(f) // 32 for f in lw if f >= 0))
    assert far >= 5
    # two writers of one block in the 4-word group the show kernel reads below t's word: the nearest one counts
    assert any(len(group_words(plan, 0, t, b)) >= 2 for t in range(64, n) for b in range(plan["nb"]))
    # from an inter frame mid-clip: a block no frame of the range has coded yet, shown at t >= 32
    assert not keys[MID]
    assert any((R.last_writers(plan, MID, MID + t) < 0).any() for t in range(32, n - MID))
    # each chunk option: a chunk boundary inside word 1 or later, with a block coded before it in that word and not again
    # up to a t of the word after it (the word keeps the chunk before's bits)
    for start in (0, MID):
        for chunk in INDEX_CHUNKS:
            hit = False
            for a in range(chunk, n - start, chunk):
                wd = a // 32
                if wd < 1 or a % 32 == 0:
                    continue
                lo, hi = start + 32 * wd, start + min(32 * wd + 31, n - start - 1)
                before = plan["coded"][lo:start + a].any(axis=0)
                after = plan["coded"][start + a:hi + 1]
                if (before & ~after[0]).any():
                    hit = True
                    break
            assert hit, (start, chunk)


def landings(truth, step):
    """(start, hit) of every FindChange walk() makes, from the oracle's significance."""
    n, shown, out = len(truth), 0, []
    while shown < n - 1:
        start = shown + 1
        f = R.expected_landing(truth, start)
        out.append((start, f))
        shown = f
        if step and shown < n - 1:
            shown += 1
    return out


@pytest.mark.parametrize("bits", [16, 8])
@pytest.mark.parametrize("size", [(37, 23), (64, 48)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_find_change_edges(bits, size):
    """Some FindChange hit lies 64+ walk entries after the start of its range, and the block it changes was last coded 32+
    entries before (an earlier segment of the change scan, whatever the segment length up to 32)."""
    w, h = size
    frames, keys, pal, plan = clip(bits, w, h)
    truth = R.truth_run(bits, w, h, pal, frames, keys, plan["lines"], key_row=plan["lines"])
    found = False
    for step in (False, True):
        for start, hit in landings(truth, step):
            wl = R.walk_list(plan, start, hit)
            if not truth[hit][1] or hit not in wl or wl.index(hit) < 64:
                continue
            j = wl.index(hit)
            for b in np.nonzero(plan["coded"][hit])[0]:
                prev = R.last_writer(plan, start, hit - 1, int(b))
                if prev >= 0 and j - wl.index(prev) >= 32 and R.scan_segment(plan["nb"], len(wl)) <= 32:
                    found = True
    assert found


@pytest.mark.parametrize("size", SIZES[1:], ids=lambda s: f"{s[0]}x{s[1]}")
def test_end_markers_where_the_schedule_puts_them(size):
    w, h = size
    frames, keys, pal, plan = clip(8, w, h)
    nbx, nby, srow = plan["nbx"], plan["nby"], plan["srow"]
    want = (srow * nbx, srow * nbx + nbx - 1, (nby - 1) * nbx)
    got = [plan["markers"].get(f) for f in R.MARKERS_AT]
    assert got == [want[j % 3] for j in range(len(R.MARKERS_AT))]
    for edge in (32, 64, 128):   # both sides of each word boundary
        assert edge - 1 in plan["markers"] and edge + 1 in plan["markers"]
    # 16-bit: a truncated frame and one with an odd trailing byte
    f16, _, _, _ = clip(16, w, h)
    assert len(f16[R.MARKERS_AT[1]]) % 2 == 1 and len(f16[R.MARKERS_AT[4]]) % 2 == 1


def test_full_hd_clip_edges():
    """The 1920x1080 8-bit index case: ~96 frames, blocks left alone for 64 frames or more."""
    frames, keys, pal, plan = R.long_clip(8, 1920, 1080, seed=11, n=96)
    assert any((t - R.last_writers(plan, 0, t) >= 64).any() for t in range(64, 96))
