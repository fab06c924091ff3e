"""The directed clips of tests/msv1_row_sweep_clips.py and the models of tests/row_sweep_ref.py, without a GPU: the clips hold what
they were built for (census, asserted on the oracle alone), the oracle keeps the paint of the pixels no block covers, the model of
msv1_coded_bitmap_kernel's rows[] / stop[] and of the host loop behind them equals the oracle's block_changes on every frame, the
model of uncovered_pixel enumerates exactly the uncovered pixels — and every named mistake is caught: which size catches which is
stated in CATCHES and asserted both ways.

Only references are compared with the oracle here: nothing of this file runs a kernel."""
import functools

import numpy as np
import pytest

import msv1_range_clips as R
import msv1_row_sweep_clips as S
import row_sweep_ref as ref

IDS = lambda s: f"{s[0]}x{s[1]}"
ALL = set(S.SIZES)
ONE_ROW = {(4, 4), (8, 4)}          # one wave, one block row, no cut that starts a row
SEVERAL = ALL - ONE_ROW             # more than one wave and more than one row
LONG_ROWS = {(260, 24), (262, 26), (1028, 8), (1030, 10)}
WITH_REMAINDER = [s for s in S.SIZES if s[0] % 4 or s[1] % 4]

# mistake: (the sizes whose 16-bit sweep shows it, the sizes whose 8-bit sweep shows it) — exactly these, by this reasoning:
CATCHES = {
    # d = 32 missing: a lane sees 31 lanes ahead.  Only a row segment of more than 32 lanes in one wave has a block further from its
    # first lane: nbx = 65 (MARK of block 63, lane 63 of row 0's segment) and nbx = 257; nbx = 17 and 5 have no such segment
    "ladder_stops_at_16": (LONG_ROWS, LONG_ROWS),
    # the first lane of a row takes the bits of the rows behind it in its wave: a MARK in the next row sets this row too.  It takes
    # two rows in one wave: not 1x1, 2x1
    "no_row_guard": (SEVERAL, SEVERAL),
    # __shfl_up hands lane 0 its own row, so lane 0 never stores: whatever row lies on lane 0 of a wave loses that wave's bits —
    # row 0 of every picture through wave 0 (the MARK of block 0), so every size; see test_no_lane0_store_at_68x16 for the rest
    "no_lane0_store": (ALL, ALL),
    # a row that starts inside a wave is never stored: it takes a second row
    "first_lane_of_wave_only": (SEVERAL, SEVERAL),
    # only an 8-bit end marker leaves blocks untouched (a 16-bit stream that ends paints the rest).  With a maximum the stop is the
    # first block of the LAST wave, so a cut in an earlier row resets rows the frame never walked: it takes two waves and two rows
    "stop_is_max": (set(), SEVERAL),
    # one row short: the row of the marker is not walked.  A cut inside a row leaves the row's flag 1 either way (c = m - 1 lies in
    # it and the frame before set it); a cut that starts a row must clear it.  8-bit, and a second row
    "stop_row_not_reset": (set(), SEVERAL),
    # blk / 64 is blk / nbx on wave 0 only where nbx >= 64 or there is one row; block nbx is in row 1 and in wave 0 at 17 and 5,
    # and block 64 is in row 0 but "row 1" at 65 and 257
    "div_by_64": (SEVERAL, SEVERAL),
}
assert set(CATCHES) == set(ref.ROW_MISTAKES)


@functools.lru_cache(maxsize=None)
def clip(bits, w, h):
    frames, keys, marks, stops = S.sweep(bits, w, h)
    pal, lines = R.palette(bits), R.straddle_lines(h)
    truth = S.painted_truth(bits, w, h, pal, frames, keys, lines)
    plan = R.make_plan(bits, w, h, frames, keys, lines)
    return frames, keys, marks, stops, pal, lines, truth, plan


def tables(bits, w, h):
    """(coded, untouched, noop) per frame and block, from the parse's control flow alone."""
    plan = clip(bits, w, h)[7]
    untouched = np.zeros_like(plan["coded"])
    for f, s in enumerate(plan["stop"]):
        if s is not None:
            untouched[f, s:] = True
    return plan["coded"], untouched, plan["early_out"]


# ---- the clips -----------------------------------------------------------------------------------------------------------------
def test_the_sizes_put_the_seams_where_the_table_says():
    geo = {s: (s[0] // 4, s[1] // 4) for s in S.SIZES}
    assert [geo[s] for s in S.SIZES] == [(1, 1), (2, 1), (17, 4), (17, 4), (65, 6), (65, 6), (257, 2), (257, 2), (5, 62), (5, 62)]
    assert [r * 17 % 64 for r in range(1, 4)] == [17, 34, 51] and 64 // 17 == 3 and 67 // 17 == 3        # 68x16
    assert 64 // 65 == 0 and 65 // 65 == 1 and 255 // 65 == 256 // 65 == 3                                  # 260x24
    assert sorted({s % 65 for s in range(64, 390, 64)}) == [59, 60, 61, 62, 63, 64]   # six seams, six columns
    assert 256 // 257 == 0 and 257 // 257 == 1 and 257 > S.WG                                               # 1028x8
    assert max(nby for _, nby in geo.values()) == S.ROWS_SHOWN and -(-64 // 5) == 13                        # 20x248
    assert [s // 5 for s in range(64, 310, 64)] == [12, 25, 38, 51] == [(s - 1) // 5 for s in range(64, 310, 64)]
    nrem = {s: int(S.uncovered(*s).sum()) for s in WITH_REMAINDER}
    assert nrem == {(70, 18): 172, (262, 26): 572, (1030, 10): 2076, (22, 250): 540}
    assert (390 + 572 + 255) // 256 == 4 and 390 - 256 == 134 and 2 * 24 == 48                              # 262x26
    assert -(-(514 + 2076) // 256) == 11 and 1030 > 4 * S.WG and 2 * 248 == 496


@pytest.mark.parametrize("size", S.SIZES, ids=IDS)
def test_marked_blocks(size):
    nbx, nby = size[0] // 4, size[1] // 4
    nb = nbx * nby
    marked = S.marked_blocks(nbx, nby)
    assert marked == sorted(set(marked)) and {0, nb - 1} <= set(marked) and all(0 <= b < nb for b in marked)
    for s in range(64, nb, 64):
        assert s - 1 in marked and s in marked
    rows = S.marked_rows(nbx, nby)
    assert {0, nby - 1} <= set(rows)
    if nby <= 12:
        assert rows == list(range(nby))
    else:
        assert rows == [0, 11, 12, 13, 24, 25, 26, 37, 38, 39, 50, 51, 52, 61] and len(marked) == 34
    for r in rows:
        assert r * nbx in marked and r * nbx + nbx - 1 in marked


@pytest.mark.parametrize("size", S.SIZES, ids=IDS)
@pytest.mark.parametrize("bits", [16, 8])
def test_census(bits, size):
    w, h = size
    frames, keys, marks, stops, pal, lines, truth, plan = clip(bits, w, h)
    nbx, nby = w // 4, h // 4
    marked = S.marked_blocks(nbx, nby)
    assert len(frames) == 1 + len(marked) + 2 * (len(marked) - 1) <= S.MAX_FRAMES
    assert len(frames) == {1: 2, 2: 5, 68: 29, 390: 68, 514: 56, 310: 101}[nbx * nby]
    assert [b for _, b in marks] == marked and [m for _, m, _ in stops] == marked[1:]
    assert sorted([0] + [f for f, _ in marks] + [f - 1 for f, _, _ in stops] + [f for f, _, _ in stops]) == list(range(len(frames)))
    assert keys == [True] + [False] * (len(frames) - 1) and not plan["raises"] and not any(plan["early_out"])
    S.check_census(truth, marks, stops, nbx, nby, bits)
    # the parse codes what the sweep meant to code
    for f, b in marks:
        assert np.flatnonzero(plan["coded"][f]).tolist() == [b], f"MARK frame {f}"
    for f, m, c in stops:
        assert plan["coded"][f - 1].all(), f"frame {f - 1}"
        want = [c] if bits == 8 else [c] + list(range(m, nbx * nby))
        assert np.flatnonzero(plan["coded"][f]).tolist() == want and plan["stop"][f] == (m if bits == 8 else None), f"STOP frame {f}"
        assert c == (m - 1 if m % nbx else max(m - nbx - 1, 0)) and 0 <= c < m


def test_the_census_notices_a_wrong_flag():
    frames, keys, marks, stops, pal, lines, truth, plan = clip(8, 68, 16)
    f = stops[3][0]
    for flip in (0, 3):
        bad = list(truth)
        bad[f] = (truth[f][0], truth[f][1], truth[f][2] ^ (1 << flip))
        with pytest.raises(AssertionError, match=f"STOP frame {f}"):
            S.check_census(bad, marks, stops, 17, 4, 8)
    bad = list(truth)
    bad[marks[2][0]] = truth[marks[2][0]][:2] + (0,)
    with pytest.raises(AssertionError, match="MARK frame"):
        S.check_census(bad, marks, stops, 17, 4, 8)


@pytest.mark.parametrize("size", WITH_REMAINDER, ids=IDS)
@pytest.mark.parametrize("bits", [16, 8])
def test_the_oracle_keeps_the_paint(bits, size):
    """A decode writes no pixel outside the block grid: every picture of the sweep holds buffer 0's paint there, pixel for pixel,
    and no block pixel holds paint."""
    w, h = size
    truth = clip(bits, w, h)[6]
    unc = S.uncovered(w, h)
    want = S.paint(w, h, 0)[unc]
    assert len(np.unique(want)) == len(want) == int(unc.sum()) and np.all(want > 0)
    assert not np.intersect1d(S.paint(w, h, 0)[unc], S.paint(w, h, 1)[unc]).size
    for f, (pic, _, _) in enumerate(truth):
        assert np.array_equal(pic[unc], want), f"frame {f}: {S.first_difference(pic, np.where(unc, S.paint(w, h, 0), pic), w, h)}"
        assert not np.isin(pic[~unc], S.paint(w, h, 0)[unc]).any() and not np.any(pic[~unc] == np.int32(R.POISON)), f"frame {f}"
    # and the plain truth_run is the same run without the paint
    frames, keys, _, _, pal, lines, _, _ = clip(bits, w, h)
    plain = R.truth_run(bits, w, h, pal, frames, keys, lines, key_row=lines, rows=True)
    for f, (pic, sig, rows) in enumerate(plain):
        assert np.array_equal(pic, S.unpainted(truth[f][0], w, h)) and (sig, rows) == truth[f][1:], f"frame {f}"


def test_first_difference_names_pixel_and_block():
    w, h = 70, 18
    a = np.zeros(w * h, dtype=np.int32)
    b = a.copy()
    assert S.first_difference(a, b, w, h) == ""
    b[5 * w + 9] = 7
    assert "pixel 359 (x=9, y=5; block 19 covers it)" in S.first_difference(a, b, w, h)
    b[5 * w + 9] = 0
    b[3 * w + 68] = 1
    b[17 * w] = 1
    msg = S.first_difference(a, b, w, h)
    assert msg.startswith("2 pixels differ") and "x=68, y=3; no block covers it" in msg


# ---- rows[] and stop[] ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", S.SIZES, ids=IDS)
@pytest.mark.parametrize("bits", [16, 8])
def test_the_row_model_equals_the_oracle(bits, size):
    w, h = size
    truth = clip(bits, w, h)[6]
    coded, untouched, noop = tables(bits, w, h)
    got = ref.rows_and_stop(coded, untouched, w // 4, h // 4, noop)
    for f, want in enumerate(t[2] for t in truth):
        assert got[f] == want, f"{bits}-bit {w}x{h} frame {f}: block_changes {got[f]:#x}, the oracle's {want:#x}"


def caught_frames(bits, size, wrong):
    w, h = size
    truth = clip(bits, w, h)[6]
    coded, untouched, noop = tables(bits, w, h)
    got = ref.rows_and_stop(coded, untouched, w // 4, h // 4, noop, wrong=wrong)
    return [f for f in range(len(truth)) if got[f] != truth[f][2]]


@pytest.mark.parametrize("wrong", ref.ROW_MISTAKES)
def test_a_wrong_row_rule_is_caught(wrong):
    for k, bits in enumerate((16, 8)):
        caught = {s for s in S.SIZES if caught_frames(bits, s, wrong)}
        assert caught == CATCHES[wrong][k], f"{wrong}, {bits}-bit: caught at {sorted(caught)}"
    assert CATCHES[wrong][0] | CATCHES[wrong][1], "no size catches it"


def test_no_lane0_store_at_68x16():
    """17 blocks to a row, 68 blocks: lane 0 of wave 0 is block 0 and lane 0 of wave 1 is block 64.  Row 0 (blocks 0..16) and the
    tail of row 3 (blocks 64..67) are stored by lane 0 alone; rows 1, 2 and the head of row 3 start inside wave 0.  So a frame shows
    the mistake exactly when a flag it must set comes from those blocks only."""
    for bits in (16, 8):
        frames, keys, marks, stops, pal, lines, truth, plan = clip(bits, 68, 16)
        lost = lambda f: any(plan["coded"][f, lo:hi].any() and not plan["coded"][f, lo2:hi2].any()
                             for lo, hi, lo2, hi2 in ((0, 17, 0, 0), (64, 68, 51, 64)))
        assert caught_frames(bits, (68, 16), "no_lane0_store") == [f for f in range(len(frames)) if lost(f)]
        by_mark = [b for f, b in marks if f in caught_frames(bits, (68, 16), "no_lane0_store")]
        assert by_mark == [0, 16, 64, 67]


def test_the_ladder_mistake_needs_a_block_32_lanes_from_its_rows_first():
    for size in sorted(LONG_ROWS):
        nbx = size[0] // 4
        frames, keys, marks, stops, pal, lines, truth, plan = clip(16, *size)
        by_mark = [b for f, b in marks if f in caught_frames(16, size, "ladder_stops_at_16")]
        first_lane = lambda b: max((b // 64) * 64, (b // nbx) * nbx)
        assert by_mark == [b for _, b in marks if b - first_lane(b) >= 32] and by_mark, size


# ---- the pixels no block covers ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", S.SIZES + [(13, 9), (37, 23), (7, 4), (4, 7), (3, 3)], ids=IDS)
def test_uncovered_order_is_the_uncovered_pixels_each_once(size):
    w, h = size
    order = ref.uncovered_order(w, h)
    want = np.flatnonzero(S.uncovered(w, h))
    assert len(order) == len(want) == (w - w // 4 * 4) * (h // 4 * 4) + w * (h - h // 4 * 4)
    assert np.array_equal(np.sort(order), want)
    cx, cy = w // 4 * 4, h // 4 * 4
    strip = (w - cx) * cy
    assert np.all(order[:strip] % w >= cx) and np.all(order[:strip] // w < cy) and np.all(order[strip:] // w >= cy)
    assert np.all(np.diff(order) > 0), "raster order: the strip row by row, then the rows"


@pytest.mark.parametrize("wrong", ref.ORDER_MISTAKES)
@pytest.mark.parametrize("size", WITH_REMAINDER + [(13, 9), (37, 23)], ids=IDS)
def test_a_wrong_order_moves_a_painted_pixel(wrong, size):
    """The copy of a painted picture into a poisoned destination: the right order brings every painted pixel over and nothing else; each
    wrong one leaves at least one painted pixel wrong."""
    w, h = size
    before = S.paint(w, h, 3)
    dst = np.full(w * h, R.POISON, dtype=np.int32)
    right = ref.copy_uncovered(before, dst, w, h)
    assert np.array_equal(right, before)
    got = ref.copy_uncovered(before, dst, w, h, wrong)
    unc = S.uncovered(w, h)
    assert np.any(got[unc] != before[unc]), f"{wrong} at {w}x{h}"
    assert S.first_difference(got, right, w, h)
