"""The lane-to-cell geometry of msv1_index_activity_kernel, checked without a GPU: on the directed clips of
tests/msv1_activity_geometry_clips.py the model of the kernel's walk (index_activity_ref.msv1_model, which enumerates lanes as the
launch does) equals THE DEFINITION over the oracle's sequential run, the clips keep what they promise, and the two wrong geometries
(`wrong="cols_is_4"`, `"one_workgroup"`) are caught on the new sizes — and provably not on the sizes the suite had before."""
import numpy as np
import pytest

import index_activity_ref as ar
import msv1_activity_geometry_clips as gc
import msv1_index_play_ref as pr
import test_index_activity_ref_cpu as old
from msv1_range_clips import make_plan, palette, truth_run

SEGMENTS = (1, 3, 7, 64)   # 64: more segments than any run has frames — clamped to one frame a segment
GEOMETRY = ("cols_is_4", "one_workgroup")


def runs_of(n, start):
    """(first, count) in index frames.  The third run is sweep frames 29 .. 34 whatever `start` is: the frames around the change at
    frame 31 — with start = 0 it crosses the bitmap word boundary with work on both sides."""
    return [(0, n), (1, 1), (29 - start, 6), (n - 1, 1)]


def sweep_case(bits, w, h, start):
    """The sweep from `start` on as an index over it sees it: (marks, coded, block_pics, before, P(-1), P)."""
    frames, keys, marks = gc.sweep(bits, w, h)
    plan = make_plan(bits, w, h, frames, keys, 36)
    assert not plan["raises"]
    pics = [t[0] for t in truth_run(bits, w, h, palette(bits), frames, keys)]
    coded = plan["coded"][start:]
    before = pics[start - 1] if start > 0 else None
    p_before, p = ar.msv1_pictures(pics[start:], coded, w, h, before)
    return marks, coded, [pr.to_blocks(x, w, h) for x in pics[start:]], before, p_before, p


@pytest.mark.parametrize("bits", [16, 8])
@pytest.mark.parametrize("size", gc.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("start", [0, 3], ids=["nothing_before", "picture_before"])
def test_the_model_equals_the_definition_on_the_sweep(bits, size, start):
    w, h = size
    marks, coded, block_pics, before, p_before, p = sweep_case(bits, w, h, start)
    n = gc.FRAMES - start
    whole = ar.activity(p, p_before, w, h)
    gc.check_properties(whole, marks, w, h, start)
    recode = gc.recode_frame(marks) - start
    assert coded[recode].all(), "every bitmap bit of the recode frame is set"
    for first, count in runs_of(n, start) + [(f - start, 1) for f, _, _ in marks if f >= start]:
        want = ar.activity(p[first:first + count], p[first - 1] if first > 0 else p_before, w, h)
        assert np.array_equal(want, whole[first:first + count])
        for segs in SEGMENTS:
            got = ar.msv1_model(coded, block_pics, w, h, first, count, segs, before)
            assert np.array_equal(got, want), f"{bits}-bit {w}x{h} start={start} first={first} n={count} segs={segs}"


@pytest.mark.parametrize("bits", [16, 8])
@pytest.mark.parametrize("size", [(80, 80), (84, 72), (272, 20)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_a_wrong_geometry_is_caught_on_the_sweep(bits, size):
    """Each wrong geometry differs from the definition over the whole sweep, and on single mark frames: exactly those
    msv1_activity_geometry_clips.caught_by names, by reasoning — there the marked block has no owner and the frame comes out zero."""
    w, h = size
    marks, coded, block_pics, before, p_before, p = sweep_case(bits, w, h, 0)
    cols, rows = ar.grid(w, h)
    whole = ar.activity(p, p_before, w, h)
    for wrong in GEOMETRY:
        assert not np.array_equal(ar.msv1_model(coded, block_pics, w, h, 0, gc.FRAMES, 1, before, wrong=wrong), whole), wrong
        differs = []
        for f, r, q in marks:
            got = ar.msv1_model(coded, block_pics, w, h, f, 1, 1, before, wrong=wrong)
            if not np.array_equal(got, whole[f:f + 1]):
                assert not got.any(), f"{wrong}: mark frame {f}"
                differs.append(f)
        expected = gc.caught_by(wrong, marks, cols, rows)
        assert differs == expected and expected, f"{wrong} at {w}x{h}: mark frames {differs}, expected {expected}"
        assert marks[-1][0] in differs, "the last cell is lost to either"


@pytest.mark.parametrize("bits", [16, 8])
@pytest.mark.parametrize("size", [(64, 32), (52, 28), (54, 30)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_the_old_sizes_cannot_catch_a_wrong_geometry(bits, size):
    """THE GAP, kept as a statement: the three sizes of test_index_activity_ref_cpu / test_index_activity_gpu have a grid of 4 x 2
    cells — four columns, 128 lanes — so both wrong geometries equal the definition for every run there.  (A size added there that
    catches them makes this test fail: it is the one to update.)"""
    w, h = size
    assert ar.grid(w, h) == (4, 2)
    for start in (0, 3):
        coded, block_pics, before, p_before, p = old.msv1_case(bits, w, h, start)
        for first, n in old.runs_of(old.MSV1_N):
            want = ar.activity(p[first:first + n], p[first - 1] if first > 0 else p_before, w, h)
            for wrong in GEOMETRY:
                got = ar.msv1_model(coded, block_pics, w, h, first, n, 1, before, wrong=wrong)
                assert np.array_equal(got, want), f"{wrong} is caught at {w}x{h} start={start} first={first} n={n}"
