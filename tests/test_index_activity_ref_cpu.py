"""The activity map of a seek index, checked without a GPU: the models of the two kernels' walks (tests/index_activity_ref.py)
equal THE DEFINITION — changed pixels per 16 x 16 cell between whole pictures of the oracle's sequential run — on the clips the GPU
tests use, and every deliberately broken walk (`wrong=`) is caught by at least one of them."""
import numpy as np
import pytest

import index_activity_ref as ar
import msv1_index_play_ref as pr
import sp_directed_clips as dc
import sp_index_ref as sref
from msv1_range_clips import Idle, long_clip, make_plan, palette, truth_run

RUNS = [(0, None), (1, 1), (31, 3), (32, 33), (-1, 1)]   # (first, n): n None = all frames, first -1 = the last frame
MSV1_N = 72                                              # words 0, 1, 2; the key frame at 70 repaints the picture as it is


def msv1_case(bits, w, h, start):
    """The first MSV1_N frames of long_clip from `start` on, as an index over them sees them: (coded, block_pics, before, P(-1), P)."""
    frames, keys, pal, plan = long_clip(bits, w, h, seed=5, n=96)
    assert not plan["raises"]
    truth = truth_run(bits, w, h, pal, frames[:start + MSV1_N], keys[:start + MSV1_N], plan["lines"], key_row=plan["lines"])
    pics = [t[0] for t in truth]
    coded = plan["coded"][start:start + MSV1_N]
    before = pics[start - 1] if start > 0 else None
    p_before, p = ar.msv1_pictures(pics[start:], coded, w, h, before)
    block_pics = [pr.to_blocks(x, w, h) for x in pics[start:]]
    return coded, block_pics, before, p_before, p


def runs_of(n):
    return [(n - 1 if first < 0 else first, n - first if count is None else count) for first, count in RUNS]


@pytest.mark.parametrize("bits", [16, 8])
@pytest.mark.parametrize("size", [(64, 32), (52, 28), (54, 30)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("start", [0, 3], ids=["nothing_before", "picture_before"])
def test_msv1_model_equals_the_definition(bits, size, start):
    w, h = size
    coded, block_pics, before, p_before, p = msv1_case(bits, w, h, start)
    caught = set()
    for first, n in runs_of(MSV1_N):
        want = ar.activity(p[first:first + n], p[first - 1] if first > 0 else p_before, w, h)
        assert want.max() <= 256
        for segs in (1, 2, 7):
            got = ar.msv1_model(coded, block_pics, w, h, first, n, segs, before)
            assert np.array_equal(got, want), f"{bits}-bit {w}x{h} start={start} first={first} n={n} segs={segs}"
        for wrong, segs in (("bit_is_16", 1), ("no_recompose", 2)):
            if not np.array_equal(ar.msv1_model(coded, block_pics, w, h, first, n, segs, before, wrong=wrong), want):
                caught.add(wrong)
    assert caught == {"bit_is_16", "no_recompose"}
    # the clip has what the map is about: bits that are set for blocks that do not change (repaints, the key frame at 70) ...
    whole = ar.activity(p, p_before, w, h)
    bits_set = coded.reshape(MSV1_N, -1).sum(axis=1)
    assert any(bits_set[t] > 0 and whole[t].sum() == 0 for t in range(1, MSV1_N))
    # ... and cells that are not whole where the size has them
    cols, rows = ar.grid(w, h)
    cw, ch = min(16, 4 * (w // 4) - 16 * (cols - 1)), min(16, 4 * (h // 4) - 16 * (rows - 1))   # the corner cell's pixels inside blocks
    assert whole.shape == (MSV1_N, rows, cols) and 0 < whole[:, rows - 1, cols - 1].max() <= cw * ch


def test_msv1_first_writer_is_compared_with_zeros():
    """cut_short_clip at 8 bits: blocks with no writer and no picture before are zeros until their first writer."""
    w, h = 64, 32
    frames, keys, pal, at = pr.cut_short_clip(8, w, h)
    plan = make_plan(8, w, h, frames, keys, 36)
    coded = plan["coded"]
    assert not coded[0, at:].any() and coded[0, :at].all()
    pics = [t[0] for t in truth_run(8, w, h, pal, frames, keys)]
    p_before, p = ar.msv1_pictures(pics, coded, w, h)
    want = ar.activity(p, p_before, w, h)
    block_pics = [pr.to_blocks(x, w, h) for x in pics]
    for segs in (1, 3):
        assert np.array_equal(ar.msv1_model(coded, block_pics, w, h, 0, len(frames), segs), want)
    assert want[2].sum() > 0, "frame 2 is the first writer of blocks the key frame left: they change from zeros"


def test_msv1_recoded_blocks_change_nothing():
    """Idle.recode: blocks coded again with the pixels they had — the bitmap bits are set, the map is zero."""
    w, h = 64, 32
    g = Idle(16, w, h, seed=3)
    frames = [g.key()] + [g.recode(list(range(k, g.nb, 3))) for k in range(3)] + [g.change([g.nb - 1])]
    keys = [True] + [False] * 4
    plan = make_plan(16, w, h, frames, keys, 36)
    assert plan["coded"][1:4].any(axis=1).all()
    pics = [t[0] for t in truth_run(16, w, h, palette(16), frames, keys)]
    p_before, p = ar.msv1_pictures(pics, plan["coded"], w, h)
    want = ar.activity(p, p_before, w, h)
    assert not want[1:4].any()
    # one block of a corner cell changed: exactly one non-zero element, the differing pixels of that block
    cols, rows = ar.grid(w, h)
    assert np.count_nonzero(want[4]) == 1 and want[4, rows - 1, cols - 1] == np.count_nonzero(p[4] != p[3])
    got = ar.msv1_model(plan["coded"], [pr.to_blocks(x, w, h) for x in pics], w, h, 0, 5)
    assert np.array_equal(got, want)
    assert not np.array_equal(ar.msv1_model(plan["coded"], [pr.to_blocks(x, w, h) for x in pics], w, h, 0, 5, wrong="bit_is_16"), want)


SP_RUNS = [(0, None), (1, 1), (31, 3), (33, 64)]


@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_sp_model_equals_the_definition_on_the_painted_clips(name):
    clip = dc.clip(name)
    w, h, n = clip.w, clip.h, dc.N
    pictures, _ = dc.oracle(name)
    comp = sref.Composer(clip, preinit=dc.KEY_ROW)
    keys_at = [t for t in range(n) if clip.keys[t]]
    runs = [(f, n - f if c is None else c) for f, c in SP_RUNS] + [(k, 5) for k in keys_at[1:2]] + [(k + 1, 5) for k in keys_at[1:2]]
    caught = set()
    zeros = np.zeros(w * h, dtype=np.uint32)
    for first, count in runs:
        want = ar.activity(pictures[first:first + count], pictures[first - 1] if first > 0 else zeros, w, h)
        assert np.array_equal(ar.sp_model(comp, w, h, first, count), want), f"{clip.name} first={first} n={count}"
        for wrong in ("rect_area", "key_ignored"):
            if not np.array_equal(ar.sp_model(comp, w, h, first, count, wrong=wrong), want):
                caught.add(wrong)
    # every painted pixel differs from the frame before: an inter frame's counts are the areas of regions(), by hand
    whole = ar.activity(pictures, zeros, w, h)
    nbx, _ = dc.geometry(w, h)
    for t in range(n):
        if clip.keys[t]:
            continue
        areas = {b: (x2 - x1) * (y2 - y1) for b, (x1, y1, x2, y2) in dc.regions(t, w, h).items()}
        flat = whole[t].reshape(-1)
        assert {b: int(v) for b, v in enumerate(flat) if v} == areas, f"{clip.name} frame {t}"
        assert flat[0] == 1
        if t in dc.REPAINTS:
            assert flat[4] == 256
    if len(keys_at) > 1:
        assert "key_ignored" in caught
    # (painted rectangles are all change: rect_area is caught on the generated clips below)


@pytest.mark.parametrize("case", [(41, 64, 48, 41, 24, 4, 11, 36), (43, 37, 23, 41, 24, 2, 11, 5), (45, 100, 52, 30, 16, 2, 11, 7)],
                         ids=lambda c: "cfg%d_%dx%d_%dbpp_v%d" % (c[0], c[1], c[2], c[4], c[5]))
def test_sp_model_equals_the_definition_on_generated_clips(case):
    cfg, w, h, n, bpp, version, key_every, key_row = case
    clip = sref.make_clip(cfg, w, h, n, bpp, version, key_every, key_row)
    pictures, _ = sref.oracle_run(clip)
    comp = sref.Composer(clip)
    zeros = np.zeros(w * h, dtype=np.uint32)
    caught = set()
    for first, count in ((0, n), (1, 1), (5, 20), (key_every, 4), (key_every + 1, 4)):
        want = ar.activity(pictures[first:first + count], pictures[first - 1] if first > 0 else zeros, w, h)
        assert np.array_equal(ar.sp_model(comp, w, h, first, count), want), f"{clip.name} first={first} n={count}"
        for wrong in ("rect_area", "key_ignored"):
            if not np.array_equal(ar.sp_model(comp, w, h, first, count, wrong=wrong), want):
                caught.add(wrong)
    assert "key_ignored" in caught
    if w >= 64:   # (at 37x23 nearly every move would leave the picture and is dropped: the rectangles there are all change)
        assert "rect_area" in caught, "motion literalised into rectangles rewrites pixels that stay"
