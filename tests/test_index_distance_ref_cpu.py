"""The distance map's definition (tests/index_distance_ref.py) pinned to the oracle's pictures, without a GPU: for every clip and
reference the GPU tests use (tests/index_distance_cases.py) the definition equals a brute-force compare of whole pictures, the row of
the reference frame is zeros, no cell's distance moves by more than the frame changed (the triangle inequality against
index_activity_ref.activity), and the clips are not vacuous: some element is 0, some is not, some cell keeps a non-zero value across
a frame that codes none of its blocks (the kernels' repeat store), and the "return" references find a second frame at distance 0.

"Some element is 0" is asserted for every clip and reference but these, which the clips, sizes and references the GPU tests must
cover make unsatisfiable; they are in for their non-zero values and their repeats, and everything else is asserted of them:
  * MSVideo1 "random": a random device picture shares no whole cell with any frame (here half of its pixels are noise);
  * MSVideo1 frame -1 with nothing before the index (start 0): P(-1) is zeros, and the key frame paints every block a colour;
  * MSVideo1 frame -1 at 8 x 8 with a picture before the index (start 3): the picture's only cell never shows P(2) again in the
    72 frames (at every other size with start 3 some cell does, and the assert stands);
  * ScreenPressor frame -1: P(-1) is zeros by contract, and no block of six of the seven clips is ever all zeros.
The ScreenPressor device picture is made so that it meets the assert (index_distance_cases.sp_picture_for).

What was looked for and not found, so that the tests say what the clips hold and no more:
  * sp_activity_clips codes an event in every block at every frame, so none of its values is ever repeated: the two generated clips
    carry the repeat store (test_sp_directed_clips_never_repeat_a_value states the gap);
  * the frame before ZERO_AT = 8 and 23 of those clips is never shown again (the region is painted B at 6 and restored as A), and at
    the matching RESTORE_AT the cells come DOWN, not to 0.  The frames before ZERO_AT = 31, 46 and 62 are shown again, at other
    frames than RESTORE_AT; those three and REPEAT_AT are the "return" references;
  * msv1_tight_clips.directed, reference frame 1: `back` (frame 4) restores the spots, but frame 3 also changed the blocks behind the
    spots, which stay changed: a spot's cell is 0 again at frame 4 only where it holds no such block, else 16 pixels for each."""
import numpy as np
import pytest

import index_activity_ref as ar
import index_distance_cases as cs
import index_distance_ref as dr
import sp_activity_clips as ac


def slow(pictures, ref, w, h, whole_blocks_only):
    """Whole pictures compared at once, then one slice per cell: no reshape trick, no cell_sums."""
    cols, rows = ar.grid(w, h)
    diff = np.stack([np.asarray(p).reshape(h, w).view(np.uint32) for p in pictures]) != np.asarray(ref).reshape(h, w).view(np.uint32)
    if whole_blocks_only:
        diff[:, h // 4 * 4:, :] = False
        diff[:, :, w // 4 * 4:] = False
    out = np.zeros((len(pictures), rows, cols), dtype=np.uint16)
    for r in range(rows):
        for q in range(cols):
            out[:, r, q] = diff[:, 16 * r:16 * r + 16, 16 * q:16 * q + 16].sum(axis=(1, 2))
    return out


def properties(d, act, ref, where):
    """Row `ref` is zeros; per cell |d[k] - d[k - 1]| <= act[k]."""
    if not isinstance(ref, str) and ref >= 0:
        assert not d[ref].any(), f"{where}: the reference frame is not at distance 0 from itself"
    step = np.abs(d[1:].astype(np.int64) - d[:-1].astype(np.int64))
    assert (step <= act[1:]).all(), f"{where}: a distance moves by more than the frame changed"
    assert d.max() <= 256


def repeats(d, coded):
    """Elements [k, r, q], k >= 1, that are non-zero in a frame that codes nothing of the cell: the value is the one before."""
    quiet = ~coded[1:] & (d[1:] != 0)
    assert (d[1:][quiet] == d[:-1][quiet]).all(), "a cell moved in a frame that codes none of its blocks"
    return int(quiet.sum())


# ---- MSVideo1 ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [16, 8])
@pytest.mark.parametrize("size", cs.MSV1_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("start", cs.MSV1_STARTS)
def test_msv1_definition_and_properties(bits, size, start):
    w, h = size
    c = cs.msv1_case(bits, w, h, start)
    act = ar.activity(c.p, c.p_before, w, h)
    coded = cs.coded_cells(c.coded, w, h)
    for ref in cs.msv1_references():
        where = f"{bits}-bit {w}x{h} start={start} ref={ref}"
        d = cs.msv1_truth(bits, w, h, start, ref)
        R = cs.msv1_reference(c, ref)
        assert np.array_equal(d, slow(c.p, R, w, h, True)), where
        assert np.array_equal(d[:5], dr.brute(c.p[:5], R, w, h, True)), where
        properties(d, act, ref, where)
        if (w, h) == (3, 3):
            assert not d.any(), f"{where}: a picture without a block has no pixel to compare"
            continue
        assert d.any(), where
        assert repeats(d, coded) > 0, f"{where}: no value is ever repeated"
        # (the references that cannot meet it, all fixed by what the GPU tests must cover: the module's docstring)
        if ref != "random" and not (ref == -1 and (start == 0 or (w, h) == (8, 8))):
            assert (d == 0).any(), where
    p = cs.msv1_pictures_for(bits, w, h, start)
    assert np.array_equal(cs.msv1_truth(bits, w, h, start, "frame"), cs.msv1_truth(bits, w, h, start, cs.MSV1_PICTURE_AT))
    assert np.array_equal(cs.msv1_truth(bits, w, h, start, "frame"), cs.msv1_truth(bits, w, h, start, "poisoned"))
    if w % 4 or h % 4:
        assert (p["frame"] != p["poisoned"]).any()


@pytest.mark.parametrize("bits", [16, 8])
@pytest.mark.parametrize("size", cs.MSV1_DIRECTED_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_msv1_directed_returns_and_single_pixels(bits, size):
    w, h = size
    c = cs.msv1_directed(bits, w, h)
    clip = c.clip
    act = ar.activity(c.p, c.p_before, w, h)
    for ref in cs.MSV1_DIRECTED_REFS:
        d = cs.msv1_directed_truth(bits, w, h, ref)
        assert np.array_equal(d, slow(c.p, c.p[ref], w, h, True))
        properties(d, act, ref, f"{bits}-bit {w}x{h} ref={ref}")
        assert d.any() and (d == 0).any()
    d1 = cs.msv1_directed_truth(bits, w, h, 1)
    totals = d1.reshape(c.n, -1).sum(axis=1)
    assert totals[0] == 0 and totals[1] == 0, "recode_all shows the key frame's picture: a frame other than the reference at distance 0"
    stay = cs.cells_of_blocks(sorted(set(clip.next_blocks) - set(clip.spots)), w, h)   # changed at 3, not restored at 4
    spot_cells = cs.cells_of_blocks(clip.spots, w, h)
    for (r, q), k in spot_cells.items():
        assert d1[2, r, q] >= 16 * k and d1[3, r, q] >= 16 * k, f"cell ({r}, {q}): the spots changed at frame 2 and stay changed at 3"
        assert d1[4, r, q] == 16 * stay.get((r, q), 0), f"cell ({r}, {q}) at `back`"
    if (w, h) == (128, 128):
        assert any(at not in stay for at in spot_cells), "no spot's cell returns to 0"
    d4 = cs.msv1_directed_truth(bits, w, h, 4)
    want = np.zeros(d4.shape[1:], dtype=np.uint16)
    for (r, q), k in cs.cells_of_blocks(clip.pixel_blocks, w, h).items():
        want[r, q] = k
    assert np.array_equal(d4[5], want), "one_pixel: one pixel for each of its blocks"


# ---- ScreenPressor -----------------------------------------------------------------------------------------------------------------
def sp_coded(name):
    """(n, rows, cols) bool: the frame has an event for the cell — a key frame, or a rectangle of the host stage's records in it."""
    c = cs.sp_case(name)
    comp = cs.sp_composer(name)
    w, h = c.clip.w, c.clip.h
    cols, rows = ar.grid(w, h)
    out = np.zeros((c.n, rows, cols), dtype=bool)
    for t in range(c.n):
        if c.clip.keys[t]:
            out[t] = True
        elif t in comp.mask:
            out[t] = ar.cell_sums(comp.mask[t], w, h) > 0
    return out


@pytest.mark.parametrize("name", cs.SP_NAMES)
def test_sp_definition_and_properties(name):
    c = cs.sp_case(name)
    w, h = c.clip.w, c.clip.h
    act = ar.activity(c.pictures, np.zeros(w * h, dtype=np.uint32), w, h)
    coded = sp_coded(name)
    for first, n in cs.sp_runs(name):
        assert 0 <= first and n >= 1 and first + n <= c.n
    repeated = 0
    for ref in cs.sp_references(name):
        where = f"{name} ref={ref}"
        d = cs.sp_truth(name, ref)
        R = cs.sp_reference(name, ref)
        assert np.array_equal(d, slow(c.pictures, R, w, h, False)), where
        assert np.array_equal(d[:3], dr.brute(c.pictures[:3], R, w, h, False)), where
        properties(d, act, ref, where)
        assert d.any() and (ref == -1 or (d == 0).any()), where   # (P(-1) is zeros: the module's docstring)
        repeated += repeats(d, coded)
    if c.directed:
        assert repeated == 0   # (see test_sp_directed_clips_never_repeat_a_value)
    else:
        assert repeated > 0, f"{name}: no value is ever repeated"
        for ref in cs.sp_references(name):
            assert repeats(cs.sp_truth(name, ref), coded) > 0, f"{name} ref={ref}: no value is ever repeated"


def test_sp_directed_clips_never_repeat_a_value():
    """A standing statement of the gap the generated clips fill: every frame of sp_activity_clips has an event in every block."""
    for name in ac.NAMES:
        assert sp_coded(name).all(), name


@pytest.mark.parametrize("name", ac.NAMES)
def test_sp_returns(name):
    """The picture before ZERO_AT = 31, 46 and 62, and the picture REPEAT_AT repeats, are shown by other frames too; at RESTORE_AT
    the blocks are nearer to the picture before the matching ZERO_AT than at ZERO_AT itself."""
    for ref, restored in cs.SP_RETURNS:
        d = cs.sp_truth(name, ref).reshape(ac.N, -1).astype(np.int64)
        # (no farther in any block, nearer in some: a part of a pixel or two has no region beside its beat)
        assert (d[ref + 1] >= d[restored]).all() and (d[ref + 1] > d[restored]).any() and d[ref + 1].all(), f"{name} ref={ref}"
    for ref in [z - 1 for z in ac.ZERO_AT[2:]] + [ac.REPEAT_AT]:
        totals = cs.sp_truth(name, ref).reshape(ac.N, -1).sum(axis=1)
        others = [t for t in range(ac.N) if t != ref and totals[t] == 0]
        assert others, f"{name}: no frame but {ref} shows its picture"
    assert not cs.sp_truth(name, ac.REPEAT_AT)[ac.REPEAT_AT - 1].any()
