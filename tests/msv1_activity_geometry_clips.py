"""Directed clips for the lane-to-cell geometry of msv1_index_activity_kernel (jsplayer_amd/csrc/msv1_index_activity_kernels.hip) — a
helper module, numpy only, no tests of its own.

The kernel maps lanes to cells arithmetically: lane gid of the launch belongs to cell gid >> 4 of the ceil(X / 16) x ceil(Y / 16)
grid in raster order, 16 cells to a workgroup, 4 to a wave; a tail group leaves at q >= cols * rows.  `sweep` is one short clip that
says, frame by frame, which cell must count and which must not; SIZES are the smallest pictures at which each piece of that
arithmetic can go wrong without the others:

  80x80    5x5 cells, 400 lanes: two workgroups, a 112-lane tail that returns, waves that straddle grid rows, all cells whole
  84x72    6x5, 480 lanes: the same with a last cell column of one block column and a last cell row of two block rows
  86x74    6x5: the same with X % 4, Y % 4 != 0 — the scalar load of the picture before the index
  272x20   17x2, 544 lanes: three workgroups; cell 16 is the first of workgroup 1, on grid row 0; the last cell row has one block row
  12x8     1x1: a picture smaller than a cell, 6 of the 16 lanes have a block
  4x4      1x1: one block

The frames of sweep(bits, w, h), built on msv1_range_clips.Idle:
  0            a key frame
  1            every block changes: every cell counts its pixels that lie inside blocks
  2 ..         one frame per MARKED cell, changing exactly one block — the cell's last block inside the picture.  The marked cells are
               the raster indices {0, 3, 4, cols - 1, cols, 15, 16, cols * rows - 1} inside the grid: the ends of the first wave, the
               first cell of the next grid row, the two sides of the workgroup seam, the last cell
  then         every block coded again with what it shows (every bitmap bit set, the map zero); the first pixel line of the last
               block row; all-skip frames up to frame 30
  31 .. 34     every fifth block, every block, block 0, the last block: runs that cross the bitmap word boundary have work on both
               sides of it"""
import numpy as np

from index_activity_ref import grid
from msv1_range_clips import Idle

SIZES = [(80, 80), (84, 72), (86, 74), (272, 20), (12, 8), (4, 4)]
FRAMES = 35
SKIP_UNTIL = 31          # all-skip frames fill the clip up to here: frame 31 is bit 31 of bitmap word 0, frame 32 bit 0 of word 1
WG, GROUP = 256, 16      # lanes of a workgroup, lanes of a cell (the kernel's constants)


def marked_cells(cols, rows):
    """The raster indices of the marked cells, clipped to the grid, in order, each once."""
    return sorted({q for q in (0, 3, 4, cols - 1, cols, 15, 16, cols * rows - 1) if 0 <= q < cols * rows})


def last_block_of(r, q, nbx, nby):
    """The last block of cell (r, q) that lies inside the picture (the lane with the highest `sub` that is live)."""
    return min(4 * r + 3, nby - 1) * nbx + min(4 * q + 3, nbx - 1)


def sweep(bits, w, h, seed=7):
    """(frames, keys, marks): the FRAMES frames above, keys (frame 0 only) and marks — (frame, r, q) per marked cell."""
    g = Idle(bits, w, h, seed)
    cols, rows = grid(w, h)
    every = list(range(g.nb))
    frames = [g.key(), g.change(every)]
    marks = []
    for cell in marked_cells(cols, rows):
        r, q = divmod(cell, cols)
        marks.append((len(frames), r, q))
        frames.append(g.change([last_block_of(r, q, g.nbx, g.nby)]))
    frames.append(g.recode(every))
    frames.append(g.first_line_only(g.nby - 1))
    assert len(frames) <= SKIP_UNTIL
    while len(frames) < SKIP_UNTIL:
        frames.append(g.all_skip("full"))
    frames += [g.change(list(range(0, g.nb, 5))), g.change(every), g.change([0]), g.change([g.nb - 1])]
    assert len(frames) == FRAMES
    return frames, [True] + [False] * (FRAMES - 1), marks


def recode_frame(marks):
    """The frame that codes every block again with what it shows: the one after the last mark."""
    return marks[-1][0] + 1


def block_pixels(w, h):
    """(rows, cols): the pixels of every cell that lie inside 4x4 blocks — what a frame that changes every block counts at most."""
    cols, rows = grid(w, h)
    nbx, nby = w // 4, h // 4
    cw = np.clip(4 * nbx - 16 * np.arange(cols), 0, 16)
    ch = np.clip(4 * nby - 16 * np.arange(rows), 0, 16)
    return np.outer(ch, cw)


def check_properties(want, marks, w, h, start=0):
    """What the clip promises, asserted on a map of the whole index by the definition (`want`, index frame t = sweep frame
    start + t) — before any answer of the code under test is looked at."""
    cols, rows = grid(w, h)
    assert want.shape == (FRAMES - start, rows, cols)
    inside = block_pixels(w, h)
    assert np.all(want <= inside[None]), "a cell counts pixels of blocks only"
    if start <= 1:
        every = want[1 - start]
        assert np.all(every > 0), "every cell changes at frame 1"
        if w >= 16 and h >= 16:
            assert every.max() == 256, "a whole cell changes whole"
    for f, r, q in marks:
        if f < start:
            continue
        one = want[f - start]
        assert np.count_nonzero(one) == 1 and 0 < one[r, q] <= 16, f"mark frame {f}: one block of cell ({r}, {q})"
    assert recode_frame(marks) >= start and not want[recode_frame(marks) - start].any(), "recoded blocks change nothing"
    assert not want[recode_frame(marks) + 2 - start:SKIP_UNTIL - start].any(), "all-skip frames change nothing"
    assert all(want[f - start].any() for f in range(SKIP_UNTIL, FRAMES)), "work on both sides of the word boundary"


def caught_by(wrong, marks, cols, rows):
    """The mark frames a wrong geometry (index_activity_ref.msv1_model's `wrong=`) must get wrong, by reasoning:
      "cols_is_4"      cell q' is taken for grid position (q' // 4, q' % 4) and stores at that position too: the marked block of
                       cell (r, q) is still counted, and at the right element, iff some lane group takes itself for (r, q) — q < 4
                       and 4 r + q inside the grid.  Every mark in a cell column >= 4 is lost;
      "one_workgroup"  lanes from 256 on own nothing: every mark in a cell of raster index >= 16 is lost."""
    if wrong == "cols_is_4":
        return [f for f, r, q in marks if not (q < 4 and 4 * r + q < cols * rows)]
    if wrong == "one_workgroup":
        return [f for f, r, q in marks if r * cols + q >= WG // GROUP]
    raise ValueError(wrong)
