"""Reference for the distance map of a seek index (jsp_index_distance / jsp_sp_index_distance) — a helper module, numpy only, no
tests of its own.

  * distance — THE DEFINITION, straight from whole pictures: element [k, r, q] is the number of pixels of the 16 x 16 cell (r, q)
    (index_activity_ref.grid / cell_sums) whose word differs between picture k and ONE reference picture.  whole_blocks_only
    (MSVideo1): only pixels inside whole 4 x 4 blocks are compared — the X % 4 / Y % 4 remainder pixels are masked out.
  * whole_block_mask — that mask.
  * brute — the same numbers the slow way, pixel by pixel into a dict of cells: what test_index_distance_ref_cpu.py holds the
    definition against.
  * msv1_reference — R for an MSVideo1 case: P(ref) of index_activity_ref.msv1_pictures, ref = -1 the picture before."""
import numpy as np

import index_activity_ref as ar


def whole_block_mask(w, h):
    """(h, w) bool: the pixels inside whole 4 x 4 blocks."""
    out = np.zeros((h, w), dtype=bool)
    out[:h // 4 * 4, :w // 4 * 4] = True
    return out


def distance(pictures, ref, w, h, whole_blocks_only=False):
    """THE DEFINITION.  pictures: P(first) .. P(first + n - 1), each (h * w,) words; ref: R, (h * w,) words.  (n, rows, cols) uint16."""
    cols, rows = ar.grid(w, h)
    out = np.zeros((len(pictures), rows, cols), dtype=np.uint16)
    r = np.asarray(ref).reshape(-1).view(np.uint32)
    assert r.size == w * h
    keep = whole_block_mask(w, h).reshape(-1) if whole_blocks_only else np.ones(w * h, dtype=bool)
    for k, pic in enumerate(pictures):
        cur = np.asarray(pic).reshape(-1).view(np.uint32)
        out[k] = ar.cell_sums((cur != r) & keep, w, h)
    return out


def brute(pictures, ref, w, h, whole_blocks_only=False):
    """distance(), pixel by pixel in plain Python: no reshape, no cell_sums."""
    cols, rows = ar.grid(w, h)
    out = np.zeros((len(pictures), rows, cols), dtype=np.uint16)
    r = [int(v) & 0xFFFFFFFF for v in np.asarray(ref).reshape(-1)]
    xs, ys = (w // 4 * 4, h // 4 * 4) if whole_blocks_only else (w, h)
    for k, pic in enumerate(pictures):
        p = [int(v) & 0xFFFFFFFF for v in np.asarray(pic).reshape(-1)]
        for y in range(ys):
            for x in range(xs):
                if p[y * w + x] != r[y * w + x]:
                    out[k, y // 16, x // 16] += 1
    return out


def msv1_reference(p_before, p, ref):
    """R = P(ref) of an MSVideo1 index: p_before for -1."""
    return p_before if ref < 0 else p[ref]
