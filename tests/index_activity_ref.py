"""Reference for the activity map of a seek index (jsp_index_activity / jsp_sp_index_activity) — a helper module, numpy only, no
tests of its own.

  * activity — THE DEFINITION, straight from whole pictures: element [k, r, q] is the number of pixels of the 16 x 16 cell (r, q)
    whose word differs between picture k and the picture before it.
  * msv1_pictures — THE PICTURE P(t) of an MSVideo1 index from the oracle's sequential run (msv1_range_clips.truth_run): the
    oracle's picture where the index has one, zeros in a block nothing has coded yet when there is no picture before the range.
  * msv1_model — msv1_index_activity_kernel's walk over a plan of msv1_range_clips (which frame codes which block): a lane per 4x4
    block enumerated as the launch enumerates them — lane gid of ceil(cells * 16 / 256) workgroups of 256 belongs to cell
    q = gid >> 4 of the grid in raster order (r = q // cols, qx = q - r * cols) and is its lane sub = gid & 15, a group with
    q >= cols * rows owns nothing — with the lanes of an edge cell that have no block alive, the bitmap words masked to the
    segment's frames and ORed over the cell, the segment that composes the picture before its own first frame, the `have` flag
    (a block nothing has coded and nothing lies under is zeros).  As in msv1_index_play_ref the model is about WHICH code a lane decodes
    and what it compares it with, not about the decode: a block's pixels as frame f codes them are the oracle's after frame f.
  * sp_model — sp_index_activity_kernel's walk over what sp_index_ref.Composer keeps (key pictures; per inter frame a literal
    image and the mask of its rectangles): the events bitmap | keymask of the run's frames word by word, literals compared and
    taken under the rectangle mask, a key frame compared with and reloaded from its picture.

`wrong=` selects a deliberately broken walk that the tests must catch:
  msv1_model: "bit_is_16" (a set bit counts as 16 changed pixels), "no_recompose" (a segment after the first starts from the picture
              before the index instead of composing the picture before its first frame), "cols_is_4" (r = q // 4, qx = q % 4: right
              on a grid of four columns only), "one_workgroup" (lanes from 256 on own nothing: right up to 16 cells only);
  sp_model:   "rect_area" (every pixel under a rectangle counts), "key_ignored" (a key frame inside the run is not an event)."""
import numpy as np

from msv1_index_play_ref import _top_bit, bitmap_words, index_last_writer, segment_length, to_blocks

CELL = 16
WG, GROUP = 256, 16   # msv1_index_activity_kernel: lanes of a workgroup, lanes of a cell


def grid(w, h):
    """(cols, rows)"""
    return (w + CELL - 1) // CELL, (h + CELL - 1) // CELL


def cell_sums(diff, w, h):
    """(h, w) bool -> (rows, cols) counts."""
    cols, rows = grid(w, h)
    full = np.zeros((rows * CELL, cols * CELL), dtype=np.int64)
    full[:h, :w] = np.asarray(diff).reshape(h, w)
    return full.reshape(rows, CELL, cols, CELL).sum(axis=(1, 3))


def activity(pictures, before, w, h):
    """THE DEFINITION.  pictures: P(first) .. P(first + n - 1), each (h * w,) words; before: P(first - 1).  (n, rows, cols) uint16."""
    cols, rows = grid(w, h)
    out = np.zeros((len(pictures), rows, cols), dtype=np.uint16)
    prev = np.asarray(before).reshape(-1).view(np.uint32)
    for k, pic in enumerate(pictures):
        cur = np.asarray(pic).reshape(-1).view(np.uint32)
        out[k] = cell_sums(cur != prev, w, h)
        prev = cur
    return out


# ---- MSVideo1 ----------------------------------------------------------------------------------------------------------------------
def block_mask_to_pixels(mask, w, h):
    """(nb,) bool per 4x4 block -> (h * w,) bool per pixel (the X % 4 / Y % 4 remainder pixels: False)."""
    nbx, nby = w // 4, h // 4
    out = np.zeros((h, w), dtype=bool)
    if nbx and nby:
        out[:nby * 4, :nbx * 4] = np.repeat(np.repeat(np.asarray(mask).reshape(nby, nbx), 4, axis=0), 4, axis=1)
    return out.reshape(-1)


def msv1_pictures(truth_pics, coded, w, h, before=None):
    """P(-1), [P(0) .. P(n - 1)] of an index over n frames.  truth_pics[t]: the oracle's picture after frame t of the index's range
    (None: it has none yet); coded: (n, nb) which frame codes which block; before: the picture before the range or None.  With a
    picture before the range the oracle's picture IS P(t) (every destination starts out holding the picture before it).  Without one
    the oracle's buffers hold whatever they held where nothing was coded: P(t) has zeros there."""
    n = coded.shape[0]
    if before is not None:
        b = np.asarray(before, dtype=np.int32).reshape(-1)
        return b, [b if truth_pics[t] is None else np.asarray(truth_pics[t], dtype=np.int32) for t in range(n)]
    zeros = np.zeros(w * h, dtype=np.int32)
    out, defined = [], np.zeros(coded.shape[1], dtype=bool)
    for t in range(n):
        defined = defined | coded[t]
        out.append(zeros if truth_pics[t] is None else np.where(block_mask_to_pixels(defined, w, h), np.asarray(truth_pics[t], dtype=np.int32), 0))
    return zeros, out


def msv1_model(coded, block_pics, w, h, first, n, segs=1, before=None, wrong=None):
    """The kernel's walk.  coded: (frames, nb); block_pics[f]: (nb, 16) pixels of the oracle's picture after frame f; before: the
    (h * w,) picture before the range or None.  (n, rows, cols) uint16."""
    bm = bitmap_words(coded)
    nbx, nby = w // 4, h // 4
    nb = nbx * nby
    cols, rows = grid(w, h)
    out = np.zeros((n, rows, cols), dtype=np.uint16)
    flat = out.reshape(-1)
    nwg = (cols * rows * GROUP + WG - 1) // WG
    under = to_blocks(before, w, h).astype(np.int32) if before is not None and nb else None
    seg = segment_length(n, segs)
    for k0 in range(0, n, seg):
        k1 = min(n, k0 + seg)
        t0, t1 = first + k0, first + k1 - 1
        # compose P(t0 - 1): the last writer <= t0 - 1, else the picture before the range, else zeros (`have` false)
        px = np.zeros((nb, 16), dtype=np.int32)
        have = np.zeros(nb, dtype=bool)
        if under is not None:
            px, have = under.copy(), np.ones(nb, dtype=bool)
        if t0 > 0 and nb and not (wrong == "no_recompose" and k0 > 0):
            m, wd = index_last_writer(bm, t0 - 1)
            for b in np.nonzero(m != 0)[0]:
                px[b] = block_pics[int(32 * wd[b] + _top_bit(m[b:b + 1])[0])][b]
                have[b] = True
        px[~have] = 0
        for g0 in range(0, nwg * WG, GROUP):
            lanes, r, qx = [], 0, 0   # the group's lanes that go on: (block, live); all 16 or none — q, r, qx are the same for the 16
            for gid in range(g0, g0 + GROUP):
                q, sub = gid >> 4, gid & 15
                if q >= cols * rows or (wrong == "one_workgroup" and gid >= WG):
                    continue   # (a tail group leaves)
                r, qx = (q // 4, q % 4) if wrong == "cols_is_4" else (q // cols, q - (q // cols) * cols)
                by, bx = r * 4 + (sub >> 2), qx * 4 + (sub & 3)
                live = by < nby and bx < nbx
                lanes.append((by * nbx + bx if live else 0, live))
            if not lanes:
                continue
            assert len(lanes) == GROUP
            for wd in range(t0 >> 5, (t1 >> 5) + 1):
                lo, hi = max(t0, 32 * wd), min(t1, 32 * wd + 31)
                rng = (0xFFFFFFFF << (lo & 31)) & (0xFFFFFFFF >> (31 - (hi & 31))) & 0xFFFFFFFF
                mine = [int(bm[wd, b]) & rng if live else 0 for b, live in lanes]
                union = 0
                for v in mine:
                    union |= v
                while union:
                    bit = (union & -union).bit_length() - 1
                    union &= union - 1
                    f, cnt = 32 * wd + bit, 0
                    for (b, live), v in zip(lanes, mine):
                        if (v >> bit) & 1:
                            nx = block_pics[f][b]
                            cnt += 16 if wrong == "bit_is_16" else int(np.count_nonzero(nx != px[b]))
                            px[b] = nx
                    at = ((f - first) * rows + r) * cols + qx   # the first lane's store, a flat element as the kernel addresses it
                    if cnt and at < flat.size:                  # (a wrong r can point behind the map: the model drops that store)
                        flat[at] = cnt
    return out


# ---- ScreenPressor ------------------------------------------------------------------------------------------------------------------
def sp_model(comp, w, h, first, n, wrong=None):
    """The kernel's walk over a sp_index_ref.Composer (key_of, key_pic, lit, mask).  (n, rows, cols) uint16."""
    cols, rows = grid(w, h)
    nframes = len(comp.key_of)
    nwords = (nframes + 31) // 32
    writers = np.zeros(nwords, dtype=np.uint64)   # frames with a rectangle anywhere (per block in the kernel: an empty block's mask is empty)
    keymask = np.zeros(nwords, dtype=np.uint64)
    for f in range(nframes):
        if comp.key_of[f] == f:
            keymask[f >> 5] |= np.uint64(1 << (f & 31))
        elif f in comp.mask:
            writers[f >> 5] |= np.uint64(1 << (f & 31))
    last = first + n - 1
    px = comp.picture(first - 1).reshape(h, w).copy() if first > 0 else np.zeros((h, w), dtype=np.uint32)
    out = np.zeros((n, rows, cols), dtype=np.uint16)
    for wd in range(first >> 5, (last >> 5) + 1):
        lo, hi = max(first, 32 * wd), min(last, 32 * wd + 31)
        rng = (0xFFFFFFFF << (lo & 31)) & (0xFFFFFFFF >> (31 - (hi & 31))) & 0xFFFFFFFF
        m, km = int(writers[wd]) & rng, int(keymask[wd]) & rng
        if wrong == "key_ignored":
            km = 0
        ev = m | km
        while ev:
            bit = (ev & -ev).bit_length() - 1
            ev &= ev - 1
            f = 32 * wd + bit
            if (m >> bit) & 1:
                inside = comp.mask[f]
                diff = inside.copy() if wrong == "rect_area" else inside & (comp.lit[f] != px)
                px[inside] = comp.lit[f][inside]
            else:
                key = comp.key_pic[comp.key_of[f]]
                diff = key != px
                px = key.copy()
            out[f - first] = cell_sums(diff, w, h)
    return out
