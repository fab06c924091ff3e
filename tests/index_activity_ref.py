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
  * sp_lane_model — the same walk lane by lane, as the launch enumerates workgroups, waves, lanes and chunk positions.

`wrong=` selects a deliberately broken walk that the tests must catch:
  msv1_model: "bit_is_16" (a set bit counts as 16 changed pixels), "no_recompose" (a segment after the first starts from the picture
              before the index instead of composing the picture before its first frame), "cols_is_4" (r = q // 4, qx = q % 4: right
              on a grid of four columns only), "one_workgroup" (lanes from 256 on own nothing: right up to 16 cells only);
  sp_model:   "rect_area" (every pixel under a rectangle counts), "key_ignored" (a key frame inside the run is not an event), "stale"
              (the register takes neither literals nor key pictures), "zeros_counted" (with first = 0 every pixel inside the picture
              counts at frame 0), "open_end" / "open_start" (the mask of a bitmap word to the run reaches frame last + 1 / first - 1:
              with `guard` the map comes with the row in front of it and the row behind it, where such a frame would be stored);
  sp_lane_model: "no_bx_guard" (a wave with bx >= nbx goes on: b names a block of the next row, or none), "chunk_whole" (`inpic` is
              all four bits whenever x0 < X: a key frame's pixels past the row's end are read from the next row of the picture),
              "three_ballots" (the fourth pixel of a chunk is never counted).
Two of them change no count, and the tests say so instead of looking for a wrong map: "open_start" handles frame first - 1 with
P(first - 1) in the register, so that nothing of it differs and nothing is stored; the lanes of a wave that "no_bx_guard" lets
go on have x0 >= 16 nbx >= X, own no pixel and count nothing — what the guard keeps away is the read of a block number past the
tables in the last row of blocks, which sp_lane_model reports in `faults`."""
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
def _sp_words(comp):
    """(writers, keymask): per 32 frames the inter frames that code a rectangle anywhere, and the key frames."""
    nframes = len(comp.key_of)
    nwords = (nframes + 31) // 32
    writers, keymask = [0] * nwords, [0] * nwords
    for f in range(nframes):
        if comp.key_of[f] == f:
            keymask[f >> 5] |= 1 << (f & 31)
        elif f in comp.mask:
            writers[f >> 5] |= 1 << (f & 31)
    return writers, keymask


def _sp_range(wd, first, last, wrong):
    """The kernel's `range`: the bits of word wd that are frames of the run."""
    lo, hi = max(first, 32 * wd), min(last, 32 * wd + 31)
    if wrong == "open_end":
        hi = min(last + 1, 32 * wd + 31)
    if wrong == "open_start" and first > 0:
        lo = max(first - 1, 32 * wd)
    return (0xFFFFFFFF << (lo & 31)) & (0xFFFFFFFF >> (31 - (hi & 31))) & 0xFFFFFFFF


def sp_model(comp, w, h, first, n, wrong=None, guard=False):
    """The kernel's walk over a sp_index_ref.Composer (key_of, key_pic, lit, mask).  (n, rows, cols) uint16; guard: (n + 2, rows,
    cols), the row the kernel would store a frame first - 1 in, the map, the row of a frame first + n — both zero in a right walk."""
    cols, rows = grid(w, h)
    writers, keymask = _sp_words(comp)
    last = first + n - 1
    px = comp.picture(first - 1).reshape(h, w).copy() if first > 0 else np.zeros((h, w), dtype=np.uint32)
    out = np.zeros((n + 2, rows, cols), dtype=np.uint16)
    for wd in range(first >> 5, (last >> 5) + 1):
        rng = _sp_range(wd, first, last, wrong)
        m, km = writers[wd] & rng, keymask[wd] & rng
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
                if wrong != "stale":
                    px[inside] = comp.lit[f][inside]
            else:
                key = comp.key_pic[comp.key_of[f]]
                diff = key != px
                if wrong == "zeros_counted" and f == 0:
                    diff = np.ones((h, w), dtype=bool)
                if wrong != "stale":
                    px = key.copy()
            out[f - first + 1] = cell_sums(diff, w, h)
    return out if guard else out[1:-1]


def sp_lane_model(comp, w, h, first, n, wrong=None, guard=False, faults=None):
    """sp_index_activity_kernel as its launch enumerates it: workgroup (gx, by), wave wv, block bx = 4 gx + wv, a wave with bx >= nbx
    leaves; lane = (row ly, chunk cx0), `mine`, the `inpic` bits; per event the count is the sum of four ballots, one per chunk
    position, and it is stored at the flat element (f - first) * nblocks + b.  The lanes start from P(first - 1) (the backward walk
    has its own model: test_sp_directed_clips_cpu.Walk).  Shape as sp_model.  `faults`: a list that takes what the walk reads outside
    the tables or the picture, as (what, by, bx, number); such a read gives the model nothing (a wave with such a block stops)."""
    nbx, nby = grid(w, h)
    nblocks = nbx * nby
    vec = w % 4 == 0                              # (the index's key pictures are 16-byte aligned)
    writers, keymask = _sp_words(comp)
    nwords = len(writers)
    block_of = (np.arange(h)[:, None] // CELL) * nbx + np.arange(w)[None, :] // CELL
    bitmap = np.zeros((nwords, nblocks), dtype=np.int64)
    for f, mask in comp.mask.items():
        for b in np.unique(block_of[mask]):
            bitmap[f >> 5, b] |= 1 << (f & 31)
    last = first + n - 1
    before = comp.picture(first - 1).reshape(-1) if first > 0 else np.zeros(w * h, dtype=np.uint32)
    flat = np.zeros((n + 2) * nblocks, dtype=np.uint16)
    lane = np.arange(64)
    ly, cx0 = lane >> 2, (lane & 3) * 4
    j = np.arange(4)[None, :]
    for by in range(nby):
        for gx in range((nbx + 3) // 4):
            for wv in range(4):
                bx = 4 * gx + wv
                if bx >= nbx and wrong != "no_bx_guard":
                    continue
                b = by * nbx + bx                 # (without the guard: a block of the next row, or none)
                if b >= nblocks:
                    if faults is not None:
                        faults.append(("block", by, bx, b))
                    continue
                y, x0 = by * 16 + ly, bx * 16 + cx0
                mine = (y < h) & (x0 < w)
                in_row = (x0[:, None] + j) < w
                inpic = mine[:, None] & (in_row | vec)
                at = (y * w + x0)[:, None] + j    # pixel i0 + j
                px = np.where(inpic, before[np.where(inpic, at, 0)], 0).astype(np.uint32)   # (index_compose: 0 outside the picture)
                if wrong == "chunk_whole":
                    inpic = np.repeat(mine[:, None], 4, axis=1)
                    past = inpic & (at >= w * h)
                    if past.any() and faults is not None:
                        faults.append(("pixel", by, bx, int(at[past].min())))
                    inpic = inpic & ~past
                safe = np.where(inpic, at, 0)
                for wd in range(first >> 5, (last >> 5) + 1):
                    rng = _sp_range(wd, first, last, None)
                    m, km = int(bitmap[wd, b]) & rng, keymask[wd] & rng
                    ev = m | km
                    while ev:
                        bit = (ev & -ev).bit_length() - 1
                        ev &= ev - 1
                        f = 32 * wd + bit
                        if (m >> bit) & 1:        # (the rectangle is block b's: it ends with the block's part of the row)
                            inside = inpic & in_row & comp.mask[f].reshape(-1)[safe]
                            v = comp.lit[f].reshape(-1)[safe]
                            diff = inside & (v != px)
                            px = np.where(inside, v, px)
                        else:
                            kx = np.where(inpic, comp.key_pic[comp.key_of[f]].reshape(-1)[safe], px)
                            diff = kx != px
                            px = kx
                        cnt = sum(int(diff[:, k].sum()) for k in range(3 if wrong == "three_ballots" else 4))
                        if cnt:
                            flat[(f - first + 1) * nblocks + b] = cnt
    out = flat.reshape(n + 2, nby, nbx)
    return out if guard else out[1:-1]
