"""The lane arithmetic of the MSVideo1 range kernels (jsplayer_amd/csrc/msv1_seek_kernels.hip) in plain numpy, with the kernels'
control flow — and, by name, the mistakes that arithmetic invites.  No GPU; tests/test_msv1_row_sweep_cpu.py holds both models to
the oracle on the clips of msv1_row_sweep_clips.py and says which clip catches which mistake.

rows_and_stop   rows[] and stop[] of msv1_coded_bitmap_kernel, wave by wave, then the host loop of jsp_index_build
                (msv1_seek.cpp, "per-row block_changes after every frame") to the block_changes after every frame
uncovered_order the pixel of lane r past the last block: uncovered_pixel (msv1_block_io.h)"""
import numpy as np

WAVE = 64
NO_STOP = 0xFFFFFFFF

ROW_MISTAKES = ("ladder_stops_at_16", "no_row_guard", "no_lane0_store", "first_lane_of_wave_only", "stop_is_max", "stop_row_not_reset",
                "div_by_64")
ORDER_MISTAKES = ("rows_first", "strip_row_by_X", "bottom_from_cy_minus_1", "no_copy")


def shfl_down(v, d):
    """__shfl_down over a wave of 64: lane l reads lane l + d, or itself when there is none."""
    out = v.copy()
    out[:WAVE - d] = v[d:]
    return out


def shfl_up(v, d):
    """__shfl_up over a wave of 64: lane l reads lane l - d, or itself when there is none."""
    out = v.copy()
    out[d:] = v[:WAVE - d]
    return out


def wave_rows_and_stop(coded, untouched, first, nblocks, nbx, nby, rows, wrong=None):
    """One wave of msv1_coded_bitmap_kernel on one frame (one bit of the kernel's words): lanes first .. first + 63.  ORs into
    rows[] what the wave's storing lanes hold and returns the wave's candidate for stop (NO_STOP: none).

    wrong:  ladder_stops_at_16        the shuffle ladder ends at d = 16
            no_row_guard              the OR crosses a row start (orow == row not asked)
            no_lane0_store            only a lane with another row above it stores (lane 0 reads itself from __shfl_up: it never does)
            first_lane_of_wave_only   only lane 0 stores
            div_by_64                 the lane's row is blk / 64"""
    lane = np.arange(WAVE)
    gid = first + lane
    inside = gid < nblocks
    blk = np.where(inside, gid, 0)
    row = np.where(inside, blk // (WAVE if wrong == "div_by_64" else nbx), -1)
    v = np.where(inside, coded[blk], False)
    u = np.where(inside, untouched[blk], False)
    d = 1
    while d < (32 if wrong == "ladder_stops_at_16" else WAVE):
        o, orow = shfl_down(v, d), shfl_down(row, d)
        take = lane + d < WAVE
        if wrong != "no_row_guard":
            take = take & (orow == row)
        v = v | (take & o)
        d <<= 1
    up = shfl_up(row, 1)
    if wrong == "no_lane0_store":
        stores = up != row
    elif wrong == "first_lane_of_wave_only":
        stores = lane == 0
    else:
        stores = (lane == 0) | (up != row)
    for l in np.flatnonzero(inside & v & stores):
        if row[l] < nby:        # (div_by_64 can name a row past the last: that store would leave the array)
            rows[row[l]] = True
    return int(blk[np.flatnonzero(u)[0]]) if u.any() else NO_STOP


def rows_and_stop(coded, untouched, nbx, nby, noop=None, wrong=None):
    """block_changes (row r in bit r) after every frame of an index whose frame f codes the blocks coded[f] and leaves the blocks
    untouched[f] alone (both n x nblocks bool, from msv1_range_clips.coded_blocks), starting from no flag set.  noop[f]: the frame
    is an early-out (it walks nothing).

    wrong (besides wave_rows_and_stop's):  stop_is_max          the waves' candidates are joined by a maximum
                                           stop_row_not_reset   the host loop stops one row short of the stop's row"""
    n, nblocks = coded.shape
    now = np.zeros(nby, dtype=bool)
    out = []
    for f in range(n):
        rows = np.zeros(nby, dtype=bool)
        cands = []
        for first in range(0, nblocks, WAVE):
            s = wave_rows_and_stop(coded[f], untouched[f], first, nblocks, nbx, nby, rows, wrong)
            if s != NO_STOP:
                cands.append(s)
        stop = NO_STOP if not cands else max(cands) if wrong == "stop_is_max" else min(cands)
        if not (noop is not None and noop[f]) and nblocks > 0:
            reached = min(min(stop, nblocks) // nbx, nby - 1)
            if wrong == "stop_row_not_reset" and stop != NO_STOP:
                reached -= 1
            now[:reached + 1] = rows[:reached + 1]
        out.append(sum(1 << r for r in np.flatnonzero(now)))
    return out


def uncovered_order(w, h, wrong=None):
    """The pixel index of every lane r = 0 .. nrem - 1 past the last block, as uncovered_pixel computes it (an int64 array; an index
    outside the picture is kept as it comes out).

    wrong:  rows_first               the two branches swapped: lanes below (X - cx) * cy take the rows formula, the rest the strip's
            strip_row_by_X           the strip's row is r / X, not r / (X - cx)
            bottom_from_cy_minus_1   the rows begin one pixel row early
            no_copy                  no lane copies anything (an empty order)"""
    cx, cy = (w // 4) * 4, (h // 4) * 4
    sw = w - cx
    rw = sw * cy
    nrem = rw + w * (h - cy)
    if wrong == "no_copy":
        return np.zeros(0, dtype=np.int64)
    out = np.zeros(nrem, dtype=np.int64)
    for r in range(nrem):
        in_strip = r < rw
        if wrong == "rows_first":
            in_strip = not in_strip
        if in_strip:
            if sw == 0:           # (only a swapped branch comes here without a strip: the kernel would divide by zero)
                out[r] = -1
                continue
            q = r if wrong != "rows_first" else r - rw
            out[r] = (q // (w if wrong == "strip_row_by_X" else sw)) * w + cx + q % sw
        else:
            q = r - rw if wrong != "rows_first" else r
            out[r] = (cy - 1 if wrong == "bottom_from_cy_minus_1" else cy) * w + q
    return out


def copy_uncovered(before, dst, w, h, wrong=None):
    """`dst` after the lanes past the last block have copied their pixel from `before` (indices outside the picture dropped)."""
    out = np.array(dst)
    order = uncovered_order(w, h, wrong)
    order = order[(order >= 0) & (order < w * h)]
    out[order] = np.asarray(before)[order]
    return out
