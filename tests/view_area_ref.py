"""Reference for jsp_display_present_area: the area-averaged window of a frame, restated in numpy from the rule in
include/jsplayer_amd.h — not from the kernel.  A plain helper module (no tests of its own): the bit-exact yardstick of
tests/test_present_area_gpu.py, with the hand answers and the named mistakes checked in tests/test_view_area_ref_cpu.py.

The rule.  Geometry as tests/view_ref.py: X = ax + ox * step, Y = ay - oy * step (16.16); a pixel shows the picture when its centre
lies inside.  Per axis, in 1/256 source pixels: s = step >> 8, c = X >> 8, lo = c - (s >> 1), hi = lo + s, clipped to the picture
(lo', hi'); source column x weighs wx(x) = max(0, min(hi', (x + 1) * 256) - max(lo', x * 256)), Wx = hi' - lo'; rows likewise.  Each
byte of the CONVERTED words: S = sum_y wy(y) sum_x wx(x) p(x, y), D = Wx * Wy, result = (S + (D >> 1)) // D.

Separable: a (win_h, frame_h) weight matrix WY and a (frame_w, win_w) matrix WX, S = WY @ plane @ WX in int64 (S < 2^36).

MISTAKES names the ways a kernel could get the rule wrong that the shared CASES must tell from the truth."""
from __future__ import annotations

from collections import namedtuple

import numpy as np

from view_ref import convert, coordinates, fixed16, view_matrix

CANVAS, CANVAS_RGB15, SETPIXELS, SETPIXELS_RGB15 = 0, 1, 2, 3
MODES = (CANVAS, CANVAS_RGB15, SETPIXELS, SETPIXELS_RGB15)
RGB15 = (CANVAS_RGB15, SETPIXELS_RGB15)

MISTAKES = (
    "truncate",              # no + (D >> 1): the quotient rounded down
    "unclipped",             # D = s * s at the picture's edges, where the footprint is clipped
    "centre16",              # c from (X >> 16) << 8: the footprint centred on a whole pixel
    "wrap32",                # S reduced mod 2^32 (a 32-bit accumulator)
    "edges_swapped",         # the weights of a footprint's first and last column (row) exchanged
    "cover_by_footprint",    # picture where the footprint touches the picture, not where the centre lies inside
)


def axis_weights(C, step, size, mistake=None):
    """For the 16.16 centres `C` (int64) of one axis of a picture `size` pixels long: (weights (len(C), size) int64, W (len(C),)
    int64, covered (len(C),) bool).  Rows of uncovered centres are zero, with W = 1."""
    C = np.asarray(C, dtype=np.int64)
    s = step >> 8
    covered = (C >= 0) & (C < size * 65536)
    c = ((C >> 16) << 8) if mistake == "centre16" else (C >> 8)
    lo = c - (s >> 1)
    hi = lo + s
    if mistake == "cover_by_footprint":
        covered = (hi > 0) & (lo < size * 256)
    lo_c, hi_c = np.maximum(lo, 0), np.minimum(hi, size * 256)
    x = np.arange(size, dtype=np.int64)[None, :]
    w = np.maximum(0, np.minimum(hi_c[:, None], (x + 1) * 256) - np.maximum(lo_c[:, None], x * 256))
    W = hi_c - lo_c
    if mistake == "edges_swapped":
        for i in np.nonzero(covered)[0]:
            nz = np.nonzero(w[i])[0]
            if len(nz) > 1:
                w[i, nz[0]], w[i, nz[-1]] = w[i, nz[-1]], w[i, nz[0]]
    if mistake == "unclipped":
        W = np.full_like(W, s)
    w[~covered] = 0
    W = np.where(covered, W, 1)
    return w, W, covered


def present_area(frame, frame_w, frame_h, win_w, win_h, k, dx, dy, mode=CANVAS, background=0xFF000000, mistake=None):
    """The window as a (win_h, win_w) uint32 array, top row first.  `frame`: frame_w * frame_h words (int32 or uint32), bottom-up."""
    assert mistake is None or mistake in MISTAKES, mistake
    img = convert(np.asarray(frame).reshape(-1)[:frame_w * frame_h].view(np.uint32), mode).reshape(frame_h, frame_w)
    X, Y = coordinates(win_w, win_h, k, dx, dy)
    step = fixed16(1.0 / k)
    wx, Wx, in_x = axis_weights(X, step, frame_w, mistake)
    wy, Wy, in_y = axis_weights(Y, step, frame_h, mistake)
    D = Wy[:, None] * Wx[None, :]
    shown = np.zeros((win_h, win_w), dtype=np.uint32)
    for byte in range(4):
        plane = ((img >> np.uint32(8 * byte)) & np.uint32(0xFF)).astype(np.int64)
        S = wy @ plane @ wx.T
        if mistake == "wrap32":
            S = S & 0xFFFFFFFF
        v = (S + (0 if mistake == "truncate" else (D >> 1))) // D
        shown |= (v & 0xFF).astype(np.uint32) << np.uint32(8 * byte)
    covered = in_y[:, None] & in_x[None, :]
    return np.where(covered, shown, np.uint32(background & 0xFFFFFFFF)).astype(np.uint32)


# ---- the shared cases ---------------------------------------------------------------------------------------------------------------
Case = namedtuple("Case", "part frame window k dx dy mode pixels seed")
# frame, window: (w, h); pixels: "random" (24-bit words; 15-bit for the RGB15 modes) or "white" (every word 0xFFFFFF)

FRAMES = ((37, 23), (64, 48), (100, 52))
WINDOWS = ((1, 1), (7, 5), (41, 29), (30, 30))          # 30 x 30: Fit leaves background bars
ZOOMS = (1.0, 2.0, 3.5, 64.0, 0.37, 1 / 2, 1 / 3, 1 / 4, 2 / 3)
POSITIONS = ((0.5, 0.5), (0.0, 0.0), (1.0, 1.0), (0.3, 0.8))
SEAM_FRAME = (600, 40)                                  # at k = 1/2 into 300 x 20, and windows across the workgroup boundaries
SEAM_WIDTHS = (300, 255, 256, 257, 259)
SEAM_HEIGHTS = (20, 8, 9, 17)


def frame_words(case):
    w, h = case.frame
    if case.pixels == "white":
        return np.full(w * h, 0xFFFFFF, dtype=np.uint32)
    bits = 15 if case.mode in RGB15 else 24
    return np.random.default_rng(case.seed).integers(0, 1 << bits, size=w * h, dtype=np.uint64).astype(np.uint32)


def _cases():
    out = []
    n = 0
    for fi, (fw, fh) in enumerate(FRAMES):
        for (ww, wh) in WINDOWS:
            views = [view_matrix(fw, fh, ww, wh, 0, 0.5, 0.5)]
            for z in ZOOMS:
                for (hor, ver) in POSITIONS:
                    views.append(view_matrix(fw, fh, ww, wh, z, hor, ver))
            for (k, dx, dy) in views:
                if not 1 / 64 <= k <= 64:                   # (Fit of 100 x 52 into 1 x 1: the call refuses such a k)
                    continue
                out.append(Case("views", (fw, fh), (ww, wh), k, dx, dy, MODES[n % 4], "random", 100 + fi))
                n += 1
    # all four picture edges clipped: the window larger than the zoomed picture and pushed half off it, each way
    for m, mode in enumerate(MODES):
        for (k, dx, dy) in ((1 / 3, -2.25, -1.75), (1 / 3, 4.5, 3.25), (0.37, -1.5, 2.5), (2 / 3, 3.0, -2.0), (1 / 4, -0.5, -0.5)):
            out.append(Case("edges", (37, 23), (41, 29), k, dx, dy, mode, "random", 200 + m))
    # every mode on one strongly minified view and on the crop
    for mode in MODES:
        out.append(Case("modes", (100, 52), (41, 29), 1 / 3, 2.0, 1.0, mode, "random", 300 + mode))
        out.append(Case("modes", (64, 48), (41, 29), 1.0, 5.0, 3.0, mode, "random", 300 + mode))
    # large sums: S beyond 32 bits
    out.append(Case("large", (130, 130), (2, 2), 1 / 64, 0.0, 0.0, CANVAS, "white", 0))
    out.append(Case("large", (130, 130), (2, 2), 1 / 64, 0.0, 0.0, SETPIXELS, "white", 0))
    k, dx, dy = view_matrix(200, 120, 10, 6, 0, 0.5, 0.5)
    out.append(Case("large", (200, 120), (10, 6), k, dx, dy, CANVAS, "white", 0))
    out.append(Case("large", (200, 120), (10, 6), k, dx, dy, CANVAS, "random", 400))
    out.append(Case("large", (200, 120), (10, 6), k, dx, dy, SETPIXELS_RGB15, "random", 401))
    out.append(Case("large", (130, 130), (3, 3), 1 / 64, 0.3, 0.6, SETPIXELS, "random", 402))
    # footprints at and just past 2 and 4 source pixels (s = 512, 513, 1024, 1025), off the pixel grid: 3, 4, 5 and 6 columns touched
    for m, k in enumerate((1 / 2, 0.499, 1 / 4, 0.2497)):
        out.append(Case("taps", (100, 52), (41, 29), k, 0.3, 0.2, MODES[m], "random", 600 + m))
        out.append(Case("taps", (100, 52), (41, 29), k, 7.0, 2.0, CANVAS, "random", 610 + m))
    # workgroup seams
    fw, fh = SEAM_FRAME
    for ww in SEAM_WIDTHS:
        for wh in SEAM_HEIGHTS:
            out.append(Case("seams", (fw, fh), (ww, wh), 1 / 2, 0.0, 0.0, CANVAS, "random", 500))
    out.append(Case("seams", (fw, fh), (259, 17), 1 / 2, 20.5, 1.25, CANVAS_RGB15, "random", 501))
    return out


CASES = _cases()
