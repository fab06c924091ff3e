"""Reference for the window a viewer shows of a frame: the view geometry of the original player's Main (Main.hx:282-286, 301-318) and
this project's resampling rule (include/jsplayer_amd.h, jsp_display_present), restated in numpy from their descriptions — not from the
kernel.  Used by the CPU tests of jsp_view_matrix / player.View and as the bit-exact yardstick of the GPU tests of jsp_display_present.

Coordinates.  The display matrix is  screen (sx, sy) = (k x - dx, -k y + win_h + dy).  With F(v) = floor(v * 65536 + 0.5) in doubles,
step = F(1 / k), ax = F((0.5 + dx) / k), ay = F((win_h + dy - 0.5) / k); output pixel (ox, oy) has the 16.16 bitmap coordinates
X = ax + ox * step, Y = ay - oy * step, and shows the picture when 0 <= X < frame_w * 65536 and 0 <= Y < frame_h * 65536, else the
background.  Bitmap row y is buffer row y (the buffer is bottom-up; the matrix's -k flips it)."""
import math

import numpy as np

NEAREST, BILINEAR = 0, 1
CANVAS, CANVAS_RGB15, SETPIXELS, SETPIXELS_RGB15 = 0, 1, 2, 3


def fit(a, mn, mx):
    """Main.hx:282-286, as written (mx below mn is not special-cased)."""
    if a < mn:
        return mn
    if a > mx:
        return mx
    return a


def view_matrix(frame_w, frame_h, win_w, win_h, zoom, hor_view_pos, ver_view_pos):
    """Main.on_stage_resize, Main.hx:301-315, in Python floats (IEEE doubles): (k, dx, dy).  zoom 0 is "Fit"."""
    vx, vy, width, height = float(frame_w), float(frame_h), float(win_w), float(win_h)
    kx, ky = width / vx, height / vy
    k = min(kx, ky)
    dx = dy = 0.0
    if zoom > 0:
        k = float(zoom)
        dx = vx * k * hor_view_pos - width / 2
        dx = fit(dx, 0.0, vx * k - width)
        dy = vy * k * (1 - ver_view_pos) - height / 2
        dy = fit(dy, 0.0, vy * k - height)
    return k, dx, dy


def convert(c, mode):
    """The four conversions of Manager.fill_bitmap_data (Manager.hx:340, 351, 370, 379) on uint32 words."""
    c = np.asarray(c).astype(np.uint32)
    if mode == CANVAS:
        return np.uint32(0xFF000000) | ((c & np.uint32(0xFF)) << np.uint32(16)) | (c & np.uint32(0xFF00)) | ((c >> np.uint32(16)) & np.uint32(0xFF))
    if mode == CANVAS_RGB15:
        return np.uint32(0xFF000000) | (c << np.uint32(3))
    if mode == SETPIXELS:
        return np.uint32(0xFF000000) | c
    if mode == SETPIXELS_RGB15:
        return c << np.uint32(11)
    raise ValueError(mode)


def fixed16(v):
    """F(v) as a Python integer.  Values beyond +-2^62 are held there: ox * step stays below 2^36, so such a window lies outside
    the picture whichever of the two integers is used, and int64 arrays can carry it."""
    f = math.floor(v * 65536.0 + 0.5) if math.isfinite(v) else (1 << 62 if v > 0 else -(1 << 62))
    return max(-(1 << 62), min(1 << 62, f))


def coordinates(win_w, win_h, k, dx, dy):
    """(X of every output column, Y of every output row) as int64 arrays."""
    step = fixed16(1.0 / k)
    ax = fixed16((0.5 + dx) / k)
    ay = fixed16((win_h + dy - 0.5) / k)
    X = np.array([ax + ox * step for ox in range(win_w)], dtype=np.int64)
    Y = np.array([ay - oy * step for oy in range(win_h)], dtype=np.int64)
    return X, Y


def present(frame, frame_w, frame_h, win_w, win_h, k, dx, dy, mode=CANVAS, filter=BILINEAR, background=0xFF000000):
    """The window as a (win_h, win_w) uint32 array, top row first.  `frame`: frame_w * frame_h words (int32 or uint32), bottom-up."""
    img = convert(np.asarray(frame).reshape(-1)[:frame_w * frame_h].view(np.uint32), mode).reshape(frame_h, frame_w)
    X, Y = coordinates(win_w, win_h, k, dx, dy)
    covered = ((Y >= 0) & (Y < frame_h * 65536))[:, None] & ((X >= 0) & (X < frame_w * 65536))[None, :]
    if filter == NEAREST:
        xi = np.clip(X >> 16, 0, frame_w - 1)          # (clipped only so that uncovered pixels index something)
        yi = np.clip(Y >> 16, 0, frame_h - 1)
        shown = img[yi[:, None], xi[None, :]]
    elif filter == BILINEAR:
        U, V = X - 32768, Y - 32768
        x0, y0 = U >> 16, V >> 16
        wx = ((U & 0xFFFF) >> 8)[None, :]
        wy = ((V & 0xFFFF) >> 8)[:, None]
        xa, xb = np.clip(x0, 0, frame_w - 1)[None, :], np.clip(x0 + 1, 0, frame_w - 1)[None, :]
        ya, yb = np.clip(y0, 0, frame_h - 1)[:, None], np.clip(y0 + 1, 0, frame_h - 1)[:, None]
        shown = np.zeros((win_h, win_w), dtype=np.uint32)
        for byte in range(4):
            plane = ((img >> np.uint32(8 * byte)) & np.uint32(0xFF)).astype(np.int64)
            p00, p10, p01, p11 = plane[ya, xa], plane[ya, xb], plane[yb, xa], plane[yb, xb]
            v = (p00 * (256 - wx) * (256 - wy) + p10 * wx * (256 - wy) + p01 * (256 - wx) * wy + p11 * wx * wy + 32768) >> 16
            shown |= v.astype(np.uint32) << np.uint32(8 * byte)
    else:
        raise ValueError(filter)
    return np.where(covered, shown, np.uint32(background & 0xFFFFFFFF)).astype(np.uint32)
