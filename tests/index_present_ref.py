"""The numpy reference of jsp_index_present / jsp_sp_index_present (include/jsplayer_amd.h): pictures -> sheet.  Cell i is the window
view_ref.present (filter 0 / 1) or view_area_ref.present_area (filter 2) gives of picture i, laid out by the contract's SHEET rule.
A plain helper module (no tests of its own); it reads nothing from the library."""
import numpy as np

import view_area_ref as va
import view_ref as vr

NEAREST, BILINEAR, AREA = 0, 1, 2
FILTERS = (NEAREST, BILINEAR, AREA)


def window(picture, w, h, win_w, win_h, k, dx, dy, mode, filter, background=0xFF000000):
    """One cell: (win_h, win_w) uint32, top row first."""
    if filter == AREA:
        return va.present_area(picture, w, h, win_w, win_h, k, dx, dy, mode=mode, background=background)
    return vr.present(picture, w, h, win_w, win_h, k, dx, dy, mode=mode, filter=filter, background=background)


def cell_origin(i, cols, win_w, win_h, pitch):
    """Index of cell i's pixel (0, 0) in a sheet of row pitch `pitch`."""
    return (i // cols) * win_h * pitch + (i % cols) * win_w


def sheet_ints(n, cols, win_w, win_h, pitch):
    """The ints the sheet occupies: up to the end of the last row of the last sheet row's cells."""
    return (-(-n // cols) * win_h - 1) * pitch + cols * win_w


def sheet(pictures, w, h, win_w, win_h, k, dx, dy, mode=vr.CANVAS, filter=BILINEAR, background=0xFF000000, cols=1, pitch=None, fill=0, total=None):
    """The windows of `pictures` (each w * h words, bottom-up) `cols` to a sheet row -> a flat uint32 array of `total` words (default:
    what the sheet occupies) in which everything that is not a cell pixel — pitch padding, the cells of the last sheet row past
    n, the words behind the sheet — holds `fill`."""
    n = len(pictures)
    pitch = cols * win_w if pitch is None else pitch
    assert n >= 1 and cols >= 1 and pitch >= cols * win_w
    need = sheet_ints(n, cols, win_w, win_h, pitch)
    total = need if total is None else total
    assert total >= need
    out = np.full(total, fill & 0xFFFFFFFF, dtype=np.uint32)
    cache = {}
    for i, pic in enumerate(pictures):
        key = id(pic)
        if key not in cache:
            cache[key] = window(pic, w, h, win_w, win_h, k, dx, dy, mode, filter, background)
        cell, at = cache[key], cell_origin(i, cols, win_w, win_h, pitch)
        for y in range(win_h):
            out[at + y * pitch: at + y * pitch + win_w] = cell[y]
    return out
