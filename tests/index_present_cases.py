"""What the GPU tests of jsp_index_present and jsp_sp_index_present share: the call through the C ABI (any pitch, any `out`), the
windows, and the comparison of a whole poisoned buffer with tests/index_present_ref.sheet.  A plain helper module.

The kernels' constants, stated here and not imported: a workgroup of 256 lanes owns a rectangle of at most 64 x 64 output pixels (four
to a lane), composes source TILES of 64 x 64 pixels whose origin is a multiple of ALIGN (4 for MSVideo1, 16 for ScreenPressor) and
loops over tiles where the rectangle's taps reach further — which the host's choice of rectangle avoids above k of about 1/14."""
import ctypes as C

import numpy as np

import index_present_ref as ipr
import view_ref as vr
from jsplayer_amd import CodecError
from jsplayer_amd import _native as N

POISON = 0x5A5A5A5A
TILE, WG_LANES, RUN = 64, 256, 4
MODES = (vr.CANVAS, vr.CANVAS_RGB15, vr.SETPIXELS, vr.SETPIXELS_RGB15)
BG = 0xFF102030


def dev_buf(n, fill=POISON, offset=0):
    """n words on the device; offset: that many ints past a 16-byte boundary."""
    import torch
    return torch.full((n + 4,), fill, dtype=torch.int32, device="cuda")[offset:offset + n]


def call(fn, codec, idx, frames, out, win_w, win_h, pitch, cols, k, dx, dy, mode, filter, background=BG, out_ints=None):
    """The C call itself (fn: "index_present" / "sp_index_present"); CodecError with jsp_last_error() when it refuses."""
    arr = (C.c_int * max(len(frames), 1))(*frames)
    ptr = out.ctypes.data if isinstance(out, np.ndarray) else out.data_ptr()
    ints = (out.size if isinstance(out, np.ndarray) else out.numel()) if out_ints is None else out_ints
    rc = getattr(N.lib(), "jsp_" + fn)(codec._h, idx._h, len(frames), arr, C.c_void_p(ptr), ints, win_w, win_h, pitch, cols, float(k), float(dx), float(dy),
                                       mode, filter, background)
    if rc != 0:
        raise CodecError(N.last_error())


def windows(w, h):
    """(name, win_w, win_h, k, dx, dy, filters) for a w x h picture: the issue's windows.  The matrix comes from view_ref.view_matrix
    (what jsp_view_matrix computes) or is given outright."""
    fit = vr.view_matrix(w, h, 100, 73, 0, 0.5, 0.5)
    assert fit[0] not in (0.5, 0.25, 1.0) and (fit[1], fit[2]) == (0.0, 0.0)
    crop = vr.view_matrix(w, h, 90, 60, 1, 0.5, 0.5)                      # 100 %, scrolled to the middle: an integral crop
    assert crop[0] == 1.0 and crop[1] == int(crop[1]) > 0 and crop[2] == int(crop[2]) > 0
    quirk = vr.view_matrix(w, h, 2 * w + 33, 120, 2, 1.0, 0.3)           # 200 %, the picture narrower than the window: fit()'s quirk
    assert quirk[0] == 2.0 and quirk[1] == -33.0                          # ... a negative dx: 33 columns of background at the LEFT
    return [
        ("fit", 100, 73) + fit + (ipr.FILTERS,),
        ("crop100", 90, 60) + crop + (ipr.FILTERS,),
        ("quirk200", 2 * w + 33, 120) + quirk + (ipr.FILTERS,),
        ("fifth", -(-w // 5), -(-h // 5), 0.2, 0.0, 0.0, (ipr.AREA,)),
        ("twentieth", 9, 7, 0.05, -0.4, 0.3, ipr.FILTERS),                # every rectangle loops over tiles
        ("k64th", 3, 2, 1.0 / 64, 0.0, 0.0, ipr.FILTERS),
        ("width1", 1, 40, 0.37, 3.3, 2.7, ipr.FILTERS),
        ("height1", 50, 1, 0.37, 3.3, 2.7, ipr.FILTERS),
        ("times64", 70, 66, 64.0, 64.0 * (w - 1) + 20, 64.0 * (h - 1) + 10, (ipr.NEAREST, ipr.BILINEAR)),   # the last pixel and the background behind it
    ]


def cell_of(flat, i, cols, win_w, win_h, pad=0):
    """Cell i of a sheet as check() returns it (a flat buffer): (win_h, win_w)."""
    pitch = cols * win_w + pad
    at = ipr.cell_origin(i, cols, win_w, win_h, pitch)
    return np.stack([flat[at + y * pitch: at + y * pitch + win_w] for y in range(win_h)])


def check(fn, codec, idx, pictures, picks, w, h, win_w, win_h, k, dx, dy, mode, filter, cols=1, pad=0, offset=0, what=""):
    """One call into a poisoned buffer `offset` ints off a 16-byte boundary, row pitch cols * win_w + pad, nine words longer than the
    sheet: every word of it equals the reference's — the cells, and the poison everywhere else."""
    pitch = cols * win_w + pad
    total = ipr.sheet_ints(len(picks), cols, win_w, win_h, pitch) + 9
    out = dev_buf(total, offset=offset)
    assert out.data_ptr() % 16 == 4 * offset
    call(fn, codec, idx, picks, out, win_w, win_h, pitch, cols, k, dx, dy, mode, filter, out_ints=total - 9)
    got = out.cpu().numpy().view(np.uint32)
    want = ipr.sheet([pictures[t] for t in picks], w, h, win_w, win_h, k, dx, dy, mode=mode, filter=filter, background=BG, cols=cols, pitch=pitch,
                     fill=POISON, total=total)
    bad = np.flatnonzero(got != want)
    if len(bad):
        i = int(bad[0])
        raise AssertionError(f"{what} {win_w}x{win_h} k={k:.4f} mode={mode} filter={filter} cols={cols} pad={pad} offset={offset}: {len(bad)} words "
                             f"differ, first at sheet row {i // pitch} column {i % pitch}: got {got[i]:08x}, want {want[i]:08x}")
    return got
