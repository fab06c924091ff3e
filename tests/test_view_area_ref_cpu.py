"""tests/view_area_ref.py against answers a reader can check by hand, its named mistakes against the shared case list, and the
binding of jsp_display_present_area — all without a GPU."""
import numpy as np
import pytest

import view_area_ref as ar
import view_ref as vr
from jsplayer_amd import _native as N
from jsplayer_amd import codec as cm


def rnd(w, h, seed, bits=24):
    return np.random.default_rng(seed).integers(0, 1 << bits, size=w * h, dtype=np.uint64).astype(np.uint32)


def box_mean(img, n):
    """(sum + n*n/2) // (n*n) of every n x n block of every byte of `img` (h, w) — the filmstrip's rounding."""
    h, w = img.shape
    out = np.zeros((h // n, w // n), dtype=np.uint32)
    for byte in range(4):
        plane = ((img >> np.uint32(8 * byte)) & np.uint32(0xFF)).astype(np.int64)
        sums = plane.reshape(h // n, n, w // n, n).sum(axis=(1, 3))
        out |= ((sums + n * n // 2) // (n * n)).astype(np.uint32) << np.uint32(8 * byte)
    return out


@pytest.mark.parametrize("mode", ar.MODES)
def test_k1_with_integral_offsets_is_the_plain_crop(mode):
    fw, fh, ww, wh, dx, dy = 37, 23, 16, 8, 5, 3
    src = rnd(fw, fh, 1, 15 if mode in ar.RGB15 else 24)
    got = ar.present_area(src, fw, fh, ww, wh, 1.0, float(dx), float(dy), mode)
    flipped = vr.convert(src, mode).reshape(fh, fw)[::-1]
    assert np.array_equal(got, flipped[fh - wh - dy:fh - dy, dx:dx + ww])
    for filt in (vr.NEAREST, vr.BILINEAR):
        assert np.array_equal(got, vr.present(src, fw, fh, ww, wh, 1.0, float(dx), float(dy), mode, filt))


@pytest.mark.parametrize("n", [2, 4, 3])
def test_k_one_nth_is_the_box_mean_with_halves_rounded_up(n):
    fw, fh = 12 * n, 5 * n
    src = rnd(fw, fh, 2)
    got = ar.present_area(src, fw, fh, fw // n, fh // n, 1.0 / n, 0.0, 0.0, ar.SETPIXELS)
    want = box_mean((src | np.uint32(0xFF000000)).reshape(fh, fw)[::-1], n)
    assert np.array_equal(got, want)
    # a half is rounded up: a 2 x 2 block of 0, 0, 0, 2 has the mean 0.5 -> 1, and 0, 0, 0, 1 has 0.25 -> 0
    if n == 2:
        tiny = np.array([0, 0, 0, 2], dtype=np.uint32)
        assert ar.present_area(tiny, 2, 2, 1, 1, 0.5, 0.0, 0.0, ar.SETPIXELS)[0, 0] == 0xFF000001
        tiny[3] = 1
        assert ar.present_area(tiny, 2, 2, 1, 1, 0.5, 0.0, 0.0, ar.SETPIXELS)[0, 0] == 0xFF000000


def test_a_half_pixel_offset_weighs_the_edge_columns_by_half():
    """k = 1/2, dx = 0.25 (half a source pixel): the footprint of output pixel 0 covers half of column 0, column 1 and half of
    column 2 — by hand (128 a + 256 b + 128 c) over two rows, D = 512 * 512."""
    row = np.array([10, 20, 40, 80], dtype=np.uint32)
    src = np.concatenate([row, row])
    got = ar.present_area(src, 4, 2, 1, 1, 0.5, 0.25, 0.0, ar.SETPIXELS)
    S = 512 * (128 * 10 + 256 * 20 + 128 * 40)
    assert got[0, 0] == (0xFF000000 | ((S + 512 * 512 // 2) // (512 * 512)))


def test_alpha_of_the_canvas_modes_stays_ff():
    fw, fh = 64, 48
    for mode in (ar.CANVAS, ar.CANVAS_RGB15, ar.SETPIXELS):
        src = rnd(fw, fh, 3, 15 if mode in ar.RGB15 else 24)
        for k in (0.37, 1 / 3, 1 / 64, 3.5):
            got = ar.present_area(src, fw, fh, 20, 15, k, 0.0, 0.0, mode, background=0xFF000000)
            assert np.all(got >> np.uint32(24) == 0xFF), (mode, k)


def test_white_stays_white_where_the_sum_passes_32_bits():
    white = np.full(130 * 130, 0xFFFFFF, dtype=np.uint32)
    got = ar.present_area(white, 130, 130, 2, 2, 1 / 64, 0.0, 0.0, ar.CANVAS)
    assert np.all(got == 0xFFFFFFFF)
    white = np.full(200 * 120, 0xFFFFFF, dtype=np.uint32)
    k, dx, dy = vr.view_matrix(200, 120, 10, 6, 0, 0.5, 0.5)
    assert k == 0.05
    s = vr.fixed16(1 / k) >> 8
    assert 255 * s * s > 1 << 32
    assert np.all(ar.present_area(white, 200, 120, 10, 6, k, dx, dy, ar.CANVAS) == 0xFFFFFFFF)


def test_the_three_filters_agree_on_which_pixels_are_picture():
    for c in ar.CASES:
        if c.part not in ("edges", "views") or c.window == (1, 1):
            continue
        (fw, fh), (ww, wh) = c.frame, c.window
        src = np.full(fw * fh, 0x123456, dtype=np.uint32)
        bg = 0x00ABCDEF
        area = ar.present_area(src, fw, fh, ww, wh, c.k, c.dx, c.dy, ar.SETPIXELS, bg)
        near = vr.present(src, fw, fh, ww, wh, c.k, c.dx, c.dy, vr.SETPIXELS, vr.NEAREST, bg)
        assert np.array_equal(area, near), c       # a flat picture: every filter shows the flat colour where it shows the picture


def test_the_case_list_holds_what_it_is_meant_to():
    parts = {c.part for c in ar.CASES}
    assert parts == {"views", "edges", "modes", "large", "taps", "seams"}
    assert {vr.fixed16(1 / c.k) >> 8 for c in ar.CASES if c.part == "taps"} == {512, 513, 1024, 1025}
    views = [c for c in ar.CASES if c.part == "views"]
    assert {c.frame for c in views} == set(ar.FRAMES) and {c.window for c in views} == set(ar.WINDOWS)
    assert any(c.dx < 0 for c in views), "the fit() quirk: a negative dx"
    assert {c.mode for c in views} == set(ar.MODES)
    # all four picture edges clipped in one window: background on every side of a window that shows picture in the middle
    clipped = 0
    for c in ar.CASES:
        if c.part != "edges":
            continue
        (fw, fh), (ww, wh) = c.frame, c.window
        w = ar.present_area(ar.frame_words(c), fw, fh, ww, wh, c.k, c.dx, c.dy, c.mode, 0x00000001)
        sides = [np.all(w[0] == 1), np.all(w[-1] == 1), np.all(w[:, 0] == 1), np.all(w[:, -1] == 1)]
        assert np.any(w != 1)
        clipped += all(sides)
    assert clipped >= 4
    # S beyond 32 bits in the large cases
    for c in ar.CASES:
        if c.part == "large":
            s = vr.fixed16(1 / c.k) >> 8
            assert 255 * s * s > 1 << 32, c
    # windows across the workgroup boundaries in x (a whole number of workgroups, one pixel less, one and three more) and in y
    span, band = cm.PRESENT_AREA_SPAN_X, cm.PRESENT_AREA_BAND_ROWS
    seams = [c.window for c in ar.CASES if c.part == "seams"]
    rests = {w % span for (w, h) in seams if w > span}
    assert {0, span - 1, 1, 3} <= rests
    assert any(h > band for (w, h) in seams) and (band == 1 or any(h % band for (w, h) in seams)) and any(h % band == 0 for (w, h) in seams)


@pytest.mark.parametrize("mistake", ar.MISTAKES)
def test_every_named_mistake_shows_on_the_cases(mistake):
    wrong = 0
    for c in ar.CASES:
        if c.part == "views" and c.frame != (37, 23):
            continue                                        # (one frame's views are enough here; the GPU test takes all)
        (fw, fh), (ww, wh) = c.frame, c.window
        src = ar.frame_words(c)
        good = ar.present_area(src, fw, fh, ww, wh, c.k, c.dx, c.dy, c.mode, 0x00123456)
        bad = ar.present_area(src, fw, fh, ww, wh, c.k, c.dx, c.dy, c.mode, 0x00123456, mistake=mistake)
        wrong += not np.array_equal(good, bad)
    assert wrong > 0, f"no case tells '{mistake}' from the rule"


def test_the_kernel_constants_python_restates():
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "jsplayer_amd", "csrc", "present_area_kernels.hip")).read()
    val = lambda name: int(re.search(r"constexpr int %s = (\d+);" % name, text).group(1))
    assert cm.PRESENT_AREA_SPAN_X == val("kAreaLanes")
    assert cm.PRESENT_AREA_BAND_ROWS == val("kAreaBandRows")
    assert cm.PRESENT_AREA == 2 and (cm.PRESENT_NEAREST, cm.PRESENT_BILINEAR) == (0, 1)


def test_the_area_call_is_bound_and_exported():
    import ctypes
    assert "jsp_display_present_area" in N.SIGNATURES
    restype, argtypes = N.SIGNATURES["jsp_display_present_area"]
    present = N.SIGNATURES["jsp_display_present"][1]
    assert restype is ctypes.c_int and len(argtypes) == len(present) - 1            # present's arguments without the filter
    assert argtypes == present[:11] + present[12:]
    assert hasattr(ctypes.CDLL(N.LIB_PATH), "jsp_display_present_area")


def test_host_side_refusals_need_no_library_call():
    """display_present_area refuses a host array as display_present does, before anything is launched."""
    host = np.zeros(16, dtype=np.int32)
    with pytest.raises(cm.CodecError, match="^display_present_area: frame buffers must be device tensors"):
        cm.display_present_area(host, 4, 4, host, 4, 4, 1.0, 0.0, 0.0)
