"""tests/view_ref.py against answers worked out by hand: the reference the GPU tests of jsp_display_present trust has to be right
on its own."""
import numpy as np

import view_ref as vr


def u32(a):
    return np.asarray(a, dtype=np.uint32)


def picture(w, h, seed=1, bits=24):
    return np.random.default_rng(seed).integers(0, 1 << bits, size=w * h, dtype=np.uint64).astype(np.uint32)


def test_k1_with_integral_offsets_is_a_plain_crop_under_both_filters():
    w, h, ww, wh, dx, dy = 13, 9, 6, 4, 5, 3
    frame = picture(w, h)
    img = vr.convert(frame, vr.CANVAS).reshape(h, w)
    # output row oy shows bitmap row win_h + dy - 1 - oy, output column ox bitmap column ox + dx
    want = np.stack([img[wh + dy - 1 - oy, dx:dx + ww] for oy in range(wh)])
    for f in (vr.NEAREST, vr.BILINEAR):
        assert np.array_equal(vr.present(frame, w, h, ww, wh, 1.0, float(dx), float(dy), vr.CANVAS, f), want), f


def test_nearest_at_200_percent_replicates_every_pixel_2x2():
    w, h = 5, 3
    frame = picture(w, h, 2)
    img = vr.convert(frame, vr.SETPIXELS).reshape(h, w)
    got = vr.present(frame, w, h, 2 * w, 2 * h, 2.0, 0.0, 0.0, vr.SETPIXELS, vr.NEAREST)
    want = np.repeat(np.repeat(img[::-1], 2, axis=0), 2, axis=1)
    assert np.array_equal(got, want)


def test_bilinear_2x2_picture_at_k2_by_hand():
    """Buffer rows (bottom-up): [0, 64], [128, 192] in the low byte.  At k = 2 the output centres fall at bitmap 0.25, 0.75, 1.25,
    1.75: the taps are (x0, x0 + 1) = (-1, 0), (0, 1), (0, 1), (1, 2) clamped to (0, 0), (0, 1), (0, 1), (1, 1) with weights
    192, 64, 192, 64 of 256 — a quarter and three quarters between the pixels, the outermost centres on the edge pixel itself.
    Rows likewise, top output row = bitmap row 1."""
    frame = u32([0, 64, 128, 192])
    got = vr.present(frame, 2, 2, 4, 4, 2.0, 0.0, 0.0, vr.SETPIXELS, vr.BILINEAR)
    want = u32([[128, 144, 176, 192],
                [96, 112, 144, 160],
                [32, 48, 80, 96],
                [0, 16, 48, 64]]) | np.uint32(0xFF000000)
    assert np.array_equal(got, want)
    # a rounding case by hand: 1 and 2 a quarter apart: (1 * 192 + 2 * 64) * 256 + 32768 >> 16 = 1.25 + 0.5 -> 1; three quarters -> 2.25 -> 2
    row = vr.present(u32([1, 2]), 2, 1, 4, 1, 2.0, 0.0, 0.0, vr.SETPIXELS, vr.BILINEAR)
    assert (row & 0xFF).tolist() == [[1, 1, 2, 2]]
    # and 0 / 255 half way (k = 2/3 puts a centre at 0.75 .. : use k = 1, dx = 0.5): (0 * 128 + 255 * 128) * 256 + 32768 >> 16 = 128
    half = vr.present(u32([0, 255]), 2, 1, 1, 1, 1.0, 0.5, 0.0, vr.SETPIXELS, vr.BILINEAR)
    assert int(half[0, 0] & 0xFF) == 128


def test_background_outside_the_picture_above_and_to_the_right():
    w, h, ww, wh = 4, 3, 6, 5
    frame = picture(w, h, 3)
    img = vr.convert(frame, vr.CANVAS).reshape(h, w)
    bg = 0x00ABCDEF                               # written as given: no alpha forced
    for f in (vr.NEAREST, vr.BILINEAR):
        got = vr.present(frame, w, h, ww, wh, 1.0, 0.0, 0.0, vr.CANVAS, f, bg)
        want = np.full((wh, ww), bg, dtype=np.uint32)
        want[wh - h:, :w] = img[::-1]           # sy = -y + win_h: the picture sits on the window's bottom edge, at its left
        assert np.array_equal(got, want), f
    # a negative dx (the quirk of fit) pushes it to the right edge
    got = vr.present(frame, w, h, ww, wh, 1.0, -2.0, 0.0, vr.CANVAS, vr.NEAREST, bg)
    want = np.full((wh, ww), bg, dtype=np.uint32)
    want[wh - h:, 2:] = img[::-1]
    assert np.array_equal(got, want)


def test_rows_are_flipped():
    w, h = 3, 4
    frame = np.repeat(np.arange(h, dtype=np.uint32), w)          # buffer row y holds y
    got = vr.present(frame, w, h, w, h, 1.0, 0.0, 0.0, vr.SETPIXELS, vr.NEAREST)
    assert (got[:, 0] & 0xFF).tolist() == [3, 2, 1, 0]


def test_each_mode_on_one_pixel_matches_the_display_convert_constants():
    """The values tests/test_avi_player.py pins jsp_display_convert's four formulas to (Manager.hx:379, 370, 351, 340)."""
    px = u32([0x00112233, 0x00FFEEDD, 0x12345678, 0x0000001F])
    want = {vr.CANVAS: [0xFF332211, 0xFFDDEEFF, 0xFF785634, 0xFF1F0000],
            vr.CANVAS_RGB15: [0xFF891198, 0xFFFF76E8, 0xFFA2B3C0, 0xFF0000F8],
            vr.SETPIXELS: [0xFF112233, 0xFFFFEEDD, 0xFF345678, 0xFF00001F],
            vr.SETPIXELS_RGB15: [0x89119800, 0xFF76E800, 0xA2B3C000, 0x0000F800]}
    for mode, row in want.items():
        assert vr.convert(px, mode).tolist() == row, mode
        for f in (vr.NEAREST, vr.BILINEAR):
            assert vr.present(px, 4, 1, 4, 1, 1.0, 0.0, 0.0, mode, f).tolist() == [row], (mode, f)


def test_geometry_known_answers():
    assert vr.view_matrix(1920, 1080, 1280, 720, 0, 0.5, 0.5) == (2 / 3, 0.0, 0.0)
    assert vr.view_matrix(1920, 1080, 1280, 720, 2, 0.5, 0.5) == (2.0, 1280.0, 720.0)
    assert vr.view_matrix(20, 12, 15, 9, 1, 0.5, 0.5) == (1.0, 2.5, 1.5)
    assert vr.view_matrix(37, 23, 64, 64, 1, 1.0, 0.5)[1] == -27.0      # fit() with mx < mn: the picture goes to the right edge
    assert vr.fit(5, 0, -27) == -27 and vr.fit(-1, 0, -27) == 0 and vr.fit(3, 0, 10) == 3
