"""The numpy reference of the thumbnail contract (tests/thumbs_ref.py) against hand-worked answers.  No GPU."""
import numpy as np
import pytest

import thumbs_ref as tr


def test_thumb_size_drops_remainders_and_odd_trailing_blocks():
    assert tr.thumb_size(64, 48, 4) == (16, 12) and tr.thumb_size(64, 48, 8) == (8, 6) and tr.thumb_size(64, 48, 16) == (4, 3)
    # 36x20: 9x5 blocks — the trailing odd block column / row fills no output pixel at s = 8, 16
    assert tr.thumb_size(36, 20, 4) == (9, 5) and tr.thumb_size(36, 20, 8) == (4, 2) and tr.thumb_size(36, 20, 16) == (2, 1)
    # 70x46: 17x11 blocks, 2 remainder pixels each way
    assert tr.thumb_size(70, 46, 4) == (17, 11) and tr.thumb_size(70, 46, 8) == (8, 5) and tr.thumb_size(70, 46, 16) == (4, 2)
    assert tr.thumb_size(7, 100, 4) == (1, 25) and tr.thumb_size(7, 100, 8) == (0, 12)
    assert tr.thumb_size(1920, 1080, 8) == (240, 135) and tr.thumb_size(1920, 1080, 16) == (120, 67)


def test_known_16x16_picture_at_all_three_scales():
    # pixel (x, y): R = x, G = 16 y, B = 200 when x is even else 201
    pic = np.zeros((16, 16), dtype=np.uint32)
    for y in range(16):
        for x in range(16):
            pic[y, x] = (x << 16) | ((16 * y) << 8) | (200 + (x & 1))
    flat = pic.reshape(-1)
    t4 = tr.thumbnail(flat, 16, 16, 4).view(np.uint32)
    assert t4.shape == (4, 4)
    for ty in range(4):
        for tx in range(4):
            # R: mean of 4tx .. 4tx+3 = 4tx + 1.5 -> (16 (4tx + 1.5) + 8) >> 4 = 4tx + 2 (half rounds up)
            # G: mean of 16 (4ty .. 4ty+3) = 64 ty + 24;  B: 200.5 -> 201
            assert t4[ty, tx] == ((4 * tx + 2) << 16) | ((64 * ty + 24) << 8) | 201, (tx, ty)
    t8 = tr.thumbnail(flat, 16, 16, 8).view(np.uint32)
    assert t8.shape == (2, 2)
    for ty in range(2):
        for tx in range(2):
            # R: 8tx + 3.5 -> 8tx + 4;  G: 16 (8ty + 3.5) = 128 ty + 56;  B: 201
            assert t8[ty, tx] == ((8 * tx + 4) << 16) | ((128 * ty + 56) << 8) | 201, (tx, ty)
    t16 = tr.thumbnail(flat, 16, 16, 16).view(np.uint32)
    # R: 7.5 -> 8;  G: 16 * 7.5 = 120;  B: 201
    assert t16.shape == (1, 1) and t16[0, 0] == (8 << 16) | (120 << 8) | 201


@pytest.mark.parametrize("s", tr.SCALES)
def test_rounding_is_half_up_not_half_even_and_not_truncation(s):
    n = s * s
    pic = np.zeros(n, dtype=np.uint32)
    pic[: n // 2] = 1            # blue mean exactly 0.5 -> 1
    assert tr.thumbnail(pic, s, s, s).view(np.uint32)[0, 0] == 1
    pic[n // 2 - 1] = 0          # just under a half -> 0
    assert tr.thumbnail(pic, s, s, s).view(np.uint32)[0, 0] == 0
    pic[:] = 2
    pic[: n // 2] = 3            # 2.5 -> 3 (half-even would give 2)
    assert tr.thumbnail(pic, s, s, s).view(np.uint32)[0, 0] == 3


@pytest.mark.parametrize("s", tr.SCALES)
def test_channels_do_not_carry_into_each_other(s):
    """All-0x00FF00FF and all-0x0000FF00: sums of R and B that would spill into G (and G into R) in unseparated fields."""
    for word in (0x00FF00FF, 0x0000FF00, 0x00FFFFFF, 0x00FF0000, 0x000000FF):
        pic = np.full(32 * 32, word, dtype=np.uint32)
        t = tr.thumbnail(pic, 32, 32, s).view(np.uint32)
        assert t.shape == (32 // s, 32 // s) and np.all(t == word), hex(word)
    # the top byte of a source word is not a channel: it never reaches the thumbnail
    pic = np.full(16 * 16, 0xFF102030, dtype=np.uint32)
    assert np.all(tr.thumbnail(pic, 16, 16, s).view(np.uint32) == 0x00102030)


def test_remainder_columns_and_rows_do_not_contribute():
    w, h = 22, 10                       # 5x2 blocks + 2 remainder pixels each way
    pic = np.full((h, w), 0x00101010, dtype=np.uint32)
    pic[:, 20:] = 0x00FFFFFF            # W % 4 remainder
    pic[8:, :] = 0x00FFFFFF             # H % 4 remainder
    assert np.all(tr.thumbnail(pic.reshape(-1), w, h, 4).view(np.uint32) == 0x00101010)
    pic[:, 16:20] = 0x00FFFFFF          # the odd trailing block column: in at s = 4, out at s = 8
    t4 = tr.thumbnail(pic.reshape(-1), w, h, 4).view(np.uint32)
    assert t4.shape == (2, 5) and np.all(t4[:, :4] == 0x00101010) and np.all(t4[:, 4] == 0x00FFFFFF)
    t8 = tr.thumbnail(pic.reshape(-1), w, h, 8).view(np.uint32)
    assert t8.shape == (1, 2) and np.all(t8 == 0x00101010)


def test_rows_keep_the_frames_order():
    pic = np.zeros((8, 4), dtype=np.uint32)
    pic[:4] = 0x10                      # rows 0..3 of the frame -> row 0 of the thumbnail
    pic[4:] = 0x20
    t = tr.thumbnail(pic.reshape(-1), 4, 8, 4).view(np.uint32)
    assert t[0, 0] == 0x10 and t[1, 0] == 0x20


def test_sheet_layout_addresses():
    tw, th, n = 3, 2, 5
    thumbs = [np.full((th, tw), 100 + k, dtype=np.int32) for k in range(n)]
    for k in range(n):
        thumbs[k][0, 0] = k             # marks pixel (0, 0)
    # cols = 1: a plain [n][th][tw] array
    s1 = tr.sheet(thumbs, 1, fill=-1)
    assert s1.shape == (n * th, tw) and np.array_equal(s1.reshape(n, th, tw), np.stack(thumbs))
    assert [tr.cell_origin(k, 1, tw, th) for k in range(n)] == [0, 6, 12, 18, 24]
    # cols = 3: two sheet rows, pitch 9; the last cell of the second row is not written
    s3 = tr.sheet(thumbs, 3, fill=-1)
    assert s3.shape == (2 * th, 9)
    assert [tr.cell_origin(k, 3, tw, th) for k in range(n)] == [0, 3, 6, 18, 21]
    flat = s3.reshape(-1)
    for k in range(n):
        assert flat[tr.cell_origin(k, 3, tw, th)] == k
    assert np.array_equal(s3[0:2, 3:6], thumbs[1]) and np.array_equal(s3[2:4, 0:3], thumbs[3]) and np.array_equal(s3[2:4, 3:6], thumbs[4])
    assert np.all(s3[2:4, 6:9] == -1)
    # cols = n: a horizontal strip
    sn = tr.sheet(thumbs, n, fill=-1)
    assert sn.shape == (th, n * tw)
    assert [tr.cell_origin(k, n, tw, th) for k in range(n)] == [0, 3, 6, 9, 12]
    for k in range(n):
        assert np.array_equal(sn[:, k * tw:(k + 1) * tw], thumbs[k])
