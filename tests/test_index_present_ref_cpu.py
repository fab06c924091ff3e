"""tests/index_present_ref.py (the numpy statement of jsp_index_present's EQUIVALENCE and SHEET) against hand-worked cases, and
Manager.present_from_index / Manager.contact_sheet — the policy alone, over a fake decoder and a fake index (no GPU): which frames
and which display matrix are asked for, that asking is a pure read of Manager and decoder, and what is refused."""
import copy

import numpy as np
import pytest

import index_present_ref as ipr
import thumbs_ref as tr
import view_ref as vr
from jsplayer_amd import player
from jsplayer_amd.avi import CODEC_MSVC16, CODEC_SCREENPRESSOR, VideoInfo

FILL = 0x5A5A5A5A
MODES = (vr.CANVAS, vr.CANVAS_RGB15, vr.SETPIXELS, vr.SETPIXELS_RGB15)


def picture(w, h, seed, bits=24):
    return np.random.default_rng(seed).integers(0, 1 << bits, size=w * h, dtype=np.uint32)


# ---- the helper ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("filter", ipr.FILTERS)
def test_k_one_with_integral_offsets_is_the_converted_crop(mode, filter):
    """k = 1: window pixel (ox, oy) has its centre in bitmap pixel (ox + dx, win_h + dy - 1 - oy) — the buffer is bottom-up — so the
    window is the converted picture, cropped and flipped, whatever the filter; outside the picture it is the background."""
    w, h, win_w, win_h, dx, dy, bg = 19, 13, 8, 6, 5, 4, 0x11223344
    pic = picture(w, h, 3, bits=15 if mode in (vr.CANVAS_RGB15, vr.SETPIXELS_RGB15) else 24)
    conv = vr.convert(pic, mode).reshape(h, w)
    got = ipr.window(pic, w, h, win_w, win_h, 1.0, float(dx), float(dy), mode, filter, bg)
    want = np.array([[conv[win_h + dy - 1 - oy, ox + dx] for ox in range(win_w)] for oy in range(win_h)], dtype=np.uint32)
    assert np.array_equal(got, want)
    # scrolled past the right edge and the top: the uncovered pixels are the background as given
    got = ipr.window(pic, w, h, win_w, win_h, 1.0, float(w - 3), float(h - win_h + 2), mode, filter, bg)
    assert np.all(got[:, 3:] == bg) and np.all(got[:2] == bg)
    assert np.array_equal(got[2:, :3], np.array([[conv[h + 1 - oy, ox + w - 3] for ox in range(3)] for oy in range(2, win_h)], dtype=np.uint32))


@pytest.mark.parametrize("s", tr.SCALES)
def test_area_at_one_over_s_is_the_thumbnail_of_the_converted_picture(s):
    """k = 1 / s, dx = dy = 0 into the (W / s) x (H / s) window: the footprints are the s x s squares, the rule rounds halves up as
    the thumbnails do.  SETPIXELS leaves the three colour bytes where they are, so the thumbnail formula applies to the picture
    itself; the window is top row first, a thumbnail keeps the frame's bottom-up rows."""
    w, h = 8 * 16, 3 * 16                                                # whole squares and whole blocks at every scale
    pic = picture(w, h, 40 + s)
    tw, th = tr.thumb_size(w, h, s)
    assert (tw, th) == (w // s, h // s)
    got = ipr.window(pic, w, h, tw, th, 1.0 / s, 0.0, 0.0, vr.SETPIXELS, ipr.AREA)
    thumb = tr.thumbnail(pic, w, h, s).view(np.uint32)
    assert np.array_equal(got, (thumb | np.uint32(0xFF000000))[::-1])


def test_sheet_offsets_padding_and_the_cells_past_n():
    w, h, win_w, win_h, cols, pitch = 12, 10, 5, 3, 2, 13
    pics = [picture(w, h, 60 + i) for i in range(5)]
    pics[3] = pics[0]                                                     # a repeat
    total = ipr.sheet_ints(5, cols, win_w, win_h, pitch) + 7
    assert ipr.sheet_ints(5, cols, win_w, win_h, pitch) == (3 * win_h - 1) * pitch + cols * win_w
    flat = ipr.sheet(pics, w, h, win_w, win_h, 0.5, 0.0, 0.0, filter=ipr.NEAREST, cols=cols, pitch=pitch, fill=FILL, total=total)
    assert flat.shape == (total,)
    written = np.zeros(total, dtype=bool)
    for i, pic in enumerate(pics):
        cell = vr.present(pic, w, h, win_w, win_h, 0.5, 0.0, 0.0, filter=vr.NEAREST)
        at = (i // cols) * win_h * pitch + (i % cols) * win_w
        assert at == ipr.cell_origin(i, cols, win_w, win_h, pitch)
        for y in range(win_h):
            assert np.array_equal(flat[at + y * pitch: at + y * pitch + win_w], cell[y])
            written[at + y * pitch: at + y * pitch + win_w] = True
    assert written.sum() == 5 * win_w * win_h
    assert np.all(flat[~written] == FILL)                                 # padding, the sixth cell, the seven words behind the sheet
    at6 = ipr.cell_origin(5, cols, win_w, win_h, pitch)
    assert not written[at6] and flat[at6] == FILL
    # n = 1, cols = 1: the plain window
    one = ipr.sheet(pics[:1], w, h, win_w, win_h, 0.5, 0.0, 0.0, filter=ipr.AREA)
    assert np.array_equal(one.reshape(win_h, win_w), ipr.window(pics[0], w, h, win_w, win_h, 0.5, 0.0, 0.0, vr.CANVAS, ipr.AREA))


# ---- the Manager's two calls ----------------------------------------------------------------------------------------------------------
N = 24
X, Y = 40, 30


class _Res:
    def __init__(self, data, sig):
        self.data_pnt, self.significant_changes = data, sig


class FakeDecoder:
    SEEKS = True

    def __init__(self):
        self.calls, self.prev = [], None

    def Preinit(self, lines):
        pass

    def PreviousFrame(self):
        return self.prev

    def IsKeyFrame(self, f):
        return f[0] == 1


class FakeIndex:
    """Present logs its arguments and paints cell i with its index frame number."""

    def __init__(self, count):
        self.frames = count
        self.significance = [True] * count
        self.presents = []

    def Present(self, frames, win_w, win_h, k, dx, dy, mode=None, filter=1, background=0xFF000000, cols=1, out=None):
        frames = list(frames)
        assert all(0 <= t < self.frames for t in frames)
        self.presents.append(dict(frames=frames, win=(win_w, win_h), matrix=(k, dx, dy), mode=mode, filter=filter, background=background,
                                  cols=cols, out=out))
        n = len(frames)
        sheet = np.zeros((-(-n // cols) * win_h, cols * win_w), dtype=np.int32) if out is None else out.reshape(-(-n // cols) * win_h, cols * win_w)
        for i, t in enumerate(frames):
            sheet[(i // cols) * win_h:(i // cols + 1) * win_h, (i % cols) * win_w:(i % cols + 1) * win_w] = t
        return sheet


class ThumbsOnlyIndex:
    def __init__(self, count):
        self.frames = count

    def Thumbs(self, frames, scale=8, cols=1, out=None):
        raise AssertionError("not asked for")


def _manager(dec, codec=CODEC_MSVC16, bpp=16):
    vi = VideoInfo(X=X, Y=Y, bpp=bpp, fps=15.0, nframes=N, codec=codec, palette=None, riff_size=0)
    return player.Manager(vi, dec, lambda n: np.full(n, -1, dtype=np.int32))


def _state(mgr, dec):
    return (copy.deepcopy(mgr.holds), mgr.frame_of_interest, mgr.next_frame_to_decode, list(mgr.log), dict(mgr.judged), list(dec.calls),
            dec.prev, [b.copy() for b in mgr.buffers])


def _same(a, b):
    return a[:7] == b[:7] and all(np.array_equal(x, y) for x, y in zip(a[7], b[7]))


@pytest.mark.parametrize("first", [0, 5])
def test_present_from_index_asks_for_the_views_window_of_one_frame(first):
    dec = FakeDecoder()
    mgr = _manager(dec)
    idx = FakeIndex(16)
    mgr.attach_index(idx, first)
    mgr.view.zoom_in()
    mgr.view.zoom_in()                                                    # 200 %
    mgr.view.scroll(True, 0.3)
    mgr.view.scroll(False, 0.8)
    before = _state(mgr, dec)
    out = np.full(20 * 12, -7, dtype=np.int32)
    got = mgr.present_from_index(first + 9, out, 20, 12, filter=ipr.AREA, background=0x01020304)
    assert _same(before, _state(mgr, dec))                                # a pure read
    (call,) = idx.presents                                                # ONE Present call
    assert call["frames"] == [9] and call["win"] == (20, 12) and call["cols"] == 1 and call["out"] is out
    assert call["matrix"] == vr.view_matrix(X, Y, 20, 12, 2, 0.3, 0.8)
    assert call["mode"] == vr.CANVAS and call["filter"] == ipr.AREA and call["background"] == 0x01020304
    assert got.shape == (12, 20) and np.all(got == 9) and np.all(out == 9)
    mgr.present_from_index(first, out, 20, 12)
    assert idx.presents[1]["filter"] == ipr.BILINEAR and idx.presents[1]["background"] == 0xFF000000   # the defaults of `present`


def test_present_from_index_converts_16_bpp_screenpressor_from_rgb15():
    for codec, bpp, mode in ((CODEC_SCREENPRESSOR, 16, vr.CANVAS_RGB15), (CODEC_SCREENPRESSOR, 24, vr.CANVAS), (CODEC_MSVC16, 16, vr.CANVAS)):
        mgr = _manager(FakeDecoder(), codec, bpp)
        idx = FakeIndex(4)
        mgr.attach_index(idx)
        mgr.present_from_index(2, None, 8, 6)
        mgr.contact_sheet(2, 8, 6)
        assert [c["mode"] for c in idx.presents] == [mode, mode]


@pytest.mark.parametrize("first", [0, 5])
@pytest.mark.parametrize("n", [1, 3, 7, 16, 40])
def test_contact_sheet_fits_the_filmstrips_frames_into_cells(first, n):
    count = 16
    dec = FakeDecoder()
    mgr = _manager(dec)
    idx = FakeIndex(count)
    mgr.attach_index(idx, first)
    mgr.view.zoom_in()                                                    # the sheet is Fit whatever the window's view is
    before = _state(mgr, dec)
    numbers, sheet = mgr.contact_sheet(n, 16, 9)
    assert _same(before, _state(mgr, dec))
    picks = [(k * count) // n for k in range(n)]
    assert numbers == [first + t for t in picks]
    (call,) = idx.presents
    assert call["frames"] == picks and call["win"] == (16, 9) and call["cols"] == n and call["out"] is None
    assert call["matrix"] == vr.view_matrix(X, Y, 16, 9, 0, 0.5, 0.5) == (min(16 / X, 9 / Y), 0.0, 0.0)
    assert call["filter"] == ipr.AREA                                     # the default: a shrunk picture
    assert sheet.shape == (9, n * 16) and [int(sheet[0, i * 16]) for i in range(n)] == picks
    numbers, sheet = mgr.contact_sheet(n, 16, 9, cols=3, filter=ipr.NEAREST)
    assert idx.presents[1]["cols"] == 3 and idx.presents[1]["filter"] == ipr.NEAREST and sheet.shape == (-(-n // 3) * 9, 48)


def test_refusals():
    dec = FakeDecoder()
    mgr = _manager(dec)
    with pytest.raises(ValueError, match="not in an attached seek index"):
        mgr.present_from_index(0, None, 8, 6)
    with pytest.raises(ValueError, match="no seek index"):
        mgr.contact_sheet(4, 8, 6)
    idx = FakeIndex(8)
    mgr.attach_index(idx, 4)
    for i in (3, 12, -1):
        with pytest.raises(ValueError, match="not in an attached seek index"):
            mgr.present_from_index(i, None, 8, 6)
    with pytest.raises(ValueError, match="at least one frame"):
        mgr.contact_sheet(0, 8, 6)
    assert idx.presents == []
    mgr.attach_index(ThumbsOnlyIndex(8), 4)
    with pytest.raises(ValueError, match="cannot present"):
        mgr.present_from_index(5, None, 8, 6)
    with pytest.raises(ValueError, match="cannot present"):
        mgr.contact_sheet(2, 8, 6)
