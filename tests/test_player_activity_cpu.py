"""Manager over the activity map of an attached seek index (activity / change_totals / change_box / next_change) — the policy
alone, over a fake decoder and a fake index whose map is a numpy array (no GPU): the map is computed once per attach_index, a box is
the union of a frame's non-zero cells flipped to display rows and clipped, and next_change lands where the cells a rectangle touches
reach min_pixels, through seek()."""
import numpy as np
import pytest

from jsplayer_amd import player
from jsplayer_amd.avi import CODEC_MSVC16, VideoInfo
from test_player_index_cpu import FRAMES, KEYS, N, FakeDecoder, FakeIndex

W, H = 40, 36            # 3 x 3 cells: the last column 8 pixels wide, the last row (the TOP of the display) 4 pixels high
COLS, ROWS = 3, 3


class ActivityIndex(FakeIndex):
    def __init__(self, dec, first, count, cells):
        super().__init__(dec, first, count)
        self.cells, self.asked = cells, 0

    def Activity(self, first=0, n=None, out=None):
        self.asked += 1
        return self.cells.copy()


def the_map(count=N):
    """Frame 2 changes 5 pixels of cell (row 0, col 0) — the display's bottom-left; frame 5 cells (0, 1) and (1, 2); frame 9 three
    pixels of the clipped corner cell (2, 2); frame 12 cell (1, 1) by 40, frame 15 by 7."""
    a = np.zeros((count, ROWS, COLS), dtype=np.int16)
    a[2, 0, 0] = 5
    a[5, 0, 1], a[5, 1, 2] = 256, 10
    a[9, 2, 2] = 3
    a[12, 1, 1] = 40
    a[15, 1, 1] = 7
    return a


def manager(first=0, count=N):
    dec = FakeDecoder()
    vi = VideoInfo(X=W, Y=H, bpp=16, fps=15.0, nframes=N, codec=CODEC_MSVC16, palette=None, riff_size=0)
    mgr = player.Manager(vi, dec, lambda n: np.full(n, -1, dtype=np.int32))
    idx = ActivityIndex(dec, first, count, the_map(count))
    mgr.attach_index(idx, first)
    return mgr, dec, idx


def test_activity_is_computed_once_and_dropped_on_attach():
    mgr, dec, idx = manager()
    a = mgr.activity()
    assert mgr.activity() is a and idx.asked == 1
    assert mgr.change_totals() == [int(v) for v in the_map().reshape(N, -1).sum(axis=1)] and idx.asked == 1
    mgr.change_box(5)
    assert idx.asked == 1
    other = ActivityIndex(dec, 0, N, np.zeros((N, ROWS, COLS), dtype=np.int16))
    mgr.attach_index(other, 0)
    assert mgr.change_totals() == [0] * N and other.asked == 1 and idx.asked == 1
    mgr.attach_index(None)
    with pytest.raises(ValueError):
        mgr.activity()
    mgr.attach_index(FakeIndex(dec, 0, N), 0)   # an index object without Activity
    with pytest.raises(ValueError):
        mgr.change_totals()


def test_change_box_flips_rows_and_clips():
    mgr, _, _ = manager()
    assert mgr.change_box(0) is None and mgr.change_box(3) is None
    assert mgr.change_box(2) == (0, H - 16, 16, 16)              # stored rows 0..15 are the display's last 16
    assert mgr.change_box(5) == (16, H - 32, W - 16, 32)         # columns 16..39 (clipped from 48), stored rows 0..31
    assert mgr.change_box(9) == (32, 0, 8, 4)                    # the corner cell: 8 x 4 pixels, the display's top right
    assert mgr.change_box(12) == (16, H - 32, 16, 16)
    with pytest.raises(ValueError):
        mgr.change_box(N)


def test_change_box_of_an_index_that_starts_later():
    mgr, _, _ = manager(first=8, count=16)
    assert mgr.change_box(8 + 2) == (0, H - 16, 16, 16)
    with pytest.raises(ValueError):
        mgr.change_box(2)
    assert len(mgr.change_totals()) == 16


def test_next_change_whole_picture_then_none_at_the_end():
    mgr, dec, _ = manager()
    mgr.seek(FRAMES, 0, KEYS)
    seen = []
    while True:
        d = mgr.next_change(FRAMES, key_flags=KEYS)
        if d is None:
            break
        seen.append(d.index)
        # what seek() leaves: the frame shown is the frame of interest, decoding goes on behind it (the fake index adopts)
        assert mgr.frame_of_interest == d.index and mgr.next_frame_to_decode == d.index + 1
        assert int(mgr.buffers[d.buffer_index][0]) == d.index
    assert seen == [2, 5, 9, 12, 15]
    calls = list(dec.calls)
    foi, nxt, log = mgr.frame_of_interest, mgr.next_frame_to_decode, len(mgr.log)
    assert mgr.next_change(FRAMES, key_flags=KEYS) is None      # nothing left: nothing shown, nothing moved
    assert dec.calls == calls and (mgr.frame_of_interest, mgr.next_frame_to_decode, len(mgr.log)) == (foi, nxt, log)


def test_next_change_with_a_rect_that_touches_some_cells():
    mgr, _, _ = manager()
    mgr.seek(FRAMES, 0, KEYS)
    # the display's top-right 8 x 4 pixels are stored rows 32..35: cell (2, 2) alone
    assert mgr.next_change(FRAMES, rect=(W - 8, 0, 8, 4), key_flags=KEYS).index == 9
    mgr.seek(FRAMES, 0, KEYS)
    # one pixel inside cell (1, 1) (display row H - 1 - 20): frames 12 and 15; the whole cell is judged (a superset of the rect)
    rect = (20, H - 1 - 20, 1, 1)
    assert mgr.next_change(FRAMES, rect=rect, key_flags=KEYS).index == 12
    assert mgr.next_change(FRAMES, rect=rect, key_flags=KEYS).index == 15
    assert mgr.next_change(FRAMES, rect=rect, key_flags=KEYS) is None
    mgr.seek(FRAMES, 0, KEYS)
    # a rect over the bottom-left cell and the one right of it, display rows H - 16 .. H - 1: frames 2 and 5
    assert mgr.next_change(FRAMES, rect=(10, H - 10, 10, 5), key_flags=KEYS).index == 2
    assert mgr.next_change(FRAMES, rect=(10, H - 10, 10, 5), key_flags=KEYS).index == 5
    # a rect that reaches past the picture is clipped; one outside it finds nothing
    mgr.seek(FRAMES, 0, KEYS)
    assert mgr.next_change(FRAMES, rect=(-50, H - 3, 60, 50), key_flags=KEYS).index == 2
    assert mgr.next_change(FRAMES, rect=(W, 0, 5, 5), key_flags=KEYS) is None


def test_next_change_with_min_pixels():
    mgr, _, _ = manager()
    mgr.seek(FRAMES, 0, KEYS)
    assert mgr.next_change(FRAMES, min_pixels=6, key_flags=KEYS).index == 5      # frame 2 changes 5
    assert mgr.next_change(FRAMES, min_pixels=6, key_flags=KEYS).index == 12     # frame 9 changes 3
    assert mgr.next_change(FRAMES, min_pixels=6, key_flags=KEYS).index == 15     # 7
    mgr.seek(FRAMES, 0, KEYS)
    assert mgr.next_change(FRAMES, min_pixels=266, key_flags=KEYS).index == 5    # 256 + 10: the cells' sum
    mgr.seek(FRAMES, 0, KEYS)
    assert mgr.next_change(FRAMES, min_pixels=267, key_flags=KEYS) is None
    assert mgr.frame_of_interest == 0


def test_skip_stills_is_untouched():
    mgr, dec, _ = manager()
    mgr.seek(FRAMES, 0, KEYS)
    d = mgr.skip_stills(FRAMES, KEYS)      # the fake index calls every frame significant: the next frame
    assert d.index == 1 and [c[0] for c in dec.calls] == ["Show", "Show"]
