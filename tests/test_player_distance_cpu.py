"""Manager over the distance map of an attached seek index (distance / distance_totals / find_picture / repeats_of / distinct_frames)
— the policy alone, over a fake decoder and a fake index whose pictures are hand-made (no GPU): a map is computed once per reference
frame and dropped by attach_index, totals are sums over the cells a display rectangle touches, find_picture lists the frames within
max_pixels in clip frame numbers, and distinct_frames compares with the LAST KEPT frame, one Distance call per kept frame over the
frames still ahead."""
import numpy as np
import pytest

from jsplayer_amd import player
from jsplayer_amd.avi import CODEC_MSVC16, VideoInfo
from test_player_index_cpu import N, FakeDecoder, FakeIndex

W, H = 40, 36            # 3 x 3 cells: the last column 8 pixels wide, the last row (the TOP of the display) 4 pixels high
COLS, ROWS = 3, 3


def pictures(count=N):
    """A picture is what its nine cells show: [frame, row, col] -> a number of pixels of the cell painted over (0: the ground).  Two
    pictures differ in a cell by the larger of the two numbers where they differ.  Frame -1 (the picture before) is all ground.
      0..3    ground;  4..7  a dialog of 30 pixels in cell (1, 1);  8..11 ground again (A -> B -> A);  12..15 the dialog again
      5       the cursor blinks besides: 2 pixels of cell (0, 0) — the display's bottom left;  13 the same
      16..    cell (2, 2), the clipped corner, grows by one pixel a frame: 1, 2, 3 ..."""
    p = np.zeros((count, ROWS, COLS), dtype=np.int64)
    p[4:8, 1, 1] = 30
    p[12:16, 1, 1] = 30
    p[5, 0, 0] = p[13, 0, 0] = 2
    for t in range(16, count):
        p[t, 2, 2] = t - 15
    return p


def between(a, b):
    return np.where(a != b, np.maximum(a, b), 0)


class DistanceIndex(FakeIndex):
    def __init__(self, dec, first, count):
        super().__init__(dec, first, count)
        self.p, self.asked = pictures(count), []

    def Distance(self, ref, first=0, n=None, out=None):
        n = self.frames - first if n is None else n
        assert -1 <= ref < self.frames and 0 <= first and n >= 1 and first + n <= self.frames
        self.asked.append((ref, first, n))
        r = np.zeros((ROWS, COLS), dtype=np.int64) if ref < 0 else self.p[ref]
        return np.stack([between(self.p[t], r) for t in range(first, first + n)]).astype(np.int16)


def manager(first=0, count=N):
    dec = FakeDecoder()
    vi = VideoInfo(X=W, Y=H, bpp=16, fps=15.0, nframes=first + count, codec=CODEC_MSVC16, palette=None, riff_size=0)
    mgr = player.Manager(vi, dec, lambda n: np.full(n, -1, dtype=np.int32))
    idx = DistanceIndex(dec, first, count)
    mgr.attach_index(idx, first)
    return mgr, dec, idx


def test_a_map_is_kept_per_reference_frame_and_dropped_on_attach():
    mgr, dec, idx = manager()
    a = mgr.distance(4)
    assert mgr.distance(4) is a and idx.asked == [(4, 0, N)]
    asked = len(idx.asked)
    b = mgr.distance(0)
    assert b is not a and mgr.distance(0) is b and mgr.distance(4) is a and len(idx.asked) == asked + 1
    mgr.distance_totals(4)
    mgr.find_picture(4)
    assert len(idx.asked) == asked + 1
    assert mgr.distance(-1) is mgr.distance(-1)          # the picture before the index
    other = DistanceIndex(dec, 0, N)
    mgr.attach_index(other, 0)
    assert mgr.distance(4) is not a and len(other.asked) == 1
    for bad in (-2, N, N + 5):
        with pytest.raises(ValueError):
            mgr.distance(bad)
    mgr.attach_index(None)
    with pytest.raises(ValueError):
        mgr.distance(0)
    mgr.attach_index(FakeIndex(dec, 0, N), 0)   # an index object without Distance
    for call in (lambda: mgr.distance(0), lambda: mgr.distance_totals(0), lambda: mgr.find_picture(0), lambda: mgr.repeats_of(0),
                 lambda: mgr.distinct_frames(1)):
        with pytest.raises(ValueError):
            call()


def test_distance_totals_and_rectangles():
    mgr, _, _ = manager()
    want = [0, 0, 0, 0, 30, 32, 30, 30, 0, 0, 0, 0, 30, 32, 30, 30] + list(range(1, N - 15))
    assert mgr.distance_totals(0) == want
    assert mgr.distance_totals(-1) == want
    # the display's bottom-left pixel lies in cell (0, 0): the cursor alone
    cursor = mgr.distance_totals(0, rect=(0, H - 1, 1, 1))
    assert [k for k, v in enumerate(cursor) if v] == [5, 13] and cursor[5] == 2
    # one pixel inside cell (1, 1): the whole cell is summed
    assert mgr.distance_totals(0, rect=(20, H - 1 - 20, 1, 1)) == [30 if 4 <= k < 8 or 12 <= k < 16 else 0 for k in range(N)]
    # the display's top right 8 x 4 pixels are the clipped corner cell
    assert mgr.distance_totals(0, rect=(W - 8, 0, 8, 4))[16:] == list(range(1, N - 15))
    # a rectangle that reaches past the picture is clipped; one outside it sees nothing
    assert mgr.distance_totals(0, rect=(-50, H - 3, 60, 50)) == cursor
    assert mgr.distance_totals(0, rect=(W, 0, 5, 5)) == [0] * N


def test_find_picture_and_repeats_of():
    mgr, _, _ = manager()
    assert mgr.find_picture(0) == [0, 1, 2, 3, 8, 9, 10, 11]
    assert mgr.repeats_of(0) == [1, 2, 3, 8, 9, 10, 11] and mgr.repeats_of(9) == [0, 1, 2, 3, 8, 10, 11]
    assert mgr.find_picture(4) == [4, 6, 7, 12, 14, 15] and mgr.repeats_of(5) == [13] and mgr.repeats_of(20) == []
    assert mgr.find_picture(4, max_pixels=2) == [4, 5, 6, 7, 12, 13, 14, 15]
    assert mgr.find_picture(0, max_pixels=3) == [0, 1, 2, 3, 8, 9, 10, 11, 16, 17, 18]
    # where the dialog is: whatever else the frame shows
    assert mgr.find_picture(4, rect=(20, H - 1 - 20, 1, 1)) == [4, 5, 6, 7, 12, 13, 14, 15]
    assert mgr.find_picture(4, rect=(W, 0, 5, 5)) == list(range(N))


def test_clip_frame_numbers_of_an_index_that_starts_later():
    mgr, _, idx = manager(first=8, count=N)
    assert mgr.find_picture(8) == [8 + k for k in (0, 1, 2, 3, 8, 9, 10, 11)]
    assert mgr.repeats_of(8 + 5) == [8 + 13]
    assert mgr.distance(7) is mgr.distance(7) and idx.asked[-1][0] == -1      # clip frame 7 is the picture before the index
    assert len(mgr.distance_totals(8)) == N
    for bad in (6, 8 + N):
        with pytest.raises(ValueError):
            mgr.find_picture(bad)
    assert mgr.distinct_frames(30, first=8 + 2, count=8) == [10, 12, 16, 17]


def test_distinct_frames_compares_with_the_last_kept_frame():
    mgr, _, idx = manager()
    # 0 is kept; 4 is the first frame 30 pixels from it; 8 the first 30 from 4; 12; then nothing reaches 30 from 12 ... but the last
    assert mgr.distinct_frames(30) == [0, 4, 8, 12, 16, N - 1]
    # one Distance call per kept frame, over the frames still ahead of it
    assert idx.asked == [(0, 1, N - 1), (4, 5, N - 5), (8, 9, N - 9), (12, 13, N - 13), (16, 17, N - 17)]
    # the cursor's two pixels count at 2: 5 differs from 4, 6 from 5
    assert mgr.distinct_frames(2)[:6] == [0, 4, 5, 6, 8, 12]
    # cell (2, 2) grows one pixel a frame, and what counts is the distance from the last KEPT frame (the larger of the two numbers):
    # from 16 (1 pixel) frame 17 is 2 away, from 17 frame 18 is 3 away
    assert mgr.distinct_frames(3, first=16) == [16, 18, 19, 20, 21, 22, 23]
    # nothing is ever far enough: the first and the last frame
    assert mgr.distinct_frames(10_000) == [0, N - 1]
    assert mgr.distinct_frames(30, first=1, count=3) == [1, 3]
    assert mgr.distinct_frames(30, first=5, count=1) == [5]
    for first, count in ((-1, 3), (0, N + 1), (N, 1), (3, 0)):
        with pytest.raises(ValueError):
            mgr.distinct_frames(30, first=first, count=count)
    keep = mgr.distinct_frames(1)
    assert keep == sorted(set(keep)) and keep[0] == 0 and keep[-1] == N - 1
