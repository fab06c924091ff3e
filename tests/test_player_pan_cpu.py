"""Manager.follow / pan / write_pan — the policy alone, over a fake decoder and a fake index (no GPU): how the activity map moves a
rectangle (a box inside, off each edge, wider than the rectangle, the clamp at all four borders, empty frames, the start), the pair
list `pan` sends, the split into calls of 4096 pairs, the flags, each case that cannot be served, and the geometry of the file
write_pan writes."""
import numpy as np
import pytest

from jsplayer_amd import avi
from jsplayer_amd.avi import CODEC_MSVC16, CODEC_MSVC8, CODEC_SCREENPRESSOR
from test_player_crop_cpu import CropIndex, manager
from test_player_index_cpu import FakeIndex

W, H = 160, 96         # 40 x 24 blocks, 10 x 6 cells of 16 x 16 pixels: a cell is 4 x 4 blocks
N = 24
FRAMES = [bytes([0, i]) for i in range(N)]
KEY = -2
SIZE = (48, 32)        # 12 x 8 blocks: three cells by two


class PanIndex(CropIndex):
    """activity: {index frame: [(grid row, grid column), ...]} — rows in the stored bottom-up order."""

    def __init__(self, dec, first, count, activity=None):
        super().__init__(dec, first, count)
        self.cells = np.zeros((count, H // 16, W // 16), dtype=np.uint16)
        for f, where in (activity or {}).items():
            for r, q in where:
                self.cells[f, r, q] = 7

    def Activity(self):
        return self.cells

    def PanFrames(self, size, pairs, tight=False):
        pairs = list(pairs)
        self.calls.append((tuple(size), pairs, tight))
        return [bytes([p[0] & 0xFF, p[1] & 0xFF, 0xEE, 0xEE]) for p in pairs], [p[0] == KEY or p[1] % 5 == 0 for p in pairs]


def pan_manager(activity=None, first=0, count=N, **kw):
    return manager(first, count, index=lambda d, f, c: PanIndex(d, f, c, activity), w=W, h=H, **kw)


def test_pan_size_rounds_up_and_clips():
    mgr, _, _ = pan_manager()
    assert mgr.pan_size((48, 32)) == (12, 8) and mgr.pan_size((45, 29)) == (12, 8) and mgr.pan_size((1, 1)) == (1, 1)
    assert mgr.pan_size((1000, 1000)) == (40, 24)
    for nothing in ((0, 8), (8, 0), (-4, 8)):
        with pytest.raises(ValueError, match="nothing of a rectangle"):
            mgr.pan_size(nothing)
    odd, _, _ = manager(w=50, h=30)
    assert odd.pan_size((1000, 1000)) == (12, 7)                  # columns 48, 49 and two rows lie in no block


def test_follow_a_box_inside_off_each_edge_and_wider():
    keep = list(range(8))
    act = {1: [(1, 1)],                      # inside the rectangle at (4, 4): it stays
           2: [(1, 4)],                      # blocks x 16 .. 19: off the right edge -> x = 20 - 12 = 8
           3: [(3, 3)],                      # blocks y 12 .. 15: off the top (stored) edge -> y = 16 - 8 = 8; x 12 .. 15 inside [8, 20)
           4: [(2, 0)],                      # blocks x 0 .. 3: off the left edge -> x = 0; y 8 .. 11 inside [8, 16)
           5: [(0, 0), (0, 1)],              # blocks y 0 .. 3: off the bottom (stored) edge -> y = 0
           6: [(1, 2), (1, 7)],              # x 8 .. 31: 24 blocks wide, wider than 12 -> centred: x = 8 + 6 = 14; y 4 .. 7 inside
           7: [(0, 5), (5, 5)]}              # y 0 .. 23 taller than 8 -> y = 8; x 20 .. 23 inside [14, 26)
    mgr, _, _ = pan_manager(act)
    path = mgr.follow(SIZE, keep, start=(4, 4))
    assert path == [(0, 4, 4), (1, 4, 4), (2, 8, 4), (3, 8, 8), (4, 0, 8), (5, 0, 0), (6, 14, 0), (7, 14, 8)]
    # the union over a gap: frames 2 and 3 together are x 12 .. 19 (off the right edge) and y 4 .. 15, 12 blocks and taller than the
    # rectangle's 8: centred, y = 4 + 2
    assert mgr.follow(SIZE, [0, 1, 3], start=(4, 4)) == [(0, 4, 4), (1, 4, 4), (3, 8, 6)]
    # index frames, not clip frames: the same map under an index that starts at clip frame 8
    mgr, _, _ = pan_manager(act, first=8, count=12)
    assert mgr.follow(SIZE, [8, 9, 10, 11], start=(4, 4)) == [(8, 4, 4), (9, 4, 4), (10, 8, 4), (11, 8, 8)]


def test_follow_clamps_at_all_four_borders_and_stays_on_empty_frames():
    # a rectangle wider than half the grid, boxes wider than it at the borders: centring would leave the grid
    size = (96, 64)                                               # 24 x 16 blocks
    act = {1: [(2, 0), (2, 6)],                                   # x 0 .. 27, 28 wide: centred x = 2
           2: [(2, 3), (2, 9)],                                   # x 12 .. 39, 28 wide: centred x = 14, still inside the grid (<= 16)
           4: [(0, 4), (4, 4)],                                   # y 0 .. 19, 20 tall: centred y = 2; x 16 .. 19 inside [14, 38)
           5: [(1, 4), (5, 4)]}                                   # y 4 .. 23: centred y = 6
    mgr, _, _ = pan_manager(act)
    assert mgr.follow(size, [0, 1, 2, 3, 4, 5], start=(8, 4)) == [(0, 8, 4), (1, 2, 4), (2, 14, 4), (3, 14, 4), (4, 14, 2), (5, 14, 6)]
    # the whole grid as the box under a rectangle of 39 x 23 blocks: centring gives (0, 0), one block of room on each axis
    mgr, _, _ = pan_manager({1: [(r, q) for r in range(6) for q in range(10)]})
    assert mgr.follow((156, 92), [0, 1], start=(1, 1)) == [(0, 1, 1), (1, 0, 0)]
    # `start` outside the grid is clamped at all four borders
    mgr, _, _ = pan_manager()
    assert [mgr.follow(SIZE, [3], start=s)[0][1:] for s in ((-5, 3), (100, 3), (3, -5), (3, 100))] == [(0, 3), (28, 3), (3, 0), (3, 16)]
    # boxes at the four corners: the least move ends exactly at the border
    act = {1: [(0, 0)], 2: [(5, 9)], 3: [(5, 0)], 4: [(0, 9)]}
    mgr, _, _ = pan_manager(act)
    assert mgr.follow(SIZE, [0, 1, 2, 3, 4], start=(14, 8)) == [(0, 14, 8), (1, 0, 0), (2, 28, 16), (3, 0, 16), (4, 28, 0)]
    # nothing changes: the rectangle stays where it starts; without a start it is centred on the picture
    mgr, _, _ = pan_manager()
    assert mgr.follow(SIZE, [2, 5, 9], start=(3, 2)) == [(2, 3, 2), (5, 3, 2), (9, 3, 2)]
    assert mgr.follow(SIZE, [2, 5, 9]) == [(2, 14, 8), (5, 14, 8), (9, 14, 8)]
    # without a start: centred on the first non-empty box of the kept range (frame 6's cell: x 24 .. 27, y 16 .. 19)
    mgr, _, _ = pan_manager({1: [(0, 0)], 6: [(4, 6)]})
    assert mgr.follow(SIZE, [2, 4, 7, 9]) == [(2, 20, 14), (4, 20, 14), (7, 20, 14), (9, 20, 14)]
    assert mgr.follow(SIZE, [7]) == [(7, 14, 8)]                  # a single frame has no gap and no box


def test_follow_refuses_what_it_cannot_serve():
    mgr, _, _ = pan_manager(first=8, count=8)
    with pytest.raises(ValueError, match="keep is empty"):
        mgr.follow(SIZE, [])
    with pytest.raises(ValueError, match=r"not strictly ascending \(9 after 9\)"):
        mgr.follow(SIZE, [9, 9])
    with pytest.raises(ValueError, match="frame 7 is not in the attached seek index"):
        mgr.follow(SIZE, [7, 9])
    mgr, _, _ = manager(0, N, index=FakeIndex, w=W, h=H)
    with pytest.raises(ValueError, match="no activity map"):
        mgr.follow(SIZE, [1, 2])


def test_the_pairs_pan_sends_and_its_flags():
    mgr, dec, idx = pan_manager(first=8, count=12)                # the index holds clip frames 8 .. 19
    path = [(9, 4, 4), (10, 4, 4), (13, 8, 4), (18, 8, 8), (19, 0, 16)]
    out, flags, shown = mgr.pan(FRAMES, SIZE, path)
    sent = [(KEY, 1, None, (4, 4)), (1, 2, (4, 4), (4, 4)), (2, 5, (4, 4), (8, 4)), (5, 10, (8, 4), (8, 8)), (10, 11, (8, 8), (0, 16))]
    assert idx.calls == [((12, 8), sent, True)]                   # ONE call, index frame numbers, tight by default
    assert out == [bytes([p[0] & 0xFF, p[1], 0xEE, 0xEE]) for p in sent] and flags == [True, False, True, True, False]
    # display rectangles, top row first: block row by is stored rows 4 by ..: display y = 96 - 4 (by + 8)
    assert shown == [(16, 48, 48, 32), (16, 48, 48, 32), (32, 48, 48, 32), (32, 32, 48, 32), (0, 0, 48, 32)]
    assert dec.calls == [] and mgr.log == []                      # nothing decoded
    mgr.pan(FRAMES, (45, 30), path[:1], tight=False)
    assert idx.calls[-1] == ((12, 8), [(KEY, 1, None, (4, 4))], False)

    class NeverKey(PanIndex):
        def PanFrames(self, size, pairs, tight=False):
            return super().PanFrames(size, pairs, tight)[0], [False] * len(pairs)

    mgr, _, _ = manager(0, N, index=NeverKey, w=W, h=H)
    assert mgr.pan(FRAMES, SIZE, [(3, 0, 0), (5, 1, 0), (6, 1, 0)])[1] == [True, False, False]   # flags[0] is True whatever the call says


def test_follow_feeds_pan():
    act = {2: [(1, 4)], 3: [(3, 3)]}
    mgr, _, idx = pan_manager(act)
    path = mgr.follow(SIZE, [0, 1, 2, 3], start=(4, 4))
    mgr.pan(FRAMES, SIZE, path)
    assert idx.calls[-1][1] == [(KEY, 0, None, (4, 4)), (0, 1, (4, 4), (4, 4)), (1, 2, (4, 4), (8, 4)), (2, 3, (8, 4), (8, 8))]


def test_more_than_4096_pairs_go_out_in_calls_of_4096():
    n = 9000
    frames = [b"\x00"] * n
    mgr, _, idx = pan_manager(count=n, n=n)
    path = [(k, k % 7, k % 5) for k in range(100, 100 + 8193 + 1)]   # 8194 entries: 4096 + 4096 + 2 pairs
    out, flags, shown = mgr.pan(frames, SIZE, path)
    assert [len(c[1]) for c in idx.calls] == [4096, 4096, 2] and all(c[0] == (12, 8) and c[2] for c in idx.calls)
    sent = [p for c in idx.calls for p in c[1]]
    assert sent[0] == (KEY, 100, None, (100 % 7, 100 % 5))
    assert sent[1:] == [(a[0], b[0], a[1:], b[1:]) for a, b in zip(path, path[1:])]
    assert len(out) == len(flags) == len(shown) == len(path) and flags == [True] + [k % 5 == 0 for k, _, _ in path[1:]]


def test_what_cannot_be_served_says_so():
    mgr, _, idx = pan_manager(first=8, count=8)
    with pytest.raises(ValueError, match="the path is empty"):
        mgr.pan(FRAMES, SIZE, [])
    with pytest.raises(ValueError, match="frame 24 is not in the clip"):
        mgr.pan(FRAMES, SIZE, [(9, 0, 0), (24, 0, 0)])
    with pytest.raises(ValueError, match=r"not strictly ascending \(9 after 9\)"):
        mgr.pan(FRAMES, SIZE, [(9, 0, 0), (9, 1, 0)])
    with pytest.raises(ValueError, match=r"not strictly ascending \(9 after 12\)"):
        mgr.pan(FRAMES, SIZE, [(12, 0, 0), (9, 0, 0)])
    with pytest.raises(ValueError, match="frame 7 is not in the attached seek index"):
        mgr.pan(FRAMES, SIZE, [(7, 0, 0), (9, 0, 0)])
    with pytest.raises(ValueError, match="frame 16 is not in the attached seek index"):
        mgr.pan(FRAMES, SIZE, [(9, 0, 0), (16, 0, 0)])
    with pytest.raises(ValueError, match="nothing of a rectangle"):
        mgr.pan(FRAMES, (0, 4), [(9, 0, 0)])
    for x, y in ((-1, 0), (0, -1), (29, 0), (0, 17)):
        with pytest.raises(ValueError, match=rf"frame 10 at block \({x}, {y}\) is outside the block grid"):
            mgr.pan(FRAMES, SIZE, [(9, 28, 16), (10, x, y)])
    assert idx.calls == []                                        # refused before anything is asked of the index
    mgr, _, _ = manager(w=W, h=H)
    with pytest.raises(ValueError, match="no seek index is attached"):
        mgr.pan(FRAMES, SIZE, [(8, 0, 0)])
    for index in (FakeIndex, CropIndex):                          # an index object without PanFrames
        mgr, _, _ = manager(8, 8, index=index, w=W, h=H)
        with pytest.raises(ValueError, match="cannot pan"):
            mgr.pan(FRAMES, SIZE, [(8, 0, 0), (10, 1, 1)])
        with pytest.raises(ValueError, match="cannot pan"):
            mgr.write_pan(FRAMES, SIZE, [(8, 0, 0), (10, 1, 1)])


@pytest.mark.parametrize("codec, bpp, pal", [(CODEC_MSVC16, 16, None), (CODEC_MSVC8, 8, bytes(range(256)) * 4)], ids=["16-bit", "8-bit"])
def test_write_pan_writes_the_rectangles_geometry(codec, bpp, pal):
    mgr, _, idx = pan_manager(first=8, count=12, codec=codec, bpp=bpp, pal=pal)
    path = [(10, 0, 0), (13, 2, 1), (16, 2, 1), (19, 28, 16)]
    want, want_keys, shown = mgr.pan(FRAMES, (45, 30), path)
    blob = mgr.write_pan(FRAMES, (45, 30), path, fps=2.0, tight=False)
    vi, frames, keys = avi.read_avi_indexed(blob)
    assert [bytes(f) for f in frames] == want and list(keys) == want_keys == [True, True, False, False]
    assert (vi.X, vi.Y, vi.bpp, vi.codec, vi.nframes) == (48, 32, bpp, codec, len(path)) and vi.fps == 2.0
    assert vi.palette == pal and codec != CODEC_SCREENPRESSOR and shown[-1] == (112, 0, 48, 32)
    assert idx.calls[0][:2] == idx.calls[1][:2] and (idx.calls[0][2], idx.calls[1][2]) == (True, False)
