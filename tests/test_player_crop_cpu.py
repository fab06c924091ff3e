"""Manager.crop_rect / crop / write_crop — the policy alone, over a fake decoder and a fake index (no GPU): how a display rectangle
becomes a block rectangle in table order (rounding outwards, the display flip, a picture height that is no multiple of 4, clipping),
the pair list `crop` sends, the split into calls of 4096 pairs, the flags, each case that cannot be served, and the geometry of the
file write_crop writes."""
import numpy as np
import pytest

from jsplayer_amd import avi, player
from jsplayer_amd.avi import CODEC_MSVC16, CODEC_MSVC8, CODEC_SCREENPRESSOR, VideoInfo
from test_player_index_cpu import FakeDecoder, FakeIndex

W, H = 50, 30          # 12 x 7 blocks; stored rows 28 and 29 (display rows 0 and 1) and columns 48, 49 lie in no block
N = 24
FRAMES = [bytes([0, i]) for i in range(N)]
KEY = -2


class CropIndex(FakeIndex):
    KEY = KEY

    def __init__(self, dec, first, count):
        super().__init__(dec, first, count)
        self.calls = []

    def CropFrames(self, rect, pairs, tight=False):
        pairs = list(pairs)
        self.calls.append((tuple(rect), pairs, tight))
        # the flag of a gap pair is true where the gap ends on a multiple of 5 (a gap that writes every block of the rectangle)
        return [bytes([a & 0xFF, b & 0xFF, 0xCC, 0xCC]) for a, b in pairs], [a == KEY or b % 5 == 0 for a, b in pairs]


def manager(first=None, count=None, index=CropIndex, codec=CODEC_MSVC16, bpp=16, pal=None, w=W, h=H, n=N):
    dec = FakeDecoder()
    vi = VideoInfo(X=w, Y=h, bpp=bpp, fps=15.0, nframes=n, codec=codec, palette=pal, riff_size=0)
    mgr = player.Manager(vi, dec, lambda k: np.full(k, -1, dtype=np.int32))
    idx = None
    if first is not None:
        idx = index(dec, first, count)
        mgr.attach_index(idx, first)
    return mgr, dec, idx


def test_crop_rect_rounds_outwards_flips_and_clips():
    mgr, _, _ = manager()
    # display rows 2 .. 29 are stored rows 27 .. 0: the picture's blocks cover display (0, 2, 48, 28)
    assert mgr.crop_rect((0, 0, W, H)) == ((0, 0, 12, 7), (0, 2, 48, 28))
    assert mgr.crop_rect((-100, -100, 1000, 1000)) == ((0, 0, 12, 7), (0, 2, 48, 28))
    # an aligned rectangle stays: display rows 6 .. 13 are stored rows 23 .. 16, block rows 4 and 5
    assert mgr.crop_rect((8, 6, 12, 8)) == ((2, 4, 3, 2), (8, 6, 12, 8))
    # one pixel: its block.  Display (17, 9) is stored row 20: block (4, 5), display rows 6 .. 9
    assert mgr.crop_rect((17, 9, 1, 1)) == ((4, 5, 1, 1), (16, 6, 4, 4))
    # Y % 4 != 0: display row y is stored row 29 - y, so display y = 2 (stored 27) is the TOP row of block row 6
    assert mgr.crop_rect((0, 2, 4, 1)) == ((0, 6, 1, 1), (0, 2, 4, 4))
    assert mgr.crop_rect((0, 5, 4, 2)) == ((0, 5, 1, 2), (0, 2, 4, 8))      # display rows 5, 6 = stored 24, 23: block rows 6 and 5
    # rounding outwards on every side
    assert mgr.crop_rect((5, 7, 6, 6)) == ((1, 4, 2, 2), (4, 6, 8, 8))          # stored rows 17 .. 22; columns 5 .. 10
    # clipped to the block grid: the columns 48, 49 and the display rows 0, 1 belong to no block
    assert mgr.crop_rect((44, 0, 6, 4)) == ((11, 6, 1, 1), (44, 2, 4, 4))
    assert mgr.crop_rect((40, 26, 100, 100)) == ((10, 0, 2, 1), (40, 26, 8, 4))
    for nothing in ((48, 0, 2, 30), (0, 0, 50, 2), (0, 30, 10, 10), (50, 0, 4, 4), (-8, 0, 8, 8), (0, -4, 8, 4), (4, 4, 0, 4), (4, 4, 4, 0)):
        with pytest.raises(ValueError, match="nothing of the rectangle"):
            mgr.crop_rect(nothing)
    # change_box's result is a rectangle crop_rect takes as it is when the picture is a multiple of 16
    big, _, _ = manager(w=64, h=48)
    assert big.crop_rect((16, 16, 32, 16)) == ((4, 4, 8, 4), (16, 16, 32, 16))


def test_the_pairs_crop_sends_and_its_flags():
    mgr, dec, idx = manager(8, 12)                            # the index holds clip frames 8 .. 19
    out, flags, shown = mgr.crop(FRAMES, (8, 6, 12, 8), [9, 10, 13, 18, 19])
    assert idx.calls == [((2, 4, 3, 2), [(KEY, 1), (1, 2), (2, 5), (5, 10), (10, 11)], False)]   # ONE call, index frame numbers
    assert out == [bytes([a & 0xFF, b, 0xCC, 0xCC]) for a, b in ((KEY, 1), (1, 2), (2, 5), (5, 10), (10, 11))]
    assert flags == [True, False, True, True, False] and shown == (8, 6, 12, 8)
    assert dec.calls == [] and mgr.log == []                  # nothing decoded
    out, flags, shown = mgr.crop(FRAMES, (17, 9, 1, 1), [8], tight=True)   # a single frame: the key pair alone
    assert idx.calls[-1] == ((4, 5, 1, 1), [(KEY, 0)], True) and flags == [True] and shown == (16, 6, 4, 4) and len(out) == 1

    class NeverKey(CropIndex):
        def CropFrames(self, rect, pairs, tight=False):
            return super().CropFrames(rect, pairs, tight)[0], [False] * len(pairs)

    mgr, _, _ = manager(0, N, index=NeverKey)
    assert mgr.crop(FRAMES, (0, 2, 8, 8), [3, 5, 6])[1] == [True, False, False]   # flags[0] is True whatever the call says


def test_more_than_4096_pairs_go_out_in_calls_of_4096():
    n = 9000
    frames = [b"\x00"] * n
    mgr, _, idx = manager(0, n, n=n)
    keep = list(range(100, 100 + 8193 + 1))                   # 8194 entries: 4096 + 4096 + 2 pairs
    out, flags, _ = mgr.crop(frames, (0, 2, 8, 8), keep, tight=True)
    assert [len(c[1]) for c in idx.calls] == [4096, 4096, 2] and all(c[0] == (0, 5, 2, 2) and c[2] for c in idx.calls)
    sent = [p for c in idx.calls for p in c[1]]
    assert sent == [(KEY, 100)] + [(k - 1, k) for k in keep[1:]] and len(out) == len(flags) == len(keep)
    assert flags == [True] + [k % 5 == 0 for k in keep[1:]]
    mgr.crop(frames, (0, 2, 8, 8), keep[:4096])
    assert [len(c[1]) for c in idx.calls[3:]] == [4096]


def test_what_cannot_be_served_says_so():
    mgr, _, idx = manager(8, 8)
    rect = (0, 2, 8, 8)
    with pytest.raises(ValueError, match="keep is empty"):
        mgr.crop(FRAMES, rect, [])
    with pytest.raises(ValueError, match="frame 24 is not in the clip"):
        mgr.crop(FRAMES, rect, [9, 24])
    with pytest.raises(ValueError, match=r"not strictly ascending \(9 after 9\)"):
        mgr.crop(FRAMES, rect, [9, 9])
    with pytest.raises(ValueError, match=r"not strictly ascending \(9 after 12\)"):
        mgr.crop(FRAMES, rect, [12, 9])
    with pytest.raises(ValueError, match="frame 7 is not in the attached seek index"):
        mgr.crop(FRAMES, rect, [7, 9])                        # (a crop has no picture before the index to start from)
    with pytest.raises(ValueError, match="frame 16 is not in the attached seek index"):
        mgr.crop(FRAMES, rect, [9, 16])
    with pytest.raises(ValueError, match="nothing of the rectangle"):
        mgr.crop(FRAMES, (48, 0, 2, 2), [9, 10])
    assert idx.calls == []                                    # refused before anything is asked of the index
    mgr, _, _ = manager()
    with pytest.raises(ValueError, match="no seek index is attached"):
        mgr.crop(FRAMES, rect, [8, 10])
    mgr, _, _ = manager(8, 8, index=FakeIndex)                # an index object without CropFrames (ScreenPressor's)
    with pytest.raises(ValueError, match="cannot crop"):
        mgr.crop(FRAMES, rect, [8, 10])
    with pytest.raises(ValueError, match="cannot crop"):
        mgr.write_crop(FRAMES, rect, [8, 10])


@pytest.mark.parametrize("codec, bpp, pal", [(CODEC_MSVC16, 16, None), (CODEC_MSVC8, 8, bytes(range(256)) * 4)], ids=["16-bit", "8-bit"])
def test_write_crop_writes_the_rectangles_geometry(codec, bpp, pal):
    mgr, _, idx = manager(8, 12, codec=codec, bpp=bpp, pal=pal)
    keep = [10, 13, 16, 19]
    want, want_keys, shown = mgr.crop(FRAMES, (5, 7, 6, 6), keep)
    blob = mgr.write_crop(FRAMES, (5, 7, 6, 6), keep, fps=2.0, tight=True)
    vi, frames, keys = avi.read_avi_indexed(blob)
    assert [bytes(f) for f in frames] == want and list(keys) == want_keys == [True, True, False, False]
    assert shown == (4, 6, 8, 8) and (vi.X, vi.Y, vi.bpp, vi.codec, vi.nframes) == (8, 8, bpp, codec, len(keep)) and vi.fps == 2.0
    assert vi.palette == pal and codec != CODEC_SCREENPRESSOR
    assert idx.calls[0][:2] == idx.calls[1][:2] and (idx.calls[0][2], idx.calls[1][2]) == (False, True)
