"""Manager.sequence / reverse / boomerang and their writers, without a GPU.  The policy over a fake decoder and a fake index: the pair
list sent in ONE PathFrames call, the orders `reverse` and `boomerang` make, the flags, each case that cannot be served.  Then the
whole way over an index that answers PathFrames with the rule in plain Python (tests/index_path_ref.py): the written AVI, read back
with avi.py and decoded by the oracle, shows the kept frames in reverse, and for a boomerang there and back, the last picture the
first."""
import numpy as np
import pytest

import index_crop_ref as cr
import msv1_crop_clips as cc
from jsplayer_amd import CodecError, avi
from jsplayer_amd.avi import CODEC_MSVC16, CODEC_MSVC8, CODEC_SCREENPRESSOR
from test_index_crop_ref_cpu import Small, source
from test_index_path_ref_cpu import made
from test_player_crop_cpu import CropIndex, manager
from test_player_index_cpu import FakeIndex

W, H = 50, 30          # 12 x 7 blocks; display rows 0 and 1 and columns 48, 49 lie in no block
N = 24
FRAMES = [bytes([0, i]) for i in range(N)]
KEY = -2


class PathIndex(CropIndex):
    def PathFrames(self, rect, pairs, tight=False):
        pairs = list(pairs)
        self.calls.append((tuple(rect), pairs, tight))
        # the flag of a pair is true where it ends on a multiple of 5 (a pair that codes every block of the rectangle)
        return [bytes([a & 0xFF, b & 0xFF, 0xDD, 0xDD]) for a, b in pairs], [a == KEY or b % 5 == 0 for a, b in pairs]


def path_manager(first=0, count=N, **kw):
    return manager(first, count, index=PathIndex, **kw)


def test_the_pairs_sequence_sends_in_one_call_and_its_flags():
    mgr, dec, idx = path_manager(8, 12)                            # the index holds clip frames 8 .. 19
    order = [13, 10, 10, 18, 9, 19, 8]
    out, flags, shown = mgr.sequence(FRAMES, order, rect=(8, 6, 12, 8))
    sent = [(KEY, 5), (5, 2), (2, 2), (2, 10), (10, 1), (1, 11), (11, 0)]
    assert idx.calls == [((2, 4, 3, 2), sent, False)]              # ONE call, index frame numbers, any direction, repeats
    assert out == [bytes([a & 0xFF, b, 0xDD, 0xDD]) for a, b in sent]
    assert flags == [True, False, False, True, False, False, True] and shown == (8, 6, 12, 8)
    assert dec.calls == [] and mgr.log == []                       # nothing decoded
    out, flags, shown = mgr.sequence(FRAMES, [12], tight=True)     # a single frame: the key pair alone; no rect: the whole block grid
    assert idx.calls[-1] == ((0, 0, 12, 7), [(KEY, 4)], True) and flags == [True] and shown == (0, 2, 48, 28) and len(out) == 1

    class NeverKey(PathIndex):
        def PathFrames(self, rect, pairs, tight=False):
            return super().PathFrames(rect, pairs, tight)[0], [False] * len(pairs)

    mgr, _, _ = manager(0, N, index=NeverKey)
    assert mgr.sequence(FRAMES, [5, 3, 3])[1] == [True, False, False]   # flags[0] is True whatever the call says


def test_reverse_and_boomerang_are_sequences_of_the_kept_frames():
    mgr, _, idx = path_manager(8, 12)
    keep = [9, 10, 13, 18]
    mgr.reverse(FRAMES, keep)
    assert idx.calls[-1] == ((0, 0, 12, 7), [(KEY, 10), (10, 5), (5, 2), (2, 1)], False)
    mgr.boomerang(FRAMES, keep, rect=(17, 9, 1, 1), tight=True)
    # there and back: the last step returns to keep[0]
    assert idx.calls[-1] == ((4, 5, 1, 1), [(KEY, 1), (1, 2), (2, 5), (5, 10), (10, 5), (5, 2), (2, 1)], True)
    mgr.boomerang(FRAMES, [11])
    assert idx.calls[-1][1] == [(KEY, 3)]
    mgr.boomerang(FRAMES, [11, 12])
    assert idx.calls[-1][1] == [(KEY, 3), (3, 4), (4, 3)]
    assert len(idx.calls) == 4                                     # one call each


def test_what_cannot_be_served_says_so():
    mgr, _, idx = path_manager(8, 8)
    with pytest.raises(ValueError, match="order is empty"):
        mgr.sequence(FRAMES, [])
    with pytest.raises(ValueError, match="frame 24 is not in the clip"):
        mgr.sequence(FRAMES, [9, 24])
    with pytest.raises(ValueError, match="frame 7 is not in the attached seek index"):
        mgr.sequence(FRAMES, [9, 7])
    with pytest.raises(ValueError, match="frame 16 is not in the attached seek index"):
        mgr.sequence(FRAMES, [16, 9])
    with pytest.raises(ValueError, match="nothing of the rectangle"):
        mgr.sequence(FRAMES, [9, 8], rect=(48, 0, 2, 30))
    with pytest.raises(ValueError, match="more than 4096 frames"):
        mgr.sequence(FRAMES, [9, 10] * 2049)
    for call in (mgr.reverse, mgr.boomerang, mgr.write_reverse, mgr.write_boomerang):
        with pytest.raises(ValueError, match="keep is empty"):
            call(FRAMES, [])
        with pytest.raises(ValueError, match=r"not strictly ascending \(9 after 12\)"):
            call(FRAMES, [12, 9])
        with pytest.raises(ValueError, match=r"not strictly ascending \(9 after 9\)"):
            call(FRAMES, [9, 9])
    assert idx.calls == []                                         # refused before anything is asked of the index
    mgr.sequence(FRAMES, [9, 10] * 2048)                           # 4096 entries are one call
    assert [len(c[1]) for c in idx.calls] == [4096]
    mgr, _, _ = manager()
    with pytest.raises(ValueError, match="no seek index is attached"):
        mgr.sequence(FRAMES, [8])
    for index in (FakeIndex, CropIndex):                           # an index object without PathFrames (ScreenPressor's)
        mgr, _, _ = manager(8, 8, index=index)
        with pytest.raises(ValueError, match="cannot step back"):
            mgr.sequence(FRAMES, [10, 8])
        with pytest.raises(ValueError, match="cannot step back"):
            mgr.write_reverse(FRAMES, [8, 10])


@pytest.mark.parametrize("codec, bpp, pal", [(CODEC_MSVC16, 16, None), (CODEC_MSVC8, 8, bytes(range(256)) * 4)], ids=["16-bit", "8-bit"])
def test_the_writers_write_the_rectangles_geometry(codec, bpp, pal):
    mgr, _, idx = path_manager(8, 12, codec=codec, bpp=bpp, pal=pal)
    order = [15, 13, 10, 18]
    want, want_keys, shown = mgr.sequence(FRAMES, order, rect=(8, 6, 12, 8))
    blob = mgr.write_sequence(FRAMES, order, rect=(8, 6, 12, 8), fps=2.0, tight=True)
    vi, frames, keys = avi.read_avi_indexed(blob)
    assert [bytes(f) for f in frames] == want and list(keys) == want_keys == [True, True, False, True]
    assert (vi.X, vi.Y, vi.bpp, vi.codec, vi.nframes) == (12, 8, bpp, codec, len(order)) and vi.fps == 2.0
    assert vi.palette == pal and codec != CODEC_SCREENPRESSOR and shown == (8, 6, 12, 8)
    assert idx.calls[0][:2] == idx.calls[1][:2] and (idx.calls[0][2], idx.calls[1][2]) == (False, True)
    vi, frames, _ = avi.read_avi_indexed(mgr.write_reverse(FRAMES, [9, 12, 14]))
    assert (vi.X, vi.Y, vi.nframes) == (48, 28, 3) and [bytes(f)[:2] for f in frames] == [bytes([KEY & 0xFF, 6]), bytes([6, 4]), bytes([4, 1])]
    vi, frames, _ = avi.read_avi_indexed(mgr.write_boomerang(FRAMES, [9, 12, 14], rect=(0, 2, 8, 4)))
    assert (vi.X, vi.Y, vi.nframes) == (8, 4, 5) and [bytes(f)[1] for f in frames] == [1, 4, 6, 4, 1]


class RefIndex:
    """An index object that answers PathFrames with tests/index_path_ref.py over a Source (test_index_crop_ref_cpu)."""
    KEY = KEY

    def __init__(self, s):
        self.s, self.frames, self.calls = s, s.n, 0

    def PathFrames(self, rect, pairs, tight=False):
        self.calls += 1
        out = [made(self.s, tuple(rect), (int(a), int(b)), tight) for a, b in pairs]
        for j, x in enumerate(out):
            if not isinstance(x, bytes):
                raise CodecError(f"index_path: pair {j}: {x}")
        return out, [cr.flag(self.s.bits, x, rect[2] * rect[3]) for x in out]


@pytest.mark.parametrize("bits", [16, 8])
@pytest.mark.parametrize("tight", [False, True], ids=["loose", "tight"])
def test_the_written_files_decode_to_the_kept_frames_in_reverse_and_there_and_back(bits, tight):
    clip = cc.tight(bits) if tight else cc.seams(bits, (5, 3, 37, 31))
    s = source(clip)
    mgr, _, _ = manager(w=cc.W, h=cc.H, n=s.n, codec=CODEC_MSVC16 if bits == 16 else CODEC_MSVC8, bpp=bits, pal=s.pal)
    idx = RefIndex(s)
    mgr.attach_index(idx, 0)
    keep = list(range(1, s.n, 2))
    display = (20, 56, 148, 124)                                   # blocks (5, 3, 37, 31)
    for rect, blocks in ((display, (5, 3, 37, 31)), (None, cc.WHOLE)):
        for write, order in ((mgr.write_reverse, keep[::-1]), (mgr.write_boomerang, keep + keep[-2::-1])):
            calls = idx.calls
            vi, frames, keys = avi.read_avi_indexed(write(clip.frames, keep, rect=rect, tight=tight))
            assert idx.calls == calls + 1                          # ONE PathFrames call
            assert (vi.X, vi.Y, vi.bpp, vi.nframes) == (4 * blocks[2], 4 * blocks[3], bits, len(order)) and keys[0]
            small = Small(s, blocks)
            pictures = []
            for k, (t, data) in enumerate(zip(order, frames)):
                pic = small.key(bytes(data)) if k == 0 else small.inter(bytes(data))
                assert np.array_equal(pic, s.sub(blocks, t)), (bits, tight, rect, k, t)
                assert bool(keys[k]) == (k == 0 or cr.flag(bits, bytes(data), blocks[2] * blocks[3]))
                pictures.append(pic.copy())
            small.close()
            if write == mgr.write_boomerang:
                assert np.array_equal(pictures[0], pictures[-1]) and not np.array_equal(pictures[0], pictures[len(keep) - 1])
    # what the index cannot make raises its CodecError
    s = source(cc.nones(bits), cc.NONES_START)
    mgr, _, _ = manager(w=cc.W, h=cc.H, n=len(s.clip.frames), codec=CODEC_MSVC16 if bits == 16 else CODEC_MSVC8, bpp=bits, pal=s.pal)
    mgr.attach_index(RefIndex(s), cc.NONES_START)
    with pytest.raises(CodecError, match="index_path: pair 1"):
        mgr.reverse(s.clip.frames, [cc.NONES_START + s.n - 2, cc.NONES_START + s.n - 1], rect=display)   # (the last frame gives a block its first code)
