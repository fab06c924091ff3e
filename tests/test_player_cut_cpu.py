"""Manager.cut / write_cut — the policy alone, over a fake decoder and a fake index (no GPU): a clip cut at a key frame is copied as
it is and never touches the index; cut at an inter frame it starts with the index's KeyFrame of that frame, asked for once; the
frames after the first are the caller's own objects with their own flags; each case that cannot be served says which it is; and
write_cut gives an AVI file that reads back as those frames and flags."""
import numpy as np
import pytest

from jsplayer_amd import avi, player
from jsplayer_amd.avi import CODEC_MSVC16, CODEC_MSVC8, VideoInfo
from test_player_index_cpu import FRAMES, KEYS, N, FakeDecoder, FakeIndex

W, H = 16, 8


class CutIndex(FakeIndex):
    def __init__(self, dec, first, count):
        super().__init__(dec, first, count)
        self.asked = []

    def KeyFrame(self, t):
        self.asked.append(t)
        return bytes([1, self.first + t, 0xEE, 0xEE])   # a key frame by FakeDecoder.IsKeyFrame, not one of the clip's


def manager(first=None, count=None, index=CutIndex, codec=CODEC_MSVC16, bpp=16, pal=None):
    dec = FakeDecoder()
    vi = VideoInfo(X=W, Y=H, bpp=bpp, fps=15.0, nframes=N, codec=codec, palette=pal, riff_size=0)
    mgr = player.Manager(vi, dec, lambda n: np.full(n, -1, dtype=np.int32))
    idx = None
    if first is not None:
        idx = index(dec, first, count)
        mgr.attach_index(idx, first)
    return mgr, dec, idx


def same_objects(a, b):
    return len(a) == len(b) and all(x is y for x, y in zip(a, b))


@pytest.mark.parametrize("flags", [KEYS, None], ids=["key_flags", "IsKeyFrame"])
def test_cut_at_a_key_frame_copies_and_never_touches_the_index(flags):
    mgr, dec, idx = manager(8, 8)
    out, keys = mgr.cut(FRAMES, 8, 13, flags)
    assert same_objects(out, FRAMES[8:14]) and keys == [True] + KEYS[9:14] and idx.asked == []
    mgr.attach_index(None)                             # and no index is needed
    out, keys = mgr.cut(FRAMES, 16, None, flags)
    assert same_objects(out, FRAMES[16:]) and keys == KEYS[16:]
    out, keys = mgr.cut(FRAMES, 0, 0, flags)
    assert same_objects(out, FRAMES[:1]) and keys == [True]
    assert dec.calls == [] and mgr.log == []           # nothing decoded


@pytest.mark.parametrize("flags", [KEYS, None], ids=["key_flags", "IsKeyFrame"])
def test_cut_at_an_inter_frame_asks_the_index_once(flags):
    mgr, dec, idx = manager(8, 10)                     # the index holds clip frames 8 .. 17
    out, keys = mgr.cut(FRAMES, 11, 20, flags)
    assert idx.asked == [3]
    assert out[0] == bytes([1, 11, 0xEE, 0xEE]) and same_objects(out[1:], FRAMES[12:21])
    assert keys == [True] + KEYS[12:21] and keys[5] is True   # (frame 16 keeps its flag)
    out, keys = mgr.cut(FRAMES, 17)                    # the index's last frame, to the end of the clip
    assert idx.asked == [3, 9] and len(out) == N - 17 and same_objects(out[1:], FRAMES[18:]) and keys == [True] + KEYS[18:]
    out, keys = mgr.cut(FRAMES, 9, 9, flags)
    assert idx.asked == [3, 9, 1] and len(out) == 1 and keys == [True]
    out, _ = mgr.cut(FRAMES, 9, N + 5, flags)          # `last` past the end: to the end
    assert len(out) == N - 9
    assert dec.calls == [] and mgr.log == []


def test_each_case_that_cannot_be_served_says_which():
    mgr, _, idx = manager()
    with pytest.raises(ValueError, match="no seek index is attached"):
        mgr.cut(FRAMES, 3, None, KEYS)
    mgr, _, idx = manager(8, 8)                        # clip frames 8 .. 15
    for first in (3, 17):
        with pytest.raises(ValueError, match="not in the attached seek index"):
            mgr.cut(FRAMES, first, None, KEYS)
    with pytest.raises(ValueError, match="before first"):
        mgr.cut(FRAMES, 10, 9, KEYS)
    with pytest.raises(ValueError, match="before first"):
        mgr.cut(FRAMES, 8, 7, KEYS)                    # (also at a key frame)
    for first in (-1, N):
        with pytest.raises(ValueError, match="not in the clip"):
            mgr.cut(FRAMES, first, None, KEYS)
    assert idx.asked == []
    mgr, _, idx = manager(8, 8, index=FakeIndex)       # an index object without KeyFrame (ScreenPressor's)
    with pytest.raises(ValueError, match="cannot make a key frame"):
        mgr.cut(FRAMES, 10, None, KEYS)
    assert same_objects(mgr.cut(FRAMES, 8, 9, KEYS)[0], FRAMES[8:10])


@pytest.mark.parametrize("codec, bpp, pal", [(CODEC_MSVC16, 16, None), (CODEC_MSVC8, 8, bytes(range(256)) * 4)], ids=["16-bit", "8-bit"])
def test_write_cut_reads_back_as_the_same_frames_and_flags(codec, bpp, pal):
    mgr, _, idx = manager(8, 10, codec=codec, bpp=bpp, pal=pal)
    want, want_keys = mgr.cut(FRAMES, 11, 20, KEYS)
    blob = mgr.write_cut(FRAMES, 11, 20, KEYS, fps=25.0)
    vi, frames, keys = avi.read_avi_indexed(blob)
    assert [bytes(f) for f in frames] == [bytes(f) for f in want] and list(keys) == want_keys
    assert (vi.X, vi.Y, vi.bpp, vi.codec, vi.nframes) == (W, H, bpp, codec, 10) and vi.fps == 25.0
    assert (vi.palette or None) == pal
    assert idx.asked == [3, 3]
