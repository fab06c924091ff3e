"""Manager.thin / write_thin — the policy alone, over a fake decoder and a fake index (no GPU): entry 0 follows `cut`; a later key
frame of the clip is copied; a frame that follows its predecessor directly is the caller's own object; every other entry is the
index's inter frame over the gap, ALL of one call from ONE DeltaFrames; the flags; each case that cannot be served says which it is;
and write_thin gives an AVI file that reads back as those frames and flags."""
import pytest

from jsplayer_amd import avi
from jsplayer_amd.avi import CODEC_MSVC16, CODEC_MSVC8
from test_player_cut_cpu import H, W, CutIndex, manager, same_objects
from test_player_index_cpu import FRAMES, KEYS, N, FakeIndex


class ThinIndex(CutIndex):
    def __init__(self, dec, first, count):
        super().__init__(dec, first, count)
        self.delta_calls = []

    def DeltaFrames(self, pairs):
        pairs = list(pairs)
        self.delta_calls.append(pairs)
        # an inter frame by FakeDecoder.IsKeyFrame, but the one over the gap (2, 7]: a gap that writes every block gives a key frame
        return [bytes([1 if (a, b) == (2, 7) else 0, self.first + b, 0xDD, self.first + a + 1]) for a, b in pairs]


def delta(a, b, key=False):
    return bytes([1 if key else 0, b, 0xDD, a + 1])


@pytest.mark.parametrize("flags", [KEYS, None], ids=["key_flags", "IsKeyFrame"])
def test_copied_own_object_and_delta_entries(flags):
    mgr, dec, idx = manager(8, 12, index=ThinIndex)           # the index holds clip frames 8 .. 19
    keep = [8, 9, 12, 13, 16, 19]
    out, keys = mgr.thin(FRAMES, keep, flags)
    assert idx.asked == []                                    # frame 8 is a key frame: copied
    assert idx.delta_calls == [[(1, 4), (8, 11)]]             # ONE call for the gaps 9 -> 12 and 16 -> 19, index frame numbers
    assert out[0] is FRAMES[8] and out[1] is FRAMES[9] and out[3] is FRAMES[13]
    assert out[4] is FRAMES[16]                               # a key frame of the clip behind a gap: copied, no Delta
    assert out[2] == delta(9, 12) and out[5] == delta(16, 19)
    assert keys == [True, False, False, False, True, False]
    assert dec.calls == [] and mgr.log == []                  # nothing decoded


def test_entry_0_at_an_inter_frame_is_the_indexs_key_frame_and_flags_follow_the_bytes():
    mgr, dec, idx = manager(8, 12, index=ThinIndex)
    out, keys = mgr.thin(FRAMES, [10, 15, 17, 18], KEYS)
    assert idx.asked == [2] and out[0] == bytes([1, 10, 0xEE, 0xEE])
    assert idx.delta_calls == [[(2, 7), (7, 9)]]
    assert out[1] == delta(10, 15, key=True) and out[2] == delta(15, 17) and out[3] is FRAMES[18]
    assert keys == [True, True, False, False]                 # the gap (2, 7] wrote every block: IsKeyFrame of the bytes says so
    out, keys = mgr.thin(FRAMES, [11], KEYS)                  # a single frame: cut's first frame alone
    assert len(out) == 1 and keys == [True] and idx.delta_calls == [[(2, 7), (7, 9)]]


def test_a_stride_and_no_index_where_none_is_needed():
    mgr, dec, idx = manager(0, N, index=ThinIndex)
    keep = list(range(0, N, 4))
    out, keys = mgr.thin(FRAMES, keep, KEYS)
    gaps = [(k - 4, k) for k in keep[1:] if not KEYS[k]]
    assert idx.delta_calls == [gaps] and idx.asked == []
    assert [o for o, k in zip(out, keep) if KEYS[k]] == [FRAMES[k] for k in keep if KEYS[k]]
    assert keys == [KEYS[k] for k in keep]
    mgr, dec, idx = manager()                                 # consecutive frames and key frames need no index at all
    out, keys = mgr.thin(FRAMES, [0, 1, 2, 8, 9, 16], KEYS)
    assert same_objects(out, [FRAMES[k] for k in (0, 1, 2, 8, 9, 16)]) and keys == [True, False, False, True, False, True]
    # the gap may start on the frame before the index: Delta from -1, the picture before the range
    mgr, dec, idx = manager(9, 8, index=ThinIndex)
    out, keys = mgr.thin(FRAMES, [8, 11], KEYS)
    assert idx.delta_calls == [[(-1, 2)]] and out[0] is FRAMES[8]


def test_each_case_that_cannot_be_served_says_which():
    mgr, _, idx = manager(8, 8, index=ThinIndex)              # clip frames 8 .. 15
    with pytest.raises(ValueError, match="keep is empty"):
        mgr.thin(FRAMES, [], KEYS)
    for keep in ([8, 8], [10, 9], [8, 12, 11]):
        with pytest.raises(ValueError, match="not strictly ascending"):
            mgr.thin(FRAMES, keep, KEYS)
    for keep in ([-1, 3], [8, N]):
        with pytest.raises(ValueError, match="not in the clip"):
            mgr.thin(FRAMES, keep, KEYS)
    for keep in ([3, 4], [8, 18], [8, 10, 20], [2, 10], [0, 10]):   # entry 0 at an inter frame outside; a gap's end, or its start, outside
        with pytest.raises(ValueError, match="not in the attached seek index"):
            mgr.thin(FRAMES, keep, KEYS)
    assert idx.asked == [] and idx.delta_calls == []          # refused before anything is asked of the index
    mgr, _, _ = manager()
    with pytest.raises(ValueError, match="no seek index is attached"):
        mgr.thin(FRAMES, [8, 10], KEYS)
    with pytest.raises(ValueError, match="no seek index is attached"):
        mgr.thin(FRAMES, [9, 10], KEYS)
    mgr, _, _ = manager(8, 8, index=CutIndex)                 # an index object without DeltaFrames
    with pytest.raises(ValueError, match="cannot span a gap"):
        mgr.thin(FRAMES, [8, 10], KEYS)
    assert len(mgr.thin(FRAMES, [9, 10, 11], KEYS)[0]) == 3   # ... serves what needs none
    mgr, _, _ = manager(8, 8, index=FakeIndex)                # ... and one without KeyFrame (ScreenPressor's)
    with pytest.raises(ValueError, match="cannot make a key frame"):
        mgr.thin(FRAMES, [9, 10], KEYS)


@pytest.mark.parametrize("codec, bpp, pal", [(CODEC_MSVC16, 16, None), (CODEC_MSVC8, 8, bytes(range(256)) * 4)], ids=["16-bit", "8-bit"])
def test_write_thin_reads_back_as_the_same_frames_and_flags(codec, bpp, pal):
    mgr, _, idx = manager(8, 12, index=ThinIndex, codec=codec, bpp=bpp, pal=pal)
    keep = [10, 15, 16, 17, 19]
    want, want_keys = mgr.thin(FRAMES, keep, KEYS)
    blob = mgr.write_thin(FRAMES, keep, KEYS, fps=2.0)
    vi, frames, keys = avi.read_avi_indexed(blob)
    assert [bytes(f) for f in frames] == [bytes(f) for f in want] and list(keys) == want_keys
    assert (vi.X, vi.Y, vi.bpp, vi.codec, vi.nframes) == (W, H, bpp, codec, len(keep)) and vi.fps == 2.0
    assert len(idx.delta_calls) == 2 and idx.delta_calls[0] == idx.delta_calls[1] == [(2, 7), (9, 11)]
