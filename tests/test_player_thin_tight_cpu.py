"""Manager.thin / write_thin with tight=True — the policy alone, over a fake decoder and a fake index (no GPU): the flag reaches the ONE
DeltaFrames call and nothing else changes — entry 0, copied key frames, directly following frames and the flags are `thin`'s; an index
object whose DeltaFrames takes no `tight` is refused before anything is asked of it."""
import pytest

from jsplayer_amd import avi
from test_player_cut_cpu import manager
from test_player_index_cpu import FRAMES, KEYS, N
from test_player_thin_cpu import ThinIndex, delta


class TightIndex(ThinIndex):
    """ThinIndex whose DeltaFrames takes `tight`: a tight frame says so in its third byte."""

    def __init__(self, dec, first, count):
        super().__init__(dec, first, count)
        self.tight_flags = []

    def DeltaFrames(self, pairs, tight=False):
        made = super().DeltaFrames(pairs)
        self.tight_flags.append(tight)
        return [f[:2] + bytes([0x77]) + f[3:] for f in made] if tight else made


def tightened(frame):
    return frame[:2] + bytes([0x77]) + frame[3:]


@pytest.mark.parametrize("flags", [KEYS, None], ids=["key_flags", "IsKeyFrame"])
def test_the_flag_reaches_exactly_one_delta_call_and_every_other_entry_is_thins(flags):
    keep = [8, 9, 12, 13, 16, 19]
    mgr, dec, idx = manager(8, 12, index=TightIndex)
    plain, plain_keys = mgr.thin(FRAMES, keep, flags)
    assert idx.tight_flags == [False] and idx.delta_calls == [[(1, 4), (8, 11)]]
    out, keys = mgr.thin(FRAMES, keep, flags, tight=True)
    assert idx.tight_flags == [False, True]                   # ONE more call, with the flag
    assert idx.delta_calls == [[(1, 4), (8, 11)]] * 2 and idx.asked == []
    assert out[2] == tightened(delta(9, 12)) and out[5] == tightened(delta(16, 19))
    for j in (0, 1, 3, 4):                                    # copied key frames and directly following frames: the caller's objects
        assert out[j] is plain[j] is FRAMES[keep[j]]
    assert keys == plain_keys == [True, False, False, False, True, False]
    assert dec.calls == [] and mgr.log == []


def test_entry_0_and_the_flags_follow_thin():
    mgr, dec, idx = manager(8, 12, index=TightIndex)
    out, keys = mgr.thin(FRAMES, [10, 15, 17, 18], KEYS, tight=True)
    assert idx.asked == [2] and out[0] == bytes([1, 10, 0xEE, 0xEE])
    assert idx.delta_calls == [[(2, 7), (7, 9)]] and idx.tight_flags == [True]
    assert out[1] == tightened(delta(10, 15, key=True)) and out[2] == tightened(delta(15, 17)) and out[3] is FRAMES[18]
    assert keys == [True, True, False, False]                 # IsKeyFrame of the bytes the tight call made
    out, keys = mgr.thin(FRAMES, [11], KEYS, tight=True)      # a single frame, and frames that need no gap: no DeltaFrames call
    assert len(out) == 1 and idx.tight_flags == [True]
    mgr.thin(FRAMES, [8, 9, 10, 16], KEYS, tight=True)
    assert idx.tight_flags == [True]
    mgr, dec, idx = manager(0, N, index=TightIndex)           # tight=False is the call without the keyword's effect
    assert mgr.thin(FRAMES, list(range(0, N, 4)), KEYS, tight=False) == mgr.thin(FRAMES, list(range(0, N, 4)), KEYS)
    assert idx.tight_flags == [False, False]


def test_an_index_whose_delta_frames_takes_no_tight_is_refused():
    mgr, _, idx = manager(8, 8, index=ThinIndex)              # DeltaFrames(pairs) only
    with pytest.raises(ValueError, match="cannot span a gap tightly"):
        mgr.thin(FRAMES, [8, 10], KEYS, tight=True)
    assert idx.delta_calls == [] and idx.asked == []          # refused before anything is asked of the index
    assert len(mgr.thin(FRAMES, [8, 10], KEYS)[0]) == 2       # ... which serves the call without the flag,
    assert len(mgr.thin(FRAMES, [9, 10, 11], KEYS, tight=True)[0]) == 3   # and what needs no gap
    with pytest.raises(ValueError, match="cannot span a gap tightly"):
        mgr.write_thin(FRAMES, [8, 10], KEYS, tight=True)


def test_write_thin_passes_the_flag():
    mgr, _, idx = manager(8, 12, index=TightIndex)
    keep = [10, 15, 16, 17, 19]
    want, want_keys = mgr.thin(FRAMES, keep, KEYS, tight=True)
    blob = mgr.write_thin(FRAMES, keep, KEYS, fps=2.0, tight=True)
    vi, frames, keys = avi.read_avi_indexed(blob)
    assert [bytes(f) for f in frames] == [bytes(f) for f in want] and list(keys) == want_keys
    assert idx.tight_flags == [True, True]
    plain = avi.read_avi_indexed(mgr.write_thin(FRAMES, keep, KEYS, fps=2.0))[1]
    assert idx.tight_flags == [True, True, False] and [bytes(f) for f in plain] != [bytes(f) for f in want]
