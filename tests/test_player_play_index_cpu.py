"""Manager.play_from_index — the policy alone, over the fake decoder and a fake index that can Play (no GPU): a run of frames of a
non-adopting index goes out in batches of the buffers that are not the decoder's previous frame, one Play per batch, and the
decoder, its previous buffer and the decode position stay where they were."""
import pytest

from test_player_sp_index_cpu import FRAMES, KEYS, N, FakeDecoder, FakeScrubIndex, _Res, _manager, _shown


class FakePlayIndex(FakeScrubIndex):
    """FakeScrubIndex plus Play: every call is logged with its destinations, which must be distinct and never the decoder's
    previous frame."""

    def __init__(self, dec, first, count, significance=None):
        super().__init__(dec, first, count, significance)
        self.plays = []

    def Play(self, first, dsts, stride=1):
        dsts = list(dsts)
        assert 0 <= first and first + (len(dsts) - 1) * stride < self.frames and stride >= 1 and dsts
        assert all(d is not self.dec.prev for d in dsts), "Play into the decoder's previous frame"
        assert len({id(d) for d in dsts}) == len(dsts), "the same buffer twice"
        self.dec.calls.append(("Play", self.first + first, len(dsts), stride))
        self.plays.append((first, dsts, stride))
        out = []
        for k, d in enumerate(dsts):
            d[:] = self.first + first + k * stride
            out.append(_Res(d, self.significance[first + k * stride]))
        return out


def test_one_play_per_batch_and_the_decoder_is_never_called():
    dec = FakeDecoder()
    mgr = _manager(dec)                                 # 9 buffers, no previous frame: batches of 9
    idx = FakePlayIndex(dec, 0, N)
    mgr.attach_index(idx, 0)
    seen = []
    out = mgr.play_from_index(2, on_frame=lambda d, buf: seen.append((d.index, int(buf[0]))), key_flags=KEYS)
    assert dec.calls == [("Play", 2, 9, 1), ("Play", 11, 9, 1), ("Play", 20, 4, 1)]
    assert seen == [(t, t) for t in range(2, N)]        # in order, each buffer holding its frame when on_frame sees it
    assert [d.index for d in out] == list(range(2, N)) and mgr.log == out
    assert [d.key for d in out] == KEYS[2:]
    assert mgr.frame_of_interest == N - 1
    assert mgr.next_frame_to_decode == 0 and dec.prev is None


def test_the_previous_buffer_is_never_a_destination_and_decoding_goes_on():
    dec = FakeDecoder()
    mgr = _manager(dec, num_buffers=3)                  # 4 buffers, one of them the previous frame: batches of 3
    mgr.play(FRAMES[:11], key_flags=KEYS[:11])
    prev, log_before = dec.prev, len(mgr.log)
    assert int(prev[0]) == 10 and mgr.next_frame_to_decode == 11
    idx = FakePlayIndex(dec, 0, 12)
    mgr.attach_index(idx, 0)
    dec.calls.clear()
    out = mgr.play_from_index(0, 8)
    assert dec.calls == [("Play", 0, 3, 1), ("Play", 3, 3, 1), ("Play", 6, 2, 1)]
    assert all(all(d is not prev for d in dsts) for _, dsts, _ in idx.plays)
    assert dec.prev is prev and int(prev[0]) == 10, "the decoder's previous frame was written or replaced"
    assert mgr.next_frame_to_decode == 11 and mgr._last_was_key is False
    assert len(mgr.log) == log_before + 8
    # holds: the last batch's frames (and what is left of the batch before it) are where the log says, the previous slot keeps its own
    prev_slot = mgr._slot_of(prev)
    assert mgr.holds[prev_slot] == range(10, 11)
    for d in out[-2:]:
        assert mgr.holds[d.buffer_index] == range(d.index, d.index + 1) and _shown(mgr, d) == d.index
    held = sorted(h.start for nb, h in enumerate(mgr.holds) if h is not None and nb != prev_slot)
    assert held == [5, 6, 7]
    # decoding goes on from where the decoder really stands (FakeDecoder asserts the order)
    dec.calls.clear()
    d = mgr.seek(FRAMES, 13, KEYS)                     # (outside the index: the stretch being decoded leads there)
    assert dec.calls == [("P", 11), ("P", 12), ("P", 13)] and _shown(mgr, d) == 13


def test_stride_count_and_verdicts():
    dec = FakeDecoder()
    mgr = _manager(dec, num_buffers=4)                  # 5 buffers: batches of 5
    sig = [i % 3 == 0 for i in range(20)]
    idx = FakePlayIndex(dec, 4, 20, sig)                # the index covers clip frames 4 .. 23
    mgr.attach_index(idx, 4)
    order = []
    out = mgr.play_from_index(5, None, 3, on_frame=lambda d, buf: order.append(d.index))
    want = list(range(5, 24, 3))
    assert [d.index for d in out] == want == order
    assert dec.calls == [("Play", 5, 5, 3), ("Play", 20, 2, 3)]
    assert [d.significant_changes for d in out] == [sig[t - 4] for t in want]
    assert [_shown(mgr, d) for d in out[-2:]] == want[-2:]
    assert mgr._known_significance()[20] == sig[16]
    out = mgr.play_from_index(23, 1, 7)
    assert [d.index for d in out] == [23] and dec.calls[-1] == ("Play", 23, 1, 7)


def test_the_four_value_errors():
    dec = FakeDecoder()
    mgr = _manager(dec)
    with pytest.raises(ValueError):                     # no index attached
        mgr.play_from_index(0, 4)
    mgr.attach_index(FakePlayIndex(dec, 8, 8), 8)       # clip frames 8 .. 15
    for start, count, stride in ((7, 2, 1), (8, 9, 1), (16, 1, 1), (9, 3, 4), (16, None, 1)):
        with pytest.raises(ValueError):                 # a frame outside the index
            mgr.play_from_index(start, count, stride)
    adopting = FakePlayIndex(dec, 0, N)
    adopting.ADOPTS = True
    mgr.attach_index(adopting, 0)
    with pytest.raises(ValueError):                     # the index adopts (MSVideo1's SeekIndex)
        mgr.play_from_index(0, 4)
    mgr.attach_index(FakeScrubIndex(dec, 0, N), 0)
    with pytest.raises(ValueError):                     # an index object without Play
        mgr.play_from_index(0, 4)
    assert dec.calls == [] and mgr.log == [] and all(h is None for h in mgr.holds)
    assert all(int(b[0]) == -1 for b in mgr.buffers)
