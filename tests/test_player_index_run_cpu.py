"""Manager.run_from_index — the policy alone, over the fake decoder and a fake adopting index that can Play (no GPU): a run of
frames of an adopting index, forward or reverse, goes out in batches of the buffers that are not the decoder's previous frame, one
Play per batch, the last frame shown is adopted in the final batch only, and decoding continues from it."""
import numpy as np
import pytest

from jsplayer_amd import player
from jsplayer_amd.avi import CODEC_MSVC16, VideoInfo
from test_player_index_cpu import FRAMES, KEYS, N, FakeDecoder, FakeIndex, _Res, _shown


class FakeAdoptingPlayIndex(FakeIndex):
    """FakeIndex plus Play: every call is logged with its destinations, which must be distinct and never the decoder's previous
    frame; `quiet` frames write nothing (as frames before the first adopting one: data_pnt is the previous frame of the build's
    time)."""
    ADOPTS = True

    def __init__(self, dec, first, count, significance=None, quiet=0, prev_at_build=None):
        super().__init__(dec, first, count, significance)
        self.plays, self.quiet, self.prev_at_build = [], quiet, prev_at_build

    def Play(self, first, dsts, stride=1, adopt=None):
        dsts = list(dsts)
        assert 0 <= first and first + (len(dsts) - 1) * stride < self.frames and stride >= 1 and dsts
        assert all(d is not self.dec.prev for d in dsts), "Play into the decoder's previous frame"
        assert len({id(d) for d in dsts}) == len(dsts), "the same buffer twice"
        assert adopt is None or 0 <= adopt < len(dsts)
        self.dec.calls.append(("Play", self.first + first, len(dsts), stride, adopt))
        self.plays.append((first, dsts, stride, adopt))
        out = []
        for k, d in enumerate(dsts):
            t = first + k * stride
            if t < self.quiet:
                out.append(_Res(self.prev_at_build, False))
            else:
                d[:] = self.first + t
                out.append(_Res(d, self.significance[t]))
        if adopt is not None:
            self.dec.prev = dsts[adopt] if first + adopt * stride >= self.quiet else self.prev_at_build
        return out


def _manager(dec, num_buffers=player.NUM_BUFFERS):
    vi = VideoInfo(X=4, Y=4, bpp=16, fps=15.0, nframes=N, codec=CODEC_MSVC16, palette=None, riff_size=0)
    return player.Manager(vi, dec, lambda n: np.full(n, -1, dtype=np.int32), num_buffers=num_buffers)


def test_forward_batches_adopt_only_in_the_last_and_play_goes_on():
    dec = FakeDecoder()
    mgr = _manager(dec)                                 # 9 buffers, no previous frame: batches of 9
    idx = FakeAdoptingPlayIndex(dec, 0, N)
    mgr.attach_index(idx, 0)
    seen = []
    out = mgr.run_from_index(2, on_frame=lambda d, buf: seen.append((d.index, int(buf[0]))), key_flags=KEYS)
    assert dec.calls == [("Play", 2, 9, 1, None), ("Play", 11, 9, 1, None), ("Play", 20, 4, 1, 3)]
    assert seen == [(t, t) for t in range(2, N)]        # in order, each buffer holding its frame when on_frame sees it
    assert [d.index for d in out] == list(range(2, N)) and mgr.log == out
    assert [d.key for d in out] == KEYS[2:]
    assert [d.significant_changes for d in out] == [None if k else True for k in KEYS[2:]]
    assert mgr.frame_of_interest == N - 1 and mgr.next_frame_to_decode == N and mgr._last_was_key is KEYS[N - 1]
    assert dec.prev is mgr.buffers[out[-1].buffer_index] and int(dec.prev[0]) == N - 1


def test_the_previous_buffer_is_never_a_destination_and_the_decoder_ends_at_the_last_frame():
    dec = FakeDecoder()
    mgr = _manager(dec)
    mgr.play(FRAMES[:11], key_flags=KEYS[:11])
    prev = dec.prev
    assert int(prev[0]) == 10 and mgr.next_frame_to_decode == 11
    idx = FakeAdoptingPlayIndex(dec, 0, N)
    mgr.attach_index(idx, 0)
    dec.calls.clear()
    out = mgr.run_from_index(0, 13, key_flags=KEYS)      # 8 buffers that are not the previous frame: 8 + 5
    assert dec.calls == [("Play", 0, 8, 1, None), ("Play", 8, 5, 1, 4)]
    assert all(all(d is not prev for d in dsts) for _, dsts, _, _ in idx.plays)
    assert int(prev[0]) == 10, "the decoder's previous frame at the start was written"
    assert mgr.next_frame_to_decode == 13 and mgr.frame_of_interest == 12 and mgr._last_was_key is False
    assert int(dec.prev[0]) == 12
    for d in out[-5:]:
        assert mgr.holds[d.buffer_index] == range(d.index, d.index + 1) and _shown(mgr, d) == d.index
    # play goes on from the frame adopted
    dec.calls.clear()
    d = mgr.worker(FRAMES[13], 13, None, KEYS[13])
    assert dec.calls == [("P", 13)] and _shown(mgr, d) == 13


def test_reverse_takes_the_lowest_frame_first_reverses_the_buffers_and_adopts_frame_zero_of_the_run():
    dec = FakeDecoder()
    mgr = _manager(dec, num_buffers=3)                  # 4 buffers, no previous frame yet: batches of 4
    idx = FakeAdoptingPlayIndex(dec, 4, 16)             # clip frames 4 .. 19
    mgr.attach_index(idx, 4)
    seen = []
    out = mgr.run_from_index(15, 10, reverse=True, on_frame=lambda d, buf: seen.append((d.index, int(buf[0]))), key_flags=KEYS)
    assert dec.calls == [("Play", 12, 4, 1, None), ("Play", 8, 4, 1, None), ("Play", 6, 2, 1, 0)]
    assert seen == [(t, t) for t in range(15, 5, -1)]
    # the buffer list of a batch is the shown order reversed: its first buffer is the one shown last
    slots = list(range(4))
    for (first, dsts, _, _), k0 in zip(idx.plays, (0, 4, 8)):
        m = len(dsts)
        assert [mgr._slot_of(d) for d in dsts] == slots[:m][::-1]
    assert mgr.next_frame_to_decode == 7 and mgr.frame_of_interest == 6 and int(dec.prev[0]) == 6
    assert mgr._last_was_key is False
    # reverse with a stride and count=None: down to the index's first frame
    dec.calls.clear()
    out = mgr.run_from_index(19, None, 5, reverse=True, key_flags=KEYS)
    assert [d.index for d in out] == [19, 14, 9, 4]
    # (the frame adopted above is the previous frame now: 3 buffers are left for a batch)
    assert dec.calls == [("Play", 9, 3, 5, None), ("Play", 4, 1, 5, 0)]
    assert mgr.next_frame_to_decode == 5 and int(dec.prev[0]) == 4


def test_stride_count_verdicts_and_a_key_frame_at_the_end():
    dec = FakeDecoder()
    mgr = _manager(dec, num_buffers=4)                  # 5 buffers: batches of 5
    sig = [i % 3 == 0 for i in range(20)]
    idx = FakeAdoptingPlayIndex(dec, 4, 20, sig)        # clip frames 4 .. 23
    mgr.attach_index(idx, 4)
    out = mgr.run_from_index(5, None, 3, key_flags=KEYS)
    want = list(range(5, 24, 3))
    assert [d.index for d in out] == want
    assert dec.calls == [("Play", 5, 5, 3, None), ("Play", 20, 2, 3, 1)]
    assert [d.significant_changes for d in out] == [None if KEYS[t] else sig[t - 4] for t in want]
    assert mgr.next_frame_to_decode == 24 and mgr._last_was_key is False
    out = mgr.run_from_index(16, 1, 7, key_flags=KEYS)
    assert [d.index for d in out] == [16] and dec.calls[-1] == ("Play", 16, 1, 7, 0)
    assert mgr._last_was_key is True and out[0].key is True and mgr.next_frame_to_decode == 17


def test_a_frame_that_wrote_nothing_extends_the_hold_of_the_buffer_that_shows_it():
    dec = FakeDecoder()
    mgr = _manager(dec)
    mgr.play(FRAMES[:3], key_flags=KEYS[:3])
    prev = dec.prev
    slot = mgr._slot_of(prev)
    assert mgr.holds[slot] == range(2, 3)
    idx = FakeAdoptingPlayIndex(dec, 3, 10, quiet=2, prev_at_build=prev)   # clip frames 3 and 4 code nothing
    mgr.attach_index(idx, 3)
    out = mgr.run_from_index(3, 4, key_flags=KEYS)
    assert [d.buffer_index for d in out[:2]] == [slot, slot] and mgr.holds[slot] == range(2, 5)
    assert [_shown(mgr, d) for d in out] == [2, 2, 5, 6]
    assert int(prev[0]) == 2 and int(dec.prev[0]) == 6


def test_the_four_value_errors():
    dec = FakeDecoder()
    mgr = _manager(dec)
    with pytest.raises(ValueError):                     # no index attached
        mgr.run_from_index(0, 4)
    mgr.attach_index(FakeAdoptingPlayIndex(dec, 8, 8), 8)       # clip frames 8 .. 15
    for start, count, stride, rev in ((7, 2, 1, False), (8, 9, 1, False), (16, 1, 1, False), (9, 3, 4, False), (16, None, 1, False),
                                      (9, 3, 1, True), (7, None, 1, True), (15, 3, 4, True), (8, 1, 0, False)):
        with pytest.raises(ValueError):                 # a frame outside the index (or no stride at all)
            mgr.run_from_index(start, count, stride, reverse=rev)
    scrub = FakeAdoptingPlayIndex(dec, 0, N)
    scrub.ADOPTS = False
    mgr.attach_index(scrub, 0)
    with pytest.raises(ValueError):                     # an index that does not adopt (ScreenPressor's: play_from_index serves it)
        mgr.run_from_index(0, 4)
    mgr.attach_index(FakeIndex(dec, 0, N), 0)
    with pytest.raises(ValueError):                     # an index object without Play
        mgr.run_from_index(0, 4)
    assert dec.calls == [] and mgr.log == [] and all(h is None for h in mgr.holds)
    assert all(int(b[0]) == -1 for b in mgr.buffers)
    assert mgr.next_frame_to_decode == 0 and mgr.frame_of_interest == 0
