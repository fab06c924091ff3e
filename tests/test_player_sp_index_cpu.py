"""Manager with an index that cannot move the decoder (ScreenPressor's SpScrubIndex, `ADOPTS` false) — the policy alone, over a
fake decoder and a fake index (no GPU): a frame inside the index is one Show into a free buffer, and the decoder, its previous
buffer and the decode position stay where they were, so decoding continues correctly afterwards."""
import numpy as np
import pytest

from jsplayer_amd import player
from jsplayer_amd.avi import CODEC_SCREENPRESSOR, VideoInfo

N = 24
KEYS = [i % 8 == 0 for i in range(N)]                   # key frames 0, 8, 16
FRAMES = [bytes([1 if k else 0, i]) for i, k in enumerate(KEYS)]


class _Res:
    def __init__(self, data, sig):
        self.data_pnt, self.significant_changes = data, sig


class FakeDecoder:
    """A decoder without Seek / FindChange (ScreenPressor): pictures are filled with the frame's number, every call is logged, and
    a frame decoded out of order is an error (the entropy state is sequential)."""
    SEEKS = False
    FINDS_CHANGES = False

    def __init__(self):
        self.calls, self.prev, self.at = [], None, -1

    def Preinit(self, lines):
        pass

    def PreviousFrame(self):
        return self.prev

    def IsKeyFrame(self, f):
        return f[0] == 1

    def DecompressI(self, src, dst):
        self.calls.append(("I", src[1]))
        dst[:] = src[1]
        self.prev, self.at = dst, src[1]
        return 0

    def DecompressP(self, src, dst):
        assert src[1] == self.at + 1, f"inter frame {src[1]} decoded after frame {self.at}"
        self.calls.append(("P", src[1]))
        dst[:] = src[1]
        self.prev, self.at = dst, src[1]
        return _Res(dst, True)


class FakeScrubIndex:
    ADOPTS = False

    def __init__(self, dec, first, count, significance=None):
        self.dec, self.first, self.frames = dec, first, count
        self.significance = significance if significance is not None else [True] * count

    def Show(self, t, dst, adopt=False):
        assert not adopt, "a ScreenPressor index cannot adopt"
        assert dst is not self.dec.prev, "Show into the decoder's previous frame"
        self.dec.calls.append(("Show", self.first + t))
        dst[:] = self.first + t
        return _Res(dst, self.significance[t])


def _manager(dec, num_buffers=player.NUM_BUFFERS):
    vi = VideoInfo(X=4, Y=4, bpp=24, fps=15.0, nframes=N, codec=CODEC_SCREENPRESSOR, palette=None, riff_size=0)
    return player.Manager(vi, dec, lambda n: np.full(n, -1, dtype=np.int32), num_buffers=num_buffers)


def _shown(mgr, d):
    return int(mgr.buffers[d.buffer_index][0])


def test_step_back_is_one_show_per_frame_and_the_decoder_is_never_called():
    dec = FakeDecoder()
    mgr = _manager(dec)
    mgr.attach_index(FakeScrubIndex(dec, 0, N), 0)
    assert _shown(mgr, mgr.seek(FRAMES, N - 1, KEYS)) == N - 1
    seen = [N - 1]
    for _ in range(N + 1):                  # two steps past frame 0: it stays
        seen.append(_shown(mgr, mgr.prev_frame(FRAMES, KEYS)))
    assert seen == list(range(N - 1, -1, -1)) + [0, 0]
    assert all(c[0] == "Show" for c in dec.calls)
    assert [c[1] for c in dec.calls] == list(range(N - 1, -1, -1))      # one Show per frame; the held frame 0 needs none
    assert mgr.next_frame_to_decode == 0 and dec.prev is None


def test_decode_position_and_previous_buffer_are_untouched_and_decoding_goes_on():
    dec = FakeDecoder()
    mgr = _manager(dec)
    mgr.play(FRAMES[:11], key_flags=KEYS[:11])          # the decoder stands behind frame 10
    prev, prev_value = dec.prev, int(dec.prev[0])
    holds_before = list(mgr.holds)
    assert mgr.next_frame_to_decode == 11 and prev_value == 10
    mgr.attach_index(FakeScrubIndex(dec, 0, 12), 0)
    dec.calls.clear()
    for t in (0, 11, 1):                                # (frames no buffer holds: 2 .. 10 are still held from the play)
        d = mgr.seek(FRAMES, t, KEYS)
        assert d.index == t and _shown(mgr, d) == t and d.significant_changes is True
    assert dec.calls == [("Show", 0), ("Show", 11), ("Show", 1)]
    assert mgr.next_frame_to_decode == 11 and mgr._last_was_key is False
    assert dec.prev is prev and int(prev[0]) == prev_value, "the decoder's previous frame was written or replaced"
    for nb, h in enumerate(holds_before):               # the other holds stay (a slot taken for a Show shows that frame now)
        assert mgr.holds[nb] == h or mgr.holds[nb] in (range(0, 1), range(11, 12), range(1, 2))
    # a seek outside the index: the stretch being decoded leads there, so decoding goes on from frame 11 (FakeDecoder asserts the order)
    dec.calls.clear()
    d = mgr.seek(FRAMES, 13, KEYS)
    assert _shown(mgr, d) == 13
    assert dec.calls == [("P", 11), ("P", 12), ("P", 13)]
    # ... and sequential play after a Show continues from the decoder's own position
    mgr.seek(FRAMES, 3, KEYS)
    dec.calls.clear()
    d = mgr.worker(FRAMES[14], 14, None, KEYS[14])
    assert dec.calls == [("P", 14)] and _shown(mgr, d) == 14


def test_log_entry_carries_the_index_verdict():
    dec = FakeDecoder()
    mgr = _manager(dec)
    sig = [i % 3 == 0 for i in range(N)]
    mgr.attach_index(FakeScrubIndex(dec, 0, N, sig), 0)
    for t in (7, 6, 8):
        d = mgr.seek(FRAMES, t, KEYS)
        assert d.significant_changes == sig[t] and d.key == KEYS[t] and mgr.log[-1] is d


def test_skip_stills_uses_the_index_verdicts():
    dec = FakeDecoder()
    mgr = _manager(dec)
    sig = [True] + [False] * 9 + [True] + [False] * (N - 11)
    mgr.attach_index(FakeScrubIndex(dec, 0, N, sig), 0)
    mgr.seek(FRAMES, 0, KEYS)
    d = mgr.skip_stills(FRAMES, KEYS)
    assert d.index == 10 and _shown(mgr, d) == 10
    d = mgr.skip_stills(FRAMES, KEYS)
    assert d.index == N - 1                               # nothing changes after 10: the last frame
    assert dec.calls == [("Show", 0), ("Show", 10), ("Show", N - 1)]
    assert mgr.next_frame_to_decode == 0


def test_walk_back_through_more_frames_than_buffers():
    dec = FakeDecoder()
    mgr = _manager(dec, num_buffers=3)
    mgr.play(FRAMES[:2], key_flags=KEYS[:2])
    prev = dec.prev
    mgr.attach_index(FakeScrubIndex(dec, 0, N), 0)
    mgr.seek(FRAMES, N - 1, KEYS)
    for t in range(N - 2, 1, -1):
        assert _shown(mgr, mgr.prev_frame(FRAMES, KEYS)) == t
    assert dec.prev is prev and int(prev[0]) == 1


def test_no_thumbnails_from_a_scrub_index():
    dec = FakeDecoder()
    mgr = _manager(dec)
    mgr.attach_index(FakeScrubIndex(dec, 0, N), 0)
    with pytest.raises(ValueError):
        mgr.preview(3)
    with pytest.raises(ValueError):
        mgr.filmstrip(4)
