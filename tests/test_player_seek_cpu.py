"""Manager.seek — the seek branch of GetDecompressedFrame (Manager.hx:216-259) — over the oracle decoders (no GPU): the
frame-by-frame path every decoder without a composed Seek takes, and the seek policy itself (nearest key frame,
DataLoader.hx:125-132; trash on a seek outside the stretch being decoded; held frames shown without a decode)."""
import numpy as np
import pytest

from jsplayer_amd import player
from jsplayer_amd import streamgen as sg
from jsplayer_amd.avi import CODEC_MSVC16, CODEC_MSVC8, CODEC_SCREENPRESSOR, VideoInfo
from oracle_binding import OracleMSVideo1, OracleScreenPressor


class _Res:
    def __init__(self, data, sig):
        self.data_pnt, self.significant_changes = data, sig


class _Counting:
    """An oracle decoder with the IVideoCodec return shapes, counting the decode calls it gets."""

    def __init__(self, o):
        self.o, self.calls = o, []

    def __getattr__(self, k):
        return getattr(self.o, k)

    def DecompressI(self, src, dst):
        self.calls.append("I")
        return self.o.DecompressI(src, dst)

    def DecompressP(self, src, dst):
        self.calls.append("P")
        return _Res(*self.o.DecompressP(src, dst))


def _make_vi(codec, w, h, bpp, n, pal):
    return VideoInfo(X=w, Y=h, bpp=bpp, fps=15.0, nframes=n, codec=codec, palette=pal, riff_size=0)


def _clip(what, n=24):
    w, h = 64, 48
    if what == "sp":
        chunks, keys, _ = sg.sp_clip(5, w, h, n, key_every=8)
        mk = lambda: _Counting(OracleScreenPressor(w, h, 24))
        return _make_vi(CODEC_SCREENPRESSOR, w, h, 24, n, None), chunks, keys, mk
    bits = 16 if what == "m16" else 8
    frames, keys, pal = sg.msv1_clip(7, w, h, n, bits=bits, p_mix=sg.msv1_p_mix(0.7, 6.0), key_every=8)
    mk = (lambda: _Counting(OracleMSVideo1(16, w, h))) if bits == 16 else (lambda: _Counting(OracleMSVideo1(8, w, h, pal)))
    return _make_vi(CODEC_MSVC16 if bits == 16 else CODEC_MSVC8, w, h, bits, n, pal), frames, keys, mk


def _manager(vi, dec):
    return player.Manager(vi, dec, lambda n: np.zeros(n, dtype=np.int32))


def _played(vi, frames, keys, mk):
    """Picture of every frame from a plain play() from 0."""
    mgr = _manager(vi, mk())
    pics = []
    mgr.play(frames, on_frame=lambda d, buf: pics.append(buf.copy()), key_flags=keys)
    return pics


def test_nearest_key_frame_clamps_and_walks_back():
    flags = [True, False, False, True, False, False]
    assert player.nearest_key_frame(flags, 0) == 0
    assert player.nearest_key_frame(flags, 2) == 0
    assert player.nearest_key_frame(flags, 3) == 3
    assert player.nearest_key_frame(flags, 5) == 3
    assert player.nearest_key_frame(flags, 99) == 3          # clamped to the last frame first
    assert player.nearest_key_frame([], 7) == 0
    assert player.nearest_key_frame([False, False, False], 2) == 0   # no key flag at all: frame 0
    assert player.nearest_key_frame([True, None, True], 1) == 0      # a missing flag is not a key frame
    assert player.nearest_key_frame([True, False, True], 9, count=5) == 2   # flags shorter than the clip: the rest are not key
    assert player.nearest_key_frame(lambda i: i % 4 == 0, 11, count=10) == 8


@pytest.mark.parametrize("what", ["m16", "m8", "sp"])
def test_seek_shows_what_play_shows(what):
    vi, frames, keys, mk = _clip(what)
    pics = _played(vi, frames, keys, mk)
    for target in (0, 1, 5, 8, 9, 15, 23):
        mgr = _manager(vi, mk())
        d = mgr.seek(frames, target, keys)
        assert d.index == target
        assert np.array_equal(mgr.buffers[d.buffer_index], pics[target]), f"{what}: seek to {target}"
        assert mgr.next_frame_to_decode == target + 1
    # one Manager, a tour of seeks backwards and forwards (held frames among them), each followed by a few frames shown the
    # way a player shows them: worker() for the next frame to decode, the seek branch otherwise
    mgr = _manager(vi, mk())
    for target in (17, 3, 12, 13, 22, 0, 9, 11):
        d = mgr.seek(frames, target, keys)
        assert np.array_equal(mgr.buffers[d.buffer_index], pics[target]), f"{what}: tour, seek to {target}"
        for i in range(target + 1, min(target + 3, len(frames))):
            d = mgr.worker(frames[i], i, None, keys[i]) if mgr.next_frame_to_decode == i else mgr.seek(frames, i, keys)
            assert np.array_equal(mgr.buffers[d.buffer_index], pics[i]), f"{what}: frame {i} after the seek to {target}"


def test_seek_policy_counts_decodes():
    vi, frames, keys, mk = _clip("m16")
    dec = mk()
    mgr = _manager(vi, dec)
    mgr.seek(frames, 13, keys)                       # key frames at 0, 8, 16: decodes 8..13
    assert dec.calls == ["I", "P", "P", "P", "P", "P"]
    dec.calls.clear()
    mgr.seek(frames, 15, keys)                       # forward inside the interval: continues at 14
    assert dec.calls == ["P", "P"]
    assert all(h is None or h.stop <= 16 for h in mgr.holds)
    dec.calls.clear()
    held = [h for h in mgr.holds if h is not None and h.start <= 15 < h.stop]
    assert held
    d = mgr.seek(frames, 15, keys)                   # a frame a buffer holds: shown without a decode
    assert dec.calls == [] and mgr.holds[d.buffer_index] is not None
    dec.calls.clear()
    mgr.seek(frames, 10, keys)                       # backwards, still held: no decode
    assert dec.calls == []
    mgr.seek(frames, 3, keys)                        # backwards, not held: every hold trashed, decoding restarts at 0
    assert dec.calls == ["I", "P", "P", "P"]
    assert all(h is None or h.stop <= 4 for h in mgr.holds)
    dec.calls.clear()
    mgr.seek(frames, 18, keys)                       # past the next key frame (16): restart there, not at 4
    assert dec.calls == ["I", "P", "P"]
    dec.calls.clear()
    mgr.seek(frames, 23, None)                       # no key flags: the bytes are scanned (IsKeyFrame); 16 is the nearest
    assert dec.calls == ["P"] * 5                    # ... and 19..23 continue the stretch 16..18
