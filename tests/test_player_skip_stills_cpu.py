"""Manager.skip_stills — SkipStills (Manager.hx:289-317) over FindPossibleChange (DataLoader.hx:239-252) and the SeekTo that
Main.play_timer does with its answer — over the oracle decoders (no GPU): the frame-by-frame path every decoder without
FindChange takes, the use of significance already known, and landing on the last frame when nothing changes."""
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


W, H = 64, 48


def _idle_msv1(bits):
    """A key frame, then stretches of all-skip frames and blocks recoded with their own colour (the 16-bit stage-2 compare
    says no), with real changes at 4, 9 and 15 and an idle tail: significance 1 only there (and at the key frames)."""
    frames, keys, pal = sg.msv1_clip(7, W, H, 1, bits=bits)
    key = frames[0]
    nb = (W // 4) * (H // 4)
    skip_all = bytes([nb & 0xFF, 0x84 + (nb >> 8)])
    change_last_row = (bytes([(nb - W // 4) & 0xFF, 0x84 + ((nb - W // 4) >> 8)]) +
                       (bytes([0x00, 0x80]) if bits == 16 else bytes([0x07, 0x80])) * (W // 4))
    out, flags = [key], [True]
    for i in range(1, 20):
        if i in (4, 9, 15):
            out.append(change_last_row if i != 9 else change_last_row[:-2] + (b"\x1f\x80" if bits == 16 else b"\x09\x80"))
        elif i == 12:
            out.append(key)        # a key frame: the Manager's rule (pixels against the frame before)
        else:
            out.append(skip_all)
        flags.append(i == 12)
    return out, flags, pal


def _vi(codec, bpp, n, pal):
    return VideoInfo(X=W, Y=H, bpp=bpp, fps=15.0, nframes=n, codec=codec, palette=pal, riff_size=0)


def _manager(vi, dec):
    return player.Manager(vi, dec, lambda n: np.zeros(n, dtype=np.int32))


def _played(vi, frames, keys, mk):
    mgr = _manager(vi, mk())
    pics = []
    mgr.play(frames, on_frame=lambda d, buf: pics.append(buf.copy()), key_flags=keys)
    return mgr.log, pics


def _expected(log, start):
    for d in log[start:]:
        if d.significant_changes:
            return d.index
    return len(log) - 1


@pytest.mark.parametrize("bits", [16, 8])
def test_skip_stills_lands_on_each_change_then_the_last_frame(bits):
    frames, keys, pal = _idle_msv1(bits)
    vi = _vi(CODEC_MSVC16 if bits == 16 else CODEC_MSVC8, bits, len(frames), pal)
    mk = lambda: _Counting(OracleMSVideo1(bits, W, H, pal))
    log, pics = _played(vi, frames, keys, mk)
    mgr = _manager(vi, mk())
    mgr.worker(frames[0], 0, None, True)
    landings = []
    while mgr.frame_of_interest < len(frames) - 1:
        want = _expected(log, mgr.frame_of_interest + 1)
        d = mgr.skip_stills(frames, keys)
        assert d.index == want
        assert mgr.frame_of_interest == want and mgr.next_frame_to_decode == want + 1
        assert np.array_equal(mgr.buffers[d.buffer_index], pics[want]), f"landing {want}"
        landings.append(want)
    assert landings[-1] == len(frames) - 1
    if bits == 16:
        assert landings[:3] == [4, 9, 12]
    # at the last frame, a skip stays there
    assert mgr.skip_stills(frames, keys).index == len(frames) - 1


def test_known_significance_is_used_and_the_fallback_counts_decodes():
    frames, keys, pal = _idle_msv1(16)
    vi = _vi(CODEC_MSVC16, 16, len(frames), pal)
    dec = _Counting(OracleMSVideo1(16, W, H))
    mgr = _manager(vi, dec)
    mgr.worker(frames[0], 0, None, True)
    dec.calls.clear()
    assert mgr.skip_stills(frames, keys).index == 4       # frames 1..4 decoded one by one, stopping at the change
    assert dec.calls == ["P"] * 4
    dec.calls.clear()
    assert mgr.skip_stills(frames, keys).index == 9
    assert dec.calls == ["P"] * 5
    # back to frame 1 (held), skip: frames 2..4 are known — the change at 4 is shown from the buffer holding it, no decode
    dec.calls.clear()
    mgr.seek(frames, 1, keys)
    d = mgr.skip_stills(frames, keys)
    assert d.index == 4 and dec.calls == []
    # back to the start, the holds gone: the known change at 9 is reached through seek() (decoding 0..9), still no re-judging
    dec.calls.clear()
    mgr.holds = [None] * len(mgr.buffers)
    mgr.seek(frames, 5, keys)
    dec.calls.clear()
    d = mgr.skip_stills(frames, keys)
    assert d.index == 9 and dec.calls == ["P"] * 4
    # past everything known: decoding goes on from 10 frame by frame up to the key frame at 12
    dec.calls.clear()
    assert mgr.skip_stills(frames, keys).index == 12
    assert dec.calls == ["P", "P", "I"]


def test_screenpressor_falls_back_frame_by_frame():
    chunks, keys, _ = sg.sp_clip(5, W, H, 16, key_every=8)
    vi = _vi(CODEC_SCREENPRESSOR, 24, len(chunks), None)
    mk = lambda: _Counting(OracleScreenPressor(W, H, 24))
    log, pics = _played(vi, chunks, keys, mk)
    dec = mk()
    mgr = _manager(vi, dec)
    mgr.worker(chunks[0], 0, None, True)
    while mgr.frame_of_interest < len(chunks) - 1:
        want = _expected(log, mgr.frame_of_interest + 1)
        n0, at = len(dec.calls), mgr.next_frame_to_decode
        d = mgr.skip_stills(chunks, keys)
        assert d.index == want
        assert len(dec.calls) - n0 == want + 1 - at          # one decode per frame up to the change, none past it
        assert np.array_equal(mgr.buffers[d.buffer_index], pics[want]), f"landing {want}"


def test_an_idle_clip_lands_on_its_last_frame():
    frames, keys, pal = _idle_msv1(16)
    frames = [f for i, f in enumerate(frames) if i not in (4, 9, 12, 15)]
    keys = [k for i, k in enumerate(keys) if i not in (4, 9, 12, 15)]
    vi = _vi(CODEC_MSVC16, 16, len(frames), pal)
    dec = _Counting(OracleMSVideo1(16, W, H))
    mgr = _manager(vi, dec)
    mgr.worker(frames[0], 0, None, True)
    d = mgr.skip_stills(frames, keys)
    assert d.index == len(frames) - 1 and d.significant_changes is False
    assert dec.calls == ["I"] + ["P"] * (len(frames) - 1)
    assert mgr.log[-1].index == len(frames) - 1
