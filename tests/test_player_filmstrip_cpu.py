"""Manager.preview / Manager.filmstrip — the policy alone, over a fake decoder and a fake index (no GPU): which frames of the
attached index are asked for, that asking is a pure read of Manager and decoder, and what is refused."""
import copy

import numpy as np
import pytest

from jsplayer_amd import player
from jsplayer_amd.avi import CODEC_MSVC16, VideoInfo

N = 24
KEYS = [i % 8 == 0 for i in range(N)]
FRAMES = [bytes([1 if k else 0, i]) for i, k in enumerate(KEYS)]
TW, TH = 3, 2


class _Res:
    def __init__(self, data, sig):
        self.data_pnt, self.significant_changes = data, sig


class FakeDecoder:
    """Pictures are filled with the frame's number; every call is logged."""
    SEEKS = True

    def __init__(self):
        self.calls, self.prev = [], None

    def Preinit(self, lines):
        pass

    def PreviousFrame(self):
        return self.prev

    def IsKeyFrame(self, f):
        return f[0] == 1

    def _paint(self, src, dst):
        dst[:] = src[1]
        self.prev = dst

    def DecompressI(self, src, dst):
        self.calls.append(("I", src[1]))
        self._paint(src, dst)
        return 0

    def DecompressP(self, src, dst):
        self.calls.append(("P", src[1]))
        self._paint(src, dst)
        return _Res(dst, True)

    def Seek(self, srcs, dst, keys):
        self.calls.append(("Seek", srcs[0][1], srcs[-1][1]))
        self._paint(srcs[-1], dst)
        return _Res(dst, True)


class FakeIndex:
    """Thumbs logs its arguments and paints thumbnail k with its index frame number."""

    def __init__(self, dec, count):
        self.dec, self.frames = dec, count
        self.significance = [True] * count
        self.thumbs = []

    def Show(self, t, dst, adopt=True):
        self.dec.calls.append(("Show", t))
        dst[:] = t
        if adopt:
            self.dec.prev = dst
        return _Res(dst, True)

    def Thumbs(self, frames, scale=8, cols=1, out=None):
        frames = list(frames)
        assert out is None and all(0 <= t < self.frames for t in frames)
        self.thumbs.append((frames, scale, cols))
        n = len(frames)
        sheet = np.zeros((-(-n // cols) * TH, cols * TW), dtype=np.int32)
        for k, t in enumerate(frames):
            sheet[(k // cols) * TH:(k // cols + 1) * TH, (k % cols) * TW:(k % cols + 1) * TW] = t
        return sheet


def _manager(dec):
    vi = VideoInfo(X=4, Y=4, bpp=16, fps=15.0, nframes=N, codec=CODEC_MSVC16, palette=None, riff_size=0)
    return player.Manager(vi, dec, lambda n: np.full(n, -1, dtype=np.int32))


def _state(mgr, dec):
    return (copy.deepcopy(mgr.holds), mgr.frame_of_interest, mgr.next_frame_to_decode, list(mgr.log), dict(mgr.judged),
            list(dec.calls), dec.prev is None or int(dec.prev[0]), [b.copy() for b in mgr.buffers])


def _same(a, b):
    return a[:7] == b[:7] and all(np.array_equal(x, y) for x, y in zip(a[7], b[7]))


@pytest.mark.parametrize("first", [0, 5])
@pytest.mark.parametrize("n", [1, 3, 7, 16, 40])
def test_filmstrip_spreads_n_frames_evenly_over_the_index(first, n):
    count = 16
    dec = FakeDecoder()
    mgr = _manager(dec)
    idx = FakeIndex(dec, count)
    mgr.attach_index(idx, first)
    numbers, sheet = mgr.filmstrip(n, scale=4)
    picks = [(k * count) // n for k in range(n)]
    assert numbers == [first + t for t in picks]
    assert idx.thumbs == [(picks, 4, n)]                       # ONE Thumbs call; cols = None: one row
    assert sheet.shape == (TH, n * TW) and [int(sheet[0, k * TW]) for k in range(n)] == picks
    if n == 1:
        assert numbers == [first]
    if n == count:
        assert picks == list(range(count))                     # every frame once
    if n > count:
        assert sorted(set(picks)) == list(range(count)) and len(picks) > len(set(picks))   # repeats, nothing left out
    assert all(0 <= t < count for t in picks) and picks == sorted(picks)


def test_filmstrip_passes_scale_and_cols_on():
    dec = FakeDecoder()
    mgr = _manager(dec)
    idx = FakeIndex(dec, 10)
    mgr.attach_index(idx, 2)
    numbers, sheet = mgr.filmstrip(5, scale=16, cols=2)
    assert idx.thumbs == [([0, 2, 4, 6, 8], 16, 2)] and numbers == [2, 4, 6, 8, 10]
    assert sheet.shape == (3 * TH, 2 * TW)
    mgr.filmstrip(4)
    assert idx.thumbs[-1] == ([0, 2, 5, 7], 8, 4)              # the default scale


def test_preview_maps_the_clip_frame_to_the_index_frame():
    dec = FakeDecoder()
    mgr = _manager(dec)
    idx = FakeIndex(dec, 8)
    mgr.attach_index(idx, 8)
    t = mgr.preview(11)
    assert idx.thumbs == [([3], 8, 1)] and t.shape == (TH, TW) and int(t[0, 0]) == 3
    mgr.preview(8, scale=4)
    mgr.preview(15, scale=16)
    assert idx.thumbs[1:] == [([0], 4, 1), ([7], 16, 1)]


def test_preview_and_filmstrip_are_pure_reads():
    dec = FakeDecoder()
    mgr = _manager(dec)
    idx = FakeIndex(dec, N)
    mgr.attach_index(idx, 0)
    mgr.seek(FRAMES, 12, KEYS)
    mgr.prev_frame(FRAMES, KEYS)
    before = _state(mgr, dec)
    mgr.preview(3)
    mgr.preview(20, scale=4)
    mgr.filmstrip(9)
    mgr.filmstrip(30, scale=16, cols=4)
    assert _same(before, _state(mgr, dec))
    assert len(idx.thumbs) == 4
    assert not any(c[0] in ("I", "P", "Seek") for c in dec.calls) and [c for c in dec.calls if c[0] == "Show"] == [("Show", 12), ("Show", 11)]
    # ... and the navigation goes on as if nothing had been asked
    assert mgr.next_frame(FRAMES, KEYS).index == 12


def test_no_index_or_outside_it_is_a_value_error_and_decodes_nothing():
    dec = FakeDecoder()
    mgr = _manager(dec)
    with pytest.raises(ValueError):
        mgr.preview(0)
    with pytest.raises(ValueError):
        mgr.filmstrip(4)
    idx = FakeIndex(dec, 8)
    mgr.attach_index(idx, 8)
    for i in (7, 16, -1, N + 5):
        with pytest.raises(ValueError):
            mgr.preview(i)
    with pytest.raises(ValueError):
        mgr.filmstrip(0)
    mgr.attach_index(None)
    with pytest.raises(ValueError):
        mgr.preview(9)
    assert dec.calls == [] and idx.thumbs == [] and mgr.log == []
