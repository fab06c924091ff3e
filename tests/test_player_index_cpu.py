"""Manager with a seek index attached (attach_index; Show = one launch on the GPU) and the navigation of Manager.hx:184-208 —
the policy alone, over a fake decoder and a fake index (no GPU): a held frame is shown as it is, a frame inside the index goes
to Show, one outside it to Seek / worker as before, and next / prev frame / key stop at the clip's ends."""
import numpy as np
import pytest

from jsplayer_amd import player
from jsplayer_amd.avi import CODEC_MSVC16, VideoInfo

N = 24
KEYS = [i % 8 == 0 for i in range(N)]                   # key frames 0, 8, 16
FRAMES = [bytes([1 if k else 0, i]) for i, k in enumerate(KEYS)]


class _Res:
    def __init__(self, data, sig):
        self.data_pnt, self.significant_changes = data, sig


class FakeDecoder:
    """Pictures are filled with the frame's number; every call is logged."""
    SEEKS = True
    FINDS_CHANGES = True

    def __init__(self, seeks=True):
        self.calls, self.prev = [], None
        if not seeks:
            self.SEEKS = False

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

    def FindChange(self, *a, **k):
        self.calls.append(("FindChange",))
        raise AssertionError("FindChange with every frame known")


class FakeIndex:
    def __init__(self, dec, first, count, significance=None):
        self.dec, self.first, self.frames = dec, first, count
        self.significance = significance if significance is not None else [True] * count

    def Show(self, t, dst, adopt=True):
        self.dec.calls.append(("Show", self.first + t))
        dst[:] = self.first + t
        if adopt:
            self.dec.prev = dst
        return _Res(dst, self.significance[t])


def _manager(dec):
    vi = VideoInfo(X=4, Y=4, bpp=16, fps=15.0, nframes=N, codec=CODEC_MSVC16, palette=None, riff_size=0)
    return player.Manager(vi, dec, lambda n: np.full(n, -1, dtype=np.int32))


def _shown(mgr, d):
    return int(mgr.buffers[d.buffer_index][0])


def test_held_frame_is_shown_without_show():
    dec = FakeDecoder()
    mgr = _manager(dec)
    mgr.attach_index(FakeIndex(dec, 0, N), 0)
    d = mgr.seek(FRAMES, 5, KEYS)
    assert _shown(mgr, d) == 5 and dec.calls == [("Show", 5)]
    d = mgr.seek(FRAMES, 5, KEYS)
    assert _shown(mgr, d) == 5 and dec.calls == [("Show", 5)]


@pytest.mark.parametrize("seeks", [True, False])
def test_show_inside_the_index_seek_or_worker_outside(seeks):
    dec = FakeDecoder(seeks)
    mgr = _manager(dec)
    mgr.attach_index(FakeIndex(dec, 8, 8), 8)
    d = mgr.seek(FRAMES, 10, KEYS)
    assert _shown(mgr, d) == 10 and dec.calls == [("Show", 10)]
    dec.calls.clear()
    d = mgr.seek(FRAMES, 20, KEYS)
    assert _shown(mgr, d) == 20
    if seeks:
        assert dec.calls == [("Seek", 16, 20)]
    else:
        assert dec.calls == [("I", 16), ("P", 17), ("P", 18), ("P", 19), ("P", 20)]
    dec.calls.clear()
    d = mgr.seek(FRAMES, 15, KEYS)          # back inside: Show again, whatever was decoded last
    assert _shown(mgr, d) == 15 and dec.calls == [("Show", 15)]
    # play continues after the frame shown
    assert mgr.next_frame_to_decode == 16


def test_step_back_through_the_index_is_one_show_per_frame():
    dec = FakeDecoder()
    mgr = _manager(dec)
    mgr.attach_index(FakeIndex(dec, 0, N), 0)
    mgr.seek(FRAMES, N - 1, KEYS)
    seen = [N - 1]
    for _ in range(N + 1):                  # two steps past frame 0: it stays
        seen.append(_shown(mgr, mgr.prev_frame(FRAMES, KEYS)))
    assert seen == list(range(N - 1, -1, -1)) + [0, 0]
    assert all(c[0] == "Show" for c in dec.calls)


def test_navigation_arithmetic_at_the_ends():
    dec = FakeDecoder()
    mgr = _manager(dec)
    assert _shown(mgr, mgr.seek(FRAMES, 0, KEYS)) == 0
    assert mgr.prev_frame(FRAMES, KEYS).index == 0
    assert mgr.prev_key(FRAMES, KEYS).index == 0
    assert mgr.next_key(FRAMES, KEYS).index == 8
    assert mgr.next_key(FRAMES, KEYS).index == 16
    assert mgr.next_key(FRAMES, KEYS).index == N - 1     # no key frame after 16: the last frame
    assert mgr.next_key(FRAMES, KEYS).index == N - 1
    assert mgr.next_frame(FRAMES, KEYS).index == N - 1
    assert mgr.prev_key(FRAMES, KEYS).index == 16
    assert mgr.prev_key(FRAMES, KEYS).index == 8         # from 16: the nearest key frame before 15
    assert mgr.next_frame(FRAMES, KEYS).index == 9
    assert mgr.prev_key(FRAMES, KEYS).index == 8
    assert mgr.prev_frame(FRAMES, KEYS).index == 7


def test_skip_stills_inside_the_index_decodes_nothing():
    dec = FakeDecoder()
    mgr = _manager(dec)
    sig = [True] + [False] * 9 + [True] + [False] * (N - 11)
    mgr.attach_index(FakeIndex(dec, 0, N, sig), 0)
    mgr.seek(FRAMES, 0, KEYS)
    d = mgr.skip_stills(FRAMES, KEYS)
    assert d.index == 10 and _shown(mgr, d) == 10
    d = mgr.skip_stills(FRAMES, KEYS)
    assert d.index == N - 1                               # nothing changes after 10: the last frame
    assert [c[0] for c in dec.calls] == ["Show", "Show", "Show"]


def test_without_an_index_nothing_changes():
    """The same navigation with no index and with an index attached and detached again: the same decoder calls, the same log."""
    runs = []
    for attach in (False, True):
        dec = FakeDecoder()
        mgr = _manager(dec)
        if attach:
            mgr.attach_index(FakeIndex(dec, 0, N), 0)
            mgr.attach_index(None)
        mgr.seek(FRAMES, 12, KEYS)
        mgr.prev_frame(FRAMES, KEYS)
        mgr.next_key(FRAMES, KEYS)
        mgr.seek(FRAMES, 3, KEYS)
        mgr.play(FRAMES[:2], key_flags=KEYS[:2])
        runs.append((dec.calls, [(d.index, d.key, d.buffer_index, d.significant_changes) for d in mgr.log]))
    assert runs[0] == runs[1]
    assert runs[0][0][:3] == [("Seek", 8, 12), ("Seek", 8, 11), ("Seek", 16, 16)]
    assert not any(c[0] == "Show" for c in runs[0][0])
