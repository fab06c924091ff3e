"""The three kernels of the ScreenPressor seek index (jsp_sp_index_show / _play / _thumbs) on the directed clips of
tests/sp_directed_clips.py, on an MI355X: walks of up to 139 records, blocks written in all 32 frames of a bitmap word, key frames
at bit 31 and bit 0 of a word, an empty middle word, 1-pixel and edge rectangles, the scalar path on a picture 83 wide, saturated
channel sums (tests/test_sp_directed_clips_cpu.py asserts that the clips hold all of that).

Truth: the painted pictures, which are also the oracle's sequential run.  Everything is bit-exact.  Every pixel of these clips names
the frame that wrote it last, so a failure says which record the walk took in place of which (describe_mismatch).  Every
destination is filled with a poison word before each call, and one more poisoned buffer that is never listed must stay poisoned."""
import numpy as np
import pytest

import sp_directed_clips as dc
import thumbs_ref as tr
from test_sp_index_gpu import POISON, dev_buf, make_sp, picture

pytestmark = pytest.mark.gpu

NAMES = ("A", "B", "C")


class Indexed:
    """A directed clip, the oracle's run over it, a codec and ONE index of the clip."""

    def __init__(self, name):
        self.clip = dc.clip(name)
        self.pictures, self.verdicts = dc.oracle(name)
        self.n, self.size = len(self.clip.keys), self.clip.w * self.clip.h
        for t in range(self.n):
            assert np.array_equal(self.pictures[t], self.clip.frames[t]), f"{self.clip.name} frame {t}: the oracle's picture is not the painted one"
        self.gpu = make_sp(self.clip, lines=dc.KEY_ROW)
        self.idx = self.gpu.BuildScrubIndex(self.clip.chunks, self.clip.keys, key_row=dc.KEY_ROW)
        assert self.idx.frames == self.n and self.idx.significance == self.verdicts
        self.extra = dev_buf(self.size)                  # never listed: must stay poisoned

    def exact(self, got, t, what):
        c = self.clip
        assert np.array_equal(got, c.frames[t]), f"{c.name} {what} frame {t}: " + dc.describe_mismatch(got, c.frames[t], c.w, c.h, c.bpp)

    def untouched(self, what):
        assert bool((self.extra == POISON).all()), f"{self.clip.name} {what}: a buffer that was not listed was written"

    def close(self):
        assert self.gpu.PreviousFrame() is None
        self.idx.close()
        self.gpu.StopAndClean()


@pytest.mark.parametrize("name", NAMES)
def test_show_every_frame_aligned_and_misaligned(name):
    """The misaligned destination takes A's and C's deep walks through the scalar instantiation (B is scalar either way)."""
    x = Indexed(name)
    dsts = {"aligned": dev_buf(x.size), "misaligned": dev_buf(x.size, misalign=True)}
    assert dsts["aligned"].data_ptr() % 16 == 0 and dsts["misaligned"].data_ptr() % 16 != 0
    for t in list(range(x.n - 1, -1, -1)) + [95, 31, 32, 139, 0]:
        for how, dst in dsts.items():
            dst.fill_(POISON)
            r = x.idx.Show(t, dst)
            assert r.data_pnt is dst
            x.exact(picture(dst), t, f"Show into the {how} buffer,")
            assert r.significant_changes == x.verdicts[t], f"{x.clip.name} t={t}: verdict"
    x.untouched("Show")
    x.close()


class Played:
    """What Show writes for every frame, and a pool of destinations; `check` plays a run and compares every picture and verdict."""

    def __init__(self, x):
        self.x = x
        self.bufs = [dev_buf(x.size) for _ in range(x.n)]
        self.shown = []
        for t in range(x.n):
            self.bufs[0].fill_(POISON)
            x.idx.Show(t, self.bufs[0])
            self.shown.append(picture(self.bufs[0]).copy())
            x.exact(self.shown[t], t, "Show,")

    def check(self, first, count, stride=1, reverse=False):
        x = self.x
        what = f"Play({first}, {count}, stride {stride}{', buffers reversed' if reverse else ''}),"
        dsts = self.bufs[:count][::-1] if reverse else self.bufs[:count]
        for b in dsts:
            b.fill_(POISON)
        res = x.idx.Play(first, dsts, stride)
        assert len(res) == count, what
        for k, (r, dst) in enumerate(zip(res, dsts)):
            t = first + k * stride
            got = picture(dst)
            assert r.data_pnt is dst, what
            x.exact(got, t, what)
            assert np.array_equal(got, self.shown[t]), f"{x.clip.name} {what} frame {t}: not what Show writes"
            assert r.significant_changes == x.verdicts[t], f"{x.clip.name} {what} frame {t}: verdict"
        x.untouched(what)


@pytest.mark.parametrize("name", NAMES)
def test_play_every_run(name):
    x = Indexed(name)
    p = Played(x)
    for first, count, stride in dc.play_runs(x.n):
        p.check(first, count, stride)
    p.check(0, x.n, reverse=True)
    p.check(31, (x.n - 32) // 2 + 1, 2, reverse=True)
    # one destination 4 bytes off 16-byte alignment among aligned ones: the whole call takes the scalar instantiation
    for odd, run in ((0, (95, 20, 1)), (7, (30, 40, 1)), (2, (62, 3, 32))):
        keep, p.bufs[odd] = p.bufs[odd], dev_buf(x.size, misalign=True)
        assert p.bufs[odd].data_ptr() % 16 != 0 and all(b.data_ptr() % 16 == 0 for k, b in enumerate(p.bufs) if k != odd)
        p.check(*run)
        p.bufs[odd] = keep
    x.close()


def check_sheet(x, picks, s, cols, what):
    """One Thumbs call into a poisoned `out` one cell longer than the sheet: every thumbnail is the reference's of the painted
    picture, the cells of the last row past the last thumbnail and the ints behind the sheet keep the poison."""
    c = x.clip
    tw, th = x.idx.ThumbSize(s)
    assert (tw, th) == tr.thumb_size(c.w, c.h, s) == (c.w // s, c.h // s), what
    rows = -(-len(picks) // cols)
    out = dev_buf(rows * th * cols * tw + tw * th)
    got = x.idx.Thumbs(picks, scale=s, cols=cols, out=out)
    assert tuple(got.shape) == (rows * th, cols * tw) and got.data_ptr() == out.data_ptr(), what
    got = got.cpu().numpy()
    want = tr.sheet([tr.thumbnail(c.frames[t], c.w, c.h, s) for t in picks], cols, fill=POISON)
    for y, px in np.argwhere(got != want)[:1]:
        cell = (y // th) * cols + px // tw
        where = f"thumbnail {cell} (frame {picks[cell]})" if cell < len(picks) else f"the empty cell {cell}"
        pytest.fail(f"{c.name} {what}: {int((got != want).sum())} sheet pixels differ, first in {where} at row {y % th}, col {px % tw}: "
                    f"want 0x{int(want[y, px]) & 0xFFFFFFFF:08x}, got 0x{int(got[y, px]) & 0xFFFFFFFF:08x}")
    assert np.all(picture(out)[rows * th * cols * tw:] == POISON), what + ": written behind the sheet"
    x.untouched(what)
    return got


@pytest.mark.parametrize("name", NAMES)
def test_thumbs_every_frame_every_scale(name):
    x = Indexed(name)
    rng = np.random.default_rng(140)
    shuffled = [int(t) for t in rng.permutation(x.n)] + [int(t) for t in rng.integers(0, x.n, 9)]
    for s in tr.SCALES:
        check_sheet(x, list(range(x.n)), s, 9, f"Thumbs of every frame, scale {s}, 9 to a row")     # 140 = 15 * 9 + 5: four empty cells
        check_sheet(x, shuffled, s, 13, f"Thumbs of a shuffled list with repeats, scale {s}")         # 149 = 11 * 13 + 6
    x.close()


def test_thumbs_saturated_channels_do_not_carry():
    """Clip S: whole blocks of 0x00FFFFFF, 0x00FF00FF, 0x0000FF00 and 0 side by side.  A cell never straddles two blocks, so every
    result word is one of those four, whatever the scale: a channel sum of 16 * 16 * 255 stays in its field."""
    x = Indexed("S")
    pure = {dc.WHITE, dc.MAGENTA, dc.GREEN, dc.BLACK}
    for s in tr.SCALES:
        tw, th = x.idx.ThumbSize(s)
        got = check_sheet(x, [0, 1, 2, 3], s, 4, f"Thumbs, scale {s}").view(np.uint32)
        assert set(int(v) for v in np.unique(got)) <= pure, f"scale {s}: a channel sum leaked into another"
        assert np.all(got[:, :tw] == dc.WHITE)
        for k in (1, 2, 3):
            cell = got[:, k * tw:(k + 1) * tw]
            for shift in (0, 8, 16):
                ch = (cell >> shift) & 0xFF
                beside = ((ch[:, :-1] == 255) & (ch[:, 1:] == 0)) | ((ch[:, :-1] == 0) & (ch[:, 1:] == 255))
                assert beside.any(), f"scale {s} frame {k}: no byte of 255 beside a byte of 0 in the channel at bit {shift}"
    dst = dev_buf(x.size)
    for t in range(4):
        dst.fill_(POISON)
        x.idx.Show(t, dst)
        assert np.array_equal(picture(dst), x.clip.frames[t]), f"S frame {t}"
    x.close()
