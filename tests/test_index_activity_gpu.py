"""The activity map of an MSVideo1 seek index (jsp_index_activity / SeekIndex.Activity) on an MI355X.

Truth: THE DEFINITION (tests/index_activity_ref.py: changed pixels per 16 x 16 cell between whole pictures) over the oracle's
sequential run (msv1_range_clips.truth_run) — nothing of it comes from the GPU.  Every case compares the WHOLE array, exactly."""
import ctypes as C

import numpy as np
import pytest

import index_activity_ref as ar
import msv1_index_play_ref as pr
from jsplayer_amd import CodecError
from jsplayer_amd import _native as N
from msv1_range_clips import POISON, Idle, dev_buf, long_clip, make_gpu, make_plan, palette, truth_run

pytestmark = pytest.mark.gpu

MSV1_N = 72   # words 0, 1, 2 of the bitmap: a run crosses two word boundaries; the key frame at 70 repaints the picture as it is
PARSE = "host"   # the msv1_parse of every codec built here; TestOnGpuParse (the end of this file) runs every test with "gpu" too


def sequential(gpu, frames, keys, hi, pool):
    for i in range(hi):
        prev = gpu.PreviousFrame()
        dst = next(b for b in pool if b is not prev)
        if keys[i]:
            assert gpu.DecompressI(frames[i], dst) == 0
        else:
            gpu.DecompressP(frames[i], dst)


class Case:
    """A codec brought to frame `start` of a clip frame by frame, its index over the `count` frames from there on, and the map of
    the whole index by the definition."""

    def __init__(self, bits, w, h, pal, frames, keys, coded, lines=36, start=0, count=None, chunk=None):
        count = len(frames) - start if count is None else count
        self.bits, self.w, self.h, self.n = bits, w, h, count
        self.frames, self.keys = frames, keys
        truth = truth_run(bits, w, h, pal, frames[:start + count], keys[:start + count], lines, key_row=lines)
        assert all(t is not None for t in truth)
        pics = [t[0] for t in truth]
        self.p_before, self.p = ar.msv1_pictures(pics[start:], coded[start:start + count], w, h, pics[start - 1] if start > 0 else None)
        self.want = ar.activity(self.p, self.p_before, w, h)
        self.gpu = make_gpu(bits, w, h, pal, lines, chunk, PARSE)   # (chunk: the msv1_seek_chunk_frames option — an index of several chunks)
        self.pool = [dev_buf(w * h) for _ in range(3)]
        sequential(self.gpu, frames, keys, start, self.pool)
        self.idx = self.gpu.BuildIndex(frames[start:start + count], keys[start:start + count])
        assert self.idx.frames == count
        self.where = f"{bits}-bit {w}x{h} start={start} ({PARSE} parse)"

    def check(self, first, n, what=""):
        got = self.idx.Activity(first, n)
        cols, rows = ar.grid(self.w, self.h)
        assert tuple(got.shape) == (n, rows, cols) and str(got.dtype) == "torch.int16"
        got = got.cpu().numpy().view(np.uint16)
        assert np.array_equal(got, self.want[first:first + n]), f"{self.where} first={first} n={n} {what}"
        return got

    def close(self):
        self.idx.close()
        self.gpu.StopAndClean()


@pytest.mark.parametrize("bits", [16, 8])
@pytest.mark.parametrize("size", [(64, 32), (52, 28), (54, 30)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("start", [0, 3], ids=["nothing_before", "picture_before"])
def test_every_run_equals_the_definition(bits, size, start):
    w, h = size
    frames, keys, pal, plan = long_clip(bits, w, h, seed=5, n=96)
    assert not plan["raises"]
    c = Case(bits, w, h, pal, frames, keys, plan["coded"], plan["lines"], start, MSV1_N)
    assert c.idx.ActivitySize() == ar.grid(w, h)
    n = c.n
    for first, count in ((0, n), (1, 1), (31, 3), (32, 33), (n - 1, 1)):
        c.check(first, count)
    assert c.want.any() and c.want.max() <= 256
    c.close()


@pytest.mark.parametrize("bits", [16, 8])
def test_segments_do_not_change_the_map(bits):
    w, h = 52, 28
    frames, keys, pal, plan = long_clip(bits, w, h, seed=5, n=96)
    c = Case(bits, w, h, pal, frames, keys, plan["coded"], plan["lines"], 3, MSV1_N)
    for segs in ("1", "2", "7", "auto"):
        c.gpu.set_option("msv1_index_activity_segments", segs)
        for first, count in ((0, c.n), (31, 3), (32, 33), (5, 1)):
            c.check(first, count, f"segments={segs}")
    for bad in ("0", "65", "-1", "many", ""):
        with pytest.raises(CodecError):
            c.gpu.set_option("msv1_index_activity_segments", bad)
    c.close()


@pytest.mark.parametrize("bits", [16, 8])
def test_recoded_blocks_change_nothing_and_one_block_is_one_element(bits):
    """Idle.recode codes blocks again with the pixels they had: the bitmap bits are set, the map is zero.  Then one block of the
    corner cell changes: exactly one non-zero element, the differing pixels of that block."""
    w, h = 64, 32
    g = Idle(bits, w, h, seed=3)
    frames = [g.key()] + [g.recode(list(range(k, g.nb, 3))) for k in range(3)] + [g.change([g.nb - 1])]
    keys = [True] + [False] * 4
    plan = make_plan(bits, w, h, frames, keys, 36)
    assert plan["coded"][1:4].any(axis=1).all()
    c = Case(bits, w, h, palette(bits), frames, keys, plan["coded"])
    got = c.check(0, 5)
    assert not got[1:4].any()
    cols, rows = ar.grid(w, h)
    changed = int(np.count_nonzero(c.p[4] != c.p[3]))
    assert 0 < changed <= 16 and np.count_nonzero(got[4]) == 1 and got[4, rows - 1, cols - 1] == changed
    c.close()


def test_a_first_writer_is_compared_with_zeros():
    """cut_short_clip at 8 bits: the key frame's end marker leaves blocks with no writer, and nothing lies before the range."""
    w, h = 64, 32
    frames, keys, pal, at = pr.cut_short_clip(8, w, h)
    plan = make_plan(8, w, h, frames, keys, 36)
    assert not plan["coded"][0, at:].any()
    c = Case(8, w, h, pal, frames, keys, plan["coded"])
    got = c.check(0, c.n)
    for first in (1, 2, 3, 9):
        c.check(first, c.n - first)
    assert got[2].any()
    c.close()


def test_nothing_else_is_written_and_the_codec_is_only_lent():
    """A sentinel behind n * rows * cols and an unrelated frame buffer stay intact; `out=` is taken; a DecompressP of the next frame
    after an Activity call returns what it returns without the call."""
    import torch
    w, h, bits = 52, 28, 16
    frames, keys, pal, plan = long_clip(bits, w, h, seed=5, n=96)
    start, count = 3, 40
    a = Case(bits, w, h, pal, frames, keys, plan["coded"], plan["lines"], start, count)
    twin = Case(bits, w, h, pal, frames, keys, plan["coded"], plan["lines"], start, count)
    cols, rows = ar.grid(w, h)
    cell = rows * cols
    first, n = 2, 35
    raw = torch.full((n * cell + 64,), 0x7BCD, dtype=torch.int16, device="cuda")
    bystander = dev_buf(w * h)
    prev = a.gpu.PreviousFrame()
    prev_pic = prev.cpu().numpy().copy()
    rows_before = a.gpu.counter("msv1_block_changes")
    lib = N.lib()
    assert lib.jsp_index_activity(a.gpu._h, a.idx._h, first, n, C.c_void_p(raw.data_ptr()), n * cell) == 0, N.last_error()
    host = raw.cpu().numpy()
    assert np.array_equal(host[:n * cell].view(np.uint16).reshape(n, rows, cols), a.want[first:first + n])
    assert np.all(host[n * cell:] == 0x7BCD), "written behind n * rows * cols"
    assert np.all(bystander.cpu().numpy().view(np.uint32) == POISON)
    out = torch.full((n, rows, cols), 0x7BCD, dtype=torch.int16, device="cuda")
    assert a.idx.Activity(first, n, out=out) is out and np.array_equal(out.cpu().numpy().view(np.uint16), a.want[first:first + n])
    with pytest.raises(CodecError):
        a.idx.Activity(first, n, out=out[:, :, :1])
    assert a.gpu.PreviousFrame() is prev and np.array_equal(prev.cpu().numpy(), prev_pic)
    assert a.gpu.counter("msv1_block_changes") == rows_before
    for i in range(start, start + 3):   # the codec still stands at frame start - 1: both go on from there alike
        res = []
        for c in (a, twin):
            p = c.gpu.PreviousFrame()
            dst = next(b for b in c.pool if b is not p)
            dst.copy_(p)
            r = c.gpu.DecompressI(frames[i], dst) if keys[i] else c.gpu.DecompressP(frames[i], dst)
            res.append((r if keys[i] else (r.data_pnt is dst, r.significant_changes), c.gpu.PreviousFrame().cpu().numpy().copy(),
                        c.gpu.counter("msv1_block_changes")))
        assert res[0][0] == res[1][0] and np.array_equal(res[0][1], res[1][1]) and res[0][2] == res[1][2], f"frame {i} after Activity"
        a.check(0, 5)
    a.close()
    twin.close()


class TestOnGpuParse:
    """Every test of this file once more with the block tables of the on-GPU parse, the codec's default (Case reads PARSE).  The
    tests above keep the host parser and their names."""

    @pytest.fixture(autouse=True)
    def parse_mode(self):
        global PARSE
        PARSE = "gpu"
        yield PARSE
        PARSE = "host"


for _name, _test in list(globals().items()):
    if _name.startswith("test_"):
        setattr(TestOnGpuParse, _name, staticmethod(_test))
