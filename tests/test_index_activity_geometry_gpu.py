"""The lane-to-cell geometry of msv1_index_activity_kernel (jsp_index_activity / SeekIndex.Activity) on an MI355X: grids of more
than four columns, more than one workgroup, a tail group that leaves inside a workgroup that has work, pictures smaller than a
cell or without a block, an index of several chunks, `out` at an odd element.

Truth: THE DEFINITION (tests/index_activity_ref.py) over the oracle's sequential run, as in test_index_activity_gpu.Case — nothing of
it comes from the GPU; what the directed clips promise (tests/msv1_activity_geometry_clips.py) is asserted on that truth before any
GPU answer is looked at.  Every case compares the WHOLE array, exactly.  (out = base + 1 BYTE is refused:
test_index_activity_refusals_gpu.py.)"""
import ctypes as C

import numpy as np
import pytest

import index_activity_ref as ar
import msv1_activity_geometry_clips as gc
from jsplayer_amd import _native as N
from msv1_range_clips import long_clip, make_gpu, make_plan, palette
import test_index_activity_gpu as base
from test_index_activity_gpu import MSV1_N, Case

pytestmark = pytest.mark.gpu

SENTINEL = 0x7BCD
SEGMENTS = ("1", "3", "7", "auto")


def sweep_case(bits, w, h, start, chunk=None):
    frames, keys, marks = gc.sweep(bits, w, h)
    plan = make_plan(bits, w, h, frames, keys, 36)
    assert not plan["raises"]
    c = Case(bits, w, h, palette(bits), frames, keys, plan["coded"], 36, start, chunk=chunk)
    assert c.n == gc.FRAMES - start and c.idx.ActivitySize() == ar.grid(w, h)
    gc.check_properties(c.want, marks, w, h, start)
    return c, marks


def raw_call(c, first, n, ptr, elems):
    return N.lib().jsp_index_activity(c.gpu._h, c.idx._h, first, n, C.c_void_p(ptr), elems)


@pytest.mark.parametrize("bits", [16, 8])
@pytest.mark.parametrize("size", gc.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("start", [0, 3], ids=["nothing_before", "picture_before"])
def test_the_sweep_equals_the_definition(bits, size, start):
    """start = 3: the index starts at frame 3 of the sweep and frame 2's picture lies before it.  The third run is sweep frames
    29 .. 34 either way."""
    w, h = size
    c, marks = sweep_case(bits, w, h, start)
    n = c.n
    for segs in SEGMENTS:
        c.gpu.set_option("msv1_index_activity_segments", segs)
        for first, count in ((0, n), (1, 1), (29 - start, 6), (n - 1, 1)):
            c.check(first, count, f"segments={segs}")
        for f, r, q in marks:
            if f >= start:
                got = c.check(f - start, 1, f"segments={segs} mark ({r}, {q})")
                assert np.count_nonzero(got) == 1 and got[0, r, q] != 0
    c.close()


@pytest.mark.parametrize("bits", [16, 8])
def test_a_chunked_index_on_the_sweep(bits):
    """msv1_seek_chunk_frames = 7 (chunks of index frames 0 .. 6, 7 .. 13, ...): runs that cross chunk seams while the last writers
    of the picture before them lie chunks back."""
    c, _ = sweep_case(bits, 84, 72, 3, chunk=7)
    for first, count in ((0, c.n), (6, 2), (7, 1), (13, 9)):
        c.check(first, count, "chunk=7")
    c.close()


@pytest.mark.parametrize("bits", [16, 8])
def test_a_chunked_index_on_the_long_clip(bits):
    w, h = 52, 28
    frames, keys, pal, plan = long_clip(bits, w, h, seed=5, n=96)
    c = Case(bits, w, h, pal, frames, keys, plan["coded"], plan["lines"], 0, MSV1_N, chunk=7)
    c.check(0, MSV1_N, "chunk=7")
    c.close()


@pytest.mark.parametrize("size,cells", [((3, 8), (1, 1)), ((20, 3), (2, 1))], ids=["3x8", "20x3"])
def test_a_picture_without_a_block_has_a_map_of_zeros(size, cells):
    """No 4x4 block fits: the grid still has its cells, no lane of the launch has a block, and the map is the zeros the host wrote."""
    import torch
    w, h = size
    gpu = make_gpu(16, w, h, parse=base.PARSE)
    idx = gpu.BuildIndex([b"\x01\x02\x03\x04", b""], [True, False])
    assert idx.ActivitySize() == cells
    n, cell = 2, cells[0] * cells[1]
    raw = torch.full((n * cell + 64,), SENTINEL, dtype=torch.int16, device="cuda")
    assert N.lib().jsp_index_activity(gpu._h, idx._h, 0, n, C.c_void_p(raw.data_ptr()), n * cell) == 0, N.last_error()
    host = raw.cpu().numpy()
    assert not host[:n * cell].any() and np.all(host[n * cell:] == SENTINEL)
    assert not idx.Activity().cpu().numpy().any()
    idx.close()
    gpu.StopAndClean()


def test_out_at_an_odd_element():
    """`out` aligned to 2 bytes and not to 4 is legal: the kernel stores 16-bit words."""
    import torch
    w, h = 80, 80
    c, _ = sweep_case(16, w, h, 0)
    cols, rows = ar.grid(w, h)
    n, cell = c.n, rows * cols
    raw = torch.full((1 + n * cell + 64,), SENTINEL, dtype=torch.int16, device="cuda")
    ptr = raw.data_ptr() + 2
    assert ptr % 4 == 2
    assert raw_call(c, 0, n, ptr, n * cell) == 0, N.last_error()
    host = raw.cpu().numpy()
    assert np.array_equal(host[1:1 + n * cell].view(np.uint16).reshape(n, rows, cols), c.want)
    assert host[0] == SENTINEL and np.all(host[1 + n * cell:] == SENTINEL)
    c.close()


def test_the_codec_goes_on_as_a_twin_that_never_asked():
    """At 272x20, three workgroups: after the calls a DecompressP of the next frame gives what it gives a codec that never saw them
    (as test_index_activity_gpu.test_nothing_else_is_written_and_the_codec_is_only_lent)."""
    w, h, bits, start = 272, 20, 16, 3
    a, marks = sweep_case(bits, w, h, start)
    twin, _ = sweep_case(bits, w, h, start)
    prev = a.gpu.PreviousFrame()
    prev_pic = prev.cpu().numpy().copy()
    rows_before = a.gpu.counter("msv1_block_changes")
    a.check(0, a.n)
    for f, r, q in marks:
        if f >= start:
            a.check(f - start, 1)
    assert a.gpu.PreviousFrame() is prev and np.array_equal(prev.cpu().numpy(), prev_pic)
    assert a.gpu.counter("msv1_block_changes") == rows_before
    res = []
    for c in (a, twin):   # both stand at frame start - 1 and go on from there alike
        p = c.gpu.PreviousFrame()
        dst = next(b for b in c.pool if b is not p)
        dst.copy_(p)
        r = c.gpu.DecompressP(a.frames[start], dst)
        res.append(((r.data_pnt is dst, r.significant_changes), c.gpu.PreviousFrame().cpu().numpy().copy(), c.gpu.counter("msv1_block_changes")))
    assert res[0][0] == res[1][0] and np.array_equal(res[0][1], res[1][1]) and res[0][2] == res[1][2]
    assert np.array_equal(res[0][1], a.p[0]), "the picture of index frame 0"
    a.check(0, 5)
    a.close()
    twin.close()


class TestOnGpuParse:
    """Every test of this file once more with the block tables of the on-GPU parse, the codec's default (base.Case reads base.PARSE).
    The tests above keep the host parser and their names."""

    @pytest.fixture(autouse=True)
    def parse_mode(self):
        base.PARSE = "gpu"
        yield base.PARSE
        base.PARSE = "host"


for _name, _test in list(globals().items()):
    if _name.startswith("test_"):
        setattr(TestOnGpuParse, _name, staticmethod(_test))
