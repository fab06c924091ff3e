"""sp_index_activity_kernel (jsp_sp_index_activity / SpScrubIndex.Activity) on an MI355X, on the directed clips of
tests/sp_activity_clips.py: values that repeat — so that a comparison with a stale register, or a rectangle's area taken for a
count, gives another number —, pictures of 17 x 17, 66 x 20, 79 x 33, 72 x 16 and 13 x 9, and every run of sp_activity_clips.runs
through the C ABI into the middle of a poisoned buffer: a store for frame first - 1 or first + n, or for a block past the grid, lands
in the poison.

Truth: THE DEFINITION (tests/index_activity_ref.py) over the oracle's sequential run — nothing of it comes from the GPU; what the
clips promise is asserted on that truth by test_sp_activity_clips_cpu.py.  Every run compares the WHOLE buffer, exactly."""
import ctypes as C

import numpy as np
import pytest

import index_activity_ref as ar
import sp_activity_clips as ac
from jsplayer_amd import _native as N
from test_sp_index_gpu import make_sp

pytestmark = pytest.mark.gpu

POISON = 0x7BCD


def describe(host, want_buf, at, cell, first, n, nbx):
    """The first wrong element of the buffer, in the map's terms."""
    e = int(np.nonzero(host != want_buf)[0][0])
    k, b = divmod(e - at, cell)
    where = "in the poison in front of the map" if e < at else "in the poison behind the map" if e >= at + n * cell else "in the map"
    return "%s: frame %d (row %d of %d), block %d (bx %d, by %d): got %d, want %d (%d elements differ)" % (
        where, first + k, k, n, b, b % nbx, b // nbx, int(host[e]) & 0xFFFF, int(want_buf[e]) & 0xFFFF, int((host != want_buf).sum()))


@pytest.mark.parametrize("name", ac.NAMES)
def test_every_run_into_a_poisoned_buffer(name):
    import torch
    c = ac.clip(name)
    want = ac.truth(name)                     # (N, rows, cols), from the oracle's pictures
    pictures, verdicts = ac.oracle(name)
    cols, rows = ar.grid(c.w, c.h)
    cell = rows * cols
    gpu = make_sp(c, lines=ac.KEY_ROW)
    idx = gpu.BuildScrubIndex(c.chunks, c.keys, key_row=ac.KEY_ROW)
    assert idx.frames == ac.N and idx.significance == verdicts
    assert idx.ActivitySize() == (cols, rows)
    lib = N.lib()
    front = (cell + 1) & ~1                   # poisoned elements in front: at least a row of the map, an even number of them
    raw = torch.empty((front + 1 + ac.N * cell + front,), dtype=torch.int16, device="cuda")
    assert raw.data_ptr() % 4 == 0
    for i, (first, n) in enumerate(ac.runs(c)):
        at = front + (i & 1)                  # every other run: `out` two bytes off a 4-byte boundary
        raw.fill_(POISON)
        ptr = raw.data_ptr() + 2 * at
        assert ptr % 4 == 2 * (i & 1) and at >= cell and raw.numel() - at - n * cell >= cell
        assert lib.jsp_sp_index_activity(gpu._h, idx._h, first, n, C.c_void_p(ptr), n * cell) == 0, N.last_error()
        host = raw.cpu().numpy()
        want_buf = np.full(host.shape, POISON, dtype=np.int16)
        want_buf[at:at + n * cell] = want[first:first + n].reshape(-1).view(np.int16)
        assert np.array_equal(host, want_buf), f"{c.name} run ({first}, {n}) " + describe(host, want_buf, at, cell, first, n, cols)
    got = idx.Activity(0, ac.N)
    assert tuple(got.shape) == (ac.N, rows, cols) and str(got.dtype) == "torch.int16"
    assert np.array_equal(got.cpu().numpy().view(np.uint16), want), f"{c.name} Activity(0, {ac.N})"
    out = torch.full((ac.N, rows, cols), POISON, dtype=torch.int16, device="cuda")
    assert idx.Activity(0, ac.N, out=out) is out and np.array_equal(out.cpu().numpy().view(np.uint16), want), f"{c.name} Activity(out=)"
    assert gpu.PreviousFrame() is None
    idx.close()
    gpu.StopAndClean()
