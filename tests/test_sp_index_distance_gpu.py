"""The distance map of a ScreenPressor seek index (jsp_sp_index_distance / SpScrubIndex.Distance) on an MI355X, on the directed clips
of tests/sp_activity_clips.py (values that repeat, pictures of 17 x 17, 66 x 20, 79 x 33, 72 x 16 and 13 x 9, key frames at bit 0 and
bit 31 of a bitmap word) and two generated clips whose blocks rest, so that a value is stored again for frames without an event.

Truth: THE DEFINITION (tests/index_distance_ref.py) over the oracle's sequential run (tests/index_distance_cases.py, which
test_index_distance_ref_cpu.py holds against a brute-force compare first) — nothing of it comes from the GPU.  Every run goes through
the C ABI into the middle of a poisoned buffer and the WHOLE buffer is compared, exactly: a store for a frame or a block outside the
map lands in the poison, and an element the launch leaves out keeps it."""
import ctypes as C

import numpy as np
import pytest

import index_activity_ref as ar
import index_distance_cases as cs
import sp_activity_clips as ac
from jsplayer_amd import CodecError
from jsplayer_amd import _native as N
from test_sp_index_gpu import dev_buf, make_sp

pytestmark = pytest.mark.gpu

POISON = 0x7BCD
REF_PICTURE = -2


def to_device(words, misalign=False):
    import torch
    buf = dev_buf(len(words), misalign=misalign)
    buf.copy_(torch.from_numpy(np.array(words).view(np.int32)))
    assert buf.data_ptr() % 16 == (4 if misalign else 0)
    return buf


@pytest.mark.parametrize("name", cs.SP_NAMES)
def test_every_run_and_reference_into_a_poisoned_buffer(name):
    import torch
    case = cs.sp_case(name)
    c = case.clip
    cols, rows = ar.grid(c.w, c.h)
    cell = rows * cols
    gpu = make_sp(c, lines=case.key_row)
    idx = gpu.BuildScrubIndex(c.chunks, c.keys, key_row=case.key_row)
    assert idx.frames == case.n and idx.ActivitySize() == (cols, rows)
    lib = N.lib()
    front = (cell + 1) & ~1                   # poisoned elements in front: at least a row of the map, an even number of them
    raw = torch.empty((front + 1 + case.n * cell + front,), dtype=torch.int16, device="cuda")
    assert raw.data_ptr() % 4 == 0
    picture = cs.sp_picture_for(name)
    refs = [(r, None, r, f"frame {r}") for r in cs.sp_ref_frames(name)]
    bufs = [to_device(picture, misalign) for misalign in (False, True)]
    refs += [(REF_PICTURE, C.c_void_p(b.data_ptr()), "picture", f"picture at {b.data_ptr() % 16} mod 16") for b in bufs]
    i = 0
    for ref_frame, ref_ptr, key, what in refs:
        want = cs.sp_truth(name, key)
        for first, n in cs.sp_runs(name):
            at = front + (i & 1)              # every other call: `out` two bytes off a 4-byte boundary
            i += 1
            raw.fill_(POISON)
            ptr = raw.data_ptr() + 2 * at
            assert lib.jsp_sp_index_distance(gpu._h, idx._h, ref_frame, ref_ptr, first, n, C.c_void_p(ptr), n * cell) == 0, N.last_error()
            host = raw.cpu().numpy()
            want_buf = np.full(host.shape, POISON, dtype=np.int16)
            want_buf[at:at + n * cell] = want[first:first + n].reshape(-1).view(np.int16)
            if not np.array_equal(host, want_buf):
                e = int(np.nonzero(host != want_buf)[0][0])
                k, b = divmod(e - at, cell)
                raise AssertionError("%s ref %s run (%d, %d): element %d (frame %d, block %d): got %d, want %d (%d elements differ)" % (
                    c.name, what, first, n, e - at, first + k, b, int(host[e]) & 0xFFFF, int(want_buf[e]) & 0xFFFF, int((host != want_buf).sum())))
    for b in bufs:
        assert np.array_equal(b.cpu().numpy().view(np.uint32), picture), "the reference picture is only read"
    # Python: frame numbers and tensors, out=
    for key in (cs.sp_ref_frames(name)[1], "picture"):
        want = cs.sp_truth(name, key)
        got = idx.Distance(bufs[0] if key == "picture" else key)
        assert tuple(got.shape) == (case.n, rows, cols) and str(got.dtype) == "torch.int16"
        assert np.array_equal(got.cpu().numpy().view(np.uint16), want), f"{c.name} Distance({key})"
    out = torch.full((3, rows, cols), POISON, dtype=torch.int16, device="cuda")
    assert idx.Distance(0, 2, 3, out=out) is out and np.array_equal(out.cpu().numpy().view(np.uint16), cs.sp_truth(name, 0)[2:5])
    with pytest.raises(CodecError):
        idx.Distance(0, 2, 3, out=out.to(torch.int32))
    # a reference tensor the kernel would read past or misread is refused in Python, before the native call: `out` keeps its poison
    out.fill_(POISON)
    px = c.w * c.h
    bad = {"short": bufs[0][:px - 1], "int16": torch.zeros(2 * px, dtype=torch.int16, device="cuda"),
           "strided": torch.zeros(2 * px, dtype=torch.int32, device="cuda")[::2], "host tensor": torch.zeros(px, dtype=torch.int32),
           "host array": np.zeros(px, dtype=np.int32)}
    for what, ref in bad.items():
        with pytest.raises(CodecError):
            idx.Distance(ref, 2, 3, out=out)
        assert bool(torch.all(out == POISON)), what
    assert gpu.PreviousFrame() is None
    idx.close()
    gpu.StopAndClean()


@pytest.mark.parametrize("name", ac.NAMES)
def test_pictures_that_come_back(name):
    """Against the frame before ZERO_AT the blocks are nearer again at the matching RESTORE_AT, and the pictures before ZERO_AT = 31,
    46, 62 and the one REPEAT_AT repeats are found again at other frames: totals of 0 (what test_index_distance_ref_cpu.py asserts of
    the truth, here of the GPU's answer)."""
    case = cs.sp_case(name)
    c = case.clip
    gpu = make_sp(c, lines=case.key_row)
    idx = gpu.BuildScrubIndex(c.chunks, c.keys, key_row=case.key_row)
    for ref, restored in cs.SP_RETURNS:
        got = idx.Distance(ref).cpu().numpy().view(np.uint16)
        assert np.array_equal(got, cs.sp_truth(name, ref)), f"{c.name} ref {ref}"
        d = got.reshape(case.n, -1).astype(np.int64)
        assert (d[ref + 1] >= d[restored]).all() and (d[ref + 1] > d[restored]).any() and not d[ref].any()
    for ref in [z - 1 for z in ac.ZERO_AT[2:]] + [ac.REPEAT_AT]:
        totals = idx.Distance(ref).cpu().numpy().view(np.uint16).reshape(case.n, -1).sum(axis=1)
        assert [t for t in range(case.n) if t != ref and totals[t] == 0], f"{c.name}: no frame but {ref} shows its picture"
    idx.close()
    gpu.StopAndClean()
