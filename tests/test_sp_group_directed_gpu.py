"""The two inter-frame group kernels, sp_pframe_group_kernel (a loader wave) and sp_pframe_group1_kernel (the workgroup stages its
own chunks), on the directed clips of tests/sp_group_clips.py, on an MI355X: chunks of one frame in a row, a chunk that fills the
literal buffer to the word, a cut that only the rounding to four words decides, frames that change nothing inside a chunk and
behind a cut, workgroups that idle beside busy ones, the workgroup with one 12 (11) pixel block, groups of 1, 16, 17, 33 and 97
frames (tests/test_sp_group_clips_cpu.py asserts that the clips hold all of that, for both forms).

Truth: the painted pictures, which are also the oracle's sequential run.  Everything is bit-exact.  Every pixel names the frame
that wrote it last, so a failure says which frame's record or literals showed up in place of which (describe_mismatch)."""
import numpy as np
import pytest

import sp_group_clips as gc
from jsplayer_amd import ScreenPressor
from test_screenpressor_gpu import dev_buf, drive_pair, to_np

pytestmark = pytest.mark.gpu

LOADER, SELF = "sp_pframe_group_kernel", "sp_pframe_group1_kernel"
# clip, buffers 4 bytes into their allocation, the kernel the groups take
CASES = [("L", False, LOADER), ("L", True, SELF), ("S", False, SELF), ("H", False, LOADER), ("H", True, SELF)]
IDS = ["%s-%s" % (name, "misaligned" if mis else "aligned") for name, mis, _ in CASES]
POISON = -1


def codec(c):
    gpu = ScreenPressor(c.w, c.h, c.bpp)
    gpu.Preinit(gc.KEY_ROW)
    return gpu


def exact(c, buf, t, what):
    got = to_np(buf).view(np.uint32)
    assert np.array_equal(got, c.frames[t]), f"{c.name} {what} frame {t}: " + gc.describe_mismatch(got, c.frames[t], c.w, c.h, c.bpp)


def coded(adopted):
    return [t for t in range(gc.N) if adopted[t]]


@pytest.mark.parametrize("name,misalign,kernel", CASES, ids=IDS)
def test_a_buffer_per_frame_replayed(name, misalign, kernel):
    c = gc.clip(name)
    gpu = codec(c)
    dsts = [dev_buf(c.w * c.h, POISON, misalign) for _ in range(gc.N)]
    extra = dev_buf(c.w * c.h, POISON, misalign)                     # never listed: must stay as it is
    assert all(d.data_ptr() % 16 == (4 if misalign else 0) for d in dsts)
    st = gpu.stage_batch(c.chunks, dsts, is_key=c.keys)
    assert st.info()["kernel_launches"] == len(gc.KEYS) + len(gc.GROUP_LENGTHS)
    other = SELF if kernel == LOADER else LOADER
    assert kernel in st.kernels() and other not in st.kernels() and "sp_pframe_kernel" not in st.kernels(), st.kernels()
    for _ in range(2):                                               # replayable
        st.decode()
    gpu.sync()
    status, adopted, _ = st.results()
    assert status == [0] * gc.N
    assert [t for t in range(gc.N) if not adopted[t]] == list(gc.UNCHANGED)
    for t in range(gc.N):
        if adopted[t]:
            exact(c, dsts[t], t, "a buffer per frame,")
        else:
            assert bool((dsts[t] == POISON).all()), f"{c.name}: frame {t} changes nothing, its buffer was written"
    assert bool((extra == POISON).all()), f"{c.name}: a buffer that was not listed was written"
    st.close()
    gpu.StopAndClean()


@pytest.mark.parametrize("name,misalign,kernel", CASES, ids=IDS)
def test_three_buffers_in_rotation(name, misalign, kernel):
    """A pool used as a player uses it (never the buffer that holds the picture before; a frame that changes nothing takes none):
    afterwards each buffer holds the last frame decoded into it."""
    c = gc.clip(name)
    gpu = codec(c)
    pool = [dev_buf(c.w * c.h, POISON, misalign) for _ in range(3)]
    order, k = [], 0
    for t in range(gc.N):
        order.append(pool[k % 3])
        k += 0 if t in gc.UNCHANGED else 1
    st = gpu.stage_batch(c.chunks, order, is_key=c.keys)
    assert kernel in st.kernels(), st.kernels()
    st.decode()
    gpu.sync()
    status, adopted, _ = st.results()
    assert status == [0] * gc.N and [t for t in range(gc.N) if not adopted[t]] == list(gc.UNCHANGED)
    for b in pool:
        mine = [t for t in coded(adopted) if order[t] is b]
        exact(c, b, mine[-1], "three buffers in rotation,")
    st.close()
    gpu.StopAndClean()


@pytest.mark.parametrize("name,misalign", [(n, m) for n, m, _ in CASES if n != "H" or not m], ids=[i for i in IDS if i != "H-misaligned"])
def test_one_launch_per_frame_gives_the_same_pictures(name, misalign):
    """The same batch with the fusion switched off: sp_pframe_kernel frame by frame."""
    c = gc.clip(name)
    gpu = codec(c)
    gpu.set_option("sp_inter_fusion", "off")
    dsts = [dev_buf(c.w * c.h, POISON, misalign) for _ in range(gc.N)]
    st = gpu.stage_batch(c.chunks, dsts, is_key=c.keys)
    assert "sp_pframe_kernel" in st.kernels() and "group" not in st.kernels(), st.kernels()
    assert st.info()["kernel_launches"] == gc.N - len(gc.UNCHANGED)
    st.decode()
    gpu.sync()
    status, adopted, _ = st.results()
    assert status == [0] * gc.N
    for t in coded(adopted):
        exact(c, dsts[t], t, "one launch per frame,")
    assert [t for t in range(gc.N) if not adopted[t]] == list(gc.UNCHANGED)
    st.close()
    gpu.StopAndClean()


@pytest.mark.parametrize("name,misalign", [("L", False), ("S", True), ("H", False)], ids=["L", "S-misaligned", "H"])
def test_frame_by_frame_beside_the_oracle(name, misalign):
    """DecompressI / DecompressP call by call, the oracle beside them: the same pictures, the painted ones."""
    c = gc.clip(name)
    drive_pair(c.w, c.h, c.bpp, c.chunks, c.keys, c.frames, lines=gc.KEY_ROW, misalign=misalign)
