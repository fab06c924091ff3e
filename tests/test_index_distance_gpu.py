"""The distance map of an MSVideo1 seek index (jsp_index_distance / SeekIndex.Distance) on an MI355X.

Truth: THE DEFINITION (tests/index_distance_ref.py: pixels per 16 x 16 cell, inside whole 4 x 4 blocks, that differ from ONE reference
picture) over the oracle's sequential run (tests/index_distance_cases.py, which test_index_distance_ref_cpu.py holds against a
brute-force compare first) — nothing of it comes from the GPU.  Every case compares the WHOLE array, exactly."""
import ctypes as C

import numpy as np
import pytest

import index_activity_ref as ar
import index_distance_cases as cs
import index_distance_ref as dr
from jsplayer_amd import CodecError
from jsplayer_amd import _native as N
from msv1_range_clips import Idle, dev_buf, make_gpu, make_plan, palette, truth_run
from test_index_activity_gpu import sequential

pytestmark = pytest.mark.gpu

PARSE = "host"   # the msv1_parse of every codec built here; TestOnGpuParse (the end of this file) runs every test with "gpu" too
SENTINEL = 0x7BCD
REF_PICTURE = -2


def to_device(words, misalign=False):
    """A device frame buffer holding `words`; misalign: at an address 4 bytes off a 16-byte boundary."""
    import torch
    buf = dev_buf(len(words), misalign=misalign)
    buf.copy_(torch.from_numpy(np.array(words, dtype=np.int32)))
    assert buf.data_ptr() % 16 == (4 if misalign else 0)
    return buf


class Case:
    """A codec brought to frame c.start of a clip frame by frame and its index over the c.n frames from there on (c: a case of
    index_distance_cases)."""

    def __init__(self, c, chunk=None):
        self.c = c
        self.gpu = make_gpu(c.bits, c.w, c.h, c.pal, c.lines, chunk, PARSE)
        self.pool = [dev_buf(c.w * c.h) for _ in range(3)]
        sequential(self.gpu, c.frames, c.keys, c.start, self.pool)
        self.idx = self.gpu.BuildIndex(c.frames[c.start:c.start + c.n], c.keys[c.start:c.start + c.n])
        assert self.idx.frames == c.n
        self.where = f"{c.bits}-bit {c.w}x{c.h} start={c.start} ({PARSE} parse)"

    def check(self, ref, want, first, n, what=""):
        got = self.idx.Distance(ref, first, n)
        cols, rows = ar.grid(self.c.w, self.c.h)
        assert tuple(got.shape) == (n, rows, cols) and str(got.dtype) == "torch.int16"
        got = got.cpu().numpy().view(np.uint16)
        assert np.array_equal(got, want[first:first + n]), f"{self.where} first={first} n={n} {what}"
        return got

    def close(self):
        self.idx.close()
        self.gpu.StopAndClean()


@pytest.mark.parametrize("bits", [16, 8])
@pytest.mark.parametrize("size", cs.MSV1_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("start", cs.MSV1_STARTS, ids=["nothing_before", "picture_before"])
def test_every_run_and_reference_equals_the_definition(bits, size, start):
    w, h = size
    c = cs.msv1_case(bits, w, h, start)
    g = Case(c)
    for ref in cs.msv1_ref_frames():
        want = cs.msv1_truth(bits, w, h, start, ref)
        for first, n in cs.msv1_runs():
            g.check(ref, want, first, n, f"ref frame {ref}")
    pictures = cs.msv1_pictures_for(bits, w, h, start)
    for name in ("frame", "poisoned", "random"):
        want = cs.msv1_truth(bits, w, h, start, name)
        for misalign in (False, True):   # (4- but not 16-byte aligned: the scalar loads of R, also where X % 4 == 0)
            buf = to_device(pictures[name], misalign)
            for first, n in cs.msv1_runs():
                g.check(buf, want, first, n, f"ref picture {name} misalign={misalign}")
            assert np.array_equal(buf.cpu().numpy(), pictures[name]), "the reference picture is only read"
    assert np.array_equal(cs.msv1_truth(bits, w, h, start, "poisoned"), cs.msv1_truth(bits, w, h, start, cs.MSV1_PICTURE_AT))
    if (w, h) == (3, 3):
        assert not any(cs.msv1_truth(bits, w, h, start, r).any() for r in cs.msv1_references())
    g.close()


@pytest.mark.parametrize("bits", [16, 8])
def test_segments_do_not_change_the_map(bits):
    w, h, start = 52, 28, 3
    g = Case(cs.msv1_case(bits, w, h, start))
    buf = to_device(cs.msv1_pictures_for(bits, w, h, start)["random"])
    for segs in ("1", "2", "7", "auto"):
        g.gpu.set_option("msv1_index_activity_segments", segs)
        for ref, want in ((-1, cs.msv1_truth(bits, w, h, start, -1)), (32, cs.msv1_truth(bits, w, h, start, 32)),
                          (buf, cs.msv1_truth(bits, w, h, start, "random"))):
            for first, n in ((0, g.c.n), (31, 3), (32, 33), (5, 1)):
                g.check(ref, want, first, n, f"segments={segs}")
    g.close()


@pytest.mark.parametrize("bits", [16, 8])
def test_an_index_built_in_chunks_of_7(bits):
    w, h, start = 54, 30, 3
    g = Case(cs.msv1_case(bits, w, h, start), chunk=7)
    for ref in (-1, 31, cs.MSV1_PICTURE_AT):
        want = cs.msv1_truth(bits, w, h, start, ref)
        for first, n in cs.msv1_runs():
            g.check(ref, want, first, n, f"chunks of 7, ref {ref}")
    g.close()


@pytest.mark.parametrize("bits", [16, 8])
@pytest.mark.parametrize("size", cs.MSV1_DIRECTED_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_blocks_that_return_and_blocks_that_change_in_one_pixel(bits, size):
    """msv1_tight_clips.directed.  Against frame 1 the spots are back at frame 4 (`back`): a spot's cell holds only the 16 pixels of
    each block behind a spot that frame 3 changed and nothing restored — 0 where it has none — while at frames 2 and 3 the spots
    count.  Against frame 4, frame 5 (`one_pixel`) counts exactly one pixel per changed block."""
    w, h = size
    c = cs.msv1_directed(bits, w, h)
    g = Case(c)
    d1 = g.check(1, cs.msv1_directed_truth(bits, w, h, 1), 0, c.n, "ref frame 1")
    stay = cs.cells_of_blocks(sorted(set(c.clip.next_blocks) - set(c.clip.spots)), w, h)
    for (r, q), k in cs.cells_of_blocks(c.clip.spots, w, h).items():
        assert d1[2, r, q] >= 16 * k and d1[3, r, q] >= 16 * k and d1[4, r, q] == 16 * stay.get((r, q), 0)
    if (w, h) == (128, 128):   # (12 x 8 is one cell, which holds a block that stays changed)
        back = [at for at in cs.cells_of_blocks(c.clip.spots, w, h) if at not in stay]
        assert back and all(d1[4][at] == 0 and d1[2][at] > 0 and d1[3][at] > 0 for at in back), "no spot's cell is 0 again at `back`"
    assert not d1[0].any() and not d1[1].any()
    d4 = g.check(4, cs.msv1_directed_truth(bits, w, h, 4), 0, c.n, "ref frame 4")
    assert int(d4[5].sum()) == len(c.clip.pixel_blocks) and d4[5].max() <= len(c.clip.pixel_blocks)
    g.check(4, cs.msv1_directed_truth(bits, w, h, 4), 5, 1, "ref frame 4")
    g.close()


@pytest.mark.parametrize("bits", [16, 8])
def test_recoded_blocks_change_no_element(bits):
    """Idle.recode codes blocks again with the pixels they had: the bitmap bits are set, the walk decodes and recounts, and every
    element stays what it was — against the key frame (zeros), the picture before it (nothing: zeros) and a device picture."""
    w, h = 64, 32
    gen = Idle(bits, w, h, seed=3)
    frames = [gen.key()] + [gen.recode(list(range(k, gen.nb, 3))) for k in range(3)] + [gen.change([gen.nb - 1])]
    keys = [True] + [False] * 4
    pal = palette(bits)
    plan = make_plan(bits, w, h, frames, keys, 36)
    assert plan["coded"][1:4].any(axis=1).all()
    truth = truth_run(bits, w, h, pal, frames, keys, 36, key_row=36)
    p_before, p = ar.msv1_pictures([t[0] for t in truth], plan["coded"], w, h, None)
    from types import SimpleNamespace
    g = Case(SimpleNamespace(bits=bits, w=w, h=h, start=0, n=5, frames=frames, keys=keys, pal=pal, lines=36))
    rng = np.random.default_rng(9)
    pic = np.where(rng.random(w * h) < 0.5, np.asarray(p[0], dtype=np.int32), np.int32(0x00123456)).astype(np.int32)
    for ref, R in ((0, p[0]), (-1, p_before), (to_device(pic), pic)):
        got = g.check(ref, dr.distance(p, R, w, h, True), 0, 5)
        assert all(np.array_equal(got[k], got[0]) for k in (1, 2, 3))
        # (a block that takes another colour is as far from the zeros of P(-1) as before)
        assert np.array_equal(got[4], got[0]) == (isinstance(ref, int) and ref == -1)
    g.close()


@pytest.mark.parametrize("bits", [16, 8])
def test_every_element_is_written_and_nothing_else(bits):
    """`out` in the middle of a poisoned buffer, at an even and at an odd 16-bit element: the launch itself writes every element of the
    map — nothing zeroes it first — and none outside it; the reference buffer and the codec stay as they were."""
    import torch
    w, h, start = 272, 16, 3
    c = cs.msv1_case(bits, w, h, start)
    g = Case(c)
    cols, rows = ar.grid(w, h)
    cell = rows * cols
    lib = N.lib()
    front = (cell + 1) & ~1
    raw = torch.empty((front + 1 + c.n * cell + front,), dtype=torch.int16, device="cuda")
    prev = g.gpu.PreviousFrame()
    prev_pic = prev.cpu().numpy().copy()
    pic = cs.msv1_pictures_for(bits, w, h, start)["random"]
    buf = to_device(pic)
    i = 0
    for ref_frame, ref_ptr, name in ((31, None, 31), (REF_PICTURE, C.c_void_p(buf.data_ptr()), "random"), (-1, None, -1)):
        want = cs.msv1_truth(bits, w, h, start, name)
        for first, n in cs.msv1_runs():
            at = front + (i & 1)
            i += 1
            raw.fill_(SENTINEL)
            assert lib.jsp_index_distance(g.gpu._h, g.idx._h, ref_frame, ref_ptr, first, n, C.c_void_p(raw.data_ptr() + 2 * at), n * cell) == 0, N.last_error()
            host = raw.cpu().numpy()
            want_buf = np.full(host.shape, SENTINEL, dtype=np.int16)
            want_buf[at:at + n * cell] = want[first:first + n].reshape(-1).view(np.int16)
            assert np.array_equal(host, want_buf), f"{g.where} ref {name} run ({first}, {n}) out at element {at}"
    assert np.array_equal(buf.cpu().numpy(), pic)
    # the codec's previous frame as the reference: it is only read, and the codec goes on
    want = dr.distance(c.p, prev_pic, w, h, True)
    g.check(prev, want, 0, c.n, "ref = the codec's previous frame")
    assert g.gpu.PreviousFrame() is prev and np.array_equal(prev.cpu().numpy(), prev_pic)
    out = torch.full((5, rows, cols), SENTINEL, dtype=torch.int16, device="cuda")
    assert g.idx.Distance(31, 30, 5, out=out) is out
    assert np.array_equal(out.cpu().numpy().view(np.uint16), cs.msv1_truth(bits, w, h, start, 31)[30:35])
    with pytest.raises(CodecError):
        g.idx.Distance(31, 30, 5, out=out[:, :, :1])
    # a reference tensor the kernel would read past or misread is refused in Python, before the native call: `out` keeps its poison
    out.fill_(SENTINEL)
    bad = {"short": buf[:w * h - 1], "int16": torch.zeros(2 * w * h, dtype=torch.int16, device="cuda"),
           "uint8": torch.zeros(4 * w * h, dtype=torch.uint8, device="cuda"), "strided": torch.zeros(2 * w * h, dtype=torch.int32, device="cuda")[::2],
           "host tensor": torch.zeros(w * h, dtype=torch.int32), "host array": np.zeros(w * h, dtype=np.int32), "bool": True, "float": 1.5}
    for what, ref in bad.items():
        with pytest.raises(CodecError):
            g.idx.Distance(ref, 30, 5, out=out)
        assert bool(torch.all(out == SENTINEL)), what
    g.close()


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
