"""A key frame for any frame of an MSVideo1 seek index (jsp_index_key_frame / SeekIndex.KeyFrame) on an MI355X.

Truth: tests/index_keyframe_ref.py, the rule in plain Python, which test_index_keyframe_ref_cpu.py pins to the oracle — nothing of it
comes from the GPU.  Every case compares BYTES, exactly, and refusals against the reference's verdicts."""
import ctypes as C

import numpy as np
import pytest

import index_keyframe_ref as kr
from jsplayer_amd import CodecError
from jsplayer_amd import _native as N
from msv1_range_clips import POISON, Idle, dev_buf, long_clip, make_gpu, palette, truth_run

pytestmark = pytest.mark.gpu

MSV1_N = 72      # frames of the index's range: bitmap words 0, 1, 2
FILL = 0xA5      # what `out` holds before a call
WG_BLOCKS = 1024   # MSV1_KEYFRAME_WG_BLOCKS (msv1_seek.h): consecutive blocks a workgroup of the two kernels owns
PARSE = "host"     # the msv1_parse of every codec built here; TestOnGpuParse (the end of this file) runs every test with "gpu" too


def sequential(gpu, frames, keys, hi, pool):
    for i in range(hi):
        prev = gpu.PreviousFrame()
        dst = next(b for b in pool if b is not prev)
        if keys[i]:
            assert gpu.DecompressI(frames[i], dst) == 0
        else:
            gpu.DecompressP(frames[i], dst)


def covered(pic, w, h):
    return np.asarray(pic).reshape(h, w)[:4 * (h // 4), :4 * (w // 4)]


class Case:
    """A codec brought to frame `start` of a clip frame by frame, its index over the `count` frames from there on, and the
    reference's codes of every frame of that range."""

    def __init__(self, bits, w, h, pal, frames, keys, lines=36, start=0, count=None, chunk=None):
        count = len(frames) - start if count is None else count
        self.bits, self.w, self.h, self.n, self.pal, self.lines = bits, w, h, count, pal, lines
        self.nbx, self.nby = w // 4, h // 4
        self.range, self.range_keys = frames[start:start + count], keys[start:start + count]
        self.codes = [kr.codes_of(bits, self.nbx, self.nby, f) for f in self.range]
        self.gpu = make_gpu(bits, w, h, pal, lines, chunk, PARSE)
        self.pool = [dev_buf(w * h) for _ in range(3)]
        sequential(self.gpu, frames, keys, start, self.pool)
        self.idx = self.gpu.BuildIndex(self.range, self.range_keys)
        assert self.idx.frames == count
        self.bound = self.idx.KeyFrameBound()
        assert self.bound == self.nbx * self.nby * (18 if bits == 16 else 10)
        self.where = f"{bits}-bit {w}x{h} start={start} chunk={chunk} ({PARSE} parse)"

    def want(self, t):
        return kr.key_frame(self.bits, self.nbx, self.nby, self.range, t, self.codes)

    def raw(self, t, cap=None):
        """The C call into a host array of FILL: (rc, *len, the array — 16 bytes longer than the bound)."""
        out = np.full(self.bound + 16, FILL, dtype=np.uint8)
        n = C.c_size_t(12345)
        rc = N.lib().jsp_index_key_frame(self.gpu._h, self.idx._h, t, C.c_void_p(out.ctypes.data), self.bound if cap is None else cap, C.byref(n))
        return rc, n.value, out

    def check(self, t):
        """Frame t against the reference: the bytes, or the refusal.  Returns the reference's answer."""
        want = self.want(t)
        where = f"{self.where} t={t}"
        prev = self.gpu.PreviousFrame()
        rc, n, out = self.raw(t)
        if isinstance(want, bytes):
            assert rc == 0, where + ": " + N.last_error()
            assert n == len(want) <= self.bound, where
            assert out[:n].tobytes() == want, where
            assert np.all(out[n:] == FILL), where + ": written behind the frame"
            assert self.idx.KeyFrame(t) == want, where
        else:
            kind, blk = want
            err = N.last_error()
            assert rc != 0 and n == 0, where
            assert err.startswith("index_key_frame:") and f"block {blk} " in err, (where, err)
            assert ("no writer" in err) == (kind == "none") and ("cut off" in err) == (kind == "cut"), (where, err)
            if kind == "cut":   # ... and names the frame whose code it is: the block's last writer
                assert f"block {blk} in frame {kr.cut_writer(self.codes, t, blk)}," in err, (where, err)
            assert np.all(out == FILL), where + ": written on a refusal"
            with pytest.raises(CodecError, match=f"block {blk} "):
                self.idx.KeyFrame(t)
        assert self.gpu.PreviousFrame() is prev, where
        return want

    def close(self):
        self.idx.close()
        self.gpu.StopAndClean()


@pytest.mark.parametrize("bits", [16, 8])
@pytest.mark.parametrize("size", [(64, 32), (52, 28), (54, 30)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("start", [0, 3], ids=["nothing_before", "picture_before"])
def test_every_frame_is_the_references_bytes_or_its_refusal(bits, size, start):
    w, h = size
    frames, keys, pal, plan = long_clip(bits, w, h, seed=5, n=96)
    assert not plan["raises"]
    truth = truth_run(bits, w, h, pal, frames[:start + MSV1_N], keys[:start + MSV1_N], plan["lines"], key_row=plan["lines"])
    c = Case(bits, w, h, pal, frames, keys, plan["lines"], start, MSV1_N)
    dst = dev_buf(w * h)
    cut, refused = 0, 0
    for t in range(MSV1_N):
        want = c.check(t)
        cut += isinstance(want, bytes)
        refused += not isinstance(want, bytes)
        # the codec and the index are untouched: Show still gives the oracle's picture
        c.idx.Show(t, dst, adopt=False)
        assert np.array_equal(covered(dst.cpu().numpy(), w, h), covered(truth[start + t][0], w, h)), f"{c.where} t={t}: Show after KeyFrame"
    assert cut > 0 and (refused > 0 or (bits, start) == (8, 0)), (cut, refused)   # (8-bit from frame 0: every frame can be cut)
    c.close()


def seam_clip(bits):
    """256 x 132 = 2112 blocks: two full workgroups of WG_BLOCKS = 1024 blocks and one of 64."""
    w, h = 256, 132
    g = Idle(bits, w, h, seed=11)
    nb = g.nb
    assert nb == 2 * WG_BLOCKS + 64
    frames = [g.key()] + [g.recode(range(k, nb, 3)) for k in range(3)] + [g.change(range(0, nb, 7)), g.recode(range(nb), how="eight")]
    return w, h, frames, [True] + [False] * 5


@pytest.mark.parametrize("bits", [16, 8])
def test_workgroup_seams_unaligned_bases_and_the_image_at_its_bound(bits):
    w, h, frames, keys = seam_clip(bits)
    c = Case(bits, w, h, palette(bits), frames, keys)
    lens = []
    for t in range(6):
        want = c.check(t)
        assert isinstance(want, bytes)
        lens.append(len(want))
    assert max(lens) <= c.bound
    nb = c.nbx * c.nby
    assert lens[0] == 2 * nb                                   # frame 0: all 2-byte codes
    assert lens[5] == c.bound                                  # frame 5: all 8-colour, every workgroup's image at its bound
    # the base of workgroup 1 (the bytes of blocks 0 .. 1023) is no multiple of 16 at some t, and at 8 bits of 4 neither (3246 at
    # t = 1, 4350 at t = 2): the image's first piece leaves 16 bits at a time
    bases = []
    for t in (1, 2, 3, 4):
        writers = [next(f for f in range(t, -1, -1) if c.codes[f][b] is not None) for b in range(WG_BLOCKS)]
        bases.append(sum(c.codes[f][b][1] for b, f in enumerate(writers)))
    assert any(b % 16 != 0 for b in bases), bases
    if bits == 8:
        assert bases[:2] == [3246, 4350] and all(b % 4 == 2 for b in bases[:2])
    c.close()


@pytest.mark.parametrize("bits", [16, 8])
@pytest.mark.parametrize("start", [0, 3])
def test_a_chunked_index_gives_the_same_bytes(bits, start):
    """msv1_seek_chunk_frames = 7: the last writers lie in other chunks than t."""
    w, h = 64, 32
    frames, keys, pal, plan = long_clip(bits, w, h, seed=5, n=96)
    c = Case(bits, w, h, pal, frames, keys, plan["lines"], start, MSV1_N, chunk=7)
    answers = [c.check(t) for t in range(MSV1_N)]
    assert any(isinstance(a, bytes) for a in answers)
    c.close()


@pytest.mark.parametrize("bits", [16, 8])
def test_cap_and_bound(bits):
    w, h = 64, 32
    frames, keys, pal, plan = long_clip(bits, w, h, seed=5, n=96)
    c = Case(bits, w, h, pal, frames, keys, plan["lines"], 0, 40)
    assert c.bound == c.nbx * c.nby * (18 if bits == 16 else 10)
    seen = 0
    for t in (0, 7, 20):
        want = c.want(t)
        assert isinstance(want, bytes)
        seen = max(seen, len(want))
        rc, n, out = c.raw(t, cap=len(want) - 1)              # one byte short: refused, *len still set, nothing written
        assert rc != 0 and n == len(want) and np.all(out == FILL) and "cap is smaller" in N.last_error(), N.last_error()
        rc, n, out = c.raw(t, cap=0)                           # asking for the length
        assert rc != 0 and n == len(want) and np.all(out == FILL)
        n2 = C.c_size_t(0)
        assert N.lib().jsp_index_key_frame(c.gpu._h, c.idx._h, t, None, 0, C.byref(n2)) != 0 and n2.value == len(want)
        rc, n, out = c.raw(t, cap=len(want))                   # exactly the length
        assert rc == 0 and n == len(want) and out[:n].tobytes() == want and np.all(out[n:] == FILL)
    assert c.bound >= seen
    at_build = c.idx.device_bytes                              # the scratch is the index's and counted (jsp_index_info)
    c.idx.KeyFrame(0)
    assert c.idx.device_bytes - at_build >= 16 + 4 + 8 * c.nbx * c.nby + c.bound
    c.close()


def test_a_picture_without_a_block_is_refused_before_any_launch():
    gpu = make_gpu(16, 3, 8, parse=PARSE)
    idx = gpu.BuildIndex([b"\x01\x02\x03\x04", b""], [True, False])
    assert idx.KeyFrameBound() == 0
    out = np.full(16, FILL, dtype=np.uint8)
    n = C.c_size_t(5)
    assert N.lib().jsp_index_key_frame(gpu._h, idx._h, 0, C.c_void_p(out.ctypes.data), 16, C.byref(n)) != 0
    assert N.last_error() == "index_key_frame: the picture has no 4x4 block" and n.value == 0 and np.all(out == FILL)
    with pytest.raises(CodecError, match="no 4x4 block"):
        idx.KeyFrame(1)
    idx.close()
    gpu.StopAndClean()


@pytest.mark.parametrize("bits", [16, 8])
def test_round_trip_through_the_gpu_codec(bits):
    """A fresh codec decodes KeyFrame(t) as a key frame and the original frames t + 1 .. t + 3 on top: each picture is Show's."""
    w, h = 54, 30
    frames, keys, pal, plan = long_clip(bits, w, h, seed=5, n=96)
    c = Case(bits, w, h, pal, frames, keys, plan["lines"], 0, MSV1_N)
    cuttable = [t for t in range(MSV1_N - 3) if isinstance(c.want(t), bytes)]
    shown = dev_buf(w * h)
    for t in (cuttable[0], cuttable[len(cuttable) // 2], cuttable[-1]):
        kf = c.idx.KeyFrame(t)
        fresh = make_gpu(bits, w, h, pal, plan["lines"], parse=PARSE)
        assert fresh.IsKeyFrame(kf)
        pool = [dev_buf(w * h) for _ in range(2)]
        assert fresh.DecompressI(kf, pool[0]) == 0
        for k in range(4):
            if k > 0:
                prev = fresh.PreviousFrame()
                dst = next(b for b in pool if b is not prev)
                dst.copy_(prev)
                if c.range_keys[t + k]:
                    assert fresh.DecompressI(c.range[t + k], dst) == 0
                else:
                    fresh.DecompressP(c.range[t + k], dst)
            shown.fill_(POISON)
            c.idx.Show(t + k, shown, adopt=False)
            assert np.array_equal(covered(fresh.PreviousFrame().cpu().numpy(), w, h), covered(shown.cpu().numpy(), w, h)), \
                f"{c.where}: frame {t + k} on top of KeyFrame({t})"
        fresh.StopAndClean()
    c.close()


class TestOnGpuParse:
    """Every test of this file once more with the block tables of the on-GPU parse — the codec's default, under which frames too
    short to code every block still get their table from the host parser: one index then mixes both sources.  (The tests above keep
    the host parser and their names.)"""

    @pytest.fixture(autouse=True)
    def parse_mode(self):
        global PARSE
        PARSE = "gpu"
        yield PARSE
        PARSE = "host"


for _name, _test in list(globals().items()):
    if _name.startswith("test_"):
        setattr(TestOnGpuParse, _name, staticmethod(_test))
