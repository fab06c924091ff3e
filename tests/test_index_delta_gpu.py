"""Inter frames that span a gap of an MSVideo1 seek index (jsp_index_delta_frames / SeekIndex.DeltaFrames) on an MI355X.

Truth: tests/index_delta_ref.py, the rule in plain Python, which test_index_delta_ref_cpu.py pins to the oracle — nothing of it comes
from the GPU.  Every case compares BYTES, exactly, and refusals against the reference's verdicts.  The directed clips
(tests/msv1_delta_clips.py) put written blocks and runs on the seams of the kernels' lanes (4 blocks), waves (256), workgroups (1024)
and of the skip word's count (multiples of 1023)."""
import ctypes as C

import numpy as np
import pytest

import index_delta_ref as dr
import index_keyframe_ref as kr
import msv1_delta_clips as dc
from jsplayer_amd import CodecError, ScreenPressor
from jsplayer_amd import _native as N
from msv1_range_clips import POISON, dev_buf, long_clip, make_gpu, palette

pytestmark = pytest.mark.gpu

FILL = 0xA5      # what `out` holds before a call
PARSE = "host"   # the msv1_parse of every codec built here; TestOnGpuParse (the end of this file) runs the tests with "gpu" too
_want = {}       # the reference's answers, worked out once per clip and start


def covered(pic, w, h):
    return np.asarray(pic).reshape(h, w)[:4 * (h // 4), :4 * (w // 4)]


def sequential(gpu, frames, keys, hi, pool):
    for i in range(hi):
        prev = gpu.PreviousFrame()
        dst = next(b for b in pool if b is not prev)
        if prev is not None:
            dst.copy_(prev)
        if keys[i]:
            assert gpu.DecompressI(frames[i], dst) == 0
        else:
            gpu.DecompressP(frames[i], dst)


class Case:
    """A codec brought to frame `start` of a clip frame by frame, its index over the frames from there on, and the reference's
    answer for every pair asked of it."""

    def __init__(self, name, bits, w, h, frames, keys, start=0, chunk=None, lines=36):
        self.name, self.bits, self.w, self.h, self.start = name, bits, w, h, start
        self.nbx, self.nby = w // 4, h // 4
        self.nb = self.nbx * self.nby
        self.pal = palette(bits)
        self.range, self.range_keys = frames[start:], keys[start:]
        self.n = len(self.range)
        key = (name, bits, start)
        if key not in _want:
            _want[key] = ([kr.codes_of(bits, self.nbx, self.nby, f) for f in self.range], {})
        self.codes, self.answers = _want[key]
        self.gpu = make_gpu(bits, w, h, self.pal, lines, chunk, PARSE)
        self.pool = [dev_buf(w * h) for _ in range(3)]
        sequential(self.gpu, frames, keys, start, self.pool)
        self.idx = self.gpu.BuildIndex(self.range, self.range_keys)
        assert self.idx.frames == self.n
        self.bound = self.idx.DeltaBound()
        assert self.bound == self.nb * (18 if bits == 16 else 10)
        self.where = f"{name} {bits}-bit {w}x{h} start={start} chunk={chunk} ({PARSE} parse)"

    def want(self, a, b):
        if (a, b) not in self.answers:
            self.answers[(a, b)] = dr.delta(self.bits, self.nbx, self.nby, self.range, a, b, self.codes)
        return self.answers[(a, b)]

    def raw(self, pairs, cap=None, room=None):
        """The C call into a host array of FILL: (rc, lens, total, the array — 16 bytes longer than `room`)."""
        n = len(pairs)
        room = n * self.bound if room is None else room
        out = np.full(room + 16, FILL, dtype=np.uint8)
        frm, to = (C.c_int * n)(*[a for a, _ in pairs]), (C.c_int * n)(*[b for _, b in pairs])
        lens, total = (C.c_size_t * n)(*([12345] * n)), C.c_size_t(12345)
        rc = N.lib().jsp_index_delta_frames(self.gpu._h, self.idx._h, n, frm, to, C.c_void_p(out.ctypes.data), room if cap is None else cap,
                                            lens, C.byref(total))
        return rc, list(lens), total.value, out

    def check(self, pairs, python=True):
        """One call for `pairs` against the reference: every frame's bytes back to back, or the first refusal in (pair, block)
        order.  Returns the reference's answers."""
        wants = [self.want(a, b) for a, b in pairs]
        prev = self.gpu.PreviousFrame()
        rc, lens, total, out = self.raw(pairs)
        bad = next((j for j, x in enumerate(wants) if not isinstance(x, bytes)), None)
        if bad is None:
            assert rc == 0, self.where + ": " + N.last_error()
            assert lens == [len(x) for x in wants] and total == sum(lens), self.where
            got, at = out[:total].tobytes(), 0
            for (a, b), x in zip(pairs, wants):
                assert got[at:at + len(x)] == x, f"{self.where} ({a}, {b}] at byte {at} of the call"
                at += len(x)
            assert np.all(out[total:] == FILL), self.where + ": written behind the frames"
            if python:
                assert self.idx.DeltaFrames(pairs) == wants, self.where
        else:
            (a, b), blk = pairs[bad], wants[bad][1]
            err = N.last_error()
            assert rc != 0 and lens == [0] * len(pairs) and total == 0, self.where
            assert err.startswith("index_delta:") and f"pair {bad} ({a}, {b}]" in err and "cut off" in err, (self.where, err)
            assert f"block {blk} in frame {dr.writer(self.codes, a, b, blk)}," in err, (self.where, err)
            assert np.all(out == FILL), self.where + ": written on a refusal"
            if python:
                with pytest.raises(CodecError, match=f"block {blk} in frame"):
                    self.idx.DeltaFrames(pairs)
        assert self.gpu.PreviousFrame() is prev, self.where
        return wants

    def close(self):
        self.idx.close()
        self.gpu.StopAndClean()


def seam_case(bits, size, **kw):
    clip = dc.seams(bits, *size)
    return Case(clip.name, bits, clip.w, clip.h, clip.frames, clip.keys, **kw), clip


@pytest.mark.parametrize("bits", [16, 8])
@pytest.mark.parametrize("size", dc.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_every_pair_of_the_seam_clips_in_one_call_and_alone(bits, size):
    c, clip = seam_case(bits, size)
    pairs = dc.pairs(c.n)
    wants = c.check(pairs)                                  # frame j starts wherever the frames before it end: unaligned bases
    assert all(isinstance(x, bytes) for x in wants)
    for f in clip.patterns:                                 # n pairs in one call equal n calls: each pattern alone
        c.check([(f - 1, f)], python=False)
    c.check([(-1, c.n - 1)], python=False)
    # the exact values: a gap that writes nothing, a gap that writes everything
    at = {name: f for f, name in clip.patterns.items()}
    assert len(c.want(at["nothing"] - 1, at["nothing"])) == 2 * -(-c.nb // 1023)
    assert c.want(-1, at["every"]) == c.idx.KeyFrame(at["every"])
    assert c.gpu.IsKeyFrame(c.want(at["every"] - 1, at["every"])) and not c.gpu.IsKeyFrame(c.want(at["spots"] - 1, at["spots"]))
    c.close()


@pytest.mark.parametrize("bits", [16, 8])
@pytest.mark.parametrize("size", [(164, 100), (128, 256)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_a_chunked_index_and_one_behind_decoded_frames_give_the_references_bytes(bits, size):
    """msv1_seek_chunk_frames = 3: the last writers lie in other chunks than b.  start = 3: the codec decoded frames 0 .. 2 one by
    one, the index starts behind them, and a = -1 is the picture they left."""
    c, _ = seam_case(bits, size, chunk=3)
    c.check(dc.pairs(c.n))
    c.close()
    c, _ = seam_case(bits, size, start=3)
    c.check(dc.pairs(c.n))
    c.close()
    c, _ = seam_case(bits, size, start=3, chunk=2)
    c.check(dc.pairs(c.n), python=False)
    c.close()


@pytest.mark.parametrize("bits", [16, 8])
def test_the_slice_size_does_not_change_the_bytes(bits):
    c, _ = seam_case(bits, (164, 100))
    pairs = dc.pairs(c.n)[:23]
    rc, lens, total, auto = c.raw(pairs)
    assert rc == 0, N.last_error()
    for s in ("1", "2", "3", "22", "23", "4096", "auto"):
        c.gpu.set_option("msv1_index_delta_slice", s)
        rc, lens2, total2, out = c.raw(pairs)
        assert rc == 0 and lens2 == lens and total2 == total and np.array_equal(out, auto), s
        c.check(pairs[:7], python=False)
    for bad in ("0", "4097", "-1", "x", ""):
        with pytest.raises(CodecError):
            c.gpu.set_option("msv1_index_delta_slice", bad)
    c.close()


@pytest.mark.parametrize("bits", [16, 8])
def test_cap_bound_lens_and_total(bits):
    c, clip = seam_case(bits, (128, 128))
    at_build = c.idx.device_bytes
    pairs = [(-1, 0), (0, 1), (1, 2), (2, 3), (0, 5)]
    wants = [c.want(a, b) for a, b in pairs]
    lens, total = [len(x) for x in wants], sum(len(x) for x in wants)
    assert max(lens) <= c.bound
    for cap in (total - 1, total - 2, 1, 0):                 # too small: refused, lens and *total still set, nothing written
        rc, got_lens, got_total, out = c.raw(pairs, cap=cap)
        assert rc != 0 and got_lens == lens and got_total == total and np.all(out == FILL), cap
        assert "cap is smaller" in N.last_error()
    n = len(pairs)
    frm, to = (C.c_int * n)(*[a for a, _ in pairs]), (C.c_int * n)(*[b for _, b in pairs])
    l2, t2 = (C.c_size_t * n)(), C.c_size_t(0)
    assert N.lib().jsp_index_delta_frames(c.gpu._h, c.idx._h, n, frm, to, None, 0, l2, C.byref(t2)) != 0      # asking for the lengths
    assert list(l2) == lens and t2.value == total
    rc, got_lens, got_total, out = c.raw(pairs, cap=total, room=total)                                           # exactly the length
    assert rc == 0 and got_lens == lens and out[:total].tobytes() == b"".join(wants) and np.all(out[total:] == FILL)
    # the scratch is the index's and counted (jsp_index_info): per pair 8 bytes per block and the frame at its bound
    c.idx.DeltaFrames(pairs)
    assert c.idx.device_bytes - at_build >= n * (8 * c.nb + c.bound)
    c.close()


@pytest.mark.parametrize("bits", [16, 8])
def test_the_first_refusing_pair_and_block_is_named_and_nothing_is_written(bits):
    """msv1_keyframe_cut_clips.firsts_cut: group i is a key frame 4i, frame 4i + 1 cut one byte short of the end of block P7[i]'s
    code (every block behind it is cut too), 4i + 2 codes the blocks behind whole, 4i + 3 codes P7[i]."""
    clip = dc.cuts(bits)
    c = Case(clip.name, bits, clip.w, clip.h, clip.frames, clip.keys)
    ok = [(-1, 0), (0, 3), (4, 7), (11, 12)]
    assert all(isinstance(c.want(a, b), bytes) for a, b in ok)
    assert c.want(4, 5) == ("cut", 3) and c.want(8, 10) == ("cut", 4) and c.want(3, 5) == ("cut", 3) and c.want(20, 21) == ("cut", 1023)
    assert sum(c.codes[5][b] == "cut" for b in range(c.nb)) == c.nb - 3        # many blocks refuse in (3, 5]: the first is named
    for s in ("auto", "1", "2"):
        c.gpu.set_option("msv1_index_delta_slice", s)
        c.check([ok[0], (4, 5), ok[1]])                     # a cut in pair 1, uncut pairs before and after it
        c.check([ok[1], (8, 10), (4, 5), ok[0]])            # two cuts: pair 1 (block 4, frame 9) is named, not pair 2's block 3
        c.check([(20, 21), ok[2], (3, 5)])                  # pair 0, in the workgroup's last lane
        c.check([ok[2], ok[3], ok[0], (3, 5)])              # the last pair of the call
        c.check(ok)                                         # ... and the call works after the refusals
    c.close()


@pytest.mark.parametrize("bits", [16, 8])
def test_long_clip_gaps(bits):
    """Writers that lie bitmap words back, 8-bit end markers, 16-bit truncated frames: a fixed sample of gaps of the long clip."""
    w, h = 52, 28
    frames, keys, pal, plan = long_clip(bits, w, h, seed=5, n=96)
    c = Case("long", bits, w, h, frames[:75], keys[:75], start=3, chunk=7, lines=plan["lines"])
    pairs = [(a, b) for a in range(-1, c.n, 5) for b in (a + 1, a + 2, a + 9, a + 33, a + 40) if b < c.n]
    good = [p for p in pairs if isinstance(c.want(*p), bytes)]
    refused = [p for p in pairs if p not in good]
    assert len(good) > 30 and (bits == 8 or refused)
    c.check(good)
    for p in refused[:3]:
        c.check([good[0], p, good[1]], python=False)
    c.close()


@pytest.mark.parametrize("bits", [16, 8])
def test_round_trip_through_the_gpu_codec(bits):
    """A fresh codec decodes KeyFrame(t0) as a key frame and the Deltas of a stride as inter frames on top: each picture is Show's."""
    c, clip = seam_case(bits, (164, 100))
    for t0, stride in ((0, 1), (1, 3), (2, 4)):
        ts = list(range(t0, c.n, stride))
        frames = [c.idx.KeyFrame(t0)] + c.idx.DeltaFrames(list(zip(ts, ts[1:])))
        fresh = make_gpu(bits, c.w, c.h, c.pal, parse=PARSE)
        pool = [dev_buf(c.w * c.h) for _ in range(2)]
        shown = dev_buf(c.w * c.h)
        for k, (t, data) in enumerate(zip(ts, frames)):
            prev = fresh.PreviousFrame()
            dst = next(b for b in pool if b is not prev)
            if k == 0:
                assert fresh.IsKeyFrame(data) and fresh.DecompressI(data, dst) == 0
            else:
                dst.copy_(prev)
                fresh.DecompressP(data, dst)
            shown.fill_(POISON)
            c.idx.Show(t, shown, adopt=False)
            # (a frame that writes nothing leaves the previous picture standing)
            assert np.array_equal(covered(fresh.PreviousFrame().cpu().numpy(), c.w, c.h), covered(shown.cpu().numpy(), c.w, c.h)), \
                f"{c.where}: frame {t} of the stride {stride} from {t0}"
        fresh.StopAndClean()
    c.close()


def test_every_argument_refusal_and_their_order():
    import torch
    W, H = 40, 24
    from jsplayer_amd import streamgen as sg
    frames, keys, _ = sg.msv1_clip(41, W, H, 6, bits=16, p_mix=sg.msv1_p_mix(0.6, 3.0))
    codec, other = make_gpu(16, W, H, parse=PARSE), make_gpu(16, W, H, parse=PARSE)
    idx, foreign = codec.BuildIndex(frames, keys), other.BuildIndex(frames, keys)
    wrong = ScreenPressor(W, H, 24)
    tiny = make_gpu(16, 3, 8, parse=PARSE)                       # a picture without a 4x4 block
    tiny_idx = tiny.BuildIndex([b"\x01\x02\x03\x04", b""], [True, False])
    lib = N.lib()
    fn, n = lib.jsp_index_delta_frames, idx.frames
    bound = idx.DeltaBound()
    assert n == 6 and bound == (W // 4) * (H // 4) * 18 and tiny_idx.DeltaBound() == 0
    first = idx.DeltaFrames([(0, 2), (2, 3)])                    # (the scratch is allocated here: from now on nothing may grow)
    out = np.full(2 * bound, FILL, dtype=np.uint8)
    stands = {"prev": codec.PreviousFrame()}

    def info():
        k, d, h = C.c_int(0), C.c_uint64(0), C.c_uint64(0)
        assert lib.jsp_index_info(idx._h, C.byref(k), C.byref(d), C.byref(h)) == 0
        return k.value, d.value, h.value

    before = info()

    def refused(what, message, c=codec._h, i=idx._h, pairs=((0, 2), (2, 3)), count=None, dst=out.ctypes.data, cap=2 * bound, lens=True, total=True,
                frm=True, to=True):
        k = len(pairs)
        a, b = (C.c_int * k)(*[p[0] for p in pairs]), (C.c_int * k)(*[p[1] for p in pairs])
        ls, size = (C.c_size_t * k)(*([777] * k)), C.c_size_t(777)
        count = k if count is None else count
        rc = fn(c, i, count, a if frm else None, b if to else None, C.c_void_p(dst) if dst else None, cap, ls if lens else None,
                C.byref(size) if total else None)
        err = N.last_error()
        print(f"jsp_index_delta_frames: {what}: {err}")
        assert rc != 0 and err == message, (what, err)
        assert size.value == (0 if total else 777) and np.all(out == FILL), what
        assert list(ls) == ([0] * k if lens and 1 <= count <= 4096 else [777] * k), what
        assert info() == before and codec.PreviousFrame() is stands["prev"], what

    def dl(what):
        return "index_delta: " + what

    def pair(j, a, b, of=n):
        return dl(f"pair {j} ({a}, {b}] is not a gap of the index (-1 <= from < to < {of} frames)")

    # ---- each refusal alone --------------------------------------------------------------------------------------------------
    refused("null codec", dl("null argument"), c=None)
    refused("null index", dl("null argument"), i=None)
    refused("null from", dl("null argument"), frm=False)
    refused("null to", dl("null argument"), to=False)
    refused("null out with a cap", dl("null argument"), dst=None)
    refused("null lens", dl("null argument"), lens=False)
    refused("null total", dl("null argument"), total=False)
    refused("wrong codec kind", "index: MSVideo1 only", c=wrong._h)
    refused("foreign index", dl("the index was built by another codec"), i=foreign._h)
    for bad in (0, -1, 4097):
        refused(f"n = {bad}", dl("n is outside 1..4096"), count=bad)
    refused("from < -1", pair(1, -2, 3), pairs=((0, 1), (-2, 3)))
    refused("to == from", pair(0, 2, 2), pairs=((2, 2), (0, 1)))
    refused("to < from", pair(1, 3, 1), pairs=((0, 1), (3, 1)))
    refused("to == nframes", pair(0, 0, n), pairs=((0, n),))
    refused("the first bad pair is named", pair(1, 4, 4), pairs=((0, 1), (4, 4), (-5, 2)))
    refused("no block", dl("the picture has no 4x4 block"), c=tiny._h, i=tiny_idx._h, pairs=((0, 1),))
    size = C.c_size_t(7)
    assert lib.jsp_index_delta_bound(None, C.byref(size)) != 0 and N.last_error() == dl("null argument") and size.value == 7
    assert lib.jsp_index_delta_bound(idx._h, None) != 0 and N.last_error() == dl("null argument")

    # ---- the earlier refusal wins ---------------------------------------------------------------------------------------------
    refused("wrong codec kind + foreign index + bad n", "index: MSVideo1 only", c=wrong._h, i=foreign._h, count=0)
    refused("foreign index + bad n", dl("the index was built by another codec"), i=foreign._h, count=0)
    refused("bad n + bad pair", dl("n is outside 1..4096"), pairs=((3, 1),), count=0)
    refused("bad pair + no block", pair(0, 0, 2, of=2), c=tiny._h, i=tiny_idx._h, pairs=((0, 2),))
    frame_buf = torch.zeros(W * H, dtype=torch.int32, device="cuda")
    ticket = codec.DecompressI_async(frames[0], frame_buf)
    stands["prev"] = codec.PreviousFrame()
    in_flight = dl("an asynchronous frame is in flight (jsp_wait for it first)")
    refused("bad pair + in flight", pair(0, 1, 1), pairs=((1, 1),))
    refused("foreign index + in flight", dl("the index was built by another codec"), i=foreign._h)
    refused("in flight", in_flight)
    refused("in flight + too-small cap", in_flight, cap=1)
    codec.wait(ticket)

    # ---- and the call that is not refused works after all that --------------------------------------------------------------------
    assert idx.DeltaFrames([(0, 2), (2, 3)]) == first and info() == before
    for x in (idx, foreign, tiny_idx):
        x.close()
    for c in (codec, other, wrong, tiny):
        c.StopAndClean()


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
