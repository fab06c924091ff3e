"""TIGHT inter frames that span a gap of an MSVideo1 seek index (jsp_index_tight_frames / SeekIndex.DeltaFrames(pairs, tight=True)) on an
MI355X: a block that the gap codes but whose 16 pixels it does not change is dropped.

Truth: tests/index_tight_ref.py, the rule in plain Python, which test_index_tight_ref_cpu.py pins to the oracle — nothing of it comes
from the GPU (its block pixels here are cut out of the oracle's whole pictures, worked out once per clip).  Every case compares BYTES,
exactly, through the C call and through the Python method, and refusals against the reference's verdicts.  The directed clips
(tests/msv1_tight_clips.py) put dropped blocks next to kept ones on the seams of the kernel's lanes (4 blocks), waves (256), workgroups
(1024) and of the skip word's count (multiples of 1023)."""
import ctypes as C

import numpy as np
import pytest

import index_delta_ref as dr
import index_tight_ref as tr
import msv1_delta_clips as dc
import msv1_keyframe_cut_clips as kc
import msv1_tight_clips as tc
import test_index_delta_gpu as base
from jsplayer_amd import CodecError, ScreenPressor
from jsplayer_amd import _native as N
from msv1_range_clips import POISON, dev_buf, make_gpu, palette, truth_run
from test_index_delta_gpu import FILL, covered

pytestmark = pytest.mark.gpu

_pixels = {}   # the reference's block pixels, worked out once per clip and start


class Case(base.Case):
    """test_index_delta_gpu.Case with the tight call and the tight reference: `want` is Tight's answer, `delta_want` Delta's."""

    def __init__(self, name, bits, w, h, frames, keys, start=0, chunk=None, lines=36, pal=None):
        super().__init__(name, bits, w, h, frames, keys, start, chunk, lines)
        if pal is not None:   # (a palette of the clip's own: the codec and the index are built again with it)
            self.close()
            self.pal = pal
            self.gpu = make_gpu(bits, w, h, pal, lines, chunk, base.PARSE)
            self.pool = [dev_buf(w * h) for _ in range(3)]
            base.sequential(self.gpu, frames, keys, start, self.pool)
            self.idx = self.gpu.BuildIndex(self.range, self.range_keys)
        key = (name, bits, start)
        if key not in _pixels:
            truth = truth_run(bits, w, h, self.pal, frames, keys, lines, key_row=lines)
            before = truth[start - 1][0] if start > 0 else None
            _pixels[key] = (tr.Pixels(bits, w, h, self.range, self.codes, self.pal, before, [t[0] for t in truth[start:]]), {})
        self.px, self.tight_answers = _pixels[key]

    delta_want = base.Case.want

    def want(self, a, b):
        if (a, b) not in self.tight_answers:
            self.tight_answers[(a, b)] = tr.tight(self.px, a, b)
        return self.tight_answers[(a, b)]

    def raw(self, pairs, cap=None, room=None, fn=None):
        n = len(pairs)
        room = n * self.bound if room is None else room
        out = np.full(room + 16, FILL, dtype=np.uint8)
        frm, to = (C.c_int * n)(*[a for a, _ in pairs]), (C.c_int * n)(*[b for _, b in pairs])
        lens, total = (C.c_size_t * n)(*([12345] * n)), C.c_size_t(12345)
        fn = fn or N.lib().jsp_index_tight_frames
        rc = fn(self.gpu._h, self.idx._h, n, frm, to, C.c_void_p(out.ctypes.data), room if cap is None else cap, lens, C.byref(total))
        return rc, list(lens), total.value, out

    def check(self, pairs, python=True):
        wants = [self.want(a, b) for a, b in pairs]
        prev = self.gpu.PreviousFrame()
        kept_before = [b.clone() for b in self.pool]
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
                assert self.idx.DeltaFrames(pairs, tight=True) == wants, self.where
        else:
            (a, b), blk = pairs[bad], wants[bad][1]
            err = N.last_error()
            assert rc != 0 and lens == [0] * len(pairs) and total == 0, self.where
            assert err.startswith("index_tight:") and f"pair {bad} ({a}, {b}]" in err and "cut off" in err, (self.where, err)
            assert f"block {blk} in frame {dr.writer(self.codes, a, b, blk)}," in err, (self.where, err)
            assert np.all(out == FILL), self.where + ": written on a refusal"
            if python:
                with pytest.raises(CodecError, match=f"index_tight: .*block {blk} in frame"):
                    self.idx.DeltaFrames(pairs, tight=True)
        assert self.gpu.PreviousFrame() is prev, self.where
        assert all(bool((x == y).all()) for x, y in zip(self.pool, kept_before)), self.where + ": a frame buffer changed"
        return wants

    def check_delta(self, pairs):
        """jsp_index_delta_frames on the same index: index_delta_ref's bytes (the scratch is shared with the tight call)."""
        wants = [self.delta_want(a, b) for a, b in pairs]
        assert all(isinstance(x, bytes) for x in wants)
        rc, lens, total, out = self.raw(pairs, fn=N.lib().jsp_index_delta_frames)
        assert rc == 0 and lens == [len(x) for x in wants] and out[:total].tobytes() == b"".join(wants), self.where
        assert self.idx.DeltaFrames(pairs) == wants == self.idx.DeltaFrames(pairs, tight=False), self.where


def directed_case(bits, size, **kw):
    clip = tc.directed(bits, *size)
    return Case(clip.name, bits, clip.w, clip.h, clip.frames, clip.keys, **kw), clip


@pytest.mark.parametrize("bits", [16, 8])
@pytest.mark.parametrize("size", tc.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_every_pair_of_the_directed_clips_in_one_call_and_alone(bits, size):
    c, clip = directed_case(bits, size)
    pairs = dc.pairs(c.n)
    wants = c.check(pairs)                                  # frame j starts wherever the frames before it end: unaligned bases
    assert all(isinstance(x, bytes) for x in wants)
    for f in range(1, c.n):                                 # n pairs in one call equal n calls: each pattern alone
        c.check([(f - 1, f)], python=False)
    for p in ((1, 4), (2, 4), (4, 6), (-1, c.n - 1)):
        c.check([p], python=False)
    # the exact values: gaps that change no pixel, a gap that changes every block
    words = -(-c.nb // 1023)
    assert len(c.want(0, 1)) == len(c.want(5, 6)) == 2 * words and len(c.delta_want(0, 1)) == len(clip.frames[1])
    assert c.want(6, 7) == clip.frames[7] and c.gpu.IsKeyFrame(c.want(6, 7)) and not c.gpu.IsKeyFrame(c.want(5, 6))
    assert c.want(-1, 7) == c.idx.KeyFrame(7)
    assert all(len(c.want(a, b)) <= len(c.delta_want(a, b)) for a, b in pairs)
    # and Delta is still Delta after the tight calls have used the scratch both share
    delta_pairs = [p for p in pairs if p[1] - p[0] <= 2]
    c.check_delta(delta_pairs)
    c.check(delta_pairs, python=False)
    c.close()


@pytest.mark.parametrize("bits", [16, 8])
@pytest.mark.parametrize("size", [(164, 100), (128, 256)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_a_chunked_index_and_one_behind_decoded_frames_give_the_references_bytes(bits, size):
    """msv1_seek_chunk_frames = 3: the writers on both sides of a gap lie in other chunks than b.  start = 3: the codec decoded
    frames 0 .. 2 one by one, the index starts behind them, and a = -1 compares against the picture they left."""
    c, _ = directed_case(bits, size, chunk=3)
    c.check(dc.pairs(c.n))
    c.close()
    c, clip = directed_case(bits, size, start=3)
    wants = c.check(dc.pairs(c.n))
    # (-1, 1]: frames 3 and 4 of the clip against the picture of frame 2 — the blocks frame 3 recoded unchanged are dropped
    assert len(c.want(-1, 1)) < len(c.delta_want(-1, 1)) and len(c.want(-1, 0)) < len(c.delta_want(-1, 0))
    c.close()
    c, _ = directed_case(bits, size, start=3, chunk=2)
    c.check(dc.pairs(c.n), python=False)
    c.close()


@pytest.mark.parametrize("bits", [16, 8])
def test_the_slice_size_does_not_change_the_bytes(bits):
    c, _ = directed_case(bits, (164, 100))
    pairs = dc.pairs(c.n)[:23]
    rc, lens, total, auto = c.raw(pairs)
    assert rc == 0, N.last_error()
    for s in ("1", "2", "3", "23", "auto"):
        c.gpu.set_option("msv1_index_delta_slice", s)
        rc, lens2, total2, out = c.raw(pairs)
        assert rc == 0 and lens2 == lens and total2 == total and np.array_equal(out, auto), s
        c.check(pairs[:7], python=False)
    c.close()


@pytest.mark.parametrize("bits", [16, 8])
def test_cap_lens_and_total(bits):
    c, clip = directed_case(bits, (128, 128))
    pairs = [(-1, 0), (0, 1), (1, 4), (2, 3), (0, 5)]
    wants = [c.want(a, b) for a, b in pairs]
    lens, total = [len(x) for x in wants], sum(len(x) for x in wants)
    for cap in (total - 1, total - 2, 1, 0):                 # too small: refused, lens and *total still set, nothing written
        rc, got_lens, got_total, out = c.raw(pairs, cap=cap)
        assert rc != 0 and got_lens == lens and got_total == total and np.all(out == FILL), cap
        assert N.last_error().startswith("index_tight: cap is smaller")
    n = len(pairs)
    frm, to = (C.c_int * n)(*[a for a, _ in pairs]), (C.c_int * n)(*[b for _, b in pairs])
    l2, t2 = (C.c_size_t * n)(), C.c_size_t(0)
    assert N.lib().jsp_index_tight_frames(c.gpu._h, c.idx._h, n, frm, to, None, 0, l2, C.byref(t2)) != 0      # asking for the lengths
    assert list(l2) == lens and t2.value == total
    rc, got_lens, got_total, out = c.raw(pairs, cap=total, room=total)                                           # exactly the length
    assert rc == 0 and got_lens == lens and out[:total].tobytes() == b"".join(wants) and np.all(out[total:] == FILL)
    c.close()


def test_two_palette_indices_of_one_colour_are_equal():
    clip, pal = tc.twins()
    c = Case(clip.name, 8, clip.w, clip.h, clip.frames, clip.keys, pal=pal)
    wants = c.check(dc.pairs(c.n))
    assert c.want(1, 2) == dr.skip_word(c.nb) and len(c.want(0, 1)) == 2 + 2 + 2   # (skip 4, block 4's code, skip 1)
    c.close()


@pytest.mark.parametrize("bits", [16, 8])
@pytest.mark.parametrize("size", tc.CUT_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_a_dropped_block_with_a_cut_code_is_not_refused(bits, size):
    clip = tc.cut_dropped(bits, *size)
    c = Case(clip.name, bits, clip.w, clip.h, clip.frames, clip.keys)
    assert c.delta_want(0, 1) == ("cut", clip.last) and isinstance(c.want(0, 1), bytes) and isinstance(c.want(0, 2), bytes)
    assert c.want(-1, 1) == ("cut", clip.last)              # nothing defined before the index: kept, and refused
    c.check([(0, 1), (0, 2), (1, 2)])
    c.check([(0, 1), (-1, 1), (0, 2)])
    c.check([(0, 2)])
    rc, lens, total, out = c.raw([(0, 1)], fn=N.lib().jsp_index_delta_frames)   # Delta refuses the pair Tight makes
    assert rc != 0 and N.last_error().startswith("index_delta:") and f"block {clip.last} in frame 1," in N.last_error()
    c.close()


@pytest.mark.parametrize("bits", [16, 8])
def test_the_first_refusing_pair_and_block_is_named_and_nothing_is_written(bits):
    """msv1_keyframe_cut_clips.firsts_cut (see test_index_delta_gpu): frame 4i + 1 is cut one byte short of the end of block P7[i]'s
    code, and every block behind it is painted from missing bytes — kept, and cut."""
    clip = dc.cuts(bits)
    c = Case(clip.name, bits, clip.w, clip.h, clip.frames, clip.keys)
    ok = [(-1, 0), (0, 3), (4, 7), (11, 12)]
    assert all(isinstance(c.want(a, b), bytes) for a, b in ok)
    assert c.want(4, 5) == ("cut", 3) and c.want(8, 10) == ("cut", 4) and c.want(3, 5) == ("cut", 3) and c.want(20, 21) == ("cut", 1023)
    for s in ("auto", "1", "2"):
        c.gpu.set_option("msv1_index_delta_slice", s)
        c.check([ok[0], (4, 5), ok[1]])                     # a cut in pair 1, uncut pairs before and after it
        c.check([ok[1], (8, 10), (4, 5), ok[0]])            # two cuts: pair 1 (block 4, frame 9) is named, not pair 2's block 3
        c.check([(20, 21), ok[2], (3, 5)])                  # pair 0, in the workgroup's last lane
        c.check([ok[2], ok[3], ok[0], (3, 5)])              # the last pair of the call
        c.check(ok)                                         # ... and the call works after the refusals
    c.close()


@pytest.mark.parametrize("bits", [16, 8])
def test_the_firsts_family_is_refused_where_the_reference_refuses(bits):
    refusals = 0
    clips = kc.family("firsts", bits)
    assert [x.name for x in clips[8:]] == [f"pair_at_{p}" for p in kc.PAIRS]
    for clip in (clips[1], clips[8], clips[10], clips[12]):     # none_at_0; "no writer" next to "cut" at the lane, wave, workgroup seams
        for start in clip.starts:
            c = Case(clip.name, bits, clip.w, clip.h, clip.frames, clip.keys, start=start)
            pairs = dc.pairs(c.n)
            good = [p for p in pairs if isinstance(c.want(*p), bytes)]
            bad = [p for p in pairs if p not in good]
            refusals += len(bad)
            c.check(good, python=False)
            for p in bad[:2]:
                c.check([good[0], p], python=False)
            c.close()
    assert refusals > 0


@pytest.mark.parametrize("bits", [16, 8])
def test_round_trip_through_the_gpu_codec(bits):
    """A fresh codec decodes KeyFrame(t0) as a key frame and the tight frames of a stride as inter frames on top: each picture is
    Show's."""
    c, clip = directed_case(bits, (164, 100))
    for t0, stride in ((0, 1), (1, 3), (0, 4), (2, 2)):
        ts = list(range(t0, c.n, stride))
        frames = [c.idx.KeyFrame(t0)] + c.idx.DeltaFrames(list(zip(ts, ts[1:])), tight=True)
        fresh = make_gpu(bits, c.w, c.h, c.pal, parse=base.PARSE)
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
            assert np.array_equal(covered(fresh.PreviousFrame().cpu().numpy(), c.w, c.h), covered(shown.cpu().numpy(), c.w, c.h)), \
                f"{c.where}: frame {t} of the stride {stride} from {t0}"
        fresh.StopAndClean()
    c.close()


def test_every_argument_refusal_and_their_order():
    import torch
    W, H = 40, 24
    from jsplayer_amd import streamgen as sg
    frames, keys, _ = sg.msv1_clip(41, W, H, 6, bits=16, p_mix=sg.msv1_p_mix(0.6, 3.0))
    codec, other = make_gpu(16, W, H, parse=base.PARSE), make_gpu(16, W, H, parse=base.PARSE)
    idx, foreign = codec.BuildIndex(frames, keys), other.BuildIndex(frames, keys)
    wrong = ScreenPressor(W, H, 24)
    tiny = make_gpu(16, 3, 8, parse=base.PARSE)                  # a picture without a 4x4 block
    tiny_idx = tiny.BuildIndex([b"\x01\x02\x03\x04", b""], [True, False])
    lib = N.lib()
    fn, n = lib.jsp_index_tight_frames, idx.frames
    bound = idx.DeltaBound()
    first = idx.DeltaFrames([(0, 2), (2, 3)], tight=True)        # (the scratch is allocated here: from now on nothing may grow)
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
        print(f"jsp_index_tight_frames: {what}: {err}")
        assert rc != 0 and err == message, (what, err)
        assert size.value == (0 if total else 777) and np.all(out == FILL), what
        assert list(ls) == ([0] * k if lens and 1 <= count <= 4096 else [777] * k), what
        assert info() == before and codec.PreviousFrame() is stands["prev"], what

    def tl(what):
        return "index_tight: " + what

    def pair(j, a, b, of=n):
        return tl(f"pair {j} ({a}, {b}] is not a gap of the index (-1 <= from < to < {of} frames)")

    # ---- each refusal alone --------------------------------------------------------------------------------------------------
    refused("null codec", tl("null argument"), c=None)
    refused("null index", tl("null argument"), i=None)
    refused("null from", tl("null argument"), frm=False)
    refused("null to", tl("null argument"), to=False)
    refused("null out with a cap", tl("null argument"), dst=None)
    refused("null lens", tl("null argument"), lens=False)
    refused("null total", tl("null argument"), total=False)
    refused("wrong codec kind", "index: MSVideo1 only", c=wrong._h)
    refused("foreign index", tl("the index was built by another codec"), i=foreign._h)
    for bad in (0, -1, 4097):
        refused(f"n = {bad}", tl("n is outside 1..4096"), count=bad)
    refused("from < -1", pair(1, -2, 3), pairs=((0, 1), (-2, 3)))
    refused("to == from", pair(0, 2, 2), pairs=((2, 2), (0, 1)))
    refused("to < from", pair(1, 3, 1), pairs=((0, 1), (3, 1)))
    refused("to == nframes", pair(0, 0, n), pairs=((0, n),))
    refused("the first bad pair is named", pair(1, 4, 4), pairs=((0, 1), (4, 4), (-5, 2)))
    refused("no block", tl("the picture has no 4x4 block"), c=tiny._h, i=tiny_idx._h, pairs=((0, 1),))

    # ---- the earlier refusal wins ---------------------------------------------------------------------------------------------
    refused("wrong codec kind + foreign index + bad n", "index: MSVideo1 only", c=wrong._h, i=foreign._h, count=0)
    refused("foreign index + bad n", tl("the index was built by another codec"), i=foreign._h, count=0)
    refused("bad n + bad pair", tl("n is outside 1..4096"), pairs=((3, 1),), count=0)
    refused("bad pair + no block", pair(0, 0, 2, of=2), c=tiny._h, i=tiny_idx._h, pairs=((0, 2),))
    frame_buf = torch.zeros(W * H, dtype=torch.int32, device="cuda")
    ticket = codec.DecompressI_async(frames[0], frame_buf)
    stands["prev"] = codec.PreviousFrame()
    in_flight = tl("an asynchronous frame is in flight (jsp_wait for it first)")
    refused("bad pair + in flight", pair(0, 1, 1), pairs=((1, 1),))
    refused("foreign index + in flight", tl("the index was built by another codec"), i=foreign._h)
    refused("in flight", in_flight)
    refused("in flight + too-small cap", in_flight, cap=1)
    codec.wait(ticket)

    # ---- and the call that is not refused works after all that --------------------------------------------------------------------
    assert idx.DeltaFrames([(0, 2), (2, 3)], tight=True) == first and info() == before
    for x in (idx, foreign, tiny_idx):
        x.close()
    for c in (codec, other, wrong, tiny):
        c.StopAndClean()


class TestOnGpuParse:
    """Every test of this file once more with the block tables of the on-GPU parse — the codec's default (the tests above keep the
    host parser and their names)."""

    @pytest.fixture(autouse=True)
    def parse_mode(self):
        base.PARSE = "gpu"
        yield base.PARSE
        base.PARSE = "host"


for _name, _test in list(globals().items()):
    if _name.startswith("test_"):
        setattr(TestOnGpuParse, _name, staticmethod(_test))
