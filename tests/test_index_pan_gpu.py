"""The frames of a block rectangle that moves over an MSVideo1 seek index (jsp_index_pan_frames / SeekIndex.PanFrames) on an MI355X.

Truth: tests/index_pan_ref.py, the rule in plain Python, which test_index_pan_ref_cpu.py pins to the oracle — nothing of it comes from
the GPU; that file also shows that every moved tight pair asked for here drops a block and keeps a block unless its clip names it
otherwise.  Every case compares BYTES, exactly, through the C call and through the Python method, keys[], lens and total against the
reference, and refusals against the reference's verdicts.  The clips (tests/msv1_pan_clips.py) are one source picture of 48 x 48
blocks under rectangles of 1023, 1024, 1025 and 6 blocks."""
import ctypes as C
import hashlib

import numpy as np
import pytest

import index_crop_ref as cr
import index_pan_ref as pr
import msv1_crop_clips as cc
import msv1_pan_clips as pc
from jsplayer_amd import CodecError, ScreenPressor
from jsplayer_amd import _native as N
from msv1_range_clips import POISON, dev_buf, make_gpu
from test_index_crop_ref_cpu import source as crop_source
from test_index_delta_gpu import sequential
from test_index_pan_ref_cpu import source

pytestmark = pytest.mark.gpu

FILL = 0xA5      # what `out` holds before a call
PARSE = "host"   # the msv1_parse of every codec built here; TestOnGpuParse (the end of this file) runs the tests with "gpu" too
KEY = pr.KEY


def what(pair):
    k = pr.kind(pair)
    return f"(key, {pair[1]})" if k == "key" else f"({pair[0]}, {pair[1]}]" if k == "still" else f"({pair[0]} -> {pair[1]}, moved)"


def xy(pairs, k):
    """from_xy / to_xy of a call: a key pair's origin at `from` is not read."""
    flat = [v for p in pairs for v in (p[k] if p[k] is not None else p[3])]
    return (C.c_int * len(flat))(*flat)


class Case:
    """A codec brought to the first frame of a clip's index frame by frame, the index over the frames from there on, and the
    reference's answers (`want(pair, tight)`: worked out once per clip)."""

    def __init__(self, clip, want, n, frames, pal, start=0, chunk=None):
        self.bits, self.pal, self.n, self.want = clip.bits, pal, n, want
        self.gpu = make_gpu(self.bits, pc.W, pc.H, pal, 36, chunk, PARSE)
        self.pool = [dev_buf(pc.W * pc.H) for _ in range(3)]
        sequential(self.gpu, clip.frames, clip.keys, start, self.pool)
        self.idx = self.gpu.BuildIndex(frames, clip.keys[start:])
        assert self.idx.frames == n
        self.where = f"{clip.name} {self.bits}-bit start={start} chunk={chunk} ({PARSE} parse)"

    @classmethod
    def of(cls, clip, chunk=None):
        s = source(clip)
        c = cls(clip, s.pan, s.n, s.range, s.pal, s.start, chunk)
        c.s = s
        return c

    def digest(self):
        h = hashlib.sha1()
        for b in self.pool:
            h.update(b.cpu().numpy().tobytes())
        return h.hexdigest(), self.gpu.PreviousFrame()

    def raw(self, size, pairs, tight=False, cap=None, room=None, keys=True, from_xy=True):
        """The C call into a host array of FILL: (rc, lens, keys, total, the array — 16 bytes longer than `room`)."""
        n = len(pairs)
        bound = self.idx.CropBound(*size)
        assert bound == size[0] * size[1] * (18 if self.bits == 16 else 10)
        room = n * bound if room is None else room
        out = np.full(room + 16, FILL, dtype=np.uint8)
        frm, to = (C.c_int * n)(*[p[0] for p in pairs]), (C.c_int * n)(*[p[1] for p in pairs])
        lens, ks, total = (C.c_size_t * n)(*([12345] * n)), (C.c_int * n)(*([77] * n)), C.c_size_t(12345)
        rc = N.lib().jsp_index_pan_frames(self.gpu._h, self.idx._h, size[0], size[1], n, frm, to, xy(pairs, 2) if from_xy else None, xy(pairs, 3),
                                          1 if tight else 0, C.c_void_p(out.ctypes.data), room if cap is None else cap, lens,
                                          ks if keys else None, C.byref(total))
        return rc, list(lens), list(ks), total.value, out

    def check(self, size, pairs, tight=False, python=True):
        """One call for `pairs` against the reference: every frame's bytes back to back and its flag, or the first refusal in
        (pair, block) order.  Returns the reference's answers."""
        wants = [self.want(p, tight) for p in pairs]
        nb = size[0] * size[1]
        before = self.digest()
        rc, lens, keys, total, out = self.raw(size, pairs, tight)
        bad = next((j for j, x in enumerate(wants) if not isinstance(x, bytes)), None)
        where = f"{self.where} {size} tight={tight}"
        if bad is None:
            assert rc == 0, where + ": " + N.last_error()
            assert lens == [len(x) for x in wants] and total == sum(lens), where
            got, at = out[:total].tobytes(), 0
            for p, x in zip(pairs, wants):
                assert got[at:at + len(x)] == x, f"{where} pair {p} at byte {at} of the call"
                at += len(x)
            assert np.all(out[total:] == FILL), where + ": written behind the frames"
            flags = [pr.flag(self.bits, x, nb) for x in wants]
            assert keys == [int(f) for f in flags], where
            assert all(flags[j] for j, p in enumerate(pairs) if p[0] == KEY or (pr.kind(p) == "moved" and not tight)), where
            if python:
                assert self.idx.PanFrames(size, pairs, tight=tight) == (wants, flags), where
        else:
            pair, (kind, j) = pairs[bad], wants[bad]
            err = N.last_error()
            assert rc != 0 and lens == [0] * len(pairs) and keys == [0] * len(pairs) and total == 0, where
            assert err.startswith(f"index_pan: pair {bad} {what(pair)}: "), (where, err)
            blocks = f"block {j} of the rectangle (block {cr.src(pc.NBX, pr.rect_of(size, pair[3]), j)} of the picture)"
            if kind == "none":
                assert f": {blocks} has no writer up to frame {pair[1]} " in err, (where, err)
            else:
                assert f"the code of {blocks} in frame {pr.writer(self.s.codes, pc.NBX, size, pair, j)}," in err and "cut off" in err, (where, err)
            assert np.all(out == FILL), where + ": written on a refusal"
            if python:
                with pytest.raises(CodecError, match=f"index_pan: pair {bad} .*block {j} of the rectangle"):
                    self.idx.PanFrames(size, pairs, tight=tight)
        assert self.digest() == before, where + ": a frame buffer or the codec's previous frame changed"
        return wants

    def close(self):
        self.idx.close()
        self.gpu.StopAndClean()


@pytest.mark.parametrize("bits", [16, 8])
@pytest.mark.parametrize("size", pc.SIZES, ids=pc.size_id)
def test_scroll_clips_followed_lagging_and_against(bits, size):
    for how in pc.HOWS:
        clip = pc.scroll(bits, size, how)
        c = Case.of(clip)
        wants = c.check(size, clip.pairs, tight=True)
        assert all(isinstance(x, bytes) for x in wants)
        loose = c.check(size, clip.pairs)                         # a moved pair without tight: the key pair of its rectangle, keys = 1
        for p, x, y in zip(clip.pairs, wants, loose):
            assert len(x) <= len(y), (clip.name, p)
            if pr.kind(p) == "moved":
                assert y == c.want((KEY, p[1], None, p[3]), False)
        for s in ("1", "2"):
            c.gpu.set_option("msv1_index_delta_slice", s)
            c.check(size, clip.pairs, tight=True, python=False)
        for p in clip.pairs[1:3]:                                 # n pairs in one call equal n calls
            c.check(size, [p], tight=True, python=False)
        c.close()
    c = Case.of(pc.scroll(bits, size, "lag"), chunk=2)            # the writers of srcA and srcB lie in different chunks of the index
    c.check(size, c.s.clip.pairs, tight=True, python=False)
    c.close()


@pytest.mark.parametrize("bits", [16, 8])
@pytest.mark.parametrize("size", pc.SIZES, ids=pc.size_id)
def test_the_kept_dropped_boundary_on_every_seam(bits, size):
    clip = pc.bounds(bits, size)
    c = Case.of(clip)
    wants = c.check(size, clip.pairs, tight=True)                 # frame j starts wherever the frames before it end: unaligned bases
    assert all(isinstance(x, bytes) for x in wants)
    c.check(size, clip.pairs)
    for s in ("1", "3", "auto"):
        c.gpu.set_option("msv1_index_delta_slice", s)
        c.check(size, clip.pairs, tight=True, python=False)
    c.close()
    c = Case.of(clip, chunk=cc.kc.CHUNK)
    c.check(size, clip.pairs, tight=True, python=False)
    c.close()


@pytest.mark.parametrize("bits", [16, 8])
def test_refusals_the_first_pair_and_block_wins_and_dropped_blocks_never_refuse(bits):
    clip = pc.cuts(bits)
    c = Case.of(clip)
    size = clip.size
    painted, across, whole = clip.pairs[:2], clip.pairs[2:5], clip.pairs[5]
    assert all(c.want(p, True) == ("cut", 1) for p in across) and all(isinstance(c.want(p, True), bytes) for p in painted + [whole])
    for s in ("auto", "1", "2"):
        c.gpu.set_option("msv1_index_delta_slice", s)
        c.check(size, painted + [whole], tight=True, python=s == "auto")   # dropped blocks with cut codes do not refuse
        for p in across:
            c.check(size, [painted[0], p, whole], tight=True, python=s == "auto")
        c.check(size, [whole, across[1], painted[1], across[0]], tight=True, python=False)   # two refusals: the first PAIR is named
        c.check(size, painted + [whole] + [across[2]], tight=True, python=False)              # the last pair of the call
        c.check(size, [whole, painted[0]], python=False)          # without tight the painted rectangle is a key pair: block 0 is cut
        c.check(size, painted + [whole], tight=True, python=False)   # ... and the call works after the refusals
    assert c.want(painted[0], False) == ("cut", 0)
    c.close()
    clip = pc.befores(bits)
    size = clip.size
    for chunk in (None, 2):
        c = Case.of(clip, chunk=chunk)
        flat, patch, rest = clip.pairs[:3], clip.pairs[3:6], clip.pairs[6:]
        assert all(c.want(p, True) == ("none", 0) for p in patch)
        wants = c.check(size, flat + rest, tight=True, python=chunk is None)
        assert all(isinstance(x, bytes) for x in wants) and all(x == pr.dr.skip_word(18) for x in wants[:3])
        for p in patch:
            c.check(size, [flat[0], p, rest[0]], tight=True, python=chunk is None)
            c.check(size, [p], python=False)                      # (without tight: the key pair refuses at the same block)
        c.gpu.set_option("msv1_index_delta_slice", "1")
        c.check(size, rest + [patch[2], patch[0]], tight=True, python=False)
        c.close()


@pytest.mark.parametrize("bits", [16, 8])
def test_a_rectangle_that_stands_gives_the_crop_references_bytes(bits):
    for rect in ((5, 3, 37, 31), (1, 1, 46, 45)):
        clip = cc.seams(bits, rect)
        s = crop_source(clip)
        size, origin = rect[2:], rect[:2]
        c = Case(clip, lambda p, tight: s.crop(rect, (p[0], p[1]), tight), s.n, s.range, s.pal)
        pairs = [(a, b, origin, origin) for a, b in cc.pairs(s.n)]
        wants = c.check(size, pairs)
        assert all(isinstance(x, bytes) for x in wants)
        assert c.idx.CropFrames(rect, [p[:2] for p in pairs]) == c.idx.PanFrames(size, pairs)
        close = [p for p in pairs if p[1] - p[0] == 1 or p[0] == KEY]
        c.check(size, close, tight=True)
        keys_only = [p for p in pairs if p[0] == KEY]
        rc, lens, keys, total, out = c.raw(size, keys_only, from_xy=False)     # from_xy may be null when every pair is a key pair
        assert rc == 0 and out[:total].tobytes() == b"".join(s.crop(rect, p[:2]) for p in keys_only) and keys == [1] * len(keys_only)
        c.gpu.set_option("msv1_index_delta_slice", "2")
        c.check(size, pairs, python=False)
        c.close()


@pytest.mark.parametrize("bits", [16, 8])
def test_cap_lens_keys_and_total(bits):
    size = (41, 25)
    clip = pc.bounds(bits, size)
    c = Case.of(clip)
    pairs = clip.pairs[:6]
    wants = [c.want(p, True) for p in pairs]
    lens, total = [len(x) for x in wants], sum(len(x) for x in wants)
    keys = [int(pr.flag(bits, x, size[0] * size[1])) for x in wants]
    assert 0 in keys and 1 in keys
    for cap in (total - 1, total - 2, 1, 0):                  # too small: refused, lens, keys and *total still set, nothing written
        rc, got_lens, got_keys, got_total, out = c.raw(size, pairs, tight=True, cap=cap)
        assert rc != 0 and got_lens == lens and got_keys == keys and got_total == total and np.all(out == FILL), cap
        assert N.last_error().startswith("index_pan: cap is smaller")
    rc, got_lens, got_keys, got_total, out = c.raw(size, pairs, tight=True, cap=total, room=total, keys=False)
    assert rc == 0 and got_lens == lens and got_keys == [77] * len(pairs) and np.all(out[total:] == FILL)
    assert out[:total].tobytes() == b"".join(wants)
    c.close()


@pytest.mark.parametrize("bits", [16, 8])
def test_a_codec_of_the_rectangles_size_decodes_the_panned_clip_on_the_gpu(bits):
    """A fresh codec of 4 bw x 4 bh pixels decodes the key pair's frame and the chained pairs' frames: each picture is rectangle B
    of Show(to)."""
    size = (33, 31)
    bw, bh = size
    for clip in (pc.scroll(bits, size, "lag"), pc.bounds(bits, size)):
        c = Case.of(clip)
        shown = dev_buf(pc.W * pc.H)
        chain = clip.pairs[:clip.chain]
        frames, flags = c.idx.PanFrames(size, chain, tight=True)
        fresh = make_gpu(bits, 4 * bw, 4 * bh, c.pal, parse=PARSE)
        pool = [dev_buf(16 * bw * bh) for _ in range(2)]
        for k, (pair, data) in enumerate(zip(chain, frames)):
            prev = fresh.PreviousFrame()
            dst = next(b for b in pool if b is not prev)
            assert bool(fresh.IsKeyFrame(data)) == flags[k]
            if k == 0:
                assert fresh.DecompressI(data, dst) == 0
            else:
                dst.copy_(prev)
                fresh.DecompressP(data, dst)
            shown.fill_(POISON)
            c.idx.Show(pair[1], shown, adopt=False)
            bx, by = pair[3]
            want = shown.cpu().numpy().reshape(pc.H, pc.W)[4 * by:4 * by + 4 * bh, 4 * bx:4 * bx + 4 * bw]
            got = fresh.PreviousFrame().cpu().numpy().reshape(4 * bh, 4 * bw)
            assert np.array_equal(got, want), f"{c.where}: pair {pair}"
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
    fn, n = lib.jsp_index_pan_frames, idx.frames
    good = ((KEY, 0, None, (2, 1)), (0, 2, (2, 1), (3, 1)))
    size = (5, 4)
    bound = idx.CropBound(*size)

    def info():
        k, d, h = C.c_int(0), C.c_uint64(0), C.c_uint64(0)
        assert lib.jsp_index_info(idx._h, C.byref(k), C.byref(d), C.byref(h)) == 0
        return k.value, d.value, h.value

    at_build = info()
    first = idx.PanFrames(size, good, tight=True)                # (the scratch is allocated here: from now on nothing may grow)
    # jsp_index_info counts the scratch: records of 2 pairs x 20 blocks and the frames at their bound on the device, the pinned side
    assert info()[0] == at_build[0] and info()[1] >= at_build[1] + 2 * 20 * 8 + 2 * bound and info()[2] > at_build[2]
    assert (idx.device_bytes, idx.host_bytes) == info()[1:]
    out = np.full(2 * bound, FILL, dtype=np.uint8)
    stands = {"prev": codec.PreviousFrame()}
    before = info()

    def refused(what, message, c=codec._h, i=idx._h, size=size, pairs=good, count=None, flags=0, dst=out.ctypes.data, cap=2 * bound,
                lens=True, total=True, frm=True, to=True, fxy=True, txy=True):
        k = len(pairs)
        a, b = (C.c_int * k)(*[p[0] for p in pairs]), (C.c_int * k)(*[p[1] for p in pairs])
        ls, ks, sz = (C.c_size_t * k)(*([777] * k)), (C.c_int * k)(*([777] * k)), C.c_size_t(777)
        count = k if count is None else count
        rc = fn(c, i, size[0], size[1], count, a if frm else None, b if to else None, xy(pairs, 2) if fxy else None, xy(pairs, 3) if txy else None,
                flags, C.c_void_p(dst) if dst else None, cap, ls if lens else None, ks, C.byref(sz) if total else None)
        err = N.last_error()
        print(f"jsp_index_pan_frames: {what}: {err}")
        assert rc != 0 and err == message, (what, err)
        assert sz.value == (0 if total else 777) and np.all(out == FILL), what
        zeroed = 1 <= count <= 4096
        assert list(ls) == ([0] * k if lens and zeroed else [777] * k) and list(ks) == ([0] * k if zeroed else [777] * k), what
        assert info() == before and codec.PreviousFrame() is stands["prev"], what

    def tl(what):
        return "index_pan: " + what

    def pair(j, a, b, of=n):
        return tl(f"pair {j} ({a}, {b}) is neither a gap of the index (-1 <= from < to < {of} frames; from <= to where the rectangle moves) "
                  f"nor a key pair (from = -2, 0 <= to)")

    def origin(j, a, b, which, o, sz=size, nbx=W // 4, nby=H // 4):
        return tl(f"pair {j} ({a}, {b}): the rectangle at `{which}` ({o[0]}, {o[1]}, {sz[0]} x {sz[1]} blocks) is outside the block grid "
                  f"({nbx} x {nby} blocks)")

    def grid(sz, nbx=W // 4, nby=H // 4):
        return tl("the rectangle's size (%d x %d blocks) is outside the block grid (%d x %d blocks)" % (tuple(sz) + (nbx, nby)))

    # ---- each refusal alone --------------------------------------------------------------------------------------------------
    refused("null codec", tl("null argument"), c=None)
    refused("null index", tl("null argument"), i=None)
    refused("null from", tl("null argument"), frm=False)
    refused("null to", tl("null argument"), to=False)
    refused("null to_xy", tl("null argument"), txy=False)
    refused("null from_xy with a gap pair", tl("null argument"), fxy=False)
    refused("null out with a cap", tl("null argument"), dst=None)
    refused("null lens", tl("null argument"), lens=False)
    refused("null total", tl("null argument"), total=False)
    refused("wrong codec kind", "index: MSVideo1 only", c=wrong._h)
    refused("foreign index", tl("the index was built by another codec"), i=foreign._h)
    for bad in ((0, 3), (3, 0), (11, 1), (1, 7), (2 ** 31 - 1, 1), (-3, -3)):
        refused(f"size {bad}", grid(bad), size=bad)
    refused("no block", grid((1, 1), 0, 0), c=tiny._h, i=tiny_idx._h, size=(1, 1), pairs=((0, 1, (0, 0), (0, 0)),))
    for bad in (0, -1, 4097):
        refused(f"n = {bad}", tl("n is outside 1..4096"), count=bad)
    for bad in (2, 3, -1, 1 << 16):
        refused(f"flags = {bad}", tl("unknown flag bits"), flags=bad)
    o, m = (2, 1), (3, 1)
    refused("from < -2", pair(1, -3, 3), pairs=((0, 1, o, o), (-3, 3, o, o)))
    refused("to == from, still", pair(0, 2, 2), pairs=((2, 2, o, o), (0, 1, o, o)))
    refused("to < from, still", pair(1, 3, 1), pairs=((0, 1, o, o), (3, 1, o, o)))
    refused("to < from, moved", pair(1, 3, 1), pairs=((2, 2, o, m), (3, 1, o, m)))
    refused("to == nframes", pair(0, 0, n), pairs=((0, n, o, m),))
    refused("from == -1 == to, moved", pair(0, -1, -1), pairs=((-1, -1, o, m),))
    refused("a key pair at nframes", pair(0, KEY, n), pairs=((KEY, n, None, o),))
    refused("a key pair below 0", pair(1, KEY, -1), pairs=((KEY, 0, None, o), (KEY, -1, None, o)))
    for bad in ((-1, 0), (0, -1), (6, 0), (0, 3), (2 ** 31 - 1, 0)):
        refused(f"B = {bad}", origin(1, 0, 1, "to", bad), pairs=((KEY, 0, None, o), (0, 1, o, bad)))
        refused(f"A = {bad}", origin(1, 0, 1, "from", bad), pairs=((KEY, 0, None, o), (0, 1, bad, o)))
        refused(f"a key pair's B = {bad}", origin(0, KEY, 1, "to", bad), pairs=((KEY, 1, None, bad),))
    refused("bad frames before a bad origin", pair(0, 3, 1), pairs=((3, 1, (9, 9), (8, 8)),))
    refused("B before A", origin(0, 0, 1, "to", (8, 8)), pairs=((0, 1, (9, 9), (8, 8)),))
    refused("the first bad pair is named", pair(1, 4, 4), pairs=((0, 1, o, o), (4, 4, o, o), (-5, 2, o, o)))

    # ---- the earlier refusal wins ---------------------------------------------------------------------------------------------
    refused("wrong codec kind + foreign index + bad n", "index: MSVideo1 only", c=wrong._h, i=foreign._h, count=0)
    refused("foreign index + bad size", tl("the index was built by another codec"), i=foreign._h, size=(0, 0))
    refused("bad size + bad n", grid((11, 1)), size=(11, 1), count=0)
    refused("bad n + bad flags", tl("n is outside 1..4096"), count=0, flags=8)
    refused("bad flags + bad pair", tl("unknown flag bits"), flags=4, pairs=((3, 1, o, o),))
    frame_buf = torch.zeros(W * H, dtype=torch.int32, device="cuda")
    ticket = codec.DecompressI_async(frames[0], frame_buf)
    stands["prev"] = codec.PreviousFrame()
    in_flight = tl("an asynchronous frame is in flight (jsp_wait for it first)")
    refused("bad pair + in flight", pair(0, 1, 1), pairs=((1, 1, o, o),))
    refused("bad size + in flight", grid((11, 6)), size=(11, 6))
    refused("in flight", in_flight)
    refused("in flight + too-small cap", in_flight, cap=1)
    codec.wait(ticket)

    with pytest.raises(CodecError, match="index_pan: the rectangle's size"):
        idx.PanFrames((11, 1), [(KEY, 0, None, (0, 0))])

    # ---- and the call that is not refused works after all that --------------------------------------------------------------------
    assert idx.PanFrames(size, good, tight=True) == first and info() == before
    assert idx.PanFrames(size, [(2, 2, o, m)])[1] == [True]      # from == to on a moved pair
    for x in (idx, foreign, tiny_idx):
        x.close()
    for c in (codec, other, wrong, tiny):
        c.StopAndClean()


class TestOnGpuParse:
    """Every test of this file once more with the block tables of the on-GPU parse — the codec's default (the tests above keep the
    host parser and their names)."""

    @pytest.fixture(autouse=True)
    def parse_mode(self):
        global PARSE
        PARSE = "gpu"
        yield PARSE
        PARSE = "host"


for _name, _test in list(globals().items()):
    if _name.startswith("test_"):
        setattr(TestOnGpuParse, _name, staticmethod(_test))
