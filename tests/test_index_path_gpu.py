"""The frames of a block rectangle along any path through an MSVideo1 seek index (jsp_index_path_frames / SeekIndex.PathFrames) on an
MI355X: steps back, holds and steps forward in one call.

Truth: tests/index_path_ref.py, the rule in plain Python, which test_index_path_ref_cpu.py pins to the oracle — nothing of it comes from
the GPU.  Every case compares BYTES, exactly, through the C call and through the Python method, keys[] against the reference's flag,
and refusals against the reference's verdicts.  The clips are test_index_crop_gpu's (tests/msv1_crop_clips.py): one source picture of
48 x 48 blocks under rectangles that put the kernel's lanes (4 blocks OF THE RECTANGLE), waves (256), workgroups (1024) and the multiples
of 1023 against row starts of the rectangle."""
import ctypes as C

import numpy as np
import pytest

import index_crop_ref as cr
import index_path_ref as pr
import msv1_crop_clips as cc
import test_index_crop_gpu as crop_gpu
from jsplayer_amd import CodecError, ScreenPressor
from jsplayer_amd import _native as N
from msv1_range_clips import POISON, dev_buf, make_gpu
from test_index_path_ref_cpu import back_pairs, chains, hold_pairs, made

pytestmark = pytest.mark.gpu

FILL = crop_gpu.FILL
KEY = pr.KEY


def what(pair):
    a, b = pair
    return f"(key, {b})" if a == KEY else f"({a} -> {b}, back)" if a > b else f"({a}, {b}]"


def chained(order):
    """The pairs of an order of frames: the key pair at its first frame, then one pair per step."""
    return [(KEY, order[0])] + list(zip(order, order[1:]))


def path_pairs(n):
    """Every pair asked of a clip of n frames in one call: steps back, holds, and the chains with their key pairs."""
    return back_pairs(n) + hold_pairs(n) + [p for order in chains(n) for p in chained(order)]


class Case(crop_gpu.Case):
    """test_index_crop_gpu.Case with the path call in place of the crop call."""

    def raw(self, rect, pairs, tight=False, cap=None, room=None, keys=True):
        n = len(pairs)
        room = n * self.bound(rect) if room is None else room
        out = np.full(room + 16, FILL, dtype=np.uint8)
        frm, to = (C.c_int * n)(*[a for a, _ in pairs]), (C.c_int * n)(*[b for _, b in pairs])
        lens, ks, total = (C.c_size_t * n)(*([12345] * n)), (C.c_int * n)(*([77] * n)), C.c_size_t(12345)
        rc = N.lib().jsp_index_path_frames(self.gpu._h, self.idx._h, *rect, n, frm, to, 1 if tight else 0, C.c_void_p(out.ctypes.data),
                                           room if cap is None else cap, lens, ks if keys else None, C.byref(total))
        return rc, list(lens), list(ks), total.value, out

    def check(self, rect, pairs, tight=False, python=True):
        wants = [made(self.s, rect, p, tight) for p in pairs]
        nb = rect[2] * rect[3]
        before = self.digest()
        rc, lens, keys, total, out = self.raw(rect, pairs, tight)
        bad = next((j for j, x in enumerate(wants) if not isinstance(x, bytes)), None)
        where = f"{self.where} {rect} tight={tight}"
        if bad is None:
            assert rc == 0, where + ": " + N.last_error()
            assert lens == [len(x) for x in wants] and total == sum(lens), where
            got, at = out[:total].tobytes(), 0
            for p, x in zip(pairs, wants):
                assert got[at:at + len(x)] == x, f"{where} pair {p} at byte {at} of the call"
                at += len(x)
            assert np.all(out[total:] == FILL), where + ": written behind the frames"
            flags = [cr.flag(self.bits, x, nb) for x in wants]
            assert keys == [int(f) for f in flags], where
            assert all(flags[j] for j, p in enumerate(pairs) if p[0] == KEY), where
            if python:
                assert self.idx.PathFrames(rect, pairs, tight=tight) == (wants, flags), where
        else:
            pair, (kind, j) = pairs[bad], wants[bad]
            err = N.last_error()
            assert rc != 0 and lens == [0] * len(pairs) and keys == [0] * len(pairs) and total == 0, where
            assert err.startswith(f"index_path: pair {bad} {what(pair)}: "), (where, err)
            blocks = f"block {j} of the rectangle (block {cr.src(cc.NBX, rect, j)} of the picture)"
            if kind == "none":
                assert f": {blocks} has no writer up to frame {pair[1]} " in err, (where, err)
            else:
                assert f"the code of {blocks} in frame {pr.writer(self.s.codes, cc.NBX, rect, pair, j)}," in err and "cut off" in err, (where, err)
            assert np.all(out == FILL), where + ": written on a refusal"
            if python:
                with pytest.raises(CodecError, match=f"index_path: pair {bad} .*block {j} of the rectangle"):
                    self.idx.PathFrames(rect, pairs, tight=tight)
        assert self.digest() == before, where + ": a frame buffer or the codec's previous frame changed"
        return wants


@pytest.mark.parametrize("bits", [16, 8])
@pytest.mark.parametrize("rect", cc.RECTS, ids=cc.rect_id)
def test_every_step_back_hold_and_chain_of_a_rectangles_clip_in_one_call_chunked_and_sliced(bits, rect):
    clip = cc.seams(bits, rect)
    c = Case(clip)
    pairs = path_pairs(c.n)
    wants = c.check(rect, pairs)                            # frame j starts wherever the frames before it end: unaligned bases
    assert all(isinstance(x, bytes) for x in wants)
    c.check(rect, pairs, tight=True)
    for f in clip.patterns:                                 # n pairs in one call equal n calls: each pattern alone, backwards
        c.check(rect, [(f, f - 1)], python=False)
    for s in ("1", "2", "auto"):
        c.gpu.set_option("msv1_index_delta_slice", s)
        c.check(rect, pairs[:9] + pairs[-5:], python=False)
        c.check(rect, pairs[20:27], tight=True, python=False)
    if rect in ((5, 3, 37, 31), (1, 1, 46, 45)):            # every pair out of slices of two pairs: each slice gathers from base 0,
        c.gpu.set_option("msv1_index_delta_slice", "2")     # and the sizes kernel is launched again for it
        c.check(rect, pairs, python=False)
        c.check(rect, pairs, tight=True, python=False)
    c.close()
    c = Case(clip, chunk=cc.kc.CHUNK)                       # the writers <= `to` lie in another chunk of the index than the window
    c.check(rect, pairs)
    c.check(rect, pairs, tight=True, python=False)
    c.close()


@pytest.mark.parametrize("bits", [16, 8])
def test_key_and_forward_pairs_are_crop_frames_and_the_whole_grid_the_whole_picture_calls(bits):
    for clip, rect in ((cc.seams(bits, (5, 3, 37, 31)), (5, 3, 37, 31)), (cc.seams(bits, (3, 2, 3, 2)), (3, 2, 3, 2)),
                       (cc.tight(bits), cc.TIGHT_RECT), (cc.seams(bits, cc.WHOLE), cc.WHOLE)):
        c = Case(clip)
        pairs = cc.pairs(c.n)
        for tight in (False, True):
            assert c.idx.PathFrames(rect, pairs, tight=tight) == c.idx.CropFrames(rect, pairs, tight=tight), (c.where, rect, tight)
        if rect == cc.WHOLE:
            gaps = [p for p in pairs if p[0] != KEY]
            frames, flags = c.idx.PathFrames(None, gaps)
            assert frames == c.idx.DeltaFrames(gaps), c.where
            assert flags == [bool(c.gpu.IsKeyFrame(x)) for x in frames], c.where
            assert c.idx.PathFrames(None, gaps, tight=True)[0] == c.idx.DeltaFrames(gaps, tight=True), c.where
            ts = list(range(c.n))
            frames, flags = c.idx.PathFrames(None, [(KEY, t) for t in ts], tight=True)
            assert frames == [c.idx.KeyFrame(t) for t in ts] and all(flags), c.where
            back = back_pairs(c.n)
            assert c.idx.PathFrames(None, back) == c.idx.PathFrames(cc.WHOLE, back)
        c.close()
    c = Case(cc.cuts(bits))                                 # ... and the refusal texts, apart from the prefix
    first = {j: f for f, _, j in c.s.clip.groups if j is not None}
    for pairs in ([(KEY, 0), (KEY, first[4] + 2), (0, 3)], [(0, 3), (first[1023], first[1023] + 2)]):
        texts = []
        for call in (c.idx.CropFrames, c.idx.PathFrames):
            with pytest.raises(CodecError) as e:
                call(cc.REFUSAL_RECT, pairs)
            texts.append(str(e.value))
        assert texts[0].startswith("index_crop: pair 1 ") and texts[1] == "index_path" + texts[0][len("index_crop"):], texts
    c.close()


@pytest.mark.parametrize("bits", [16, 8])
def test_the_tight_clip_in_every_order_of_two_frames(bits):
    clip = cc.tight(bits)
    for chunk in (None, 3):
        c = Case(clip, chunk=chunk)
        pairs = [(a, b) for a in range(-1, c.n) for b in range(c.n) if a != b] + hold_pairs(c.n) + [(KEY, t) for t in range(c.n)]
        wants = c.check(clip.rect, pairs, tight=True, python=chunk is None)
        loose = c.check(clip.rect, pairs, python=False)
        assert all(isinstance(x, bytes) for x in wants + loose)
        assert all(len(x) <= len(y) for x, y in zip(wants, loose)) and sum(len(x) < len(y) for x, y in zip(wants, loose)) > 5
        c.close()
    # from frame 4 on the picture before the index shows most blocks: a tight step back drops what it already shows, a loose one,
    # and a tight one where the pictures differ, has no code to give
    c = Case(clip, start=4)
    nb = clip.rect[2] * clip.rect[3]
    wants = c.check(clip.rect, [(KEY, 2), (2, 1), (1, 1)], tight=True)
    assert wants[1] == pr.hold(nb)
    assert c.check(clip.rect, [(KEY, 2), (2, 1)])[1][0] == "none"
    assert c.check(clip.rect, [(KEY, 2), (2, 2), (1, 0)], tight=True)[2][0] == "none"
    c.close()


@pytest.mark.parametrize("bits", [16, 8])
def test_the_first_refusing_pair_and_block_is_named_and_nothing_is_written(bits):
    rect = cc.REFUSAL_RECT
    clip = cc.cuts(bits)
    c = Case(clip)
    first = {j: f for f, _, j in clip.groups if j is not None}
    out_first = [f for f, _, j in clip.groups if j is None]
    ok = [(KEY, 0), (3, 0), (KEY, first[4] + 3), (first[4] + 3, first[4]), (out_first[0] + 3, out_first[0] + 2), (2, 2),
          (out_first[1] + 3, out_first[1] + 1)]
    assert all(isinstance(made(c.s, rect, p), bytes) for p in ok)
    for s in ("auto", "1", "2"):
        c.gpu.set_option("msv1_index_delta_slice", s)
        for j, f in first.items():                          # a cut in pair 1, pairs that are not cut before and after it
            assert made(c.s, rect, (f + 3, f + 2)) == ("cut", j)
            c.check(rect, [ok[0], (f + 3, f + 2), ok[1]], python=s == "auto")
            c.check(rect, [ok[1], (f + 3, f + 1), ok[2]], tight=True, python=False)
        # two refusals: the first PAIR is named, not the lower block
        c.check(rect, [ok[1], (first[256] + 3, first[256] + 2), (first[3] + 3, first[3] + 2), ok[0]])
        c.check(rect, [(first[1024] + 3, first[1024] + 1), ok[2], (KEY, first[0] + 1)])
        c.check(rect, ok[2:] + [(first[1023] + 3, first[1023] + 2)])   # the last pair of the call
        c.check(rect, ok)                                   # ... and the call works after the refusals
    c.close()
    clip = cc.nones(bits)
    c = Case(clip, start=cc.NONES_START)
    for k, j in enumerate(clip.at):
        assert made(c.s, rect, (k + 1, k)) == ("none", j)
        c.check(rect, [(k, k + 1), (k + 1, k), (KEY, c.n - 1)])
        c.check(rect, [(KEY, c.n - 1), (c.n - 1, c.n - 1), (c.n - 1, k)], tight=True, python=False)
    wants = c.check(rect, [(KEY, c.n - 1), (-1, c.n - 1), (0, c.n - 1), (c.n - 1, c.n - 1)])
    assert all(isinstance(x, bytes) for x in wants)
    c.close()


@pytest.mark.parametrize("bits", [16, 8])
def test_cap_lens_keys_and_total(bits):
    rect = (5, 3, 37, 31)
    c = Case(cc.seams(bits, rect))
    pairs = [(KEY, 5), (5, 3), (3, 3), (3, 2), (2, 7), (7, 6), (KEY, 2)]
    wants = [made(c.s, rect, p) for p in pairs]
    lens, total = [len(x) for x in wants], sum(len(x) for x in wants)
    keys = [int(cr.flag(bits, x, rect[2] * rect[3])) for x in wants]
    assert 0 in keys and 1 in keys
    for cap in (total - 1, total - 2, 1, 0):                 # too small: refused, lens, keys and *total still set, nothing written
        rc, got_lens, got_keys, got_total, out = c.raw(rect, pairs, cap=cap)
        assert rc != 0 and got_lens == lens and got_keys == keys and got_total == total and np.all(out == FILL), cap
        assert N.last_error().startswith("index_path: cap is smaller")
    rc, got_lens, got_keys, got_total, out = c.raw(rect, pairs, cap=total, room=total, keys=False)   # exactly the length; no keys
    assert rc == 0 and got_lens == lens and got_keys == [77] * len(pairs) and np.all(out[total:] == FILL)
    assert out[:total].tobytes() == b"".join(wants)
    c.close()


@pytest.mark.parametrize("bits", [16, 8])
def test_a_codec_of_the_rectangles_size_decodes_a_reversed_clip_and_a_boomerang_on_the_gpu(bits):
    """A fresh codec of 4 bw x 4 bh pixels decodes the key pair's frame and the chained pairs' frames: each picture is the
    sub-rectangle of Show(t)."""
    rect = (5, 3, 37, 31)
    bx, by, bw, bh = rect
    for clip, tight in ((cc.seams(bits, rect), False), (cc.tight(bits), True)):
        c = Case(clip)
        shown = dev_buf(cc.W * cc.H)
        for order in chains(c.n):
            frames, flags = c.idx.PathFrames(rect, chained(order), tight=tight)
            fresh = make_gpu(bits, 4 * bw, 4 * bh, c.pal, parse=crop_gpu.PARSE)
            pool = [dev_buf(16 * bw * bh) for _ in range(2)]
            for k, (t, data) in enumerate(zip(order, frames)):
                prev = fresh.PreviousFrame()
                dst = next(b for b in pool if b is not prev)
                assert bool(fresh.IsKeyFrame(data)) == flags[k]
                if k == 0:
                    assert fresh.DecompressI(data, dst) == 0
                else:
                    dst.copy_(prev)
                    fresh.DecompressP(data, dst)
                shown.fill_(POISON)
                c.idx.Show(t, shown, adopt=False)
                want = shown.cpu().numpy().reshape(cc.H, cc.W)[4 * by:4 * by + 4 * bh, 4 * bx:4 * bx + 4 * bw]
                got = fresh.PreviousFrame().cpu().numpy().reshape(4 * bh, 4 * bw)
                assert np.array_equal(got, want), f"{c.where}: entry {k} (frame {t}) of the order {order}"
            fresh.StopAndClean()
        c.close()


def test_every_argument_refusal_and_their_order():
    import torch
    W, H = 40, 24
    from jsplayer_amd import streamgen as sg
    frames, keys, _ = sg.msv1_clip(41, W, H, 6, bits=16, p_mix=sg.msv1_p_mix(0.6, 3.0))
    parse = crop_gpu.PARSE
    codec, other = make_gpu(16, W, H, parse=parse), make_gpu(16, W, H, parse=parse)
    idx, foreign = codec.BuildIndex(frames, keys), other.BuildIndex(frames, keys)
    wrong = ScreenPressor(W, H, 24)
    tiny = make_gpu(16, 3, 8, parse=parse)                       # a picture without a 4x4 block
    tiny_idx = tiny.BuildIndex([b"\x01\x02\x03\x04", b""], [True, False])
    lib = N.lib()
    fn, n = lib.jsp_index_path_frames, idx.frames
    good = (2, 1, 5, 4)
    bound = idx.CropBound(5, 4)
    usual = ((KEY, 2), (2, 0))

    def info():
        k, d, h = C.c_int(0), C.c_uint64(0), C.c_uint64(0)
        assert lib.jsp_index_info(idx._h, C.byref(k), C.byref(d), C.byref(h)) == 0
        return k.value, d.value, h.value

    at_build = info()
    first = idx.PathFrames(good, usual)                          # (the scratch is allocated here: from now on nothing may grow)
    # jsp_index_info counts the scratch: records of 2 pairs x 20 blocks and the frames at their bound on the device, the pinned side
    assert info()[0] == at_build[0] and info()[1] >= at_build[1] + 2 * 20 * 8 + 2 * bound and info()[2] > at_build[2]
    assert (idx.device_bytes, idx.host_bytes) == info()[1:]
    out = np.full(2 * bound, FILL, dtype=np.uint8)
    stands = {"prev": codec.PreviousFrame()}
    before = info()

    def refused(what, message, c=codec._h, i=idx._h, rect=good, pairs=usual, count=None, flags=0, dst=out.ctypes.data,
                cap=2 * bound, lens=True, total=True, frm=True, to=True):
        k = len(pairs)
        a, b = (C.c_int * k)(*[p[0] for p in pairs]), (C.c_int * k)(*[p[1] for p in pairs])
        ls, ks, size = (C.c_size_t * k)(*([777] * k)), (C.c_int * k)(*([777] * k)), C.c_size_t(777)
        count = k if count is None else count
        rc = fn(c, i, *rect, count, a if frm else None, b if to else None, flags, C.c_void_p(dst) if dst else None, cap, ls if lens else None,
                ks, C.byref(size) if total else None)
        err = N.last_error()
        print(f"jsp_index_path_frames: {what}: {err}")
        assert rc != 0 and err == message, (what, err)
        assert size.value == (0 if total else 777) and np.all(out == FILL), what
        zeroed = 1 <= count <= 4096
        assert list(ls) == ([0] * k if lens and zeroed else [777] * k) and list(ks) == ([0] * k if zeroed else [777] * k), what
        assert info() == before and codec.PreviousFrame() is stands["prev"], what

    def tl(what):
        return "index_path: " + what

    def pair(j, a, b, of=n):
        return tl(f"pair {j} ({a}, {b}) is no pair of the index: `to` is one of its {of} frames, `from` is one too (a step forward, a "
                  f"hold or a step back), or -1 (before the range), or -2 (a key pair)")

    def grid(rect, nbx=W // 4, nby=H // 4):
        return tl("the rectangle (%d, %d, %d x %d blocks) is outside the block grid (%d x %d blocks)" % (rect + (nbx, nby)))

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
    for bad in ((-1, 0, 3, 3), (0, -1, 3, 3), (0, 0, 0, 3), (0, 0, 3, 0), (0, 0, 11, 1), (8, 0, 3, 1), (0, 0, 1, 7), (0, 4, 1, 3),
                (2 ** 31 - 1, 0, 2 ** 31 - 1, 1), (0, 0, -3, -3)):
        refused(f"rectangle {bad}", grid(bad), rect=bad)
    refused("no block", grid((0, 0, 1, 1), 0, 0), c=tiny._h, i=tiny_idx._h, rect=(0, 0, 1, 1), pairs=((1, 0),))
    for bad in (0, -1, 4097):
        refused(f"n = {bad}", tl("n is outside 1..4096"), count=bad)
    for bad in (2, 3, -1, 1 << 16):
        refused(f"flags = {bad}", tl("unknown flag bits"), flags=bad)
    refused("from < -2", pair(1, -3, 3), pairs=((1, 0), (-3, 3)))
    refused("from == -1 with to == -1", pair(0, -1, -1), pairs=((-1, -1), (1, 0)))
    refused("a step back to before the range", pair(1, 3, -1), pairs=((3, 3), (3, -1)))
    refused("from == nframes", pair(0, n, 0), pairs=((n, 0),))
    refused("to == nframes", pair(0, 0, n), pairs=((0, n),))
    refused("from == to == nframes", pair(1, n, n), pairs=((2, 2), (n, n)))
    refused("a key pair at nframes", pair(0, KEY, n), pairs=((KEY, n),))
    refused("a key pair below 0", pair(1, KEY, -1), pairs=((KEY, 0), (KEY, -1)))
    refused("the first bad pair is named", pair(1, 4, n), pairs=((4, 1), (4, n), (-5, 2)))

    # ---- the earlier refusal wins ---------------------------------------------------------------------------------------------
    refused("wrong codec kind + foreign index + bad n", "index: MSVideo1 only", c=wrong._h, i=foreign._h, count=0)
    refused("foreign index + bad rectangle", tl("the index was built by another codec"), i=foreign._h, rect=(0, 0, 0, 0))
    refused("bad rectangle + bad n", grid((9, 0, 2, 1)), rect=(9, 0, 2, 1), count=0)
    refused("bad n + bad flags", tl("n is outside 1..4096"), count=0, flags=8)
    refused("bad flags + bad pair", tl("unknown flag bits"), flags=4, pairs=((3, -1),))
    frame_buf = torch.zeros(W * H, dtype=torch.int32, device="cuda")
    ticket = codec.DecompressI_async(frames[0], frame_buf)
    stands["prev"] = codec.PreviousFrame()
    in_flight = tl("an asynchronous frame is in flight (jsp_wait for it first)")
    refused("bad pair + in flight", pair(0, n, 1), pairs=((n, 1),))
    refused("bad rectangle + in flight", grid((0, 0, 11, 6)), rect=(0, 0, 11, 6))
    refused("in flight", in_flight)
    refused("in flight + too-small cap", in_flight, cap=1)
    codec.wait(ticket)

    # ---- the calls that move forward only still refuse a step back and a hold -----------------------------------------------------
    for call in (lambda p: idx.CropFrames(good, p), lambda p: idx.DeltaFrames(p), lambda p: idx.PanFrames((5, 4), [(a, b, (2, 1), (2, 1)) for a, b in p])):
        for bad in ((3, 1), (2, 2)):
            with pytest.raises(CodecError, match="pair 0"):
                call([bad])
    with pytest.raises(CodecError, match="index_path: the rectangle"):
        idx.PathFrames((0, 0, 11, 1), [(KEY, 0)])

    # ---- and the call that is not refused works after all that --------------------------------------------------------------------
    assert idx.PathFrames(good, usual) == first and info() == before
    assert idx.PathFrames(None, usual) == idx.PathFrames((0, 0, W // 4, H // 4), usual)
    for x in (idx, foreign, tiny_idx):
        x.close()
    for c in (codec, other, wrong, tiny):
        c.StopAndClean()


class TestOnGpuParse:
    """Every test of this file once more with the block tables of the on-GPU parse — the codec's default (the tests above keep the
    host parser and their names)."""

    @pytest.fixture(autouse=True)
    def parse_mode(self):
        crop_gpu.PARSE = "gpu"
        yield crop_gpu.PARSE
        crop_gpu.PARSE = "host"


for _name, _test in list(globals().items()):
    if _name.startswith("test_"):
        setattr(TestOnGpuParse, _name, staticmethod(_test))
