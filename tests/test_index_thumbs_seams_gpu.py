"""msv1_index_thumbs_kernel past one workgroup, at ties, at saturation and with a top byte in the pixel words, on an MI355X.

tests/test_index_thumbs_gpu.py runs pictures of at most 192 work-items a thumbnail: one workgroup at every scale.  The sizes here
(thumbs_charts.MSV1_SIZES; tests/test_thumbs_charts_cpu.py asserts their launches) are the smallest that cross a workgroup in all six
instantiations of the kernel — 86x70: a partly filled second workgroup whose boundary lies inside a thumbnail row; 128x64: exactly two
full workgroups; 12x520: one output column at s = 8, refused at s = 16.  The chart clips (thumbs_charts) put ties, saturated cells and
a palette word with a top byte under every scale.

Truth as in test_index_thumbs_gpu.py: the oracle's pictures, then tests/thumbs_ref.py.  Every comparison is exact."""
from functools import lru_cache

import numpy as np
import pytest

import msv1_range_clips as rc
import thumbs_charts as tc
import thumbs_ref as tr
from jsplayer_amd import CodecError
from jsplayer_amd import streamgen as sg
from oracle_binding import OracleMSVideo1
from test_index_thumbs_gpu import POISON, check, dev_buf, mixed_clip, oracle_pictures

pytestmark = pytest.mark.gpu

PARSE = "host"
FF = 0xFFFFFFFF


@pytest.fixture(autouse=True, params=["host", "gpu"])
def parse_mode(request):
    """Every test runs with the block tables of the host parser and of the on-GPU parse."""
    global PARSE
    PARSE = request.param
    yield request.param
    PARSE = "host"


def size_id(s):
    return f"{s[0]}x{s[1]}"


def make_gpu(bits, w, h, pal=None, chunk=None):
    return rc.make_gpu(bits, w, h, pal, 36, chunk, PARSE)


@lru_cache(maxsize=None)
def mixed(bits, w, h, seed=0):
    """(frames, keys, palette, the oracle's pictures): once for both parse modes; nobody changes them."""
    frames, keys, pal = mixed_clip(bits, w, h, seed)
    return frames, keys, pal, oracle_pictures(bits, w, h, pal, frames, keys)


def refused_too_small(idx, s):
    out = dev_buf(64)
    with pytest.raises(CodecError, match="too small") as e:
        idx.Thumbs([0], scale=s, out=out)
    assert "index_thumbs" in str(e.value)
    with pytest.raises(CodecError, match="too small"):
        idx.ThumbSize(s)
    assert np.all(out.cpu().numpy().view(np.uint32) == POISON)


@pytest.mark.parametrize("bits", [16, 8])
@pytest.mark.parametrize("size", tc.MSV1_SIZES, ids=size_id)
def test_every_frame_shuffled_with_repeats_where_every_scale_has_a_second_workgroup(bits, size):
    w, h = size
    frames, keys, pal, pictures = mixed(bits, w, h)
    g = make_gpu(bits, w, h, pal)
    n = len(frames)
    rng = np.random.default_rng(23 + bits + w)
    picks = [int(t) for t in rng.permutation(n)] + [int(t) for t in rng.integers(0, n, size=6)] + [n - 1, n - 1, 0]
    assert len(picks) % 5 != 0
    with g.BuildIndex(frames, keys) as idx:
        for s in tr.SCALES:
            if s not in tc.valid_scales(w, h):
                assert (w, h, s) == (12, 520, 16)
                refused_too_small(idx, s)
                continue
            assert tc.lanes(w, h, s)["workgroups"] > 1
            for cols in (1, 5):
                check(idx, pictures, picks, w, h, s, cols, f"{bits}-bit {w}x{h} s={s} cols={cols} ({PARSE} parse)")
    g.StopAndClean()


@pytest.mark.parametrize("bits", [16, 8])
def test_several_chunks_at_86x70(bits):
    w, h = 86, 70
    frames, keys, pal, pictures = mixed(bits, w, h, 3)
    g = make_gpu(bits, w, h, pal, chunk=5)
    with g.BuildIndex(frames, keys) as idx:
        picks = list(range(len(frames) - 1, -1, -1))
        for s in tr.SCALES:
            for cols in (1, 5):
                check(idx, pictures, picks, w, h, s, cols, f"{bits}-bit chunked s={s} cols={cols} ({PARSE} parse)")
    g.StopAndClean()


# ---- the picture before the index, with words of 0xFFFFFFFF in it ---------------------------------------------------------------
BEFORE_W, BEFORE_H, BEFORE_START = 86, 70, 4


def ff_mask(w, h):
    """(h, w) bool: of the whole 16x16 cells, every third (diagonals) wholly, every third in every other 4x4 block, the rest not."""
    y, x = np.mgrid[0:16 * (h // 16), 0:16 * (w // 16)]
    kind = (x // 16 + y // 16) % 3
    out = np.zeros((h, w), dtype=bool)
    out[:y.shape[0], :x.shape[1]] = (kind == 0) | ((kind == 1) & ((x // 4 + y // 4) % 2 == 1))
    return out


def oracle_pictures_painted(bits, w, h, pal, frames, keys, start_fill, paint_after, mask, lines=36):
    """test_index_thumbs_gpu.oracle_pictures with buffers that start as `start_fill`, and with the words under `mask` of the picture
    of frame `paint_after` set to 0xFFFFFFFF in the buffer the decoder holds as its previous frame (as the GPU side does)."""
    o = OracleMSVideo1(bits, w, h, pal)
    o.Preinit(lines)
    bufs = [np.full(w * h, start_fill & FF, dtype=np.uint32).view(np.int32) for _ in range(3)]
    out = []
    for i, (src, key) in enumerate(zip(frames, keys)):
        prev = o.PreviousFrame()
        dst = next(b for b in bufs if b is not prev)
        if prev is not None:
            np.copyto(dst, prev)
        if key:
            assert o.DecompressI(src, dst) == 0
        else:
            o.DecompressP(src, dst)
        pic = o.PreviousFrame()
        assert pic is not None
        if i == paint_after:
            pic.reshape(h, w)[mask] = -1
        out.append(pic.copy())
    o.close()
    return out


@lru_cache(maxsize=None)
def before_clip(bits):
    w, h, start = BEFORE_W, BEFORE_H, BEFORE_START
    base, bkeys, pal = sg.msv1_clip(830 + bits, w, h, 12, bits=bits, p_mix=sg.msv1_p_mix(0.6, 5.0), key_every=100)
    gen = rc.Idle(bits, w, h, 9)
    every_other = gen.change(list(range(0, gen.nb, 2)))
    allskip = gen.all_skip("long")
    idle = [allskip, bytes([0x10, 0x84]) if bits == 16 else allskip, allskip]
    frames = [base[0], every_other, base[1], base[2]] + idle + list(base[3:])
    keys = [True, False, False, False] + [False] * 3 + list(bkeys[3:])
    pictures = oracle_pictures_painted(bits, w, h, pal, frames, keys, FF, start - 1, ff_mask(w, h))
    return frames, keys, pal, pictures


@pytest.mark.parametrize("bits", [16, 8])
def test_picture_before_the_index_holds_words_of_all_ones(bits):
    """The codec is brought to frame 4 frame by frame in buffers that start as 0xFFFFFFFF; the index starts there with three frames
    that code nothing.  Frame 1 is an inter frame that codes every other block.

    No stream leaves the buffers' fill inside the block grid: a skip code with no picture before it raises (as the reference does),
    and a frame that is adopted codes or copies every whole block — only an 8-bit end marker leaves blocks alone.  So the words of
    0xFFFFFFFF are written by the caller into the buffer the codec holds as its previous frame (ff_mask: whole 16x16 cells, and
    cells with every other block), on both sides alike: the picture before an index is what that buffer holds when the index is
    built.  They bring all-255 bytes and a top byte of 0xFF to the kernel's `before` path at both bit depths."""
    import torch
    w, h, start = BEFORE_W, BEFORE_H, BEFORE_START
    frames, keys, pal, pictures = before_clip(bits)
    mask = ff_mask(w, h)
    before = pictures[start - 1]
    assert np.all(before.view(np.uint32).reshape(h, w)[mask] == FF) and np.any(before.view(np.uint32).reshape(h, w)[~mask] != FF)
    for s in tr.SCALES:
        t = tr.thumbnail(before, w, h, s).view(np.uint32)
        assert np.any(t == 0x00FFFFFF) and np.any(t != 0x00FFFFFF) and np.all(t >> 24 == 0), s
    g = make_gpu(bits, w, h, pal)
    pool = [dev_buf(w * h, -1) for _ in range(3)]
    for i in range(start):
        prev = g.PreviousFrame()
        dst = next(b for b in pool if b is not prev)
        if prev is not None:
            dst.copy_(prev)
        if keys[i]:
            assert g.DecompressI(frames[i], dst) == 0
        else:
            g.DecompressP(frames[i], dst)
    prev = g.PreviousFrame()
    prev.view(h, w)[torch.from_numpy(mask).to(prev.device)] = -1
    torch.cuda.synchronize()
    assert np.array_equal(prev.cpu().numpy(), before)
    with g.BuildIndex(frames[start:], keys[start:]) as idx:
        for buf in pool:
            buf.fill_(POISON)                                           # the index keeps a copy of the picture before, not the buffer
        picks = list(range(idx.frames))
        rel = pictures[start:]
        for s in tr.SCALES:
            check(idx, rel, picks, w, h, s, 4, f"{bits}-bit before of all ones s={s} ({PARSE} parse)")
            for t in range(3):
                got = idx.Thumbs([t], scale=s).cpu().numpy()
                assert np.array_equal(got, tr.thumbnail(before, w, h, s)), f"{bits}-bit idle frame {t} s={s} ({PARSE} parse)"
    g.StopAndClean()


# ---- the chart clips ----------------------------------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def charts(bits, w, h):
    frames, keys, pal = tc.msv1_chart_clip(bits, w, h)
    return frames, keys, pal, oracle_pictures(bits, w, h, pal, frames, keys)


@pytest.mark.parametrize("bits", [16, 8])
@pytest.mark.parametrize("size", tc.MSV1_SIZES, ids=size_id)
def test_chart_clips_ties_saturation_and_the_top_byte(bits, size):
    w, h = size
    frames, keys, pal, pictures = charts(bits, w, h)
    v = tc.msv1_values(bits)
    scales = tc.valid_scales(w, h)
    # what the reference holds, before the kernel is asked
    for s in scales:
        per = [tc.census(p, w, h, s, v["top"]) for p in pictures]
        assert all(sum(c[ch]["tie"] for c in per) > 0 for ch in "rgb"), s
        ex = tr.thumbnail(pictures[tc.EXTREMES_AT], w, h, s).view(np.uint32)
        if s == 16 or 16 not in scales:
            assert np.any(ex == v["word_bright"]) and np.any(ex == 0), s
    if bits == 8:
        for t in range(3):
            assert np.any(pictures[t].view(np.uint32) >> 24 == 0xFF)
            for s in scales:
                assert np.all(tr.thumbnail(pictures[t], w, h, s).view(np.uint32) >> 24 == 0)
    g = make_gpu(bits, w, h, pal)
    with g.BuildIndex(frames, keys) as idx:
        for s in tr.SCALES:
            if s not in scales:
                refused_too_small(idx, s)
                continue
            check(idx, pictures, [4, 0, 3, 1, 2], w, h, s, 2, f"{bits}-bit charts {w}x{h} s={s} ({PARSE} parse)")
    g.StopAndClean()
