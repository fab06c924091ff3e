"""Thumbnails of a seek index (jsp_index_thumb_size / jsp_index_thumbs, SeekIndex.ThumbSize / Thumbs) on an MI355X.

Truth is the oracle, not the library: the clip decoded frame by frame with OracleMSVideo1 into buffers that start as zeros (each
destination first copied from the picture before it), then the contract's formula in numpy (tests/thumbs_ref.py: box mean per channel,
rounded half up, integer arithmetic).  Every comparison is exact."""
import ctypes as C
import os
import subprocess
import zlib

import numpy as np
import pytest

import msv1_range_clips as rc
import thumbs_ref as tr
from jsplayer_amd import CodecError, MSVideo1_16bit, MSVideo1_8bit, ScreenPressor
from jsplayer_amd import _native as N
from jsplayer_amd import streamgen as sg
from oracle_binding import OracleMSVideo1

pytestmark = pytest.mark.gpu

POISON = 0x5A5A5A5A
PARSE = "host"
SIZES = [(64, 48), (36, 20), (70, 46)]   # block counts multiples of 4; odd (a trailing column / row dropped at s = 8, 16); W % 4, H % 4 != 0


@pytest.fixture(autouse=True, params=["host", "gpu"])
def parse_mode(request):
    """Every test runs with the block tables of the host parser and of the on-GPU parse."""
    global PARSE
    PARSE = request.param
    yield request.param
    PARSE = "host"


def dev_buf(n, fill=POISON):
    import torch
    return torch.full((n,), fill, dtype=torch.int32, device="cuda")


def make_gpu(bits, w, h, pal=None, lines=36, chunk=None):
    c = MSVideo1_16bit(w, h) if bits == 16 else MSVideo1_8bit(w, h, pal or b"")
    c.set_option("msv1_parse", PARSE)
    if chunk:
        c.set_option("msv1_seek_chunk_frames", str(chunk))
    c.Preinit(lines)
    return c


def oracle_pictures(bits, w, h, pal, frames, keys, lines=36, keep=None):
    """The picture after every frame (zeros while there is none), buffers starting as zeros.  keep: only these frames (others None)."""
    o = OracleMSVideo1(bits, w, h, pal)
    o.Preinit(lines)
    bufs = [np.zeros(w * h, dtype=np.int32) for _ in range(3)]
    out = []
    for i, (src, key) in enumerate(zip(frames, keys)):
        prev = o.PreviousFrame()
        dst = next(b for b in bufs if b is not prev)
        if prev is not None:
            np.copyto(dst, prev)
        else:
            dst.fill(0)
        if key:
            assert o.DecompressI(src, dst) == 0
        else:
            o.DecompressP(src, dst)
        pic = o.PreviousFrame()
        if keep is not None and i not in keep:
            out.append(None)
        else:
            out.append(np.zeros(w * h, dtype=np.int32) if pic is None else pic.copy())
    o.close()
    return out


def gpu_prefix(g, frames, keys, start, w, h):
    """Frames [0, start) one by one, zero-started buffers, each destination first copied from the picture before it."""
    pool = [dev_buf(w * h, 0) for _ in range(3)]
    for i in range(start):
        prev = g.PreviousFrame()
        dst = next(b for b in pool if b is not prev)
        if prev is not None:
            dst.copy_(prev)
        if keys[i]:
            assert g.DecompressI(frames[i], dst) == 0
        else:
            g.DecompressP(frames[i], dst)
    return pool


def mixed_clip(bits, w, h, seed=0):
    """A key frame, inter frames with skips, all-skip frames, early-outs, an 8-bit end marker part-way, a truncated frame, the odd
    trailing byte (16-bit), key frames mid-range."""
    frames, keys, pal = sg.msv1_clip(700 + seed + bits, w, h, 14, bits=bits, p_mix=sg.msv1_p_mix(0.6, 5.0), key_every=6)
    nb = (w // 4) * (h // 4)
    allskip = b"".join(bytes([min(nb - k, 255), 0x84]) for k in range(0, nb, 255))
    out, ks = list(frames[:4]), list(keys[:4])
    out += [allskip, bytes([0x10, 0x84]), frames[4]]
    ks += [False, False, keys[4]]
    full = frames[5] if not keys[5] else frames[4]
    out.append(full[: max(2, len(full) // 2)])                          # truncated
    ks.append(False)
    if bits == 8:
        out.append(full[:10] + b"\x00\x00" + full[12:])                 # end marker part-way
    else:
        out.append(full + b"\x07")                                      # odd trailing byte
    ks.append(False)
    out += list(frames[5:])
    ks += list(keys[5:])
    out.append(allskip)
    ks.append(False)
    return out, ks, pal


def want_sheet(pictures, picks, w, h, s, cols, fill=POISON):
    return tr.sheet([tr.thumbnail(pictures[t], w, h, s) for t in picks], cols, fill)


def check(idx, pictures, picks, w, h, s, cols, what):
    """Thumbs into a poison-filled sheet against the oracle's pictures; the cells past the last thumbnail keep the poison."""
    tw, th = tr.thumb_size(w, h, s)
    assert idx.ThumbSize(s) == (tw, th), what
    rows = -(-len(picks) // cols) * th
    out = dev_buf(rows * cols * tw + 3)                                 # (three words of slack: nothing past the sheet is written)
    got = idx.Thumbs(picks, scale=s, cols=cols, out=out)
    assert tuple(got.shape) == (rows, cols * tw), what
    want = want_sheet(pictures, picks, w, h, s, cols)
    bad = np.argwhere(got.cpu().numpy() != want)
    assert len(bad) == 0, f"{what}: {len(bad)} pixels differ, first at sheet (row, column) {tuple(bad[0])}"
    assert np.all(out.cpu().numpy()[rows * cols * tw:].view(np.uint32) == POISON), what


@pytest.mark.parametrize("bits", [16, 8])
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_every_frame_shuffled_with_repeats_matches_the_oracle(bits, size):
    w, h = size
    frames, keys, pal = mixed_clip(bits, w, h)
    pictures = oracle_pictures(bits, w, h, pal, frames, keys)
    g = make_gpu(bits, w, h, pal)
    n = len(frames)
    rng = np.random.default_rng(11 + bits + w)
    picks = [int(t) for t in rng.permutation(n)] + [int(t) for t in rng.integers(0, n, size=6)] + [n - 1, n - 1, 0]
    with g.BuildIndex(frames, keys) as idx:
        for s in tr.SCALES:
            for cols in (1, len(picks), 5):                             # an array, a strip, a sheet whose last row is partly empty
                assert len(picks) % 5 != 0
                check(idx, pictures, picks, w, h, s, cols, f"{bits}-bit {w}x{h} s={s} cols={cols} ({PARSE} parse)")
        # out=None: a new zero-filled sheet
        got = idx.Thumbs(picks[:7], scale=4, cols=3)
        assert np.array_equal(got.cpu().numpy(), want_sheet(pictures, picks[:7], w, h, 4, 3, fill=0))
    g.StopAndClean()


@pytest.mark.parametrize("bits", [16, 8])
def test_picture_before_the_range_and_leading_frames_that_code_nothing(bits):
    """The index starts inside the clip with three frames that code nothing: Show writes nothing for them (they lie before
    first_adopted), their thumbnail is the thumbnail of the picture before the range."""
    w, h = 70, 46
    base, bkeys, pal = sg.msv1_clip(810 + bits, w, h, 12, bits=bits, p_mix=sg.msv1_p_mix(0.6, 5.0), key_every=100)
    nb = (w // 4) * (h // 4)
    allskip = b"".join(bytes([min(nb - k, 255), 0x84]) for k in range(0, nb, 255))
    idle = [allskip, bytes([0x10, 0x84]) if bits == 16 else allskip, allskip]
    start = 4
    frames = list(base[:start]) + idle + list(base[start:])
    keys = list(bkeys[:start]) + [False] * 3 + list(bkeys[start:])
    pictures = oracle_pictures(bits, w, h, pal, frames, keys)
    g = make_gpu(bits, w, h, pal)
    pool = gpu_prefix(g, frames, keys, start, w, h)
    assert np.array_equal(g.PreviousFrame().cpu().numpy(), pictures[start - 1])
    with g.BuildIndex(frames[start:], keys[start:]) as idx:
        dst = dev_buf(w * h)
        for t in range(3):
            assert idx.Show(t, dst, adopt=False).data_pnt is not dst and np.all(dst.cpu().numpy().view(np.uint32) == POISON)
        for buf in pool:
            buf.fill_(POISON)                                           # the index keeps a copy of the picture before, not the buffer
        picks = list(range(idx.frames))
        rel = pictures[start:]
        for s in tr.SCALES:
            check(idx, rel, picks, w, h, s, 4, f"{bits}-bit before+idle s={s} ({PARSE} parse)")
            for t in range(3):
                got = idx.Thumbs([t], scale=s).cpu().numpy()
                assert np.array_equal(got, tr.thumbnail(pictures[start - 1], w, h, s))
    g.StopAndClean()


def test_no_picture_before_and_a_key_frame_that_ends_at_an_end_marker():
    """8-bit, a fresh codec: the key frame stops at an end marker part-way, nothing was there before — the blocks it leaves show 0
    until a later frame codes them."""
    w, h = 64, 48
    gen = rc.Idle(8, w, h, 5)
    pal = rc.palette(8)
    at = 7 * gen.nbx + 5                                                # the marker's block: part-way through a block row
    key = gen.key()
    frames = [key[: 2 * at] + b"\x00\x00"]                              # (solid 8-bit codes: two bytes a block)
    for b in range(at, gen.nb):
        gen.col[b] = None
    frames.append(gen.change([3, 17, at - 1]))
    frames.append(gen.change([2, at + 1, gen.nb - 1]))                  # two of the blocks the key frame left
    frames.append(gen.all_skip("long"))
    frames.append(gen.change([at, at + 9]))
    keys = [True] + [False] * (len(frames) - 1)
    pictures = oracle_pictures(8, w, h, pal, frames, keys)
    assert np.all(pictures[0].reshape(h, w)[8 * 4:] == 0) and np.any(pictures[0] != 0)
    g = make_gpu(8, w, h, pal)
    with g.BuildIndex(frames, keys) as idx:
        for s in tr.SCALES:
            check(idx, pictures, [4, 0, 1, 2, 3, 0], w, h, s, 2, f"end-marker key frame s={s} ({PARSE} parse)")
    g.StopAndClean()


@pytest.mark.parametrize("bits", [16, 8])
def test_several_chunks(bits):
    w, h = 36, 20
    frames, keys, pal = mixed_clip(bits, w, h, seed=3)
    pictures = oracle_pictures(bits, w, h, pal, frames, keys)
    g = make_gpu(bits, w, h, pal, chunk=5)
    with g.BuildIndex(frames, keys) as idx:
        picks = list(range(len(frames) - 1, -1, -1))
        for s in tr.SCALES:
            check(idx, pictures, picks, w, h, s, 3, f"{bits}-bit chunked s={s} ({PARSE} parse)")
    g.StopAndClean()


@pytest.mark.parametrize("bits", [16, 8])
@pytest.mark.parametrize("chunk", [None, 37])
def test_long_clip_every_seventh_frame(bits, chunk):
    """300 frames: blocks idle for more than four bitmap words, key frames mid-range, end markers / damage around frames 32, 64, 128."""
    w, h = 64, 48
    frames, keys, pal, plan = rc.long_clip(bits, w, h, seed=21 + bits, n=300)
    assert not plan["raises"]
    picks = list(range(0, 300, 7)) + [299]
    pictures = oracle_pictures(bits, w, h, pal, frames, keys, lines=plan["lines"], keep=set(picks))
    g = make_gpu(bits, w, h, pal, lines=plan["lines"], chunk=chunk)
    with g.BuildIndex(frames, keys, key_row=plan["lines"]) as idx:
        for s in tr.SCALES:
            check(idx, pictures, picks, w, h, s, 8, f"{bits}-bit long clip s={s} chunk={chunk} ({PARSE} parse)")
    g.StopAndClean()


@pytest.mark.parametrize("bits", [16, 8])
def test_equals_the_formula_on_show_and_leaves_no_trace(bits):
    w, h = 70, 46
    frames, keys, pal = mixed_clip(bits, w, h, seed=5)
    start, n = 3, len(frames)
    runs = []
    for call_thumbs in (True, False):
        g = make_gpu(bits, w, h, pal)
        pool = gpu_prefix(g, frames, keys, start, w, h)
        prev = g.PreviousFrame()
        prev_pixels = prev.cpu().numpy().copy()
        idx = g.BuildIndex(frames[start:], keys[start:])
        if call_thumbs:
            for t in (0, 1, 4, 7, idx.frames - 1):
                dst = dev_buf(w * h, 0)
                r = idx.Show(t, dst, adopt=False)
                shown = dst if r.data_pnt is dst else prev            # Show writes nothing: the picture before the range
                for s in tr.SCALES:
                    got = idx.Thumbs([t], scale=s).cpu().numpy()
                    assert np.array_equal(got, tr.thumbnail(shown.cpu().numpy(), w, h, s)), f"{bits}-bit t={t} s={s} ({PARSE} parse)"
            idx.Thumbs(list(range(idx.frames)), scale=8, cols=4)
        assert g.PreviousFrame() is prev and np.array_equal(prev.cpu().numpy(), prev_pixels)
        nxt = next(b for b in pool if b is not prev)
        nxt.copy_(prev)
        r = g.DecompressP(frames[start], nxt) if not keys[start] else None
        if r is None:
            assert g.DecompressI(frames[start], nxt) == 0
        after = g.PreviousFrame().cpu().numpy().copy()
        dst = dev_buf(w * h)
        s2 = idx.Show(5, dst, adopt=True)
        runs.append((None if r is None else (r.significant_changes, r.data_pnt is nxt), after, dst.cpu().numpy().copy(), s2.significant_changes,
                     g.PreviousFrame() is dst))
        idx.close()
        g.StopAndClean()
    a, b = runs
    assert a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and a[3:] == b[3:]


def test_every_refusal_leaves_out_untouched_and_names_the_call():
    import torch
    w, h = 64, 48
    frames, keys, pal = mixed_clip(16, w, h, seed=7)
    a = make_gpu(16, w, h)
    pool = gpu_prefix(a, frames, keys, 2, w, h)
    idx = a.BuildIndex(frames[2:], keys[2:])
    tw, th = idx.ThumbSize(8)
    out = dev_buf(4 * tw * th)

    def refused(match, *args, **kw):
        with pytest.raises(CodecError, match=match) as e:
            idx.Thumbs(*args, **kw)
        assert "index_thumbs" in str(e.value)

    refused("1..4096", [], scale=8, out=out)
    refused("1..4096", [0] * 4097, scale=8, out=dev_buf(16))
    for bad in (-1, idx.frames, 1 << 20):
        refused("outside the index", [0, bad], scale=8, out=out)
    for bad in (0, 1, 2, 5, 12, 32, -8):
        refused("scale", [0], scale=bad, out=out)
    refused("cols", [0, 1], scale=8, cols=0, out=out)
    refused("cols", [0, 1], scale=8, cols=-3, out=out)
    refused("smaller than the sheet", [0, 1, 2, 3, 4], scale=8, out=out)          # five thumbnails, room for four
    refused("smaller than the sheet", [0, 1, 2], scale=8, cols=2, out=out[: 4 * tw * th - 1])   # two sheet rows of two cells
    host = np.full(4 * tw * th, POISON, dtype=np.uint32).view(np.int32)
    refused("device", [0], scale=8, out=host)
    assert np.all(host.view(np.uint32) == POISON)
    prev = a.PreviousFrame()
    ticket = a.DecompressP_async(frames[2], next(b for b in pool if b is not prev))
    refused("in flight", [0], scale=8, out=out)
    a.wait(ticket)
    # null arguments (the C ABI itself)
    lib = N.lib()
    one = (C.c_int * 1)(0)
    for args in ((None, idx._h, 1, one, 8, 1, C.c_void_p(out.data_ptr()), out.numel()),
                 (a._h, None, 1, one, 8, 1, C.c_void_p(out.data_ptr()), out.numel()),
                 (a._h, idx._h, 1, None, 8, 1, C.c_void_p(out.data_ptr()), out.numel()),
                 (a._h, idx._h, 1, one, 8, 1, None, out.numel())):
        assert lib.jsp_index_thumbs(*args) != 0 and "index_thumbs: null argument" in N.last_error()
    wv, hv = C.c_int(-1), C.c_int(-1)
    assert lib.jsp_index_thumb_size(None, 8, C.byref(wv), C.byref(hv)) != 0 and "index_thumb_size" in N.last_error()
    assert lib.jsp_index_thumb_size(idx._h, 8, None, C.byref(hv)) != 0
    assert lib.jsp_index_thumb_size(idx._h, 3, C.byref(wv), C.byref(hv)) != 0 and (wv.value, hv.value) == (-1, -1)
    with pytest.raises(CodecError, match="scale"):
        idx.ThumbSize(7)
    # an index of another codec; ScreenPressor
    other = make_gpu(16, w, h)
    idx._codec = other
    refused("another codec", [0], scale=8, out=out)
    sp = ScreenPressor(w, h, 24)
    idx._codec = sp
    refused("MSVideo1 only", [0], scale=8, out=out)
    idx._codec = a
    sp.StopAndClean()
    other.StopAndClean()
    # a picture too small for one thumbnail pixel at this scale
    tiny_frames, tiny_keys, _ = sg.msv1_clip(5, 12, 4, 3, bits=16, p_mix=sg.msv1_p_mix(0.5, 3.0))
    t = make_gpu(16, 12, 4)
    tiny = t.BuildIndex(tiny_frames, tiny_keys)
    assert tiny.ThumbSize(4) == (3, 1)
    for s in (8, 16):
        with pytest.raises(CodecError, match="too small") as e:
            tiny.Thumbs([0], scale=s, out=out)
        assert "index_thumbs" in str(e.value)
        with pytest.raises(CodecError, match="too small"):
            tiny.ThumbSize(s)
    tiny.close()
    t.StopAndClean()
    assert np.all(out.cpu().numpy().view(np.uint32) == POISON)
    # and the call still works; a closed index / codec raise as Show does
    got = idx.Thumbs([1, 0], scale=8, cols=2, out=out)
    assert tuple(got.shape) == (th, 2 * tw) and got.data_ptr() == out.data_ptr()
    idx.close()
    with pytest.raises(CodecError, match="index is closed"):
        idx.Thumbs([0])
    with pytest.raises(CodecError, match="index is closed"):
        idx.ThumbSize(8)
    idx2 = a.BuildIndex(frames[2:], keys[2:])
    a.StopAndClean()
    with pytest.raises(CodecError, match="codec is closed"):
        idx2.Thumbs([0])
    idx2.close()
    torch.cuda.synchronize()


_FULL = {}


def test_1080p_inter70_sixteen_frames_against_the_oracle():
    from jsplayer_amd import workloads as wl
    name = "msvideo1_16_1080p_inter70"
    if "clip" not in _FULL:                                              # (built and decoded once for both parse modes)
        c = wl.build_clips(name)[0]
        assert len(c.frames) == 512
        picks = [(k * 512) // 16 for k in range(16)]
        pics = oracle_pictures(16, wl.W, wl.H, None, c.frames, c.keys, keep=set(picks))
        _FULL["clip"], _FULL["picks"] = c, picks
        _FULL["thumbs"] = {t: tr.thumbnail(pics[t], wl.W, wl.H, 8) for t in picks}
    c, picks = _FULL["clip"], _FULL["picks"]
    codec = wl.make_codec(name, options={"msv1_parse": PARSE})
    with codec.BuildIndex(c.frames, c.keys) as idx:
        assert idx.ThumbSize(8) == (240, 135)
        order = picks[::-1]
        got = idx.Thumbs(order, scale=8, cols=4).cpu().numpy()
        want = tr.sheet([_FULL["thumbs"][t] for t in order], 4)
        assert got.shape == (4 * 135, 4 * 240)
        bad = np.argwhere(got != want)
        assert len(bad) == 0, f"{len(bad)} pixels differ, first at {tuple(bad[0])} ({PARSE} parse)"
    codec.StopAndClean()


def test_jsp_play_filmstrip_prints_the_crcs_of_thumbs(tmp_path):
    from jsplayer_amd import avi
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "examples", "jsp_play")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-s", "-C", os.path.join(root, "examples")])
    w, h, n = 320, 240, 40
    frames, keys, _ = sg.msv1_clip(97, w, h, n, p_mix=sg.msv1_p_mix(0.7, 6.0), key_every=16)
    path = tmp_path / "clip.avi"
    path.write_bytes(avi.write_avi(w, h, frames, fourcc=b"CRAM", bpp=16, fps=15.0, key_flags=keys))
    res = subprocess.run([exe, str(path), "--filmstrip", "9:8"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert res.returncode == 0, res.stderr.decode()
    lines = [l.split() for l in res.stdout.decode().splitlines() if l and l[0].isdigit()]
    picks = [(k * n) // 9 for k in range(9)]
    assert [int(l[0]) for l in lines] == picks
    g = make_gpu(16, w, h)
    with g.BuildIndex(frames, keys) as idx:
        tw, th = idx.ThumbSize(8)
        thumbs = idx.Thumbs(picks, scale=8, cols=1).cpu().numpy().reshape(9, th * tw)
    g.StopAndClean()
    assert [l[1] for l in lines] == ["%08x" % (zlib.crc32(thumbs[k].tobytes()) & 0xFFFFFFFF) for k in range(9)]
    # the option goes alone and checks its arguments
    for extra in (["--filmstrip", "0"], ["--filmstrip", "4", "--step-back"]):
        assert subprocess.run([exe, str(path)] + extra, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120).returncode == 2
