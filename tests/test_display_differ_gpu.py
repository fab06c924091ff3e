"""display_convert_kernel and frames_differ_kernel (jsplayer_amd/csrc/display_kernels.hip) at their vector / scalar seams, on an MI355X.

Truth: tests/display_ref.py (convert_ref, differ_ref: the header's description in numpy).  Every comparison is bit-exact, nothing
is sampled.  The cases are display_ref.DIFFER_CASES / CONVERT_CASES; tests/test_display_ref_cpu.py shows what they reach (which
loop, vector component, grid-stride iteration and lane reads the one differing pixel; which path and how many workgroups a row)
and that each of the kernels' possible mistakes named there gives a wrong answer on them.

Pointer offsets are made by slicing one over-allocated tensor; every buffer handed to the calls is a device tensor."""
import itertools
import threading

import numpy as np
import pytest

import display_ref as dr
from jsplayer_amd import _native as N
from jsplayer_amd import codec as cm

pytestmark = pytest.mark.gpu


def to_dev(a):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).cuda()
    assert t.data_ptr() % 16 == 0
    return t


def host(t):
    return t.cpu().numpy().view(np.uint32)


def xor_bit(t, index, bit):
    """One bit of one pixel of a device tensor, flipped (twice: restored)."""
    t[index] ^= (-2 ** 31 if bit == 31 else 1 << bit)


# ---- frames_differ ------------------------------------------------------------------------------------------------------------------
def _run_differ_cases(cases, pad):
    """Every case, grouped by pointer offsets: A and B hold the same pixels at their offsets; the poke goes into B (and into the host
    copy differ_ref reads) and is taken back when the next case pokes elsewhere."""
    import torch
    checked = 0
    for (oa, ob), group in itertools.groupby(cases, key=lambda c: (c.off_a, c.off_b)):
        group = list(group)
        n_max = max(c.n for c in group)
        pixels = dr.random_words(n_max, 11 + oa + 4 * ob)
        A, B = np.zeros(n_max + pad, np.uint32), np.zeros(n_max + pad, np.uint32)
        A[oa:oa + n_max] = pixels
        B[ob:ob + n_max] = pixels
        dA, dB = to_dev(A), to_dev(B)
        a, b = dA[oa:oa + n_max], dB[ob:ob + n_max]
        assert (a.data_ptr() - dA.data_ptr(), b.data_ptr() - dB.data_ptr()) == (4 * oa, 4 * ob)
        h_b = pixels.copy()
        poked = None
        for c in group:
            if (c.poke, c.bit) != poked:
                if poked is not None and poked[0] is not None:
                    xor_bit(b, *poked)
                    h_b[poked[0]] ^= np.uint32(1 << poked[1])
                if c.poke is not None:
                    xor_bit(b, c.poke, c.bit)
                    h_b[c.poke] ^= np.uint32(1 << c.bit)
                poked = (c.poke, c.bit)
                torch.cuda.synchronize()
            want = dr.differ_ref(pixels, h_b, c.first, c.n)
            assert want == dr.case_expect(c)
            assert cm.frames_differ(a, b, c.first, c.n) == want, c
            checked += 1
        if poked is not None and poked[0] is not None:
            xor_bit(b, *poked)
        assert np.array_equal(host(dB)[ob:ob + n_max], pixels) and np.array_equal(host(dA)[oa:oa + n_max], pixels)   # only read; pokes restored
    return checked


def test_frames_differ_every_first_and_every_poke_up_to_19_pixels():
    """n = 1 .. 19, every first in 0 .. n, every single-pixel difference and none, five pairs of pointer offsets: 14 345 calls."""
    cases = [c for c in dr.DIFFER_CASES if c.part == "exhaustive"]
    assert _run_differ_cases(cases, pad=8) == len(cases) == 14345


def test_frames_differ_where_the_capped_grid_wraps():
    """2048 * 1024 + 3 * 1024 + 7 pixels: the 2048 workgroups take a second iteration on the vector path (five on the scalar path,
    both pointers offset by one int); the one difference at each seam in turn."""
    cases = [c for c in dr.DIFFER_CASES if c.part == "wrap"]
    assert _run_differ_cases(cases, pad=8) == len(cases)
    assert sum(dr.case_expect(c) for c in cases) >= 40 and sum(c.poke is not None and not dr.case_expect(c) for c in cases) == 2


def test_frames_differ_on_a_non_default_stream():
    import torch
    n = 4 * dr.LANES * dr.VEC + 3
    pixels = dr.random_words(n, 21)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        handle = torch.cuda.current_stream().cuda_stream
        assert handle != 0
        a, b = to_dev(pixels), to_dev(pixels)
        xor_bit(b, n - 2, 0)                                  # (queued on the side stream, as the compare is)
        assert cm.frames_differ(a, b, 0, n, stream=handle) is True
        assert cm.frames_differ(a, b, n - 1, n, stream=handle) is False
        assert cm.frames_differ(a, b, 5, n - 2, stream=handle) is False
    side.synchronize()


def test_frames_differ_from_a_second_host_thread():
    """The result word is per host thread: a thread that never called before gets one of its own, and uses it twice."""
    import torch
    n = 1000
    pixels = dr.random_words(n, 22)
    a, b = to_dev(pixels), to_dev(pixels)
    xor_bit(b, 501, 31)
    torch.cuda.synchronize()
    assert cm.frames_differ(a, b, 0, n) is True
    got = []

    def work():
        try:
            got.append(cm.frames_differ(a, b, 502, n))
            got.append(cm.frames_differ(a, b, 501, n))
        except Exception as e:                                 # (an exception in a thread would otherwise pass unseen)
            got.append(e)

    t = threading.Thread(target=work)
    t.start()
    t.join()
    assert got == [False, True]
    assert cm.frames_differ(a, b, 502, n) is False


# ---- display_convert ----------------------------------------------------------------------------------------------------------------
_REFS = {}


def _source(w, h):
    return dr.random_words(w * h, 7 * w + h)


def _ref(w, h, mode, flip):
    key = (w, h, mode, flip)
    if key not in _REFS:
        _REFS[key] = dr.convert_ref(_source(w, h), w, h, mode, flip)
    return _REFS[key]


@pytest.mark.parametrize("mode", dr.MODES)
def test_display_convert_sizes_offsets_and_sentinels(mode):
    """Every width x height of CONVERT_CASES, both flips; widths divisible by 4 also with src, dst and both off their 16-byte
    boundary.  `out` lies inside a larger tensor between 16 sentinel ints on each side, which must come back intact."""
    import torch
    G = dr.GUARD
    checked = 0
    for (w, h), group in itertools.groupby([c for c in dr.CONVERT_CASES if c.mode == mode], key=lambda c: (c.w, c.h)):
        src = _source(w, h)
        d_src = {}
        for off in range(4):
            d_src[off] = to_dev(np.concatenate([np.zeros(off, np.uint32), src]))
        big = torch.empty(G + 3 + w * h + G, dtype=torch.int32, device="cuda")
        assert big.data_ptr() % 16 == 0
        for c in group:
            big.fill_(dr.SENTINEL)
            frame = d_src[c.off_src][c.off_src:]
            out = big[G + c.off_dst:G + c.off_dst + w * h]
            assert (frame.data_ptr() % 16, out.data_ptr() % 16) == (4 * c.off_src, 4 * c.off_dst)
            cm.display_convert(frame, out, w, h, c.mode, c.flip)
            got = host(big)
            lo, hi = G + c.off_dst, G + c.off_dst + w * h
            assert np.array_equal(got[lo:hi], _ref(w, h, c.mode, c.flip)), c
            assert np.all(got[:lo] == dr.SENTINEL) and np.all(got[hi:] == dr.SENTINEL), f"{c}: written outside out"
            checked += 1
        for off in range(4):
            assert np.array_equal(host(d_src[off])[off:], src)                       # the frame is only read
    assert checked == len(dr.CONVERT_CASES) // 4


def test_display_convert_in_place_without_flip():
    """out is frame: allowed without flip_rows (each pixel is read and written by the same lane)."""
    for (w, h, off) in [(1, 1, 0), (7, 3, 0), (256, 2, 0), (1028, 3, 0), (1028, 3, 1), (2052, 5, 0), (257, 5, 0)]:
        src = _source(w, h)
        for mode in dr.MODES:
            t = to_dev(np.concatenate([np.full(off, dr.SENTINEL, np.uint32), src, np.full(dr.GUARD, dr.SENTINEL, np.uint32)]))
            frame = t[off:off + w * h]
            cm.display_convert(frame, frame, w, h, mode, False)
            got = host(t)
            assert np.array_equal(got[off:off + w * h], _ref(w, h, mode, False)), (w, h, off, mode)
            assert np.all(got[:off] == dr.SENTINEL) and np.all(got[off + w * h:] == dr.SENTINEL)


def test_display_convert_on_a_non_default_stream():
    """Source written, converted and read back on the side stream."""
    import torch
    w, h = 1028, 5
    src = _source(w, h)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        handle = torch.cuda.current_stream().cuda_stream
        assert handle != 0
        d_src = to_dev(src)
        out = torch.full((w * h + dr.GUARD,), dr.SENTINEL, dtype=torch.int32, device="cuda")
        cm.display_convert(d_src, out, w, h, cm.DISPLAY_CANVAS, True, stream=handle)
        got = host(out)
    side.synchronize()
    assert np.array_equal(got[:w * h], _ref(w, h, cm.DISPLAY_CANVAS, True)) and np.all(got[w * h:] == dr.SENTINEL)


def test_display_convert_height_bound():
    """Height 65535 (the bound the header states, from HIP's documented grid-y limit) works at width 1 with the flip; one more, a
    width past the bound and the other bad arguments are refused with nothing written."""
    import torch
    G, top = dr.GUARD, dr.MAX_DIM
    src = dr.random_words(top + 1, 31)
    d_src = to_dev(src)
    big = torch.full((G + top + 1 + G,), dr.SENTINEL, dtype=torch.int32, device="cuda")
    out = big[G:G + top]
    cm.display_convert(d_src, out, 1, top, cm.DISPLAY_SETPIXELS_RGB15, True)
    got = host(big)
    assert np.array_equal(got[G:G + top], dr.convert_ref(src, 1, top, dr.SETPIXELS_RGB15, True))
    assert np.all(got[:G] == dr.SENTINEL) and np.all(got[G + top:] == dr.SENTINEL)
    big.fill_(dr.SENTINEL)
    lib = N.lib()
    f, o = d_src.data_ptr(), big.data_ptr() + 4 * G
    for (frame, dst, w, h, mode) in [(f, o, 1, top + 1, 3), (f, o, top + 1, 1, 3), (f, o, 1, 2 ** 31 - 1, 0), (f, o, 0, 1, 0), (f, o, 1, 0, 0),
                                     (f, o, -1, 1, 0), (f, o, 1, -1, 0), (f, o, 1, 1, 4), (f, o, 1, 1, -1), (None, o, 1, 1, 0), (f, None, 1, 1, 0)]:
        assert lib.jsp_display_convert(frame, dst, w, h, mode, 1, None) == N.JSP_ERROR_OCCURED, (w, h, mode)
        assert N.last_error().startswith("display_convert:"), N.last_error()
    with pytest.raises(cm.CodecError, match="^display_convert:.*65535"):
        cm.display_convert(d_src, big[G:], 1, top + 1, cm.DISPLAY_CANVAS, True)
    torch.cuda.synchronize()
    assert np.all(host(big) == dr.SENTINEL)
    assert np.array_equal(host(d_src), src)


# ---- the fused key-frame compare at its first pixel ------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["play", "pipelined"])
def test_fused_key_compare_on_either_side_of_its_first_pixel(how):
    """A 64x40 16-bit MSVideo1 clip whose key frames differ from the picture before them in ONE pixel: buffer index 36 X - 1 (the
    last one the Manager's compare leaves out), 36 X (the first one it reads), X Y - 1 (the last)."""
    import torch
    from jsplayer_amd import MSVideo1_16bit, MSVideo1_8bit, ScreenPressor, avi, player
    from test_avi_player import ORACLE_CLASSES
    w, h = dr.COMPARE_W, dr.COMPARE_H
    frames, keys, pictures, lit = dr.compare_boundary_clip()
    assert sorted(lit.values()) == [36 * w - 1, 36 * w, w * h - 1] and player.INSIGNIFICANT_LINES == dr.COMPARE_ROW == 36
    for f, index in lit.items():                             # by construction: the pictures on both sides differ in exactly that index
        assert keys[f] and not keys[f - 1] and keys[f - 2] and not keys[f + 1] and keys[f + 2]
        assert np.flatnonzero(pictures[f] != pictures[f - 1]).tolist() == [index] == np.flatnonzero(pictures[f + 2] != pictures[f + 1]).tolist()
    blob = avi.write_avi(w, h, frames, fourcc=b"CRAM", bpp=16, key_flags=keys)
    vi, got = avi.read_avi(blob)
    cpu = player.Manager(vi, player.make_decoder(vi, ORACLE_CLASSES), lambda n: np.zeros(n, dtype=np.int32))
    cpu.play(got, key_flags=keys)
    depth = 3
    dec = player.make_decoder(vi, (MSVideo1_16bit, MSVideo1_8bit, ScreenPressor))
    gpu = player.Manager(vi, dec, lambda n: torch.zeros(n, dtype=torch.int32, device="cuda"), num_buffers=player.NUM_BUFFERS + depth)
    assert gpu._fused_compare
    shown = []
    show = lambda d, buf: shown.append(host(buf).copy())
    if how == "play":
        gpu.play(got, key_flags=keys, on_frame=show)
    else:
        gpu.play_pipelined(got, depth=depth, key_flags=keys, on_frame=show)
    assert [(d.index, d.key, d.significant_changes, d.state) for d in gpu.log] == [(d.index, d.key, d.significant_changes, d.state) for d in cpu.log]
    sig = {d.index: d.significant_changes for d in gpu.log}
    assert [sig[f] for f in sorted(lit)] == [False, True, True]
    assert [sig[f + 2] for f in sorted(lit)] == [False, True, True]          # and back to the base picture: the same one pixel
    assert len(shown) == len(pictures) and all(np.array_equal(s, p) for s, p in zip(shown, pictures))
    dec.StopAndClean()
