"""What the GPU tests of jsp_index_tensor and jsp_sp_index_tensor share: the call through the C ABI into a poisoned byte buffer, the
comparison of every byte of it with tests/index_tensor_ref.tensor, the windows and the dtype / layout pairs, the rounding cases, the
cross-check on the device (Present into an int sheet, then a table lookup with torch ops) and the refusals.  A plain helper module."""
import ctypes as C
import itertools

import numpy as np
import pytest

import index_present_cases as ic
import index_present_ref as ipr
import index_tensor_ref as itr
import view_ref as vr
from jsplayer_amd import CodecError
from jsplayer_amd import _native as N
from jsplayer_amd.codec import normalisation

POISON_BYTE = 0x5A
BG = ic.BG
EXTRA = 7                                                      # elements of poison behind the tensor
PAIRS = list(itertools.product(itr.DTYPES, itr.LAYOUTS))       # the 8 (dtype, layout) pairs
SCALE, BIAS = (1.0 / 255, 0.5 / 255, 2.0), (0.0, -0.25, 1.5)   # a plain mapping, different per channel
IMAGENET = normalisation((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))


def byte_buf(nbytes, offset=0):
    """nbytes of poison on the device, `offset` bytes past a 16-byte boundary."""
    import torch
    whole = torch.full((nbytes + 32,), POISON_BYTE, dtype=torch.uint8, device="cuda")
    assert whole.data_ptr() % 16 == 0
    return whole[offset:offset + nbytes]


def floats(values):
    return None if values is None else (C.c_float * 3)(*[float(v) for v in values])


def call(fn, codec, idx, frames, out, win_w, win_h, k, dx, dy, mode, filter, dtype, layout, scale=SCALE, bias=BIAS, background=BG, out_bytes=None):
    """The C call itself (fn: "index_tensor" / "sp_index_tensor"); `out` a torch byte tensor, a numpy array or an address; CodecError
    with jsp_last_error() when it refuses."""
    arr = (C.c_int * max(len(frames), 1))(*frames)
    if isinstance(out, int):
        ptr, size = out, out_bytes
    elif isinstance(out, np.ndarray):
        ptr, size = out.ctypes.data, out.nbytes
    else:
        ptr, size = out.data_ptr(), out.numel() * out.element_size()
    rc = getattr(N.lib(), "jsp_" + fn)(codec._h, idx._h, len(frames), arr, C.c_void_p(ptr), size if out_bytes is None else out_bytes, win_w, win_h,
                                       float(k), float(dx), float(dy), mode, filter, background, dtype, layout, floats(scale), floats(bias))
    if rc != 0:
        raise CodecError(N.last_error())


def check(fn, codec, idx, pictures, picks, w, h, win_w, win_h, k, dx, dy, mode, filter, dtype, layout, scale=SCALE, bias=BIAS, offset=0, background=BG,
          what=""):
    """One call into a poisoned buffer `offset` ELEMENTS past a 16-byte boundary, EXTRA elements longer than the tensor: every byte of
    it equals the reference's — the tensor, and the poison behind it.  Returns the reference's bit patterns."""
    esize = itr.ESIZE[dtype]
    count = len(picks) * 3 * win_h * win_w
    out = byte_buf((count + EXTRA) * esize, offset * esize)
    assert out.data_ptr() % 16 == (offset * esize) % 16
    call(fn, codec, idx, picks, out, win_w, win_h, k, dx, dy, mode, filter, dtype, layout, scale, bias, background, out_bytes=count * esize)
    got = out.cpu().numpy()
    want_bits = itr.tensor([pictures[t] for t in picks], w, h, win_w, win_h, k, dx, dy, mode, filter, background, dtype, layout, scale, bias)
    want = np.concatenate([want_bits.reshape(-1).view(np.uint8), np.full(EXTRA * esize, POISON_BYTE, dtype=np.uint8)])
    bad = np.flatnonzero(got != want)
    if len(bad):
        e = int(bad[0]) // esize
        g = got[e * esize:(e + 1) * esize].tobytes().hex()
        x = want[e * esize:(e + 1) * esize].tobytes().hex()
        raise AssertionError(f"{what} {win_w}x{win_h} k={k:.4f} mode={mode} filter={filter} dtype={dtype} layout={layout} offset={offset}: {len(bad)} bytes "
                             f"differ, first in element {e} of {count} (+{EXTRA}): got {g}, want {x} (little-endian bytes)")
    return want_bits


def matrix_windows(w, h):
    """The windows every dtype, layout and filter runs on: fit (rows on 16-byte boundaries), 101 x 73 (a width that is no multiple of
    4) and twentieth (every rectangle loops over tiles)."""
    wins = {name: rest for name, *rest in ic.windows(w, h)}
    return [("fit",) + tuple(wins["fit"][:5]), ("fit101", 101, 73) + vr.view_matrix(w, h, 101, 73, 0, 0.5, 0.5), ("twentieth",) + tuple(wins["twentieth"][:5])]


def check_every_dtype_layout_and_filter(fn, codec, idx, pictures, picks, w, h, mode, what):
    for name, ww, wh, k, dx, dy in matrix_windows(w, h):
        for f in ipr.FILTERS:
            for dtype, layout in PAIRS:
                check(fn, codec, idx, pictures, picks, w, h, ww, wh, k, dx, dy, mode, f, dtype, layout, what=f"{what} {name}")


def check_the_other_windows(fn, codec, idx, pictures, picks, w, h, mode, what):
    """Every other window of index_present_cases.windows with one (dtype, layout) pair per filter, the pairs in rotation; then fit with
    `out` one element past a 16-byte boundary — element by element on a call that is otherwise vector-shaped — for every pair."""
    turn, seen = 0, set()
    for name, ww, wh, k, dx, dy, filters in ic.windows(w, h):
        if name in ("fit", "twentieth"):
            continue
        for f in filters:
            dtype, layout = PAIRS[turn % len(PAIRS)]
            turn += 3                                          # (3 and 8 are coprime: the pairs come round evenly)
            seen.add((dtype, layout))
            bits = check(fn, codec, idx, pictures, picks, w, h, ww, wh, k, dx, dy, mode, f, dtype, layout, what=f"{what} {name}")
            if name == "quirk200" and dtype == itr.U8 and layout == itr.NCHW:     # background at the left of every cell, mapped as any pixel
                assert np.all(bits[:, 0, :, :33] == (BG & 0xFF)) and np.all(bits[:, 2, :, :33] == ((BG >> 16) & 0xFF))
    assert seen == set(PAIRS)
    name, ww, wh, k, dx, dy = matrix_windows(w, h)[0]
    for i, (dtype, layout) in enumerate(PAIRS):
        check(fn, codec, idx, pictures, picks, w, h, ww, wh, k, dx, dy, mode, ipr.FILTERS[i % 3], dtype, layout, offset=1, what=f"{what} fit, out one element off")


def check_rounding(fn, codec, idx, pictures, picks, w, h, mode, what):
    """The contract's rounding cases on quirk200 (background, whose R, G, B bytes are 0x30, 0x20, 0x10, and with 0xFF000000 bytes of
    0) and fit: ties to even, overflow to infinity, the ImageNet normalisation, -0.0 as a bias."""
    wins = {name: rest for name, *rest in ic.windows(w, h)}
    one, zero = (1.0,) * 3, (0.0,) * 3
    for name in ("fit", "quirk200"):
        ww, wh, k, dx, dy = wins[name][:5]
        args = (fn, codec, idx, pictures, picks, w, h, ww, wh, k, dx, dy, mode)
        for layout in itr.LAYOUTS:
            tag = f"{what} {name}"
            bits = check(*args, ipr.BILINEAR, itr.BF16, layout, scale=one, bias=(256.0,) * 3, what=tag + " bf16 ties")
            ties = itr.tensor([pictures[t] for t in picks], w, h, ww, wh, k, dx, dy, mode, ipr.BILINEAR, BG, itr.U8, layout) & 1
            assert ties.any() and not (bits[ties == 1] & 1).any()                 # every odd byte was a tie, and went to the even neighbour
            bits = check(*args, ipr.AREA, itr.F16, layout, scale=one, bias=(2048.0,) * 3, what=tag + " f16 ties")
            bits = check(*args, ipr.NEAREST, itr.F16, layout, scale=(300.0,) * 3, bias=zero, what=tag + " f16 overflow")
            if mode == vr.CANVAS:                                                 # (RGB15 bytes end at 248 too, but a clip need not reach 219)
                assert (bits == 0x7C00).any() and (bits < 0x7C00).any()
            check(*args, ipr.AREA, itr.F32, layout, scale=IMAGENET[0], bias=IMAGENET[1], what=tag + " f32 normalised")
            check(*args, ipr.BILINEAR, itr.F16, layout, scale=IMAGENET[0], bias=IMAGENET[1], what=tag + " f16 normalised")
            for dtype in (itr.F32, itr.F16, itr.BF16):
                bits = check(*args, ipr.NEAREST, dtype, layout, scale=one, bias=(-0.0,) * 3, background=0xFF000000, what=tag + " bias -0.0")
                if name == "quirk200":
                    assert (bits == 0).any()                                      # a byte 0: 0 * 1 + -0.0 = +0.0
                check(*args, ipr.NEAREST, dtype, layout, scale=(-1.0,) * 3, bias=(-0.0,) * 3, background=0xFF000000, what=tag + " -0.0")
    ww, wh, k, dx, dy = wins["fit"][:5]
    check(fn, codec, idx, pictures, picks, w, h, ww, wh, k, dx, dy, mode, ipr.AREA, itr.U8, itr.NHWC, scale=None, bias=None, what=what + " u8 without scale and bias")


def check_against_present_on_the_device(idx, picks, w, h, mode, what):
    """Per filter: Present of the same frames into an int sheet with cols = 1, then bytes -> table lookup -> layout with torch ops on the
    GPU, the table built by the numpy rule; the result equals Tensor (the Python method: a new tensor, and the caller's)."""
    import torch
    torch_dtype = {itr.F32: torch.float32, itr.F16: torch.float16, itr.BF16: torch.bfloat16, itr.U8: torch.uint8}
    carrier = {itr.F32: torch.int32, itr.F16: torch.int16, itr.BF16: torch.int16, itr.U8: torch.uint8}
    signed = {itr.F32: np.int32, itr.F16: np.int16, itr.BF16: np.int16, itr.U8: np.uint8}
    n = len(picks)
    for name, ww, wh, k, dx, dy in matrix_windows(w, h)[:2]:
        for turn, f in enumerate(ipr.FILTERS):
            sheet = idx.Present(picks, ww, wh, k, dx, dy, mode=mode, filter=f, background=BG, cols=1)
            words = sheet.reshape(n, wh, ww)
            for dtype, layout in PAIRS[turn::3] + PAIRS[:1]:
                tab = torch.from_numpy(itr.table(dtype, SCALE, BIAS).view(signed[dtype])).cuda()
                planes = torch.stack([tab[ch][((words >> (8 * ch)) & 0xFF).long()] for ch in range(3)], dim=1)      # (n, 3, H, W)
                want = planes if layout == itr.NCHW else planes.permute(0, 2, 3, 1).contiguous()
                got = idx.Tensor(picks, ww, wh, k, dx, dy, mode=mode, filter=f, background=BG, dtype=torch_dtype[dtype], layout=("nchw", "nhwc")[layout],
                                 scale=SCALE, bias=BIAS)
                assert got.dtype == torch_dtype[dtype] and tuple(got.shape) == tuple(want.shape) and got.is_contiguous()
                assert torch.equal(got.view(carrier[dtype]), want), f"{what} {name} filter {f} dtype {dtype} layout {layout}: not Present + lookup"
                out = torch.zeros(got.numel() + 5, dtype=torch_dtype[dtype], device="cuda")
                mine = idx.Tensor(picks, ww, wh, k, dx, dy, mode=mode, filter=f, background=BG, dtype=torch_dtype[dtype], layout=("nchw", "nhwc")[layout],
                                  scale=SCALE, bias=BIAS, out=out)
                assert mine.data_ptr() == out.data_ptr() and torch.equal(mine.view(carrier[dtype]), want) and bool((out[-5:] == 0).all())


def check_refusals(fn, codec, idx, nframes, refused_kind, in_flight, other_codec, wrong_kind, wrong_prefix):
    """Every refusal of the contract leaves `out` untouched and names its call.  in_flight(): queues an asynchronous frame and returns
    what ends it."""
    ww, wh = 20, 10
    out = byte_buf(4 * 3 * ww * wh * 4)
    good = dict(frames=[0], out=out, win_w=ww, win_h=wh, k=0.5, dx=0.0, dy=0.0, mode=vr.CANVAS, filter=ipr.BILINEAR, dtype=itr.F32, layout=itr.NCHW)

    def refused(match, on=None, prefix=fn + ":", **kw):
        args = dict(good, **kw)
        with pytest.raises(CodecError, match=match) as e:
            call(fn, on or codec, idx, **args)
        assert str(e.value).startswith(prefix), str(e.value)
        assert bool((out == POISON_BYTE).all()), match + ": out was written"

    refused("1..4096", frames=[])
    refused("1..4096", frames=[0] * 4097)
    for bad in (0, -1, 16385):
        refused("window size", win_w=bad)
        refused("window size", win_h=bad)
    for bad in (1.0 / 65, 64.5, 0.0, -1.0):
        refused("k outside", k=bad)
    for name in ("k", "dx", "dy"):
        for bad in (float("nan"), float("inf"), -float("inf")):
            refused("finite", **{name: bad})
    for bad in (-1, vr.SETPIXELS, vr.SETPIXELS_RGB15, 4, 99):
        refused("mode must be", mode=bad)
    for bad in (-1, 3):
        refused("unknown filter", filter=bad)
    for bad in (-1, 4, 99):
        refused("unknown dtype", dtype=bad)
    for bad in (-1, 2):
        refused("unknown layout", layout=bad)
    for dtype in (itr.F32, itr.F16, itr.BF16):
        refused("required", dtype=dtype, scale=None)
        refused("required", dtype=dtype, bias=None)
        for bad in (float("nan"), float("inf"), -float("inf")):
            refused("must be finite", dtype=dtype, scale=(1.0, bad, 1.0))
            refused("must be finite", dtype=dtype, bias=(0.0, 0.0, bad))
    for bad in (-1, nframes, 1 << 20):
        refused("outside the index", frames=[0, bad])
    for dtype in itr.DTYPES:
        refused("smaller than the tensor", dtype=dtype, out_bytes=3 * ww * wh * itr.ESIZE[dtype] - 1)
        refused("smaller than the tensor", dtype=dtype, frames=[0, 1], out_bytes=2 * 3 * ww * wh * itr.ESIZE[dtype] - 1)
    refused("smaller than the tensor", frames=[0, 1, 2, 3, 0])                               # five cells, room for four
    refused("not aligned", out=out[2:])
    refused("not aligned", out=out[1:], dtype=itr.F16)
    refused("not aligned", out=out[1:], dtype=itr.BF16)
    host = np.full(3 * ww * wh * 4, POISON_BYTE, dtype=np.uint8)
    refused("device buffer", out=host)
    assert np.all(host == POISON_BYTE)
    done = in_flight()
    refused("in flight")
    done()
    # null arguments (the C ABI itself)
    lib = N.lib()
    one = (C.c_int * 1)(0)
    tail = (out.numel(), ww, wh, 0.5, 0.0, 0.0, 0, 1, 0, itr.F32, itr.NCHW, floats(SCALE), floats(BIAS))
    for args in ((None, idx._h, 1, one, C.c_void_p(out.data_ptr())), (codec._h, None, 1, one, C.c_void_p(out.data_ptr())),
                 (codec._h, idx._h, 1, None, C.c_void_p(out.data_ptr())), (codec._h, idx._h, 1, one, None)):
        assert getattr(lib, "jsp_" + fn)(*args, *tail) != 0 and N.last_error().startswith(fn + ": null argument")
    refused("another codec", on=other_codec)
    refused(refused_kind, on=wrong_kind, prefix=wrong_prefix)
    assert bool((out == POISON_BYTE).all())
