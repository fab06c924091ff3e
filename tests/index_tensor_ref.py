"""The numpy reference of jsp_index_tensor / jsp_sp_index_tensor (include/jsplayer_amd.h): pictures -> a dense tensor.  Cell i is the
window index_present_ref.window gives of picture i (the contract of Present); channel ch of a pixel is byte ch of its word, and the
element is that byte pushed through THE RULE of the header, stated here with numpy's IEEE arithmetic.  A plain helper module (no tests
of its own); it reads nothing from the library."""
import numpy as np

import index_present_ref as ipr

F32, F16, BF16, U8 = 0, 1, 2, 3
DTYPES = (F32, F16, BF16, U8)
NCHW, NHWC = 0, 1
LAYOUTS = (NCHW, NHWC)
ESIZE = {F32: 4, F16: 2, BF16: 2, U8: 1}
RAW = {F32: np.uint32, F16: np.uint16, BF16: np.uint16, U8: np.uint8}     # the unsigned type that holds an element's bit pattern


def bf16_bits(f):
    """float32 array -> the bfloat16 bit patterns (uint16), rounded to nearest-even from the float's bits."""
    bits = np.ascontiguousarray(f, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((bits + 0x7FFF + ((bits >> 16) & 1)) >> 16).astype(np.uint16)


def table(dtype, scale=None, bias=None):
    """(3, 256) bit patterns (RAW[dtype]): the element of byte v of channel ch.  scale and bias are rounded to float32 first, as the C
    call takes floats."""
    v = np.arange(256)
    if dtype == U8:
        return np.tile(v.astype(np.uint8), (3, 1))
    rows = []
    for ch in range(3):
        s, b = np.float32(scale[ch]), np.float32(bias[ch])
        with np.errstate(over="ignore"):
            f = np.float32(np.float64(v) * np.float64(s) + np.float64(b))
            if dtype == F32:
                rows.append(f.view(np.uint32))
            elif dtype == F16:
                rows.append(f.astype(np.float16).view(np.uint16))
            else:
                rows.append(bf16_bits(f))
    return np.stack(rows)


_WINDOWS = {}   # (id(picture), the window's arguments) -> (picture, window): the picture is held, so its id stays its own


def cached_window(picture, w, h, win_w, win_h, k, dx, dy, mode, filter, background):
    key = (id(picture), w, h, win_w, win_h, float(k), float(dx), float(dy), mode, filter, background)
    if key not in _WINDOWS:
        if len(_WINDOWS) > 400:
            _WINDOWS.clear()
        _WINDOWS[key] = (picture, ipr.window(picture, w, h, win_w, win_h, k, dx, dy, mode, filter, background))
    return _WINDOWS[key][1]


def from_windows(cells, dtype, layout, scale=None, bias=None):
    """Windows ((win_h, win_w) uint32 each) -> the tensor's bit patterns: (n, 3, win_h, win_w) or (n, win_h, win_w, 3) of RAW[dtype]."""
    tab = table(dtype, scale, bias)
    out = np.stack([np.stack([tab[ch][(cell >> (8 * ch)) & 0xFF] for ch in range(3)]) for cell in cells])
    return np.ascontiguousarray(out if layout == NCHW else out.transpose(0, 2, 3, 1))


def tensor(pictures, w, h, win_w, win_h, k, dx, dy, mode, filter, background, dtype, layout, scale=None, bias=None):
    """The tensor of `pictures` (each w * h words, bottom-up) as an array of bit patterns (RAW[dtype]; see from_windows): compare it
    with the library's bytes as it is — -0.0, ties and infinities count."""
    cells = [cached_window(p, w, h, win_w, win_h, k, dx, dy, mode, filter, background) for p in pictures]
    return from_windows(cells, dtype, layout, scale, bias)


def as_values(bits, dtype):
    """The bit patterns as numbers (float32 for the float types, bfloat16 widened exactly)."""
    if dtype == U8:
        return bits
    if dtype == F32:
        return bits.view(np.float32)
    if dtype == F16:
        return bits.view(np.float16).astype(np.float32)
    return (bits.astype(np.uint32) << 16).view(np.float32)
