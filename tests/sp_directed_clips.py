"""Directed clips for the ScreenPressor seek index (a helper module, no tests of its own): clips PAINTED so that every bitmap
word, key-frame position, walk depth and rectangle shape the index kernels compute with is fixed by hand, and so that every pixel
names the frame that wrote it last.

streamgen.SpEncoder codes, per 16x16 block, exactly the bounding box of the pixels that differ from the picture before
(gen/sp_encoder.cpp), and with no hints it codes nothing as motion.  A frame's colours differ from those of every other frame at
every pixel, so painting a region in frame t makes the encoder emit precisely that region as block rectangles of frame t.

The colouring: frame t gives pixel i (row-major index) the value (t << 16) | i at 24 bpp.  At 16 bpp a pixel is three 5-bit
components, one per byte; they hold t (8 bits) and 7 bits of i:
    byte 0 = t & 31,   byte 1 = (t >> 5) | ((s & 3) << 3),   byte 2 = s >> 2,   s = (i ^ (i >> 7)) & 127.
A coded key frame at k paints the whole picture with k's colours.  A flat key frame is one colour: (t << 16) | 0xFFFF at 24 bpp
(no pixel index is that large here).  At 16 bpp a flat key frame's colour is two stream bytes, of which the first is the frame
header; the encoder takes bits 8..14 of the colour it is given, so t (< 128) goes there and the decoder's picture holds
byte 2 = (t >> 2) << 3, byte 1 = (t & 3) << 6 and a byte 0 above 31, which no painted pixel has.

The block roles of an inter frame t (nbx blocks to a row, nby rows of blocks):
    0                 one pixel, at position (7 t) % 256 of the block: a 1x1 rectangle in every frame, never covered
    1                 row t % 16: covered after 16 writers, older ones left below
    2                 column 0 when t % 32 == 0, column 15 when t % 32 == 31
    3                 never written
    4                 the whole block at frames 40, 100 and 129
    nbx - 1           rows 3..8 over its whole width when t % 5 == 0 (the partial block at the right edge)
    (nby - 1) * nbx   2x2 at its top-left corner when t % 3 == 0, 2x2 in the picture's last two rows (columns 14, 15) when
                      t % 3 == 1 (the partial block at the bottom edge)
    nbx + 1           5x5 at offset (t % 11, t % 11), in bitmap words 1 and 3 only, at bits 10..18
"""
from __future__ import annotations

from functools import lru_cache
from typing import Dict, List, Tuple

import numpy as np

import sp_index_ref as ref
from jsplayer_amd import streamgen as sg

N = 140                      # five bitmap words, the last one holding 12 frames
KEY_ROW = 5                  # key frames: pixels from this row on decide the verdict; also the codec's Preinit lines
REPAINTS = (40, 100, 129)    # block 4

# name: (width, height, bpp, version, coded key frames, flat key frames)
SPECS = {
    "A": (84, 36, 24, 4, (0, 31, 32, 96), (63,)),   # 6x3 blocks, the right one 4 pixels wide, the bottom row 4 high: the vector path
    "B": (83, 36, 24, 3, (0,), ()),                 # X % 4 != 0: the scalar path, the right block 3 pixels wide, one key frame
    "C": (84, 36, 16, 2, (0, 64), (33,)),           # the range coder, 16 bpp
}


def geometry(w: int, h: int) -> Tuple[int, int]:
    return (w + 15) // 16, (h + 15) // 16


def colours(t: int, w: int, h: int, bpp: int) -> np.ndarray:
    """Frame t's colouring of the whole picture, (h, w) uint32."""
    i = np.arange(w * h, dtype=np.uint32)
    if bpp == 16:
        s = (i ^ (i >> 7)) & 127
        v = np.uint32(t & 31) | ((np.uint32(t >> 5) | ((s & 3) << 3)) << 8) | ((s >> 2) << 16)
    else:
        assert w * h < 0xFFFF
        v = np.uint32(t << 16) | i
    return v.astype(np.uint32).reshape(h, w)


def flat_request(t: int, bpp: int) -> int:
    """The colour to hand SpEncoder.encode_flat for a flat key frame at t."""
    if bpp == 16:
        assert t < 128
        return t << 8
    return (t << 16) | 0xFFFF


def writer_of(value: int, bpp: int) -> int:
    """The frame that painted a pixel of this value."""
    value = int(value)
    if bpp == 16:
        b0, b1, b2 = value & 0xFF, (value >> 8) & 0xFF, (value >> 16) & 0xFF
        if b0 > 31:                                   # a flat key frame's colour
            return ((b2 >> 3) << 2) | (b1 >> 6)
        return (b0 & 31) | ((b1 & 7) << 5)
    return (value >> 16) & 0xFF


def describe_mismatch(got, want, w: int, h: int, bpp: int) -> str:
    """'' when the pictures are equal, else where the first wrong pixel is and which frames wrote the two values."""
    got = np.asarray(got).reshape(-1).view(np.uint32)
    want = np.asarray(want).reshape(-1).view(np.uint32)
    bad = np.nonzero(got != want)[0]
    if len(bad) == 0:
        return ""
    nbx, _ = geometry(w, h)
    y, x = divmod(int(bad[0]), w)
    return "%d pixels differ, first in block %d, row %d, col %d: want writer frame %d, got frame %d (want 0x%08x, got 0x%08x)" % (
        len(bad), (y // 16) * nbx + x // 16, y % 16, x % 16, writer_of(want[bad[0]], bpp), writer_of(got[bad[0]], bpp),
        int(want[bad[0]]), int(got[bad[0]]))


def regions(t: int, w: int, h: int) -> Dict[int, Tuple[int, int, int, int]]:
    """What inter frame t paints: {block: (x1, y1, x2, y2) inside the block} — at most one rectangle a block, as the encoder codes."""
    nbx, nby = geometry(w, h)
    pw, ph = w - 16 * (nbx - 1), h - 16 * (nby - 1)   # the partial blocks' width and height
    out = {}
    p = (7 * t) % 256
    out[0] = (p % 16, p // 16, p % 16 + 1, p // 16 + 1)
    out[1] = (0, t % 16, 16, t % 16 + 1)
    if t % 32 == 0:
        out[2] = (0, 0, 1, 16)
    elif t % 32 == 31:
        out[2] = (15, 0, 16, 16)
    if t in REPAINTS:
        out[4] = (0, 0, 16, 16)
    if t % 5 == 0:
        out[nbx - 1] = (0, 3, pw, 9)
    if t % 3 == 0:
        out[(nby - 1) * nbx] = (0, 0, 2, 2)
    elif t % 3 == 1:
        out[(nby - 1) * nbx] = (14, ph - 2, 16, ph)
    if (t >> 5) in (1, 3) and 10 <= (t & 31) <= 18:
        o = t % 11
        out[nbx + 1] = (o, o, o + 5, o + 5)
    return out


def paint(before: np.ndarray, t: int, w: int, h: int, bpp: int, skip=()) -> np.ndarray:
    """The picture of inter frame t: `before` with frame t's regions in frame t's colours.  `skip`: blocks whose role is left out
    (for the test that the census notices a missing role)."""
    nbx, _ = geometry(w, h)
    c = colours(t, w, h, bpp)
    out = before.copy()
    for b, (x1, y1, x2, y2) in regions(t, w, h).items():
        if b in skip:
            continue
        by, bx = divmod(b, nbx)
        ys, xs = slice(by * 16 + y1, by * 16 + y2), slice(bx * 16 + x1, bx * 16 + x2)
        out[ys, xs] = c[ys, xs]
    return out


def build(name: str, skip=()) -> ref.Clip:
    """Clip A, B or C: encoded with no hints, so every changed block is coded as literals of its bounding box."""
    w, h, bpp, version, coded, flat = SPECS[name]
    enc = sg.SpEncoder(w, h, bpp, version)
    chunks: List[bytes] = []
    keys: List[bool] = []
    frames: List[np.ndarray] = []
    coded_as: List[np.ndarray] = []
    pic = None
    for t in range(N):
        if t in coded:
            pic = colours(t, w, h, bpp)
            chunks.append(enc.encode_i(pic))
        elif t in flat:
            chunks.append(enc.encode_flat(flat_request(t, bpp)))
            pic = enc.current().reshape(h, w).copy()
            assert len(np.unique(pic)) == 1 and writer_of(pic[0, 0], bpp) == t
        else:
            pic = paint(pic, t, w, h, bpp, skip)
            chunks.append(enc.encode_p(pic))
        keys.append(t in coded or t in flat)
        frames.append(pic.reshape(-1).astype(np.uint32))
        coded_as.append(enc.current())
    enc.close()
    out = ref.Clip(f"directed_{name}_v{version}_{bpp}bpp_{w}x{h}", w, h, bpp, version, KEY_ROW, chunks, keys, frames)
    out.encoder_frames = coded_as          # what the encoder says a decoder holds; `frames` is what was painted
    return out


@lru_cache(maxsize=None)
def clip(name: str) -> ref.Clip:
    """The clip, built once a process; nobody changes it."""
    return build_saturated() if name == "S" else build(name)


@lru_cache(maxsize=None)
def oracle(name: str):
    """(pictures, verdicts) of the oracle's sequential run over the clip, once a process."""
    return ref.oracle_run(clip(name), preinit=KEY_ROW)


WHITE, MAGENTA, GREEN, BLACK = 0x00FFFFFF, 0x00FF00FF, 0x0000FF00, 0x00000000


def build_saturated() -> ref.Clip:
    """Clip S, for the thumbnails' channel sums: 64x48 (4x3 blocks), a white key picture and three inter frames that repaint whole
    blocks with saturated colours.  From frame 1 on, block 0 is magenta beside a black (frames 1, 2) or white (frame 3) block 1,
    and from frame 2 on block 2 is green beside the white block 3: R, G and B each meet 0 and 255 in neighbouring cells at every
    scale, and a sum that carried into the field above it would show."""
    w, h = 64, 48
    enc = sg.SpEncoder(w, h, 24, 4)
    pic = np.full((h, w), WHITE, dtype=np.uint32)
    chunks, frames = [enc.encode_i(pic)], [pic.reshape(-1).copy()]
    coded_as = [enc.current()]
    for paints in ({0: MAGENTA, 1: BLACK, 5: GREEN}, {2: GREEN, 6: BLACK}, {1: WHITE, 9: MAGENTA}):
        pic = pic.copy()
        for b, colour in paints.items():
            by, bx = divmod(b, 4)
            pic[by * 16:by * 16 + 16, bx * 16:bx * 16 + 16] = colour
        chunks.append(enc.encode_p(pic))
        frames.append(pic.reshape(-1).copy())
        coded_as.append(enc.current())
    enc.close()
    out = ref.Clip("directed_S_v4_24bpp_64x48", w, h, 24, 4, KEY_ROW, chunks, [True, False, False, False], frames)
    out.encoder_frames = coded_as
    return out


# The runs of jsp_sp_index_play the tests play: (first, count, stride).
CROSSINGS = (30, 31, 32, 33, 62, 63, 64, 94, 95, 96, 97, 127, 128)
STRIDES = (1, 2, 31, 32, 33, 64)


def play_runs(n: int = N) -> List[Tuple[int, int, int]]:
    runs = [(0, n, 1)]
    runs += [(first, min(6, n - first), 1) for first in range(n)]
    runs += [(first, (n - 1 - first) // stride + 1, stride) for first in CROSSINGS for stride in STRIDES]
    runs += [(0, 2, n - 1), (n - 1, 1, 1)]
    return runs
