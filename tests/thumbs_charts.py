"""Chart clips for the filmstrip kernels (msv1_index_thumbs_kernel, sp_index_thumbs_kernel): key frames that put a PRESCRIBED SUM into
every s x s cell, so that exact ties, saturated cells and a non-zero top byte are there by construction and not by chance.  A plain
helper module (numpy only, no tests of its own).

A chart of scale C (4, 8, 16) numbers the C x C cells of the block grid in raster order, partial cells at the right and bottom
included.  Cell c holds K = LADDER[C][c mod len] pixels of colour A, the rest B.  K is spread over the cell's (C / 4)^2 blocks as evenly
as possible, the extra going to the first blocks in raster order; a block with k A-pixels has them at its k lowest flag bits (bit
4 y + x of the 2-colour code: k <= 15, so bit 15 stays clear and the code stays a 2-colour code).  A and B differ by one step of the
format in every channel (R and B up, G down), so a cell's sum is `s * s * B + K` steps and K alone decides the rounding.

The extremes frame is a chequerboard of 16 x 16 cells, the format's brightest value against 0.

census() says what a picture holds at a scale; lanes() what a launch of msv1_index_thumbs_kernel looks like at a size."""
from __future__ import annotations

from functools import lru_cache
from typing import Dict, List, Tuple

import numpy as np

import msv1_range_clips as rc
import sp_index_ref as ref
import thumbs_ref as tr
from jsplayer_amd import streamgen as sg

LADDER = {
    4: (0, 1, 7, 8, 9, 15),
    8: (0, 1, 4, 28, 31, 32, 33, 36, 60),                  # 4, 28, 36: the 16-bit ties (bytes move in steps of 8: K = 4 mod 8)
    16: (0, 1, 16, 112, 127, 128, 129, 144, 240),          # 16, 112, 144: the 16-bit ties (K = 16 mod 32)
}
CHARTS = (4, 8, 16)
FRAME_NAMES = ("chart4", "chart8", "chart16", "extremes", "inter")
EXTREMES_AT, INTER_AT = 3, 4
WG = 256                                                   # work-items of a workgroup of msv1_index_thumbs_kernel

# the smallest pictures whose launch crosses a workgroup at every scale (lanes(); tests/test_thumbs_charts_cpu.py asserts the table)
MSV1_SIZES = [(86, 70), (128, 64), (12, 520)]


def valid_scales(w: int, h: int) -> Tuple[int, ...]:
    return tuple(s for s in tr.SCALES if min(tr.thumb_size(w, h, s)) > 0)


# ---- the charts, as masks over the picture --------------------------------------------------------------------------------------
def block_counts(w: int, h: int, c: int) -> np.ndarray:
    """(nby, nbx): the A-pixels of every whole 4x4 block of chart c."""
    nbx, nby = w // 4, h // 4
    g = c // 4
    ncx = -(-nbx // g)
    by, bx = np.mgrid[0:nby, 0:nbx]
    cell = (by // g) * ncx + bx // g
    k = np.asarray(LADDER[c])[cell % len(LADDER[c])]
    j = (by % g) * g + bx % g                              # the block's place in its cell, raster order
    return k // (g * g) + (j < k % (g * g))


def chart_mask(w: int, h: int, c: int) -> np.ndarray:
    """(h, w) bool: the pixels of colour A.  Pixels outside the whole 4x4 blocks are B."""
    k = block_counts(w, h, c)
    nby, nbx = k.shape
    y, x = np.mgrid[0:4 * nby, 0:4 * nbx]
    out = np.zeros((h, w), dtype=bool)
    out[:4 * nby, :4 * nbx] = (4 * (y % 4) + x % 4) < k[y // 4, x // 4]
    return out


def extremes_mask(w: int, h: int) -> np.ndarray:
    """(h, w) bool: the bright pixels of the extremes frame (inside the whole 4x4 blocks)."""
    nbx, nby = w // 4, h // 4
    y, x = np.mgrid[0:4 * nby, 0:4 * nbx]
    out = np.zeros((h, w), dtype=bool)
    out[:4 * nby, :4 * nbx] = (x // 16 + y // 16) % 2 == 0
    return out


# ---- MSVideo1 ---------------------------------------------------------------------------------------------------------------------
PAL_ZERO, PAL_A, PAL_B, PAL_BRIGHT = 0, 1, 2, 3            # entries of the 8-bit palette
WORD_A8, WORD_B8 = 0xFFFF0080, 0x00FE017F                  # R 255 / 254, G 0 / 1, B 128 / 127; A's top byte is 0xFF


def msv1_palette() -> bytes:
    """256 little-endian words; the four entries the charts use, the rest a ramp nobody shows."""
    pal = np.array([(i * 0x010305) & 0xFFFFFF for i in range(256)], dtype="<u4")
    pal[[PAL_ZERO, PAL_A, PAL_B, PAL_BRIGHT]] = [0, WORD_A8, WORD_B8, 0x00FFFFFF]
    return pal.tobytes()


def msv1_values(bits: int) -> Dict[str, int]:
    """What the stream names (a, b, bright, dark), the words they decode to, and the largest byte of the format."""
    if bits == 8:
        return dict(a=PAL_A, b=PAL_B, bright=PAL_BRIGHT, dark=PAL_ZERO, word_a=WORD_A8, word_b=WORD_B8, word_bright=0x00FFFFFF, top=255)
    a, b = (31 << 10) | (0 << 5) | 16, (30 << 10) | (1 << 5) | 15
    return dict(a=a, b=b, bright=0x7FFF, dark=0, word_a=0x00F80080, word_b=0x00F00878, word_bright=0x00F8F8F8, top=248)


def msv1_chart_codes(g: rc.Idle, c: int) -> List[bytes]:
    v = msv1_values(g.bits)
    codes = []
    for k in block_counts(g.w, g.h, c).reshape(-1):
        if k == 0 and g.bits == 8:                          # (a 2-colour code with flags 0 is the 8-bit end marker)
            codes.append(g.solid(v["b"]))
        else:
            codes.append(g.two(v["a"], v["b"], flags=(1 << int(k)) - 1))
    return codes


def msv1_extremes_codes(g: rc.Idle) -> List[bytes]:
    v = msv1_values(g.bits)
    bright = extremes_mask(g.w, g.h)[0:4 * g.nby:4, 0:4 * g.nbx:4].reshape(-1)
    return [g.solid(v["bright"] if on else v["dark"]) for on in bright]


@lru_cache(maxsize=None)
def msv1_chart_clip(bits: int, w: int, h: int):
    """(frames, keys, palette): chart(4), chart(8), chart(16) and the extremes as key frames, then an inter frame that recodes every
    third block as chart(16) has it — index frames whose last writer differs from block to block."""
    g = rc.Idle(bits, w, h, 0)
    charts = {c: msv1_chart_codes(g, c) for c in CHARTS}
    frames = [g.encode(charts[c]) for c in CHARTS] + [g.encode(msv1_extremes_codes(g))]
    frames.append(g.encode([code if b % 3 == 0 else None for b, code in enumerate(charts[16])]))
    return frames, [True] * 4 + [False], msv1_palette() if bits == 8 else None


def msv1_chart_pictures(bits: int, w: int, h: int) -> List[np.ndarray]:
    """What the clip's frames show, from the masks (zero-started buffers: the pixels outside the block grid are 0)."""
    v = msv1_values(bits)
    grid = np.zeros((h, w), dtype=bool)
    grid[:4 * (h // 4), :4 * (w // 4)] = True
    pics = [np.where(chart_mask(w, h, c), v["word_a"], np.where(grid, v["word_b"], 0)).astype(np.uint32) for c in CHARTS]
    pics.append(np.where(extremes_mask(w, h), v["word_bright"], 0).astype(np.uint32))
    third = np.zeros((h, w), dtype=bool)
    blocks = (np.arange((h // 4) * (w // 4)) % 3 == 0).reshape(h // 4, w // 4)
    third[:4 * (h // 4), :4 * (w // 4)] = np.kron(blocks, np.ones((4, 4), dtype=bool))
    pics.append(np.where(third, pics[2], pics[3]).astype(np.uint32))
    return [p.reshape(-1) for p in pics]


# ---- ScreenPressor --------------------------------------------------------------------------------------------------------------
# name: (width, height, bpp, entropy version); 48x32: whole blocks, the vector path; 37x23: the scalar path, partial blocks
SP_SPECS = {
    "48x32_24": (48, 32, 24, 4),
    "37x23_24": (37, 23, 24, 2),
    "48x32_16": (48, 32, 16, 3),
    "37x23_16": (37, 23, 16, 2),
}
SP_NAMES = tuple(SP_SPECS)
SP_KEY_ROW = 5
SP_RECT = (10, 10, 22, 22)                                 # x1, y1, x2, y2 of the inter frame's repaint: it crosses four 16x16 blocks


def sp_values(bpp: int) -> Dict[str, int]:
    """At 16 bpp a pixel is three 5-bit components, one per byte."""
    if bpp == 16:
        return dict(word_a=0x1F0010, word_b=0x1E010F, word_bright=0x1F1F1F, top=31)
    return dict(word_a=0xFF0080, word_b=0xFE017F, word_bright=0xFFFFFF, top=255)


def sp_chart_pictures(w: int, h: int, bpp: int) -> List[np.ndarray]:
    v = sp_values(bpp)
    pics = [np.where(chart_mask(w, h, c), v["word_a"], v["word_b"]).astype(np.uint32) for c in CHARTS]
    pics.append(np.where(extremes_mask(w, h), v["word_bright"], 0).astype(np.uint32))
    x1, y1, x2, y2 = SP_RECT
    inter = pics[EXTREMES_AT].copy()
    inter[y1:y2, x1:x2] = pics[0][y1:y2, x1:x2]
    pics.append(inter)
    return pics


@lru_cache(maxsize=None)
def sp_chart_clip(name: str) -> ref.Clip:
    """The clip, built once a process; nobody changes it.  `frames` are the encoder's own pictures."""
    w, h, bpp, version = SP_SPECS[name]
    enc = sg.SpEncoder(w, h, bpp, version)
    chunks, frames = [], []
    for t, pic in enumerate(sp_chart_pictures(w, h, bpp)):
        chunks.append(enc.encode_i(pic) if t != INTER_AT else enc.encode_p(pic))
        assert np.array_equal(enc.current(), pic.reshape(-1)), (name, t)
        frames.append(pic.reshape(-1).astype(np.uint32))
    enc.close()
    return ref.Clip(f"charts_{name}_v{version}", w, h, bpp, version, SP_KEY_ROW, chunks, [t != INTER_AT for t in range(len(chunks))], frames)


# ---- what a picture holds ---------------------------------------------------------------------------------------------------------
def census(picture, w: int, h: int, s: int, top: int = 255) -> Dict[str, object]:
    """Per channel ("r", "g", "b"): how many whole cells of scale s have a sum whose remainder mod s * s is exactly s * s / 2 (tie),
    non-zero and below it (below), above it (above), and how many have every byte at `top`, the format's maximum (full).
    "top_byte": a covered pixel's top byte is non-zero.  "full_beside_zero": a cell with every byte of every channel at `top` has a
    4-neighbour whose bytes are all 0."""
    tw, th = tr.thumb_size(w, h, s)
    assert tw > 0 and th > 0
    pic = np.asarray(picture).reshape(-1).view(np.uint32).reshape(h, w)[:th * s, :tw * s].astype(np.int64)
    n = s * s
    out: Dict[str, object] = {}
    full, zero = np.ones((th, tw), dtype=bool), np.ones((th, tw), dtype=bool)
    for name, pos in (("r", 16), ("g", 8), ("b", 0)):
        c = ((pic >> pos) & 0xFF).reshape(th, s, tw, s).sum(axis=(1, 3))
        rem = c % n
        out[name] = dict(tie=int((rem == n // 2).sum()), below=int(((rem > 0) & (rem < n // 2)).sum()), above=int((rem > n // 2).sum()),
                         full=int((c == top * n).sum()))
        full &= c == top * n
        zero &= c == 0
    out["top_byte"] = bool((pic >> 24).any())
    out["full_beside_zero"] = bool((full[:, :-1] & zero[:, 1:]).any() or (full[:, 1:] & zero[:, :-1]).any() or
                                   (full[:-1] & zero[1:]).any() or (full[1:] & zero[:-1]).any())
    return out


def lanes(w: int, h: int, s: int) -> Dict[str, object]:
    """The launch of msv1_index_thumbs_kernel for one thumbnail: work-items (a lane per block of every whole output pixel),
    workgroups of 256, whether the last one is partly filled, whether a workgroup boundary falls inside a thumbnail row."""
    tw, th = tr.thumb_size(w, h, s)
    gg = (s // 4) ** 2
    n = tw * th * gg
    wgs = -(-n // WG)
    inside = any((WG * k // gg) % tw != 0 for k in range(1, wgs))
    return dict(lanes=n, workgroups=wgs, partial_tail=n % WG != 0, seam_inside_row=inside)
