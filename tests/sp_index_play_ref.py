"""Reference for playback from the ScreenPressor seek index (jsp_sp_index_play): a numpy model of the FORWARD walk, over the same
host-stage records as sp_index_ref.Composer.

sp_index_play_kernel composes frame `first` backwards (Composer.picture), keeps the pixels and walks forward: a frame that changes
the block lays its literal rectangles over them, a key frame (coded or flat) replaces them with its key picture, any other frame
leaves them alone; every stride-th frame is emitted.  Like the kernel, `play` reads the frames 32 to a word — which of them write,
which are key frames, which are emitted — and visits only those.  The claim it pins: carrying pixels forward equals the backward
walk at every frame.
"""
from __future__ import annotations

from typing import List

import numpy as np

import sp_index_ref as ref


def play(comp: ref.Composer, first: int, n: int, stride: int = 1) -> List[np.ndarray]:
    """The pictures of frames first, first + stride, ..., first + (n - 1) * stride, walked forward from frame `first`."""
    keys = comp.clip.keys
    assert n >= 1 and stride >= 1 and 0 <= first and first + (n - 1) * stride < len(keys)
    last = first + (n - 1) * stride
    px = comp.picture(first).reshape(comp.clip.h, comp.clip.w).copy()
    out = [px.reshape(-1).copy()]
    next_out = first + stride
    for w in range(first >> 5, (last >> 5) + 1):
        lo, hi = max(first + 1, 32 * w), min(last, 32 * w + 31)
        if lo > hi:
            continue
        in_range = (0xFFFFFFFF << (lo & 31)) & (0xFFFFFFFF >> (31 - (hi & 31))) & 0xFFFFFFFF
        m = sum(1 << (f & 31) for f in range(32 * w, min(32 * w + 32, len(keys))) if f in comp.mask) & in_range
        km = sum(1 << (f & 31) for f in range(32 * w, min(32 * w + 32, len(keys))) if keys[f]) & in_range
        om = 0
        f = next_out
        while f <= hi:
            om |= 1 << (f & 31)
            f += stride
        assert not (m & km), "a key frame sets no bitmap bit"
        ev = m | km | om
        while ev:
            bit = (ev & -ev).bit_length() - 1
            ev &= ev - 1
            f = 32 * w + bit
            if (m >> bit) & 1:
                px[comp.mask[f]] = comp.lit[f][comp.mask[f]]
            elif (km >> bit) & 1:
                px = comp.key_pic[f].copy()
            if (om >> bit) & 1:
                assert f == next_out
                out.append(px.reshape(-1).copy())
                next_out += stride
    assert len(out) == n
    return out
