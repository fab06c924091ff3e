"""Directed clips for the activity map of a ScreenPressor seek index (a helper module, no tests of its own): clips whose VALUES
REPEAT, at the smallest pictures at which the lane geometry of sp_index_activity_kernel can still go wrong.

The painted clips of sp_directed_clips give every frame colours no other frame has, so every painted pixel differs from whatever
was there: a walk that never takes a literal into its register, or that counts a rectangle's area, counts the same on them.  Here
a pixel holds one of four values — A, B, 0 and the flat key frame's colour F — and what a frame codes is compared with what the
walk carried.  streamgen.SpEncoder is given no hints: it codes, per 16x16 block, exactly the bounding box of the pixels that differ.

N = 70 frames: bitmap words 0 and 1 in full, word 2 with six frames.  Key frames (KEYS): coded at 0 (its four left columns 0, the rest A),
32 (bit 0 of word 1), 40 (the picture of frame 39 again: a key event that changes nothing), 63 (bit 31 of word 1) and 64 (a key
frame right behind a key frame); flat at 20, inter frames behind it.

Every block of every clip carries every role.  A block's PART is what of it lies inside the picture, bw x bh pixels; positions
are relative to it (positions()):
    beat    the pixel ((5 b + 3) % bw, (3 b + 1) % bh) toggles in every inter frame (toggle: A becomes B, anything else A): an
            event in every inter frame and every block, and a pixel that returns to the value it held two frames before.  The key
            frames at 32 and 63 toggle it too, and leave the rest.
    far     the corner of the part farthest from the beat.  In every fifth inter frame it toggles as well: the rectangle reaches
            from the beat to it and covers pixels that stay (parts of fewer than three pixels have nothing between the two).  The
            key frame at 64 toggles it and leaves the rest.
    region  the far corner's half of its row.  Painted B at 6 (it is non-zero from there on, also where frame 0 left zeros), 0 at
            ZERO_AT — over non-zero pixels, the beat included where it lies inside: every pixel of it counts — and A again at
            RESTORE_AT (the beat keeps its toggle there: it must change in every inter frame).  The zeros of 31 and 62 are carried
            through the key frames at 32, and at 63 and 64.
In a part of one pixel the three are the same pixel: it toggles, goes to 0 at ZERO_AT and toggles on from there."""
from __future__ import annotations

from functools import lru_cache
from typing import Dict, List, Tuple

import numpy as np

import index_activity_ref as ar
import sp_index_ref as ref
from jsplayer_amd import streamgen as sg

N = 70
KEY_ROW = 5                                   # key frames: pixels from this row on decide the verdict; also the codec's Preinit lines
FLAT_AT = 20
REPEAT_AT = 40                                # a coded key frame that repeats the picture before it
BEAT_KEYS, FAR_KEY = (32, 63), 64             # coded key frames that toggle the beat / the far pixel of every block
KEYS = (0, FLAT_AT, 32, REPEAT_AT, 63, 64)
HOLES_EVERY = 5
PAINT_B_AT = (6,)
ZERO_AT = (8, 23, 31, 46, 62)
RESTORE_AT = (11, 26, 33, 48, 66)
ZERO_COLUMNS = 4                              # frame 0: columns 0..3 are 0 (a part of every block of the first column is not)

# name: (width, height, bpp, entropy version)
SPECS = {
    "17x17": (17, 17, 24, 4),    # 2x2 blocks, X % 16 = 1: the scalar path, the edge block one pixel wide and one high
    "66x20": (66, 20, 24, 3),    # nbx = 5 (nbx % 4 = 1), X % 16 = 2
    "79x33": (79, 33, 16, 2),    # X % 16 = 15, Y % 16 = 1, the range coder, 16 bpp
    "72x16": (72, 16, 24, 4),    # the vector path, X % 16 = 8, nby = 1
    "13x9": (13, 9, 24, 2),      # one block: waves 1..3 of the only workgroup leave; chunk 3 has one pixel
}
NAMES = tuple(SPECS)
SCALAR = tuple(n for n in NAMES if SPECS[n][0] % 4)


def values(bpp: int) -> Tuple[int, int]:
    """(A, B): at 16 bpp a pixel is three 5-bit components, one per byte."""
    return (0x0A141E, 0x1F0001) if bpp == 16 else (0xA1B2C3, 0x00FF01)


def flat_request(bpp: int) -> int:
    """The colour handed to SpEncoder.encode_flat (sp_directed_clips.flat_request: at 16 bpp the encoder takes bits 8..14)."""
    return 77 << 8 if bpp == 16 else 0xC0FFEE


def parts(w: int, h: int) -> List[Tuple[int, int, int, int]]:
    """(x, y, bw, bh) of every block's part inside the picture, in raster order of the blocks."""
    nbx, nby = ar.grid(w, h)
    return [(bx * 16, by * 16, min(16, w - bx * 16), min(16, h - by * 16)) for by in range(nby) for bx in range(nbx)]


def positions(b: int, bw: int, bh: int):
    """beat (x, y), far (x, y), region (y, x_lo, x_hi) of block b, relative to its part."""
    beat = ((5 * b + 3) % bw, (3 * b + 1) % bh)
    far = (0 if 2 * beat[0] >= bw else bw - 1, 0 if 2 * beat[1] >= bh else bh - 1)
    half = max(1, bw // 2)
    region = (far[1], 0, half) if far[0] == 0 else (far[1], bw - half, bw)
    return beat, far, region


def toggle(v, a: int, b: int):
    return b if int(v) == a else a


def paint(before: np.ndarray, t: int, w: int, h: int, bpp: int, skip=()) -> np.ndarray:
    """The picture of inter frame t.  `skip`: roles left out ("holes": for the test that the census notices)."""
    a, bb = values(bpp)
    out = before.copy()
    for b, (x, y, bw, bh) in enumerate(parts(w, h)):
        beat, far, (ry, rx0, rx1) = positions(b, bw, bh)
        at = (y + beat[1], x + beat[0])
        out[at] = toggle(before[at], a, bb)
        if t % HOLES_EVERY == 0 and bw * bh >= 3 and "holes" not in skip:
            at_far = (y + far[1], x + far[0])
            out[at_far] = toggle(before[at_far], a, bb)
        if t in ZERO_AT:
            out[y + ry, x + rx0:x + rx1] = 0
        elif t in PAINT_B_AT or t in RESTORE_AT:
            keep = out[at]
            out[y + ry, x + rx0:x + rx1] = bb if t in PAINT_B_AT else a
            out[at] = keep
    return out


def key_picture(before: np.ndarray, t: int, w: int, h: int, bpp: int) -> np.ndarray:
    """The picture of the coded key frame at t."""
    a, bb = values(bpp)
    if t == 0:
        out = np.full((h, w), a, dtype=np.uint32)
        out[:, :ZERO_COLUMNS] = 0
        return out
    out = before.copy()
    if t == REPEAT_AT:
        return out
    for b, (x, y, bw, bh) in enumerate(parts(w, h)):
        beat, far, _ = positions(b, bw, bh)
        px = beat if t in BEAT_KEYS else far
        out[y + px[1], x + px[0]] = toggle(before[y + px[1], x + px[0]], a, bb)
    return out


def build(name: str, skip=()) -> ref.Clip:
    w, h, bpp, version = SPECS[name]
    enc = sg.SpEncoder(w, h, bpp, version)
    chunks: List[bytes] = []
    frames: List[np.ndarray] = []
    pic = None
    for t in range(N):
        if t == FLAT_AT:
            chunks.append(enc.encode_flat(flat_request(bpp)))
            pic = enc.current().reshape(h, w).copy()
            assert len(np.unique(pic)) == 1 and int(pic[0, 0]) not in (0,) + values(bpp)
        elif t in KEYS:
            pic = key_picture(pic, t, w, h, bpp)
            chunks.append(enc.encode_i(pic))
        else:
            pic = paint(pic, t, w, h, bpp, skip)
            chunks.append(enc.encode_p(pic))
        assert np.array_equal(enc.current(), pic.reshape(-1)), (name, t)
        frames.append(pic.reshape(-1).astype(np.uint32))
    enc.close()
    return ref.Clip(f"activity_{name}_v{version}_{bpp}bpp", w, h, bpp, version, KEY_ROW, chunks, [t in KEYS for t in range(N)], frames)


@lru_cache(maxsize=None)
def clip(name: str) -> ref.Clip:
    """The clip, built once a process; nobody changes it."""
    return build(name)


@lru_cache(maxsize=None)
def oracle(name: str):
    """(pictures, verdicts) of the oracle's sequential run over the clip, once a process."""
    return ref.oracle_run(clip(name), preinit=KEY_ROW)


@lru_cache(maxsize=None)
def composer(name: str) -> ref.Composer:
    return ref.Composer(clip(name), preinit=KEY_ROW)


@lru_cache(maxsize=None)
def truth(name: str) -> np.ndarray:
    """THE DEFINITION over the oracle's pictures, all N frames: (N, rows, cols) uint16.  Nobody changes it."""
    c = clip(name)
    out = ar.activity(oracle(name)[0], np.zeros(c.w * c.h, dtype=np.uint32), c.w, c.h)
    out.setflags(write=False)
    return out


def runs(c: ref.Clip) -> List[Tuple[int, int]]:
    """The (first, n) every test walks: the ends of the bitmap words, the key frames and their neighbours."""
    n = len(c.keys)
    out = [(0, n), (0, 1), (1, 1), (1, 31), (30, 3), (31, 1), (31, 2), (32, 1), (32, 32), (33, 30), (33, 31), (39, 3), (40, 1), (41, 1),
           (64, 6), (n - 1, 1)]
    for k in (t for t in range(n) if c.keys[t]):
        out += [(k, 1), (k + 1, 1), (k - 1, 2)]
    seen, uniq = set(), []
    for first, count in out:
        if first >= 0 and first + count <= n and (first, count) not in seen:
            seen.add((first, count))
            uniq.append((first, count))
    return uniq


def census(c: ref.Clip, pictures, comp: ref.Composer) -> Dict[str, object]:
    """What the clip holds, ASSERTED: from the oracle's pictures and the masks of the host stage's records (what the kernel is given),
    not from what the painter meant.  Returns the facts it found."""
    w, h, n = c.w, c.h, len(c.keys)
    pics = [np.asarray(p).view(np.uint32).reshape(h, w) for p in pictures]
    zeros = np.zeros((h, w), dtype=np.uint32)
    diff = [pics[t] != (pics[t - 1] if t else zeros) for t in range(n)]
    changed = np.stack([ar.cell_sums(d, w, h) for d in diff])                 # (n, rows, cols)
    where = [(slice(y, y + bh), slice(x, x + bw)) for x, y, bw, bh in parts(w, h)]
    for t in range(n):
        if c.keys[t]:
            assert t not in comp.mask and comp.key_of[t] == t
            continue
        assert t in comp.mask, f"{c.name}: inter frame {t} codes nothing"
        for b, at in enumerate(where):
            assert comp.mask[t][at].any(), f"{c.name}: inter frame {t} has no event in block {b}"
            assert not (diff[t][at] & ~comp.mask[t][at]).any(), f"{c.name}: frame {t} changes a pixel of block {b} outside its rectangle"
    # a store of a frame next to a run lands in the row in front of the map or behind it only if that frame has something to store
    # (the key frame at REPEAT_AT changes nothing: in front of the run (REPEAT_AT + 1, 1) there is nothing that could be stored)
    for first, count in runs(c):
        for t in ([first - 1] if first > 0 else []) + ([first + count] if first + count < n else []):
            if t != REPEAT_AT:
                assert changed[t].all(), f"{c.name}: frame {t} beside the run ({first}, {count}) leaves a block unchanged"
    slack = {}
    for b, (at, (_, _, bw, bh)) in enumerate(zip(where, parts(w, h))):
        if bw * bh < 3:
            continue
        slack[b] = [t for t in comp.mask if (comp.mask[t][at] & ~diff[t][at]).any()]
        assert slack[b], f"{c.name}: no rectangle of block {b} covers a pixel that stays"
        wide = max(3, ((bw + 1) // 2) * ((bh + 1) // 2))      # the far corner is at least half the part away from the beat, each way
        assert any(diff[t][at].sum() == 2 and comp.mask[t][at].sum() >= wide for t in slack[b]), \
            f"{c.name}: no frame of block {b} changes just two pixels far apart"
    back = [t for t in range(2, n) if ((pics[t] == pics[t - 2]) & (pics[t] != pics[t - 1])).any()]
    assert back, f"{c.name}: no pixel returns to the value it held two frames earlier"
    assert (pics[0] == 0).any() and (pics[0] != 0).any(), f"{c.name}: frame 0 has no zeros, or nothing else"
    to_zero = [t for t in range(1, n) if ((pics[t] == 0) & (pics[t - 1] != 0)).any()]
    assert to_zero, f"{c.name}: no frame changes a pixel to 0"
    from_zero = [t for t in range(1, n) if ((pics[t] != 0) & (pics[t - 1] == 0)).any()]
    assert from_zero and max(from_zero) > min(to_zero)
    assert c.keys[REPEAT_AT] and comp.key_of[REPEAT_AT] == REPEAT_AT and not changed[REPEAT_AT].any(), f"{c.name}: frame {REPEAT_AT}"
    kinds = {t: c.chunks[t][0] & 0xF for t in range(n) if c.keys[t]}                # 1: flat, 2: coded
    assert kinds == {t: (1 if t == FLAT_AT else 2) for t in KEYS}, kinds
    for t in BEAT_KEYS + (FAR_KEY,):
        for b, at in enumerate(where):
            d = diff[t][at]
            assert d.any() and (d.size == 1 or not d.all()), f"{c.name}: key frame {t}, block {b}"
    return dict(changed=changed, slack=slack, back=back, to_zero=to_zero, coded_bytes=[len(x) for x in c.chunks])
