"""Directed MOTION clips for the ScreenPressor inter-frame kernel, sp_pframe_kernel (a helper module, no tests of its own): clips
PAINTED by hand whose inter frames move blocks with the reference's rule (ScreenPressor.hx:400-405) — ONE linear index
(y + my) * X + x + mx into the picture before, no clipping per axis, 0 outside [0, X * Y) — so that the motion branch of the kernel,
the host stage's shadow move and its "same vector" flag, literalise_motion and the quarter rule between the two are all run on
vectors, rectangles and edges chosen on purpose.  The encoder takes a hinted vector whenever the painted target equals that move of
the picture before (gen/sp_encoder.cpp), so painting a block with `move` below and hinting its vector codes it as motion.

No two pixels of a key picture are equal, none is 0, and every literal repaint takes colours never used before in the clip
(`Colours`): an accidental match could only shrink a bounding box or spoil a vector, and the census of
tests/test_sp_motion_clips_cpu.py would say so.

    clip   size    bpp  version   what it is for
    M      76x56   24   4         X % 4 == 0, the right block 12 wide, the bottom block row 8 high: 16-byte loads and stores
    U      75x56   24   3         X % 4 != 0: the scalar arm everywhere, the right block 11 wide
    H      76x56   16   2         M's painting through the range coder: no "same vector" flag, the 16 bpp context constants
    Q      64x64   24   4         the quarter rule: 4096 pixels, 16 whole blocks
    (M2    76x56   24   2         M's painting through the range coder, for the typed-array decoder under node, which reads version 2 only)

M, U and H: 5 blocks to a row (block = 5 * block row + column), 4 block rows.  One role a frame (`table`):

    t   role       blocks (column, block row): vector
    0   key
    1   in-frame   (1,1) and (2,1): (-3,-2), the second "same as last"; (3,1) repainted; (4,1): (-3,-2) again behind the data block;
                   (1,2): (6,5); (2,2) columns 0..3: (7,-4)  — mx % 4 = 1, 2 and 3, every my != 0, every source inside the picture
    2   edges      (0,0): (-1,0), pixel (0,0) reads index -1; (4,3): (1,0), the last pixel reads index X*Y; (2,0): (2,-5), rows 0..4
                   from above the picture; (2,3): (0,3), rows 5..7 from below it; (1,1): (0,-256) and (3,1): (0,255), all outside
    3   wrap       (0,1): (-9,0), its left pixels from the end of the row above; (4,1): (9,0), its right pixels from the start of the
                   row below; (1,2): (-256,0) and (2,2): (255,1), more than three rows away and inside; (1,1), (3,1) repainted
    4   subrect    (1,1) (3,2)-(9,7): (2,1); (2,1) the pixel (5,5): (-4,3); (3,1) column 15: (1,-1); (4,1) its last three columns,
                   rows 4..8: (-6,2); (1,3) columns 2..6, rows 1..7: (3,-2); the blocks that hold zeros since t = 2 repainted
    5   scroll     every block: (-4,-1) — every source overlaps blocks this frame rewrites; row 0 from above the picture
    6   mixed      (1,1): (20,-14); (1,2) below it repainted, its top row the moved block's bottom row (left half: the pixel above,
                   right half: the pixel above-left); (2,1) right of it repainted, its column 0 the moved block's column 15;
                   (3,2) (4,4)-(8,10) repainted; (0,2): (7,-4); (1,0) repainted; the rest unchanged
    7   nothing    (src[0] == 0)
    8   carry      (2,1): (7,-4), the vector t = 6 ended with — coded in full, lastmx / lastmy restart per frame; (3,1): (7,-4)
    9   key
    10  chain      literal: (1,0) whole, (1,1) (2,3)-(10,8), (3,3) whole
    11  chain      light: (1,1), (2,1): (5,3); (0,2): (7,6) — 768 pixels
    12  chain      heavy: the 15 blocks of block rows 0..2: (-5,2) — 3648 (3600) pixels
    13  chain      literal: (2,1) whole, (2,2) (1,1)-(5,3)
    14  chain      light: (1,1), (1,2): (9,-3) — pixels the heavy frame moved

Q: t = 1 moves the four middle blocks by (3,-2): 1024 pixels = X*Y / 4, literalised; t = 2 moves the four corner blocks and the one
pixel (7,7) of block (1,1): 1025 pixels, kept.
"""
from __future__ import annotations

from functools import lru_cache
from typing import List, Tuple

import numpy as np

import sp_index_ref as ref
from jsplayer_amd import streamgen as sg

KEY_ROW = 5                  # key frames: pixels from this row on decide the verdict; also the codec's Preinit lines
PB_SUBRECT, PB_MOTION, PB_DATA = 1, 2, 4

# name: (width, height, bpp, version)
SPECS = {"M": (76, 56, 24, 4), "U": (75, 56, 24, 3), "H": (76, 56, 16, 2), "Q": (64, 64, 24, 4), "M2": (76, 56, 24, 2)}
NAMES = ("M", "U", "H", "Q")
ROLE_CLIPS = ("M", "U", "H")          # the clips that hold the catalogue of roles
ROLES = ("in-frame", "edges", "wrap", "subrect", "scroll", "mixed", "nothing", "carry", "chain")
Q_ROLES = ("quarter", "over")


def geometry(w: int, h: int) -> Tuple[int, int]:
    return (w + 15) // 16, (h + 15) // 16


def table(name: str, skip=()) -> List[Tuple[str, list]]:
    """One (role, entries) per frame.  Entries: ("move", block, rectangle or None = the whole block, (mx, my)) and
    ("lit", block, rectangle or None, echo) — a repaint with fresh colours; echo "above": the top row then repeats the row above it
    (left half) and the row above it one to the left (right half); echo "left": column 0 then repeats the column left of it.
    Rectangles are (x1, y1, x2, y2) inside the block, x2 and y2 exclusive.  `skip`: roles left out — their frames change nothing —
    for the test that the census notices a missing role."""
    w, h, _, _ = SPECS[name]
    nbx, nby = geometry(w, h)
    pw, ph = w - 16 * (nbx - 1), h - 16 * (nby - 1)

    def B(bx, by):
        return by * nbx + bx

    if name == "Q":
        frames = [
            ("key", []),
            ("quarter", [("move", B(bx, by), None, (3, -2)) for by in (1, 2) for bx in (1, 2)]),
            ("over", [("move", B(0, 0), None, (5, 4)), ("move", B(3, 0), None, (-5, 4)), ("move", B(1, 1), (7, 7, 8, 8), (2, 2)),
                      ("move", B(0, 3), None, (5, -4)), ("move", B(3, 3), None, (-5, -4))]),
        ]
    else:
        frames = [
            ("key", []),
            ("in-frame", [("move", B(1, 1), None, (-3, -2)), ("move", B(2, 1), None, (-3, -2)), ("lit", B(3, 1), None, None),
                          ("move", B(4, 1), None, (-3, -2)), ("move", B(1, 2), None, (6, 5)), ("move", B(2, 2), (0, 0, 4, 16), (7, -4))]),
            ("edges", [("move", B(0, 0), None, (-1, 0)), ("move", B(2, 0), None, (2, -5)), ("move", B(1, 1), None, (0, -256)),
                       ("move", B(3, 1), None, (0, 255)), ("move", B(2, 3), None, (0, 3)), ("move", B(4, 3), None, (1, 0))]),
            ("wrap", [("move", B(0, 1), None, (-9, 0)), ("lit", B(1, 1), None, None), ("lit", B(3, 1), None, None),
                      ("move", B(4, 1), None, (9, 0)), ("move", B(1, 2), None, (-256, 0)), ("move", B(2, 2), None, (255, 1))]),
            ("subrect", [("lit", B(0, 0), None, None), ("lit", B(2, 0), None, None), ("move", B(1, 1), (3, 2, 10, 8), (2, 1)),
                         ("move", B(2, 1), (5, 5, 6, 6), (-4, 3)), ("move", B(3, 1), (15, 0, 16, 16), (1, -1)),
                         ("move", B(4, 1), (pw - 3, 4, pw, 9), (-6, 2)), ("move", B(1, 3), (2, 1, 7, ph), (3, -2)),
                         ("lit", B(2, 3), None, None), ("lit", B(4, 3), None, None)]),
            ("scroll", [("move", b, None, (-4, -1)) for b in range(nbx * nby)]),
            ("mixed", [("lit", B(1, 0), None, None), ("move", B(1, 1), None, (20, -14)), ("lit", B(2, 1), None, "left"),
                       ("move", B(0, 2), None, (7, -4)), ("lit", B(1, 2), None, "above"), ("lit", B(3, 2), (4, 4, 9, 11), None)]),
            ("nothing", []),
            ("carry", [("move", B(2, 1), None, (7, -4)), ("move", B(3, 1), None, (7, -4))]),
            ("key", []),
            ("chain", [("lit", B(1, 0), None, None), ("lit", B(1, 1), (2, 3, 11, 9), None), ("lit", B(3, 3), None, None)]),
            ("chain", [("move", B(1, 1), None, (5, 3)), ("move", B(2, 1), None, (5, 3)), ("move", B(0, 2), None, (7, 6))]),
            ("chain", [("move", B(bx, by), None, (-5, 2)) for by in range(3) for bx in range(nbx)]),
            ("chain", [("lit", B(2, 1), None, None), ("lit", B(2, 2), (1, 1, 6, 4), None)]),
            ("chain", [("move", B(1, 1), None, (9, -3)), ("move", B(1, 2), None, (9, -3))]),
        ]
    return [(role, [] if role in skip else sorted(entries, key=lambda e: e[1])) for role, entries in frames]


def frames_of(name: str, role: str) -> List[int]:
    return [t for t, (r, _) in enumerate(table(name)) if r == role]


def role_at(c: ref.Clip, t: int) -> str:
    """The role of frame t of a clip that `build` made."""
    return table(c.name.split("_")[1])[t][0]


def block_box(b: int, w: int, h: int) -> Tuple[int, int, int, int]:
    """(x16, y16, width, height) of block b."""
    nbx, _ = geometry(w, h)
    by, bx = divmod(b, nbx)
    return bx * 16, by * 16, min(16, w - bx * 16), min(16, h - by * 16)


def rect_of(entry, w: int, h: int) -> Tuple[int, int, int, int]:
    _, _, bw, bh = block_box(entry[1], w, h)
    return tuple(entry[2]) if entry[2] is not None else (0, 0, bw, bh)


def move(before: np.ndarray, y0: int, y1: int, x0: int, x1: int, mx: int, my: int) -> np.ndarray:
    """The reference's move of the rectangle rows y0..y1-1, columns x0..x1-1: pixel (x, y) takes index (y + my) * X + x + mx of the
    picture before, 0 outside the buffer."""
    h, w = before.shape
    flat = before.reshape(-1)
    ys, xs = np.mgrid[y0:y1, x0:x1]
    j = (ys + my) * w + xs + mx
    inside = (j >= 0) & (j < w * h)
    return np.where(inside, flat[np.clip(j, 0, w * h - 1)], 0).astype(np.uint32)


class Colours:
    """Colours never used before in the clip: code k (1, 2, ...) times an odd number, which permutes the 24 (15) bits; never 0."""

    def __init__(self, bpp: int):
        self.bpp, self.next = bpp, 1

    def fresh(self, n: int) -> np.ndarray:
        codes = np.arange(self.next, self.next + n, dtype=np.uint64)
        self.next += n
        if self.bpp == 16:
            assert self.next <= 1 << 15, "out of 15-bit colours"
            v = (codes * np.uint64(0x2E5)) & np.uint64(0x7FFF)
            v = (v & np.uint64(31)) | (((v >> np.uint64(5)) & np.uint64(31)) << np.uint64(8)) | (((v >> np.uint64(10)) & np.uint64(31)) << np.uint64(16))
        else:
            assert self.next <= 1 << 24
            v = (codes * np.uint64(0x010305)) & np.uint64(0xFFFFFF)
        return v.astype(np.uint32)


def paint(before: np.ndarray, entries, colours: Colours) -> Tuple[np.ndarray, np.ndarray]:
    """(the picture of an inter frame, its hints): `before` with the entries' moves, all of them from `before`, then the repaints."""
    h, w = before.shape
    nbx, nby = geometry(w, h)
    out = before.copy()
    hints = np.full((nbx * nby, 2), sg.NO_HINT, dtype=np.int16)
    for e in entries:
        x16, y16, _, _ = block_box(e[1], w, h)
        x1, y1, x2, y2 = rect_of(e, w, h)
        if e[0] == "move":
            out[y16 + y1:y16 + y2, x16 + x1:x16 + x2] = move(before, y16 + y1, y16 + y2, x16 + x1, x16 + x2, *e[3])
            hints[e[1]] = e[3]
    for e in entries:
        x16, y16, bw, _ = block_box(e[1], w, h)
        x1, y1, x2, y2 = rect_of(e, w, h)
        if e[0] == "lit":
            out[y16 + y1:y16 + y2, x16 + x1:x16 + x2] = colours.fresh((y2 - y1) * (x2 - x1)).reshape(y2 - y1, x2 - x1)
            if e[3] == "above":
                out[y16, x16:x16 + bw // 2] = out[y16 - 1, x16:x16 + bw // 2]
                out[y16, x16 + bw // 2:x16 + bw] = out[y16 - 1, x16 + bw // 2 - 1:x16 + bw - 1]
            elif e[3] == "left":
                out[y16 + y1:y16 + y2, x16] = out[y16 + y1:y16 + y2, x16 - 1]
    return out, hints


def build(name: str, skip=()) -> ref.Clip:
    w, h, bpp, version = SPECS[name]
    enc = sg.SpEncoder(w, h, bpp, version)
    colours = Colours(bpp)
    chunks: List[bytes] = []
    keys: List[bool] = []
    frames: List[np.ndarray] = []
    coded_as: List[np.ndarray] = []
    pic = None
    for role, entries in table(name, skip):
        if role == "key":
            pic = colours.fresh(w * h).reshape(h, w)
            chunks.append(enc.encode_i(pic))
        else:
            pic, hints = paint(pic, entries, colours)
            chunks.append(enc.encode_p(pic, hints))
        keys.append(role == "key")
        frames.append(pic.reshape(-1).astype(np.uint32))
        coded_as.append(enc.current())
    enc.close()
    out = ref.Clip(f"motion_{name}_v{version}_{bpp}bpp_{w}x{h}", w, h, bpp, version, KEY_ROW, chunks, keys, frames)
    out.encoder_frames = coded_as          # what the encoder says a decoder holds; `frames` is what was painted
    return out


@lru_cache(maxsize=None)
def clip(name: str) -> ref.Clip:
    """The clip, built once a process; nobody changes it."""
    return build(name)


@lru_cache(maxsize=None)
def oracle(name: str):
    """(pictures, verdicts) of the oracle's sequential run over the clip, once a process."""
    return ref.oracle_run(clip(name), preinit=KEY_ROW)


def plan(name: str, skip=()) -> List[dict]:
    """Per frame, worked out from the table alone: dict(role, kind "key" / "none" / "inter", blocks = {block: (flags, rectangle,
    vector)} of the blocks the frame codes, motion_pixels, prev_pixels, data_pixels as the host stage counts them (an unchanged block
    and the block around a sub-rectangle count as copied; so does a moved rectangle), literalised = what a staged batch does with the
    frame: its motion blocks become literal ones when they hold at most a quarter of the picture's pixels)."""
    w, h, _, _ = SPECS[name]
    nbx, nby = geometry(w, h)
    out = []
    for role, entries in table(name, skip):
        p = dict(role=role, kind="key" if role == "key" else "inter" if entries else "none", blocks={}, motion_pixels=0, prev_pixels=0,
                 data_pixels=0, literalised=False)
        if p["kind"] == "inter":
            coded = {e[1]: e for e in entries}
            assert len(coded) == len(entries), "one entry a block"
            for b in range(nbx * nby):
                _, _, bw, bh = block_box(b, w, h)
                if b not in coded:
                    p["prev_pixels"] += bw * bh
                    continue
                e = coded[b]
                x1, y1, x2, y2 = rect = rect_of(e, w, h)
                sub = rect != (0, 0, bw, bh)
                area = (x2 - x1) * (y2 - y1)
                if sub:
                    p["prev_pixels"] += bw * bh
                if e[0] == "move":
                    p["prev_pixels"] += area
                    p["motion_pixels"] += area
                    p["blocks"][b] = (PB_MOTION | (PB_SUBRECT if sub else 0), rect, tuple(e[3]))
                else:
                    p["data_pixels"] += area
                    p["blocks"][b] = (PB_DATA | (PB_SUBRECT if sub else 0), rect, (0, 0))
            p["literalised"] = p["motion_pixels"] * 4 <= w * h
        out.append(p)
    return out


def kept(name: str) -> List[int]:
    """The frames a staged batch leaves their motion blocks: a launch of sp_pframe_kernel each."""
    return [t for t, p in enumerate(plan(name)) if p["kind"] == "inter" and not p["literalised"]]


def launches(name: str, fused: bool = True, lo: int = 0, hi: int = None) -> int:
    """How many kernels a staged batch of the clip's frames lo..hi-1 launches, a buffer per frame: one per key frame; with the
    fusion — which a batch with fewer than two inter frames does not take — one per run of literalised inter frames (a frame that
    changes nothing breaks no run, a key frame or a kept frame ends it) and one per kept frame; without it one per inter frame
    that changes something."""
    frames = plan(name)[lo:hi]
    fused = fused and sum(1 for p in frames if p["kind"] != "key") >= 2
    n, in_run = 0, False
    for p in frames:
        if p["kind"] == "none":
            continue
        if p["kind"] == "inter" and p["literalised"] and fused:
            n += 0 if in_run else 1
            in_run = True
        else:
            n += 1
            in_run = False
    return n


def launch_kinds(name: str, fused: bool = True, lo: int = 0, hi: int = None) -> Tuple[bool, bool]:
    """(a staged batch of frames lo..hi-1 launches sp_pframe_kernel, it launches a group kernel)."""
    frames = plan(name)[lo:hi]
    fused = fused and sum(1 for p in frames if p["kind"] != "key") >= 2
    inter = [p for p in frames if p["kind"] == "inter"]
    return any(not (fused and p["literalised"]) for p in inter), any(fused and p["literalised"] for p in inter)


def pieces(name: str) -> List[Tuple[int, int]]:
    """The clip cut into batches (lo, hi) so that every kept frame shares a batch of two with one literalised frame and nothing
    else: that batch's two launches and two kernel names say which of the two frames took which."""
    if name == "Q":
        return [(0, 1), (1, 3)]
    return [(0, 2), (2, 4), (4, 5), (5, 7), (7, 12), (12, 14), (14, 15)]


def describe_mismatch(got, want, w: int, h: int) -> str:
    """'' when the pictures are equal, else where the first wrong pixel is."""
    got = np.asarray(got).reshape(-1).view(np.uint32)
    want = np.asarray(want).reshape(-1).view(np.uint32)
    bad = np.nonzero(got != want)[0]
    if len(bad) == 0:
        return ""
    nbx, _ = geometry(w, h)
    y, x = divmod(int(bad[0]), w)
    return "%d pixels differ, first in block %d, row %d, col %d (want 0x%08x, got 0x%08x)" % (
        len(bad), (y // 16) * nbx + x // 16, y % 16, x % 16, int(want[bad[0]]), int(got[bad[0]]))


def staged(c: ref.Clip):
    """The host stage's answer for every frame of a clip as a staged batch has them (hoststage_binding.HostStage.decode_batch with
    the quarter rule on): a list of dicts."""
    import hoststage_binding as hb
    hs = hb.HostStage(c.w, c.h, c.bpp)
    hs.preinit(KEY_ROW)
    out = hs.decode_batch(c.chunks, c.keys, 1, literalise=True)
    hs.close()
    return out
