"""Directed inter-frame groups for msv1_blocks_temporal_kernel (jsplayer_amd/csrc/msv1_kernels.hip): short clips assembled
code by code with the toolkit of tests/msv1_directed_streams.py, so that every picture is known BY CONSTRUCTION, each
built to put one seam of the kernel's loader / worker hand-over in front of it.  A plain helper module (numpy only).

Seams (the numbers are those of the clips' `seams`):
  1. the frame-count cut (T_NF = 16 frames a chunk), chunk buffers reused from the third chunk on;
  2. the code-area cut (T_CODE = 14 KiB a chunk), the rows of the frames cut off fetched again, an exact fit and one
     16-byte step either side of it;
  3. no-op frames (16-bit only: empty, or skip codes shorter than size_of_just_skips) in front, between, behind — and
     their neighbour, the all-skip frame of size_of_just_skips bytes, which rewrites every block and is not adopted;
  4. the span arithmetic: `lo` rounded down to 16, `hi` clipped to the frame's end, a span of more than 1024 bytes,
     a tile with no coded block (need = 0);
  5. the zeroing behind the end of a frame's data in a REUSED chunk buffer: a truncated frame, a code word cut in two;
  6. the partial last tile: nblocks % 256 in {0, 1, 2, 3, 5, 16, 255};
  7. the stage-2 compare: cmp_row_lo % 4 != 0, the last live lane, rows below cmp_row_lo, identical pixels re-coded,
     pixels carried in registers across skipped and no-op frames, the buffer from before the group, the word boundaries
     of s_sig (frames 31, 32, 63, 64), 8-bit (never compares);
  8. where the group starts (a synchronous DecompressI into a buffer of its own, or a key frame inside the batch), a key
     frame in the middle of a group, 2, 3 and 5 destination buffers in rotation;
  9. Y % 4 != 0 (temporal launch + msv1_edge_compare_kernel, buffers that differ only outside the block grid) and
     X % 4 != 0 (the same clip through the per-frame msv1_blocks_kernel).

Each clip states its `claims` about the plan — ("chunks", tile, n), ("opens", tile, chunk, frame), ("cut", tile, chunk,
kept, over), ("fit", tile, chunk, slot, over), ("need", tile, frame, bytes), ("lo", tile, frame, first code's offset in
the frame, lo's offset in the frame), ("clipped", tile, frame), ("empty_last", tile), ("no_prev_fetch" | "prev_fetch",
tile) — which tests/test_msv1_temporal_clips_cpu.py proves through msv1_temporal_plan.plan; frame numbers count the
frames of the batch (= of the group: every clip here is one temporal group unless it says otherwise).

The 4-byte table fetch of a partial tile's last quad (msv1_kernels.hip:322) reads up to 3 entries past the frame's row:
the next frame's row, or for the last frame of the batch up to 12 bytes past the nblocks * nframes entries that
msv1_codec.cpp asks for — inside the allocation, since DeviceBuffer::reserve (common.h) allocates n + n / 4 + 256 bytes.
The entries fetched so are never used (msv1_kernels.hip:342 `lane * 4 + k < live_blocks`, :441 `live`).

Not reachable through the C ABI, so not in the catalogue:
  * a code-area cut at kept < 3 (16-bit) or kept < 5 (8-bit), and with it the `kept > 0` guard of msv1_kernels.hip:353
    ("a chunk's first frame is always admitted"): a tile's frame needs at most 256 * 18 + 30 bytes rounded up to 16, so
    three frames (with their T_SLACK) always fit T_CODE — 3 * (4640 + 64) = 14112 <= 14336; 8-bit codes are at most
    10 bytes a block, 2560 + 16 a frame;
  * an 8-bit end marker or a skip code with no previous frame inside a group: plan_launches runs such frames alone
    (msv1_codec.cpp:228, :1278 `special`).  A TRUNCATED frame is not special — msv1_host.cpp:57-85 goes on with missing
    bytes, every block is "coded" — so seam 5 is reachable, and the clips below reach it in chunk 2 and later;
  * 8-bit no-op frames: the early-out is the 16-bit decoder's (msv1_host.cpp:37)."""
from __future__ import annotations

import functools
import zlib
from dataclasses import dataclass, field

import numpy as np

import msv1_directed_streams as D

PREFILL = D.PREFILL
LINES = 36
SIZES = {(64, 64): 0, (64, 68): 16, (1028, 4): 1, (24, 172): 2, (28, 148): 3, (36, 116): 5, (68, 60): 255}   # nblocks % 256
THREE_TILES = (64, 132)
Y_EDGE, X_EDGE = (64, 66), (66, 64)
UNTOUCHED = "untouched"      # a frame's `picture`: the decoder writes nothing (no-op)


@dataclass
class Clip:
    name: str
    bits: int
    w: int
    h: int
    lines: int
    nbuf: int                    # buffers in rotation; a synchronous key frame goes into one more, index nbuf
    start: str                   # "sync": a key frame through DecompressI first; "batch": the batch's frame 0 is the key frame
    sync_key: object             # bytes of that key frame (start == "sync")
    prefills: list               # what each buffer holds before anything is decoded (nbuf + 1 values)
    frames: list = field(default_factory=list)     # [(bytes, is_key)]
    dsts: list = field(default_factory=list)       # buffer index per frame
    pictures: list = field(default_factory=list)   # per frame: grid picture (flat, gw * gh), UNTOUCHED, or None (malformed: oracle only)
    claims: list = field(default_factory=list)
    seams: tuple = ()
    kernel: str = "msv1_blocks_temporal_kernel"
    edge: bool = False           # msv1_edge_compare_kernel runs too
    significant: dict = field(default_factory=dict)   # frame -> bool: what the clip was built to make the compare say

    @property
    def gw(self):
        return self.w // 4 * 4

    @property
    def gh(self):
        return self.h // 4 * 4

    @property
    def nblocks(self):
        return (self.w // 4) * (self.h // 4)


def _rng(*what):
    return np.random.default_rng(zlib.crc32(repr(what).encode()))


class Builder:
    """A clip under construction: keeps the previous picture by construction and hands out buffers as Manager does (the
    next of the rotation that is not the previous frame)."""

    def __init__(self, name, bits, w, h, seams, lines=LINES, nbuf=3, start="sync", prefills=None, key_items=None):
        self.bits, self.gw, self.gh = bits, w // 4 * 4, h // 4 * 4
        self.nb = (w // 4) * (h // 4)
        self.rng = _rng(name, bits)
        self.pal = D.palette(bits)
        self.prev_pic, self.prev_buf, self.last = None, None, -1
        c = self.clip = Clip(f"{name}_{bits}", bits, w, h, lines, nbuf, start, None, prefills or [PREFILL] * (nbuf + 1), seams=tuple(seams))
        key_items = key_items or self.stream().finish().items
        a = D.assemble(bits, self.gw, self.gh, key_items, None, self.pal)
        self.key_items = list(key_items)
        if start == "sync":
            c.sync_key = a.data
            self.prev_pic, self.prev_buf = a.picture, nbuf
        else:
            self.raw(a.data, a.picture, True, adopted=True)

    def stream(self, skips=False):
        return D.Stream(self.bits, self.gw, self.gh, self.rng, skips)

    def _dst(self):
        d = (self.last + 1) % self.clip.nbuf
        if d == self.prev_buf:
            d = (d + 1) % self.clip.nbuf
        assert d != self.prev_buf
        self.last = d
        return d

    def raw(self, data, picture, key=False, adopted=False):
        c = self.clip
        d = self._dst()
        c.frames.append((bytes(data), key))
        c.dsts.append(d)
        c.pictures.append(picture)
        if adopted:
            self.prev_pic, self.prev_buf = picture, d
        return len(c.frames) - 1

    def items(self, items, key=False, cut=None):
        """A frame from toolkit items; `cut`: only its first `cut` bytes (a truncated frame: no picture by construction)."""
        a = D.assemble(self.bits, self.gw, self.gh, items, self.prev_pic, self.pal)
        if cut is not None:
            return self.raw(a.data[:cut], None, key, adopted=True)
        assert not a.short and a.picture is not None, "the catalogue's well-formed frames cover every block"
        return self.raw(a.data, a.picture, key, adopted=a.coded > 0)

    def noop(self, data=b""):
        assert self.bits == 16 and len(data) < 10
        return self.raw(data, UNTOUCHED)

    # -- frames
    def dense_items(self):
        s = self.stream()
        for _ in range(self.nb):
            s.add(s.rand("eight"))
        return s.items

    def dense(self, **kw):
        return self.items(self.dense_items(), **kw)

    def sparse_items(self, k, per_tile=3):
        """A few random codes in every tile (their place moves with k), skip codes everywhere else."""
        s, at = self.stream(True), 0
        for t in range((self.nb + 255) // 256):
            live = min(256, self.nb - t * 256)
            n = min(per_tile, live)
            first = t * 256 + (k * 37 + t * 11) % (live - n + 1)
            if first > at:
                s.add(("skip", first - at))
            for j in range(n):
                s.add(s.rand(("eight", "two", "solid")[(k + j) % 3]))
            at = first + n
        if at < self.nb:
            s.add(("skip", self.nb - at))
        return s.items

    def sparse(self, k, **kw):
        return self.items(self.sparse_items(k), **kw)

    def sized_items(self, need, tail_skips=1):
        """Codes from byte 0 whose last one is an 8-colour code starting at need - 18, the rest of the frame skipped in
        `tail_skips` skip codes: the tile's `hi` is `need` exactly where the data reaches that far."""
        s = self.stream()
        for k in range(1, 200):
            if s._exact_ok(need - 18, k):
                break
        else:
            raise D.Infeasible(f"{need - 18} bytes")
        s.fill_exact(need - 18, k)
        s.add(s.rand("eight"))
        left = self.nb - k - 1
        for j in range(tail_skips):
            n = left // tail_skips + (1 if j < left % tail_skips else 0)
            s.add(("skip", n))
        return s.items

    def recode_items(self, changes, same=()):
        """Skip everything but the blocks of `same` (coded again exactly as the key frame's items coded them: only valid while
        those blocks still show the key frame) and of `changes` ({block: item})."""
        todo = dict(changes)
        for b in same:
            todo[b] = self.key_items[b]
        out, at = [], 0
        for b in sorted(todo):
            if b > at:
                out.append(("skip", b - at))
            out.append(todo[b])
            at = b + 1
        if at < self.nb:
            out.append(("skip", self.nb - at))
        return out

    def claim(self, *c):
        self.clip.claims.append(tuple(c))

    def done(self):
        return self.clip


def solid_key(bits, nb, rng):
    """A key frame of solid blocks, every block a colour of its own kind (so that a re-coded block can differ from it in chosen
    rows) -> (items, colour per block)."""
    cols = []
    for b in range(nb):
        cols.append(int(rng.integers(1, 0x100)) if bits == 8 else int(rng.integers(0x20, 0x3FF)))   # (16-bit: high byte < 4: not a skip code)
    return [("solid", c) for c in cols], cols


def rows_item(bits, base, other, rows23):
    """An 8-colour code that shows `base` in rows 0-1 and `other` in rows 2-3 of its block (rows23) or the other way round."""
    top, bottom = (base, other) if rows23 else (other, base)
    cols = [top] * 4 + [bottom] * 4
    if bits == 16:
        cols[0] |= 0x8000
        return ("eight", 0x1234, tuple(cols))
    return ("eight", 0x9234, tuple(cols))


# ---- the catalogue ------------------------------------------------------------------------------------------------------------
def _counts(bits):
    out = []
    for n, nbuf, start in ((1, 3, "sync"), (15, 3, "batch"), (16, 2, "sync"), (17, 2, "batch"), (32, 3, "sync"), (33, 5, "sync"), (49, 5, "batch")):
        b = Builder(f"count_{n}", bits, 64, 68, (1, 8), nbuf=nbuf, start=start)
        for k in range(n - (start == "batch")):
            b.sparse(k)
        for t in (0, 1):
            b.claim("chunks", t, (n + 15) // 16)
            for c in range((n + 15) // 16):
                b.claim("opens", t, c, 16 * c)
            b.claim("prev_fetch" if start == "sync" else "no_prev_fetch", t)
        out.append(b.done())
    return out


def _code_cut(bits):
    """The densest frames (every block an 8-colour code): 4608 bytes a tile and frame in 16-bit, 2560 in 8-bit — three / five
    fill a chunk.  Then a chunk closed by a frame that fits exactly, one that leaves 16 bytes, one that is 16 bytes too long."""
    per, full = (3, 4608) if bits == 16 else (5, 2560)
    used = per * (full + 64)
    exact = 14 * 1024 - used
    b = Builder("code_cut", bits, 64, 64, (2, 4), nbuf=32)      # (a buffer a frame: every picture stays to be looked at)
    tail = 1 if bits == 16 else 5                 # (8-bit: the data must reach `need` bytes — the last code is 10 bytes, hi = its start + 18)
    for _ in range(per):
        b.dense()
    b.claim("cut", 0, 0, per, per * (full + 64) + full - 14 * 1024)
    b.claim("opens", 0, 1, per)
    for chunk, over in ((1, 0), (2, -16)):
        for _ in range(per):
            b.dense()
        f = b.items(b.sized_items(exact + over, tail))
        b.claim("need", 0, f, exact + over)
        b.claim("fit", 0, chunk, per, over)
        b.claim("opens", 0, chunk + 1, f + 1)
    for _ in range(per):
        b.dense()
    f = b.items(b.sized_items(exact + 16, tail))
    b.claim("cut", 0, 3, per, 16)
    b.claim("opens", 0, 4, f)
    b.claim("need", 0, f, exact + 16)
    for _ in range(per):
        b.dense()                                 # behind the short frame: the cut comes one frame later than in chunk 0
    b.claim("cut", 0, 4, per, (exact + 16 + 64) + (per - 1) * (full + 64) + full - 14 * 1024)
    b.sparse(1)
    b.sparse(2)
    b.claim("chunks", 0, 6)
    return [b.done()]


def _noops():
    out = []
    b = Builder("noop_front", 16, 64, 68, (3, 7), lines=6)
    b.noop()
    b.noop(b"\x00\x84")
    f = b.items(b.recode_items({}, same=(100, 260)))               # identical pixels: only the previous frame's own pixels make that so
    b.clip.significant[f] = False
    b.sparse(1)
    b.claim("prev_fetch", 0)
    b.claim("opens", 0, 0, 2)
    out.append(b.done())
    b = Builder("noop_between", 16, 64, 68, (3, 7), lines=6)
    b.sparse(0)
    b.noop()
    b.sparse(1)
    b.noop(b"\x05\x84\x06\x84")
    b.noop(b"\xff\x87\xff\x87")
    b.sparse(2)
    b.noop()
    b.claim("chunks", 0, 1)
    out.append(b.done())
    b = Builder("noop_tail", 16, 64, 68, (3, 1))
    for k in range(16):
        b.sparse(k)
    for _ in range(3):
        b.noop()
    b.claim("chunks", 0, 2)
    b.claim("empty_last", 0)
    b.claim("empty_last", 1)
    out.append(b.done())
    b = Builder("noop_17th", 16, 64, 68, (3, 1), nbuf=24)                    # no-ops take no slot: 16 written frames and 5 no-ops are ONE chunk
    for k in range(16):
        b.sparse(k)
        if k % 3 == 0 and k < 15:
            b.noop()
    b.claim("chunks", 0, 1)
    out.append(b.done())
    b = Builder("allskip_neighbour", 16, 64, 68, (3, 7), lines=6)
    b.sparse(0)
    b.items([("skip", 60), ("skip", 60), ("skip", 60), ("skip", 60), ("skip", 32)])    # 10 bytes = size_of_just_skips: written, not adopted
    b.sparse(1)
    b.noop(b"\x3c\x84" * 4)                                                             # 8 bytes of the same: a no-op
    b.sparse(2)
    out.append(b.done())
    return out


def _span(bits):
    b = Builder("span", bits, 64, 68, (4,), nbuf=8)
    for skips, lo in ((0, 0), (1, 0), (7, 0), (8, 16)):
        s = b.stream(True)
        for _ in range(skips):
            s.add(("skip", 1))
        for _ in range(120):
            s.add(s.rand("eight"))
        s.add(("skip", 272 - 120 - skips))                         # tile 1: skipped altogether
        f = b.items(s.items)
        b.claim("lo", 0, f, 2 * skips, lo)
        b.claim("need", 1, f, 0)
        b.claim("rounds", 0, f, 2)
    s = b.stream(True)                                              # the last code a solid one (2 bytes): hi = its start + 18 lies past the data
    s.add(("skip", 200))
    for _ in range(71):
        s.add(s.rand("two"))
    s.add(s.rand("solid"))
    f = b.items(s.items)
    b.claim("clipped", 1, f)
    b.sparse(3)
    return [b.done()]


def _tails(bits):
    """Behind two chunks of the densest frames (every byte of both chunk buffers non-zero as far as a frame reaches), in tile 0:
    a frame cut in the middle of a code, one cut in the middle of a code WORD, one whose data ends exactly where the tile's
    first code would start — each followed by a dense frame (a truncated frame's picture is the oracle's to say, and whatever
    follows must not depend on it)."""
    per = 3 if bits == 16 else 5
    size = 18 if bits == 16 else 10
    b = Builder("tails", bits, 64, 68, (5,), nbuf=24)
    for _ in range(2 * per):
        b.dense()
    f = b.dense(cut=size * 150 + 2)                 # the code word of block 150 and nothing of its colours (too long to go into chunk 1)
    b.claim("opens", 0, 2, f)
    b.claim("clipped", 0, f)
    b.dense()
    it = b.dense_items()
    data = D.assemble(bits, b.gw, b.gh, it, None, b.pal).data
    k = next(k for k in range(60, 200) if data[size * k] != 0)
    b.dense(cut=size * k + 1)                       # half a code word (16-bit: the odd last byte; 8-bit: avail == 1)
    b.dense()
    b.dense()
    if bits == 16:                                  # 10 bytes of skip codes (not a no-op), then nothing: block 100's code starts at the end
        f = b.items([("skip", 20)] * 5 + b.dense_items()[:172], cut=10)
    else:                                           # 8-bit: no data at all — every code of every tile starts at the end
        f = b.items(b.dense_items(), cut=0)
        b.claim("need", 0, f, 0)
    b.dense()
    f = b.dense(cut=size * 256)                     # the end exactly on tile 1's first code
    b.claim("need", 1, f, 0)
    b.dense()
    b.sparse(1)
    return [b.done()]


def _partial(bits):
    out = []
    for (w, h), rem in SIZES.items():
        nb = (w // 4) * (h // 4)
        b = Builder(f"partial_{w}x{h}", bits, w, h, (6, 7), lines=0, nbuf=2)
        b.sparse(0)
        b.dense()
        last = nb - 1
        s = b.stream(True)                          # only the last live lane is coded
        s.add(("skip", last))
        s.add(s.rand("eight"))
        b.items(s.items)
        s = b.stream(True)                          # the whole last quad and the lane in front of it
        n = min(5, nb)
        s.add(("skip", nb - n))
        for _ in range(n):
            s.add(s.rand("two"))
        b.items(s.items)
        b.sparse(3)
        b.claim("chunks", (nb - 1) // 256, 1)
        out.append(b.done())
    return out


def _significance():
    out = []
    rng = _rng("solid key")
    items, cols = solid_key(16, 256, rng)
    other = [c ^ 0x15 for c in cols]
    # Preinit(6): blocks rows 0-1 are insignificant for stage 1, pixel rows 0-5 for the compare — rows 6-7 of block row 1 count
    b = Builder("sig_rows", 16, 64, 64, (7,), lines=6, key_items=items)
    say = b.clip.significant
    say[b.items(b.recode_items({}, same=(40, 200)))] = False                                        # identical pixels re-coded
    say[b.items(b.recode_items({20: rows_item(16, cols[20], other[20], True)}, same=(40,)))] = True      # rows 6-7 of block row 1
    say[b.items(b.recode_items({20: ("solid", cols[20])}, same=(40,)))] = True                         # ... and back
    say[b.items(b.recode_items({21: rows_item(16, cols[21], other[21], False), 3: ("solid", other[3])}, same=(40,)))] = False   # rows 4-5 and block row 0 only
    say[b.items(b.recode_items({255: ("two", 0x7FFF, cols[255], other[255])}, same=(40,)))] = True       # one pixel of the last lane
    out.append(b.done())
    b = Builder("sig_carried", 16, 64, 64, (7, 3), lines=6, key_items=items, nbuf=8)
    say = b.clip.significant
    say[b.items(b.recode_items({130: ("solid", other[130])}))] = True
    b.noop()
    b.items([("skip", 52)] * 4 + [("skip", 48)])
    say[b.items(b.recode_items({130: ("solid", other[130])}))] = False       # equal to what the registers carry, not to the buffer from before the group
    b.noop(b"\x00\x84")
    say[b.items(b.recode_items({130: ("solid", cols[130])}))] = True         # equal to the buffer from before the group, not to the registers
    out.append(b.done())
    b = Builder("sig_last_lane", 16, 64, 68, (7, 6), lines=6)
    say = b.clip.significant
    say[b.items(b.recode_items({}, same=(271,)))] = False
    s = b.stream()
    say[b.items(b.recode_items({271: s.rand("eight")}))] = True
    out.append(b.done())
    # the word boundaries of s_sig: 66 frames, of which exactly 31, 32, 63 and 64 change a pixel that counts
    b = Builder("sig_words", 16, 64, 64, (7, 1), lines=6, key_items=items, nbuf=5)
    say = b.clip.significant
    now = list(cols)
    for f in range(66):
        blk = 64 + f
        if f in (31, 32, 63, 64):
            now[blk] = other[blk]
            say[b.items(b.recode_items({blk: ("solid", now[blk])}))] = True
        else:
            say[b.items(b.recode_items({blk: ("solid", now[blk])}))] = False
    b.claim("chunks", 0, 5)
    out.append(b.done())
    return out


def _starts(bits):
    out = []
    b = Builder("key_mid", bits, 64, 68, (8,), nbuf=2, start="batch")
    for k in range(3):
        b.sparse(k)
    b.items(b.stream().finish().items, key=True)
    for k in range(3, 6):
        b.sparse(k)
    b.claim("chunks", 0, 1)
    b.claim("no_prev_fetch", 0)
    out.append(b.done())
    w, h = THREE_TILES
    b = Builder("three_tiles", bits, w, h, (8, 1, 6), nbuf=5)
    for k in range(18):
        b.sparse(k)
    b.dense()
    b.sparse(19)
    for t in range(3):
        b.claim("chunks", t, 2)
    out.append(b.done())
    return out


def _edges(bits):
    """The same frames at 64x66 (temporal + edge compare) and 66x64 (per-frame kernel).  Buffers 0 and 1 and the synchronous key
    frame's hold the same pixels outside the block grid, buffer 2 others: re-coding identical pixels is significant exactly
    when one of the two buffers compared is buffer 2."""
    out = []
    for name, (w, h) in (("y_edge", Y_EDGE), ("x_edge", X_EDGE)):
        b = Builder(name, bits, w, h, (9,), lines=6, nbuf=3, prefills=[PREFILL, PREFILL, 0x00123456, PREFILL])
        b.clip.edge = bits == 16
        if w % 4:
            b.clip.kernel = "msv1_blocks_kernel"
        for k in range(7):
            b.items(b.recode_items({}, same=(40 + k, 200 + k)))
        b.sparse(1)
        b.sparse(2)
        out.append(b.done())
    return out


@functools.lru_cache(maxsize=None)
def catalogue():
    clips = []
    for bits in (16, 8):
        clips += _counts(bits) + _code_cut(bits) + _span(bits) + _tails(bits) + _partial(bits) + _starts(bits) + _edges(bits)
    clips += _noops() + _significance()
    names = [c.name for c in clips]
    assert len(set(names)) == len(names)
    assert all(len(c.frames) <= 72 for c in clips)
    return clips


def by_name(name):
    return next(c for c in catalogue() if c.name == name)


def names():
    return [c.name for c in catalogue()]
