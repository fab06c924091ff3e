"""Directed MSVideo1 streams for the on-GPU parse (jsplayer_amd/csrc/msv1_parse_kernels.hip): frames assembled code by code
so that a chosen code, skip run, end marker or end of data lies at a chosen place relative to a tile, wave or lane-group
boundary of the parse — with the picture known BY CONSTRUCTION (from the items, not from any decoder).

A plain helper module (no tests of its own, numpy only):
  * assemble     — items -> (bytes, expected picture, layout); refuses items whose bytes would read as another code kind;
  * Stream       — a frame under construction: random valid filler whose sizes make byte offsets come out exactly
                   (fill_to, fill_exact), `place` (a chosen code `back` slots before a chosen byte offset), `finish`;
  * catalogue    — the named cases per bit depth, each a short clip (a key frame built here, then the directed frame; or the
                   directed frame alone where it is a key frame) with, per frame, the picture by construction (None where the
                   stream is malformed: only the oracle says what the reference does with those) and whether the on-GPU
                   parse settles the frame or hands it to the host parser (`host`);
  * tile_spans   — the block span each tile owns, from the layout.
tests/test_msv1_directed_streams_cpu.py checks every geometric claim made here with a plain walk over the bytes;
tests/test_msv1_tile_edges_gpu.py sends the catalogue through every decode path."""
from __future__ import annotations

import functools
import zlib
from dataclasses import dataclass, field

import numpy as np

# The parse cuts a frame's bytes into tiles of msv1_small_tile_bytes() (the one-frame launches and the table-writing batch
# form: 256 lanes x 16 slots x 2 bytes) or msv1_parse_tile_bytes() (the batch forms: 256 lanes x JSP_BATCH_LS = 32 slots).
SMALL_TILE = 8192
BATCH_TILE = 16384
TILES = (SMALL_TILE, BATCH_TILE)
LANES = 256            # lanes per tile; a wave is 64 of them, the fused kernel's in-wave walk groups them 10 + 6 x 9
PREFILL = 0x00A5A5A5   # what the tests' frame buffers hold before a frame is decoded into them

SIZES = {16: (256, 192), 8: (320, 256)}   # smallest frames whose densest stream (18 / 10 bytes a block) spans three 16 KiB tiles
BIG = (512, 320)                          # 10240 blocks: more than the 8192 of msv1_parse_emit's staging buffer
KIND_SLOTS = {16: {"solid": 1, "two": 3, "eight": 9, "skip": 1}, 8: {"solid": 1, "two": 2, "eight": 5, "skip": 1, "end": 1}}


class Refused(ValueError):
    """An item whose bytes would be read as another kind of code (or that cannot stand where it was put)."""


class Infeasible(ValueError):
    """No run of valid codes has the bytes / blocks asked for."""


# ---- items -> bytes ---------------------------------------------------------------------------------------------------------------
def encode_item(bits, item):
    kind = item[0]
    if kind == "raw":
        return bytes(item[1])
    if kind == "skip":
        n = item[1]
        if not 0 <= n <= 1023:
            raise Refused(f"skip count {n}")
        return bytes([n & 0xFF, 0x84 + (n >> 8)])
    if kind == "end":
        if bits != 8:
            raise Refused("the 16-bit format has no end marker")
        return b"\x00\x00"
    if bits == 16:
        if kind == "solid":
            c = item[1]
            if not 0 <= c <= 0x7FFF or (c >> 10) == 1:
                raise Refused(f"solid colour {c:#x}: its high byte would read as a skip code (or lose bit 15)")
            return bytes([c & 0xFF, 0x80 | (c >> 8)])
        flags, cols = (item[1], item[2:4]) if kind == "two" else (item[1], tuple(item[2]))
        if not 0 <= flags <= 0x7FFF:
            raise Refused(f"pattern flags {flags:#x}: the high byte must stay below 0x80")
        if any(not 0 <= c <= 0xFFFF for c in cols):
            raise Refused("colour out of range")
        if kind == "two":
            if cols[0] & 0x8000:
                raise Refused("2-colour code whose first colour has bit 15 set: it would read as an 8-colour code")
        elif kind == "eight":
            if len(cols) != 8 or not cols[0] & 0x8000:
                raise Refused("8-colour code: eight colours, bit 15 of the first one set")
        else:
            raise Refused(f"unknown item {kind}")
        out = bytearray([flags & 0xFF, flags >> 8])
        for c in cols:
            out += bytes([c & 0xFF, c >> 8])
        return bytes(out)
    if kind == "solid":
        c = item[1]
        if not 0 <= c <= 255:
            raise Refused("palette index out of range")
        hi = (c >> 4) & 0xF            # any high byte 0x80..0x8F but the skip codes' 0x84..0x87 (the decoder ignores it)
        return bytes([c, 0x80 | (hi + 4 if 4 <= hi <= 7 else hi)])
    if kind == "two":
        flags, cols = item[1], item[2:4]
        if not 0 < flags <= 0x7FFF:
            raise Refused(f"2-colour flags {flags:#x}: 0 is the end marker, 0x8000 and up are other codes")
    elif kind == "eight":
        flags, cols = item[1], tuple(item[2])
        if not 0x9000 <= flags <= 0xFFFF or len(cols) != 8:
            raise Refused(f"8-colour flags {flags:#x}: the high byte must be 0x90 or more")
    else:
        raise Refused(f"unknown item {kind}")
    if any(not 0 <= c <= 255 for c in cols):
        raise Refused("palette index out of range")
    return bytes([flags & 0xFF, flags >> 8]) + bytes(cols)


def rgb555(c):
    """MSVideo1.hx:211-214: 5 bits a channel, left-aligned in 0x00RRGGBB (bit 15 plays no part)."""
    c = np.asarray(c, dtype=np.int64)
    return ((c & 0x1F) << 3) | ((c & 0x3E0) << 6) | ((c & 0x7C00) << 9)


def palette_ints(pal_bytes):
    p = np.zeros(256, dtype=np.int64)
    v = np.frombuffer(bytes(pal_bytes)[: len(pal_bytes) // 4 * 4], dtype="<u4")[:256]
    p[: len(v)] = v
    return p


_QUAD = np.array([((y & 2) << 1) + (x & 2) for y in range(4) for x in range(4)])
_PREV, _KEEP, _SOLID, _TWO, _EIGHT = 0, 1, 2, 3, 4


def _blocks_of(img, w, h):
    nbx, nby = w // 4, h // 4
    return img.reshape(h, w)[: nby * 4, : nbx * 4].reshape(nby, 4, nbx, 4).transpose(0, 2, 1, 3).reshape(nbx * nby, 16)


@dataclass
class Assembled:
    data: bytes
    picture: object            # flat uint32 array (w * h), or None: malformed stream / the reference raises
    layout: list               # (byte offset, first block, blocks covered, kind, slots) of every code, in order
    consumed: int              # bytes up to the end of the code that covers the last block (or of the end marker); -1: too short
    short: bool                # the data ends before every block is covered (and no end marker stopped the walk)
    ended: bool                # an 8-bit end marker stopped the walk
    skip_codes: int
    coded: int


def assemble(bits, w, h, items, prev=None, palette=None, fill=PREFILL):
    """items -> Assembled.  `prev`: the previous picture (flat uint32; what a skipped block shows), None: there is none, and a
    skip code makes the reference raise.  Blocks behind an end marker keep `fill`.  Trailing bytes go in as ("raw", bytes), last."""
    assert w % 4 == 0 and h % 4 == 0
    nb = (w // 4) * (h // 4)
    what = np.full(nb, _KEEP, dtype=np.int8)
    flags = np.zeros(nb, dtype=np.int64)
    cols = np.zeros((nb, 8), dtype=np.int64)
    out, layout = bytearray(), []
    blk, done, ended, consumed, nskip, ncoded = 0, False, False, -1, 0, 0
    for k, item in enumerate(items):
        b = encode_item(bits, item)
        kind = item[0]
        if kind == "raw":
            if k != len(items) - 1:
                raise Refused("raw bytes anywhere but at the end")
            out += b
            break
        if done:
            raise Refused(f"item {k} ({kind}) behind the last block: trailing bytes go in as raw")
        pos = len(out)
        out += b
        if kind == "end":
            layout.append((pos, blk, 0, kind, 1))
            done = ended = True
            consumed = len(out)
            continue
        if kind == "skip":
            n = item[1] if item[1] else nb - blk
            n = min(n, nb - blk)
            what[blk:blk + n] = _PREV
            nskip += 1
        else:
            n = 1
            ncoded += 1
            c = (item[1],) if kind == "solid" else item[2:4] if kind == "two" else item[2]
            cols[blk, : len(c)] = c              # colour words / palette indices: turned into pixels below, all at once
            flags[blk] = 0 if kind == "solid" else item[1]
            what[blk] = {"solid": _SOLID, "two": _TWO, "eight": _EIGHT}[kind]
        layout.append((pos, blk, n, kind, len(b) // 2))
        blk += n
        if blk >= nb:
            done = True
            consumed = len(out)
    short = not done
    raises = nskip > 0 and prev is None
    picture = None
    if not short and not raises:
        cols = rgb555(cols) if bits == 16 else palette_ints(palette or b"")[cols]
        bit = (flags[:, None] >> np.arange(16)[None, :]) & 1                     # a set bit: the FIRST colour of the pair
        px = np.where(bit == 1, cols[:, 0:1], cols[:, 1:2])                       # 2-colour
        px = np.where((what == _SOLID)[:, None], cols[:, 0:1], px)
        px8 = np.take_along_axis(cols, _QUAD[None, :] + (1 - bit), axis=1)        # 8-colour: a pair per 2x2 quadrant
        px = np.where((what == _EIGHT)[:, None], px8, px)
        px = np.where((what == _KEEP)[:, None], np.int64(fill), px)
        if prev is not None:
            px = np.where((what == _PREV)[:, None], _blocks_of(np.asarray(prev, dtype=np.int64), w, h), px)
        nbx, nby = w // 4, h // 4
        picture = px.reshape(nby, nbx, 4, 4).transpose(0, 2, 1, 3).reshape(h * w).astype(np.uint32)
    return Assembled(bytes(out), picture, layout, consumed, short, ended, nskip, ncoded)


def tile_spans(layout, tile, nb):
    """Per tile of `tile` bytes: [first block, end block) of the codes that START in it (clipped to the frame's nb blocks);
    (b, b) for a tile that owns nothing, b being where the chain stands."""
    if not layout:
        return []
    ntiles = layout[-1][0] // tile + 1
    spans, at = [], 0
    k = 0
    for t in range(ntiles):
        first = min(at, nb)
        while k < len(layout) and layout[k][0] < (t + 1) * tile:
            at = layout[k][1] + layout[k][2]
            k += 1
        spans.append((first, min(at, nb)))
    return spans


# ---- a frame under construction -------------------------------------------------------------------------------------------------
class Stream:
    def __init__(self, bits, w, h, rng, skips=False):
        self.bits, self.w, self.h, self.rng, self.skips = bits, w, h, rng, skips
        self.nb = (w // 4) * (h // 4)
        self.items, self.nbytes, self.blocks = [], 0, 0
        self.sizes = (2, 6, 18) if bits == 16 else (2, 4, 10)
        self.claims = []

    # -- random valid items
    def rand(self, kind):
        r, bits = self.rng, self.bits
        if kind == "solid":
            if bits == 8:
                return ("solid", int(r.integers(0, 256)))
            while True:
                c = int(r.integers(0, 0x8000))
                if (c >> 10) != 1:
                    return ("solid", c)
        if kind == "two":
            if bits == 8:
                return ("two", int(r.integers(1, 0x8000)), int(r.integers(0, 256)), int(r.integers(0, 256)))
            return ("two", int(r.integers(0, 0x8000)), int(r.integers(0, 0x8000)), int(r.integers(0, 0x10000)))
        if kind == "eight":
            if bits == 8:
                return ("eight", int(r.integers(0x9000, 0x10000)), tuple(int(v) for v in r.integers(0, 256, 8)))
            c = [int(v) for v in r.integers(0, 0x10000, 8)]
            c[0] |= 0x8000
            return ("eight", int(r.integers(0, 0x8000)), tuple(c))
        raise ValueError(kind)

    def size(self, item):
        return len(item[1]) if item[0] == "raw" else 2 * KIND_SLOTS[self.bits][item[0]]

    def add(self, item):
        n = self.size(item)
        if item[0] == "skip":
            cover = item[1] if item[1] else self.nb - self.blocks
        else:
            cover = 0 if item[0] in ("raw", "end") else 1
        if item[0] not in ("raw", "end") and (cover < 1 or self.blocks + cover > self.nb):
            raise Refused(f"{item[0]} at block {self.blocks}: it would cover blocks the frame does not have")
        at = self.nbytes
        self.items.append(item)
        self.nbytes += n
        self.blocks += cover
        return at

    def _min_codes(self, nbytes):
        """(An upper bound of) the fewest coded blocks whose codes are exactly `nbytes` long."""
        big = self.sizes[2]
        q, rem = divmod(nbytes, big)
        tab = {0: 0, 2: 1, 4: 2, 6: 1, 8: 2, 10: 3, 12: 2, 14: 3, 16: 4} if self.bits == 16 else {0: 0, 2: 1, 4: 1, 6: 2, 8: 2}
        return q + tab[rem]

    def _weights(self, need):
        p8 = min(0.97, max(0.2, need / self.sizes[2] * 1.15))
        return {"solid": (1 - p8) * 0.4, "two": (1 - p8) * 0.6, "eight": p8}

    def _pick(self, cands):
        tot = sum(wt for _, wt in cands)
        u = self.rng.random() * tot
        for it, wt in cands:
            u -= wt
            if u <= 0:
                return it
        return cands[-1][0]

    def _random_codes(self, nbytes, room, skips):
        """Random valid codes, exactly `nbytes` long, covering at most `room` blocks -> (items, blocks covered)."""
        if nbytes < 0 or nbytes % 2:
            raise Infeasible(f"{nbytes} bytes")
        items, left, used = [], nbytes, 0
        while left:
            free = room - used
            if free < 1:
                raise Infeasible(f"{left} bytes left and no block to put them in")
            wts = self._weights(left / free)
            cands = [(k, wts[k]) for k, s in zip(("solid", "two", "eight"), self.sizes)
                     if s <= left and self._min_codes(left - s) <= free - 1]
            if skips:
                n = int(self.rng.integers(1, 7))
                if self._min_codes(left - 2) <= free - n:
                    cands.append((("skip", n), 0.08))
            if not cands:
                raise Infeasible(f"{left} bytes in {free} blocks")
            it = self._pick(cands)
            it = self.rand(it) if isinstance(it, str) else it
            items.append(it)
            left -= self.size(it)
            used += it[1] if it[0] == "skip" else 1
        return items, used

    def fill_to(self, offset, max_blocks):
        """Random valid codes from here up to byte `offset` exactly, covering at most `max_blocks` blocks."""
        items, _ = self._random_codes(offset - self.nbytes, min(max_blocks, self.nb - self.blocks), self.skips)
        for it in items:
            self.add(it)

    def _exact_ok(self, nbytes, k):
        """k coded blocks can be exactly nbytes long: sizes are 2, 2 + u, 2 + 4u."""
        u = self.sizes[1] - 2
        if k < 0 or nbytes < 2 * k or (nbytes - 2 * k) % u:
            return False
        x = (nbytes - 2 * k) // u
        return x - 3 * (x // 4) <= k

    def fill_exact(self, nbytes, blocks):
        """Random valid codes, exactly `nbytes` long AND covering exactly `blocks` blocks (skip codes soak up the blocks the
        coded ones leave when the stream may hold them)."""
        if not self.skips:
            left, k = nbytes, blocks
            if not self._exact_ok(left, k):
                raise Infeasible(f"{nbytes} bytes for exactly {blocks} coded blocks")
            while k:
                wts = self._weights(left / k)
                cands = [(kind, wts[kind]) for kind, s in zip(("solid", "two", "eight"), self.sizes) if self._exact_ok(left - s, k - 1)]
                it = self.rand(self._pick(cands))
                self.add(it)
                left -= self.size(it)
                k -= 1
            return
        for j in range(1, 64):
            items, c = self._random_codes(nbytes - 2 * j, blocks - j, False)
            spare = blocks - c
            if not j <= spare <= 1023 * j:
                continue
            counts = [1] * j
            spare -= j
            while spare:
                i = int(self.rng.integers(0, j))
                d = min(spare, 1023 - counts[i], int(self.rng.integers(1, 1024)))
                counts[i] += d
                spare -= d
            for n in counts:
                items.insert(int(self.rng.integers(0, len(items) + 1)), ("skip", n))
            for it in items:
                self.add(it)
            return
        raise Infeasible(f"{nbytes} bytes for exactly {blocks} blocks")

    def place(self, item, boundary, back, max_blocks):
        """`item` so that it starts `back` slots before byte `boundary`; random filler in front.  Records the claim."""
        self.fill_to(boundary - 2 * back, max_blocks)
        at = self.add(item)
        slots = self.size(item) // 2
        self.claims.append({"boundary": boundary, "back": back, "slots": slots, "at": at, "kind": item[0],
                            "entry": (slots - back) if back else 0})
        return at

    def finish(self, dense=False):
        """Random valid codes until every block is covered."""
        wts = {"solid": 0.05, "two": 0.15, "eight": 0.8} if dense else {"solid": 0.25, "two": 0.5, "eight": 0.25}
        while self.blocks < self.nb:
            cands = list(wts.items())
            if self.skips:
                cands.append((("skip", min(int(self.rng.integers(1, 40)), self.nb - self.blocks)), 0.06))
            it = self._pick(cands)
            self.add(self.rand(it) if isinstance(it, str) else it)
        return self


# ---- the catalogue ------------------------------------------------------------------------------------------------------------
@dataclass
class Case:
    name: str
    group: str
    bits: int
    w: int
    h: int
    frames: list                 # [(bytes, is_key)]
    pictures: list               # per frame: flat uint32 picture by construction, or None (malformed / raises: oracle only)
    host: list                   # per frame: True — the on-GPU parse hands the frame to the host parser, by design
    layouts: list                # per frame: the assembler's layout
    consumed: list               # per frame: bytes up to the end of the code that covers the last block (-1: the data ends first)
    coded: list                  # per frame: coded blocks on the chain
    claims: list = field(default_factory=list)   # placements of the directed (last) frame
    raises: bool = False         # the reference raises on the directed frame
    why_host: str = ""

    @property
    def directed(self):
        return len(self.frames) - 1

    @property
    def key_case(self):
        return len(self.frames) == 1 and self.frames[0][1]

    @property
    def any_host(self):
        return any(self.host)


def _rng(*what):
    return np.random.default_rng(zlib.crc32(repr(what).encode()))


@functools.lru_cache(maxsize=None)
def palette(bits):
    if bits != 8:
        return None
    q = np.random.default_rng(77).integers(0, 256, (256, 4), dtype=np.uint8)
    q[:, 3] = 0                      # RGBQUADs (B, G, R, 0), as found behind the BITMAPINFOHEADER
    return q.tobytes()


@functools.lru_cache(maxsize=None)
def key_frame(bits, w, h):
    """The key frame in front of the inter-frame cases of one geometry: random codes, no skips -> Assembled."""
    s = Stream(bits, w, h, _rng("key", bits, w, h)).finish()
    return assemble(bits, w, h, s.items, None, palette(bits))


def _budget(bits, offset):
    """Blocks a frame may have used up at byte `offset` so that its densest continuation still reaches three 16 KiB tiles."""
    return int(offset / (15.0 if bits == 16 else 8.5)) + 8


def _case(name, group, bits, w, h, stream_or_items, key, host=False, why="", claims=None, alone=False):
    items = stream_or_items.items if isinstance(stream_or_items, Stream) else list(stream_or_items)
    claims = claims if claims is not None else (stream_or_items.claims if isinstance(stream_or_items, Stream) else [])
    if key or alone:
        a = assemble(bits, w, h, items, None, palette(bits))
        clip = [(a, key)]
    else:
        k = key_frame(bits, w, h)
        a = assemble(bits, w, h, items, k.picture, palette(bits))
        clip = [(k, True), (a, False)]
    raises = a.skip_codes > 0 and (key or alone)
    return Case(name, group, bits, w, h, [(x.data, kf) for x, kf in clip], [x.picture for x, _ in clip],
                [False] * (len(clip) - 1) + [bool(host)], [x.layout for x, _ in clip], [x.consumed for x, _ in clip],
                [x.coded for x, _ in clip], list(claims), raises, why)


GROUP_LANES = (10, 19, 28)       # where the first lane groups of the in-wave walk end (10 + 6 x 9 lanes a wave)
WAVE_LANES = (64, 128, 192)      # where the waves of a tile end
LANE_BYTES = (SMALL_TILE // LANES, BATCH_TILE // LANES)     # 16- and 32-slot lanes
STRADDLE_BOUNDARIES = tuple(sorted(
    {lane * nbytes for lane in GROUP_LANES + WAVE_LANES for nbytes in LANE_BYTES}      # inside the first tile
    | {SMALL_TILE + 10 * LANE_BYTES[0], BATCH_TILE + 19 * LANE_BYTES[1], BATCH_TILE + 128 * LANE_BYTES[1]}   # inside a later tile
    | {SMALL_TILE, BATCH_TILE, 2 * BATCH_TILE}))
# (lane-group boundaries of the in-wave walk at lanes 10, 19 and 28 and every wave boundary for 16- and 32-slot lanes, a group
# and a wave boundary inside a later tile of either size, then the first and second multiple of 8 KiB and of 16 KiB — and with
# 24576 the third of 8 KiB)


@functools.lru_cache(maxsize=None)
def catalogue(bits):
    """The cases of one bit depth, in a fixed order."""
    w, h = SIZES[bits]
    nb = (w // 4) * (h // 4)
    bw, bh = BIG
    bnb = (bw // 4) * (bh // 4)
    slots = KIND_SLOTS[bits]
    cases = []

    def S(name, skips, size=None):
        return Stream(bits, *(size or (w, h)), _rng(name, bits), skips)

    def add(name, group, s, key, **kw):
        size = (s.w, s.h) if isinstance(s, Stream) else (w, h)
        cases.append(_case(f"{name}_{'key' if key else 'inter'}", group, bits, *size, s, key, **kw))

    def valid_bytes(rng, n):
        """The first n bytes of a random well-formed frame."""
        return assemble(bits, w, h, Stream(bits, w, h, rng).finish().items, None, palette(bits)).data[:n]

    # -- straddles: every multi-slot kind, back = 0 .. slots - 1, at every boundary of STRADDLE_BOUNDARIES in one frame
    for kind in ("two", "eight"):
        for back in range(slots[kind]):
            for key in (True, False):
                s = S(f"straddle_{kind}_{back}_{key}", not key)
                for b in STRADDLE_BOUNDARIES:
                    s.place(s.rand(kind), b, back, _budget(bits, b - s.nbytes))
                add(f"straddle_{kind}_back{back}", "straddle" if not (bits == 16 and back == 1) else "straddle+halo", s.finish(dense=True), key)

    # -- halo word, data ending right behind it (16-bit): the flags word on a tile's last slot, its first colour the last word of the data
    if bits == 16:
        for tile in TILES:
            for kind, c0 in (("two", 0x1234), ("eight", 0x9234)):
                s = S(f"halo_end_{kind}_{tile}", True)
                s.fill_to(tile - 2, _budget(bits, tile))
                s.add(("raw", bytes([0x5A, 0x3C, c0 & 0xFF, c0 >> 8])))
                add(f"halo_end_{kind}_{tile // 1024}k", "halo", s, False, host=True, why="the data ends inside the code: too short")

    # -- end of data
    for tile in TILES:
        for key in ((False, True) if tile == BATCH_TILE else (False,)):
            s = S(f"end_exact_{tile}_{key}", not key)
            s.fill_exact(tile, nb)
            add(f"end_exact_{tile // 1024}k", "end", s, key)
        for past in (2, 4, 16):
            s = S(f"end_past_{tile}_{past}", True)
            s.fill_exact(tile + past, nb)
            add(f"end_{past}_past_{tile // 1024}k", "end", s, False)
        s = S(f"end_midcode_{tile}", True)
        s.place(s.rand("eight"), tile + 4, 0, _budget(bits, tile))
        cut = assemble(bits, w, h, s.items, key_frame(bits, w, h).picture, palette(bits)).data[: tile + 10]
        add(f"end_midcode_{tile // 1024}k", "end", [("raw", cut)], False, host=True, why="the data ends inside a code of the second tile: too short")
    s = S("end_odd_pad", True)
    s.fill_exact(BATCH_TILE, nb)
    s.add(("raw", b"\x00"))
    add("end_odd_pad", "end", s, False)

    # -- trailing bytes: every block covered inside the first tile, one and two further tiles of bytes behind
    for key in (True, False):
        cover = 12000 if (key and bits == 8) else 7000
        for fill in ("random", "zeros", "8400"):
            for total in (2 * BATCH_TILE, 3 * BATCH_TILE):
                s = S(f"trailing_{fill}_{total}_{key}", not key)
                s.fill_exact(cover, nb)
                n = total - cover
                tail = {"random": s.rng.integers(0, 256, n, dtype=np.uint8).tobytes(), "zeros": bytes(n), "8400": b"\x00\x84" * (n // 2)}[fill]
                s.add(("raw", tail))
                add(f"trailing_{fill}_{total // BATCH_TILE}tiles", "trailing", s, key)

    # -- skips across tiles
    for tile in TILES:
        s = S(f"skip_last_slot_{tile}", True)
        s.place(("skip", 37), tile, 1, _budget(bits, tile))
        add(f"skip_run_last_slot_{tile // 1024}k", "skip", s.finish(dense=True), False)
        for where, back in (("last", 1), ("first", 0)):
            s = S(f"skip_rest_{where}_{tile}", True)
            s.place(("skip", 0), tile, back, _budget(bits, tile))
            s.add(("raw", valid_bytes(s.rng, 3000)))
            add(f"skip_rest_{where}_slot_{tile // 1024}k", "skip", s, False)
    # skip counts of 1023 back to back: one tile's span past the 8192 blocks msv1_parse_emit stages and past two 4096-block windows
    s = S("skip1023_tile0", True, BIG)
    s.add(s.rand("solid"))
    for _ in range(4):
        s.add(("skip", 1023))
    s.add(s.rand("two"))
    for _ in range(5):
        s.add(("skip", 1023))
    s.add(s.rand("eight"))
    add("skip1023_tile0", "skip", s.finish(), False)
    s = S("skip1023_tile1", True, BIG)
    s.fill_to(BATCH_TILE - 2, BATCH_TILE // s.sizes[2] + 150)
    for _ in range(8):
        s.add(("skip", 1023))
        s.add(s.rand("solid"))
    add("skip1023_tile1", "skip", s.finish(), False)

    # -- saturation: whole tiles of "skip the rest of the frame" (0xFFFFF blocks each in the parse: the sums pass 2^28)
    for ntiles in (1, 3):
        add(f"saturate_{ntiles}tiles", "saturate", [("skip", 0), ("raw", b"\x00\x84" * (ntiles * BATCH_TILE // 2 - 1))], False)
    s = S("saturate_after_codes", True)
    s.fill_to(3000, 600)
    s.add(("skip", 0))
    s.add(("raw", b"\x00\x84" * ((3 * BATCH_TILE - s.nbytes) // 2)))
    add("saturate_after_codes", "saturate", s, False)

    # -- staging windows: a 16 KiB tile of one-slot solid codes is 8192 blocks, two windows of 4096
    for key in (True, False):
        for name, rest in (("first", 3000), ("second", 6000)):
            s = S(f"window_{name}_{key}", not key, BIG)
            s.fill_exact(BATCH_TILE, bnb - rest)
            for _ in range(rest):
                s.add(s.rand("solid"))
            extra = Stream(bits, bw, bh, s.rng)
            s.add(("raw", b"".join(encode_item(bits, extra.rand("solid")) for _ in range(BATCH_TILE // 2 - rest))))
            add(f"window_last_block_in_{name}", "window", s, key)
    s = S("window_all_solid", False, BIG)
    for _ in range(bnb):
        s.add(s.rand("solid"))
    add("window_all_solid", "window", s, True)

    # -- 8-bit end marker
    if bits == 8:
        for tile in TILES:
            for where, at in (("first_slot", tile), ("last_slot", tile - 2)):
                s = S(f"marker_{where}_{tile}", True)
                s.fill_to(at, _budget(bits, tile))
                s.add(("end",))
                s.add(("raw", valid_bytes(s.rng, 5000)))
                add(f"marker_{where}_{tile // 1024}k", "marker", s, False, host=True, why="an end marker on the chain")
            for back in (1, 2):     # 00 00 on the next tile's first slot, inside a 5-slot code: not on the chain
                for key in ((True, False) if tile == BATCH_TILE else (False,)):
                    s = S(f"marker_off_{tile}_{back}_{key}", not key)
                    idx = [int(v) for v in s.rng.integers(1, 256, 8)]
                    idx[2 * back - 2] = idx[2 * back - 1] = 0
                    s.place(("eight", 0x9ABC, tuple(idx)), tile, back, _budget(bits, tile))
                    add(f"marker_off_chain_back{back}_{tile // 1024}k", "marker", s.finish(dense=True), key)

    # -- a skip code with nothing to copy from: the reference raises
    s = S("skip_without_previous", True)
    s.add(("skip", 5))
    cases.append(_case("skip_without_previous", "raise", bits, w, h, s.finish(), False, host=True,
                       why="a skip code with no previous frame: the reference raises", alone=True))

    # -- batch layout: frames of 1, 2 and 3 tiles in mixed order, a too-short one and an all-skip one in the middle
    cases.append(_batch_layout(bits))
    names = [c.name for c in cases]
    assert len(set(names)) == len(names), "case names must be unique"
    return cases


def _batch_layout(bits):
    w, h = SIZES[bits]
    nb = (w // 4) * (h // 4)
    pal = palette(bits)
    clip, prev = [], None

    def frame(name, nbytes, key, skips=True):
        nonlocal prev
        s = Stream(bits, w, h, _rng("batch", name, bits), skips and not key)
        s.fill_exact(nbytes, nb)
        a = assemble(bits, w, h, s.items, prev, pal)
        clip.append((a, key, False))
        prev = a.picture
        return a

    frame("key3", 2 * BATCH_TILE + 7000, True)
    frame("one", 9000, False)
    frame("two", BATCH_TILE + 4000, False)
    full = frame("cut", BATCH_TILE + 5000, False)
    clip.pop()
    prev = clip[-1][0].picture
    clip.append((assemble(bits, w, h, [("raw", full.data[: BATCH_TILE + 1000])], prev, pal), False, True))   # too short
    prev = None   # (what the reference paints for the missing blocks is the oracle's to say: no picture by construction from here on)
    per = 3 if bits == 16 else 5
    clip.append((assemble(bits, w, h, [("skip", per)] * (nb // per), clip[1][0].picture, pal), False, False))   # all-skip
    for name, nbytes in (("three", 2 * BATCH_TILE + 3000), ("last", 5000)):
        s = Stream(bits, w, h, _rng("batch", name, bits), True)
        s.fill_exact(nbytes, nb)
        clip.append((assemble(bits, w, h, s.items, clip[1][0].picture, pal), False, False))
    pictures = [a.picture if i < 3 else None for i, (a, _, _) in enumerate(clip)]
    return Case("batch_layout", "batch", bits, w, h, [(a.data, k) for a, k, _ in clip], pictures, [hst for _, _, hst in clip],
                [a.layout for a, _, _ in clip], [a.consumed for a, _, _ in clip], [a.coded for a, _, _ in clip], [], False,
                "one member's data ends in its second tile: too short")


def tile_count(nbytes, tile=BATCH_TILE):
    return (nbytes + tile - 1) // tile
