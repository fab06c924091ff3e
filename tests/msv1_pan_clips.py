"""Directed clips for the frames of a block rectangle that MOVES over an MSVideo1 seek index (jsp_index_pan_frames,
jsplayer_amd/csrc/msv1_index_pan_kernels.hip) — a helper module, plain Python, no tests of its own.  Truth for them is
tests/index_pan_ref.py, which test_index_pan_ref_cpu.py pins to the oracle on every clip here.

One source picture: 192 x 192, 48 x 48 blocks.  Every block of every picture is ONE colour, coded as a 1-, 2- or 8-colour code in
turn by (block + frame) % 3: equal pixels come from unequal codes all the time.  At 8 bits the palette (`pal8`) holds every colour
twice, at index v and at v ^ 128, and a block that is to show what another block showed gets the OTHER index.  A frame codes the
blocks whose colour value differs from the picture before, so a block can be kept without a writer in the gap and dropped with one.

SIZES = 33x31 (1023 blocks, one run), 32x32 (1024, one workgroup), 41x25 (1025), 3x2 (6 blocks: fewer than two lanes' share).

  scroll(bits, size, how)   content moves over a flat background.  "follow": the rectangle moves with it — every moved pair is ALL
                            DROPPED; "lag": flat content moves one block a frame further than the rectangle — a border of kept
                            blocks, its leading and its trailing column; "against": the rectangle moves the other way.
  bounds(bits, size)        one frame per pattern of `patterns(size)`: the rectangle hops between two origins and the frame is built
                            so that exactly the pattern's blocks j are kept — the kept / dropped boundary on j = 3|4, 255|256,
                            1022|1023, 1023|1024, on every row start of the rectangle, "nothing" (all dropped) and "every" (all kept).
                            Every other kept block keeps the colour it had: it has NO writer in the gap.  In the frames of the odd
                            patterns every block outside the rectangle changes.
  cuts(bits)                frame 1 ends one byte short of the code of block CUT_AT: the decoder paints that block and every block
                            behind it from missing bytes.  A rectangle moved within the painted blocks drops them all though every
                            code is cut; one that straddles CUT_AT refuses there.
  befores(bits)             an index from frame BEFORE_START: blocks without a writer that equal, or differ from, the block at the
                            other origin in the picture before the range.

A clip is kc.Clip with .size, .pal, .pairs = [(a, b, A, B)] in index frames (a chain behind a KEY pair comes first: .chain of them),
.named = {pair: "all dropped" | "all kept" | ("none", j) | ("cut", j)} for the moved tight pairs that are not a mix.

  spliced(bits)             frames of `bounds` and then of `cuts` in one clip, for calls of different kinds on one index
                            (tests/test_index_clip_interleave_gpu.py); no pairs of its own."""
import numpy as np

import msv1_delta_clips as dc
import msv1_keyframe_cut_clips as kc
from index_crop_ref import KEY, src
from msv1_range_clips import Idle, palette

W = H = 192
NBX = NBY = 48
NB = NBX * NBY
SIZES = ((33, 31), (32, 32), (41, 25), (3, 2))
HOWS = ("follow", "lag", "against")

_cache = {}


def size_id(size):
    return "%dx%d" % tuple(size)


def pal8():
    """The 8-bit palette: 128 different colours, entry v ^ 128 a copy of entry v."""
    if "pal" not in _cache:
        pal = bytearray(palette(8))
        for i in range(128):
            pal[4 * i:4 * i + 3] = bytes([i, 255 - i, (37 * i) & 255])
            pal[4 * (i + 128):4 * (i + 128) + 4] = pal[4 * i:4 * i + 4]
        _cache["pal"] = bytes(pal)
    return _cache["pal"]


class Paint:
    """Pictures of one colour value per block, and the frames between them."""

    def __init__(self, bits, seed):
        self.bits = bits
        self.g = Idle(bits, W, H, seed)
        self.rng = np.random.default_rng(seed)

    def same(self, u, v):
        return (u & 127) == (v & 127) if self.bits == 8 else u == v

    def colour(self, *avoid):
        while True:
            v = int(self.rng.integers(1, 128)) if self.bits == 8 else self.g.colour()
            if not any(self.same(v, u) for u in avoid):
                return v

    def twin(self, v):
        """Another value of the same pixels where the format has one."""
        return v ^ 128 if self.bits == 8 else v

    def code(self, b, t, v):
        return kc.code(self.g, kc.KINDS[(b + t) % 3], v)

    def key(self, pic, t=0):
        return self.g.encode([self.code(b, t, v) for b, v in enumerate(pic)])

    def frame(self, prev, pic, t):
        return self.g.encode([self.code(b, t, v) if v != prev[b] else None for b, v in enumerate(pic)])


def _clip(name, p, size, frames, start=0):
    c = kc.Clip(name, p.g, frames, [True] + [False] * (len(frames) - 1), starts=(start,))
    c.size, c.pal, c.start = size, (pal8() if p.bits == 8 else None), start
    c.pairs, c.chain, c.named = [], 0, {}
    return c


def _slab(pic, x0, y0, w, h, colour_of):
    for y in range(y0, y0 + h):
        for x in range(x0, x0 + w):
            if 0 <= x < NBX and 0 <= y < NBY:
                pic[y * NBX + x] = colour_of(x - x0, y - y0)


def scroll(bits, size, how):
    k = ("scroll", bits, size, how)
    if k in _cache:
        return _cache[k]
    bw, bh = size
    p = Paint(bits, 101 + 7 * bw + bh + HOWS.index(how))
    bg = p.colour()
    small = bw < 5
    if how == "follow":
        n, cw, ch = 4, max(1, bw - 2), max(1, bh - 2)
        rect = [(1 + t, 1 + t) for t in range(n)]
        at = [(r[0] + (1 if bw > 2 else 0), r[1] + (1 if bh > 2 else 0)) for r in rect]
    elif how == "lag":
        n, cw, ch = (3 if small else 4), max(1, bw - 4), max(1, bh - 2)
        rect = [(1 + t, 1 + t) for t in range(n)]
        at = [(r[0] + t, r[1] + (1 if bh > 2 else 0)) for t, r in enumerate(rect)]
    else:
        n, cw, ch = (2 if small else 3), max(1, bw - 4), max(1, bh - 2)
        rect = [(4 - t, 2) for t in range(n)]
        at = [(4 + t, 2 + (1 if bh > 2 else 0)) for t in range(n)]
    fg = p.colour(bg)
    content = [[fg if how == "lag" else p.colour(bg) for _ in range(cw)] for _ in range(ch)]
    pics = []
    for t in range(n):
        pic = [bg] * NB
        _slab(pic, at[t][0], at[t][1], cw, ch, lambda x, y, t=t: content[y][x] if t % 2 == 0 else p.twin(content[y][x]))
        pics.append(pic)
    frames = [p.key(pics[0])] + [p.frame(pics[t - 1], pics[t], t) for t in range(1, n)]
    c = _clip(f"pan_scroll_{how}_{size_id(size)}", p, size, frames)
    c.rects = rect
    c.pairs = [(KEY, 0, None, rect[0])] + [(t - 1, t, rect[t - 1], rect[t]) for t in range(1, n)]
    c.chain = len(c.pairs)
    c.pairs += [(1, 1, rect[0], rect[1]), (-1, 1, rect[0], rect[1])]       # a pan across a standing picture; from before the range
    if n > 2:
        c.pairs += [(0, 2, rect[0], rect[2]), (0, 2, rect[1], rect[1])]      # a stride of two; a still pair among the moved ones
    if how == "follow":
        for q in c.pairs:
            if q[0] >= 0 and q[0] < q[1] and q[2] != q[3]:
                c.named[q] = "all dropped"
    c.named[(-1, 1, rect[0], rect[1])] = "all kept"                         # nothing before the range defines P(-1)
    _cache[k] = c
    return c


def patterns(size):
    """[(name, the blocks j the frame keeps)] for a rectangle of this size; a pattern that would keep nothing or everything is left
    out unless that is its name."""
    bw, bh = size
    nb = bw * bh
    every = range(nb)
    made = [("nothing", []), ("every", list(every)),
            ("from_4", [j for j in every if j >= 4]), ("to_4", [j for j in every if j < 4]),
            ("to_256", [j for j in every if j < 256]), ("from_256", [j for j in every if j >= 256]),
            ("to_1023", [j for j in every if j < 1023]), ("from_1023", [j for j in every if j >= 1023]),
            ("to_1024", [j for j in every if j < 1024]), ("from_1024", [j for j in every if j >= 1024]),
            ("row_starts", [j for j in every if j % bw == 0]), ("not_row_starts", [j for j in every if j % bw != 0]),
            ("from_row_2", [j for j in every if j >= bw]), ("to_row_2", [j for j in every if j < bw]),
            ("singles", [j for j in every if j % 2 == 0]), ("last", [nb - 1]), ("first", [0]),
            ("spots", dc.pattern("spots", nb)), ("to_wg", dc.pattern("to_wg", nb))]
    return [(name, ks) for name, ks in made if name in ("nothing", "every") or 0 < len(ks) < nb]


ORIGINS = ((2, 3), (3, 2))


def bounds(bits, size):
    k = ("bounds", bits, size)
    if k in _cache:
        return _cache[k]
    bw, bh = size
    nb = bw * bh
    p = Paint(bits, 131 + 5 * bw + bh)
    pic = [p.colour() for _ in range(NB)]
    frames = [p.key(pic)]
    pairs, names, kept, named = [(KEY, 0, None, ORIGINS[0])], {}, {}, {}
    for i, (name, ks) in enumerate(patterns(size)):
        t = i + 1
        A, B = ORIGINS[i % 2], ORIGINS[(i + 1) % 2]
        ra, rb = (A[0], A[1], bw, bh), (B[0], B[1], bw, bh)
        keep = set(ks)
        new = list(pic)
        inside = set()
        for j in range(nb):
            sa, sb = src(NBX, ra, j), src(NBX, rb, j)
            inside.add(sb)
            if j not in keep:
                new[sb] = p.twin(pic[sa])
            elif j % 2 == 0 and not p.same(pic[sb], pic[sa]):
                new[sb] = pic[sb]                                   # kept, and no frame of the gap writes it
            else:
                new[sb] = p.colour(pic[sa])
        if i % 2 == 1:
            for b in range(NB):
                if b not in inside:
                    new[b] = p.colour(pic[b])
        frames.append(p.frame(pic, new, t))
        pair = (t - 1, t, A, B)
        pairs.append(pair)
        names[pair], kept[pair] = name, sorted(keep)
        if name in ("nothing", "every"):
            named[pair] = "all dropped" if name == "nothing" else "all kept"
        pic = new
    c = _clip(f"pan_bounds_{size_id(size)}", p, size, frames)
    c.pairs, c.patterns, c.kept, c.named, c.chain = pairs, names, kept, named, len(pairs)
    _cache[k] = c
    return c


CUT_SIZE = (6, 3)
CUT_AT = 10 * NBX + 20      # block (20, 10)


def cuts(bits):
    k = ("cuts", bits)
    if k in _cache:
        return _cache[k]
    p = Paint(bits, 171)
    pic = [p.colour() for _ in range(NB)]
    new = []
    for b, v in enumerate(pic):   # (no block shows what it or its left neighbour showed, or what that neighbour shows now)
        new.append(p.colour(v, pic[b - 1], new[b - 1] if b else v))
    whole = b"".join(p.code(b, 1, new[b]) for b in range(CUT_AT))
    frames = [p.key(pic), whole + p.code(CUT_AT, 1, new[CUT_AT])[:-1], p.g.encode([None] * NB)]
    c = _clip("pan_cuts", p, CUT_SIZE, frames)
    painted = ((5, 12), (6, 12))                                    # every block of both rectangles lies behind CUT_AT
    across = ((18, 10), (19, 10))                                   # block 1 of the rectangle at `to` is CUT_AT
    c.pairs = [(1, 1) + painted, (1, 2) + painted, (1, 1) + across, (0, 1) + across, (1, 2) + across, (0, 1, (10, 4), (11, 4))]
    for q in c.pairs[:2]:
        c.named[q] = "all dropped"
    for q in c.pairs[2:5]:
        c.named[q] = ("cut", 1)
    c.named[c.pairs[5]] = "all kept"
    _cache[k] = c
    return c


BEFORE_START = 3
BEFORE_SIZE = (6, 3)


def befores(bits):
    k = ("befores", bits)
    if k in _cache:
        return _cache[k]
    p = Paint(bits, 181)
    bg = p.colour()
    pic0 = [bg] * NB
    _slab(pic0, 40, 40, 4, 4, lambda x, y: p.colour(bg))
    pic1 = list(pic0)
    _slab(pic1, 20, 20, 10, 6, lambda x, y: p.colour(bg))            # the patch: in the picture before the range, never written in it
    pic2 = list(pic1)
    _slab(pic2, 40, 40, 4, 4, lambda x, y: p.colour(bg))
    pic3 = list(pic2)
    _slab(pic3, 10, 5, 6, 3, lambda x, y: p.colour(bg))              # index frame 0 writes these 18 blocks and nothing else
    pic4 = list(pic3)
    _slab(pic4, 12, 6, 1, 1, lambda x, y: p.colour(bg, pic3[6 * NBX + 12]))
    pics = [pic0, pic1, pic2, pic3, pic4]
    frames = [p.key(pic0)] + [p.frame(pics[t - 1], pics[t], t) for t in range(1, 5)]
    c = _clip("pan_befores", p, BEFORE_SIZE, frames, start=BEFORE_START)
    flat = ((0, 30), (1, 30))
    patch = ((19, 20), (20, 20))
    wrote = ((9, 4), (10, 4))
    c.pairs = [(-1, 0) + flat, (0, 1) + flat, (0, 0) + flat,          # no writer, equal in the picture before the range: dropped
               (-1, 0) + patch, (0, 1) + patch, (1, 1) + patch,        # no writer and different: refuses
               (-1, 0) + wrote, (0, 0) + wrote, (-1, 1) + wrote, (0, 1) + wrote, (1, 1) + wrote,   # row 4 unwritten and flat, rows 5, 6 written
               (KEY, 1, None, (10, 5)), (-1, 1, (10, 5), (10, 5))]
    for q in c.pairs[:3]:
        c.named[q] = "all dropped"
    for q in c.pairs[3:6]:
        c.named[q] = ("none", 0)
    _cache[k] = c
    return c


WANDER_SIZE = (64, 48)      # pixels: 16 x 12 blocks


def wander(bits, n=10):
    """A blob of 6 x 6 blocks of random colours that wanders over a flat background, (+7, -5) blocks a frame and back again from
    frame n // 2 on: what a rectangle of WANDER_SIZE has to follow (jsp_play --pan, Manager.follow).  kc.Clip; no pairs."""
    k = ("wander", bits, n)
    if k not in _cache:
        p = Paint(bits, 191)
        bg = p.colour()
        blob = [[p.colour(bg) for _ in range(6)] for _ in range(6)]
        pics = []
        for t in range(n):
            s = t if t < n // 2 else n - 1 - t
            pic = [bg] * NB
            _slab(pic, 2 + 7 * s, 34 - 5 * s, 6, 6, lambda x, y, t=t: blob[y][x] if t % 2 == 0 else p.twin(blob[y][x]))
            pics.append(pic)
        frames = [p.key(pics[0])] + [p.frame(pics[t - 1], pics[t], t) for t in range(1, n)]
        _cache[k] = _clip("pan_wander", p, None, frames)
    return _cache[k]


SPLICE_HEAD = 6             # frames of bounds(bits, (32, 32)) in front of a spliced clip


def spliced(bits):
    """One index for every clip call at once: the first SPLICE_HEAD frames of bounds(bits, (32, 32)) — the key frame and the patterns
    nothing, every, from_4, to_4, to_256 — then the cut frame of cuts(bits) (index frame SPLICE_HEAD: its data ends one byte short of
    the code of block CUT_AT) and that clip's empty frame.  A code carries no position and no reference, so the frames of two clips of
    one picture size and palette in a row are a clip.  kc.Clip without a size and without pairs."""
    k = ("spliced", bits)
    if k not in _cache:
        frames = list(bounds(bits, (32, 32)).frames[:SPLICE_HEAD]) + list(cuts(bits).frames[1:3])
        _cache[k] = _clip("pan_spliced", Paint(bits, 211), None, frames)
    return _cache[k]


def all_clips(bits):
    out = [scroll(bits, size, how) for size in SIZES for how in HOWS] + [bounds(bits, size) for size in SIZES]
    return out + [cuts(bits), befores(bits)]
