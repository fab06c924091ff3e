"""Reference for the MSVideo1 16-bit encoder (jsp_msv1_encode_frames / Msv1Encoder.EncodeFrames) — a helper module, plain Python, no
tests of its own.  The skip word and the run-head rule are index_delta_ref's.

THE RULE (include/jsplayer_amd.h, "Encode"; the decoder it inverts: MSVideo1.hx:119-181).
A picture is width x height 32-bit words, row y at y * pitch; nbx = width >> 2, nby = height >> 2 blocks in table order, pixel
k = 4 * y + x of a block is flag bit k; the width % 4 / height % 4 remainder pixels are never read.
  q(p) = ((p >> 3) & 0x1F) | ((p >> 6) & 0x3E0) | ((p >> 9) & 0x7C00) — no other bit of a word is read;  v[k] = q(p[k]).
Quadrant i holds pixels QUADS[i]; its last pixel is QUADS[i][3]; its colour pair is stream colours 2i (bit SET) and 2i + 1 (CLEAR).
The code of a block, on v alone:
  1. all 16 equal c: the word 0x8000 | c — unless (c & 0x7C00) == 0x0400, whose high byte 0x84..0x87 would be a skip: then the six
     bytes 00 00, c, c;
  2. exactly two distinct values: B = v[15], A the other; the word has bit k set where v[k] == A; then A, B;
  3. otherwise 18 bytes: the word, F0 | 0x8000, S0, F1, S1, F2, S2, F3, S3.  A quadrant of at most two values: S = the last pixel's,
     F the other (F = S when there is one), bits set where v[k] != S.  A quadrant of three or four values: Y = R + 2 G + B of the 5-bit
     fields, T the sum of the four Y, a pixel is high when 4 Y > T; the last pixel's group is the pixels on its side of that test;
     S = per channel floor((sum + n // 2) / n) over that group, F the same over the other group (F = S when it is empty); bits are
     set for the other group.
Key(P) = the codes of blocks 0 .. nblocks-1.  Inter(Q, P): block i is CODED when v of P differs from v of Q in one of its 16
pixels; the frame is index_delta_ref's rule with "written" read as "coded".

`wrong` states one of three deliberately wrong variants (WRONG), each of which test_msv1_encode_ref_cpu.py shows to miss."""
import numpy as np

from index_delta_ref import RUN, skip_word

WRONG = ("colour_order_by_value",   # the colour pair is ordered by value (smaller first), not tied to the last pixel
         "solid_red_one",           # a solid block of red field 1 gets the two-byte word, which the decoder reads as a skip
         "compare_words")           # Inter compares the 32-bit words, not the quantised values
QUADS = ((0, 1, 4, 5), (2, 3, 6, 7), (8, 9, 12, 13), (10, 11, 14, 15))


def q(p):
    p = int(p) & 0xFFFFFFFF
    return ((p >> 3) & 0x1F) | ((p >> 6) & 0x3E0) | ((p >> 9) & 0x7C00)


def from_rgb15(c):
    """What the decoder makes of a 15-bit colour (MSVideo1.hx:211-214)."""
    return ((c & 0x1F) << 3) | ((c & 0x3E0) << 6) | ((c & 0x7C00) << 9)


def blocks_of(pic, width, height):
    """The 16 words of every block in table order, from a (height, width) array (any pitch and sign are the caller's slicing)."""
    pic = np.asarray(pic).reshape(height, -1)[:, :width].astype(np.int64) & 0xFFFFFFFF
    nbx, nby = width >> 2, height >> 2
    return [[int(pic[4 * by + y, 4 * bx + x]) for y in range(4) for x in range(4)] for by in range(nby) for bx in range(nbx)]


def _luma(c):
    return (c & 0x1F) + 2 * ((c >> 5) & 0x1F) + ((c >> 10) & 0x1F)


def _mean(cs):
    n = len(cs)
    out = 0
    for sh in (0, 5, 10):
        out |= ((sum((c >> sh) & 0x1F for c in cs) + n // 2) // n) << sh
    return out


def _le16(*words):
    return b"".join(bytes([w & 0xFF, (w >> 8) & 0xFF]) for w in words)


def quadrant(v, i, wrong=None):
    """(F, S, the bits of the word this quadrant sets)."""
    idx = QUADS[i]
    last = v[idx[3]]
    vals = {v[k] for k in idx}
    if len(vals) <= 2:
        S = last
        F = next((v[k] for k in idx if v[k] != S), S)
        if wrong == "colour_order_by_value":
            F, S = max(vals), min(vals)
        return F, S, sum(1 << k for k in idx if v[k] != S)
    ys = [_luma(v[k]) for k in idx]
    T = sum(ys)
    high = [4 * y > T for y in ys]
    mine = [k for k, h in zip(idx, high) if h == high[3]]
    other = [k for k in idx if k not in mine]
    S = _mean([v[k] for k in mine])
    F = _mean([v[k] for k in other]) if other else S
    return F, S, sum(1 << k for k in other)


def code(v, wrong=None):
    """The code of a block from its 16 quantised values."""
    vals = set(v)
    if len(vals) == 1:
        c = v[15]
        if (c & 0x7C00) != 0x0400 or wrong == "solid_red_one":
            return _le16(0x8000 | c)
        return _le16(0, c, c)
    if len(vals) == 2:
        B = v[15]
        A = next(x for x in v if x != B)
        if wrong == "colour_order_by_value":
            A, B = max(vals), min(vals)
        return _le16(sum(1 << k for k in range(16) if v[k] == A), A, B)
    word, colours = 0, []
    for i in range(4):
        F, S, bits = quadrant(v, i, wrong)
        word |= bits
        colours += [F, S]
    colours[0] |= 0x8000
    return _le16(word, *colours)


def key(pic, width, height, wrong=None):
    return b"".join(code([q(p) for p in blk], wrong) for blk in blocks_of(pic, width, height))


def coded_blocks(prev, pic, width, height, wrong=None):
    """Per block: whether Inter(prev, pic) codes it."""
    a, b = blocks_of(prev, width, height), blocks_of(pic, width, height)
    if wrong == "compare_words":
        return [x != y for x, y in zip(a, b)]
    return [[q(p) for p in x] != [q(p) for p in y] for x, y in zip(a, b)]


def inter(prev, pic, width, height, wrong=None):
    blocks = blocks_of(pic, width, height)
    coded = coded_blocks(prev, pic, width, height, wrong)
    nb = len(blocks)
    out = bytearray()
    for i in range(nb):
        if coded[i]:
            out += code([q(p) for p in blocks[i]], wrong)
            continue
        if not (i == 0 or coded[i - 1] or i % RUN == 0):
            continue
        nxt = next((k for k in range(i + 1, nb) if coded[k]), nb)
        out += skip_word(min(nxt, (i // RUN + 1) * RUN, nb) - i)
    return bytes(out)


def encode(pictures, previous, width, height, wrong=None):
    """One frame per picture: Key when its previous is None, else Inter."""
    previous = previous if previous is not None else [None] * len(pictures)
    return [key(p, width, height, wrong) if r is None else inter(r, p, width, height, wrong) for p, r in zip(pictures, previous)]


def exact_picture(rng, width, height, kinds=("solid", "solid_red_one", "two_last_high", "two_last_low", "quad_one", "quad_two")):
    """A picture every MSVideo1 16-bit decoder could have produced: words are from_rgb15 of something and every quadrant has at most two
    colours.  Blocks cycle through `kinds` so that each is there by construction; remainder pixels are random words."""
    pic = rng.integers(0, 1 << 32, size=(height, width), dtype=np.uint64).astype(np.uint32)
    nbx, nby = width >> 2, height >> 2
    for by in range(nby):
        for bx in range(nbx):
            kind = kinds[(by * nbx + bx) % len(kinds)]
            v = [0] * 16
            if kind == "solid":
                c = int(rng.integers(0, 0x8000))
                c = c if (c & 0x7C00) != 0x0400 else c ^ 0x4000
                v = [c] * 16
            elif kind == "solid_red_one":
                v = [0x0400 | int(rng.integers(0, 0x400))] * 16
            elif kind in ("two_last_high", "two_last_low"):
                a = int(rng.integers(0, 0x8000))
                b = (a + 1 + int(rng.integers(0, 0x7FFE))) % 0x8000
                hi, lo = max(a, b), min(a, b)
                v = [hi if rng.integers(0, 2) else lo for _ in range(16)]
                v[0], v[15] = (lo, hi) if kind == "two_last_high" else (hi, lo)
            else:
                for i, idx in enumerate(QUADS):
                    a = int(rng.integers(0, 0x8000))
                    b = a if kind == "quad_one" else (a + 1 + int(rng.integers(0, 0x7FFE))) % 0x8000
                    for n, k in enumerate(idx):
                        v[k] = b if n == (i % 4) else a
            for k in range(16):
                pic[4 * by + k // 4, 4 * bx + k % 4] = from_rgb15(v[k])
    return pic


def lossy_picture(rng, width, height):
    """Random 32-bit words with the top byte set: nearly every quadrant has four colours."""
    return (rng.integers(0, 1 << 24, size=(height, width), dtype=np.uint64).astype(np.uint32) | np.uint32(0xFF000000))


def rgb(r, g, b):
    """The 15-bit value of 5-bit fields."""
    return (r << 10) | (g << 5) | b


# quadrant values (pixels in the order of QUADS[i], the last one last) for the lossy step's corners
EQUAL_Y = (rgb(4, 0, 0), rgb(0, 2, 0), rgb(0, 0, 4), rgb(2, 1, 0))        # four colours, Y = 4 each: nobody is high, F = S = the mean
LAST_ALONE = (rgb(1, 0, 0), rgb(0, 1, 0), rgb(0, 0, 1), rgb(31, 31, 31))  # the last pixel alone on the high side: S = itself
LAST_ALONE_LOW = (rgb(31, 30, 31), rgb(30, 31, 31), rgb(31, 31, 30), rgb(0, 0, 1))   # ... and alone on the low side
THREE = (rgb(9, 9, 9), rgb(9, 9, 9), rgb(20, 3, 7), rgb(1, 30, 2))        # three distinct values


def directed_picture(width, height, top=0xFF000000):
    """A picture whose blocks cycle through the corners above, one per quadrant position; remainder pixels are `top`."""
    pic = np.full((height, width), top, dtype=np.uint32)
    corners = (EQUAL_Y, LAST_ALONE, LAST_ALONE_LOW, THREE)
    nbx, nby = width >> 2, height >> 2
    for blk in range(nbx * nby):
        by, bx = divmod(blk, nbx)
        for i, idx in enumerate(QUADS):
            vals = corners[(blk + i) % 4]
            for n, k in enumerate(idx):
                pic[4 * by + k // 4, 4 * bx + k % 4] = from_rgb15(vals[n]) | top | (blk & 7)   # (bits q drops: must not matter)
    return pic


def change_blocks(rng, pic, width, blocks, dropped_bits_only=False):
    """A copy of `pic` in which exactly `blocks` change: every pixel of them gets a new value (or, dropped_bits_only, a change in
    bits q drops — which codes nothing)."""
    out = pic.copy()
    nbx = width >> 2
    for blk in blocks:
        by, bx = divmod(blk, nbx)
        tile = out[4 * by:4 * by + 4, 4 * bx:4 * bx + 4]
        if dropped_bits_only:
            tile ^= np.uint32(0x5A070307)
        else:
            tile ^= np.uint32(0x00080808 << int(rng.integers(0, 5)))   # one bit of every 5-bit field flips
    return out
