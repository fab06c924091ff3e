"""Directed clips for the TIGHT inter frame that spans a gap of an MSVideo1 seek index (jsp_index_tight_frames, the TIGHT form of
msv1_index_delta_sizes_kernel) — a helper module, plain Python, no tests of its own.  Built on msv1_range_clips.Idle, which keeps what
every block shows; truth for them is tests/index_tight_ref.py, which test_index_tight_ref_cpu.py pins to the oracle on every clip here.

`directed(bits, w, h)` is one clip per size of SIZES (1023, 1024, 1025, 2048 and 6 blocks: a lane owns 4 blocks, a wave 256, a
workgroup 1024, a skip word never crosses a multiple of 1023).  S = msv1_delta_clips.SPOTS inside the picture plus the last block.

  0 key           solid blocks
  1 recode_all    every block recoded with what it shows, the kinds of code in turn: Tight(0, 1) is ceil(nb / 1023) skip words,
                  Delta(0, 1) is as long as a key frame
  2 change_spots  new colours at S
  3 recode_next   new colours at the blocks s + 1; the blocks of S that are no such block recoded unchanged.  In Tight(2, 3) a dropped
                  block stands directly before a kept one at 0 | 1, 3 | 4 (lane), 255 | 256 (wave), 1022 | 1023 and 2045 | 2046
                  (multiples of 1023).  The blocks s + 2 outside S and s + 1 are recoded unchanged as well: a dropped block BEHIND a
                  kept one, with an unwritten block behind it, which must not become a run head
  4 back          the blocks of S take their colours of frame 1 again: Tight(1, 4) drops them — dropped blocks next to each other at
                  3, 4 and 255, 256 and 1022 .. 1025, so that the run-head test of the lane that looks at blk0 - 1 = 1023 sees a block
                  that is written but not kept; Tight(2, 4) and Tight(3, 4) keep them
  5 one_pixel     the 16 consecutive blocks 248 .. 263 (clipped to the picture; the picture's first 16 where it is smaller), which
                  straddle the wave seam: block k of them differs from what it showed in pixel k only, as a 2-colour code with one flag
                  bit (pixel 15: all flag bits but that one, the colours swapped — the flag word's top bit is not free)
  6 key_same      a key frame of the clip (its key flag set) with what the blocks hold: solid blocks as 2-colour codes, the blocks
                  of one_pixel with the bytes they have.  Tight(5, 6) is all skips and no key frame
  7 every         new colours everywhere: Tight = Delta = the frame's own bytes, a key frame
  8 recode_odd    (one more than the seams of frame 3 can hold: 1022 | 1023 and 1023 | 1024 cannot both be dropped | kept in one
                  frame) the odd blocks of S recoded unchanged, the blocks behind them given new colours: in Tight(7, 8) dropped |
                  kept at 3 | 4, 255 | 256, 1023 | 1024 (workgroup), 2045 | 2046, 2047 | 2048

`twins()` is an 8-bit clip whose palette holds one colour at two indices, and a block recoded from one index to the other.
`cut_dropped(bits, w, h)`: a frame that ends with HALF of the last block's solid code word, whose one byte paints the colour the block
already shows: the block's writer's code is cut, and Tight drops the block all the same."""
import msv1_delta_clips as dc
import msv1_keyframe_cut_clips as kc
import pyref_msv1
from msv1_range_clips import Idle, palette

SIZES = ((124, 132), (128, 128), (164, 100), (128, 256), (12, 8))
NBLOCKS = (1023, 1024, 1025, 2048, 6)
NAMES = ("key", "recode_all", "change_spots", "recode_next", "back", "one_pixel", "key_same", "every", "recode_odd")
SEAMS_3 = ((0, 1), (3, 4), (255, 256), (1022, 1023), (2045, 2046))        # dropped | kept in Tight(2, 3)
SEAMS_8 = ((3, 4), (255, 256), (1023, 1024), (2045, 2046), (2047, 2048))  # dropped | kept in Tight(7, 8)


def spots(nb):
    return sorted({b for b in dc.SPOTS + (nb - 1,) if b < nb})


def pixel_blocks(nb):
    first = 248 if nb > 248 else 0
    return list(range(first, min(first + 16, nb)))


def one_pixel_code(g, k, new, old):
    """A 2-colour code that shows `new` in pixel k and `old` in the 15 others."""
    if k < 15:
        return g.two(new, old, flags=1 << k)
    return g.two(old, new, flags=0x7FFF)


_cache = {}


def fresh(g, b, also=None):
    """A colour for block b whose frame-buffer word differs from the one the block shows (and from that of `also`): at 8 bits two
    indices may name one colour, and a random index is the old one once in 255."""
    if "pal" not in _cache:
        _cache["pal"] = pyref_msv1.palette_ints(palette(8))
    word = (lambda v: _cache["pal"][v]) if g.bits == 8 else (lambda v: v)
    while True:
        v = g.colour()
        if all(old is None or word(old) != word(v) for old in (g.col[b], also)):
            return v


def change(g, blocks, shift=0):
    """kc.mixed with colours that are `fresh`: every block of `blocks` changes in the frame buffer."""
    codes = [None] * g.nb
    for b in blocks:
        g.col[b] = fresh(g, b)
        codes[b] = kc.code(g, kc.KINDS[(b + shift) % 3], g.col[b])
    return codes


def directed(bits, w, h):
    """The clip of one size, built once: kc.Clip with .names = {frame: name}, .spots = S, .pixel_blocks."""
    if (bits, w, h) in _cache:
        return _cache[(bits, w, h)]
    g = Idle(bits, w, h, seed=71 + w + h)
    nb = g.nb
    S = spots(nb)
    frames, keys = [g.key()], [True]
    # 1 recode_all
    frames.append(g.encode([kc.code(g, kc.KINDS[b % 3], g.col[b]) for b in range(nb)]))
    first = list(g.col)
    # 2 change_spots
    frames.append(g.encode(change(g, S)))
    # 3 recode_next
    nxt = sorted({s + 1 for s in S if s + 1 < nb})
    codes = [None] * nb
    for b in nxt:   # (not the colour of frame 1 either: `back` changes the block again)
        g.col[b] = fresh(g, b, also=first[b])
        codes[b] = kc.code(g, kc.KINDS[(b + 1) % 3], g.col[b])
    after = sorted({s + 2 for s in S if s + 2 < nb} - set(S) - set(nxt))
    for s in [s for s in S if s not in nxt] + after:
        codes[s] = kc.code(g, kc.KINDS[(s + 2) % 3], g.col[s])
    frames.append(g.encode(codes))
    # 4 back
    codes = [None] * nb
    for s in S:
        g.col[s] = first[s]
        codes[s] = kc.code(g, kc.KINDS[s % 3], g.col[s])
    frames.append(g.encode(codes))
    # 5 one_pixel
    held = {}
    codes = [None] * nb
    for k, b in enumerate(pixel_blocks(nb)):
        held[b] = codes[b] = one_pixel_code(g, k, fresh(g, b), g.col[b])
        g.col[b] = None
    frames.append(g.encode(codes))
    # 6 key_same
    frames.append(g.encode([held[b] if b in held else g.two(g.col[b], g.col[b]) for b in range(nb)]))
    # 7 every
    frames.append(g.encode(change(g, range(nb), 2)))
    # 8 recode_odd
    odd = [s for s in S if s % 2 == 1]
    codes = change(g, [s + 1 for s in odd if s + 1 < nb], 2)
    for s in odd:
        codes[s] = kc.code(g, kc.KINDS[(s + 1) % 3], g.col[s])
    frames.append(g.encode(codes))
    keys += [False] * 5 + [True, False, False]
    c = kc.Clip(f"tight_{w}x{h}", g, frames, keys, starts=(0, 3))
    c.names = dict(enumerate(NAMES))
    c.spots, c.pixel_blocks, c.next_blocks, c.after, c.odd = S, pixel_blocks(nb), nxt, after, odd
    assert len(frames) == len(NAMES) == len(keys)
    _cache[(bits, w, h)] = c
    return c


TWINS = (17, 200)   # the two palette indices of one colour


def twins(w=12, h=8):
    """(clip, palette): 8 bits; the palette's entry TWINS[1] is made a copy of entry TWINS[0].  Frame 0 is a key frame in which block
    2 shows index TWINS[0]; frame 1 recodes block 2 as index TWINS[1] (other bytes, the same word in a frame buffer) and gives block
    4 a new colour; frame 2 recodes block 2 as a 2-colour code of both indices."""
    pal = bytearray(palette(8))
    i, j = TWINS
    pal[4 * j:4 * j + 4] = pal[4 * i:4 * i + 4]
    g = Idle(8, w, h, seed=73)
    g.key()
    g.col[2] = i
    frames = [g.encode([g.solid(v) for v in g.col])]
    codes = [None] * g.nb
    codes[2] = g.solid(j)
    g.col[4] = next(v for v in range(1, 256) if v not in (i, j, g.col[4]) and pal[4 * v:4 * v + 4] != pal[4 * g.col[4]:4 * g.col[4] + 4])
    codes[4] = g.solid(g.col[4])
    frames.append(g.encode(codes))
    codes = [None] * g.nb
    codes[2] = g.two(i, j, flags=0x1234)
    frames.append(g.encode(codes))
    c = kc.Clip("twins", g, frames, [True, False, False], starts=(0,))
    return c, bytes(pal)


CUT_SIZES = ((24, 8), (164, 100))
CUT_COLOUR = 0x5A   # (16 bits: below 0x100, so that the code word's first byte alone says it)


def cut_dropped(bits, w, h):
    """Frame 0: a key frame whose last block shows CUT_COLOUR.  Frame 1: new colours for every block but the last, then ONE byte,
    CUT_COLOUR — half of the last block's solid code word, which paints the block solid from that byte: the same picture, a cut code.
    Frame 2: a new colour for block 0.  Delta refuses (0, 1] and (0, 2] at the last block; Tight drops it."""
    if ("cut", bits, w, h) in _cache:
        return _cache[("cut", bits, w, h)]
    g = Idle(bits, w, h, seed=79 + w)
    g.key()
    last = g.nb - 1
    g.col[last] = CUT_COLOUR
    frames = [g.encode([g.solid(v) for v in g.col])]
    frames.append(b"".join(change(g, range(last), 1)[:last]) + bytes([CUT_COLOUR]))
    frames.append(g.encode(change(g, [0])))
    c = kc.Clip(f"cut_dropped_{w}x{h}", g, frames, [True, False, False], starts=(0,))
    c.last = last
    _cache[("cut", bits, w, h)] = c
    return c
