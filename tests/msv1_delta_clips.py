"""Directed clips for the inter frame that spans a gap of an MSVideo1 seek index (jsp_index_delta_frames,
jsplayer_amd/csrc/msv1_index_delta_kernels.hip) — a helper module, plain Python, no tests of its own.  Built on msv1_range_clips.Idle
and the code helpers of msv1_keyframe_cut_clips; truth for them is tests/index_delta_ref.py, which test_index_delta_ref_cpu.py pins to
the oracle on every clip here.

The kernels give a lane 4 consecutive blocks, a wave 256, a workgroup 1024; a skip word never crosses a multiple of 1023.  SIZES are
the pictures whose block counts put those two grids against each other: 1023, 1024, 1025, 2046, 2048, 4096, and 6 blocks (fewer than
two lanes' share).  `seams(bits, w, h)` is one clip per size: a key frame, then one inter frame per PATTERN — the blocks the frame
WRITES (those outside the picture dropped).  Delta(f - 1, f) sees pattern f alone; the other pairs see unions of consecutive patterns.

  spots     single written blocks at 0, the lane seam (3, 4), the wave seam (255, 256), 1022 .. 1025, 2045 .. 2048, the last block
  nothing   a gap that writes nothing: ceil(nblocks / 1023) skip words, at 16 bits below the early-out threshold
  every     a gap that writes everything: no skip word; from -1 it is KeyFrame
  to_1023   all but blocks 1000 .. 1022: a run that ends exactly at a multiple of 1023
  to_wg     all but blocks 1000 .. 1023: a run that ends exactly at a workgroup's end, with the multiple of 1023 inside it
  across    all but blocks 1023 .. 3071 (or to the end): a run from a workgroup's last block across the whole next one into the
            third — the two-workgroup look-ahead — with multiples of 1023 (2046, 3069) inside it
  singles   every other block: isolated single-block skips between codes of every length (the kinds go round by block number)
  last      the last block alone: one run from block 0 over every multiple of 1023
  first     block 0 alone: a run that ends at nblocks
  wg_first  blocks 1024 and 2048 alone: runs that end on a workgroup's first block

`cuts(bits)` is msv1_keyframe_cut_clips.firsts_cut: a lone "cut" at each block of P7, for the refusals."""
import msv1_keyframe_cut_clips as kc
from msv1_range_clips import Idle

SIZES = ((124, 132), (128, 128), (164, 100), (124, 264), (128, 256), (256, 256), (12, 8))
NBLOCKS = (1023, 1024, 1025, 2046, 2048, 4096, 6)
SPOTS = (0, 3, 4, 255, 256, 1022, 1023, 1024, 1025, 2045, 2046, 2047, 2048)
PATTERNS = ("spots", "nothing", "every", "to_1023", "to_wg", "across", "singles", "last", "first", "wg_first")


def pattern(name, nb):
    """The blocks the frame of this pattern writes in a picture of nb blocks."""
    every = range(nb)
    if name == "spots":
        return sorted({b for b in SPOTS + (nb - 1,) if b < nb})
    if name == "nothing":
        return []
    if name == "every":
        return list(every)
    if name == "to_1023":
        return [b for b in every if not 1000 <= b < 1023]
    if name == "to_wg":
        return [b for b in every if not 1000 <= b < 1024]
    if name == "across":
        return [b for b in every if not 1023 <= b < 3072]
    if name == "singles":
        return [b for b in every if b % 2 == 0]
    if name == "last":
        return [nb - 1]
    if name == "first":
        return [0]
    if name == "wg_first":
        return [b for b in (1024, 2048) if b < nb]
    raise KeyError(name)


_cache = {}


def seams(bits, w, h):
    """The clip of one size, built once: kc.Clip with .patterns = {frame: name}."""
    if (bits, w, h) not in _cache:
        g = Idle(bits, w, h, seed=31 + w + h)
        frames, keys, names = [g.key()], [True], {}
        for k, name in enumerate(PATTERNS):
            names[len(frames)] = name
            frames.append(kc.whole(g, pattern(name, g.nb), k))
            keys.append(False)
        c = kc.Clip(f"seams_{w}x{h}", g, frames, keys, starts=(0,))
        c.patterns = names
        _cache[(bits, w, h)] = c
    return _cache[(bits, w, h)]


def pairs(n, first=-1):
    """Every pair (a, b], first <= a < b < n."""
    return [(a, b) for a in range(first, n) for b in range(a + 1, n)]


def cuts(bits):
    return kc.family("firsts", bits)[0]
