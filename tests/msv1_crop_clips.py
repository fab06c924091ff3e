"""Directed clips for the frames of a block rectangle of an MSVideo1 seek index (jsp_index_crop_frames,
jsplayer_amd/csrc/msv1_index_crop_kernels.hip) — a helper module, plain Python, no tests of its own.  Built on msv1_range_clips.Idle and
the code helpers of msv1_keyframe_cut_clips; truth for them is tests/index_crop_ref.py, which test_index_crop_ref_cpu.py pins to the
oracle on every clip here.

One source picture: 192 x 192, 48 x 48 blocks.  The kernels give a lane 4 consecutive blocks OF THE RECTANGLE, a wave 256, a workgroup
1024; a skip word never crosses a multiple of 1023 in the rectangle's numbering.  RECTS:

  (0, 0, 48, 48)   2304 blocks  the whole grid: identity with the whole-picture calls
  (5, 3, 37, 31)   1147         odd width; blocks 1023 and 1024 lie in the middle of a row
  (8, 8, 32, 32)   1024         exactly one workgroup
  (8, 8, 33, 31)   1023         exactly one run
  (1, 1, 46, 45)   2070         three workgroups, the two-workgroup look-ahead, 2046
  (47, 0, 1, 48)   48           one column: every block is a row start
  (0, 47, 48, 1)   48           one row
  the four corners, 1 x 1       single blocks
  (3, 2, 3, 2)     6            fewer blocks than two lanes' share

`seams(bits, rect)`: a key frame, then one inter frame per pattern of msv1_delta_clips.PATTERNS, taken in the rectangle's numbering: the
frame writes src(j) for j in pattern(name, nb).  The blocks OUTSIDE the rectangle are written adversarially: in the frames of the
odd patterns (PATTERNS[1], [3], ..) every outside block is written, in the others none — an outside block is written next to an
unwritten row start, and the reverse.

`cuts(bits)` and `nones(bits)`, both under REFUSAL_RECT = (5, 3, 37, 31) with AT = rectangle blocks 0, 3, 4, 255, 256, 1023, 1024
and nb - 1, and OUTSIDE = the source blocks just in front of src(0) and just behind src(nb - 1):
  cuts    per position a group of four frames in msv1_keyframe_cut_clips.firsts_cut's manner — key | whole codes up to the block and
          its code one byte short | the blocks behind it whole | the block alone: a lone cut code at the block for the group's frames
          1 and 2.  Groups for the OUTSIDE blocks as well: the whole picture's key frame refuses there, the rectangle's does not.
  nones   three frames to decode one by one; then (index frame 0) a frame that codes every block but those of AT and OUTSIDE; then one
          frame per position of AT, ascending: the first block of the rectangle without a writer is each of AT in turn.  The OUTSIDE
          blocks are never written.

`tight(bits)`: msv1_tight_clips.directed of the rectangle's own size (its toggling and recode content on the lane, wave, workgroup
and 1023 seams in the rectangle's numbering), every code moved to src(j) of TIGHT_RECT = (5, 3, 37, 31); outside blocks get new
colours in odd frames and in the key frames."""
import index_keyframe_ref as kr
import msv1_delta_clips as dc
import msv1_keyframe_cut_clips as kc
import msv1_tight_clips as tc
from index_crop_ref import src
from msv1_range_clips import Idle

W = H = 192
NBX = NBY = 48
WHOLE = (0, 0, 48, 48)
CORNERS = ((0, 0, 1, 1), (47, 0, 1, 1), (0, 47, 1, 1), (47, 47, 1, 1))
RECTS = (WHOLE, (5, 3, 37, 31), (8, 8, 32, 32), (8, 8, 33, 31), (1, 1, 46, 45), (47, 0, 1, 48), (0, 47, 48, 1)) + CORNERS + ((3, 2, 3, 2),)
REFUSAL_RECT = TIGHT_RECT = (5, 3, 37, 31)

_cache = {}


def rect_id(rect):
    return "%d_%d_%dx%d" % rect


def blocks_of(rect):
    """src(j) for every j of the rectangle."""
    return [src(NBX, rect, j) for j in range(rect[2] * rect[3])]


def seams(bits, rect):
    """The clip of one rectangle, built once: kc.Clip with .patterns = {frame: name}, .rect, .inside (src(j) by j), .outside."""
    if ("seams", bits, rect) not in _cache:
        g = Idle(bits, W, H, seed=91 + 7 * rect[0] + 3 * rect[1] + rect[2] + rect[3])
        inside = blocks_of(rect)
        outside = sorted(set(range(g.nb)) - set(inside))
        nb = len(inside)
        frames, keys, names = [g.key()], [True], {}
        for k, name in enumerate(dc.PATTERNS):
            names[len(frames)] = name
            written = [inside[j] for j in dc.pattern(name, nb)] + (outside if k % 2 == 1 else [])
            frames.append(kc.whole(g, sorted(written), k))
            keys.append(False)
        c = kc.Clip("crop_seams_" + rect_id(rect), g, frames, keys, starts=(0,))
        c.patterns, c.rect, c.inside, c.outside = names, rect, inside, outside
        _cache[("seams", bits, rect)] = c
    return _cache[("seams", bits, rect)]


def pairs(n):
    """The pairs asked of a seams clip of n frames: every consecutive pair, the unions of two and three patterns, every frame from
    before the range, and a key pair at every frame."""
    from index_crop_ref import KEY
    out = [(a, b) for b in range(1, n) for a in (b - 1, b - 2, b - 3) if a >= 0]
    return out + [(-1, b) for b in range(n)] + [(KEY, t) for t in range(n)]


def positions(rect):
    nb = rect[2] * rect[3]
    return sorted({j for j in (0, 3, 4, 255, 256, 1023, 1024, nb - 1) if j < nb})


def outside_of(rect):
    """The source blocks just in front of src(0) and just behind src(nb - 1)."""
    inside = blocks_of(rect)
    return [b for b in (inside[0] - 1, inside[-1] + 1) if 0 <= b < NBX * NBY]


def cuts(bits, rect=REFUSAL_RECT):
    """kc.Clip with .groups = [(first frame, source block, j or None for an outside block)]."""
    if ("cuts", bits, rect) not in _cache:
        g = Idle(bits, W, H, seed=93)
        nb = g.nb
        inside = blocks_of(rect)
        frames, keys, groups = [], [], []
        for i, (p, j) in enumerate([(inside[j], j) for j in positions(rect)] + [(p, None) for p in outside_of(rect)]):
            groups.append((len(frames), p, j))
            before = b"".join(x for x in kc.mixed(g, range(p), i) if x is not None)
            frames += [g.key(), before + kc.one(g, p, kc.KINDS[i % 3])[:-1], kc.whole(g, range(p + 1, nb), i),
                       g.encode([None] * p + [kc.one(g, p, kc.KINDS[(i + 1) % 3])] + [None] * (nb - p - 1))]
            keys += [True, False, False, False]
        c = kc.Clip("crop_cuts", g, frames, keys, starts=(0,))
        c.groups, c.rect = groups, rect
        _cache[("cuts", bits, rect)] = c
    return _cache[("cuts", bits, rect)]


NONES_START = 3


def nones(bits, rect=REFUSAL_RECT):
    """kc.Clip for an index from frame NONES_START, with .at = the positions j (index frame 1 + k writes src(at[k]))."""
    if ("nones", bits, rect) not in _cache:
        g = Idle(bits, W, H, seed=94)
        nb = g.nb
        inside = blocks_of(rect)
        at = positions(rect)
        holes = {inside[j] for j in at} | set(outside_of(rect))
        frames = kc.warm_up(g) + [kc.whole(g, [b for b in range(nb) if b not in holes], 1)]
        for k, j in enumerate(at):
            p = inside[j]
            frames.append(g.encode([None] * p + [kc.one(g, p, kc.KINDS[k % 3])] + [None] * (nb - p - 1)))
        c = kc.Clip("crop_nones", g, frames, [True] + [False] * (len(frames) - 1), starts=(NONES_START,))
        c.at, c.rect = at, rect
        _cache[("nones", bits, rect)] = c
    return _cache[("nones", bits, rect)]


def tight(bits, rect=TIGHT_RECT):
    """msv1_tight_clips.directed of 4 bw x 4 bh pixels, moved into the rectangle: kc.Clip with .inner = that clip, .rect."""
    if ("tight", bits, rect) not in _cache:
        bx, by, bw, bh = rect
        inner = tc.directed(bits, 4 * bw, 4 * bh)
        g = Idle(bits, W, H, seed=95)
        inside = blocks_of(rect)
        outside = sorted(set(range(g.nb)) - set(inside))
        frames = []
        for f, data in enumerate(inner.frames):
            table = kr.codes_of(bits, bw, bh, data)
            codes = kc.mixed(g, outside if inner.keys[f] or f % 2 == 1 else [], f)
            for j, c in enumerate(table):
                assert c != "cut"
                if c is not None:
                    codes[inside[j]] = bytes(data)[c[0]:c[0] + c[1]]
            frames.append(g.encode(codes))
        c = kc.Clip("crop_tight", g, frames, list(inner.keys), starts=(0,))
        c.inner, c.rect, c.inside = inner, rect, inside
        _cache[("tight", bits, rect)] = c
    return _cache[("tight", bits, rect)]
