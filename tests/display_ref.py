"""References, launch plans and directed cases for the two per-pixel kernels behind the codec (jsplayer_amd/csrc/display_kernels.hip):
display_convert_kernel (jsp_display_convert) and frames_differ_kernel (jsp_frames_differ, launch_frames_differ).

A plain helper module (no tests of its own, numpy only):
  * convert_ref, differ_ref — the operations, from the header's description (include/jsplayer_amd.h), not from the kernels;
  * differ_plan / convert_plan — a restatement of how the kernels and their launchers CUT the work: which loop reads a pixel, as
    which component of which 16-byte vector, in which grid-stride iteration, by which lane; vector or scalar path, workgroups a row;
  * differ_model / convert_model — the answer a kernel cut that way gives, and the answer it gives with one named mistake
    (DIFFER_MISTAKES, CONVERT_MISTAKES) — so that a test can show that the directed cases tell the two apart;
  * DIFFER_CASES, CONVERT_CASES — the cases both tests/test_display_ref_cpu.py (census, mistakes) and
    tests/test_display_differ_gpu.py (the kernels themselves) go through.

The constants below are literals in display_kernels.hip (256 lanes, the 2048 cap; the 4 is the width of u32x4);
test_display_ref_cpu.py compares them with the kernel text, so a retune of the kernel fails there first.

Addresses.  Only an address's remainder mod 16 matters.  The cases give pointer offsets in ints from a 16-byte aligned allocation
(the GPU test asserts the alignment of its allocations), so a case's address is 4 * offset."""
from __future__ import annotations

from collections import namedtuple

import numpy as np

LANES = 256          # lanes of a workgroup (both kernels)
VEC = 4              # pixels of a 16-byte vector
GRID_CAP = 2048      # most workgroups a frames_differ launch takes
WAVE = 64            # lanes of a wave: lane & 63 == 0 issues the atomicOr after the ballot
MAX_DIM = 65535      # jsp_display_convert: width and height 1 .. 65535 (the grid-y limit HIP documents)

CANVAS, CANVAS_RGB15, SETPIXELS, SETPIXELS_RGB15 = 0, 1, 2, 3
MODES = (CANVAS, CANVAS_RGB15, SETPIXELS, SETPIXELS_RGB15)


# ---- the operations ---------------------------------------------------------------------------------------------------------------
def convert_word(c, mode):
    """The four formulas of JSP_DISPLAY_* on uint32 words (bits shifted out are lost)."""
    c = np.asarray(c).astype(np.uint32)
    if mode == CANVAS:
        return np.uint32(0xFF000000) | ((c & np.uint32(0xFF)) << np.uint32(16)) | (c & np.uint32(0xFF00)) | ((c >> np.uint32(16)) & np.uint32(0xFF))
    if mode == CANVAS_RGB15:
        return np.uint32(0xFF000000) | (c << np.uint32(3))
    if mode == SETPIXELS:
        return np.uint32(0xFF000000) | c
    if mode == SETPIXELS_RGB15:
        return c << np.uint32(11)
    raise ValueError(mode)


def convert_ref(src, w, h, mode, flip):
    """jsp_display_convert: every word converted by `mode`; with `flip`, output row y is source row h - 1 - y.  Flat uint32."""
    rows = np.asarray(src).view(np.uint32)[: w * h].reshape(h, w)
    if flip:
        rows = rows[::-1]
    return convert_word(rows, mode).reshape(w * h)


def differ_ref(a, b, first, n):
    """jsp_frames_differ: any a[i] != b[i] for first <= i < n."""
    return bool(np.any(np.asarray(a)[first:n] != np.asarray(b)[first:n]))


# ---- frames_differ: the cut ---------------------------------------------------------------------------------------------------------
def differ_grid(first, n, cap=GRID_CAP):
    """Workgroups both launchers ask for (0: nothing is launched)."""
    if first >= n:
        return 0
    grid = ((n - first) // VEC + LANES - 1) // LANES + 1
    return min(grid, cap) if cap else grid


Where = namedtuple("Where", "region component iteration lane last_vector")
# region: None (outside [first, n): no loop reads it), "scalar_only", "head", "body", "tail"; component: 0..3 in the body, else None;
# iteration: the grid-stride iteration of the loop that reads it; lane: the lane within its workgroup; last_vector: in the body's last vector


class DifferPlan:
    """How one launch cuts [first, n).  vec_ok: both pointers 16-byte aligned.  With vec_ok and lo4 < hi4 the range is a scalar head
    [first, lo4), a body [lo4, hi4) of whole vectors and a scalar tail [hi4, n); otherwise ONE scalar loop reads all of it
    (`scalar_only`; `short` says it is for want of a whole vector, not for the pointers)."""

    def __init__(self, addr_a, addr_b, first, n):
        self.addr_a, self.addr_b, self.first, self.n = addr_a, addr_b, first, n
        self.grid = differ_grid(first, n)
        self.threads = self.grid * LANES
        self.vec_ok = ((addr_a | addr_b) & 15) == 0
        self.lo4, self.hi4 = (first + 3) & ~3, n & ~3
        self.has_body = self.grid > 0 and self.vec_ok and self.lo4 < self.hi4
        self.scalar_only = self.grid > 0 and not self.has_body
        self.short = self.scalar_only and self.vec_ok
        self.head_len = self.lo4 - first if self.has_body else 0
        self.tail_len = n - self.hi4 if self.has_body else 0
        self.body_iterations = -(-((self.hi4 - self.lo4) // VEC) // self.threads) if self.has_body else 0
        self.scalar_iterations = -(-(n - first) // self.threads) if self.scalar_only else 0

    def where(self, i):
        if self.grid == 0 or not self.first <= i < self.n:
            return Where(None, None, None, None, False)
        if not self.has_body:
            k, r = divmod(i - self.first, self.threads)
            return Where("scalar_only", None, k, r % LANES, False)
        if i < self.lo4:
            return Where("head", None, 0, (i - self.first) % LANES, False)
        if i >= self.hi4:
            return Where("tail", None, 0, (i - self.hi4) % LANES, False)
        v, c = divmod(i - self.lo4, VEC)
        k, r = divmod(v, self.threads)
        return Where("body", c, k, r % LANES, i >= self.hi4 - VEC)


def differ_plan(addr_a, addr_b, first, n):
    return DifferPlan(addr_a, addr_b, first, n)


DIFFER_MISTAKES = (
    "no_head",                 # the head loop missing
    "no_tail",                 # the tail missing (behind a body)
    "drop_w",                  # the .w component left out of the compare
    "one_iteration",           # no grid-stride: every loop runs once
    "first_ignored",           # the range starts at pixel 0
    "first_plus_one",          # first off by one: the range starts at first + 1
    "first_minus_one",         # first off by one, the other way: the range starts at first - 1
    "lane0_only",              # `diff` instead of the ballot: only what a wave's lane 0 found counts
    "uncapped_stride",         # the stride from the grid before the cap, the launch with the cap
)


def _loop_reads(off, threads, stride, once):
    """A grid-stride loop of `threads` lanes stepping by `stride` over offsets 0 ..: the lane (within its workgroup) that reads
    offset `off`, or None."""
    k, r = divmod(off, stride)
    if r >= threads or (once and k > 0):
        return None
    return r % LANES


def differ_model(plan, diffs, mistake=None):
    """What a kernel that cuts the range as `plan` says answers when a and b differ exactly at the indices `diffs` (which may lie
    outside [first, n): the buffers are longer than the range) — with `mistake`, what that wrong kernel answers."""
    assert mistake is None or mistake in DIFFER_MISTAKES, mistake
    if plan.grid == 0:
        return False
    first, n, threads = plan.first, plan.n, plan.threads          # (the launcher's grid and the pointers stay as they are)
    if mistake == "first_ignored":
        first = 0
    elif mistake == "first_plus_one":
        first += 1
    elif mistake == "first_minus_one":
        first = max(first - 1, 0)
    stride = differ_grid(plan.first, plan.n, cap=None) * LANES if mistake == "uncapped_stride" else threads
    once = mistake == "one_iteration"
    lo4, hi4 = (first + 3) & ~3, n & ~3
    body = plan.vec_ok and lo4 < hi4
    for i in diffs:
        if not first <= i < n:
            continue
        if not body:
            lane = _loop_reads(i - first, threads, stride, once)
        elif i < lo4:
            lane = None if mistake == "no_head" else _loop_reads(i - first, threads, stride, once)
        elif i >= hi4:
            lane = None if mistake == "no_tail" else _loop_reads(i - hi4, threads, stride, once)
        else:
            v, c = divmod(i - lo4, VEC)
            lane = None if (mistake == "drop_w" and c == 3) else _loop_reads(v, threads, stride, once)
        if lane is not None and (mistake != "lane0_only" or lane % WAVE == 0):
            return True
    return False


# ---- frames_differ: the cases ---------------------------------------------------------------------------------------------------------
DifferCase = namedtuple("DifferCase", "part off_a off_b first n poke bit")
# a = A[off_a : off_a + n], b = B[off_b : off_b + n] of two 16-byte aligned allocations that hold the same pixels; `poke`: the one
# index (of the views) where b then differs, by XOR with 1 << bit — or None: no difference anywhere

EXHAUSTIVE_N = range(1, 20)
EXHAUSTIVE_OFFSETS = ((0, 0), (1, 1), (0, 1), (2, 0), (3, 3))
WRAP_N = GRID_CAP * LANES * VEC + 3 * LANES * VEC + 7       # 2 100 231: the capped grid's one pass is 2 097 152 pixels
WRAP_FIRSTS = (0, 5)
WRAP_OFFSETS = ((0, 0), (1, 1))                            # the vector path (2 iterations), the scalar path (5)


def _exhaustive_cases():
    out = []
    for (oa, ob) in EXHAUSTIVE_OFFSETS:
        for n in EXHAUSTIVE_N:
            for poke in [None] + list(range(n)):
                bit = 31 if (poke or 0) % 2 == 0 else 0
                for first in range(n + 1):
                    out.append(DifferCase("exhaustive", oa, ob, first, n, poke, bit))
    return out


def _wrap_cases():
    out = []
    n = WRAP_N
    for (oa, ob) in WRAP_OFFSETS:
        for first in WRAP_FIRSTS:
            lo4, hi4 = (first + 3) & ~3, n & ~3
            vec = (oa, ob) == (0, 0)
            unit, start = (VEC, lo4) if vec else (1, first)        # what a lane reads at a time, where the striding loop starts
            one_pass = differ_grid(first, n) * LANES * unit
            pokes = [None,
                     start + (1000 * LANES + 77) * unit + (2 if vec else 0),             # first iteration: workgroup 1000, lane 77 (component 2)
                     start + one_pass - 1,                                               # the last pixel of the first iteration
                     start + one_pass,                                                   # the first pixel of the second iteration
                     start + one_pass + (2 * LANES + 130) * unit + (3 if vec else 0),    # second iteration: workgroup 2, lane 130 (.w)
                     hi4 - 3, hi4 - 1]                                                   # the last vector (the scalar path's last iteration)
            pokes += list(range(hi4, n))                           # every tail pixel
            pokes += list(range(first, lo4))                       # every head pixel
            if first > 0:
                pokes.append(first - 1)                            # just outside: no difference
            for k, poke in enumerate(pokes):
                out.append(DifferCase("wrap", oa, ob, first, n, poke, 31 if k % 2 == 0 else 0))
    return out


DIFFER_CASES = _exhaustive_cases() + _wrap_cases()


def case_plan(c):
    return differ_plan(4 * c.off_a, 4 * c.off_b, c.first, c.n)


def case_diffs(c):
    return () if c.poke is None else (c.poke,)


def case_expect(c):
    """differ_ref of the case without building its buffers: the one difference lies in the range or it does not."""
    return c.poke is not None and c.first <= c.poke < c.n


# ---- display_convert: the cut, the model, the cases --------------------------------------------------------------------------------
ConvertPlan = namedtuple("ConvertPlan", "vec gx gx_vector scalar_by")
# vec: the 16-byte path; gx: workgroups a row; gx_vector: what the vector path would take for this width; scalar_by: what forces the
# scalar path, a subset of {"src", "dst", "width"}


def convert_plan(addr_src, addr_dst, w):
    by = set()
    if addr_src & 15:
        by.add("src")
    if addr_dst & 15:
        by.add("dst")
    if w & 3:
        by.add("width")
    vec = not by
    gx_vector = max((w // VEC + LANES - 1) // LANES, 1)
    gx = gx_vector if vec else max((w + LANES - 1) // LANES, 1)
    return ConvertPlan(vec, gx, gx_vector, frozenset(by))


CONVERT_MISTAKES = (
    "flip_off_by_one",         # flipped source row Y - y
    "vector_overrun",          # the vector loop running to X + 3
    "mode1_no_alpha",          # JSP_DISPLAY_CANVAS_RGB15 without the 0xFF000000
    "mode3_shift_10",          # JSP_DISPLAY_SETPIXELS_RGB15 shifted by 10
    "scalar_one_pass",         # the scalar path without its stride loop on a grid sized for vectors: the first 256 * gx_vector columns
)

GUARD = 16                     # sentinel ints on each side of `out`
SENTINEL = 0x5A5A5A5A
OUTSIDE = 0xC3C3C3C3           # what the model reads where a wrong kernel reads past the source


def convert_model(src, w, h, mode, flip, plan, mistake=None):
    """`out` with its GUARD sentinel ints on each side, as a kernel cut like `plan` leaves it (rows written in order: where a wrong
    kernel writes a pixel twice, the later row stands).  Without a mistake: sentinels, convert_ref, sentinels."""
    assert mistake is None or mistake in CONVERT_MISTAKES, mistake
    s = np.concatenate([np.asarray(src).view(np.uint32)[: w * h], np.full(w + VEC, OUTSIDE, np.uint32)])
    out = np.full(GUARD + w * h + GUARD, SENTINEL, np.uint32)

    def conv(c):
        if mistake == "mode1_no_alpha" and mode == CANVAS_RGB15:
            return c << np.uint32(3)
        if mistake == "mode3_shift_10" and mode == SETPIXELS_RGB15:
            return c << np.uint32(10)
        return convert_word(c, mode)

    cols = w
    if plan.vec and mistake == "vector_overrun":
        cols = w + VEC                                            # x = X passes x < X + 3: one vector past the row
    if not plan.vec and mistake == "scalar_one_pass":
        cols = min(w, LANES * plan.gx_vector)
    for y in range(h):
        ys = (h - y if mistake == "flip_off_by_one" else h - 1 - y) if flip else y
        out[GUARD + y * w: GUARD + y * w + cols] = conv(s[ys * w: ys * w + cols])
    return out


ConvertCase = namedtuple("ConvertCase", "w h mode flip off_src off_dst")
CONVERT_WIDTHS = (1, 2, 3, 4, 5, 7, 8, 255, 256, 257, 1023, 1024, 1025, 1028, 2052)
CONVERT_HEIGHTS = (1, 2, 3, 5)
CONVERT_OFFSETS = ((0, 0),) + tuple((k, 0) for k in (1, 2, 3)) + tuple((0, k) for k in (1, 2, 3)) + tuple((k, k) for k in (1, 2, 3))


def _convert_cases():
    out = []
    for w in CONVERT_WIDTHS:
        for h in CONVERT_HEIGHTS:
            for (os_, od) in (CONVERT_OFFSETS if w % 4 == 0 else ((0, 0),)):
                for mode in MODES:
                    for flip in (False, True):
                        out.append(ConvertCase(w, h, mode, flip, os_, od))
    return out


CONVERT_CASES = _convert_cases()


def convert_case_plan(c):
    return convert_plan(4 * c.off_src, 4 * c.off_dst, c.w)


def random_words(n, seed):
    """Pixels that cover all 32 bits."""
    return np.random.default_rng(seed).integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)


# ---- the fused key-frame compare at its first pixel: a directed MSVideo1 clip -------------------------------------------------------
COMPARE_W, COMPARE_H, COMPARE_ROW = 64, 40, 36             # 16-bit MSVideo1; the Manager's INSIGNIFICANT_LINES
COMPARE_LIT = (COMPARE_ROW * COMPARE_W - 1, COMPARE_ROW * COMPARE_W, COMPARE_W * COMPARE_H - 1)
# the last pixel the compare leaves out, the first one it reads, the last one of the frame


def compare_boundary_clip():
    """-> (frames, key flags, pictures by construction, lit): key frames alternating with an all-skip inter frame (so the Manager's
    byte shortcut for a key frame behind a key frame does not apply): base, then for each index of COMPARE_LIT a key frame that
    differs from base in that ONE buffer index, and base again behind each.  lit: {frame number: buffer index} of the lit key frames."""
    import msv1_directed_streams as ds
    w, h = COMPARE_W, COMPARE_H
    nbx, nb = w // 4, (w // 4) * (h // 4)
    c0, c1 = 0x1234, 0x2A5B                                 # two 15-bit colours (neither reads as a skip code)

    def key(index=None):
        items = [("solid", c0)] * nb
        if index is not None:
            y, x = divmod(index, w)
            bit = (y % 4) * 4 + x % 4
            # a set flag bit shows the FIRST colour of the pair, and bit 15 of the flags cannot be set: light bit 15 by clearing it
            item = ("two", 0x7FFF, c0, c1) if bit == 15 else ("two", 1 << bit, c1, c0)
            items[(y // 4) * nbx + x // 4] = item
        return ds.assemble(16, w, h, items)

    base = key()
    frames, keys, pictures, lit = [], [], [], {}
    order = [None]
    for index in COMPARE_LIT:
        order += [index, None]                              # base, lit, base, lit, base, lit, base
    for index in order:
        a = base if index is None else key(index)
        if frames:
            frames.append(ds.assemble(16, w, h, [("skip", 0)], prev=pictures[-1]).data)
            keys.append(False)
            pictures.append(pictures[-1])
        if index is not None:
            lit[len(frames)] = index
        frames.append(a.data)
        keys.append(True)
        pictures.append(a.picture)
    return frames, keys, pictures, lit
