"""tests/display_ref.py without a GPU: its references against the oracle, a census of what its directed cases put in front of
frames_differ_kernel and display_convert_kernel, every named mistake of the two models caught by those cases, its constants
against the kernel text — and the host-side refusals of codec.display_convert / frames_differ / display_present.

Census of DIFFER_CASES (14 345 exhaustive + 48 wrap cases; printed by running this file, asserted below as "at least one").
`inside`: the poke is the only difference and lies in the range; `outside`: the only difference lies at first - 1.

    feature                            inside                  outside
    scalar_only (pointers)               5341                      685
    short (lo4 >= hi4)                    218                       75
    head of 1 / 2 / 3            24 / 48 / 75             24 / 24 / 25
    body component 0 / 1 / 2 / 3  202 / 202 / 202 / 206   25 / 24 / 24 / 24
    body iteration >= 1                     8                        1
    tail of 1 / 2 / 3            28 / 56 / 90             24 / 24 / 25
    finding lane & 63 != 0               5239                        -
    last vector of the body               452                        -

CONVERT_CASES: 2208 (15 widths x 4 heights x 4 modes x 2 flips; the 6 widths divisible by 4 with 10 pairs of pointer offsets).

An outside case has no finding pixel, so it has no finding lane and no last vector; its features are those of its range (the
paths a kernel that starts one pixel early would take), and its body component is the slot the outside pixel holds in its
16-byte vector (a kernel that rounds `first` down to a vector reads it there)."""
import os
from collections import Counter

import numpy as np
import pytest

import display_ref as dr

SOURCE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "jsplayer_amd", "csrc", "display_kernels.hip")
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "jsplayer_amd.h")


# ---- the references ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", [(1, 1), (3, 5), (4, 1), (7, 3), (64, 48), (321, 7)])
def test_references_agree_with_the_oracle_on_random_words(w, h):
    from oracle_binding import orc_display_convert, orc_frames_differ
    src = dr.random_words(w * h, 100 + w)
    for mode in dr.MODES:
        for flip in (False, True):
            assert np.array_equal(dr.convert_ref(src, w, h, mode, flip), orc_display_convert(src.view(np.int32), w, h, mode, flip).view(np.uint32)), (mode, flip)
    n = w * h
    a = src.view(np.int32)
    rng = np.random.default_rng(w)
    for poke in [None] + sorted({0, n - 1, n // 2, int(rng.integers(0, n))}):
        b = a.copy()
        if poke is not None:
            b[poke] ^= np.int32(-2 ** 31) if poke % 2 == 0 else np.int32(1)
        for first in sorted({0, 1, n // 2, n - 1, n, poke or 0, (poke or 0) + 1}):
            if first <= n:
                assert dr.differ_ref(a, b, first, n) == orc_frames_differ(a, b, first, n), (poke, first)


def test_references_give_the_hand_worked_answers():
    """The values test_avi_player.test_oracle_display_and_differ_known_answers pins the oracle to."""
    px = np.array([0x00112233, 0x00FFEEDD, 0x12345678, 0x0000001F], dtype=np.uint32)
    u = lambda a: a.tolist()
    assert u(dr.convert_ref(px, 4, 1, 0, False)) == [0xFF332211, 0xFFDDEEFF, 0xFF785634, 0xFF1F0000]
    assert u(dr.convert_ref(px, 4, 1, 1, False)) == [0xFF891198, 0xFFFF76E8, 0xFFA2B3C0, 0xFF0000F8]
    assert u(dr.convert_ref(px, 4, 1, 2, False)) == [0xFF112233, 0xFFFFEEDD, 0xFF345678, 0xFF00001F]
    assert u(dr.convert_ref(px, 4, 1, 3, False)) == [0x89119800, 0xFF76E800, 0xA2B3C000, 0x0000F800]
    assert u(dr.convert_ref(px, 2, 2, 2, True)) == [0xFF345678, 0xFF00001F, 0xFF112233, 0xFFFFEEDD]
    other = px.copy()
    other[1] ^= 1
    assert not dr.differ_ref(px, px.copy(), 0, 4) and dr.differ_ref(px, other, 0, 4) and not dr.differ_ref(px, other, 2, 4)


# ---- frames_differ: census and mistakes ---------------------------------------------------------------------------------------------
def differ_census():
    """(inside, outside): Counters of features over DIFFER_CASES."""
    inside, outside = Counter(), Counter()
    for c in dr.DIFFER_CASES:
        if c.poke is None:
            continue
        p = dr.case_plan(c)
        if c.first <= c.poke < c.n:
            wh = p.where(c.poke)
            f = [wh.region if not p.short else "short"]
            if wh.region == "head":
                f.append(f"head_{p.head_len}")
            if wh.region == "tail":
                f.append(f"tail_{p.tail_len}")
            if wh.region == "body":
                f.append(f"body_c{wh.component}")
                if wh.iteration >= 1:
                    f.append("body_iter1+")
                if wh.last_vector:
                    f.append("last_vector")
            if wh.lane & (dr.WAVE - 1):
                f.append("lane_not_wave0")
            inside.update(f)
        elif c.poke == c.first - 1 and p.grid:
            f = ["short" if p.short else "scalar_only"] if p.scalar_only else []
            if p.has_body:
                f.append(f"body_c{c.poke % dr.VEC}")
                if p.head_len:
                    f.append(f"head_{p.head_len}")
                if p.tail_len:
                    f.append(f"tail_{p.tail_len}")
                if p.body_iterations > 1:
                    f.append("body_iter1+")
            outside.update(f)
    return inside, outside


BOTH = ["scalar_only", "short", "head_1", "head_2", "head_3", "body_c0", "body_c1", "body_c2", "body_c3", "body_iter1+", "tail_1", "tail_2", "tail_3"]
INSIDE_ONLY = ["lane_not_wave0", "last_vector"]


def test_differ_cases_hold_one_difference_or_none_and_count_as_planned():
    ex = [c for c in dr.DIFFER_CASES if c.part == "exhaustive"]
    assert len(ex) == len(dr.EXHAUSTIVE_OFFSETS) * sum((n + 1) ** 2 for n in dr.EXHAUSTIVE_N) == 14345
    per = Counter((c.off_a, c.off_b, c.n) for c in ex)
    assert all(per[(oa, ob, n)] == (n + 1) ** 2 for (oa, ob) in dr.EXHAUSTIVE_OFFSETS for n in dr.EXHAUSTIVE_N)
    assert {(c.first, c.poke) for c in ex if (c.off_a, c.off_b, c.n) == (0, 0, 19)} == {(f, p) for f in range(20) for p in [None] + list(range(19))}
    for c in dr.DIFFER_CASES:
        assert c.poke is None or 0 <= c.poke < c.n                      # (one XOR-ed bit is one differing pixel)
        assert 0 <= c.first <= c.n and c.bit in (0, 31)
    assert {c.bit for c in dr.DIFFER_CASES if c.poke is not None} == {0, 31}
    wrap = [c for c in dr.DIFFER_CASES if c.part == "wrap"]
    assert {c.n for c in wrap} == {2048 * 1024 + 3 * 1024 + 7} and {c.first for c in wrap} == {0, 5}
    assert {(c.off_a, c.off_b) for c in wrap} == {(0, 0), (1, 1)}


def test_the_wrap_size_is_where_the_capped_grid_wraps():
    n = dr.WRAP_N
    assert dr.differ_grid(0, n, cap=None) > dr.GRID_CAP == dr.differ_grid(0, n) == dr.differ_grid(5, n)
    for first in dr.WRAP_FIRSTS:
        assert dr.differ_plan(0, 0, first, n).body_iterations == 2 and dr.differ_plan(4, 4, first, n).scalar_iterations == 5
    # the sizes the existing test uses take one iteration: 1920x1080 has a grid of 2026 that covers 2 074 624 pixels
    p = dr.differ_plan(0, 0, 0, 1920 * 1080)
    assert (p.grid, p.threads * dr.VEC, p.body_iterations) == (2026, 2074624, 1)
    assert dr.differ_plan(0, 0, 0, 3840 * 2160).body_iterations == 4


def test_differ_census_reaches_every_region_from_inside_and_from_just_outside():
    inside, outside = differ_census()
    for f in BOTH + INSIDE_ONLY:
        assert inside[f] > 0, f"no case whose only difference lies in: {f}"
    for f in BOTH:
        assert outside[f] > 0, f"no case whose only difference lies just outside a range with: {f}"
    # the wrap cases name their places: check them against the plan
    for (oa, ob) in dr.WRAP_OFFSETS:
        for first in dr.WRAP_FIRSTS:
            cs = [c for c in dr.DIFFER_CASES if c.part == "wrap" and (c.off_a, c.off_b, c.first) == (oa, ob, first)]
            p = dr.case_plan(cs[0])
            wh = [p.where(c.poke) for c in cs[1:5]]
            assert [w.iteration for w in wh] == ([0, 0, 1, 1] if p.has_body else [0, 0, 1, 1])
            assert (wh[2].lane, wh[3].lane, wh[0].lane) == (0, 130, 77) and wh[1].lane == 255
            if p.has_body:
                assert (wh[0].component, wh[1].component, wh[2].component, wh[3].component) == (2, 3, 0, 3)
                assert p.where(cs[5].poke).last_vector and p.where(cs[6].poke).last_vector and p.tail_len == 3
                assert sum(p.where(c.poke).region == "tail" for c in cs[1:]) == 3
                assert sum(p.where(c.poke).region == "head" for c in cs[1:]) == p.head_len == (3 if first else 0)
            else:
                assert p.where(cs[6].poke).iteration == 4
            assert (cs[-1].poke == first - 1) == (first > 0)


def test_the_model_without_a_mistake_is_the_reference_on_every_case():
    for c in dr.DIFFER_CASES:
        assert dr.differ_model(dr.case_plan(c), dr.case_diffs(c)) == dr.case_expect(c), c
    # case_expect is differ_ref: on real buffers, for the small cases
    a = dr.random_words(32, 1)
    for c in dr.DIFFER_CASES[::37]:
        if c.part == "exhaustive":
            b = a.copy()
            if c.poke is not None:
                b[c.poke] ^= np.uint32(1 << c.bit)
            assert dr.differ_ref(a, b, c.first, c.n) == dr.case_expect(c)


@pytest.mark.parametrize("mistake", dr.DIFFER_MISTAKES)
def test_every_differ_mistake_gives_a_wrong_answer_on_some_case(mistake):
    wrong = [c for c in dr.DIFFER_CASES if dr.differ_model(dr.case_plan(c), dr.case_diffs(c), mistake) != dr.case_expect(c)]
    assert wrong, f"{mistake}: no case tells it from the kernel"
    if mistake in ("one_iteration", "uncapped_stride"):
        assert all(c.part == "wrap" for c in wrong)                     # (only a range the capped grid wraps on shows these)
    if mistake == "uncapped_stride":
        assert any((c.off_a, c.off_b) == (0, 0) for c in wrong) and any((c.off_a, c.off_b) == (1, 1) for c in wrong)


# ---- display_convert: census and mistakes --------------------------------------------------------------------------------------------
def test_convert_cases_cover_the_sizes_and_reach_every_path():
    assert {c.w for c in dr.CONVERT_CASES} == {1, 2, 3, 4, 5, 7, 8, 255, 256, 257, 1023, 1024, 1025, 1028, 2052}
    assert {c.h for c in dr.CONVERT_CASES} == {1, 2, 3, 5}
    by_size = Counter((c.w, c.h) for c in dr.CONVERT_CASES)
    assert all(by_size[(w, h)] == 8 * (10 if w % 4 == 0 else 1) for w in dr.CONVERT_WIDTHS for h in dr.CONVERT_HEIGHTS)
    for w in (4, 2052):
        assert {(c.off_src, c.off_dst) for c in dr.CONVERT_CASES if c.w == w} == {(0, 0), (1, 0), (2, 0), (3, 0), (0, 1), (0, 2), (0, 3), (1, 1), (2, 2), (3, 3)}
    seen = Counter()
    for c in dr.CONVERT_CASES:
        p = dr.convert_case_plan(c)
        seen["vector" if p.vec else "scalar", "one" if p.gx == 1 else "several"] += 1
        if not p.vec:
            seen["by", tuple(sorted(p.scalar_by))] += 1
        assert p.vec == (not p.scalar_by) and p.gx * dr.LANES * (dr.VEC if p.vec else 1) >= c.w     # one pass covers a row
    for key in [("vector", "one"), ("vector", "several"), ("scalar", "one"), ("scalar", "several"), ("by", ("src",)), ("by", ("dst",)), ("by", ("width",))]:
        assert seen[key] > 0, key
    # scalar with several workgroups a row at a width divisible by 4: the misaligned 1028 and 2052
    assert any(not dr.convert_case_plan(c).vec and dr.convert_case_plan(c).gx > 1 and c.w % 4 == 0 for c in dr.CONVERT_CASES)


def _convert_sources():
    return {(w, h): dr.random_words(w * h, 7 * w + h) for w in dr.CONVERT_WIDTHS for h in dr.CONVERT_HEIGHTS}


def test_the_convert_model_without_a_mistake_is_the_reference_between_intact_sentinels():
    srcs = _convert_sources()
    for c in dr.CONVERT_CASES:
        got = dr.convert_model(srcs[c.w, c.h], c.w, c.h, c.mode, c.flip, dr.convert_case_plan(c))
        assert np.all(got[:dr.GUARD] == dr.SENTINEL) and np.all(got[-dr.GUARD:] == dr.SENTINEL)
        assert np.array_equal(got[dr.GUARD:-dr.GUARD], dr.convert_ref(srcs[c.w, c.h], c.w, c.h, c.mode, c.flip)), c


@pytest.mark.parametrize("mistake", dr.CONVERT_MISTAKES)
def test_every_convert_mistake_leaves_a_wrong_buffer_on_some_case(mistake):
    srcs = _convert_sources()
    wrong = []
    for c in dr.CONVERT_CASES:
        p = dr.convert_case_plan(c)
        if not np.array_equal(dr.convert_model(srcs[c.w, c.h], c.w, c.h, c.mode, c.flip, p, mistake),
                              dr.convert_model(srcs[c.w, c.h], c.w, c.h, c.mode, c.flip, p)):
            wrong.append(c)
    assert wrong, f"{mistake}: no case tells it from the kernel"
    if mistake == "vector_overrun":
        # with one row only the sentinels behind `out` show it
        c = next(c for c in wrong if c.h == 1)
        got = dr.convert_model(srcs[c.w, 1], c.w, 1, c.mode, c.flip, dr.convert_case_plan(c), mistake)
        assert np.array_equal(got[dr.GUARD:dr.GUARD + c.w], dr.convert_ref(srcs[c.w, 1], c.w, 1, c.mode, c.flip)) and np.any(got[-dr.GUARD:] != dr.SENTINEL)
    if mistake == "scalar_one_pass":
        assert {c.w for c in wrong} >= {1025, 1028, 2052}


# ---- the constants, against the kernel text ------------------------------------------------------------------------------------------
def test_constants_are_those_of_the_kernel_text():
    with open(SOURCE) as f:
        text = f.read()
    L, V, G, W = dr.LANES, dr.VEC, dr.GRID_CAP, dr.WAVE
    # both launchers of frames_differ_kernel size the grid alike
    assert text.count(f"std::min<size_t>((count / {V} + {L - 1}) / {L} + 1, {G})") == 2
    for expr in (f"const size_t stride = (size_t)gridDim.x * {L};",
                 f"lo4 + ((size_t)blockIdx.x * {L} + threadIdx.x) * {V}; i < hi4; i += stride * {V}",
                 f"first + (size_t)blockIdx.x * {L} + threadIdx.x; i < lo4; i += stride",
                 f"lo + (size_t)blockIdx.x * {L} + threadIdx.x; i < hi; i += stride",
                 f"(first + {V - 1}) & ~size_t({V - 1}), hi4 = n & ~size_t({V - 1})",
                 f"(threadIdx.x & {W - 1}) == 0",
                 f"(blockIdx.x * {L} + threadIdx.x) * {V}; x < X; x += gridDim.x * {L} * {V}",
                 f"blockIdx.x * {L} + threadIdx.x; x < X; x += gridDim.x * {L})",
                 f"(width / (vec ? {V} : 1) + {L - 1}) / {L}",
                 "flip ? Y - 1 - y : y",
                 f"width > {dr.MAX_DIM} || height > {dr.MAX_DIM}"):
        assert text.count(expr) == 1, expr
    with open(HEADER) as f:
        assert f"width and height 1 .. {dr.MAX_DIM}" in f.read()


# ---- the clip for the fused key-frame compare -------------------------------------------------------------------------------------
def test_compare_boundary_clip_is_what_it_says_through_the_oracle():
    """The clip tests/test_display_differ_gpu.py plays: each lit key frame differs from the pictures around it in exactly its one
    buffer index, the oracle decodes the pictures built here, and the Manager over the oracle logs False, True, True."""
    from jsplayer_amd import avi, player
    from test_avi_player import ORACLE_CLASSES
    w, h = dr.COMPARE_W, dr.COMPARE_H
    frames, keys, pictures, lit = dr.compare_boundary_clip()
    assert list(lit.values()) == [36 * w - 1, 36 * w, w * h - 1] and player.INSIGNIFICANT_LINES == dr.COMPARE_ROW
    for f, index in lit.items():
        assert keys[f] and not keys[f - 1] and keys[f - 2] and not keys[f + 1] and keys[f + 2]
        assert np.flatnonzero(pictures[f] != pictures[f - 1]).tolist() == [index] == np.flatnonzero(pictures[f + 2] != pictures[f + 1]).tolist()
    blob = avi.write_avi(w, h, frames, fourcc=b"CRAM", bpp=16, key_flags=keys)
    vi, got = avi.read_avi(blob)
    cpu = player.Manager(vi, player.make_decoder(vi, ORACLE_CLASSES), lambda n: np.zeros(n, dtype=np.int32))
    shown = []
    cpu.play(got, key_flags=keys, on_frame=lambda d, buf: shown.append(buf.view(np.uint32).copy()))
    assert len(shown) == len(pictures) and all(np.array_equal(s, p) for s, p in zip(shown, pictures))
    sig = {d.index: d.significant_changes for d in cpu.log}
    assert [sig[f] for f in lit] == [False, True, True] == [sig[f + 2] for f in lit]


# ---- the Python entry points take device tensors only ---------------------------------------------------------------------------------
def test_display_entry_points_refuse_host_memory_before_the_library_is_touched(monkeypatch):
    import torch
    from jsplayer_amd import _native as N
    from jsplayer_amd import codec as cm
    touched = []

    class Touched(Exception):
        pass

    def no_lib():
        touched.append(1)
        raise Touched("the native library was asked for")

    monkeypatch.setattr(N, "lib", no_lib)
    host_np = np.zeros(64, np.int32)
    host_t = torch.zeros(64, dtype=torch.int32)

    class Device:                       # stands for a device tensor (no GPU here): it must get past the refusal, to N.lib()
        is_cuda, dtype = True, torch.int32
        def data_ptr(self): return 0x1000
        def is_contiguous(self): return True
        def numel(self): return 64

    dev = Device()
    for host in (host_np, host_t, [0] * 64, None):
        for (a, b) in ((host, dev), (dev, host), (host, host)):
            with pytest.raises(cm.CodecError, match="^display_convert:"):
                cm.display_convert(a, b, 8, 8)
            with pytest.raises(cm.CodecError, match="^frames_differ:"):
                cm.frames_differ(a, b, 0, 64)
            with pytest.raises(cm.CodecError, match="^display_present:"):
                cm.display_present(a, 8, 8, b, 8, 8, 1.0, 0.0, 0.0)
    for (first, n) in ((-1, 64), (0, -1), (-5, -5)):
        with pytest.raises(cm.CodecError, match="^frames_differ:"):
            cm.frames_differ(dev, dev, first, n)
    assert not touched
    with pytest.raises(Touched):                                                      # the stand-in does reach the library
        cm.frames_differ(dev, dev, 0, 64)
    assert touched == [1]


if __name__ == "__main__":
    ins, outs = differ_census()
    print(f"{len(dr.DIFFER_CASES)} differ cases, {len(dr.CONVERT_CASES)} convert cases")
    for f in BOTH + INSIDE_ONLY:
        print(f"  {f:16s} inside {ins[f]:6d}   outside {outs[f]:6d}")
