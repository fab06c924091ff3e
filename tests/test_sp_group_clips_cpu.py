"""The directed clips of tests/sp_group_clips.py for the two inter-frame group kernels, without a GPU: the clips are exact on the
CPU, they put in front of both kernel forms what they were painted for (a census, asserted, taken from the host stage's own block
records through sp_group_plan.plan), and a walk that makes one of the kernels' possible mistakes (sp_group_plan.FAULTS) leaves a
wrong picture on them.  sp_group_plan's constants are compared with sp_kernels.hip: a retune of the kernel fails here first.

Observed with `PYTHONPATH=.:tests python tests/test_sp_group_clips_cpu.py` (numpy only, nothing measured on a GPU).  The three
random clips are those of test_inter_groups_at_odd_sizes_and_in_a_three_buffer_rotation: none of them ever cuts a chunk on the
rounding or takes a chunk of one frame in the loader form, two of them never cut a chunk on literals at all, and all three let
unrounded_test through; 100x52 and 1928x24 let skip_after_cut through as well.

Census, over every group of a clip (printed by running this file, not asserted):

    clip     form      wgs  cut by   of them   of them   chunks of   most
                            literals exact     rounding  one frame   chunks
    L        loader      9        6        1         1         4     12
    L        self       15        7        5         0         4      8
    S        self       15        7        5         0         4      8
    H        loader      9        6        1         1         4     12
    H        self       15        7        5         0         4      8
    100x52   loader      4        0        0         0         0      4
    100x52   self        8        0        0         0         1      3
    640x360  loader    115       26        1         0         0      6
    640x360  self      230      150       18         0         8      5
    1928x24  loader     32        0        0         0         0      5
    1928x24  self       62        1        0         0         2      4

Frames a faulty walk gets wrong (0 = the clip lets the mistake through); the random clips reach the loader form in their
test, the self-staging column is what they would do if they reached it:

    fault            L loader / self   S self   H loader / self   100x52 loader / self   640x360 loader / self   1928x24 loader / self
    skip_after_cut   93 / 93           93       93 / 93           0 / 0                  61 / 61                0 / 37
    dst_by_group     111 / 153         153      111 / 153         35 / 48                61 / 71                56 / 71
    dst_by_chunk     132 / 163         163      132 / 163         51 / 51                72 / 72                72 / 72
    unrounded_test   87 / -            -        87 / -            0 / -                  0 / -                  0 / -
    stride_16        164 / 164         164      164 / 164         51 / 51                72 / 72                72 / 72
    no_minus_x1      164 / 164         164      164 / 164         51 / 51                72 / 72                72 / 72
    row8_reads_row   164 / -           -        164 / -           50 / -                 72 / -                 72 / -
    stale_tail       0 / 0             0        0 / 0             0 / 0                  0 / 0                  0 / 0
    one_frame_more   99 / 61           61       99 / 61           35 / 13                56 / 39                56 / 36
    stagger_always   - / 0             0        - / 0             - / 0                  - / 0                  - / 0
    swapped_buffer   71 / -            -        71 / -            47 / -                 62 / -                 55 / -

(stale_tail and stagger_always move cuts and change no picture, on any clip: sp_group_plan.PLAN_ONLY, asserted on the plan below.
In the self-staging form a whole workgroup repaint is 1024 words, half its buffer, so two repaints fill a chunk exactly and a
chunk of one frame comes from the stagger or the end of a group, never from the literals.)
"""
import os
import re

import numpy as np
import pytest

import hoststage_binding as hb
import sp_group_clips as gc
import sp_group_plan as gp

NAMES = ("L", "S", "H")
CASES = [(name, form) for name in NAMES for form in gc.FORMS_OF[name]]
SOURCE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "jsplayer_amd", "csrc", "sp_kernels.hip")


def pictures_of(c, group, form, fault=None):
    """{frame of the clip: picture} as the walk leaves them, a buffer per frame."""
    prev = c.frames[group["before"]].reshape(c.h, c.w)
    return gp.walk(form, group["records"], group["payloads"], prev, group["ts"], fault)


def wrong_frames(c, groups, form, fault):
    bad = 0
    for g in groups:
        out = pictures_of(c, g, form, fault)
        bad += sum(1 for t in g["ts"] if not np.array_equal(out[t].reshape(-1), c.frames[t]))
    return bad


# ------------------------------------------------------------------------------------------------------------------ exactness

@pytest.mark.parametrize("name", NAMES)
def test_every_pixel_names_its_last_writer(name):
    w, h, bpp, _ = gc.SPECS[name]
    c = gc.clip(name)
    nbx, _ = gc.geometry(w, h)
    last = np.zeros((h, w), dtype=np.int64)
    decode = np.vectorize(lambda v: gc.writer_of(v, bpp))
    for t in range(gc.N):
        if t in gc.KEYS:
            last[:] = t
        for b, (x1, y1, x2, y2) in ({} if t in gc.KEYS else gc.regions(t, w, h)).items():
            by, bx = divmod(b, nbx)
            last[by * 16 + y1:by * 16 + y2, bx * 16 + x1:bx * 16 + x2] = t
        assert np.array_equal(decode(c.frames[t]).reshape(h, w), last), f"frame {t}"
    assert w * h < 65535


@pytest.mark.parametrize("name", NAMES)
def test_encoder_oracle_and_host_stage_equal_the_painting(name):
    c = gc.clip(name)
    pictures, _ = gc.oracle(name)
    descs = gc.records(name)
    assert len(c.chunks) == gc.N
    before = None
    for t in range(gc.N):
        want = c.frames[t]
        d = descs[t]
        assert d["status"] == 0, (t, d["error"])
        if c.keys[t]:
            assert d["kind"] == hb.KIND_INTRA
            staged = hb.expand_iframe(d, c.w, c.h)
        elif t in gc.UNCHANGED:
            assert d["kind"] == hb.KIND_NONE and not d["adopted"]
            staged = before
        else:
            assert d["kind"] == hb.KIND_INTER and d["literalised"] and d["adopted"], t
            assert not any(b[0] & hb.PB_MOTION for b in d["blocks"]), f"frame {t}: a block coded as motion"
            staged = hb.expand_pframe(d, before, c.w, c.h)
        for what, got in (("the encoder's picture", c.encoder_frames[t]), ("the oracle's picture", pictures[t]),
                          ("expand_pframe over the host stage's records", staged)):
            assert np.array_equal(got, want), f"{c.name} frame {t}, {what}: " + gc.describe_mismatch(got, want, c.w, c.h, c.bpp)
        before = want
    assert [t for t in range(gc.N) if descs[t]["kind"] == hb.KIND_NONE] == list(gc.UNCHANGED)


@pytest.mark.parametrize("name,form", CASES)
def test_the_walk_equals_the_painting(name, form):
    c = gc.clip(name)
    for g in gc.groups(gc.records(name)):
        out = pictures_of(c, g, form)
        for t in g["ts"]:
            assert np.array_equal(out[t].reshape(-1), c.frames[t]), f"{c.name} {form} frame {t}: " + \
                gc.describe_mismatch(out[t], c.frames[t], c.w, c.h, c.bpp)
    # three buffers in rotation: each ends with the last frame stored to it
    g = gc.groups(gc.records(name))[0]
    out = gp.walk(form, g["records"], g["payloads"], c.frames[g["before"]].reshape(c.h, c.w), [i % 3 for i in range(len(g["ts"]))])
    for b in range(3):
        t = [t for i, t in enumerate(g["ts"]) if i % 3 == b][-1]
        assert np.array_equal(out[b].reshape(-1), c.frames[t])


# --------------------------------------------------------------------------------------------------------------------- census

def run_of(flags):
    """The longest run of true values."""
    best = cur = 0
    for f in flags:
        cur = cur + 1 if f else 0
        best = max(best, cur)
    return best


def census(form, c, descs=None):
    """What the clip puts in front of one kernel form, from the host stage's records: a dict of the facts the tests assert."""
    F = gp.FORM[form]
    descs = gc.staged(c) if descs is None else descs
    groups = gc.groups(descs)
    nbx, nby = gc.geometry(c.w, c.h)
    pw, ph = c.w - 16 * (nbx - 1), c.h - 16 * (nby - 1)
    out = dict(group_lengths=[len(g["ts"]) for g in groups], unchanged=[t for t, d in enumerate(descs) if d["kind"] == hb.KIND_NONE])
    long = max(groups, key=lambda g: len(g["ts"]))
    plans = gp.plan(form, long["records"], nbx, nby)
    out["plans"] = plans
    out["most_chunks"] = max(len(p) for p in plans.values())
    out["single_frame_chunks_in_a_row"] = max(run_of(k.nf == 1 and k.why == gp.LITERALS for k in p) for p in plans.values())
    out["exact_fills"] = [(wg, k.f0, k.nf) for wg, p in plans.items() for k in p if k.words == F.words and k.why == gp.LITERALS]
    out["rounding_cuts"] = [(wg, k.f0) for wg, p in plans.items() for k in p
                            if k.why == gp.LITERALS and k.next_unrounded <= F.words < k.next_words]
    out["literal_cuts"] = sum(1 for p in plans.values() for k in p if k.why == gp.LITERALS)
    out["cap_chunks"] = sum(1 for g in groups for p in gp.plan(form, g["records"], nbx, nby).values() for k in p if k.nf == F.cap)
    out["staggered"] = [(wg, p[0].nf) for wg, p in plans.items()
                        if p[0].why == gp.STAGGER and p[0].nf < F.cap and p[0].next_words <= F.words and p[0].words > 0]
    # per workgroup and frame of the long group: the literal words, unrounded
    need = {wg: gp._need(form, long["records"], nbx, nby, wg[0], wg[1], False) for wg in plans}
    out["full_frames_in_a_row"] = max(run_of(n.sum(axis=1) == F.blocks * 256) for n in need.values())
    written = {wg: sum(int(gp._need(form, g["records"], nbx, nby, wg[0], wg[1], False).sum()) for g in groups) for wg in plans}
    out["never_written"] = [wg for wg, n in written.items() if n == 0]
    # a busy workgroup beside a sparse one of the same block row: their chunks start at different frames
    cuts = {wg: [k.f0 for k in p] for wg, p in plans.items()}
    out["neighbours_differ"] = [(a, b) for a in plans for b in plans if a[1] == b[1] and a[0] < b[0] and cuts[a] != cuts[b]
                                and any(k.why == gp.LITERALS for k in plans[a]) and not any(k.why == gp.LITERALS for k in plans[b])
                                and written[b] > 0]
    last_wx = (nbx - 1) // F.blocks
    out["short_workgroup_blocks"] = nbx - last_wx * F.blocks
    out["short_workgroup_written"] = [by for by in range(nby) if written[(last_wx, by)] > 0]
    shapes = set()
    writers = {}
    for i, table in enumerate(long["records"]):
        for b in np.nonzero(table[:, 0])[0]:
            x1, y1, x2, y2 = (int(v) for v in table[b, 1:5])
            by, bx = divmod(int(b), nbx)
            writers.setdefault(int(b), []).append(i)
            if x1 % 4:
                shapes.add("x1 % 4 != 0")
            if x2 - x1 in (1, 2, 3, 5, 15):
                shapes.add("width %d" % (x2 - x1))
            if (y1, y2) == (7, 9):
                shapes.add("rows 7..8")
            if y2 <= 8 and y2 - y1 == 1:
                shapes.add("one row below 8")
            if y1 >= 8:
                shapes.add("rows from 8 on only")
            if bx == nbx - 1 and x2 == pw:
                shapes.add("reaches the right edge of a block %d wide" % pw)
            if by == nby - 1 and y2 == ph:
                shapes.add("reaches the picture's last row")
            if by == nby - 1 and bx == nbx - 1 and y2 == ph and x2 == pw:
                shapes.add("the picture's bottom right corner")
    out["shapes"] = shapes
    out["sixteen_then_alone"] = [b for b, fs in writers.items() if len(fs) == 16 and fs[-1] - fs[0] == 15 and fs[-1] < len(long["records"]) - 1]
    # the unchanged frames: p = how many frames of the long group come before it
    inside, after_cut = [], []
    for t in out["unchanged"]:
        if not long["ts"][0] < t < long["ts"][-1]:
            continue
        p = sum(1 for u in long["ts"] if u < t)
        for wg, pl in plans.items():
            for k in pl:
                if k.words and k.f0 < p < k.f0 + k.nf:
                    inside.append(t)
                if k.why == gp.LITERALS and k.f0 + k.nf == p:
                    after_cut.append(t)
    out["unchanged_inside_a_chunk"], out["unchanged_after_a_literal_cut"] = sorted(set(inside)), sorted(set(after_cut))
    return out


_census = {}


def census_of(name, form):
    if (name, form) not in _census:
        _census[(name, form)] = census(form, gc.clip(name), gc.records(name))
    return _census[(name, form)]


def check_census(cs, form, pw):
    """Every role of the issue's list a - i; raises AssertionError naming the first that is missing."""
    F = gp.FORM[form]
    assert cs["group_lengths"] == list(gc.GROUP_LENGTHS), cs["group_lengths"]
    assert cs["full_frames_in_a_row"] >= 3, "a: no three frames in a row that repaint a whole workgroup"
    if form == "loader":
        assert cs["single_frame_chunks_in_a_row"] >= 3, "a: no three chunks of one frame in a row"
        assert any(nf == 2 for _, _, nf in cs["exact_fills"]), "b: no chunk of 2048 + 1024 words"
        assert cs["rounding_cuts"], "c: no cut that only the rounding decides"
    else:
        # (1024 words are half the buffer: two repaints fill a chunk exactly, chunks of one frame come from the stagger)
        assert sum(1 for _, _, nf in cs["exact_fills"] if nf == 2) >= 2, "b: no chunks of 1024 + 1024 words"
        assert not cs["rounding_cuts"]
        assert any(nf == 1 for _, nf in cs["staggered"]), "no first chunk cut to one frame by the stagger"
        assert len(cs["staggered"]) >= 3, "the stagger cuts no first chunk that the literal buffer would have let grow"
    assert cs["exact_fills"], "b: no chunk fills the literal buffer exactly"
    assert cs["most_chunks"] >= 5, "no workgroup refills both chunk buffers twice"
    assert cs["cap_chunks"] >= 3, "no chunk reaches the frame cap"
    assert cs["neighbours_differ"], "d: no sparse workgroup beside a busy one"
    assert cs["never_written"], "e: every workgroup is written"
    assert cs["short_workgroup_blocks"] == 1 and len(cs["short_workgroup_written"]) == 3, "f: the workgroup with one block"
    want = {"x1 % 4 != 0", "width 1", "width 2", "width 3", "width 5", "width 15", "rows 7..8", "one row below 8", "rows from 8 on only",
            "reaches the right edge of a block %d wide" % pw, "reaches the picture's last row", "the picture's bottom right corner"}
    assert want <= cs["shapes"], "g: missing %s" % sorted(want - cs["shapes"])
    assert cs["unchanged"] == list(gc.UNCHANGED), "h"
    assert cs["unchanged_inside_a_chunk"] and cs["unchanged_after_a_literal_cut"], "h: " + repr((cs["unchanged_inside_a_chunk"], cs["unchanged_after_a_literal_cut"]))
    assert cs["sixteen_then_alone"], "i: no block written in 16 frames in a row and then left alone"
    assert F.blocks * 256 <= F.words


@pytest.mark.parametrize("name,form", CASES)
def test_census(name, form):
    c = gc.clip(name)
    cs = census_of(name, form)
    check_census(cs, form, c.w - 16 * (gc.geometry(c.w, c.h)[0] - 1))
    if form == "loader":
        # the chunks of workgroup (0, 0), as painted: frames 1..4 | 5 | 6 | 7 | 8, 9 = 3072 words | 10, with 12 left out by 4 words
        first = [(k.f0, k.nf, k.words, k.why) for k in cs["plans"][(0, 0)][:6]]
        assert first == [(0, 4, 2312, gp.LITERALS), (4, 1, 2048, gp.LITERALS), (5, 1, 2048, gp.LITERALS), (6, 1, 2048, gp.LITERALS),
                         (7, 2, 3072, gp.LITERALS), (9, 1, 2048, gp.LITERALS)], first
        k = cs["plans"][(0, 0)][5]
        assert (k.next_unrounded, k.next_words) == (2048 + 1021, 2048 + 1028)
        assert 11 in cs["unchanged_after_a_literal_cut"]
    else:
        first = [(k.f0, k.nf, k.words, k.why) for k in cs["plans"][(0, 0)][:5]]
        assert first == [(0, 1, 8, gp.STAGGER), (1, 3, 1045, gp.LITERALS), (4, 2, 2048, gp.LITERALS), (6, 2, 2048, gp.LITERALS),
                         (8, 2, 2048, gp.LITERALS)], first


@pytest.mark.parametrize("roles,says", [(("full",), "a:"), (("fill",), "b:"), (("rounding",), "c:"), (("sparse", "sixteen", "edge"), "d:"),
                                        (("edge",), "f:"), (("halves", "shapes"), "g:"), (("sixteen",), "i:")])
def test_the_census_notices_a_missing_role(roles, says):
    """(d: blocks 8..16 of block row 0 hold three roles; g: rows 7..8 are painted by two.)"""
    c = gc.build("L", skip=roles)
    with pytest.raises(AssertionError, match=says):
        check_census(census("loader", c), "loader", 12)


def test_the_census_notices_a_missing_role_in_the_self_staging_form():
    for role, says in (("full", "a:"), ("sixteen", "i:")):
        with pytest.raises(AssertionError, match=says):
            check_census(census("self", gc.build("S", skip=(role,))), "self", 11)


# ---------------------------------------------------------------------------------------------------------------- wrong walks

@pytest.mark.parametrize("fault", [f for f in gp.FAULTS if f not in gp.PLAN_ONLY])
@pytest.mark.parametrize("name,form", CASES)
def test_a_wrong_walk_fails_on_the_directed_clips(name, form, fault):
    if form not in gp.FAULTS[fault]:
        return                                          # (the mistake is one the other kernel could make)
    c = gc.clip(name)
    assert wrong_frames(c, gc.groups(gc.records(name)), form, fault) > 0, f"fault {fault} passes clip {name} in the {form} form"


@pytest.mark.parametrize("fault", gp.PLAN_ONLY)
@pytest.mark.parametrize("name,form", CASES)
def test_a_mistake_that_moves_cuts_only_shows_in_the_plan(name, form, fault):
    """stale_tail and stagger_always cannot change a picture (sp_group_plan's docstring says why): the walk stays exact and the
    plan of the long group differs — more chunks, or more words in the workgroup with one block."""
    if form not in gp.FAULTS[fault]:
        return
    c = gc.clip(name)
    groups = gc.groups(gc.records(name))
    assert wrong_frames(c, groups, form, fault) == 0
    nbx, nby = gc.geometry(c.w, c.h)
    good, bad = gp.plan(form, groups[0]["records"], nbx, nby), gp.plan(form, groups[0]["records"], nbx, nby, fault)
    brief = lambda p: {wg: [(k.f0, k.nf, k.words) for k in ks] for wg, ks in p.items()}   # noqa: E731
    assert brief(good) != brief(bad)
    if fault == "stale_tail":
        short = ((nbx - 1) // gp.FORM[form].blocks, 0)
        assert sum(k.words for k in bad[short]) > sum(k.words for k in good[short])
    else:
        assert sum(len(p) for p in bad.values()) > sum(len(p) for p in good.values())


# ------------------------------------------------------------------------------------------------------------------ constants

def test_the_plans_constants_are_the_kernels():
    src = open(SOURCE).read()

    def one(pattern):
        found = re.findall(pattern, src)
        assert len(found) == 1, (pattern, found)
        return found[0]

    assert int(one(r"constexpr int G2_BLOCKS = (\d+);")) == gp.G2_BLOCKS
    assert int(one(r"constexpr int G2_CF = (\d+);")) == gp.G2_CF
    assert int(one(r"constexpr int G2_LW = (\d+);")) == gp.G2_LW
    got = one(r"constexpr int chunk = (\d+), lit_words = (\d+), stagger = (\d+);")
    assert tuple(int(v) for v in got) == (gp.chunk, gp.lit_words, gp.stagger)
    # the self-staging form's four blocks to a workgroup, its stagger, and the rounding of the loader form
    assert int(one(r"constexpr int PWG = (\d+);")) == gp.SELF_BLOCKS * 64
    assert one(r"dim3 grid\(\(g\.nbx \+ 3\) / (\d+), g\.nby\);\n    // A chunk of") == str(gp.SELF_BLOCKS)
    one(r"const int first = 1 \+ \(int\)\(\(blockIdx\.x \* 5u \+ blockIdx\.y \* 3u\) % \(unsigned\)chunk_frames\);")
    one(r"need\[h\] = \(\(uint32_t\)\(pb\.x2 - pb\.x1\) \* \(uint32_t\)\(pb\.y2 - pb\.y1\) \+ 3u\) & ~3u;")
    assert gp.FORM["loader"] == (gp.G2_BLOCKS, gp.G2_CF, gp.G2_LW, True, 0)
    assert gp.FORM["self"] == (gp.SELF_BLOCKS, gp.chunk, gp.lit_words, False, gp.stagger)


# ------------------------------------------------------------------------------------------------- observed, printed, not asserted

RANDOM_CLIPS = [(100, 52), (640, 360), (1928, 24)]       # test_inter_groups_at_odd_sizes_and_in_a_three_buffer_rotation


def random_clip(w, h):
    import sp_index_ref as ref
    from jsplayer_amd import streamgen as sg
    chunks, keys, frames = sg.sp_clip(985, w, h, 76, version=4, unchanged_at=(7, 20, 21),
                                      p_mix_at={9: dict(unchanged=0.5, motion=0.2), 30: dict(unchanged=0.97, motion=0.01)})
    return ref.Clip(f"{w}x{h}", w, h, 24, 4, 36, chunks, keys, [f.astype(np.uint32) for f in frames])


def census_row(label, form, c, descs):
    F = gp.FORM[form]
    nbx, nby = gc.geometry(c.w, c.h)
    row = dict(wg=0, lit=0, exact=0, rounding=0, single=0, most=0)
    for g in gc.groups(descs):
        plans = gp.plan(form, g["records"], nbx, nby)
        row["wg"] = len(plans)
        for p in plans.values():
            row["most"] = max(row["most"], len(p))
            for k in p:
                row["lit"] += k.why == gp.LITERALS
                row["exact"] += k.why == gp.LITERALS and k.words == F.words
                row["rounding"] += k.why == gp.LITERALS and k.next_unrounded <= F.words
                row["single"] += k.nf == 1 and k.why != gp.END
    return "    %-8s %-7s %5d %8d %8d %9d %9d %6d" % (label, form, row["wg"], row["lit"], row["exact"], row["rounding"], row["single"], row["most"])


def observed_tables():
    lines = ["Census, over every group of a clip (printed by running this file, not asserted):", "",
             "    clip     form      wgs  cut by   of them   of them   chunks of   most",
             "                            literals exact     rounding  one frame   chunks"]
    randoms = []
    for w, h in RANDOM_CLIPS:
        c = random_clip(w, h)
        randoms.append((c, gc.staged(c)))
    for name, form in CASES:
        lines.append(census_row(name, form, gc.clip(name), gc.records(name)))
    for c, descs in randoms:
        for form in gp.FORMS:
            lines.append(census_row(c.name, form, c, descs))
    lines += ["", "Frames a faulty walk gets wrong (0 = the clip lets the mistake through); the random clips reach the loader form in their",
              "test, the self-staging column is what they would do if they reached it:", "",
              "    fault            L loader / self   S self   H loader / self   " + "   ".join("%s loader / self" % c.name for c, _ in randoms)]
    for fault, forms in gp.FAULTS.items():
        cells = []
        for name in NAMES:
            c, groups = gc.clip(name), gc.groups(gc.records(name))
            cells.append(" / ".join("%d" % wrong_frames(c, groups, form, fault) if form in forms else "-" for form in gc.FORMS_OF[name]))
        for c, descs in randoms:
            groups = gc.groups(descs)
            cells.append(" / ".join("%d" % wrong_frames(c, groups, form, fault) if form in forms else "-" for form in gp.FORMS))
        lines.append("    %-16s %-17s %-8s %-17s " % (fault, cells[0], cells[1], cells[2]) + "   ".join("%-20s" % v for v in cells[3:]))
    return "\n".join(lines)


if __name__ == "__main__":
    print(observed_tables())
