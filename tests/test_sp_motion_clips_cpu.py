"""The directed motion clips of tests/sp_motion_clips.py, without a GPU: the host stage reports exactly the motion blocks, rectangles
and vectors the clips were painted for (a census, asserted against sp_motion_clips.plan and against the catalogue of roles); the
painted picture, the kernel's restatement over the host stage's records (hoststage_binding.expand_pframe), the oracle and the
restatement after literalise_motion are one and the same picture; a staged batch literalises exactly the frames that move at most
a quarter of their pixels; the reference's typed-array reads under node give the painted pictures; and a restatement with one of
the motion branch's possible mistakes built in (hoststage_binding.MOTION_FAULTS) leaves a wrong picture on the role meant to catch
it."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import hoststage_binding as hb
import sp_motion_clips as mc

HERE = os.path.dirname(os.path.abspath(__file__))
NODE = shutil.which("node")


@pytest.fixture(scope="module")
def decoded():
    """name -> the host stage's answer per frame, motion kept (HostStage.decode), each with `literal`: the same frame after
    literalise_motion."""
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = decode(mc.clip(name))
        return cache[name]
    return get


def decode(c):
    hs = hb.HostStage(c.w, c.h, c.bpp)
    hs.preinit(mc.KEY_ROW)
    out = []
    for t, (src, key) in enumerate(zip(c.chunks, c.keys)):
        d = hs.decode(key, src)
        assert d["status"] == 0, (c.name, t, d["error"])
        d["literal"] = hs.literalise_motion(d) if d["kind"] == hb.KIND_INTER else None
        out.append(d)
    hs.close()
    return out


# --------------------------------------------------------------------------------------------------------------------- census

def records_of(d):
    """{block: (flags, rectangle, vector)} of the blocks a frame codes."""
    out = {}
    for b in np.nonzero(d["blocks"][:, 0])[0]:
        r = d["blocks"][b]
        mx, my = (int(v) for v in np.frombuffer(r[8:12].tobytes(), dtype=np.int16))
        out[int(b)] = (int(r[0]), tuple(int(v) for v in r[1:5]), (mx, my))
    return out


def check_census(name, c, descs, plan):
    """The host stage's records are the plan's, block for block, and (M, U, H) every role of the catalogue is there with what it is
    for; raises AssertionError naming the first thing that is missing."""
    nbx, nby = mc.geometry(c.w, c.h)
    pw, ph = c.w - 16 * (nbx - 1), c.h - 16 * (nby - 1)
    assert len(descs) == len(plan)
    for role in mc.Q_ROLES if name == "Q" else mc.ROLES:
        assert any(p["role"] == role and (p["blocks"] or role == "nothing") for p in plan), f"{role}: no frame of this role"
    recs = []
    for t, (d, p) in enumerate(zip(descs, plan)):
        where = f"{c.name} frame {t} ({p['role']})"
        kind = {hb.KIND_INTRA: "key", hb.KIND_NONE: "none", hb.KIND_INTER: "inter"}[d["kind"]]
        assert kind == p["kind"], f"{where}: decoded as {kind}, planned as {p['kind']}"
        got = records_of(d) if kind == "inter" else {}
        recs.append(got)
        for b, want in p["blocks"].items():
            assert b in got, f"{where}: block {b} is not coded"
            assert got[b] == want, f"{where}: block {b} is coded as (flags, rectangle, vector) {got[b]}, painted as {want}"
        for b, r in got.items():
            assert b in p["blocks"], f"{where}: block {b} is coded {r}, the table does not paint it"
        assert (d["motion_pixels"], d["prev_pixels"], d["data_pixels"]) == (p["motion_pixels"], p["prev_pixels"], p["data_pixels"]), \
            f"{where}: motion / copied / literal pixels"
    moved = [{b: r for b, r in g.items() if r[0] & hb.PB_MOTION} for g in recs]
    if name == "Q":
        assert [p["role"] for p in plan] == ["key", "quarter", "over"]
        assert descs[1]["motion_pixels"] * 4 == c.w * c.h and len(moved[1]) == 4, "quarter: not exactly a quarter of the picture"
        assert descs[2]["motion_pixels"] * 4 == c.w * c.h + 4 and len(moved[2]) == 5, "over: not one pixel more than a quarter"
        assert sum(1 for r in moved[2].values() if r[1][2] - r[1][0] == 1 and r[1][3] - r[1][1] == 1) == 1, "over: no 1x1 rectangle"
        return
    by_role = {role: [t for t, p in enumerate(plan) if p["role"] == role and (p["blocks"] or role == "nothing")] for role in mc.ROLES}

    def vectors(role, pick=lambda b, r: True):
        return {r[2] for t in by_role[role] for b, r in moved[t].items() if pick(b, r)}

    def subs(role):
        return [(b, r[1]) for t in by_role[role] for b, r in moved[t].items() if r[0] & hb.PB_SUBRECT]

    v = vectors("in-frame")
    assert {mx % 4 for mx, my in v} >= {1, 2, 3} and all(my != 0 for mx, my in v), f"in-frame: vectors {sorted(v)}"
    t = by_role["in-frame"][0]
    assert any(b + 1 in moved[t] and moved[t][b + 1][2] == r[2] for b, r in moved[t].items()), "in-frame: no vector repeated on the next block"
    assert any(b + 2 in moved[t] and moved[t][b + 2][2] == r[2] and recs[t].get(b + 1, (0,))[0] & hb.PB_DATA for b, r in moved[t].items()), \
        "in-frame: no vector repeated behind a data block"
    assert (-1, 0) in vectors("edges", lambda b, r: b == 0), "edges: block 0 does not read index -1"
    assert (1, 0) in vectors("edges", lambda b, r: b == nbx * nby - 1), "edges: the last block does not read index X*Y"
    assert any(my == -5 for mx, my in vectors("edges", lambda b, r: b < nbx)), "edges: no top-row block from above the picture"
    assert any(my == 3 for mx, my in vectors("edges", lambda b, r: b >= nbx * (nby - 1))), "edges: no bottom-row block from below the picture"
    assert {(0, -256), (0, 255)} <= vectors("edges"), "edges: the extremes of my"
    assert any(mx == -9 for mx, my in vectors("wrap", lambda b, r: b % nbx == 0)), "wrap: no column-0 block reading the row above"
    assert any(mx == 9 for mx, my in vectors("wrap", lambda b, r: b % nbx == nbx - 1)), "wrap: the right block does not read the row below"
    assert {(-256, 0), (255, 1)} <= vectors("wrap"), "wrap: the extremes of mx"
    s = subs("subrect")
    assert any(x1 % 4 and (x2 - x1) % 4 for _, (x1, y1, x2, y2) in s), "subrect: no rectangle off the 4-pixel grid"
    assert any((x2 - x1, y2 - y1) == (1, 1) for _, (x1, y1, x2, y2) in s), "subrect: no 1x1 rectangle"
    assert any((x1, y1, x2, y2) == (15, 0, 16, 16) for _, (x1, y1, x2, y2) in s), "subrect: no column 15 alone"
    assert any(b % nbx == nbx - 1 and x2 == pw and x1 > 0 for b, (x1, y1, x2, y2) in s), "subrect: none at the picture's right edge"
    assert any(b >= nbx * (nby - 1) and y2 == ph for b, (x1, y1, x2, y2) in s), "subrect: none in the bottom block row"
    t = by_role["scroll"][0]
    assert len(moved[t]) == nbx * nby and len({r[2] for r in moved[t].values()}) == 1 and not subs("scroll"), "scroll: not every block whole by one vector"
    assert descs[t]["motion_pixels"] == c.w * c.h
    t = by_role["mixed"][0]
    kinds = {r[0] for r in recs[t].values()}
    assert {hb.PB_MOTION, hb.PB_DATA, hb.PB_DATA | hb.PB_SUBRECT} <= kinds and len(recs[t]) < nbx * nby, f"mixed: block kinds {sorted(kinds)}"
    assert any(recs[t].get(b + nbx, (0,))[0] == hb.PB_DATA and recs[t].get(b + 1, (0,))[0] == hb.PB_DATA for b in moved[t]), \
        "mixed: no motion block with a repainted block below it and one to its right"
    t = by_role["carry"][0]
    assert by_role["nothing"] == [t - 1] and descs[t - 1]["kind"] == hb.KIND_NONE, "carry: not behind a frame that changes nothing"
    last = [r[2] for b, r in sorted(moved[t - 2].items())][-1]
    first = [r[2] for b, r in sorted(moved[t].items())]
    assert first[0] == last and first[1] == last, "carry: the first vector is not the last one of the motion frame before"
    ch = by_role["chain"]
    assert len(ch) == 5 and ch == list(range(ch[0], ch[0] + 5)) and plan[ch[0] - 1]["kind"] == "key", "chain: not five frames behind a key frame"
    share = [descs[t]["motion_pixels"] * 4 / (c.w * c.h) for t in ch]
    assert share[0] == 0 and 0 < share[1] <= 1 and share[2] > 1 and share[3] == 0 and 0 < share[4] <= 1, f"chain: motion shares {share}"
    heavy = np.zeros((c.h, c.w), bool)
    for b in moved[ch[2]]:
        x16, y16, bw, bh = mc.block_box(b, c.w, c.h)
        heavy[y16:y16 + bh, x16:x16 + bw] = True
    for b, r in moved[ch[4]].items():
        x16, y16, bw, bh = mc.block_box(b, c.w, c.h)
        ys, xs = np.mgrid[y16:y16 + bh, x16:x16 + bw]
        j = (ys + r[2][1]) * c.w + xs + r[2][0]
        assert heavy.reshape(-1)[j].all(), "chain: the last light frame moves pixels the heavy frame did not move"


@pytest.mark.parametrize("name", mc.NAMES)
def test_census(name, decoded):
    check_census(name, mc.clip(name), decoded(name), mc.plan(name))


@pytest.mark.parametrize("role", [r for r in mc.ROLES if r != "nothing"])
def test_the_census_notices_a_missing_role(role):
    c = mc.build("M", skip=(role,))
    descs = decode(c)
    with pytest.raises(AssertionError, match=role + ": no frame of this role"):
        check_census("M", c, descs, mc.plan("M", skip=(role,)))
    # and against the whole plan the clip's own records give the missing frame away
    t = mc.frames_of("M", role)[0]
    with pytest.raises(AssertionError, match=rf"frame {t} \({role}\): decoded as none, planned as inter"):
        check_census("M", c, descs, mc.plan("M"))


def test_the_census_notices_a_rectangle_that_shrank():
    """A painting that matches the picture before in a block's last column: the plan's whole block is coded as a sub-rectangle."""
    c = mc.clip("U")
    descs = [dict(d) for d in decode(c)]
    t = mc.frames_of("U", "in-frame")[0]
    blocks = descs[t]["blocks"].copy()
    b = next(iter(mc.plan("U")[t]["blocks"]))
    blocks[b, 3] -= 1
    blocks[b, 0] |= hb.PB_SUBRECT
    descs[t]["blocks"] = blocks
    with pytest.raises(AssertionError, match=f"block {b} is coded as"):
        check_census("U", c, descs, mc.plan("U"))


# ------------------------------------------------------------------------------------------------------------------- pictures

@pytest.mark.parametrize("name", mc.NAMES + ("M2",))
def test_painting_restatement_oracle_and_literalised_restatement_are_one_picture(name, decoded):
    c = mc.clip(name)
    pictures, _ = mc.oracle(name)
    before = None
    for t, d in enumerate(decoded(name)):
        want = c.frames[t]
        if d["kind"] == hb.KIND_INTRA:
            got = [("expand_iframe", hb.expand_iframe(d, c.w, c.h))]
        elif d["kind"] == hb.KIND_NONE:
            assert not d["adopted"]
            got = [("the picture before", before)]
        else:
            assert d["adopted"]
            lit = d["literal"]
            assert not any(b[0] & hb.PB_MOTION for b in lit["blocks"]), f"{c.name} frame {t}: a motion block survives literalise_motion"
            assert all(int(np.frombuffer(b[12:16].tobytes(), np.uint32)[0]) % 4 == 0 for b in lit["blocks"] if b[0]), "a rectangle's literals start on a 16-byte boundary"
            got = [("expand_pframe over the host stage's records", hb.expand_pframe(d, before, c.w, c.h)),
                   ("expand_pframe after literalise_motion", hb.expand_pframe(lit, before, c.w, c.h))]
        got += [("the encoder's picture", c.encoder_frames[t]), ("the oracle's picture", pictures[t])]
        for what, pic in got:
            assert np.array_equal(pic, want), f"{c.name} frame {t}, {what}: " + mc.describe_mismatch(pic, want, c.w, c.h)
        before = want


@pytest.mark.parametrize("name", mc.NAMES)
def test_a_staged_batch_literalises_up_to_a_quarter_and_keeps_the_rest(name):
    c = mc.clip(name)
    plan = mc.plan(name)
    descs = mc.staged(c)
    before = None
    for t, (d, p) in enumerate(zip(descs, plan)):
        assert d["status"] == 0, (t, d["error"])
        if p["kind"] == "inter":
            assert d["literalised"] == p["literalised"], f"{c.name} frame {t} ({p['role']}): {d['motion_pixels']} of {c.w * c.h} pixels moved"
            assert any(b[0] & hb.PB_MOTION for b in d["blocks"]) == (p["motion_pixels"] > 0 and not p["literalised"])
            got = hb.expand_pframe(d, before, c.w, c.h)
            assert np.array_equal(got, c.frames[t]), f"{c.name} frame {t}: " + mc.describe_mismatch(got, c.frames[t], c.w, c.h)
        before = c.frames[t]
    if name == "Q":
        assert [p["motion_pixels"] for p in plan] == [0, 1024, 1025] and c.w * c.h == 4096
        assert [d["literalised"] for d in descs] == [False, True, False]
        assert mc.kept(name) == [2] and mc.launches(name) == 3
    else:
        role_of = [p["role"] for p in plan]
        ch = mc.frames_of(name, "chain")
        assert set(mc.frames_of(name, "scroll") + [ch[2]]) <= set(mc.kept(name))
        assert all(descs[t]["literalised"] for t in (ch[0], ch[1], ch[3], ch[4]))
        assert mc.kept(name) == [t for t in range(len(plan)) if role_of[t] in ("edges", "scroll")] + [ch[2]]
        assert mc.launches(name) == 10 and mc.launches(name, fused=False) == 14


@pytest.mark.parametrize("name", mc.NAMES)
def test_staged_as_the_seek_index_stages_no_motion_block_survives(name):
    """literalise_all: every inter frame literalised, the heavy and scroll frames too; the pictures do not change."""
    c = mc.clip(name)
    hs = hb.HostStage(c.w, c.h, c.bpp)
    hs.preinit(mc.KEY_ROW)
    descs = hs.decode_batch(c.chunks, c.keys, 1, literalise="all")
    hs.close()
    before = None
    for t, (d, p) in enumerate(zip(descs, mc.plan(name))):
        assert d["status"] == 0, (t, d["error"])
        if p["kind"] == "inter":
            assert d["literalised"] and not any(b[0] & hb.PB_MOTION for b in d["blocks"]), f"{c.name} frame {t}"
            got = hb.expand_pframe(d, before, c.w, c.h)
            assert np.array_equal(got, c.frames[t]), f"{c.name} frame {t}: " + mc.describe_mismatch(got, c.frames[t], c.w, c.h)
        before = c.frames[t]


# --------------------------------------------------------------------------------------------------------------- JS semantics

@pytest.mark.skipif(NODE is None, reason="node not installed")
def test_the_references_typed_array_reads_give_the_painted_pictures():
    """The plain typed-array decoder of tests/js/sp_js_semantics.js under node — an Int32Array read outside the buffer is undefined,
    stored as 0: the reference's own rule — over H and over M's painting coded as version 2 (that decoder reads the range coder
    only)."""
    names = ("M2", "H")
    cases = [dict(w=c.w, h=c.h, bpp=c.bpp, lines=mc.KEY_ROW, prefill=0x00A5A5A5,
                  frames=[dict(key=bool(k), bytes=list(s)) for s, k in zip(c.chunks, c.keys)]) for c in (mc.clip(n) for n in names)]
    res = subprocess.run([NODE, os.path.join(HERE, "js", "sp_js_semantics.js")], input=json.dumps(cases).encode(),
                         stdout=subprocess.PIPE, check=True, timeout=300)
    checked = 0
    for name, jres in zip(names, json.loads(res.stdout)):
        c = mc.clip(name)
        plan = mc.plan(name)
        _, verdicts = mc.oracle(name)
        assert len(jres) == len(c.chunks)
        for t, jr in enumerate(jres):
            assert not jr["raised"] and not jr["hang"], (name, t)
            if plan[t]["kind"] == "none":
                assert jr["same"], (name, t)
                continue
            if plan[t]["kind"] == "key":
                assert jr["state"] == 0, (name, t)
            else:
                assert not jr["same"] and jr["signif"] == verdicts[t], (name, t)
            got = np.array(jr["dst"], dtype=np.int64).astype(np.uint32)
            assert np.array_equal(got, c.frames[t]), f"{c.name} frame {t} under node: " + mc.describe_mismatch(got, c.frames[t], c.w, c.h)
            checked += 1
    assert checked == 2 * 14


# ---------------------------------------------------------------------------------------------------------------- wrong kernels

# the role whose frames must show the mistake
CAUGHT_BY = {"clip_per_axis": "wrap", "oob_is_colocated": "edges", "reads_written_frame": "scroll", "subrect_ignored": "subrect",
             "vector_swapped": "in-frame"}


def test_every_fault_is_named():
    assert set(CAUGHT_BY) == set(hb.MOTION_FAULTS)


@pytest.mark.parametrize("fault", hb.MOTION_FAULTS)
@pytest.mark.parametrize("name", mc.ROLE_CLIPS)
def test_a_wrong_motion_branch_fails_on_its_role(name, fault, decoded):
    c = mc.clip(name)
    descs = decoded(name)
    wrong = 0
    for t in mc.frames_of(name, CAUGHT_BY[fault]):
        got = hb.expand_pframe(descs[t], c.frames[t - 1], c.w, c.h, fault=fault)
        wrong += int((got != c.frames[t]).sum())
    assert wrong > 0, f"fault {fault} passes the {CAUGHT_BY[fault]} frames of clip {name}"
