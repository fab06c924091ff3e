"""The directed clips of tests/sp_activity_clips.py, without a GPU: the oracle reproduces what was painted, the clips hold what
they were painted for (census, asserted on the oracle's pictures and the host stage's records), the two models of
sp_index_activity_kernel's walk (index_activity_ref.sp_model, sp_lane_model) equal THE DEFINITION on every run the GPU test walks,
and every deliberately broken walk is caught — which clip catches which is stated in CATCHES and asserted both ways.

Only references are compared with the oracle here: nothing of this file runs a kernel."""
import numpy as np
import pytest

import index_activity_ref as ar
import sp_activity_clips as ac

ALL = set(ac.NAMES)
# wrong walk: the clips on which some run's map (with its guard rows) differs from the definition — exactly these
CATCHES = {
    "rect_area": ALL,                       # what the painted clips A/B/C cannot see: their rectangles are all change
    "stale": ALL,                           # ... nor this: their registers are never compared with a value that comes back
    "key_ignored": ALL,
    "zeros_counted": ALL,
    "open_end": ALL,
    "three_ballots": ALL,
    # `inpic` whole where the row ends inside a chunk: the scalar sizes.  At 72 x 16 every chunk is whole.
    "chunk_whole": set(ac.SCALAR),
}
# wrong walks that change no count (index_activity_ref's docstring has why); no_bx_guard reads a block number past the tables where
# a workgroup has a wave with bx >= nbx: nbx % 4 != 0 — 66 x 20, 17 x 17 and 13 x 9 among them
SILENT = ("open_start", "no_bx_guard")
LANE = ("no_bx_guard", "chunk_whole", "three_ballots")


def walk(name, first, n, wrong=None, faults=None):
    c = ac.clip(name)
    if wrong in LANE:
        return ar.sp_lane_model(ac.composer(name), c.w, c.h, first, n, wrong=wrong, guard=True, faults=faults)
    return ar.sp_model(ac.composer(name), c.w, c.h, first, n, wrong=wrong, guard=True)


def guarded(name, first, n):
    """The definition over the oracle's pictures with a zero row in front and behind."""
    want = ac.truth(name)[first:first + n]
    zero = np.zeros((1,) + want.shape[1:], dtype=np.uint16)
    return np.concatenate([zero, want, zero])


@pytest.mark.parametrize("name", ac.NAMES)
def test_the_oracle_reproduces_the_painting(name):
    c = ac.clip(name)
    pictures, verdicts = ac.oracle(name)
    assert len(c.chunks) == ac.N and (c.w, c.h, c.bpp, c.version) == ac.SPECS[name]
    for t in range(ac.N):
        assert np.array_equal(pictures[t], c.frames[t]), f"{c.name} frame {t}: the oracle's picture is not the painted one"
        assert np.array_equal(ac.composer(name).picture(t), c.frames[t]), f"{c.name} frame {t}: Composer.picture"
        if not c.keys[t]:
            assert ac.composer(name).verdict_p[t] == verdicts[t], f"{c.name} frame {t}: host-stage verdict differs from DecompressP's"
    assert verdicts[ac.REPEAT_AT] is False and verdicts[ac.FAR_KEY] is True
    a, b = ac.values(c.bpp)
    flat = int(c.frames[ac.FLAT_AT][0])
    assert set(np.unique(np.concatenate(c.frames)).tolist()) == {0, a, b, flat}, "a handful of values"
    legal = 0x1F1F1F if c.bpp == 16 else 0xFFFFFF
    assert a & ~legal == 0 and b & ~legal == 0


@pytest.mark.parametrize("name", ac.NAMES)
def test_census(name):
    c = ac.clip(name)
    facts = ac.census(c, ac.oracle(name)[0], ac.composer(name))
    assert ar.grid(c.w, c.h) == {"17x17": (2, 2), "66x20": (5, 2), "79x33": (5, 3), "72x16": (5, 1), "13x9": (1, 1)}[name]
    assert set(ac.ZERO_AT) <= set(facts["to_zero"])
    runs = ac.runs(c)
    assert len(runs) == len(set(runs)) and {(0, ac.N), (31, 2), (33, 31), (39, 3), (41, 1), (64, 6), (ac.N - 1, 1), (19, 2), (63, 2), (65, 1)} <= set(runs)


def test_the_census_notices_a_missing_role():
    soft = ac.build("66x20", skip=("holes",))
    import sp_index_ref as ref
    with pytest.raises(AssertionError, match="changes just two pixels far apart"):
        ac.census(soft, soft.frames, ref.Composer(soft, preinit=ac.KEY_ROW))


@pytest.mark.parametrize("name", ac.NAMES)
def test_both_models_equal_the_definition(name):
    c = ac.clip(name)
    comp = ac.composer(name)
    for first, n in ac.runs(c):
        want = guarded(name, first, n)
        faults = []
        assert np.array_equal(ar.sp_model(comp, c.w, c.h, first, n, guard=True), want), f"{c.name} sp_model first={first} n={n}"
        assert np.array_equal(ar.sp_lane_model(comp, c.w, c.h, first, n, guard=True, faults=faults), want), f"{c.name} sp_lane_model first={first} n={n}"
        assert not faults
        assert np.array_equal(ar.sp_model(comp, c.w, c.h, first, n), want[1:-1])
    # by hand: the beat alone gives every inter frame a count of at least 1 in every block, and the repeated key frame changes nothing
    whole = ac.truth(name)
    for t in range(ac.N):
        if not c.keys[t]:
            assert whole[t].min() >= 1, f"{c.name} frame {t}"
            if t % ac.HOLES_EVERY and t not in ac.ZERO_AT + ac.RESTORE_AT + ac.PAINT_B_AT:
                assert (whole[t] == 1).all(), f"{c.name} frame {t}: the beat and nothing else"
    assert not whole[ac.REPEAT_AT].any()
    zero_part = min(ac.ZERO_COLUMNS, c.w)
    assert int(whole[0].sum()) == (c.w - zero_part) * c.h, "frame 0: the non-zero pixels and no others"


@pytest.mark.parametrize("wrong", sorted(CATCHES))
def test_a_wrong_walk_is_caught(wrong):
    caught, where = set(), {}
    for name in ac.NAMES:
        for first, n in ac.runs(ac.clip(name)):
            if not np.array_equal(walk(name, first, n, wrong), guarded(name, first, n)):
                caught.add(name)
                where.setdefault(name, (first, n))
    assert caught == CATCHES[wrong], f"{wrong}: caught on {sorted(caught)} (first failing runs {where})"


def test_open_end_shows_in_the_row_behind_the_map_only():
    for name in ac.NAMES:
        for first, n in ac.runs(ac.clip(name)):
            got, want = walk(name, first, n, "open_end"), guarded(name, first, n)
            assert np.array_equal(got[:-1], want[:-1])
            if (first + n) & 31 and first + n < ac.N and first + n != ac.REPEAT_AT:
                assert got[-1].all(), f"{name} ({first}, {n}): frame {first + n} has a count in every block"


@pytest.mark.parametrize("wrong", SILENT)
def test_a_wrong_walk_that_changes_no_count(wrong):
    """open_start: frame first - 1 is compared with the picture it made.  no_bx_guard: the waves that go on own no pixel; what they
    do is read a block number past the tables, in the last row of blocks, wherever nbx is no multiple of 4."""
    reads = {}
    for name in ac.NAMES:
        for first, n in ac.runs(ac.clip(name)):
            faults = []
            assert np.array_equal(walk(name, first, n, wrong, faults), guarded(name, first, n)), f"{wrong} {name} ({first}, {n})"
            reads.setdefault(name, set()).update(faults)
    if wrong == "no_bx_guard":
        for name in ac.NAMES:
            nbx, nby = ar.grid(*ac.SPECS[name][:2])
            want = {("block", nby - 1, bx, (nby - 1) * nbx + bx) for bx in range(nbx, 4 * ((nbx + 3) // 4))}
            assert reads[name] == want and want, name
        assert len(reads["13x9"]) == 3 and len(reads["17x17"]) == 2 and len(reads["66x20"]) == 3


def test_chunk_whole_reads_past_the_picture_in_its_last_row():
    for name in ac.NAMES:
        c = ac.clip(name)
        faults = []
        walk(name, 0, ac.N, "chunk_whole", faults)
        assert bool(faults) == (name in ac.SCALAR)
        assert all(what == "pixel" and at >= c.w * c.h for what, _, _, at in faults)
