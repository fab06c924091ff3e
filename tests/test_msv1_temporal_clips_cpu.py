"""The directed inter-frame groups of tests/msv1_temporal_clips.py for msv1_blocks_temporal_kernel, without a GPU:
  * the kernel's restatement (tests/msv1_temporal_plan.py) confirms every claim a clip makes about chunks, cuts and spans;
  * its walk with no fault leaves in every buffer, and says in every flag, what the CPU oracle does (Manager's buffer protocol,
    frame by frame), for frames laid out as the host parse and as the on-GPU parse lay them out — and the oracle's pictures
    are the pictures by construction;
  * a walk that makes one of the kernel's possible mistakes (msv1_temporal_plan.FAULTS) leaves a wrong picture or flag on the
    clips named in CATCHES: the catalogue would fail a kernel with that mistake, and says which seam it broke;
  * the model's constants are the kernel's.

Observed once on an MI355X with two libraries built with a deliberate mistake in the kernel (not kept): with significance filed
under the chunk slot (`tf.index = kept`), tests/test_msv1_temporal_directed_gpu.py failed on exactly the twelve clips the table
below gives for slot_index, in both parse modes, and on tails_16 (the same record also says whose odd last byte to keep); with the
zeroing loop of step 4 left out it failed on tails_16 alone, as the table gives for stale_tail.

The table (printed in full, with the number of wrong buffers + flags, by `PYTHONPATH=.:tests python tests/test_msv1_temporal_clips_cpu.py`):

    swapped_buffer      count_33, count_49, code_cut, tails (16 and 8), sig_words_16
    skip_after_cut      code_cut, tails (16 and 8)
    slot_index          count_17_16, count_32_16, count_33_16, count_49_16, code_cut_16, three_tiles_16, noop_front_16, noop_between_16,
                        noop_17th_16, allskip_neighbour_16, sig_carried_16, sig_words_16
    sig_one_word        count_33_16, count_49_16, sig_words_16
    first_lost_to_noop  noop_front_16, noop_between_16, noop_17th_16, allskip_neighbour_16, sig_carried_16
    block_rows          sig_rows_16
    quad_guard          partial_1028x4, _24x172, _28x148, _36x116, _68x60 (16 and 8; not 64x64 and 64x68: no partial quad)
    stale_tail          tails_16 (the 8-bit decode masks every colour byte by `avail`)
    tail_byte_dropped   tails_16
    hi_short            36 clips, among them code_cut, span, tails (16 and 8)
    lo_unrounded_at     all 49 temporal clips (a tile's first code rarely starts on a multiple of 16); span pins offsets 0, 2, 14, 16
    noop_takes_slot     noop_front_16, noop_between_16, noop_tail_16, noop_17th_16, allskip_neighbour_16, sig_carried_16

What a test of the kernel can look at is what a batch leaves behind — the buffers after the last frame and a flag per frame — so
the clips whose evidence is a picture (code_cut, span, tails, noop_17th, sig_carried) decode every frame into a buffer of its own.
tests/test_msv1_temporal_directed_gpu.py sends the same clips through the kernel."""
import functools
import os
import re

import numpy as np
import pytest

import msv1_directed_streams as D
import msv1_temporal_clips as K
import msv1_temporal_plan as P
from oracle_binding import OracleMSVideo1

SOURCE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "jsplayer_amd", "csrc", "msv1_kernels.hip")

# Which clips catch which fault (every one of them is run with the fault below; the full table is printed by running this file).
CATCHES = {
    "swapped_buffer": ["count_33_16", "count_49_16", "count_33_8", "count_49_8", "code_cut_16", "code_cut_8", "tails_16", "tails_8", "sig_words_16"],
    "skip_after_cut": ["code_cut_16", "code_cut_8", "tails_16", "tails_8"],
    "slot_index": ["count_17_16", "count_32_16", "count_33_16", "count_49_16", "code_cut_16", "three_tiles_16", "noop_front_16", "noop_between_16",
                   "noop_17th_16", "allskip_neighbour_16", "sig_carried_16", "sig_words_16"],
    "sig_one_word": ["count_33_16", "count_49_16", "sig_words_16"],
    "first_lost_to_noop": ["noop_front_16", "noop_between_16", "noop_17th_16", "allskip_neighbour_16", "sig_carried_16"],
    "block_rows": ["sig_rows_16"],
    "quad_guard": ["partial_1028x4_16", "partial_24x172_16", "partial_28x148_16", "partial_36x116_16", "partial_68x60_16",
                   "partial_1028x4_8", "partial_24x172_8", "partial_28x148_8", "partial_36x116_8", "partial_68x60_8"],
    "stale_tail": ["tails_16"],        # (the 8-bit decode masks every colour byte by `avail`: it never looks at bytes behind the end)
    "tail_byte_dropped": ["tails_16"],
    "hi_short": ["code_cut_16", "code_cut_8", "span_16", "span_8", "tails_16", "tails_8"],
    "lo_unrounded_at": ["span_16", "span_8"],
    "noop_takes_slot": ["noop_front_16", "noop_between_16", "noop_tail_16", "noop_17th_16", "allskip_neighbour_16", "sig_carried_16"],
}

NAMES = [
    "count_1_16", "count_15_16", "count_16_16", "count_17_16", "count_32_16", "count_33_16", "count_49_16", "code_cut_16", "span_16",
    "tails_16", "partial_64x64_16", "partial_64x68_16", "partial_1028x4_16", "partial_24x172_16", "partial_28x148_16",
    "partial_36x116_16", "partial_68x60_16", "key_mid_16", "three_tiles_16", "y_edge_16", "x_edge_16",
    "count_1_8", "count_15_8", "count_16_8", "count_17_8", "count_32_8", "count_33_8", "count_49_8", "code_cut_8", "span_8",
    "tails_8", "partial_64x64_8", "partial_64x68_8", "partial_1028x4_8", "partial_24x172_8", "partial_28x148_8",
    "partial_36x116_8", "partial_68x60_8", "key_mid_8", "three_tiles_8", "y_edge_8", "x_edge_8",
    "noop_front_16", "noop_between_16", "noop_tail_16", "noop_17th_16", "allskip_neighbour_16",
    "sig_rows_16", "sig_carried_16", "sig_last_lane_16", "sig_words_16"]
# (stated, not derived at import: building the catalogue takes a second, and every collection of the suite would pay for it)


def test_the_names_stated_here_are_the_catalogue_s():
    assert NAMES == K.names()


def test_every_seam_has_clips_of_both_depths():
    for seam in range(1, 10):
        for bits in (16, 8):
            if seam == 3 and bits == 8:
                continue                                    # (no-op frames are the 16-bit decoder's)
            assert any(seam in c.seams and c.bits == bits for c in K.catalogue()), (seam, bits)
    sig8 = [c for c in K.catalogue() if c.bits == 8]
    assert sig8 and all(not any(oracle_run(c.name)[2]) for c in sig8), "8-bit never compares: no frame is significant"


def test_the_seven_sizes_have_the_remainders_they_are_listed_for():
    assert sorted(K.SIZES.values()) == [0, 1, 2, 3, 5, 16, 255]
    for (w, h), rem in K.SIZES.items():
        assert (w // 4) * (h // 4) % 256 == rem and w % 4 == 0 and h % 4 == 0, (w, h)
        for bits in (16, 8):
            c = K.by_name(f"partial_{w}x{h}_{bits}")
            assert c.nblocks % 256 == rem and P.tiles(c.nblocks) == 2 - (rem in (0, 255))
    w, h = K.THREE_TILES
    assert P.tiles((w // 4) * (h // 4)) == 3
    assert K.Y_EDGE[1] % 4 and not K.Y_EDGE[0] % 4 and K.X_EDGE[0] % 4 and not K.X_EDGE[1] % 4


# ---- the oracle, Manager's buffer protocol -------------------------------------------------------------------------------------
def fresh_buffers(c):
    return [np.full(c.w * c.h, v, dtype=np.uint32) for v in c.prefills]


def grid(c, buf):
    return np.asarray(buf).view(np.uint32).reshape(c.h, c.w)[:c.gh, :c.gw].reshape(-1)


@functools.lru_cache(maxsize=None)
def oracle_run(name):
    """-> (buffers at the end, adopted per frame, significant per frame); asserts on the way that the clip hands out buffers as
    Manager would (never the previous frame) and that every picture by construction is the oracle's."""
    c = K.by_name(name)
    orc = OracleMSVideo1(c.bits, c.w, c.h, D.palette(c.bits))
    orc.Preinit(c.lines)
    bufs = [b.view(np.int32) for b in fresh_buffers(c)]
    if c.start == "sync":
        assert orc.DecompressI(c.sync_key, bufs[c.nbuf]) == 0
    adopted, signif = [], []
    for i, ((src, key), d) in enumerate(zip(c.frames, c.dsts)):
        assert bufs[d] is not orc.PreviousFrame(), f"{name} frame {i}: the clip decodes into the previous frame"
        before = bufs[d].copy()
        if key:
            assert orc.DecompressI(src, bufs[d]) == 0
            adopted.append(True)
            signif.append(False)
        else:
            data, sig = orc.DecompressP(src, bufs[d])
            adopted.append(data is bufs[d])
            signif.append(sig)
        pic = c.pictures[i]
        if isinstance(pic, str):
            assert pic == K.UNTOUCHED and np.array_equal(bufs[d], before) and not adopted[-1], f"{name} frame {i}: a no-op frame"
        elif pic is not None:
            assert np.array_equal(grid(c, bufs[d]), pic), f"{name} frame {i}: the oracle's picture is not the one by construction"
    orc.close()
    return [b.view(np.uint32) for b in bufs], adopted, signif


def model_run(c, align, fault=None):
    """The model over the clip's batch (the synchronous key frame walked by the same model first) -> (buffers, adopted, signif, staged)."""
    bufs = fresh_buffers(c)
    pal = D.palette(c.bits)
    rows = [0] * (c.h // 4)
    prev = None
    if c.start == "sync":
        st0 = P.stage(c.bits, c.w, c.h, [c.sync_key], [True], [c.nbuf], c.lines, None, align, pal, rows)
        P.run(st0, bufs)
        prev = st0.prev_after
    st = P.stage(c.bits, c.w, c.h, [f for f, _ in c.frames], [k for _, k in c.frames], c.dsts, c.lines, prev, align, pal, rows)
    status, adopted, signif = P.run(st, bufs, fault)
    assert status == [0] * len(c.frames)
    return bufs, adopted, signif, st


@pytest.mark.parametrize("name", NAMES)
def test_pictures_by_construction_are_the_oracles_and_flags_are_what_the_clip_was_built_for(name):
    c = K.by_name(name)
    _, adopted, signif = oracle_run(name)
    for f, want in c.significant.items():
        assert signif[f] == want, f"{name} frame {f}: built to be {'' if want else 'in'}significant"
    assert len(c.frames) == len(c.dsts) == len(c.pictures) and len(c.prefills) == c.nbuf + 1


@pytest.mark.parametrize("align", [P.HOST_ALIGN, P.GPU_ALIGN], ids=["host-layout", "gpu-layout"])
@pytest.mark.parametrize("name", NAMES)
def test_the_walk_equals_the_oracle(name, align):
    c = K.by_name(name)
    obufs, oadopted, osignif = oracle_run(name)
    bufs, adopted, signif, st = model_run(c, align)
    for k, (a, b) in enumerate(zip(obufs, bufs)):
        assert np.array_equal(a, b), f"{name}: buffer {k} differs"
    assert adopted == oadopted and signif == osignif, name
    kinds = {kind for _, _, kind in st.groups}
    assert kinds == ({"temporal"} if c.kernel == "msv1_blocks_temporal_kernel" else {"blocks"}), (name, st.groups)
    assert len(st.groups) == 1, "every clip is one group"


# ---- claims ---------------------------------------------------------------------------------------------------------------------
def check_claim(c, st, plans, claim):
    kind, t = claim[0], claim[1]
    chunks = plans[t]
    group = st.frames
    slot_of = {s.frame: (ci, s) for ci, ck in enumerate(chunks) for s in ck.slots}
    if kind == "chunks":
        return len(chunks) == claim[2]
    if kind == "opens":
        ck = chunks[claim[2]]
        return ck.slots[0].frame == claim[3] and (claim[2] == 0 or chunks[claim[2] - 1].next == claim[3])
    if kind == "cut":
        ck = chunks[claim[2]]
        return ck.cut and len(ck.slots) == claim[3] and ck.over == claim[4] and ck.next == ck.rows[claim[3]]
    if kind == "fit":
        ck = chunks[claim[2]]
        # (the frame in that slot is the chunk's last, admitted with `over` bytes to spare or none; the next one closes the chunk)
        return len(ck.slots) == claim[3] + 1 and ck.fits[claim[3]] == claim[4] and ck.cut and ck.over > 0
    if kind == "need":
        return slot_of[claim[2]][1].need == claim[3]
    if kind == "rounds":
        return (slot_of[claim[2]][1].need + 1023) // 1024 >= claim[3]
    if kind == "lo":
        a = group[claim[2]]
        live = a.desc[t * P.WG:(t + 1) * P.WG]
        first = int(live[live < P.UNTOUCHED].min())
        return first - a.beg == claim[3] and slot_of[claim[2]][1].lo - a.beg == claim[4]
    if kind == "clipped":
        a = group[claim[2]]
        live = a.desc[t * P.WG:(t + 1) * P.WG]
        s = slot_of[claim[2]][1]
        return int(live[live < P.UNTOUCHED].max()) + 18 > a.stream_end and s.lo + s.need >= a.stream_end > s.lo + s.need - 16
    if kind == "empty_last":
        return len(chunks) >= 2 and not chunks[-1].slots and chunks[-1].next == len(group) and chunks[-2].next < len(group)
    if kind in ("prev_fetch", "no_prev_fetch"):
        return chunks[0].slots[0].first_uses_prev == (kind == "prev_fetch")
    raise AssertionError(f"unknown claim {claim}")


@pytest.mark.parametrize("align", [P.HOST_ALIGN, P.GPU_ALIGN], ids=["host-layout", "gpu-layout"])
@pytest.mark.parametrize("name", NAMES)
def test_the_plan_confirms_every_claim(name, align):
    c = K.by_name(name)
    *_, st = model_run(c, align)
    plans = P.plan(st.frames, st.nblocks)
    for claim in c.claims:
        assert check_claim(c, st, plans, claim), f"{name}: {claim} does not hold; tile {claim[1]}: {P.brief(plans)[claim[1]]}"
    for t, chunks in plans.items():                       # what holds for every plan
        assert chunks[-1].next == len(st.frames) and all(len(ck.slots) <= P.T_NF for ck in chunks)
        kept = [s.frame for ck in chunks for s in ck.slots]
        assert kept == [i for i, a in enumerate(st.frames) if not a.noop], "every written frame is in exactly one chunk, in order"
        for ck in chunks:
            assert all(s.code_at + s.need <= P.T_CODE for s in ck.slots[1:]) and all(s.lo % 16 == 0 for s in ck.slots)


def test_the_exact_fit_and_its_two_neighbours_fall_either_side():
    """code_cut: chunk 1 ends with a frame that fills the code area to the byte, chunk 2 with one 16 bytes shorter — both admitted;
    the same frame 16 bytes longer is refused by chunk 3 and opens chunk 4."""
    for bits, per in ((16, 3), (8, 5)):
        c = K.by_name(f"code_cut_{bits}")
        *_, st = model_run(c, P.HOST_ALIGN)
        chunks = P.plan(st.frames, st.nblocks)[0]
        used = lambda ck, k: ck.slots[k].code_at + ck.slots[k].need      # noqa: E731
        assert used(chunks[1], per) == P.T_CODE and used(chunks[2], per) == P.T_CODE - 16
        assert chunks[3].cut and chunks[3].over == 16 and len(chunks[3].slots) == per
        assert [len(ck.slots) for ck in chunks[:5]] == [per, per + 1, per + 1, per, per]


def test_seam_5_lies_in_reused_buffers():
    """tails: the truncated frames of tile 0 are in chunk 2 or later, and the chunk that had their buffer before held code bytes as
    far as a block of theirs may read."""
    for bits in (16, 8):
        c = K.by_name(f"tails_{bits}")
        *_, st = model_run(c, P.HOST_ALIGN)
        chunks = P.plan(st.frames, st.nblocks)[0]
        cut = [i for i, p in enumerate(c.pictures) if p is None]
        assert len(cut) == 4
        for f in cut[:3]:                                 # (the fourth ends on tile 1's first code: whole in tile 0)
            ci, s = next((ci, s) for ci, ck in enumerate(chunks) for s in ck.slots if s.frame == f)
            assert ci >= 2, (bits, f, ci)
            before = chunks[ci - 2]
            filled = max(x.code_at + x.need for x in before.slots)
            assert filled >= s.code_at + s.need + 18 or s.need == 0, (bits, f)
        assert all(st.frames[f].host for f in cut[:3]) and sum(a.host for a in st.frames) >= 3


# ---- wrong walks ----------------------------------------------------------------------------------------------------------------
def wrong(name, fault):
    """How many buffers and flags a faulty walk gets wrong on a clip."""
    c = K.by_name(name)
    obufs, _, osignif = oracle_run(name)
    bufs, _, signif, _ = model_run(c, P.HOST_ALIGN, fault)
    return sum(1 for a, b in zip(obufs, bufs) if not np.array_equal(a, b)) + sum(1 for a, b in zip(osignif, signif) if a != b)


def test_every_fault_is_named():
    assert sorted(CATCHES) == sorted(P.FAULTS) and all(CATCHES[f] for f in P.FAULTS)
    assert all(n in NAMES for names in CATCHES.values() for n in names)
    assert not P.PLAN_ONLY and set(P.MOVES_PLAN) <= set(P.FAULTS)


@pytest.mark.parametrize("fault", P.FAULTS)
def test_a_wrong_walk_fails_on_the_clips_named_for_it(fault):
    for name in CATCHES[fault]:
        if K.by_name(name).kernel != "msv1_blocks_temporal_kernel":
            continue
        assert wrong(name, fault) > 0, f"fault {fault} passes clip {name}"


@pytest.mark.parametrize("fault", P.MOVES_PLAN)
def test_a_fault_that_moves_the_plan_shows_there_too(fault):
    for name in CATCHES[fault]:
        c = K.by_name(name)
        *_, st = model_run(c, P.HOST_ALIGN)
        assert P.brief(P.plan(st.frames, st.nblocks)) != P.brief(P.plan(st.frames, st.nblocks, fault)), (fault, name)


# ---- constants ------------------------------------------------------------------------------------------------------------------
def test_the_models_constants_are_the_kernels():
    src = open(SOURCE).read()

    def one(pattern):
        found = re.findall(pattern, src)
        assert len(found) == 1, (pattern, found)
        return found[0]

    assert int(one(r"constexpr int T_NF = (\d+);")) == P.T_NF
    assert one(r"constexpr int T_CODE = (\d+) \* 1024;") == str(P.T_CODE // 1024)
    assert int(one(r"constexpr int T_SLACK = (\d+);")) == P.T_SLACK
    assert int(one(r"constexpr int TW = (\d+);")) * 64 == P.WG
    one(r"if \(used \+ need > \(uint32_t\)T_CODE && kept > 0\) break;")
    one(r"used = \(used \+ need \+ T_SLACK \+ 15u\) & ~15u;")
    one(r"lo = min\(lo, dd\[k\]\); hi = max\(hi, dd\[k\] \+ 18u\);")


def table():
    lines = ["clips a faulty walk gets wrong (buffers + flags wrong; 0 = the clip lets the mistake through):", ""]
    for fault in P.FAULTS:
        hits = [(n, wrong(n, fault)) for n in NAMES if K.by_name(n).kernel == "msv1_blocks_temporal_kernel"]
        lines.append("  %-20s %s" % (fault, " ".join(f"{n}:{k}" for n, k in hits if k)))
    return "\n".join(lines)


if __name__ == "__main__":
    print(table())
