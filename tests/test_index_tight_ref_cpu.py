"""The TIGHT inter frame that spans a gap of a seek index, checked without a GPU: the plain-Python statement of the rule
(tests/index_tight_ref.py) is pinned to the oracle as test_index_delta_ref_cpu.py pins Delta's.  The oracle decodes frames 0 .. a of a
clip, then Tight(a, b) as an inter frame on top: the result is its own sequential picture of frame b on every pixel a block covers.
Minimality against the oracle's whole pictures: every kept block whose P(a) is defined differs between the oracle's pictures of a and
b, every dropped written block is equal in them.  Then the structure of the bytes with the kept set, the lengths and exact values the
rule promises, properties of the directed clips themselves, and four deliberately wrong variants of the rule, each failing on a
directed clip.  Nothing of the GPU is involved."""
import numpy as np
import pytest

import index_delta_ref as dr
import index_keyframe_ref as kr
import index_tight_ref as tr
import msv1_delta_clips as dc
import msv1_keyframe_cut_clips as kc
import msv1_tight_clips as tc
from msv1_range_clips import long_clip, palette, truth_run
from test_index_delta_ref_cpu import LINES, covered, oracle_at, sample, structure


def blocks_of(pic, w, h):
    """The covered part of a picture as (nblocks, 16) words."""
    c = covered(pic, w, h)
    return c.reshape(h // 4, 4, w // 4, 4).transpose(0, 2, 1, 3).reshape(-1, 16)


def check_clip(bits, w, h, pal, frames, keys, start, pairs, lines=LINES, truth=None, chains=True, decode=False):
    """Tight of every pair of an index over frames[start:], against the oracle.  decode: block pixels come from the per-block decode
    of pyref_msv1 (clips without a cut code), else from the oracle's whole pictures.  Returns (bytes by pair, refusals by pair,
    (written, kept) by pair)."""
    nbx, nby = w // 4, h // 4
    nb = nbx * nby
    truth = truth or truth_run(bits, w, h, pal, frames, keys, lines, key_row=lines)
    rng = frames[start:]
    codes = [kr.codes_of(bits, nbx, nby, f) for f in rng]
    before = truth[start - 1][0] if start > 0 else None
    px = tr.Pixels(bits, w, h, rng, codes, pal, before, None if decode else [t[0] for t in truth[start:]])
    blocks = {}

    def pic_blocks(t):   # the oracle's picture of index frame t (-1: the one before the index)
        if t not in blocks:
            blocks[t] = blocks_of(truth[start + t][0], w, h)
        return blocks[t]

    got, refused, sets = {}, {}, {}
    by_a = {}
    for a, b in pairs:
        by_a.setdefault(a, []).append(b)
    for a in sorted(by_a):
        base = start + a
        for b in by_a[a]:
            # (a fresh oracle per pair: it takes a skipped block from the last picture IT decoded, and a dropped block may have
            # looked different there)
            o = oracle_at(bits, w, h, pal, frames, keys, base, lines) if base >= 0 else None
            where = f"{bits}-bit {w}x{h} start={start} ({a}, {b}]"
            written, kept = sets[(a, b)] = tr.kept_set(px, a, b)
            t = tr.tight(px, a, b)
            d = dr.delta(bits, nbx, nby, rng, a, b, codes)
            # minimality, against the oracle's whole pictures
            ks = set(kept)
            assert ks <= set(written), where
            if base >= 0:
                differs = np.any(pic_blocks(a) != pic_blocks(b), axis=1)
                for i in written:
                    defined = start > 0 or dr.writer(codes, -1, a, i) is not None
                    if i in ks:
                        assert not defined or differs[i], f"{where}: block {i} is kept and did not change"
                    else:
                        assert defined and not differs[i], f"{where}: block {i} is dropped and changed"
            else:
                assert kept == written, where
            if o is not None and not isinstance(t, bytes):
                o.close()
            if not isinstance(t, bytes):
                assert t[0] == "cut" and t[1] in ks and codes[dr.writer(codes, a, b, t[1])][t[1]] == "cut", where
                assert all(codes[dr.writer(codes, a, b, i)][i] != "cut" for i in kept if i < t[1]), where
                assert not isinstance(d, bytes), where          # (a kept block is a written one: Delta refuses too, maybe earlier)
                refused[(a, b)] = t
                continue
            got[(a, b)] = t
            structure(bits, nb, t, kept, where)
            if isinstance(d, bytes):
                assert len(t) <= len(d), where
                assert (t == d) == (kept == written), where
            if o is None:   # no picture before the index: nothing is defined, nothing is dropped
                assert t == d, where
                continue
            assert bool(o.IsKeyFrame(t)) == (len(kept) == nb), where
            pic = np.array(truth[base][0], dtype=np.int32)
            o.DecompressP(t, pic)
            assert np.array_equal(covered(pic, w, h), covered(truth[start + b][0], w, h)), where
            o.close()
            if not differs.any():
                assert len(t) == 2 * -(-nb // dr.RUN) and not kept, where
    if chains:   # Tight(a, b) then Tight(b, c) on a fresh oracle at a: the picture of c
        done = 0
        for (a, b), d1 in got.items():
            nxt = next((c for (b2, c) in got if b2 == b and c > b), None)
            if nxt is None or start + a < 0 or done >= 12:
                continue
            done += 1
            o = oracle_at(bits, w, h, pal, frames, keys, start + a, lines)
            pic = np.array(truth[start + a][0], dtype=np.int32)
            o.DecompressP(d1, pic)
            pic2 = pic.copy()
            o.DecompressP(got[(b, nxt)], pic2)
            assert np.array_equal(covered(pic2, w, h), covered(truth[start + nxt][0], w, h)), f"{bits}-bit start={start} chain {a}->{b}->{nxt}"
            o.close()
        assert done > 0 or len(got) < 3
    return got, refused, sets


@pytest.mark.parametrize("bits", [16, 8])
@pytest.mark.parametrize("start", [0, 3])
def test_long_clip_tight_frames_decode_to_the_oracles_pictures(bits, start):
    w, h, n = 52, 28, 72
    frames, keys, pal, plan = long_clip(bits, w, h, seed=5, n=96)
    assert not plan["raises"]
    got, refused, sets = check_clip(bits, w, h, pal, frames[:start + n], keys[:start + n], start, sample(n), plan["lines"])
    assert len(got) > 100 and any(b - a >= 17 for a, b in got)
    assert any(len(k) < len(wr) for wr, k in sets.values())          # the clip repaints blocks with what they show: some are dropped


@pytest.mark.parametrize("name", kc.FAMILIES)
@pytest.mark.parametrize("bits", [16, 8])
def test_key_frame_cut_clips_tight_frames_decode_to_the_oracles_pictures(name, bits):
    pal = palette(bits)
    for clip in kc.family(name, bits):
        truth = truth_run(bits, clip.w, clip.h, pal, clip.frames, clip.keys, LINES, key_row=LINES)
        every = 300 if clip.nb <= 64 else 60
        for start in clip.starts:
            got, refused, _ = check_clip(bits, clip.w, clip.h, pal, clip.frames, clip.keys, start,
                                         sample(len(clip.frames) - start, every=every), truth=truth)
            assert got, clip.name


@pytest.mark.parametrize("size", [(164, 100), (128, 256), (12, 8)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("bits", [16, 8])
def test_delta_seam_clips_every_pair(bits, size):
    """Every frame of these clips gives every block it writes a new colour: Tight differs from Delta only where a random colour
    repeats (check_clip holds t == d to kept == written)."""
    clip = dc.seams(bits, *size)
    n = len(clip.frames)
    got, refused, _ = check_clip(bits, clip.w, clip.h, palette(bits), clip.frames, clip.keys, 0, dc.pairs(n), decode=True)
    assert not refused and len(got) == n * (n + 1) // 2


@pytest.mark.parametrize("size", tc.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("bits", [16, 8])
@pytest.mark.parametrize("start", [0, 3])
def test_directed_clips_every_pair(bits, size, start):
    w, h = size
    clip = tc.directed(bits, w, h)
    nb, S = clip.nb, clip.spots
    assert nb == tc.NBLOCKS[tc.SIZES.index(size)]
    n = len(clip.frames) - start
    got, refused, sets = check_clip(bits, w, h, palette(bits), clip.frames, clip.keys, start, dc.pairs(n), decode=True)
    assert not refused and len(got) == n * (n + 1) // 2
    words = -(-nb // dr.RUN)
    codes = [kr.codes_of(bits, clip.nbx, clip.nby, f) for f in clip.frames[start:]]

    def at(a, b):   # by the clip's frame numbers
        return a - start, b - start

    def delta(a, b):
        return dr.delta(bits, clip.nbx, clip.nby, clip.frames[start:], *at(a, b), codes)

    if start == 0:
        # recode_all: nothing but skip words where Delta is as long as the frame, which codes every block
        assert got[at(0, 1)] == b"".join(dr.skip_word(min(dr.RUN, nb - k * dr.RUN)) for k in range(words))
        assert delta(0, 1) == clip.frames[1] and len(clip.frames[1]) > 2 * nb
        assert got[(-1, 0)] == clip.frames[0] == delta(-1, 0)
        # back: Tight(1, 4) drops S; Tight(2, 4) keeps it
        assert sets[at(1, 4)] == (sorted(set(S) | set(clip.next_blocks) | set(clip.after)), sorted(set(clip.next_blocks) - set(S)))
        assert set(S) <= set(sets[at(2, 4)][1])
    assert set(S) <= set(sets[at(3, 4)][1])
    # one_pixel: every one of the 16 blocks is kept
    assert sets[at(4, 5)] == (clip.pixel_blocks, clip.pixel_blocks)
    # key_same: all skips, no key frame, though the frame codes every block; every pair that spans it is shorter than Delta
    assert got[at(5, 6)] == got[at(0 if start == 0 else 5, 1 if start == 0 else 6)] and len(got[at(5, 6)]) == 2 * words
    assert sets[at(5, 6)] == (list(range(nb)), []) and len(delta(5, 6)) == len(clip.frames[6])
    assert (len(got[at(4, 6)]) < len(delta(4, 6)) or nb <= 16) and sets[at(4, 6)][1] == clip.pixel_blocks
    # every: Tight = Delta = the frame's own bytes
    assert got[at(6, 7)] == delta(6, 7) == clip.frames[7]
    assert got[at(3, 7)] == clip.frames[7]


@pytest.mark.parametrize("bits", [16, 8])
def test_the_seams_the_directed_clips_are_there_for(bits):
    """Properties of the INPUTS: a dropped block directly before a kept one on every seam, and dropped blocks next to each other."""
    pal = palette(bits)
    seen3, seen8 = set(), set()
    for w, h in tc.SIZES:
        clip = tc.directed(bits, w, h)
        codes = [kr.codes_of(bits, clip.nbx, clip.nby, f) for f in clip.frames]
        px = tr.Pixels(bits, w, h, clip.frames, codes, pal)
        for (a, b), seams, seen in (((2, 3), tc.SEAMS_3, seen3), ((7, 8), tc.SEAMS_8, seen8)):
            written, kept = tr.kept_set(px, a, b)
            for d, k in seams:
                if k < clip.nb:
                    assert d in written and d not in kept and k in kept, (w, h, a, b, d, k)
                    seen.add((d, k))
        written, kept = tr.kept_set(px, 2, 3)
        for s in clip.after:   # dropped behind a kept block ...
            assert s in written and s not in kept and s - 1 in kept, (w, h, s)
        assert clip.nb <= 16 or any(s + 1 not in written for s in clip.after), (w, h)   # ... an unwritten block behind it
        written, kept = tr.kept_set(px, 1, 4)
        if clip.nb > 1024:     # the lane that looks at blk0 - 1 = 1023 for the workgroup's first block: written, not kept
            assert 1023 in written and 1023 not in kept and 1024 not in kept
    assert seen3 == set(tc.SEAMS_3) and seen8 >= set(tc.SEAMS_8[:4])
    assert {(3, 4), (255, 256), (1023, 1024), (1022, 1023), (2045, 2046)} <= seen3 | seen8


def test_two_palette_indices_of_one_colour_are_equal():
    clip, pal = tc.twins()
    got, refused, sets = check_clip(8, clip.w, clip.h, pal, clip.frames, clip.keys, 0, dc.pairs(3), decode=True)
    assert not refused
    assert sets[(0, 1)] == ([2, 4], [4]) and sets[(1, 2)] == ([2], []) and sets[(0, 2)] == ([2, 4], [4])
    assert got[(1, 2)] == dr.skip_word(clip.nb)
    assert clip.frames[0][4:6] != clip.frames[1][2:4]               # other bytes for block 2 ...
    ints = tr.pyref.palette_ints(pal)
    assert ints[tc.TWINS[0]] == ints[tc.TWINS[1]]                   # ... the same word


@pytest.mark.parametrize("size", tc.CUT_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("bits", [16, 8])
def test_a_dropped_block_with_a_cut_code_does_not_refuse(bits, size):
    clip = tc.cut_dropped(bits, *size)
    nb, last = clip.nb, clip.last
    codes = [kr.codes_of(bits, clip.nbx, clip.nby, f) for f in clip.frames]
    assert codes[1][last] == "cut" and all(c not in (None, "cut") for c in codes[1][:last])
    got, refused, sets = check_clip(bits, clip.w, clip.h, palette(bits), clip.frames, clip.keys, 0, dc.pairs(3))
    # with no picture before the index nothing is defined at a = -1: the block is kept there, and refuses
    assert refused == {(-1, 1): ("cut", last), (-1, 2): ("cut", last)}
    for b in (1, 2):
        assert dr.delta(bits, clip.nbx, clip.nby, clip.frames, 0, b, codes) == ("cut", last)       # Delta refuses the pair
        assert sets[(0, b)] == (list(range(nb)), list(range(last)))                                # Tight drops the block
        assert got[(0, b)][-2:] == dr.skip_word(1)
    assert got[(0, 1)] == clip.frames[1][:-1] + dr.skip_word(1)


# ---- the deliberately wrong variants: each differs from the rule, and fails a check the rule passes, on a directed clip --------------
def rule_and_wrong(bits, clip, pal, a, b, wrong, pictures=False):
    codes = [kr.codes_of(bits, clip.nbx, clip.nby, f) for f in clip.frames]
    truth = truth_run(bits, clip.w, clip.h, pal, clip.frames, clip.keys, LINES, key_row=LINES)
    px = tr.Pixels(bits, clip.w, clip.h, clip.frames, codes, pal, None, [t[0] for t in truth] if pictures else None)
    return truth, px, tr.tight(px, a, b), tr.tight(px, a, b, wrong=wrong)


def decodes_to(bits, clip, pal, truth, a, b, data):
    o = oracle_at(bits, clip.w, clip.h, pal, clip.frames, clip.keys, a)
    pic = np.array(truth[a][0], dtype=np.int32)
    o.DecompressP(data, pic)
    o.close()
    return np.array_equal(covered(pic, clip.w, clip.h), covered(truth[b][0], clip.w, clip.h))


@pytest.mark.parametrize("bits", [16, 8])
def test_wrong_first_pixel_only(bits):
    """one_pixel: block k changes in pixel k; a compare of word 0 alone keeps the first block only."""
    clip, pal = tc.directed(bits, 164, 100), palette(bits)
    truth, px, right, bad = rule_and_wrong(bits, clip, pal, 4, 5, "first_pixel_only")
    assert tr.kept_set(px, 4, 5, "first_pixel_only")[1] == clip.pixel_blocks[:1]
    assert bad != right and len(bad) < len(right)
    assert decodes_to(bits, clip, pal, truth, 4, 5, right) and not decodes_to(bits, clip, pal, truth, 4, 5, bad)


@pytest.mark.parametrize("bits", [16, 8])
@pytest.mark.parametrize("pair", [(2, 3), (1, 4)])
def test_wrong_neighbour_written(bits, pair):
    """recode_next: an unwritten block behind a dropped one is no run head — the run began at the dropped block or before it.  With
    "written" for "kept" it gets a skip word of its own, and the frame covers more blocks than the picture has."""
    clip, pal = tc.directed(bits, 164, 100), palette(bits)
    truth, px, right, bad = rule_and_wrong(bits, clip, pal, *pair, "neighbour_written")
    kept = tr.kept_set(px, *pair)[1]
    structure(bits, clip.nb, right, kept, "the rule")
    assert bad != right and len(bad) > len(right)
    assert dr.walk(bits, bad)[2] > clip.nb
    with pytest.raises(AssertionError):
        structure(bits, clip.nb, bad, kept, "wrong")
    assert decodes_to(bits, clip, pal, truth, *pair, right) and not decodes_to(bits, clip, pal, truth, *pair, bad)


@pytest.mark.parametrize("bits", [16, 8])
def test_wrong_bytes_not_pixels(bits):
    """recode_all: other bytes, the same pixels.  Comparing bytes keeps blocks that the oracle's pictures show unchanged."""
    clip, pal = tc.directed(bits, 128, 128), palette(bits)
    truth, px, right, bad = rule_and_wrong(bits, clip, pal, 0, 1, "bytes_not_pixels")
    kept = tr.kept_set(px, 0, 1, "bytes_not_pixels")[1]
    assert tr.kept_set(px, 0, 1)[1] == [] and len(kept) > clip.nb // 2 and len(bad) > 100 * len(right)
    same = ~np.any(blocks_of(truth[0][0], clip.w, clip.h) != blocks_of(truth[1][0], clip.w, clip.h), axis=1)
    assert same.all() and kept                                        # minimality: a kept block that did not change
    assert decodes_to(bits, clip, pal, truth, 0, 1, bad)              # (the picture is right all the same: only minimality sees it)


@pytest.mark.parametrize("bits", [16, 8])
def test_wrong_dropped_refuses(bits):
    clip, pal = tc.cut_dropped(bits, 24, 8), palette(bits)
    truth, px, right, bad = rule_and_wrong(bits, clip, pal, 0, 1, "dropped_refuses", pictures=True)
    assert isinstance(right, bytes) and bad == ("cut", clip.last)
    assert decodes_to(bits, clip, pal, truth, 0, 1, right)
