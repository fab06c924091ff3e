"""The directed key-frame clips (tests/msv1_keyframe_cut_clips.py), checked without a GPU: on every clip the plain-Python rule
(tests/index_keyframe_ref.py) is pinned to the oracle as in test_index_keyframe_ref_cpu.py, and gives every verdict the clip plans.
Then the conditions that keep test_index_keyframe_cuts_gpu.py honest: each is a property of the INPUTS, derived from the code lengths
in a comment, so that the GPU test cannot pass while leaving a case out."""
import numpy as np
import pytest

import index_keyframe_ref as kr
import msv1_keyframe_cut_clips as kc
from msv1_range_clips import POISON, coded_blocks, palette, truth_run
from oracle_binding import OracleMSVideo1

LINES = 36
_codes = {}


def covered(pic, w, h):
    return np.asarray(pic).reshape(h, w)[:4 * (h // 4), :4 * (w // 4)]


def codes_of(clip):
    """The reference's codes of every frame of a clip, worked out once."""
    key = (clip.name, clip.bits)
    if key not in _codes:
        _codes[key] = [kr.codes_of(clip.bits, clip.nbx, clip.nby, f) for f in clip.frames]
    return _codes[key]


def answers(clip, start):
    """key_frame of every frame of an index over frames[start:], a "cut" with its writer: bytes, ("none", b) or ("cut", b, writer)."""
    codes = codes_of(clip)[start:]
    out = []
    for t in range(len(codes)):
        a = kr.key_frame(clip.bits, clip.nbx, clip.nby, clip.frames[start:], t, codes)
        out.append(a + (kr.cut_writer(codes, t, a[1]),) if not isinstance(a, bytes) and a[0] == "cut" else a)
    return out


def verdict(a):
    return "bytes" if isinstance(a, bytes) else a


def all_clips():
    return [pytest.param(name, bits, id=f"{name}-{bits}") for name in kc.FAMILIES for bits in (16, 8)]


@pytest.mark.parametrize("name,bits", all_clips())
def test_the_reference_is_the_oracles_on_every_clip(name, bits):
    pal = palette(bits)
    for clip in kc.family(name, bits):
        w, h, nbx, nby = clip.w, clip.h, clip.nbx, clip.nby
        n = len(clip.frames)
        truth = truth_run(bits, w, h, pal, clip.frames, clip.keys, LINES, key_row=LINES)
        assert len(truth) == n and all(x is not None and x[0] is not None for x in truth), clip.name
        for i, c in enumerate(codes_of(clip)):   # the reference codes a block exactly where coded_blocks says so
            assert [x is not None for x in c] == list(coded_blocks(bits, nbx, nby, clip.frames[i])[0]), f"{clip.name} frame {i}"
        for start in clip.starts:
            got = answers(clip, start)
            for t, want in clip.planned(start).items():
                assert verdict(got[t]) == want, f"{clip.name} {bits}-bit start={start} t={t}"
            assert any(isinstance(a, bytes) for a in got), clip.name
            for t, kf in enumerate(got):
                if not isinstance(kf, bytes):
                    continue
                where = f"{clip.name} {bits}-bit start={start} t={t}"
                assert len(kf) % 2 == 0 and 2 * clip.nb <= len(kf) <= clip.nb * kc.LENGTH[bits]["eight"], where
                o = OracleMSVideo1(bits, w, h, pal)
                o.Preinit(LINES)
                assert o.IsKeyFrame(kf), where
                a = np.full(w * h, POISON, dtype=np.int32)
                assert o.DecompressI(kf, a) == 0, where
                assert np.array_equal(covered(a, w, h), covered(truth[start + t][0], w, h)), where
                nxt = start + t + 1
                if nxt < n:
                    b = a.copy()
                    if clip.keys[nxt]:
                        assert o.DecompressI(clip.frames[nxt], b) == 0, where
                    else:
                        o.DecompressP(clip.frames[nxt], b)
                    assert np.array_equal(covered(o.PreviousFrame(), w, h), covered(truth[nxt][0], w, h)), where + " and the frame after it"
                o.close()


@pytest.mark.parametrize("bits", [16, 8])
def test_ends_reaches_every_kind_and_cut_and_the_rules_verdict(bits):
    (clip,) = kc.family("ends", bits)
    nb = clip.nb
    assert nb == 12 and (nb // 1023) * 2 + 10 == 10          # the 16-bit early-out threshold of this picture
    middle, last = nb // 2 - 1, nb - 1
    # every (kind, d, p): d = 0 .. L bytes of each of the three kinds, at a middle block and at the last one
    seen = {(g["kind"], g["d"], g["p"]) for g in clip.groups if g["what"] == "cut"}
    assert seen == {(k, d, p) for k in kc.KINDS for d in range(kc.LENGTH[bits][k] + 1) for p in (middle, last)}
    assert {g["p"] for g in clip.groups if g["what"] == "skip"} == {middle, last} and sum(g["what"] == "solid0" for g in clip.groups) == 1
    codes = codes_of(clip)
    for start in clip.starts:
        got = answers(clip, start)
        for g in clip.groups:
            f0, p, d, L = g["first"] - start, g["p"], g["d"], g["L"]
            if f0 < 0:
                continue
            where = f"{bits}-bit start={start} group {g}"
            at = [verdict(got[f0 + k]) for k in range(3 if g["what"] == "solid0" else 4)]
            cut = ("cut", p, f0 + 1)
            if g["what"] == "cut" and d < L:
                # block p's code starts at o = e' - d, e' the frame's length.  d < 2: the code word is not below e.  2 <= d < L: o + L > e.
                # (16 bits, odd d: e = e' - 1, so o + 2 <= e fails at d = 1 and o + L <= e at the others; d = 2 of a 2- or 8-colour code:
                # the colour word at o + 2 is not below e.)  Frame 2 codes only the blocks behind p, frame 3 codes p whole.
                assert at == ["bytes", cut, cut, "bytes"], where
                o, e = sum(c[1] for c in codes[g["first"] + 1][:p]), len(clip.frames[g["first"] + 1])
                assert o == e - d
            elif g["what"] == "cut":
                # d == L: o + L == e and p is whole.  The blocks behind p lie wholly past the end: the first of them, p + 1, is cut —
                # or there is none.  Frame 2 codes them whole.
                assert codes[g["first"] + 1][p] == (len(clip.frames[g["first"] + 1]) - L, L), where
                assert at == ["bytes", "bytes" if p == last else ("cut", p + 1, f0 + 1), "bytes", "bytes"], where
            elif g["what"] == "skip":
                # two bytes, a skip code over blocks 0 .. p-1.  16 bits: shorter than 10 bytes and skip codes only, an early-out, no
                # block written.  8 bits: no early-out, blocks p .. are painted from missing bytes: o = 2 = e for block p.
                assert len(clip.frames[g["first"] + 1]) == 2
                assert at == (["bytes"] * 4 if bits == 16 else ["bytes", cut, cut, "bytes"]), where
            else:
                # one solid code for block 0: o = 0 = e - 2 is whole; block 1 has o = 2 = e.  Frame 2 codes 1 .. whole.
                assert codes[g["first"] + 1][0] == (0, 2) and len(clip.frames[g["first"] + 1]) == 2
                assert at == ["bytes", ("cut", 1, f0 + 1), "bytes"], where
    # the equalities of the rule are reached with a WHOLE code: o == e - 2 (solid), o == e - L; and o == e - 4 with a cut one
    # (16 bits, d = 4 of a 6- or 18-byte code: settled, not there)
    assert ("two", 4, middle) in seen and ("eight", 4, last) in seen


@pytest.mark.parametrize("bits", [16, 8])
def test_firsts_reaches_every_seam_with_both_kinds(bits):
    clips = {c.name: c for c in kc.family("firsts", bits)}
    assert clips["firsts_cut"].nb == kc.WG_BLOCKS + 1
    # a lane owns 4 consecutive blocks, a wave 64 lanes = 256 blocks, a workgroup 1024: P7 is both sides of each seam, and block 0
    assert set(kc.P7) == {0, 4 - 1, 4, 256 - 1, 256, 1024 - 1, 1024}
    # the lone cut at every p, one byte short of the end of p's code, until the group's last frame codes p: two refusals per p, both
    # naming the truncated frame (an index from frame 3 starts inside the group of p = 0)
    for start in (0, 3):
        got = [verdict(a) for a in answers(clips["firsts_cut"], start)]
        first = 1 if start else 0
        cuts = [a for a in got[first:] if a != "bytes"]
        assert cuts == [("cut", p, 4 * i + 1 - start) for i, p in enumerate(kc.P7) if i >= first for _ in range(2)]
    # the lone "no writer" at every p, and the pairs: "none" at p first, then — p coded — the cut at p + 1 with its writer, index frame 0
    for p in kc.P7:
        got = [verdict(a) for a in answers(clips[f"none_at_{p}"], 3)]
        assert got == [("none", p), ("none", p), "bytes"]
    assert set(kc.PAIRS) == {3, 4, 255, 256, 1023}       # across each seam, and the first block behind the lane and the wave seam
    for p in kc.PAIRS:
        clip = clips[f"pair_at_{p}"]
        got = [verdict(a) for a in answers(clip, 3)]
        assert got == [("none", p), ("none", p), ("cut", p + 1, 0), "bytes"]
        assert [verdict(a) for a in answers(clip, 0)][3:] == [("cut", p + 1, 3)] * 3 + ["bytes"]
        # both refuse at once at index frames 0 and 1: p has no writer, p + 1 has a cut one, and so has every block behind it —
        # a frame's end that cuts a code leaves every later block to missing bytes, so "cut" in front of "none" cannot be built
        codes = codes_of(clip)[3:]
        assert all(c[p] is None for c in codes[:2]) and codes[0][p + 1] == "cut"
        assert all(codes[0][b] == "cut" for b in range(p + 1, clip.nb))


def lo_of(bits, frames):
    return {16: [0, 4, 8, 12, 0, 4, 8, 12, 0], 8: [0, 2, 4, 6, 8, 10, 12, 14, 0]}[bits][:frames]


@pytest.mark.parametrize("bits", [16, 8])
def test_pieces_sweeps_both_ends_of_the_image(bits):
    eight, sweep, one_block, two_blocks = kc.family("pieces", bits)
    L = kc.LENGTH[bits]
    codes = codes_of(sweep)
    los, his, inside, across = [], set(), 0, 0
    for t in range(len(sweep.frames)):
        (lo0, hi0), (lo1, hi1) = kc.images(codes, t, sweep.nb)
        assert lo0 == 0 and hi1 - lo1 in L.values()
        los.append(lo1)
        his.add(hi1 % 16)
        inside += lo1 // 16 == (hi1 - 1) // 16
        across += lo1 // 16 != (hi1 - 1) // 16
    # Workgroup 1's base is the bytes of blocks 0 .. 1023: 1024 solid codes = 2048 = 0 mod 16, plus L(two) - L(solid) = 4 (8 bits: 2)
    # per block coded as a 2-colour code, k = 0 .. 8 of them behind each of the three key frames
    per_key = kc.SWEEP + 1
    assert los == lo_of(bits, per_key) * 3
    assert set(los) == ({0, 4, 8, 12} if bits == 16 else set(range(0, 16, 2)))
    # the last workgroup holds the last block alone, L = 2, 6, 18 (2, 4, 10) by the key frame's kind: hi % 16 = lo + L mod 16.
    # 16 bits: lo = 0 mod 4 and L = 2 mod 4 give {2, 6, 10, 14}, each reached (L = 2 at the four lo).  8 bits: lo runs over every
    # even residue, so hi % 16 does too — 0 included (lo = 14, L = 2): the image ends on a piece's end
    assert his == ({2, 6, 10, 14} if bits == 16 else set(range(0, 16, 2)))
    # lo + L <= 16 lies inside one piece (L = 2 at every lo), lo + L > 16 in two (the 8-colour code at every lo but, 8 bits, 0 .. 6)
    assert inside > 0 and across > 0
    # the single 8-colour code at p shifts every block behind p by L(eight) - L(solid): frame 1 + i has it at P7[i] alone
    codes = codes_of(eight)
    for i, p in enumerate(kc.P7):
        lens = [codes[kr.cut_writer(codes, 1 + i, b)][b][1] for b in range(eight.nb)]
        assert lens == [L["solid"]] * p + [L["eight"]] + [L["solid"]] * (eight.nb - p - 1)
    # whole frames smaller than a 16-byte piece: at most 10 bytes (8 bits), and 2 .. 6 or 18 > 16 at 16 bits
    assert (one_block.nb, two_blocks.nb) == (1, 2)
    sizes = {len(a) for c in (one_block, two_blocks) for a in answers(c, 0)}
    assert all(isinstance(a, bytes) for c in (one_block, two_blocks) for a in answers(c, 0)) and min(sizes) == 2 and any(s < 16 for s in sizes)


@pytest.mark.parametrize("bits", [16, 8])
def test_gaps_lie_between_a_writer_and_t(bits):
    (clip,) = kc.family("gaps", bits)
    codes = codes_of(clip)
    assert len(clip.gap_frames) >= 8
    spread, marked = 0, 0
    for f in clip.gap_frames:
        coded = [b for b, c in enumerate(codes[f]) if c is not None]
        stop = coded_blocks(bits, clip.nbx, clip.nby, clip.frames[f])[1]
        if coded:   # (8 bits) an end marker in the middle: codes in front of it only, and the blocks behind keep their writers
            assert bits == 8 and stop is not None and 0 < max(coded) < stop < clip.nb
            marked += 1
        writers = [kr.cut_writer(codes, f, b) for b in range(clip.nb)]
        behind = writers if stop is None else writers[stop:]
        assert all(w < f for w in behind)
        assert len(set(writers)) >= 3, f"frame {f}: neighbouring blocks have writers in different frames"
        spread += len({w // kc.CHUNK for w in writers}) > 1     # ... and in different chunks of CHUNK frames
    assert spread > 0 and marked == (2 if bits == 8 else 0)
    if bits == 16:   # an empty frame, a short one of skip codes only, and an all-skip frame long enough to be parsed
        assert {len(clip.frames[f]) for f in clip.gap_frames} == {0, 2, 10}
        for f in clip.gap_frames:
            assert coded_blocks(16, clip.nbx, clip.nby, clip.frames[f])[2] == (len(clip.frames[f]) < 10), f"frame {f}: an early-out below 10 bytes"
    assert all(isinstance(a, bytes) for a in answers(clip, 0))
