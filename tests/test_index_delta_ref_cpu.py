"""The inter frame that spans a gap of a seek index, checked without a GPU: the plain-Python statement of the rule
(tests/index_delta_ref.py) is pinned to the oracle.  The oracle decodes frames 0 .. a of a clip, then Delta(a, b) as an inter frame on
top: the result is its own sequential picture of frame b on every pixel a block covers.  Then the structure of the bytes, the exact
values the rule promises, and three deliberately wrong variants of the rule, each failing on a directed clip.  Nothing of the GPU is
involved."""
import numpy as np
import pytest

import index_delta_ref as dr
import index_keyframe_ref as kr
import msv1_delta_clips as dc
import msv1_keyframe_cut_clips as kc
from msv1_range_clips import POISON, coded_blocks, long_clip, palette, truth_run
from oracle_binding import OracleMSVideo1

LINES = 36


def covered(pic, w, h):
    return np.asarray(pic).reshape(h, w)[:4 * (h // 4), :4 * (w // 4)]


def sample(n, first=-1, every=300):
    """Every pair (a, b] of n frames while there are at most `every`; else the gaps of 1 and 2 frames everywhere, and gaps of 5, 17
    and 40 frames from every 7th frame."""
    pairs = dc.pairs(n, first)
    if len(pairs) <= every:
        return pairs
    return [(a, b) for a, b in pairs if b - a <= 2 or ((a + 1) % 7 == 0 and b - a in (5, 17, 40))]


def oracle_at(bits, w, h, pal, frames, keys, upto, lines=LINES):
    """An oracle that has decoded frames 0 .. upto one by one."""
    o = OracleMSVideo1(bits, w, h, pal)
    o.Preinit(lines)
    bufs = [np.full(w * h, POISON, dtype=np.int32) for _ in range(2)]
    for i in range(upto + 1):
        prev = o.PreviousFrame()
        dst = next(b for b in bufs if b is not prev)
        if prev is not None:
            np.copyto(dst, prev)
        if keys[i]:
            assert o.DecompressI(frames[i], dst) == 0
        else:
            o.DecompressP(frames[i], dst)
    return o


def structure(bits, nb, data, written, where):
    """Codes on exactly the written blocks, skips and codes cover nb exactly, no skip word crosses a multiple of 1023, every skip
    word stands at a run head."""
    codes, skips, blocks = dr.walk(bits, data)
    assert [c[0] for c in codes] == written, where
    assert blocks == nb, where
    ws = set(written)
    for at, count in skips:
        assert 1 <= count <= dr.RUN and at // dr.RUN == (at + count - 1) // dr.RUN, (where, at, count)
        assert at == 0 or at % dr.RUN == 0 or at - 1 in ws, (where, at)
        assert at + count == nb or (at + count) % dr.RUN == 0 or at + count in ws, (where, at, count)


def check_clip(bits, w, h, pal, frames, keys, start, pairs, lines=LINES, truth=None, chains=True):
    """Delta of every pair of an index over frames[start:], against the oracle.  Returns (bytes by pair, refusals by pair)."""
    nbx, nby = w // 4, h // 4
    nb = nbx * nby
    truth = truth or truth_run(bits, w, h, pal, frames, keys, lines, key_row=lines)
    rng = frames[start:]
    codes = [kr.codes_of(bits, nbx, nby, f) for f in rng]
    got, refused = {}, {}
    by_a = {}
    for a, b in pairs:
        by_a.setdefault(a, []).append(b)
    for a in sorted(by_a):
        base = start + a
        o = oracle_at(bits, w, h, pal, frames, keys, base, lines) if base >= 0 else None
        for b in by_a[a]:
            where = f"{bits}-bit {w}x{h} start={start} ({a}, {b}]"
            d = dr.delta(bits, nbx, nby, rng, a, b, codes)
            written = [i for i in range(nb) if dr.writer(codes, a, b, i) is not None]
            if not isinstance(d, bytes):
                assert d[0] == "cut" and d[1] in written and codes[dr.writer(codes, a, b, d[1])][d[1]] == "cut", where
                assert all(codes[dr.writer(codes, a, b, i)][i] != "cut" for i in written if i < d[1]), where
                refused[(a, b)] = d
                continue
            got[(a, b)] = d
            structure(bits, nb, d, written, where)
            # codes_of, the decoder's own control flow, codes exactly the written set (16 bits: unless it takes the early-out)
            parsed = kr.codes_of(bits, nbx, nby, d)
            early = bits == 16 and coded_blocks(16, nbx, nby, d)[2]
            assert [i for i, c in enumerate(parsed) if c is not None] == ([] if early else written), where
            assert not early or not written, where
            assert all(c != "cut" for c in parsed), where
            kf = kr.key_frame(bits, nbx, nby, rng, b, codes)
            if isinstance(kf, bytes):
                assert len(d) <= len(kf), where
            if a == -1 and len(written) == nb:
                assert d == kf, where
            if o is None:   # no picture before the index: the frame decodes only where it writes everything
                if len(written) == nb:
                    k = OracleMSVideo1(bits, w, h, pal)
                    k.Preinit(lines)
                    assert k.IsKeyFrame(d), where
                    pic = np.full(w * h, POISON, dtype=np.int32)
                    assert k.DecompressI(d, pic) == 0, where
                    assert np.array_equal(covered(pic, w, h), covered(truth[start + b][0], w, h)), where
                    k.close()
                continue
            assert bool(o.IsKeyFrame(d)) == (len(written) == nb), where
            pic = np.array(truth[base][0], dtype=np.int32)
            o.DecompressP(d, pic)
            assert np.array_equal(covered(pic, w, h), covered(truth[start + b][0], w, h)), where
        if o is not None:
            o.close()
    if chains:   # Delta(a, b) then Delta(b, c) on a fresh oracle at a: the picture of c
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
    return got, refused


@pytest.mark.parametrize("bits", [16, 8])
@pytest.mark.parametrize("start", [0, 3])
def test_long_clip_deltas_decode_to_the_oracles_pictures(bits, start):
    w, h, n = 52, 28, 72
    frames, keys, pal, plan = long_clip(bits, w, h, seed=5, n=96)
    assert not plan["raises"]
    got, refused = check_clip(bits, w, h, pal, frames[:start + n], keys[:start + n], start, sample(n), plan["lines"])
    assert len(got) > 100
    assert bool(refused) == (bits == 16)      # the truncated 16-bit frames (31, 63) cut codes off; 8-bit end markers cut nothing
    assert any(b - a >= 17 for a, b in got)


@pytest.mark.parametrize("name", kc.FAMILIES)
@pytest.mark.parametrize("bits", [16, 8])
def test_key_frame_cut_clips_deltas_decode_to_the_oracles_pictures(name, bits):
    pal = palette(bits)
    cut = 0
    for clip in kc.family(name, bits):
        truth = truth_run(bits, clip.w, clip.h, pal, clip.frames, clip.keys, LINES, key_row=LINES)
        every = 300 if clip.nb <= 64 else 60
        for start in clip.starts:
            got, refused = check_clip(bits, clip.w, clip.h, pal, clip.frames, clip.keys, start, sample(len(clip.frames) - start, every=every),
                                      truth=truth)
            assert got, clip.name
            cut += len(refused)
    assert cut > 0 or name in ("pieces", "gaps")


@pytest.mark.parametrize("size", dc.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("bits", [16, 8])
def test_seam_clips_every_pair(bits, size):
    w, h = size
    clip = dc.seams(bits, w, h)
    nb = clip.nb
    assert nb == dc.NBLOCKS[dc.SIZES.index(size)]
    n = len(clip.frames)
    got, refused = check_clip(bits, w, h, palette(bits), clip.frames, clip.keys, 0, dc.pairs(n))
    assert not refused and len(got) == n * (n + 1) // 2
    at = {name: f for f, name in clip.patterns.items()}
    # a gap that writes nothing: ceil(nb / 1023) skip words, and at 16 bits the decoder's early-out takes it
    idle = got[(at["nothing"] - 1, at["nothing"])]
    words = -(-nb // dr.RUN)
    assert len(idle) == 2 * words
    assert dr.walk(bits, idle)[1] == [(k * dr.RUN, min(dr.RUN, nb - k * dr.RUN)) for k in range(words)]
    if bits == 16:
        assert len(idle) < (nb // 1023) * 2 + 10 and coded_blocks(16, clip.nbx, clip.nby, idle)[2]
    # a gap that writes everything: no skip word; from -1 it is the key frame, from anywhere its bytes
    codes = [kr.codes_of(bits, clip.nbx, clip.nby, f) for f in clip.frames]
    full = got[(at["every"] - 1, at["every"])]
    assert dr.walk(bits, full)[1] == [] and full == clip.frames[at["every"]]
    assert got[(-1, at["every"])] == kr.key_frame(bits, clip.nbx, clip.nby, clip.frames, at["every"], codes)
    assert got[(-1, 0)] == clip.frames[0]


@pytest.mark.parametrize("bits", [16, 8])
def test_the_runs_the_seam_clips_are_there_for(bits):
    """Properties of the INPUTS: each run the GPU test relies on exists in the reference's bytes."""
    def skips(w, h, name):
        clip = dc.seams(bits, w, h)
        f = next(f for f, n in clip.patterns.items() if n == name)
        codes = [kr.codes_of(bits, clip.nbx, clip.nby, x) for x in clip.frames]
        return dr.walk(bits, dr.delta(bits, clip.nbx, clip.nby, clip.frames, f - 1, f, codes))[1]

    assert skips(164, 100, "to_1023") == [(1000, 23)]                      # ends exactly at a multiple of 1023
    assert skips(164, 100, "to_wg") == [(1000, 23), (1023, 1)]              # ends exactly at a workgroup's end, 1023 inside it
    # from workgroup 0's last block across workgroup 1 into workgroup 2: the heads at 1023 and 2046 look two workgroups ahead
    assert skips(256, 256, "across") == [(1023, 1023), (2046, 1023), (3069, 3)]
    assert skips(128, 256, "across") == [(1023, 1023), (2046, 2)]           # ... and to the end of the picture: clipped by nblocks
    assert skips(124, 264, "across") == [(1023, 1023)]                      # nblocks itself a multiple of 1023
    assert skips(256, 256, "last") == [(0, 1023), (1023, 1023), (2046, 1023), (3069, 1023), (4092, 3)]
    assert skips(256, 256, "first") == [(1, 1022), (1023, 1023), (2046, 1023), (3069, 1023), (4092, 4)]
    assert skips(128, 256, "wg_first") == [(0, 1023), (1023, 1), (1025, 1021), (2046, 2)]
    assert skips(256, 256, "wg_first")[:5] == [(0, 1023), (1023, 1), (1025, 1021), (2046, 2), (2049, 1020)]
    assert skips(12, 8, "spots") == [(1, 2)] and skips(12, 8, "nothing") == [(0, 6)]
    singles = skips(128, 128, "singles")
    assert len(singles) == 512 and all(c == 1 for _, c in singles)
    # ... between codes of every pair of lengths
    clip = dc.seams(bits, 128, 128)
    f = next(f for f, n in clip.patterns.items() if n == "singles")
    lens = [c[1] if c else None for c in kr.codes_of(bits, clip.nbx, clip.nby, clip.frames[f])]
    around = {(lens[b - 1], lens[b + 1]) for b in range(1, clip.nb - 1, 2)}
    L = sorted(kc.LENGTH[bits].values())
    assert {x for x, _ in around} == set(L) == {y for _, y in around}, around
    spots = {at for at, _ in skips(256, 256, "spots")}
    assert {1, 5, 257, 1026, 2049} <= spots


# ---- the deliberately wrong variants: each differs from the rule, and fails a check the rule passes, on a directed clip ---------------
def wrong_on(bits, w, h, name, wrong):
    clip = dc.seams(bits, w, h)
    f = next(f for f, n in clip.patterns.items() if n == name)
    codes = [kr.codes_of(bits, clip.nbx, clip.nby, x) for x in clip.frames]
    right = dr.delta(bits, clip.nbx, clip.nby, clip.frames, f - 1, f, codes)
    bad = dr.delta(bits, clip.nbx, clip.nby, clip.frames, f - 1, f, codes, wrong=wrong)
    written = [i for i in range(clip.nb) if codes[f][i] is not None]
    structure(bits, clip.nb, right, written, "the rule")
    return clip, f, right, bad, written


@pytest.mark.parametrize("bits", [16, 8])
def test_wrong_chunks_counted_from_the_runs_start(bits):
    clip, f, right, bad, written = wrong_on(bits, 256, 256, "first", "chunks_from_run_start")
    assert bad != right and len(bad) < len(right) + 1
    assert dr.walk(bits, bad)[1][0] == (1, 1023)                 # crosses block 1023
    with pytest.raises(AssertionError):
        structure(bits, clip.nb, bad, written, "wrong")


@pytest.mark.parametrize("bits", [16, 8])
def test_wrong_count_not_clipped_at_nblocks(bits):
    clip, f, right, bad, written = wrong_on(bits, 164, 100, "first", "count_past_nblocks")
    assert bad != right and len(bad) == len(right)
    assert dr.walk(bits, bad)[2] == 2046 > clip.nb == 1025       # covers blocks the picture does not have
    with pytest.raises(AssertionError):
        structure(bits, clip.nb, bad, written, "wrong")


@pytest.mark.parametrize("bits", [16, 8])
def test_wrong_no_head_after_a_written_block(bits):
    """... and this one the oracle sees: the codes behind the missing skip word land on the wrong blocks."""
    w, h = 128, 128
    clip, f, right, bad, written = wrong_on(bits, w, h, "spots", "no_head_after_written")
    assert bad != right and len(bad) < len(right)
    with pytest.raises(AssertionError):
        structure(bits, clip.nb, bad, written, "wrong")
    pal = palette(bits)
    truth = truth_run(bits, w, h, pal, clip.frames, clip.keys, LINES, key_row=LINES)
    pics = []
    for data in (right, bad):
        o = oracle_at(bits, w, h, pal, clip.frames, clip.keys, f - 1)
        pic = np.array(truth[f - 1][0], dtype=np.int32)
        o.DecompressP(data, pic)
        pics.append(pic)
        o.close()
    assert np.array_equal(covered(pics[0], w, h), covered(truth[f][0], w, h))
    assert not np.array_equal(covered(pics[1], w, h), covered(truth[f][0], w, h))
