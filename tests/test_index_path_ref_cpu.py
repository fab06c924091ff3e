"""The frames of a block rectangle along any path through a seek index, checked without a GPU: the plain-Python statement of the rule
(tests/index_path_ref.py) is pinned to the oracle.  The oracle decodes the source clip; an oracle of the rectangle's size, 4 bw x 4 bh,
decodes a key pair's frame and then the frames of chained pairs — steps back, holds, steps forward: after each it holds the
sub-rectangle of the source's picture.  Then the identity with index_crop_ref for key and forward pairs, the refusals, four
deliberately wrong variants of the rule, each failing on a named clip.  Nothing of the GPU is involved."""
import numpy as np
import pytest

import index_crop_ref as cr
import index_delta_ref as dr
import index_path_ref as pr
import msv1_crop_clips as cc
from test_index_crop_ref_cpu import Small, source
from test_index_delta_ref_cpu import structure

KEY = pr.KEY


def made(s, rect, pair, tight=False, wrong=None):
    """index_path_ref.path of a Source (test_index_crop_ref_cpu), worked out once."""
    k = ("path", rect, pair, tight, wrong)
    if k not in s._made:
        s._made[k] = pr.path(s.bits, cc.NBX, s.range, rect, pair, s.codes, tight, s.px, wrong)
    return s._made[k]


def back_pairs(n):
    """The BACK pairs asked of a clip of n frames: one, two and three frames back to every frame, and from the last to the first."""
    out = [(b + d, b) for b in range(n) for d in (1, 2, 3) if b + d < n]
    return out + [(n - 1, 0)]


def hold_pairs(n):
    return [(t, t) for t in range(n)]


def chains(n):
    """Orders of frames: descending with stride 1 and stride 3 from n - 1, and a boomerang 0 -> n - 1 -> 0 with stride 2."""
    up = list(range(0, n, 2))
    if up[-1] != n - 1:
        up.append(n - 1)
    return [list(range(n - 1, -1, -1)), list(range(n - 1, -1, -3)), up + up[-2::-1]]


def kept_by_the_pictures(s, rect, pair, tight):
    """The blocks j a pair keeps, from the source's tables and the ORACLE's pictures alone: coded by a frame of (lo, hi], and with
    tight different in the pictures of a and b (both defined: the clip has a picture before the index, or frame 0 codes every block)."""
    a, b = pair
    lo, hi = min(a, b), max(a, b)
    out = []
    for j, blk in enumerate(cc.blocks_of(rect)):
        if not any(s.codes[f][blk] is not None for f in range(lo + 1, hi + 1)):
            continue
        if tight:
            y, x = 4 * (blk // cc.NBX), 4 * (blk % cc.NBX)
            if np.array_equal(s.pictures[a][y:y + 4, x:x + 4], s.pictures[b][y:y + 4, x:x + 4]):
                continue
        out.append(j)
    return out


def fails(s, rect, pair, data, tight=False):
    """Whether `data` is NOT a frame the rule promises for a pair with from >= 0: a refusal where the right rule has none (or the
    reverse), bytes that break the structure of a frame of nb blocks, or bytes that do not take the rectangle from the source's
    picture of `from` to that of `to`."""
    right = made(s, rect, pair, tight)
    if not isinstance(data, bytes) or not isinstance(right, bytes):
        return data != right
    a, b = pair
    try:
        structure(s.bits, rect[2] * rect[3], data, kept_by_the_pictures(s, rect, pair, tight), "")
    except AssertionError:
        return True
    before = s.crop(rect, (KEY, a))
    if not isinstance(before, bytes):   # (no key frame to decode on top of: the structure is all that can be seen)
        return False
    small = Small(s, rect)
    try:
        small.key(before)
        return not np.array_equal(small.inter(data), s.sub(rect, b))
    finally:
        small.close()


@pytest.mark.parametrize("bits", [16, 8])
@pytest.mark.parametrize("rect", cc.RECTS, ids=cc.rect_id)
def test_steps_back_holds_and_chains_decode_to_the_sub_rectangle_of_the_oracles_pictures(bits, rect):
    s = source(cc.seams(bits, rect))
    nb = rect[2] * rect[3]
    pairs = back_pairs(s.n) + hold_pairs(s.n)
    for tight in (False, True):
        for pair in pairs:
            data = made(s, rect, pair, tight)
            assert isinstance(data, bytes), (rect, pair, tight, data)     # frame 0 codes every block: no step back refuses
            assert len(data) <= nb * (18 if bits == 16 else 10)
            assert len(data) <= len(made(s, rect, pair, False))
            if tight and pair[0] - pair[1] != 1:                           # (tight: the neighbours, as the crop test samples them)
                continue
            assert not fails(s, rect, pair, data, tight), (s.clip.name, bits, rect, pair, tight)
    for t in range(s.n):
        assert made(s, rect, (t, t)) == made(s, rect, (t, t), True) == pr.hold(nb)
    for f in range(1, s.n):   # Back(f, f - 1) and Delta(f - 1, f) touch the same blocks: the same skip words
        assert dr.walk(bits, made(s, rect, (f, f - 1)))[1] == dr.walk(bits, s.crop(rect, (f - 1, f)))[1], (rect, f)
        assert [c[0] for c in dr.walk(bits, made(s, rect, (f, f - 1)))[0]] == [c[0] for c in dr.walk(bits, s.crop(rect, (f - 1, f)))[0]]
    for order in chains(s.n):
        for tight in (False, True):
            small = Small(s, rect)
            assert np.array_equal(small.key(made(s, rect, (KEY, order[0]), tight)), s.sub(rect, order[0]))
            for a, b in zip(order, order[1:]):
                data = made(s, rect, (a, b), tight)
                assert np.array_equal(small.inter(data), s.sub(rect, b)), (s.clip.name, rect, a, b, tight)
                assert bool(small.o.IsKeyFrame(data)) == cr.flag(bits, data, nb) == (len(kept_by_the_pictures(s, rect, (a, b), tight)) == nb)
            small.close()


@pytest.mark.parametrize("bits", [16, 8])
def test_the_tight_clip_in_every_order_of_two_frames(bits):
    clip = cc.tight(bits)
    s, rect = source(clip), clip.rect
    shorter = 0
    for a in range(s.n):
        for b in range(s.n):
            if a == b:
                continue
            tight, loose = made(s, rect, (a, b), True), made(s, rect, (a, b), False)
            assert isinstance(tight, bytes) and isinstance(loose, bytes) and len(tight) <= len(loose), (a, b)
            shorter += len(tight) < len(loose)
            if abs(a - b) <= 2 or (a, b) in ((s.n - 1, 0), (4, 1), (1, 4)):
                assert not fails(s, rect, (a, b), tight, True), (bits, a, b)
                assert not fails(s, rect, (a, b), loose, False), (bits, a, b)
    assert shorter > 5
    # frame 1 recodes what frame 0 shows: back over it is all skips, as forward is; frame 4 takes the spots back to frame 1, so
    # a step from 4 back to 1 drops them
    assert made(s, rect, (1, 0), True) == pr.hold(rect[2] * rect[3]) == made(s, rect, (0, 1), True)
    spots = set(clip.inner.spots)
    assert spots <= {j for j, _ in pr.kept(cc.NBX, rect, (4, 1), s.codes)}
    assert not spots & {j for j, _ in pr.kept(cc.NBX, rect, (4, 1), s.codes, True, s.px)}


@pytest.mark.parametrize("bits", [16, 8])
def test_key_and_forward_pairs_are_index_crop_ref(bits):
    for clip, rect, start in ((cc.seams(bits, (5, 3, 37, 31)), (5, 3, 37, 31), 0), (cc.seams(bits, (3, 2, 3, 2)), (3, 2, 3, 2), 0),
                              (cc.tight(bits), cc.TIGHT_RECT, 0), (cc.cuts(bits), cc.REFUSAL_RECT, 0),
                              (cc.nones(bits), cc.REFUSAL_RECT, cc.NONES_START)):
        s = source(clip, start)
        pairs = cc.pairs(min(s.n, 12))
        for tight in (False, True):
            for p in pairs[::1 if s.n < 12 else 3]:
                assert made(s, rect, p, tight) == s.crop(rect, p, tight), (clip.name, p, tight)


@pytest.mark.parametrize("bits", [16, 8])
def test_a_step_back_refuses_at_every_listed_block_and_nowhere_outside(bits):
    rect = cc.REFUSAL_RECT
    nb = rect[2] * rect[3]
    clip = cc.cuts(bits)
    s = source(clip)
    assert [j for _, _, j in clip.groups] == [0, 3, 4, 255, 256, 1023, 1024, nb - 1, None, None]
    for first, p, j in clip.groups:
        # frame first + 3 codes block p alone; its last writer before that is frame first + 1, whose code of it is cut off
        for pair in ((first + 3, first + 2), (first + 3, first + 1)):
            if j is None:   # (back to frame first + 1 the window holds frame first + 2, which codes every block behind p, and
                # the end of frame first + 1's data cuts those as well: only the step over frame first + 3 alone is asked)
                assert pair[1] != first + 2 or isinstance(made(s, rect, pair), bytes), (p, pair)
            else:
                assert made(s, rect, pair) == ("cut", j), (j, pair)
                assert pr.writer(s.codes, cc.NBX, rect, pair, j) == first + 1
        assert isinstance(made(s, rect, (first + 3, first)), bytes)       # (back to the group's key frame: whole codes)
        assert not fails(s, rect, (first + 3, first), made(s, rect, (first + 3, first)))
    clip = cc.nones(bits)
    s = source(clip, cc.NONES_START)
    assert clip.at == [0, 3, 4, 255, 256, 1023, 1024, nb - 1] and s.n == 1 + len(clip.at)
    for k, j in enumerate(clip.at):
        # index frame k + 1 codes src(j) alone, and nothing up to frame k does: the picture before the index shows there
        assert made(s, rect, (k + 1, k)) == ("none", j) == made(s, rect, (k + 1, k), True), (k, j)
        assert isinstance(made(s, rect, (k, k + 1)), bytes) and not fails(s, rect, (k, k + 1), made(s, rect, (k, k + 1)))
        assert made(s, rect, (s.n - 1, k)) == ("none", j)                 # (further back: the FIRST block without a writer)
        assert made(s, rect, (k, k)) == pr.hold(nb)


WRONG_ON = {"code_of_from": ("seams", (5, 3, 37, 31), 0),
            "window_at_to": ("seams", (1, 1, 46, 45), 0),
            "skips_no_writer": ("nones", cc.REFUSAL_RECT, cc.NONES_START),
            # from frame 4: "key_same" (index frame 2) codes every block with what it shows, and most blocks have no earlier writer in the index
            "tight_needs_written_to": ("tight", cc.TIGHT_RECT, 4)}


@pytest.mark.parametrize("bits", [16, 8])
@pytest.mark.parametrize("wrong", pr.WRONG)
def test_each_wrong_variant_fails_on_its_clip(bits, wrong):
    name, rect, start = WRONG_ON[wrong]
    clip = cc.seams(bits, rect) if name == "seams" else getattr(cc, name)(bits)
    s = source(clip, start)
    tight = wrong == "tight_needs_written_to"
    pairs = back_pairs(s.n) + hold_pairs(s.n)[::3]
    right = [p for p in pairs if isinstance(made(s, rect, p, tight), bytes)]
    assert right and not any(fails(s, rect, p, made(s, rect, p, tight), tight) for p in right[::3])
    bad = [p for p in pairs if fails(s, rect, p, made(s, rect, p, tight, wrong), tight)]
    print(f"{wrong} ({bits} bits): fails on {len(bad)} of {len(pairs)} pairs, first {bad[:3]}")
    assert bad and all(a > b for a, b in bad), wrong
    if wrong == "skips_no_writer":
        assert all(made(s, rect, p)[0] == "none" and isinstance(made(s, rect, p, False, wrong), bytes) for p in bad)
    if wrong == "tight_needs_written_to":   # the right rule drops what the picture before the index already shows
        assert (2, 1) in bad and made(s, rect, (2, 1), True) == pr.hold(rect[2] * rect[3]) and made(s, rect, (2, 1), True, wrong)[0] == "none"
