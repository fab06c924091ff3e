"""The frames of a block rectangle that moves over a seek index, checked without a GPU: the plain-Python statement of the rule
(tests/index_pan_ref.py) is pinned to the oracle.  The oracle decodes the source clip; an oracle of the rectangle's size, holding
rectangle A of the source's picture of `from`, decodes a pair's frame and then holds rectangle B of the picture of `to`; chains start
from a KEY pair's frame.  Then four deliberately wrong variants of the rule, each failing on a named clip, the identity with
index_crop_ref for a rectangle that stands, and that every moved tight pair the clips ask for drops a block and keeps a block unless
the clip names it otherwise.  Nothing of the GPU is involved."""
import numpy as np
import pytest

import index_delta_ref as dr
import index_keyframe_ref as kr
import index_pan_ref as pr
import index_tight_ref as tr
import msv1_crop_clips as cc
import msv1_pan_clips as pc
from msv1_range_clips import POISON, truth_run
from test_index_crop_ref_cpu import LINES, Small
from test_index_crop_ref_cpu import source as crop_source

KEY = pr.KEY
_sources = {}


class Source:
    """A pan clip's index from its start: the oracle's pictures, codes_of of every frame, the block pixels, and the reference's answers
    (worked out once per pair)."""

    def __init__(self, clip):
        self.clip, self.bits, self.start, self.size, self.pal = clip, clip.bits, clip.start, clip.size, clip.pal
        truth = truth_run(clip.bits, pc.W, pc.H, self.pal, clip.frames, clip.keys, LINES, key_row=LINES)
        self.range = clip.frames[self.start:]
        self.pictures = [np.asarray(t[0]).reshape(pc.H, pc.W) for t in truth[self.start:]]
        self.before = np.asarray(truth[self.start - 1][0]).reshape(pc.H, pc.W) if self.start > 0 else None
        self.codes = [kr.codes_of(clip.bits, pc.NBX, pc.NBY, f) for f in self.range]
        self.px = tr.Pixels(clip.bits, pc.W, pc.H, self.range, self.codes, self.pal, self.before, [t[0] for t in truth[self.start:]])
        self.n = len(self.range)
        self._made = {}

    def pan(self, pair, tight=False, wrong=None):
        k = (pair, tight, wrong)
        if k not in self._made:
            self._made[k] = pr.pan(self.bits, pc.NBX, self.range, self.size, pair, self.codes, tight, self.px, wrong)
        return self._made[k]

    def kept(self, pair):
        return pr.kept(self.px, pc.NBX, self.size, pair)

    def sub(self, origin, t):
        """Rectangle `origin` of the picture of index frame t (-1: of the picture before the range, None without one)."""
        pic = self.before if t < 0 else self.pictures[t]
        if pic is None:
            return None
        (bx, by), (bw, bh) = origin, self.size
        return pic[4 * by:4 * by + 4 * bh, 4 * bx:4 * bx + 4 * bw]


def source(clip):
    k = (clip.name, clip.bits)
    if k not in _sources:
        _sources[k] = Source(clip)
    return _sources[k]


def small(s):
    return Small(s, (0, 0) + tuple(s.size))


def fails(s, pair, data, tight=True):
    """Whether `data` is NOT a frame the rule promises for the pair: a refusal where the right rule has none (or the reverse), words
    that do not cover the rectangle's blocks, or bytes that a decoder holding rectangle A of the picture of `from` does not turn into
    rectangle B of the picture of `to`."""
    right = s.pan(pair, tight)
    if not isinstance(data, bytes) or not isinstance(right, bytes):
        return data != right
    a, b, A, B = pair
    nb = s.size[0] * s.size[1]
    try:
        codes, skips, covered = dr.walk(s.bits, data)
    except AssertionError:
        return True
    if covered != nb:
        return True
    o = small(s)
    try:
        if a == KEY:
            return not (o.o.IsKeyFrame(data) and np.array_equal(o.key(data), s.sub(B, b)))
        o.key((b"\x05\x80" if s.bits == 8 else b"\x05\x81") * nb)   # (any key frame: the decoder needs a frame before)
        held = s.sub(A, a)
        o.pic[:] = POISON if held is None else np.ascontiguousarray(held).reshape(-1)   # (in place: it is the decoder's frame before)
        return not np.array_equal(o.inter(data), s.sub(B, b))
    finally:
        o.close()


def moved_tight(clip):
    return [q for q in clip.pairs if pr.kind(q) == "moved"]


@pytest.mark.parametrize("bits", [16, 8])
def test_every_clip_decodes_to_rectangle_b_of_the_oracles_pictures(bits):
    done = 0
    for clip in pc.all_clips(bits):
        s = source(clip)
        nb = s.size[0] * s.size[1]
        for pair in clip.pairs:
            for tight in (True, False):
                data = s.pan(pair, tight)
                if isinstance(data, bytes):
                    assert len(data) <= nb * (18 if bits == 16 else 10)
                    assert not fails(s, pair, data, tight), (clip.name, bits, pair, tight)
                    done += 1
        # the chain: a fresh decoder, the KEY pair's frame, then every pair's frame on top of the one before
        if clip.chain:
            for tight in (True, False):
                o = small(s)
                for k, pair in enumerate(clip.pairs[:clip.chain]):
                    data = s.pan(pair, tight)
                    assert isinstance(data, bytes), (clip.name, pair)
                    got = o.key(data) if k == 0 else o.inter(data)
                    assert np.array_equal(got, s.sub(pair[3], pair[1])), (clip.name, bits, pair, tight)
                    if k:
                        assert clip.pairs[k - 1][1] == pair[0] and clip.pairs[k - 1][3] == pair[2]
                    assert bool(o.o.IsKeyFrame(data)) == pr.flag(bits, data, nb)
                o.close()
    assert done > 100


@pytest.mark.parametrize("bits", [16, 8])
def test_every_moved_tight_pair_drops_a_block_and_keeps_a_block_unless_named(bits):
    """So that a comparison of bytes cannot pass on empty frames, or on key frames."""
    mixes = 0
    for clip in pc.all_clips(bits):
        s = source(clip)
        nb = s.size[0] * s.size[1]
        assert moved_tight(clip), clip.name
        for pair in moved_tight(clip):
            kept, got, name = s.kept(pair), s.pan(pair, True), clip.named.get(pair)
            where = (clip.name, bits, pair)
            if name == "all dropped":
                assert kept == [] and isinstance(got, bytes) and not dr.walk(bits, got)[0], where
            elif name == "all kept":
                assert len(kept) == nb and got == s.pan((KEY, pair[1], None, pair[3])), where
            elif isinstance(name, tuple):
                assert got == name and name[1] in kept, where
            else:
                assert 0 < len(kept) < nb and isinstance(got, bytes), where + (len(kept),)
                assert [c[0] for c in dr.walk(bits, got)[0]] == kept, where
                mixes += 1
            loose = s.pan(pair, False)
            assert loose == s.pan((KEY, pair[1], None, pair[3])), where
            if isinstance(got, bytes) and isinstance(loose, bytes):
                assert len(got) <= len(loose) and pr.flag(bits, loose, nb), where
    assert mixes > 40


@pytest.mark.parametrize("bits", [16, 8])
def test_the_clips_reach_what_they_claim(bits):
    for size in pc.SIZES:
        clip = pc.bounds(bits, size)
        s = source(clip)
        bw, nb = size[0], size[0] * size[1]
        unwritten = 0
        for pair, name in clip.patterns.items():
            kept = s.kept(pair)
            assert kept == clip.kept[pair], (clip.name, name)
            # kept blocks no frame of the gap writes, dropped blocks the gap writes with other bytes
            srcb = [pr.cr.src(pc.NBX, pr.rect_of(size, pair[3]), j) for j in range(nb)]
            unwritten += sum(dr.writer(s.codes, pair[0], pair[1], srcb[j]) is None for j in kept)
            if name == "nothing":
                assert sum(dr.writer(s.codes, pair[0], pair[1], b) is not None for b in srcb) > nb // 2
        assert unwritten > 0, clip.name
        names = set(clip.patterns.values())
        assert {"nothing", "every", "row_starts", "not_row_starts"} <= names
        if nb > 4:
            assert {"from_4", "to_4"} <= names
        if nb > 1023:
            assert {"to_256", "from_256", "to_1023", "from_1023"} <= names       # 255|256 and 1022|1023 from both sides
        if nb > 1024:
            assert {"to_1024", "from_1024"} <= names                              # 1023|1024: the second workgroup's only block
        if nb == 1023:
            assert {"to_256", "from_256"} <= names and dr.walk(bits, s.pan(next(p for p, m in clip.patterns.items() if m == "nothing"), True))[1] == [(0, 1023)]
    # the lagging rectangle: the kept blocks are two columns of the rectangle
    clip = pc.scroll(bits, (33, 31), "lag")
    s = source(clip)
    for pair in clip.pairs[1:clip.chain]:
        assert len({j % 33 for j in s.kept(pair)}) == 2 and len(s.kept(pair)) == 2 * 29, pair
    # the cut clip: every block of the painted rectangles has a cut code, and the frames are skip words only
    clip = pc.cuts(bits)
    s = source(clip)
    for pair in clip.pairs[:2]:
        srcb = [pr.cr.src(pc.NBX, pr.rect_of(clip.size, pair[3]), j) for j in range(18)]
        assert all(s.codes[1][b] == "cut" for b in srcb) and s.pan(pair, True) == dr.skip_word(18)
        assert s.pan(pair, False) == ("cut", 0)
    assert pr.writer(s.codes, pc.NBX, clip.size, clip.pairs[2], 1) == 1
    # the clip from mid-range: no writers where it says so
    clip = pc.befores(bits)
    s = source(clip)
    assert s.before is not None and s.start == pc.BEFORE_START
    for pair in clip.pairs[:6]:
        srcb = [pr.cr.src(pc.NBX, pr.rect_of(clip.size, pair[3]), j) for j in range(18)]
        assert all(dr.writer(s.codes, -1, pair[1], b) is None for b in srcb), pair


WRONG_ON = {"movement_ignored": ("scroll", (32, 32), "against"),    # the pan across a standing picture: nothing seems to change
            "gated_by_written": ("bounds", (41, 25), None),        # kept blocks that no frame of the gap writes
            "code_from_src_a": ("bounds", (3, 2), None),
            "dropped_refuses": ("cuts", None, None)}               # dropped blocks whose codes are cut


@pytest.mark.parametrize("bits", [16, 8])
@pytest.mark.parametrize("wrong", pr.WRONG)
def test_each_wrong_variant_fails_on_its_clip(bits, wrong):
    family, size, how = WRONG_ON[wrong]
    clip = pc.scroll(bits, size, how) if family == "scroll" else pc.bounds(bits, size) if family == "bounds" else pc.cuts(bits)
    s = source(clip)
    pairs = moved_tight(clip)
    assert not any(fails(s, p, s.pan(p, True)) for p in pairs)
    bad = [p for p in pairs if fails(s, p, s.pan(p, True, wrong=wrong))]
    print(f"{wrong} ({bits} bits): fails on {len(bad)} of {len(pairs)} pairs of {clip.name}, first {bad[:2]}")
    assert bad, wrong
    if wrong == "movement_ignored":
        assert any(p[0] == p[1] for p in bad)
    if wrong == "dropped_refuses":
        assert all(isinstance(s.pan(p, True, wrong=wrong), tuple) for p in bad)
        b = source(pc.befores(bits))
        assert b.pan(b.clip.pairs[0], True, wrong=wrong) == ("none", 0) and isinstance(b.pan(b.clip.pairs[0], True), bytes)


@pytest.mark.parametrize("bits", [16, 8])
def test_a_rectangle_that_stands_is_the_crop_reference(bits):
    for rect in ((5, 3, 37, 31), (1, 1, 46, 45)):
        s = crop_source(cc.seams(bits, rect))
        size, origin = rect[2:], rect[:2]
        for a, b in cc.pairs(s.n):
            for tight in (False, True):
                if tight and not (b - a == 1 or a == KEY):
                    continue
                pair = (a, b, None if a == KEY else origin, origin)
                got = pr.pan(bits, cc.NBX, s.range, size, pair, s.codes, tight, s.px)
                assert got == s.crop(rect, (a, b), tight), (rect, a, b, tight)
    s = crop_source(cc.nones(bits), cc.NONES_START)
    rect = cc.REFUSAL_RECT
    for k in range(s.n):
        assert pr.pan(bits, cc.NBX, s.range, rect[2:], (KEY, k, None, rect[:2]), s.codes) == s.crop(rect, (KEY, k))
