"""The frames of a block rectangle of a seek index, checked without a GPU: the plain-Python statement of the rule
(tests/index_crop_ref.py) is pinned to the oracle.  The oracle decodes the source clip; an oracle of the rectangle's size, 4 bw x 4 bh,
decodes a key pair's frame and then gap pairs' frames on top: after each it holds the sub-rectangle of the source's picture.  Then the
identity with the whole-picture references for the whole grid, four deliberately wrong variants of the rule, each failing on a named
clip, and that the clips reach the seams and refusals they claim.  Nothing of the GPU is involved."""
import numpy as np
import pytest

import index_crop_ref as cr
import index_delta_ref as dr
import index_keyframe_ref as kr
import index_tight_ref as tr
import msv1_crop_clips as cc
from msv1_range_clips import POISON, palette, truth_run
from oracle_binding import OracleMSVideo1
from test_index_delta_ref_cpu import structure

LINES = 36
_sources = {}


class Source:
    """A clip's index from frame `start`: the oracle's pictures, codes_of of every frame, the block pixels for the tight rule."""

    def __init__(self, clip, start=0):
        self.clip, self.bits, self.start = clip, clip.bits, start
        self.pal = palette(clip.bits)
        truth = truth_run(clip.bits, cc.W, cc.H, self.pal, clip.frames, clip.keys, LINES, key_row=LINES)
        self.range = clip.frames[start:]
        self.pictures = [np.asarray(t[0]).reshape(cc.H, cc.W) for t in truth[start:]]
        self.codes = [kr.codes_of(clip.bits, cc.NBX, cc.NBY, f) for f in self.range]
        before = truth[start - 1][0] if start > 0 else None
        self.px = tr.Pixels(clip.bits, cc.W, cc.H, self.range, self.codes, self.pal, before, [t[0] for t in truth[start:]])
        self.n = len(self.range)
        self._made = {}

    def crop(self, rect, pair, tight=False, wrong=None):
        k = (rect, pair, tight, wrong)
        if k not in self._made:
            self._made[k] = cr.crop(self.bits, cc.NBX, self.range, rect, pair, self.codes, tight, self.px, wrong)
        return self._made[k]

    def sub(self, rect, t):
        bx, by, bw, bh = rect
        return self.pictures[t][4 * by:4 * by + 4 * bh, 4 * bx:4 * bx + 4 * bw]


def source(clip, start=0):
    k = (clip.name, clip.bits, start)
    if k not in _sources:
        _sources[k] = Source(clip, start)
    return _sources[k]


class Small:
    """An oracle of the rectangle's size, fed frames one after the other."""

    def __init__(self, s, rect):
        self.w, self.h = 4 * rect[2], 4 * rect[3]
        self.o = OracleMSVideo1(s.bits, self.w, self.h, s.pal)
        self.o.Preinit(LINES)
        self.pic = np.full(self.w * self.h, POISON, dtype=np.int32)

    def key(self, data):
        assert self.o.IsKeyFrame(data)
        pic = np.full(self.w * self.h, POISON, dtype=np.int32)
        assert self.o.DecompressI(data, pic) == 0
        self.pic = pic
        return pic.reshape(self.h, self.w)

    def inter(self, data):
        pic = self.pic.copy()
        self.o.DecompressP(data, pic)
        self.pic = pic
        return pic.reshape(self.h, self.w)

    def close(self):
        self.o.close()


def written_in(s, rect, a, b, tight):
    """The blocks j of the rectangle that a gap pair codes."""
    v = cr.Virtual(s.px, cc.NBX, rect)
    if tight:
        return tr.kept_set(v, a, b)[1]
    return [j for j in range(len(v.order)) if dr.writer(v.codes, a, b, j) is not None]


def fails(s, rect, pair, data, tight=False):
    """Whether `data` is NOT a frame the rule promises for the pair: a refusal where the right rule has none (or the reverse), bytes
    that break the structure of a frame of nb blocks, or bytes that do not decode to the sub-rectangle of the source's picture."""
    right = s.crop(rect, pair, tight)
    if not isinstance(data, bytes) or not isinstance(right, bytes):
        return data != right
    nb = rect[2] * rect[3]
    a, b = pair
    small = Small(s, rect)
    try:
        if a == cr.KEY:
            if not cr.flag(s.bits, data, nb) or not small.o.IsKeyFrame(data):
                return True
            return not np.array_equal(small.key(data), s.sub(rect, b))
        try:
            structure(s.bits, nb, data, written_in(s, rect, a, b, tight), "")
        except AssertionError:
            return True
        before = s.crop(rect, (cr.KEY, a)) if a >= 0 else None
        if not isinstance(before, bytes):   # (no key frame to decode on top of: the structure is all that can be seen)
            return False
        small.key(before)
        return not np.array_equal(small.inter(data), s.sub(rect, b))
    finally:
        small.close()


def check(s, rect, pairs, tight):
    """Every pair against the oracle; then chains of gap pairs behind a key pair.  Returns the number of frames decoded."""
    nb = rect[2] * rect[3]
    done = 0
    for pair in pairs:
        data = s.crop(rect, pair, tight)
        assert isinstance(data, bytes), (rect, pair, data)
        assert len(data) <= nb * (18 if s.bits == 16 else 10)
        assert not fails(s, rect, pair, data, tight), (s.clip.name, s.bits, rect, pair, tight)
        if pair[0] == -1 and s.start == 0:   # nothing before the index: every block has a writer, and the frame is the key frame
            assert data == s.crop(rect, (cr.KEY, pair[1])), (rect, pair)
        done += 1
    for t0, stride in ((0, 1), (1, 2), (2, 3)):
        ts = list(range(t0, s.n, stride))
        small = Small(s, rect)
        assert np.array_equal(small.key(s.crop(rect, (cr.KEY, t0), tight)), s.sub(rect, t0))
        for a, b in zip(ts, ts[1:]):
            data = s.crop(rect, (a, b), tight)
            assert np.array_equal(small.inter(data), s.sub(rect, b)), (s.clip.name, rect, a, b, tight)
            assert bool(small.o.IsKeyFrame(data)) == cr.flag(s.bits, data, nb) == (len(written_in(s, rect, a, b, tight)) == nb)
            done += 1
        small.close()
    return done


@pytest.mark.parametrize("bits", [16, 8])
@pytest.mark.parametrize("rect", cc.RECTS, ids=cc.rect_id)
def test_seam_clips_decode_to_the_sub_rectangle_of_the_oracles_pictures(bits, rect):
    s = source(cc.seams(bits, rect))
    pairs = cc.pairs(s.n)
    assert check(s, rect, pairs, False) > len(pairs)
    assert check(s, rect, [p for p in pairs if p[1] - p[0] == 1 or p[0] == cr.KEY], True) > 0


@pytest.mark.parametrize("bits", [16, 8])
def test_the_tight_clip_decodes_to_the_sub_rectangle_and_drops_what_the_inner_clip_drops(bits):
    clip = cc.tight(bits)
    s, rect = source(clip), clip.rect
    inner = clip.inner
    icodes = [kr.codes_of(bits, inner.nbx, inner.nby, f) for f in inner.frames]
    truth = truth_run(bits, inner.w, inner.h, s.pal, inner.frames, inner.keys, LINES, key_row=LINES)
    ipx = tr.Pixels(bits, inner.w, inner.h, inner.frames, icodes, s.pal, None, [t[0] for t in truth])
    pairs = [(a, b) for a in range(s.n) for b in range(a + 1, min(a + 4, s.n))] + [(cr.KEY, t) for t in range(s.n)]
    assert check(s, rect, pairs, True) > 0 and check(s, rect, pairs[::3], False) > 0
    shorter = 0
    for a, b in [p for p in pairs if p[0] >= 0]:
        # the rectangle's frames are the inner clip's own tight and delta frames: the clip of the rectangle's size, byte for byte
        assert s.crop(rect, (a, b), True) == tr.tight(ipx, a, b), (a, b)
        assert s.crop(rect, (a, b), False) == dr.delta(bits, inner.nbx, inner.nby, inner.frames, a, b, icodes), (a, b)
        shorter += len(s.crop(rect, (a, b), True)) < len(s.crop(rect, (a, b), False))
    assert shorter > 5
    assert s.crop(rect, (0, 1), True) == b"".join(dr.skip_word(c) for c in (1023, inner.nb - 1023))


@pytest.mark.parametrize("bits", [16, 8])
def test_the_whole_grid_reproduces_the_whole_picture_references(bits):
    for clip in (cc.seams(bits, cc.WHOLE), cc.tight(bits), cc.cuts(bits)):
        s = source(clip)
        for a, b in [(a, b) for b in range(s.n) for a in (-1, b - 1, b - 2) if -1 <= a < b][:40]:
            assert s.crop(cc.WHOLE, (a, b)) == dr.delta(bits, cc.NBX, cc.NBY, s.range, a, b, s.codes), (clip.name, a, b)
            if clip.name != "crop_cuts":
                assert s.crop(cc.WHOLE, (a, b), True) == tr.tight(s.px, a, b), (clip.name, a, b)
        for t in range(min(s.n, 12)):
            assert s.crop(cc.WHOLE, (cr.KEY, t)) == kr.key_frame(bits, cc.NBX, cc.NBY, s.range, t, s.codes), (clip.name, t)
            assert s.crop(cc.WHOLE, (cr.KEY, t), True) == s.crop(cc.WHOLE, (cr.KEY, t))


WRONG_ON = {"neighbour_in_source": ("seams", (5, 3, 37, 31)),       # outside blocks written next to an unwritten row start
            "run_in_source_numbering": ("seams", (1, 1, 46, 45)),   # src(j) % 1023 == 0 in the middle of a run, j % 1023 == 0 without a word
            "row_of_source": ("seams", (3, 2, 3, 2)),
            "key_skips_unwritten": ("nones", cc.REFUSAL_RECT)}


@pytest.mark.parametrize("bits", [16, 8])
@pytest.mark.parametrize("wrong", cr.WRONG)
def test_each_wrong_variant_fails_on_its_clip(bits, wrong):
    kind, rect = WRONG_ON[wrong]
    if kind == "seams":
        s = source(cc.seams(bits, rect))
    else:
        s = source(cc.nones(bits), cc.NONES_START)
    pairs = cc.pairs(s.n)
    right = [p for p in pairs if isinstance(s.crop(rect, p), bytes)]
    assert not any(fails(s, rect, p, s.crop(rect, p)) for p in right[::4])
    bad = [p for p in pairs if fails(s, rect, p, s.crop(rect, p, wrong=wrong))]
    print(f"{wrong} ({bits} bits): fails on {len(bad)} of {len(pairs)} pairs, first {bad[:3]}")
    assert bad, wrong
    if wrong == "key_skips_unwritten":
        assert all(p[0] == cr.KEY for p in bad)
    if wrong == "neighbour_in_source":
        assert any(p[1] - p[0] == 1 and p[1] % 2 == 0 for p in bad)   # (a frame of an odd pattern: the outside is written)


@pytest.mark.parametrize("bits", [16, 8])
def test_the_seam_clips_reach_the_seams_they_claim(bits):
    def skips_of(rect, name):
        s = source(cc.seams(bits, rect))
        f = next(f for f, n in s.clip.patterns.items() if n == name)
        return dr.walk(bits, s.crop(rect, (f - 1, f)))[1]

    # (5, 3, 37, 31): runs cross the row ends of the rectangle (37 is no divisor of a run's end) and 1023 | 1024 mid-row
    rect = (5, 3, 37, 31)
    assert 1023 % 37 != 0 and 1024 % 37 != 0
    assert skips_of(rect, "last") == [(0, 1023), (1023, 1147 - 1024)]
    assert skips_of(rect, "nothing") == [(0, 1023), (1023, 124)]
    assert (1000, 23) in skips_of(rect, "to_1023") and (1000, 23) in skips_of(rect, "to_wg") and (1023, 1) in skips_of(rect, "to_wg")
    assert (1023, 124) in skips_of(rect, "across")
    # every run of more than one row crosses a row start whose source neighbour lies outside the rectangle
    assert any(at // 37 != (at + count - 1) // 37 for at, count in skips_of(rect, "spots"))
    assert skips_of((8, 8, 32, 32), "nothing") == [(0, 1023), (1023, 1)] and skips_of((8, 8, 33, 31), "nothing") == [(0, 1023)]
    # (1, 1, 46, 45): three workgroups; a run from block 1023 over the whole second workgroup to the end, cut at 2046
    assert skips_of((1, 1, 46, 45), "across") == [(1023, 1023), (2046, 24)]
    assert skips_of((1, 1, 46, 45), "last") == [(0, 1023), (1023, 1023), (2046, 23)]
    assert skips_of((1, 1, 46, 45), "wg_first") == [(0, 1023), (1023, 1), (1025, 1021), (2046, 2), (2049, 21)]
    assert skips_of((47, 0, 1, 48), "singles") == [(j, 1) for j in range(1, 48, 2)] == skips_of((0, 47, 48, 1), "singles")
    for rect in cc.CORNERS:
        assert skips_of(rect, "nothing") == [(0, 1)] and skips_of(rect, "every") == []
    assert skips_of((3, 2, 3, 2), "first") == [(1, 5)]
    # the outside is written in the frames of the odd patterns and in no other
    s = source(cc.seams(bits, (5, 3, 37, 31)))
    for f, name in s.clip.patterns.items():
        k = cc.dc.PATTERNS.index(name)
        coded = {i for i, c in enumerate(s.codes[f]) if c is not None}
        assert (set(s.clip.outside) <= coded) if k % 2 == 1 else not (set(s.clip.outside) & coded), name


@pytest.mark.parametrize("bits", [16, 8])
def test_the_refusal_clips_refuse_at_every_listed_block_and_nowhere_outside(bits):
    rect = cc.REFUSAL_RECT
    nb = rect[2] * rect[3]
    clip = cc.cuts(bits)
    s = source(clip)
    assert [j for _, _, j in clip.groups] == [0, 3, 4, 255, 256, 1023, 1024, nb - 1, None, None]
    for first, p, j in clip.groups:
        whole_key = kr.key_frame(bits, cc.NBX, cc.NBY, s.range, first + 2, s.codes)
        assert whole_key == ("cut", p)
        if j is None:   # a cut code just outside: the whole picture refuses, the rectangle does not (in frame first + 1 the end
            # of the data cuts every block behind p as well; frame first + 2 codes those whole)
            for pair in ((cr.KEY, first + 2), (first, first + 2), (first + 1, first + 2)):
                assert isinstance(s.crop(rect, pair), bytes), (p, pair)
            assert dr.delta(bits, cc.NBX, cc.NBY, s.range, first, first + 2, s.codes) == ("cut", p)
            continue
        assert cr.src(cc.NBX, rect, j) == p
        for pair in ((cr.KEY, first + 1), (cr.KEY, first + 2), (first, first + 2), (first, first + 1)):
            assert s.crop(rect, pair) == ("cut", j), (j, pair)
            assert cr.writer(s.codes, cc.NBX, rect, pair, j) == first + 1
        assert s.crop(rect, (first, first + 2), True) == ("cut", j)          # (new colours: kept)
        for pair in ((cr.KEY, first), (cr.KEY, first + 3), (first + 1, first + 2), (first + 1, first + 3), (first, first + 3)):
            assert isinstance(s.crop(rect, pair), bytes), (j, pair)
        assert not fails(s, rect, (cr.KEY, first + 3), s.crop(rect, (cr.KEY, first + 3)))
    clip = cc.nones(bits)
    s = source(clip, cc.NONES_START)
    assert clip.at == [0, 3, 4, 255, 256, 1023, 1024, nb - 1] and s.n == 1 + len(clip.at)
    for k, j in enumerate(clip.at):
        assert s.crop(rect, (cr.KEY, k)) == ("none", j) == s.crop(rect, (cr.KEY, k), True), (k, j)
        assert isinstance(s.crop(rect, (-1, k)), bytes) and isinstance(s.crop(rect, (0, k), True) if k else b"", bytes)
    last = s.n - 1
    assert isinstance(s.crop(rect, (cr.KEY, last)), bytes) and not fails(s, rect, (cr.KEY, last), s.crop(rect, (cr.KEY, last)))
    assert kr.key_frame(bits, cc.NBX, cc.NBY, s.range, last, s.codes) == ("none", cc.outside_of(rect)[0])
    # a gap pair over blocks without a writer skips them: decoded on top of the picture before the index it is the source's picture
    assert not fails(s, rect, (0, last), s.crop(rect, (0, last)))
