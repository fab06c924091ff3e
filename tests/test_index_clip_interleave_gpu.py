"""The clip calls of an MSVideo1 seek index — DeltaFrames, DeltaFrames(tight), CropFrames, PathFrames, PanFrames — one after the other
on ONE index, on an MI355X.  They run one host loop (clip_frames, msv1_seek.cpp) over three scratch buffers of the index, and a call
of one slice gathers from the records its sizes launch left: nothing one call leaves may reach another.

Seven calls in a fixed order, then the same seven in reverse order, with two refused calls (a cut code) in the middle of each round:
every result equals the plain-Python rule (index_delta_ref, index_tight_ref, index_crop_ref, index_pan_ref, index_path_ref — pinned to
the oracle by the test_index_*_ref_cpu files), the second round equals the first, and jsp_index_info says the same after both.

The index: msv1_pan_clips.spliced, the 48 x 48-block picture of tests/msv1_pan_clips.py — the first frames of its `bounds` clip for
32 x 32 blocks (the kept / dropped seam on j = 3|4 and 255|256, all and nothing), then the cut frame of its `cuts` clip (block CUT_AT
ends one byte short) and that clip's empty frame.  Rectangles of 33 x 32 blocks are two workgroups, the whole grid is three, 3 x 2 is
less than two lanes' share."""
import ctypes as C

import pytest

import index_crop_ref as cr
import index_delta_ref as dr
import index_pan_ref as pr
import index_path_ref as par
import index_tight_ref as tr
import msv1_pan_clips as pc
from jsplayer_amd import CodecError
from jsplayer_amd import _native as N
from test_index_pan_gpu import Case
from test_index_pan_ref_cpu import source

pytestmark = pytest.mark.gpu

KEY = pr.KEY
CUT = pc.SPLICE_HEAD           # the index frame whose data ends within the code of block pc.CUT_AT
A, B = pc.ORIGINS              # the two origins the bounds clip hops between
BIG, SMALL, GRID = (33, 32), (3, 2), (0, 0, pc.NBX, pc.NBY)

_made = {}


# (name, the call on a SeekIndex, the rule for one pair on a Source, the blocks of a frame — None: no flags —, the pairs)
def calls():
    def delta(tight):
        return (lambda idx, pairs: idx.DeltaFrames(pairs, tight=tight),
                lambda s, p: tr.tight(s.px, *p) if tight else dr.delta(s.bits, pc.NBX, pc.NBY, s.range, p[0], p[1], s.codes))

    def crop(rect, tight):
        return (lambda idx, pairs: idx.CropFrames(rect, pairs, tight=tight),
                lambda s, p: cr.crop(s.bits, pc.NBX, s.range, rect, p, s.codes, tight, s.px))

    def path(rect, tight):
        return (lambda idx, pairs: idx.PathFrames(rect, pairs, tight=tight),
                lambda s, p: par.path(s.bits, pc.NBX, s.range, rect, p, s.codes, tight, s.px))

    def pan(size, tight):
        return (lambda idx, pairs: idx.PanFrames(size, pairs, tight=tight),
                lambda s, p: pr.pan(s.bits, pc.NBX, s.range, size, p, s.codes, tight, s.px))

    return [
        ("delta", *delta(False), None, [(-1, 0), (0, 1), (1, 3), (2, 5), (4, 5)]),
        ("crop 33x32", *crop(A + BIG, False), 33 * 32, [(KEY, 0), (0, 1), (1, 2), (0, 4), (KEY, 5)]),
        ("pan 3x2", *pan(SMALL, False), 6, [(KEY, 0, None, A), (0, 1, A, A), (1, 2, A, B), (2, 2, B, (4, 2)), (2, 3, (4, 2), (4, 2))]),
        ("path grid", *path(GRID, False), pc.NB, [(KEY, 5), (5, 3), (3, 3), (3, 0), (0, 2), (7, 7)]),
        ("tight", *delta(True), None, [(0, 1), (1, 3), (-1, 2), (3, 4)]),
        ("crop 3x2", *crop(B + SMALL, True), 6, [(KEY, 2), (2, 3), (3, 5), (5, CUT)]),
        ("pan 33x32", *pan(BIG, True), 33 * 32, [(KEY, 0, None, A), (0, 1, A, B), (1, 2, B, A), (2, 4, A, (10, 7)), (4, 5, (10, 7), (10, 7))]),
    ]


def wanted(bits):
    """The rule's answer to every call, worked out once per bit depth: [(frames, flags or None)]."""
    k = ("want", bits)
    if k not in _made:
        s = source(pc.spliced(bits))
        out = []
        for name, _, rule, nb, pairs in calls():
            frames = [rule(s, p) for p in pairs]
            assert all(isinstance(x, bytes) for x in frames), name
            out.append((frames, None if nb is None else [cr.flag(bits, x, nb) for x in frames]))
        assert dr.delta(bits, pc.NBX, pc.NBY, s.range, CUT - 1, CUT, s.codes) == ("cut", pc.CUT_AT)
        _made[k] = out
    return _made[k]


def info(idx):
    n, dev, host = C.c_int(0), C.c_uint64(0), C.c_uint64(0)
    assert N.lib().jsp_index_info(idx._h, C.byref(n), C.byref(dev), C.byref(host)) == 0
    return n.value, dev.value, host.value


def refused(idx):
    """Two calls that a cut code refuses, through the pan scratch and through the delta scratch."""
    with pytest.raises(CodecError, match=f"index_pan: pair 1 .*block 1 of the rectangle \\(block {pc.CUT_AT} of the picture\\) in frame {CUT},"):
        idx.PanFrames(pc.CUT_SIZE, [(KEY, 0, None, (19, 10)), (CUT - 1, CUT, (18, 10), (19, 10))])
    with pytest.raises(CodecError, match=f"index_delta: pair 2 \\({CUT - 1}, {CUT}\\]: the code of block {pc.CUT_AT} in frame {CUT},"):
        idx.DeltaFrames([(0, 1), (1, 2), (CUT - 1, CUT)])


@pytest.mark.parametrize("slice_", ["1", "auto"])
@pytest.mark.parametrize("bits", [16, 8])
def test_seven_calls_forward_and_in_reverse_leave_nothing_to_each_other(bits, slice_):
    want = wanted(bits)
    c = Case.of(pc.spliced(bits))
    try:
        c.gpu.set_option("msv1_index_delta_slice", slice_)
        seven = calls()

        def run(k):
            name, call, _, nb, pairs = seven[k]
            got = call(c.idx, pairs)
            return (got, None) if nb is None else got

        first = {}
        for k in range(7):
            first[k] = run(k)
            assert first[k] == want[k], f"{c.where} slice {slice_}: {seven[k][0]} in the first round"
            if k == 3:
                refused(c.idx)
        after_first = info(c.idx)
        for k in reversed(range(7)):
            assert run(k) == first[k], f"{c.where} slice {slice_}: {seven[k][0]} in the second round"
            if k == 3:
                refused(c.idx)
        assert info(c.idx) == after_first, f"{c.where} slice {slice_}"
        assert (c.idx.device_bytes, c.idx.host_bytes) == after_first[1:]
    finally:
        c.close()
