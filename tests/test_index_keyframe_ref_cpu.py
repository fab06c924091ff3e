"""The key frame of a seek index, checked without a GPU: the plain-Python statement of the rule (tests/index_keyframe_ref.py) is pinned
to the oracle.  For every frame t of the range whose key_frame is bytes, the oracle says that they are a key frame, decodes them to
its own sequential picture of frame t on every pixel a block covers, and decodes the original frame t + 1 on top of that to its
picture of t + 1.  Nothing of the GPU is involved."""
import numpy as np
import pytest

import index_keyframe_ref as kr
from msv1_range_clips import POISON, coded_blocks, long_clip, truth_run
from oracle_binding import OracleMSVideo1

N = 72   # frames of the index's range

# (bits, start) -> (cuttable, refused, kind of the refusals) of the N frames, the same for the three sizes.  16-bit from 0: the
# truncated frame 31 blackens blocks with codes past its end, and they stay until key 70.  8-bit from 0: end markers leave blocks
# alone, nothing is cut off.  From 3: blocks show the picture before the range until key 70 (t = 67 of the range) codes them all.
EXPECTED = {(16, 0): (33, 39, "cut"), (8, 0): (72, 0, None), (16, 3): (5, 67, "none"), (8, 3): (5, 67, "none")}


def covered(pic, w, h):
    """The pixels of a picture (h * w words) that a 4x4 block covers."""
    return np.asarray(pic).reshape(h, w)[:4 * (h // 4), :4 * (w // 4)]


@pytest.mark.parametrize("bits", [16, 8])
@pytest.mark.parametrize("size", [(64, 32), (52, 28), (54, 30)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("start", [0, 3])
def test_key_frames_decode_to_the_oracles_pictures(bits, size, start):
    w, h = size
    nbx, nby = w // 4, h // 4
    frames, keys, pal, plan = long_clip(bits, w, h, seed=5, n=96)
    assert not plan["raises"]
    truth = truth_run(bits, w, h, pal, frames[:start + N + 1], keys[:start + N + 1], plan["lines"], key_row=plan["lines"])
    assert all(x is not None and x[0] is not None for x in truth)
    rng = frames[start:start + N]
    codes = [kr.codes_of(bits, nbx, nby, f) for f in rng]
    for i, c in enumerate(codes):   # the reference codes a block exactly where coded_blocks says so
        want = coded_blocks(bits, nbx, nby, rng[i])[0]
        assert [x is not None for x in c] == list(want), f"frame {start + i}"
        assert np.array_equal(want, plan["coded"][start + i])
    cuttable, refused = 0, {"none": 0, "cut": 0}
    for t in range(N):
        kf = kr.key_frame(bits, nbx, nby, rng, t, codes)
        if t in (0, 40, N - 1):   # (with and without the codes handed in)
            assert kf == kr.key_frame(bits, nbx, nby, rng, t)
        if not isinstance(kf, bytes):
            refused[kf[0]] += 1
            assert 0 <= kf[1] < nbx * nby
            continue
        cuttable += 1
        where = f"{bits}-bit {w}x{h} start={start} t={t}"
        assert len(kf) % 2 == 0 and 2 * nbx * nby <= len(kf) <= nbx * nby * (18 if bits == 16 else 10), where
        o = OracleMSVideo1(bits, w, h, pal)
        o.Preinit(plan["lines"])
        assert o.IsKeyFrame(kf), where
        a = np.full(w * h, POISON, dtype=np.int32)
        assert o.DecompressI(kf, a) == 0, where
        assert np.array_equal(covered(a, w, h), covered(truth[start + t][0], w, h)), where
        b = a.copy()
        nxt = start + t + 1
        if keys[nxt]:
            assert o.DecompressI(frames[nxt], b) == 0, where
        else:
            o.DecompressP(frames[nxt], b)
        pic = o.PreviousFrame()   # (a frame that codes nothing leaves the picture where it was)
        assert np.array_equal(covered(pic, w, h), covered(truth[nxt][0], w, h)), where + " and the frame after it"
        o.close()
    want_cut, want_refused, kind = EXPECTED[(bits, start)]
    assert cuttable == want_cut and sum(refused.values()) == want_refused, (cuttable, refused)
    assert cuttable > 0 and (kind is None or refused[kind] == want_refused)


def test_codes_of_lengths_and_cuts():
    """The three lengths of both depths, and each way the end cuts a code off: half a code word, a code word without the colour word
    that settles its length (16-bit), a code without its last byte."""
    solid16, two16 = bytes([0x10, 0x90]), bytes([0x5A, 0x5A, 1, 2, 3, 4])
    eight16 = bytes([0x34, 0x12, 1, 0x82]) + bytes(14)
    full = solid16 + two16 + eight16
    assert kr.codes_of(16, 3, 1, full + bytes(20)) == [(0, 2), (2, 6), (8, 18)]
    assert kr.codes_of(16, 3, 1, full) == [(0, 2), (2, 6), (8, 18)]
    assert kr.codes_of(16, 3, 1, full[:-1]) == [(0, 2), (2, 6), "cut"]            # an odd end: the last word is half there
    assert kr.codes_of(16, 3, 1, full[:11]) == [(0, 2), (2, 6), "cut"]            # the colour word is missing: the length is not settled
    assert kr.codes_of(16, 3, 1, full[:8]) == [(0, 2), (2, 6), "cut"]             # wholly past the end
    assert kr.codes_of(16, 3, 1, full[:7]) == [(0, 2), "cut", "cut"]
    assert kr.codes_of(16, 3, 1, bytes([1, 0x84]) + full)[:1] == [None]            # a skip code is no code of the block
    solid8, two8, eight8 = bytes([7, 0x80]), bytes([0x5A, 0x5A, 1, 2]), bytes([0x34, 0x92]) + bytes(8)
    full = solid8 + two8 + eight8
    assert kr.codes_of(8, 3, 1, full) == [(0, 2), (2, 4), (6, 10)]
    assert kr.codes_of(8, 3, 1, full[:-1]) == [(0, 2), (2, 4), "cut"]
    assert kr.codes_of(8, 3, 1, full[:7]) == [(0, 2), (2, 4), "cut"]              # half a code word
    assert kr.codes_of(8, 3, 1, full[:5]) == [(0, 2), "cut", "cut"]
    assert kr.codes_of(8, 3, 1, solid8 + bytes(2) + full) == [(0, 2), None, None]   # the end marker
    assert kr.key_frame(8, 3, 1, [full, bytes([1, 0x84]) + two8 + bytes([1, 0x84])], 1) == solid8 + two8 + eight8
    assert kr.key_frame(8, 3, 1, [solid8 + bytes(2), full[:7]], 0) == ("none", 1)
    assert kr.key_frame(8, 3, 1, [full, full[:7]], 1) == ("cut", 2)
