"""The rule of the MSVideo1 16-bit encoder (include/jsplayer_amd.h, "Encode"), stated in plain Python (tests/msv1_encode_ref.py) and
pinned to the oracle: every promise of the header, with OracleMSVideo1 as the decoder.  D(P) is the oracle's decode of Key(P).
Needs no GPU; tests/test_msv1_encode_gpu.py holds the kernels to this reference byte for byte."""
import os
import re

import numpy as np
import pytest

import msv1_encode_ref as er
from index_delta_ref import skip_word, walk
from oracle_binding import OracleMSVideo1

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(4, 4), (22, 9), (64, 32), (260, 132)]


def covered(pic, w, h):
    return np.asarray(pic).reshape(h, w)[:(h >> 2) * 4, :(w >> 2) * 4].astype(np.uint32)


def decode_sequence(w, h, frames):
    """The oracle's pictures of a key frame and the inter frames behind it: what the decoder calls the current picture after each."""
    orc = OracleMSVideo1(16, w, h)
    bufs = [np.zeros(w * h, dtype=np.int32) for _ in range(3)]
    out = []
    for t, data in enumerate(frames):
        dst = next(b for b in bufs if b is not orc.PreviousFrame())
        if t == 0:
            assert orc.IsKeyFrame(data), "the first frame must be a key frame"
            assert orc.DecompressI(data, dst) == 0
            out.append(covered(dst.view(np.uint32), w, h).copy())
        else:
            shown, _ = orc.DecompressP(data, dst)
            out.append(covered(shown.view(np.uint32), w, h).copy())
    return out


def D(w, h, pic):
    return decode_sequence(w, h, [er.key(pic, w, h)])[0]


def quantised(pic, w, h):
    c = covered(pic, w, h)
    return ((c >> 3) & 0x1F) | ((c >> 6) & 0x3E0) | ((c >> 9) & 0x7C00)


@pytest.mark.parametrize("w,h", SIZES)
def test_exact_pictures_come_back_as_they_are(w, h):
    rng = np.random.default_rng(w * 1000 + h)
    pic = er.exact_picture(rng, w, h)
    data = er.key(pic, w, h)
    nb = (w >> 2) * (h >> 2)
    codes, skips, blocks = walk(16, data)
    assert blocks == nb and not skips and len(data) <= nb * 18
    want = er.from_rgb15(quantised(pic, w, h))
    assert np.array_equal(want, covered(pic, w, h) & 0x00F8F8F8)
    assert np.array_equal(D(w, h, pic), want)
    if nb >= 6:   # every kind of block is there, by construction
        lengths = [length for _, _, length in codes[:6]]
        assert lengths == [2, 6, 6, 6, 18, 18]
        assert data[codes[1][1]:codes[1][1] + 2] == b"\x00\x00"                         # red field 1: the two-colour code of one colour
        v15 = lambda i: er.q(er.blocks_of(pic, w, h)[i][15])
        for i in (2, 3):                                                                # B = v[15], whichever side it is on
            at = codes[i][1]
            word, A, B = (int.from_bytes(data[at + k:at + k + 2], "little") for k in (0, 2, 4))
            assert B == v15(i) and not word & 0x8000 and not A & 0x8000 and (A < B) == (i == 2)


@pytest.mark.parametrize("w,h", SIZES)
def test_lossy_pictures_settle_after_one_pass(w, h):
    rng = np.random.default_rng(w * 7 + h)
    for pic in (er.lossy_picture(rng, w, h), er.directed_picture(w, h)):
        once = D(w, h, pic)
        full = np.zeros((h, w), dtype=np.uint32)
        full[:once.shape[0], :once.shape[1]] = once
        assert np.array_equal(D(w, h, full), once)                    # D(D(P)) == D(P)
        assert er.key(full, w, h) == er.key(full | np.uint32(0xFF070707), w, h)   # no bit that q drops is read


def test_the_corners_of_the_lossy_step():
    v = [0] * 16
    for n, k in enumerate(er.QUADS[0]):
        v[k] = er.EQUAL_Y[n]
    F, S, bits = er.quadrant(v, 0)
    assert bits == 0 and F == S == er.rgb(2, 1, 1)        # sums (6, 3, 4) + 2, over 4: nobody is high, one group
    for n, k in enumerate(er.QUADS[3]):
        v[k] = er.LAST_ALONE[n]
    F, S, bits = er.quadrant(v, 3)
    assert S == er.rgb(31, 31, 31) and F == 0 and bits == (1 << 10) | (1 << 11) | (1 << 14)   # (1 + 1) // 3 == 0 per channel
    for n, k in enumerate(er.QUADS[2]):
        v[k] = er.LAST_ALONE_LOW[n]
    F, S, bits = er.quadrant(v, 2)
    assert S == er.rgb(0, 0, 1) and F == er.rgb(31, 31, 31) and bits == (1 << 8) | (1 << 9) | (1 << 12)   # (92 + 1) // 3 == 31
    for n, k in enumerate(er.QUADS[1]):
        v[k] = er.THREE[n]
    F, S, bits = er.quadrant(v, 1)
    # Y = 36, 36, 33, 63; T = 168: only the last pixel is high
    assert S == er.rgb(1, 30, 2) and F == er.rgb((9 + 9 + 20 + 1) // 3, (9 + 9 + 3 + 1) // 3, (9 + 9 + 7 + 1) // 3) and bits == 0b1001100


def clip(w, h, seed):
    """Pictures P0 .. P5 and what each gap is: nothing, dropped bits only, every block, some blocks, some blocks of a lossy picture."""
    rng = np.random.default_rng(seed)
    nb = (w >> 2) * (h >> 2)
    p0 = er.exact_picture(rng, w, h)
    p1 = p0.copy()
    p2 = er.change_blocks(rng, p1, w, range(nb), dropped_bits_only=True)
    p3 = er.change_blocks(rng, p2, w, range(nb))
    some = sorted(set(int(b) for b in rng.integers(0, nb, size=max(1, nb // 5))))
    p4 = er.change_blocks(rng, p3, w, some)
    p5 = er.lossy_picture(rng, w, h)
    p5[:8] = p4[:8]
    return [p0, p1, p2, p3, p4, p5], some


@pytest.mark.parametrize("w,h", SIZES)
def test_a_clip_decodes_to_D_of_every_picture(w, h):
    pics, some = clip(w, h, w + h)
    nb = (w >> 2) * (h >> 2)
    frames = [er.key(pics[0], w, h)] + [er.inter(a, b, w, h) for a, b in zip(pics, pics[1:])]
    shown = decode_sequence(w, h, frames)
    for t, pic in enumerate(pics):
        assert np.array_equal(shown[t], D(w, h, pic)), t
    nothing = b"".join(skip_word(min(1023, nb - at)) for at in range(0, nb, 1023))
    assert frames[1] == nothing and frames[2] == nothing                      # a gap that changes nothing / only bits q drops
    assert frames[3] == er.key(pics[3], w, h)                                 # every block coded: the key frame, byte for byte
    codes, skips, blocks = walk(16, frames[4])
    assert [b for b, _, _ in codes] == some and blocks == nb
    for a, b, f in zip(pics, pics[1:], frames[1:]):
        assert len(f) <= len(er.key(b, w, h))
        assert OracleMSVideo1(16, w, h).IsKeyFrame(f) == all(er.coded_blocks(a, b, w, h))


def test_equal_quantised_blocks_encode_alike_whatever_the_words():
    w, h = 22, 9
    rng = np.random.default_rng(5)
    pic = er.lossy_picture(rng, w, h)
    assert er.key(pic, w, h) == er.key(pic ^ np.uint32(0x12070707), w, h)


@pytest.mark.parametrize("wrong", er.WRONG)
def test_each_wrong_rule_misses(wrong):
    w, h = 64, 32
    pics, _ = clip(w, h, 11)
    right = [er.key(pics[0], w, h)] + [er.inter(a, b, w, h) for a, b in zip(pics, pics[1:])]
    bad = [er.key(pics[0], w, h, wrong)] + [er.inter(a, b, w, h, wrong) for a, b in zip(pics, pics[1:])]
    assert bad != right
    if wrong == "compare_words":      # the pictures are right, a promise is not: a gap that changes nothing visible is not skipped
        assert bad[2] == er.key(pics[2], w, h) and len(bad[2]) > len(right[2])
        return
    orc = OracleMSVideo1(16, w, h)
    dst = np.zeros(w * h, dtype=np.int32)
    rc = orc.DecompressI(bad[0], dst) if orc.IsKeyFrame(bad[0]) else -1
    assert rc != 0 or not np.array_equal(covered(dst.view(np.uint32), w, h), covered(pics[0], w, h) & 0x00F8F8F8)


def test_the_header_states_the_rule_and_the_binding_has_the_calls():
    from jsplayer_amd import _native as N
    from jsplayer_amd import codec
    header = open(os.path.join(ROOT, "include", "jsplayer_amd.h")).read()
    for name in ("jsp_msv1_encoder_create", "jsp_msv1_encoder_destroy", "jsp_msv1_encode_bound", "jsp_msv1_encode_frames"):
        assert name in N.SIGNATURES and re.search(r"^[a-z_ ]+\*? ?%s\(" % name, header, re.M), name
    assert "((p >> 3) & 0x1F) | ((p >> 6) & 0x3E0) | ((p >> 9) & 0x7C00)" in header and "MSVideo1.hx:119-181" in header
    assert hasattr(codec.Msv1Encoder, "EncodeFrames") and hasattr(codec.Msv1Encoder, "Bound") and hasattr(codec.Msv1Encoder, "close")


def test_sizes_are_refused_before_any_device_is_looked_for():
    from jsplayer_amd import CodecError, Msv1Encoder
    for w, h in ((3, 4), (4, 3), (16385, 4), (4, 16385), (0, 0)):
        with pytest.raises(CodecError, match=r"^msv1_encode: width and height"):
            Msv1Encoder(w, h)
