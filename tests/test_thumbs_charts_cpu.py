"""The chart clips of tests/thumbs_charts.py hold what they are made for — asserted from decoded pictures, not from what the painter
meant — and five named wrong formulas each miss the reference on them.  No GPU.

The pictures: the MSVideo1 charts decoded by the pure-Python decoder (pyref_msv1.decode), the ScreenPressor ones the encoder's own."""
from functools import lru_cache

import numpy as np
import pytest

import pyref_msv1 as py
import thumbs_charts as tc
import thumbs_ref as tr
from oracle_binding import OracleMSVideo1

MSV1 = [(bits, w, h) for bits in (16, 8) for w, h in tc.MSV1_SIZES]


def msv1_id(c):
    return f"{c[0]}bit_{c[1]}x{c[2]}"


@lru_cache(maxsize=None)
def msv1_pictures(bits, w, h):
    """pyref_msv1.decode over the chart clip, zero-started: uint32 pictures."""
    frames, keys, pal = tc.msv1_chart_clip(bits, w, h)
    palette = py.palette_ints(pal) if pal else None
    prev, out = np.zeros((h, w), np.int64), []
    for src in frames:
        prev, coded, _ = py.decode(bits, w, h, src, prev=prev, palette=palette, dst=prev)
        assert coded
        out.append(prev.astype(np.uint32).reshape(-1))
    return out


def oracle_pictures(bits, w, h):
    frames, keys, pal = tc.msv1_chart_clip(bits, w, h)
    o = OracleMSVideo1(bits, w, h, pal)
    o.Preinit(36)
    bufs = [np.zeros(w * h, dtype=np.int32) for _ in range(3)]
    out = []
    for src, key in zip(frames, keys):
        prev = o.PreviousFrame()
        dst = next(b for b in bufs if b is not prev)
        if prev is not None:
            np.copyto(dst, prev)
        if key:
            assert o.DecompressI(src, dst) == 0
        else:
            o.DecompressP(src, dst)
        assert o.PreviousFrame() is dst
        out.append(dst.view(np.uint32).copy())
    o.close()
    return out


def chart_sets():
    """(name, w, h, top, eight_bit_msv1, pictures) of every chart clip of both codecs."""
    for bits, w, h in MSV1:
        yield msv1_id((bits, w, h)), w, h, tc.msv1_values(bits)["top"], bits == 8, msv1_pictures(bits, w, h)
    for name in tc.SP_NAMES:
        w, h, bpp, _ = tc.SP_SPECS[name]
        yield "sp_" + name, w, h, tc.sp_values(bpp)["top"], False, tc.sp_chart_clip(name).frames


@pytest.mark.parametrize("case", MSV1, ids=msv1_id)
def test_the_decoded_charts_are_the_masks_and_both_decoders_agree(case):
    """pyref_msv1 and the oracle agree word for word, TOP BYTE INCLUDED: neither masks a palette word (the codec does not either:
    Preinit copies the palette's words whole), so the 8-bit chart itself carries the 0xFF top byte of colour A to the kernel."""
    bits, w, h = case
    mine, theirs, meant = msv1_pictures(bits, w, h), oracle_pictures(bits, w, h), tc.msv1_chart_pictures(bits, w, h)
    assert len(mine) == len(theirs) == len(meant) == len(tc.FRAME_NAMES)
    for name, a, b, c in zip(tc.FRAME_NAMES, mine, theirs, meant):
        assert np.array_equal(a, b), f"{name}: pyref_msv1 and the oracle differ"
        assert np.array_equal(a, c), f"{name}: not the picture the masks describe"
    v = tc.msv1_values(bits)
    nb = (w // 4) * (h // 4)
    for c, pic in zip(tc.CHARTS, mine):
        # every cell holds its rung: A-pixels per whole cell
        tw, th = tr.thumb_size(w, h, c)
        if tw > 0 and th > 0:
            got = (pic.reshape(h, w)[:th * c, :tw * c] == v["word_a"]).reshape(th, c, tw, c).sum(axis=(1, 3))
            ncx = -(-(w // 4) // (c // 4))
            cy, cx = np.mgrid[0:th, 0:tw]
            assert np.array_equal(got, np.asarray(tc.LADDER[c])[(cy * ncx + cx) % len(tc.LADDER[c])])
        assert tc.block_counts(w, h, c).max() <= 15 and tc.block_counts(w, h, c).size == nb
    if bits == 8:
        assert any(int(p.max()) >> 24 == 0xFF for p in mine[:3])


@pytest.mark.parametrize("name", tc.SP_NAMES)
def test_the_screenpressor_charts_paint_a_where_the_msvideo1_charts_set_the_flag(name):
    w, h, bpp, _ = tc.SP_SPECS[name]
    clip = tc.sp_chart_clip(name)
    v, m = tc.sp_values(bpp), tc.msv1_values(8)
    assert clip.keys == [True, True, True, True, False] and all(len(c) > 0 for c in clip.chunks)
    grid = np.zeros((h, w), dtype=bool)
    grid[:4 * (h // 4), :4 * (w // 4)] = True
    for t, twin in enumerate(tc.msv1_chart_pictures(8, w, h)[:4]):
        sp, twin = clip.frames[t].reshape(h, w), twin.reshape(h, w)
        a = (v["word_a"], m["word_a"]) if t < 3 else (v["word_bright"], m["word_bright"])
        assert np.array_equal((sp == a[0]) & grid, twin == a[1]), tc.FRAME_NAMES[t]
    x1, y1, x2, y2 = tc.SP_RECT
    changed = (clip.frames[4] != clip.frames[3]).reshape(h, w)
    ys, xs = np.nonzero(changed)
    assert {(int(y) // 16, int(x) // 16) for y, x in zip(ys, xs)} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert ys.min() >= y1 and ys.max() < y2 and xs.min() >= x1 and xs.max() < x2


def test_census_conditions_hold_for_every_chart_clip_at_every_valid_scale():
    """Over the union of a clip's frames, per channel: a tie, a cell below the half, a cell above it; an all-maximum cell next to an
    all-zero one; 8-bit MSVideo1: the top byte set somewhere.

    One (format, scale) cannot hold a cell off the half: MSVideo1 16-bit at s = 4.  Every RGB555 byte is a multiple of 8, so a sum
    of 16 of them is a multiple of 8 and its remainder mod 16 is 0 or 8 — exact or a tie, nothing else exists.  There the condition
    is a tie and an exact cell per channel, and that no other remainder occurs."""
    seen = 0
    for name, w, h, top, eight, pictures in chart_sets():
        scales = tc.valid_scales(w, h)
        assert scales == ((4, 8) if (w, h) == (12, 520) else (4, 8, 16)), name
        for s in scales:
            per = [tc.census(p, w, h, s, top) for p in pictures]
            for ch in "rgb":
                tie, below, above = (sum(c[ch][k] for c in per) for k in ("tie", "below", "above"))
                assert tie > 0, f"{name} s={s} {ch}: no tie"
                if top == 248 and s == 4:
                    tw, th = tr.thumb_size(w, h, s)
                    assert below == 0 and above == 0 and tie < len(per) * tw * th, f"{name} s={s} {ch}"
                else:
                    assert below > 0 and above > 0, f"{name} s={s} {ch}: below {below}, above {above}"
                assert sum(c[ch]["full"] for c in per) > 0, f"{name} s={s} {ch}: no saturated cell"
            assert per[tc.EXTREMES_AT]["full_beside_zero"], f"{name} s={s}: no all-maximum cell next to an all-zero one"
            assert any(c["top_byte"] for c in per) == eight, f"{name} s={s}: top byte"
            seen += 1
    assert seen == 2 * (3 + 3 + 2) + 4 * 3


# ---- five wrong formulas, beside thumbs_ref.thumbnail ---------------------------------------------------------------------------
def wrong_thumbnail(picture, w, h, s, how):
    """thumbs_ref.thumbnail with one named mistake.
    truncate      no rounding term
    half_even     a tie goes to the even neighbour
    half_less_1   rounding term s * s / 2 - 1
    unmasked_rb   R and B summed in one 32-bit word under 0xFFFF00FF: the top byte is added into R's field
    wrap16_twice  the rounding term added twice to a field that wraps at 2^16, the quotient cut to a byte"""
    tw, th = tr.thumb_size(w, h, s)
    pic = np.asarray(picture).reshape(-1).view(np.uint32).reshape(h, w)[:th * s, :tw * s].astype(np.int64)
    n, shift = s * s, {4: 4, 8: 6, 16: 8}[s]
    half = n // 2
    sums = {pos: ((pic >> pos) & 0xFF).reshape(th, s, tw, s).sum(axis=(1, 3)) for pos in (16, 8, 0)}
    if how == "unmasked_rb":
        rb = (pic & 0xFFFF00FF).reshape(th, s, tw, s).sum(axis=(1, 3)) & 0xFFFFFFFF
        sums[16], sums[0] = rb >> 16, rb & 0xFFFF
    out = np.zeros((th, tw), dtype=np.int64)
    for pos, c in sums.items():
        if how == "truncate":
            q = c >> shift
        elif how == "half_even":
            q, rem = c >> shift, c & (n - 1)
            q = q + ((rem > half) | ((rem == half) & (q & 1 == 1)))
        elif how == "half_less_1":
            q = (c + half - 1) >> shift
        elif how == "wrap16_twice":
            q = (((c + 2 * half) & 0xFFFF) >> shift) & 0xFF
        else:
            q = (c + half) >> shift
        out = (out + (q << pos)) & 0xFFFFFFFF
    return out.astype(np.uint32).view(np.int32)


WRONG = ("truncate", "half_even", "half_less_1", "unmasked_rb", "wrap16_twice")


def test_each_named_wrong_formula_misses_the_reference_on_the_charts():
    """Which clips catch which, at EVERY valid scale of the clip:
      truncate, half_even, half_less_1, wrap16_twice   every chart clip of both codecs (a tie over an even quotient is in every one:
                                                       R's lower value is 254, 240 or 30)
      unmasked_rb                                      the 8-bit MSVideo1 clips and no other: only a palette puts a top byte into a
                                                       picture that a stream decodes
    and wrap16_twice turns the saturated cells of the extremes frame — 0x00FFFFFF in the reference — into 0 where the format reaches
    255."""
    for name, w, h, top, eight, pictures in chart_sets():
        for s in tc.valid_scales(w, h):
            want = [tr.thumbnail(p, w, h, s) for p in pictures]
            for how in WRONG:
                differs = [t for t, p in enumerate(pictures) if not np.array_equal(wrong_thumbnail(p, w, h, s, how), want[t])]
                if how == "unmasked_rb" and not eight:
                    assert differs == [], f"{name} s={s} {how}: frames {differs}"
                else:
                    assert differs, f"{name} s={s}: {how} equals the reference on every frame"
                if how in ("half_even", "half_less_1"):       # (they differ on ties only: the charts, not the solid extremes)
                    assert tc.EXTREMES_AT not in differs
            if top == 255:
                ex = pictures[tc.EXTREMES_AT]
                bright = want[tc.EXTREMES_AT].view(np.uint32) == 0x00FFFFFF
                assert bright.any() and (want[tc.EXTREMES_AT] == 0).any()
                assert np.all(wrong_thumbnail(ex, w, h, s, "wrap16_twice").view(np.uint32)[bright] == 0)
    # the formulas are the reference's where nothing is wrong with them: a picture of exact cells without a top byte
    flat = np.full(32 * 32, 0x00102030, dtype=np.uint32)
    for s in tr.SCALES:
        for how in ("truncate", "half_even", "half_less_1", "unmasked_rb"):
            assert np.array_equal(wrong_thumbnail(flat, 32, 32, s, how), tr.thumbnail(flat, 32, 32, s)), how


# ---- the launches of msv1_index_thumbs_kernel at the GPU tests' sizes -----------------------------------------------------------
# (w, h, s): (lanes, workgroups of 256, last one partly filled, a boundary inside a thumbnail row)
LANES = {
    (86, 70, 4): (357, 2, True, True),       # 21 x 17
    (86, 70, 8): (320, 2, True, True),       # 10 x 8, four lanes a pixel: the odd trailing block column and row dropped
    (86, 70, 16): (320, 2, True, True),      # 5 x 4, sixteen lanes a pixel
    (128, 64, 4): (512, 2, False, False),    # two full workgroups, the boundary on a row seam
    (128, 64, 8): (512, 2, False, False),
    (128, 64, 16): (512, 2, False, False),
    (12, 520, 4): (390, 2, True, True),      # 3 x 130
    (12, 520, 8): (260, 2, True, False),     # one output column (every pixel is a row): a wave covers sixteen thumbnail rows
}


def test_lane_counts_of_the_seam_sizes():
    got = {}
    for w, h in tc.MSV1_SIZES:
        for s in tc.valid_scales(w, h):
            l = tc.lanes(w, h, s)
            got[(w, h, s)] = (l["lanes"], l["workgroups"], l["partial_tail"], l["seam_inside_row"])
    assert got == LANES
    assert tr.thumb_size(12, 520, 16)[0] == 0 and tr.thumb_size(12, 520, 8) == (1, 65)
    for s in tr.SCALES:
        rows = [v for (w, h, sc), v in LANES.items() if sc == s]
        assert all(r[1] > 1 for r in rows), s
        assert any(r[2] for r in rows) and any(r[0] % tc.WG == 0 for r in rows), s
        assert any(r[3] for r in rows), s
    # the sizes of tests/test_index_thumbs_gpu.py stay inside one workgroup at every scale: what this file's sizes are for
    for w, h in ((64, 48), (36, 20), (70, 46)):
        assert all(tc.lanes(w, h, s)["workgroups"] == 1 for s in tr.SCALES)
