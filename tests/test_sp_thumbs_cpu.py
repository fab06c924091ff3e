"""Thumbnails of a ScreenPressor seek index, the parts that need no GPU: the two calls are in the C ABI and its ctypes table,
SpScrubIndex has the methods of SeekIndex, and the thumbnail of what the index composes (tests/sp_index_ref.Composer, fed by the
product's host stage) is the thumbnail of the oracle's picture — for 16 bpp with every byte a 5-bit mean.

One thing the 16-bpp rule has to say about the reference: a FLAT 16-bpp key frame fills the picture with its components already
shifted left by 3 (ScreenPressor.hx:134-139), so its bytes reach 248 — in the frame, hence in its thumbnail, and in the inter frames
on top of it where they leave it showing.  A byte's mean never exceeds the bytes it is the mean of, which is what holds for every
frame; "at most 31" holds for every frame of a clip without flat key frames, and that is asserted on such a clip."""
import inspect
import os
import re

import numpy as np
import pytest

import sp_index_ref as ref
import thumbs_ref as tr
from jsplayer_amd import _native as N
from jsplayer_amd import codec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_two_calls_are_in_the_abi_table_and_declared_in_the_header():
    header = open(os.path.join(ROOT, "include", "jsplayer_amd.h")).read()
    for name in ("jsp_sp_index_thumb_size", "jsp_sp_index_thumbs"):
        assert name in N.SIGNATURES, name
        assert re.search(r"^int %s\(" % name, header, re.M), name + " is not declared in the header"
    assert N.SIGNATURES["jsp_sp_index_thumb_size"] == N.SIGNATURES["jsp_index_thumb_size"]
    assert N.SIGNATURES["jsp_sp_index_thumbs"] == N.SIGNATURES["jsp_index_thumbs"]


def test_sp_scrub_index_has_the_methods_of_seek_index():
    for name in ("ThumbSize", "Thumbs"):
        assert hasattr(codec.SpScrubIndex, name), name
        assert inspect.signature(getattr(codec.SpScrubIndex, name)) == inspect.signature(getattr(codec.SeekIndex, name))
    assert codec.SpScrubIndex.ThumbSize is codec.SeekIndex.ThumbSize and codec.SpScrubIndex.Thumbs is codec.SeekIndex.Thumbs   # shared, not copied
    assert codec.SpScrubIndex._THUMB_CALLS == ("sp_index_thumb_size", "sp_index_thumbs")
    assert codec.SeekIndex._THUMB_CALLS == ("index_thumb_size", "index_thumbs")


@pytest.mark.parametrize("w,h,s", [(37, 23, 4), (37, 23, 8), (37, 23, 16), (100, 52, 8), (1920, 1080, 16), (12, 4, 4), (320, 240, 4)])
def test_whole_squares_of_the_picture_is_the_msvideo1_formula_at_these_scales(w, h, s):
    assert tr.thumb_size(w, h, s) == (w // s, h // s)


@pytest.mark.parametrize("case", [(48, 100, 52, 30, 24, 4, 11, 7),
                                  (49, 37, 23, 30, 16, 3, 0, 5),     # 16 bpp, coded key frame only: every byte of every picture is 5 bits
                                  (50, 37, 23, 30, 16, 3, 11, 5)],   # 16 bpp with flat key frames (see the module docstring)
                         ids=lambda c: "cfg%d_%dx%d_%dbpp_v%d_k%d" % (c[0], c[1], c[2], c[4], c[5], c[6]))
def test_thumbnail_of_the_composition_is_the_thumbnail_of_the_oracles_picture(case):
    cfg, w, h, n, bpp, version, key_every, key_row = case
    clip = ref.make_clip(cfg, w, h, n, bpp, version, key_every, key_row)
    pictures, _ = ref.oracle_run(clip)
    comp = ref.Composer(clip)
    for t in range(n):
        for s in tr.SCALES:
            got = tr.thumbnail(comp.picture(t), w, h, s)
            assert got.shape == (h // s, w // s)
            assert np.array_equal(got, tr.thumbnail(pictures[t], w, h, s)), f"frame {t} scale {s}"
            assert int(got.view(np.uint8).max()) <= int(pictures[t].view(np.uint8).max()), f"frame {t} scale {s}"
            if bpp == 16 and key_every == 0:   # one 5-bit component per byte (streamgen.py, Manager.hx:362-370): so is its mean
                assert int(got.view(np.uint8).max()) <= 31, f"frame {t} scale {s}"
