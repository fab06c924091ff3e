"""sp_index_thumbs_kernel at ties, at saturation and next to zeros, on an MI355X: the ScreenPressor chart clips of
tests/thumbs_charts.py (24 and 16 bpp; 48x32, whole blocks and the vector path; 37x23, partial blocks and the scalar path).

The random clips of test_sp_index_thumbs_gpu.py meet an exact tie or a cell of all-255 bytes only by chance; the kernel rounds both
fields of its packed R/B word at once (S * S / 2 * 0x00010001) and cuts each to a byte after the shift.  Here every scale sees ties
over even and odd quotients, cells one step either side of the half, and all-maximum cells against all-zero ones.

Truth: tests/thumbs_ref.py over the pictures of sp_index_ref.oracle_run (which are also the encoder's).  Everything is bit-exact."""
from functools import lru_cache

import numpy as np
import pytest

import sp_index_ref as ref
import thumbs_charts as tc
import thumbs_ref as tr
from test_sp_index_thumbs_gpu import check, make_sp

pytestmark = pytest.mark.gpu


@lru_cache(maxsize=None)
def oracle(name):
    """The oracle's pictures of the clip, once a process; nobody changes them."""
    return ref.oracle_run(tc.sp_chart_clip(name), preinit=tc.SP_KEY_ROW)[0]


@pytest.mark.parametrize("name", tc.SP_NAMES)
def test_chart_clips_every_frame_every_scale(name):
    clip = tc.sp_chart_clip(name)
    w, h, top = clip.w, clip.h, tc.sp_values(clip.bpp)["top"]
    pictures = oracle(name)
    for t, pic in enumerate(pictures):
        assert np.array_equal(pic, clip.frames[t]), f"{clip.name}: frame {t} is not the encoder's picture"
    # what the reference holds, before the kernel is asked
    bright = tc.sp_values(clip.bpp)["word_bright"]
    for s in tr.SCALES:
        per = [tc.census(p, w, h, s, top) for p in pictures]
        for ch in "rgb":
            assert all(sum(c[ch][k] for c in per) > 0 for k in ("tie", "below", "above", "full")), (s, ch)
        ex = tr.thumbnail(pictures[tc.EXTREMES_AT], w, h, s).view(np.uint32)
        assert per[tc.EXTREMES_AT]["full_beside_zero"] and np.any(ex == bright) and np.any(ex == 0), s
    gpu = make_sp(clip, lines=tc.SP_KEY_ROW)
    idx = gpu.BuildScrubIndex(clip.chunks, clip.keys, key_row=tc.SP_KEY_ROW)
    picks = [4, 0, 3, 1, 2, 3, 0]
    for s in tr.SCALES:
        for cols in (1, 3):
            check(idx, pictures, picks, w, h, s, cols, f"{clip.name} s={s} cols={cols}")
    assert gpu.PreviousFrame() is None
    idx.close()
    gpu.StopAndClean()
