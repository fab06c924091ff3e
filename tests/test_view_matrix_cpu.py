"""jsp_view_matrix (Main.on_stage_resize's display matrix, Main.hx:301-315) through the library, without a GPU: known answers, the
fit() quirk, exact agreement with tests/view_ref.py and every refusal."""
import ctypes as C
import math
import re
import os

import numpy as np
import pytest

import view_ref as vr
from jsplayer_amd import _native as N
from jsplayer_amd import codec as cm


def vm(fw, fh, ww, wh, zoom, hor=0.5, ver=0.5):
    return cm.view_matrix(fw, fh, ww, wh, zoom, hor, ver)


def test_known_answers_1080p_in_a_720p_window():
    assert vm(1920, 1080, 1280, 720, 0) == (2 / 3, 0.0, 0.0)                     # Fit
    assert vm(1920, 1080, 1280, 720, 2, 0.5, 0.5) == (2.0, 1280.0, 720.0)
    assert vm(1920, 1080, 1280, 720, 2, 0.0, 0.5)[1] == 0.0
    assert vm(1920, 1080, 1280, 720, 2, 1.0, 0.5)[1] == 2560.0
    assert vm(1920, 1080, 1280, 720, 2, 0.5, 1.0)[2] == 0.0
    assert vm(1920, 1080, 1280, 720, 2, 0.5, 0.0)[2] == 1440.0
    # Fit ignores the view positions, and takes the smaller of the two ratios
    assert vm(1920, 1080, 1280, 720, 0, 0.0, 1.0) == (2 / 3, 0.0, 0.0)
    assert vm(100, 100, 50, 20, 0) == (0.2, 0.0, 0.0) and vm(100, 100, 20, 50, 0) == (0.2, 0.0, 0.0)


def test_an_odd_window_gives_half_pixel_offsets():
    assert vm(20, 12, 15, 9, 1) == (1.0, 2.5, 1.5)


def test_the_fit_quirk_a_narrow_picture_goes_to_the_right_edge():
    # 37 wide in a 64-wide window at 100 %: mx = 37 - 64 = -27; a = 37 - 32 = 5 is above it -> dx = -27
    k, dx, dy = vm(37, 23, 64, 64, 1, 1.0, 0.5)
    assert (k, dx) == (1.0, -27.0)
    assert vm(37, 23, 64, 64, 1, 0.0, 0.5)[1] == 0.0          # a = -32 < 0 -> 0: the left edge
    assert vm(37, 23, 64, 64, 1, 0.5, 0.0)[2] == 0.0          # a = 23 - 32 = -9 < 0 is tested first -> 0
    assert vm(37, 46, 64, 64, 1, 0.5, 0.0)[2] == -18.0        # a = 46 - 32 = 14 > mx = -18 -> -18


def test_sweep_equals_the_reference_exactly():
    rng = np.random.default_rng(20)
    n = 0
    for _ in range(400):
        fw, fh, ww, wh = (int(v) for v in rng.integers(1, 4000, size=4))
        zoom = [0.0, 1.0, 2.0, float(rng.uniform(0.01, 8.0)), float(rng.integers(1, 9)) / 3][int(rng.integers(0, 5))]
        hor, ver = (float(rng.uniform(0, 1)) if rng.random() < 0.8 else float(rng.choice([0.0, 1.0, 1.5])) for _ in range(2))
        got, want = vm(fw, fh, ww, wh, zoom, hor, ver), vr.view_matrix(fw, fh, ww, wh, zoom, hor, ver)
        assert got == want, (fw, fh, ww, wh, zoom, hor, ver, got, want)
        n += got[1] != 0 or got[2] != 0
    assert n > 100                                            # (the sweep is not all Fit / clamped to 0)


@pytest.mark.parametrize("args", [
    (0, 12, 15, 9, 1.0, 0.5, 0.5), (20, 0, 15, 9, 1.0, 0.5, 0.5), (20, 12, 0, 9, 1.0, 0.5, 0.5), (20, 12, 15, 0, 1.0, 0.5, 0.5),
    (-3, 12, 15, 9, 0.0, 0.5, 0.5), (20, 12, 15, -1, 0.0, 0.5, 0.5),
    (20, 12, 15, 9, -1.0, 0.5, 0.5), (20, 12, 15, 9, math.nan, 0.5, 0.5), (20, 12, 15, 9, math.inf, 0.5, 0.5),
    (20, 12, 15, 9, 1.0, -0.1, 0.5), (20, 12, 15, 9, 1.0, math.nan, 0.5), (20, 12, 15, 9, 1.0, math.inf, 0.5),
    (20, 12, 15, 9, 1.0, 0.5, -0.1), (20, 12, 15, 9, 1.0, 0.5, math.nan), (20, 12, 15, 9, 1.0, 0.5, -math.inf),
])
def test_refusals_leave_the_outputs_alone(args):
    lib = N.lib()
    k, dx, dy = C.c_double(-7.0), C.c_double(-8.0), C.c_double(-9.0)
    assert lib.jsp_view_matrix(*args, C.byref(k), C.byref(dx), C.byref(dy)) == N.JSP_ERROR_OCCURED
    assert N.last_error().startswith("view_matrix:")
    assert (k.value, dx.value, dy.value) == (-7.0, -8.0, -9.0)
    with pytest.raises(cm.CodecError, match="^view_matrix:"):
        cm.view_matrix(*args)


def test_null_outputs_are_refused_and_nothing_is_written():
    lib = N.lib()
    good = (20, 12, 15, 9, 1.0, 0.5, 0.5)
    for missing in range(3):
        vals = [C.c_double(-7.0), C.c_double(-8.0), C.c_double(-9.0)]
        ptrs = [C.byref(v) for v in vals]
        ptrs[missing] = None
        assert lib.jsp_view_matrix(*good, *ptrs) == N.JSP_ERROR_OCCURED
        assert N.last_error().startswith("view_matrix:")
        assert [v.value for v in vals] == [-7.0, -8.0, -9.0]
    k, dx, dy = C.c_double(), C.c_double(), C.c_double()
    assert lib.jsp_view_matrix(*good, C.byref(k), C.byref(dx), C.byref(dy)) == 0 and (k.value, dx.value, dy.value) == (1.0, 2.5, 1.5)


def test_python_constants_follow_the_kernel_source():
    """codec.PRESENT_SPAN_X / PRESENT_BAND_ROWS (what the GPU tests size their windows by) restate the kernel's constants."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "jsplayer_amd", "csrc", "present_kernels.hip")).read()
    val = lambda name: int(re.search(r"constexpr int %s = (\d+);" % name, text).group(1))
    assert cm.PRESENT_SPAN_X == val("kPresentLanes") * val("kPresentRun")
    assert cm.PRESENT_BAND_ROWS == val("kPresentBandRows")
    assert (cm.PRESENT_NEAREST, cm.PRESENT_BILINEAR) == (0, 1)
