"""Which refusal jsp_display_present and jsp_display_present_area give, word for word, and which of two wins.

The GPU tests of the two calls (test_present_gpu.py, test_present_area_gpu.py: test_every_refusal_leaves_out_alone) ask for the
prefix of the message only.  Here every bad argument of their lists has its full message, and every pair of them that fails two
different checks has the message of the EARLIER check: the order below is the order of the checks in the two entry points.
Every case is refused before any HIP call, so `frame` and `out` are small integers that nothing dereferences."""
import itertools
import math

import pytest

from jsplayer_amd import _native as N


def _gpu_visible():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


pytestmark = pytest.mark.skipif(
    _gpu_visible(), reason="frame and out are made-up addresses: were a case accepted by mistake, a kernel would run on them. "
                           "With a GPU the refusals are tested on real buffers (test_present_gpu.py, test_present_area_gpu.py)")

FW, FH, WW, WH = 20, 12, 16, 8
GOOD = dict(frame=64, fw=FW, fh=FH, out=128, ww=WW, wh=WH, pitch=WW, k=1.0, dx=0.0, dy=0.0, mode=0, filter=1)

NULL = "null pointer"
FRAME = "frame size outside 1..16384"
WINDOW = "window size outside 1..16384"
PITCH = "out_pitch below win_w"
FINITE = "k, dx, dy must be finite"
K_RANGE = "k outside 1/64..64"
MODE = "unknown mode"
FILTER = "unknown filter"

# (argument change, message), in the order of the checks: both calls check in this order, the area call has no filter
ORDER = [
    (dict(frame=None), NULL), (dict(out=None), NULL),
    (dict(fw=0), FRAME), (dict(fw=-1), FRAME), (dict(fw=16385), FRAME), (dict(fh=0), FRAME), (dict(fh=16385), FRAME),
    (dict(ww=0), WINDOW), (dict(ww=16385, pitch=16385), WINDOW), (dict(wh=0), WINDOW), (dict(wh=-2), WINDOW), (dict(wh=16385), WINDOW),
    (dict(pitch=WW - 1), PITCH), (dict(pitch=0), PITCH),
    (dict(k=math.nan), FINITE), (dict(k=math.inf), FINITE),
    (dict(dx=math.nan), FINITE), (dict(dx=math.inf), FINITE), (dict(dy=math.nan), FINITE), (dict(dy=-math.inf), FINITE),
    (dict(k=1.0 / 65), K_RANGE), (dict(k=64.5), K_RANGE), (dict(k=0.0), K_RANGE), (dict(k=-1.0), K_RANGE),
    (dict(mode=-1), MODE), (dict(mode=4), MODE),
    (dict(filter=-1), FILTER), (dict(filter=2), FILTER),
]


def _present(a):
    return N.lib().jsp_display_present(a["frame"], a["fw"], a["fh"], a["out"], a["ww"], a["wh"], a["pitch"], a["k"], a["dx"], a["dy"],
                                       a["mode"], a["filter"], 0xFF000000, None)


def _present_area(a):
    return N.lib().jsp_display_present_area(a["frame"], a["fw"], a["fh"], a["out"], a["ww"], a["wh"], a["pitch"], a["k"], a["dx"], a["dy"],
                                            a["mode"], 0xFF000000, None)


CALLS = {
    "display_present": (_present, ORDER),
    "display_present_area": (_present_area, [(change, why) for change, why in ORDER if why != FILTER]),
}


def _refused_with(call, prefix, change, why):
    assert call(dict(GOOD, **change)) == N.JSP_ERROR_OCCURED, change
    assert N.last_error() == f"{prefix}: {why}", change


@pytest.mark.parametrize("prefix", CALLS)
def test_every_bad_argument_has_its_message(prefix):
    call, order = CALLS[prefix]
    for change, why in order:
        _refused_with(call, prefix, change, why)


@pytest.mark.parametrize("prefix", CALLS)
def test_of_two_bad_arguments_the_earlier_check_refuses(prefix):
    call, order = CALLS[prefix]
    pairs = 0
    for (first, why), (second, other) in itertools.combinations(order, 2):      # `first` is checked before `second`
        if why == other or set(first) & set(second):
            continue
        _refused_with(call, prefix, {**first, **second}, why)
        pairs += 1
    assert pairs >= 200     # (28 or 26 changes in 8 or 7 checks: most pairs count)


def test_the_lists_are_those_of_the_gpu_tests():
    """Every bad argument of test_every_refusal_leaves_out_alone (both files) is in ORDER: the same 28, and 26 without the filter."""
    assert len(ORDER) == 28 and len(CALLS["display_present_area"][1]) == 26
    assert [why for _, why in ORDER] == sorted((why for _, why in ORDER), key=[NULL, FRAME, WINDOW, PITCH, FINITE, K_RANGE, MODE, FILTER].index)
