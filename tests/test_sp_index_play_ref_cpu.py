"""The one claim sp_index_play_kernel rests on, checked without a GPU: carrying a frame's pixels FORWARD (tests/sp_index_play_ref.py:
literal rectangles laid over them, a key picture at a key frame, nothing at an unchanged frame) equals the backward walk of the seek
index at every frame — and so the encoder's pictures and the oracle's sequential run — for the clip shapes of
test_sp_index_ref_cpu.py, from every kind of first frame, across key frames and a bitmap word boundary, at strides 1, 2, 5 and 32."""
import numpy as np
import pytest

import sp_index_play_ref as play_ref
import sp_index_ref as ref
from test_sp_index_ref_cpu import CASES


def _runs(clip):
    """(first, n, stride) to walk: first on and off key frames, runs that cross one and several key frames and the boundary between
    bitmap words 0 and 1, strides 1, 2, 5 and 32."""
    n = len(clip.keys)
    keys = [t for t, k in enumerate(clip.keys) if k]
    runs = [(0, n, 1)]                                                # everything: every key frame inside, every word boundary
    for stride in (2, 5, 32):
        for first in (0, 1, 3):
            runs.append((first, (n - 1 - first) // stride + 1, stride))
    for k in keys[1:]:
        for first in (k - 1, k, k + 1):                               # just before, on and just behind a key frame
            if 0 <= first < n:
                runs.append((first, min(5, n - first), 1))
    runs.append((29, min(6, n - 29), 1))                              # off a key frame, across frame 31 | 32 where the clip is that long
    runs.append((7, n - 7, 1))                                        # an inter frame first, several key frames (or none) inside
    runs.append((n - 1, 1, 1))                                        # the last frame alone
    return runs


@pytest.mark.parametrize("case", CASES, ids=lambda c: "cfg%d_%dx%d_%dbpp_v%d_k%d" % (c[0], c[1], c[2], c[4], c[5], c[6]))
def test_forward_walk_equals_backward_walk_encoder_and_oracle(case):
    cfg, w, h, n, bpp, version, key_every, key_row = case
    clip = ref.make_clip(cfg, w, h, n, bpp, version, key_every, key_row)
    pictures, _ = ref.oracle_run(clip)
    comp = ref.Composer(clip)
    backward = [comp.picture(t) for t in range(n)]
    crossed_keys, crossed_word, firsts_on_key, firsts_off_key = 0, False, 0, 0
    for first, count, stride in _runs(clip):
        got = play_ref.play(comp, first, count, stride)
        assert len(got) == count
        last = first + (count - 1) * stride
        crossed_keys = max(crossed_keys, sum(clip.keys[first + 1:last + 1]))
        crossed_word = crossed_word or (first >> 5) != (last >> 5)
        firsts_on_key += clip.keys[first]
        firsts_off_key += not clip.keys[first]
        for k, pic in enumerate(got):
            t = first + k * stride
            what = f"{clip.name} Play({first}, {count}, stride {stride}) frame {t}"
            assert np.array_equal(pic, backward[t]), what + ": not the backward walk's picture"
            assert np.array_equal(pic, clip.frames[t]), what + ": not the encoder's picture"
            assert np.array_equal(pic, pictures[t]), what + ": not the oracle's picture"
    assert firsts_on_key and firsts_off_key
    assert crossed_word or n <= 32
    assert crossed_keys >= (3 if key_every else 0), "no run crosses several key frames"


def test_the_runs_cover_what_the_kernel_must_cope_with():
    clip = ref.make_clip(41, 64, 48, 41, 24, 4, 11, 36)
    runs = _runs(clip)
    assert {s for _, _, s in runs} == {1, 2, 5, 32}
    flat = [t for t, (c, k) in enumerate(zip(clip.chunks, clip.keys)) if k and (c[0] & 0xF) == 1]
    assert any(first < t <= first + (n - 1) * s for t in flat for first, n, s in runs), "no run crosses a flat key frame"
    assert any(n > 1 and s == 32 for _, n, s in runs), "stride 32 never emits a second frame"
