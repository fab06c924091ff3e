"""The premise of the ScreenPressor seek index, checked without a GPU: composing every frame from the literalised host-stage
records (tests/sp_index_ref.py: last writer per pixel, key picture underneath) reproduces the encoder's pictures and the oracle's
sequential run exactly — every frame of every clip."""
import numpy as np
import pytest

import sp_index_ref as ref

CASES = [   # (config, width, height, frames, bpp, version, key_every, key_row)
    (41, 64, 48, 41, 24, 4, 11, 36),
    (42, 100, 52, 41, 24, 3, 11, 7),
    (43, 37, 23, 41, 24, 2, 11, 5),
    (44, 64, 48, 41, 16, 4, 11, 36),
    (45, 100, 52, 30, 16, 2, 11, 7),
    (46, 37, 23, 30, 16, 3, 11, 5),
    (47, 64, 48, 80, 24, 4, 0, 36),      # one key frame, 79 frames behind it
]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "cfg%d_%dx%d_%dbpp_v%d_k%d" % (c[0], c[1], c[2], c[4], c[5], c[6]))
def test_composition_equals_encoder_and_oracle(case):
    cfg, w, h, n, bpp, version, key_every, key_row = case
    clip = ref.make_clip(cfg, w, h, n, bpp, version, key_every, key_row)
    assert clip.keys[0] and sum(clip.keys) >= (4 if key_every else 1)
    pictures, verdicts = ref.oracle_run(clip)
    comp = ref.Composer(clip)
    # (p_mix_at asks for 45 - 60 % moved blocks; a move that would leave the picture is dropped, which is most of them at 64x48)
    if w >= 100:
        assert max(comp.motion_share.values()) > 0.25, "no frame moves more than a quarter of its blocks"
    assert any(t not in comp.mask and not clip.keys[t] for t in range(n)), "no unchanged frame"
    for t in range(n):
        got = comp.picture(t)
        assert np.array_equal(got, clip.frames[t]), f"frame {t}: composition differs from the encoder's picture"
        assert np.array_equal(got, pictures[t]), f"frame {t}: composition differs from the oracle's picture"
        if not clip.keys[t]:
            assert comp.verdict_p[t] == verdicts[t], f"frame {t}: host-stage verdict differs from DecompressP's"


def test_clip_has_the_key_frame_kinds_the_index_must_cope_with():
    clip = ref.make_clip(41, 64, 48, 41, 24, 4, 11, 36)
    flat = [t for t, (c, k) in enumerate(zip(clip.chunks, clip.keys)) if k and (c[0] & 0xF) == 1]
    coded = [t for t, (c, k) in enumerate(zip(clip.chunks, clip.keys)) if k and (c[0] & 0xF) == 2]
    assert flat and len(coded) >= 3
    assert any(clip.keys[t] and clip.keys[t - 1] for t in range(1, len(clip.keys))), "no key frame right behind a key frame"
    assert any(not clip.keys[t + 1] for t in flat if t + 1 < len(clip.keys)), "no inter frame behind a flat key frame"
