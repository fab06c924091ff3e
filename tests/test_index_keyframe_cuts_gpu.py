"""jsp_index_key_frame / SeekIndex.KeyFrame on the directed clips of tests/msv1_keyframe_cut_clips.py, on an MI355X: every way a
frame's end cuts a code (ends), the first refusing block at the lane, wave and workgroup seams with both kinds next to each other
(firsts), the scan and both ends of the gather kernel's image (pieces), frames that write nothing between a writer and t (gaps).

Truth: tests/index_keyframe_ref.py, which test_msv1_keyframe_cut_clips_cpu.py pins to the oracle on these clips and holds to what the
clips plan — nothing of it comes from the GPU.  Every frame of every clip goes through test_index_keyframe_gpu.Case.check: the BYTES,
exactly, or the refusal with its kind, block and writer frame; nothing written behind the frame or on a refusal; *len 0 on a refusal;
PreviousFrame where it was.  Every clip runs as one chunk, in chunks of 7 frames, and — where it allows — behind three frames decoded
one by one; and all of it with the block tables of the host parser and of the on-GPU parse."""
import numpy as np
import pytest

import msv1_keyframe_cut_clips as kc
import test_index_keyframe_gpu as base
from msv1_range_clips import POISON, dev_buf, make_gpu, palette
from test_index_keyframe_gpu import Case, covered, seam_clip

pytestmark = pytest.mark.gpu

SETUPS = {"one_chunk": (0, None), "chunks_of_7": (0, kc.CHUNK), "picture_before": (3, None)}


@pytest.fixture(autouse=True, params=["host", "gpu"])
def parse_mode(request):
    """Every test runs with the block tables of the host parser and of the on-GPU parse (base.Case reads base.PARSE)."""
    base.PARSE = request.param
    yield request.param
    base.PARSE = "host"


def case_of(clip, start=0, chunk=None):
    return Case(clip.bits, clip.w, clip.h, palette(clip.bits), clip.frames, clip.keys, start=start, chunk=chunk)


@pytest.mark.parametrize("bits", [16, 8])
@pytest.mark.parametrize("setup", list(SETUPS))
@pytest.mark.parametrize("name", kc.FAMILIES)
def test_every_frame_of_every_clip(name, setup, bits):
    start, chunk = SETUPS[setup]
    ran = 0
    for clip in kc.family(name, bits):
        if start not in clip.starts:
            continue
        c = case_of(clip, start, chunk)
        c.where = f"{clip.name} {c.where}"
        for t in range(c.n):
            c.check(t)
        c.close()
        ran += 1
    assert ran > 0


@pytest.mark.parametrize("bits", [16, 8])
@pytest.mark.parametrize("name", kc.FAMILIES)
def test_round_trip_through_the_gpu_codec(name, bits):
    """A fresh codec decodes KeyFrame(t) as a key frame and the original frames t + 1 .. t + 3 on top: each picture is Show's.  t: the
    first frame of the family's first clip that can be cut and has a frame in front of it that cannot (ends, firsts), or that
    lies behind the first frames that write nothing (gaps), or has a 16-byte-unaligned workgroup base (pieces: the sweep, frame 2)."""
    clip = kc.family(name, bits)[1 if name == "pieces" else 0]
    c = case_of(clip)
    w, h, pal = clip.w, clip.h, palette(bits)
    answers = [c.want(t) for t in range(c.n - 3)]
    if name in ("ends", "firsts"):
        t = next(t for t in range(1, c.n - 3) if isinstance(answers[t], bytes) and not isinstance(answers[t - 1], bytes))
    else:
        t = clip.gap_frames[2] if name == "gaps" else 2
    kf = c.idx.KeyFrame(t)
    assert kf == answers[t]
    fresh = make_gpu(bits, w, h, pal, parse=base.PARSE)
    assert fresh.IsKeyFrame(kf)
    pool = [dev_buf(w * h) for _ in range(2)]
    shown = dev_buf(w * h)
    assert fresh.DecompressI(kf, pool[0]) == 0
    for k in range(4):
        if k > 0:
            prev = fresh.PreviousFrame()
            dst = next(b for b in pool if b is not prev)
            dst.copy_(prev)
            if c.range_keys[t + k]:
                assert fresh.DecompressI(c.range[t + k], dst) == 0
            else:
                fresh.DecompressP(c.range[t + k], dst)
        shown.fill_(POISON)
        c.idx.Show(t + k, shown, adopt=False)
        assert np.array_equal(covered(fresh.PreviousFrame().cpu().numpy(), w, h), covered(shown.cpu().numpy(), w, h)), \
            f"{clip.name} {c.where}: frame {t + k} on top of KeyFrame({t})"
    fresh.StopAndClean()
    c.close()


def test_the_on_gpu_parse_hands_truncated_frames_to_the_host_parser(parse_mode):
    """The mixture of table sources the parse_mode fixture is meant to reach is reached: with msv1_parse = gpu, building the index
    of a clip with frames too short to code every block raises "host_parsed_frames" by at least the number of such frames, and a
    clip of whole frames leaves it alone.  With the host parser the counter counts nothing."""
    (clip,) = kc.family("ends", 16)
    short = sum(1 for g in clip.groups if g["what"] == "cut" and not (g["d"] == g["L"] and g["p"] == clip.nb - 1))
    assert short >= 50
    c = case_of(clip)
    rose = c.gpu.counter("host_parsed_frames")
    assert rose >= short if parse_mode == "gpu" else rose == 0, rose
    assert rose < c.n                                              # ... and the whole frames of the same index stayed with the GPU
    c.close()
    w, h, frames, keys = seam_clip(16)                             # whole frames only
    c = Case(16, w, h, None, frames, keys)
    assert c.gpu.counter("host_parsed_frames") == 0
    assert isinstance(c.check(3), bytes)
    c.close()
