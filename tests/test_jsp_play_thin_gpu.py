"""examples/jsp_play clip.avi --thin FIRST[:COUNT[:STRIDE]] OUT.avi on MSVideo1 clips: OUT.avi holds the frames FIRST + k * STRIDE, and
every CRC pair the example prints — OUT.avi played back through the ordinary decode loop beside the clip's own frames — is equal.  The
file's frames and flags are those of Manager.thin over a SeekIndex of its own from the same key frame: the first a KeyFrame, key frames
of the clip copied, the others DeltaFrames' inter frames.  A gap that cannot be spanned exits with 1, the library's text and no file."""
import os
import subprocess

import numpy as np
import pytest

from jsplayer_amd import avi, player
from jsplayer_amd import streamgen as sg
from jsplayer_amd.avi import CODEC_MSVC16, CODEC_MSVC8, VideoInfo
from msv1_range_clips import long_clip, make_gpu

pytestmark = pytest.mark.gpu

W, H = 64, 32
FIRST, COUNT, STRIDE = 6, 11, 8   # frames 6, 14, .. 86: 22 (16 bits) and 70 (8 bits) are key frames of the clips


def exe_path():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "examples", "jsp_play")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-s", "-C", os.path.join(root, "examples")])
    return exe


def run(path, extra):
    res = subprocess.run([exe_path(), str(path), "--thin"] + extra, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    return res.returncode, [l.split() for l in res.stdout.decode().splitlines()], res.stderr.decode()


def clip_of(bits):
    if bits == 8:      # end markers, repaints, all-skip frames; key frames 0 and 70
        frames, keys, pal, _ = long_clip(8, W, H, seed=5, n=96)
        return frames, keys, pal
    frames, keys, _ = sg.msv1_clip(97, W, H, 96, p_mix=sg.msv1_p_mix(0.9, 6.0), key_every=22)
    return frames, keys, None


@pytest.mark.parametrize("parse_mode", ["host", "gpu"])
@pytest.mark.parametrize("bits", [16, 8])
def test_jsp_play_thin_writes_a_time_lapse_that_plays_back_as_the_originals_frames(tmp_path, bits, parse_mode):
    frames, keys, pal = clip_of(bits)
    keep = [FIRST + k * STRIDE for k in range(COUNT)]
    assert not keys[FIRST] and keep[-1] < len(frames)
    path, out = tmp_path / "clip.avi", tmp_path / "out.avi"
    path.write_bytes(avi.write_avi(W, H, frames, fourcc=b"CRAM", bpp=bits, fps=15.0, palette=pal, key_flags=keys))
    rc, lines, err = run(path, [f"{FIRST}:{COUNT}:{STRIDE}", str(out)])
    assert rc == 0, err
    assert [l[0] for l in lines] == [str(k) for k in keep]
    assert all(len(l) == 3 and l[1] == l[2] for l in lines), lines
    assert len({l[1] for l in lines}) > 1                      # (the pictures do change over the run)
    vi, got, got_keys = avi.read_avi_indexed(out.read_bytes())
    assert (vi.X, vi.Y, vi.bpp, vi.nframes) == (W, H, bits, COUNT) and (vi.palette or None) == pal
    # the same frames and flags from Manager.thin, over a SeekIndex of its own from the key frame before FIRST
    dec = make_gpu(bits, W, H, pal, parse=parse_mode)
    info = VideoInfo(X=W, Y=H, bpp=bits, fps=15.0, nframes=len(frames), codec=CODEC_MSVC16 if bits == 16 else CODEC_MSVC8, palette=pal, riff_size=0)
    mgr = player.Manager(info, dec, lambda n: np.zeros(n, dtype=np.int32))
    with dec.BuildIndex(frames[:keep[-1] + 1], keys[:keep[-1] + 1]) as idx:
        mgr.attach_index(idx, 0)
        want, want_keys = mgr.thin(frames, keep, keys)
        assert [bytes(f) for f in got] == [bytes(f) for f in want] and list(got_keys) == want_keys
        assert want[0] == idx.KeyFrame(FIRST) and want_keys[0]
        blob = mgr.write_thin(frames, keep, keys, fps=15.0 / STRIDE)
        assert [bytes(f) for f in avi.read_avi_indexed(blob)[1]] == [bytes(f) for f in want]
    copied = [j for j, k in enumerate(keep) if keys[k]]
    assert all(bytes(got[j]) == bytes(frames[keep[j]]) and got_keys[j] for j in copied)
    assert copied
    dec.StopAndClean()
    # to the end of the clip without a count; stride 1 copies every frame behind the first
    rc, lines, err = run(path, [f"{FIRST}", str(out)])
    assert rc == 0 and [l[0] for l in lines] == [str(k) for k in range(FIRST, len(frames), 8)] and all(l[1] == l[2] for l in lines), err
    rc, lines, err = run(path, [f"{FIRST}:6:1", str(out)])
    assert rc == 0 and len(lines) == 6 and all(l[1] == l[2] for l in lines), err
    _, got, _ = avi.read_avi_indexed(out.read_bytes())
    assert [bytes(f) for f in got[1:]] == [bytes(f) for f in frames[FIRST + 1:FIRST + 6]]
    for extra in ([f"{FIRST}:{COUNT + 2}:{STRIDE}", str(out)], [str(len(frames)), str(out)], ["5:0", str(out)], ["5:2:0", str(out)],
                  ["5", str(out), "--step-back"], ["5"]):
        rc, lines, err = run(path, extra)                      # past the end; an empty run; no stride; it goes alone; no file name
        assert rc != 0 and not lines, extra


def test_jsp_play_thin_refuses_where_the_library_does(tmp_path):
    """16-bit long_clip: the truncated frame 31 cuts codes off, and nothing codes those blocks again before key 70."""
    frames, keys, _, _ = long_clip(16, W, H, seed=5, n=96)
    path, out = tmp_path / "clip.avi", tmp_path / "out.avi"
    path.write_bytes(avi.write_avi(W, H, frames, fourcc=b"CRAM", bpp=16, fps=15.0, key_flags=keys))
    rc, lines, err = run(path, ["8:4:8", str(out)])            # frames 8, 16, 24, 32: the gap (24, 32] holds frame 31
    assert rc == 1 and not lines and "index_delta:" in err and "cut off" in err and "frame 31" in err, err
    assert not out.exists()
    rc, lines, err = run(path, ["8:3:8", str(out)])            # ... and without that gap it is served
    assert rc == 0 and len(lines) == 3 and all(l[1] == l[2] for l in lines), err
