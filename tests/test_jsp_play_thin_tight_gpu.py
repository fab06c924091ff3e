"""examples/jsp_play clip.avi --thin-tight FIRST[:COUNT[:STRIDE]] OUT.avi on MSVideo1 clips: what --thin does, with
jsp_index_tight_frames.  The example exits 0, every CRC pair it prints — OUT.avi played back through the ordinary decode loop beside
the clip's own frames — is equal, OUT.avi is no longer than --thin's, and its frames and flags are those of
Manager.thin(..., tight=True)."""
import os
import subprocess

import numpy as np
import pytest

from jsplayer_amd import avi, player
from jsplayer_amd.avi import CODEC_MSVC16, CODEC_MSVC8, VideoInfo
from msv1_range_clips import long_clip, make_gpu, palette
from msv1_tight_clips import directed
from test_jsp_play_thin_gpu import exe_path

pytestmark = pytest.mark.gpu


def run(path, flag, extra):
    res = subprocess.run([exe_path(), str(path), flag] + extra, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    return res.returncode, [l.split() for l in res.stdout.decode().splitlines()], res.stderr.decode()


@pytest.mark.parametrize("bits", [16, 8])
def test_jsp_play_thin_tight_plays_back_as_the_originals_frames_and_is_no_longer_than_thin(tmp_path, bits):
    """The directed clip: frame 1 recodes every block unchanged, frame 6 is a key frame of the picture as it stands."""
    clip = directed(bits, 164, 100)
    w, h, frames, keys, pal = clip.w, clip.h, clip.frames, clip.keys, palette(bits)
    path, tight, plain = tmp_path / "clip.avi", tmp_path / "tight.avi", tmp_path / "plain.avi"
    path.write_bytes(avi.write_avi(w, h, frames, fourcc=b"CRAM", bpp=bits, fps=15.0, palette=pal, key_flags=keys))
    first, count, stride = 1, 4, 2                            # frames 1, 3, 5, 7: the gap (5, 7] spans the key frame 6
    keep = [first + k * stride for k in range(count)]
    rc, lines, err = run(path, "--thin-tight", [f"{first}:{count}:{stride}", str(tight)])
    assert rc == 0, err
    assert [l[0] for l in lines] == [str(k) for k in keep]
    assert all(len(l) == 3 and l[1] == l[2] for l in lines), lines
    assert len({l[1] for l in lines}) > 1
    rc, plain_lines, err = run(path, "--thin", [f"{first}:{count}:{stride}", str(plain)])
    assert rc == 0 and plain_lines == lines, err             # the same pictures
    assert os.path.getsize(tight) < os.path.getsize(plain)   # ... in fewer bytes: (1, 3] and (3, 5] hold blocks recoded unchanged
    vi, got, got_keys = avi.read_avi_indexed(tight.read_bytes())
    assert (vi.X, vi.Y, vi.bpp, vi.nframes) == (w, h, bits, count)
    dec = make_gpu(bits, w, h, pal)
    info = VideoInfo(X=w, Y=h, bpp=bits, fps=15.0, nframes=len(frames), codec=CODEC_MSVC16 if bits == 16 else CODEC_MSVC8, palette=pal, riff_size=0)
    mgr = player.Manager(info, dec, lambda n: np.zeros(n, dtype=np.int32))
    with dec.BuildIndex(frames[:keep[-1] + 1], keys[:keep[-1] + 1]) as idx:
        mgr.attach_index(idx, 0)
        want, want_keys = mgr.thin(frames, keep, keys, tight=True)
        assert [bytes(f) for f in got] == [bytes(f) for f in want] and list(got_keys) == want_keys
        loose = mgr.thin(frames, keep, keys)[0]
        assert all(len(t) <= len(d) for t, d in zip(want, loose)) and sum(map(len, want)) < sum(map(len, loose))
    dec.StopAndClean()
    for extra in (["5:0", str(tight)], ["5:2:0", str(tight)], ["5", str(tight), "--step-back"], ["5"]):
        rc, lines, err = run(path, "--thin-tight", extra)     # an empty run; no stride; it goes alone; no file name
        assert rc != 0 and not lines, extra


def test_jsp_play_thin_tight_on_a_long_clip_and_where_the_library_refuses(tmp_path):
    """8-bit long_clip (end markers, repaints, the key frame 70 that repaints the picture as it is): never longer than --thin.
    16-bit long_clip: the truncated frame 31 paints the blocks behind its end black — kept, and their codes are cut."""
    W, H = 64, 32
    frames, keys, pal, _ = long_clip(8, W, H, seed=5, n=96)
    path, tight, plain = tmp_path / "clip.avi", tmp_path / "tight.avi", tmp_path / "plain.avi"
    path.write_bytes(avi.write_avi(W, H, frames, fourcc=b"CRAM", bpp=8, fps=15.0, palette=pal, key_flags=keys))
    rc, lines, err = run(path, "--thin-tight", ["6:11:8", str(tight)])
    assert rc == 0 and len(lines) == 11 and all(l[1] == l[2] for l in lines), err
    rc, plain_lines, err = run(path, "--thin", ["6:11:8", str(plain)])
    assert rc == 0 and plain_lines == lines and os.path.getsize(tight) <= os.path.getsize(plain), err
    frames, keys, _, _ = long_clip(16, W, H, seed=5, n=96)
    path.write_bytes(avi.write_avi(W, H, frames, fourcc=b"CRAM", bpp=16, fps=15.0, key_flags=keys))
    out = tmp_path / "out.avi"
    rc, lines, err = run(path, "--thin-tight", ["8:4:8", str(out)])   # frames 8, 16, 24, 32: the gap (24, 32] holds frame 31
    assert rc == 1 and not lines and "index_tight:" in err and "cut off" in err and "frame 31" in err, err
    assert not out.exists()
    rc, lines, err = run(path, "--thin-tight", ["8:3:8", str(out)])   # ... and without that gap it is served
    assert rc == 0 and len(lines) == 3 and all(l[1] == l[2] for l in lines), err
