"""examples/jsp_play --activity [FIRST[:COUNT]] on an AVI of either codec: the lines it prints — frame, changed pixels, the box of the
frame's non-zero cells in display coordinates — and the CRC of the map are those of SeekIndex.Activity / SpScrubIndex.Activity and
Manager.change_box over the same clip."""
import os
import subprocess
import zlib

import numpy as np
import pytest

from jsplayer_amd import ScreenPressor, avi, player
from jsplayer_amd import streamgen as sg
from jsplayer_amd.avi import CODEC_MSVC16, CODEC_SCREENPRESSOR, VideoInfo
from msv1_range_clips import make_gpu

pytestmark = pytest.mark.gpu

W, H, N = 320, 232, 24   # 20 x 15 cells, the last row 8 pixels high


def run(exe, path, extra):
    res = subprocess.run([exe, str(path), "--activity"] + extra, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    return res.returncode, [l.split() for l in res.stdout.decode().splitlines()], res.stderr.decode()


@pytest.mark.parametrize("kind", ["msvideo1", "screenpressor"])
def test_jsp_play_activity_prints_the_map(tmp_path, kind):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "examples", "jsp_play")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-s", "-C", os.path.join(root, "examples")])
    path = tmp_path / "clip.avi"
    if kind == "msvideo1":
        frames, keys, _ = sg.msv1_clip(97, W, H, N, p_mix=sg.msv1_p_mix(0.9, 6.0), key_every=16)
        path.write_bytes(avi.write_avi(W, H, frames, fourcc=b"CRAM", bpp=16, fps=15.0, key_flags=keys))
        dec = make_gpu(16, W, H)
        idx = dec.BuildIndex(frames, keys)
        vi = VideoInfo(X=W, Y=H, bpp=16, fps=15.0, nframes=N, codec=CODEC_MSVC16, palette=None, riff_size=0)
    else:
        frames, keys, _ = sg.sp_clip(98, W, H, N, bpp=24, version=4, key_every=16)
        path.write_bytes(avi.write_avi(W, H, frames, fourcc=b"SCPR", bpp=24, fps=15.0, key_flags=keys))
        dec = ScreenPressor(W, H, 24)
        dec.Preinit(player.INSIGNIFICANT_LINES)
        idx = dec.BuildScrubIndex(frames, keys)
        vi = VideoInfo(X=W, Y=H, bpp=24, fps=15.0, nframes=N, codec=CODEC_SCREENPRESSOR, palette=None, riff_size=0)
    whole = idx.Activity().cpu().numpy().view(np.uint16)
    cols, rows = idx.ActivitySize()
    mgr = player.Manager(vi, dec, lambda n: np.zeros(n, dtype=np.int32))
    mgr.attach_index(idx, 0)
    for extra, first, count in (([], 0, N), (["3:10"], 3, 10), ([str(N - 1)], N - 1, 1)):
        rc, lines, err = run(exe, path, extra)
        assert rc == 0, err
        part = whole[first:first + count]
        assert lines[-1] == ["map", f"{cols}x{rows}x{count}", "%08x" % zlib.crc32(part.tobytes())], extra
        assert len(lines) == count + 1
        for k, line in enumerate(lines[:-1]):
            box = mgr.change_box(first + k)
            want = [str(first + k), str(int(part[k].sum(dtype=np.int64))), "-" if box is None else ",".join(str(v) for v in box)]
            assert line == want, (extra, k)
    assert whole.any()
    for extra in (["0:%d" % (N + 1)], [str(N)], ["5:0"], ["--step-back"]):   # past the end; an empty run; it goes alone
        rc, lines, err = run(exe, path, extra)
        assert rc != 0 and not lines, extra
    idx.close()
    dec.StopAndClean()
