"""examples/jsp_play clip.avi --pan WxH[:loose] FIRST[:COUNT[:STRIDE]] OUT.avi on a small MSVideo1 clip whose content wanders.  The
example exits 0, the path it prints is the one Manager.follow gives for the same frames, OUT.avi decodes — through the project's own
player on the GPU — to the rectangles of the source's pictures along that path, and its geometry, frames and flags are those of
Manager.pan / write_pan (the Python path)."""
import subprocess
import zlib

import numpy as np
import pytest

import msv1_pan_clips as pc
from jsplayer_amd import avi, player
from jsplayer_amd.avi import CODEC_MSVC16, CODEC_MSVC8, VideoInfo
from msv1_range_clips import dev_buf, make_gpu
from test_jsp_play_crop_gpu import crcs_of
from test_jsp_play_thin_gpu import exe_path

pytestmark = pytest.mark.gpu


def run(path, extra):
    res = subprocess.run([exe_path(), str(path), "--pan"] + extra, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    return res.returncode, [l.split() for l in res.stdout.decode().splitlines()], res.stderr.decode()


def pictures_of(bits, pal, frames, keys):
    """The ordinary decode loop over the source clip: every picture as an H x W array."""
    dec = make_gpu(bits, pc.W, pc.H, pal)
    pool = [dev_buf(pc.W * pc.H) for _ in range(2)]
    out = []
    for data, key in zip(frames, keys):
        prev = dec.PreviousFrame()
        dst = next(b for b in pool if b is not prev)
        if key:
            assert dec.DecompressI(data, dst) == 0
        else:
            dst.copy_(prev)
            dec.DecompressP(data, dst)
        out.append(dec.PreviousFrame().cpu().numpy().astype(np.int32).reshape(pc.H, pc.W).copy())
    dec.StopAndClean()
    return out


@pytest.mark.parametrize("bits", [16, 8])
@pytest.mark.parametrize("tight", [True, False], ids=["tight", "loose"])
def test_jsp_play_pan_follows_as_the_python_path_does_and_its_clip_decodes_to_the_rectangles(tmp_path, bits, tight):
    clip = pc.wander(bits)
    frames, keys, pal = clip.frames, clip.keys, clip.pal
    path, out = tmp_path / "clip.avi", tmp_path / "pan.avi"
    path.write_bytes(avi.write_avi(pc.W, pc.H, frames, fourcc=b"CRAM", bpp=bits, fps=15.0, palette=pal, key_flags=keys))
    size = (62, 45)                                            # rounded up to blocks: 16 x 12
    first, count, stride = 1, 5, 2
    keep = [first + k * stride for k in range(count)]
    rc, lines, err = run(path, ["%dx%d" % size + ("" if tight else ":loose"), f"{first}:{count}:{stride}", str(out)])
    assert rc == 0, err
    dec = make_gpu(bits, pc.W, pc.H, pal)
    info = VideoInfo(X=pc.W, Y=pc.H, bpp=bits, fps=15.0, nframes=len(frames), codec=CODEC_MSVC16 if bits == 16 else CODEC_MSVC8, palette=pal,
                     riff_size=0)
    mgr = player.Manager(info, dec, lambda n: np.zeros(n, dtype=np.int32))
    assert mgr.pan_size(size) == (16, 12) and lines[0] == ["pan", "blocks", "16", "12"]
    vi, got, got_keys = avi.read_avi_indexed(out.read_bytes())
    assert (vi.X, vi.Y, vi.bpp, vi.nframes) == (64, 48, bits, count)
    with dec.BuildIndex(frames[:keep[-1] + 1], keys[:keep[-1] + 1]) as idx:
        mgr.attach_index(idx, 0)
        route = mgr.follow(size, keep)
        assert [(int(l[0]), int(l[1]), int(l[2])) for l in lines[1:]] == route
        assert len({r[1] for r in route}) > 2 and len({r[2] for r in route}) > 2          # the rectangle moves on both axes
        assert all(len(l) == 5 and l[3] == l[4] for l in lines[1:]), lines
        want, want_keys, shown = mgr.pan(frames, size, route, tight=tight)
        assert [bytes(f) for f in got] == [bytes(f) for f in want] and list(got_keys) == want_keys
        blob = mgr.write_pan(frames, size, route, tight=tight)
        if tight:
            assert sum(len(f) for f in want) < sum(len(f) for f in mgr.pan(frames, size, route, tight=False)[0])
    dec.StopAndClean()
    vi2, mine, mine_keys = avi.read_avi_indexed(blob)
    assert (vi2.X, vi2.Y, vi2.bpp) == (vi.X, vi.Y, vi.bpp) and [bytes(f) for f in mine] == want
    # the written clip through a decoder of its own size: the rectangles of the source's pictures along the path
    pictures = pictures_of(bits, pal, frames[:keep[-1] + 1], keys)
    along = ["%08x" % zlib.crc32(np.ascontiguousarray(pictures[k][4 * y:4 * y + 48, 4 * x:4 * x + 64]).tobytes()) for k, x, y in route]
    assert crcs_of(bits, vi2.X, vi2.Y, pal, mine, mine_keys) == along == [l[3] for l in lines[1:]]
    assert len(set(along)) > 1
    assert shown == [(4 * x, pc.H - 4 * (y + 12), 64, 48) for _, x, y in route]
    if tight and bits == 16:
        # no height; no x; text behind the size; a part that is no number; an empty run; not alone; with --crop; no file name
        for extra in (["64", "1", str(out)], ["64x", "1", str(out)], ["64x48:tight", "1", str(out)], ["ax48", "1", str(out)],
                      ["0x48", "1", str(out)], ["64x48", "5:0", str(out)], ["64x48", "1", str(out), "--step-back"], ["64x48", "1", str(out), "--crop", "8:8:8:8", "1", str(out)],
                      ["64x48", "1"]):
            rc, bad, err = run(path, extra)
            assert rc != 0 and not [l for l in bad if l[0] != "pan"], extra
