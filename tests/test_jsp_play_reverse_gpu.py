"""examples/jsp_play clip.avi --reverse / --boomerang FIRST[:COUNT[:STRIDE]][:tight] OUT.avi on MSVideo1 clips.  The example exits 0,
every CRC pair it prints — OUT.avi played back through a decoder of ITS size beside the clip's own pictures — is equal, the frames
come in reverse (boomerang: there and back, the last picture the first), and OUT.avi's geometry, frames and flags are those of
Manager.reverse / boomerang and their writers (the Python path), whose clip decodes to the same CRCs."""
import subprocess

import numpy as np
import pytest

import msv1_crop_clips as cc
from jsplayer_amd import avi, player
from jsplayer_amd.avi import CODEC_MSVC16, CODEC_MSVC8, VideoInfo
from jsplayer_amd.streamgen import sp_clip
from msv1_range_clips import make_gpu, palette
from test_jsp_play_crop_gpu import crcs_of
from test_jsp_play_thin_gpu import exe_path

pytestmark = pytest.mark.gpu


def run(path, option, extra):
    res = subprocess.run([exe_path(), str(path), option] + extra, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    return res.returncode, [l.split() for l in res.stdout.decode().splitlines()], res.stderr.decode()


@pytest.mark.parametrize("bits", [16, 8])
@pytest.mark.parametrize("tight", [False, True], ids=["loose", "tight"])
@pytest.mark.parametrize("option", ["--reverse", "--boomerang"])
def test_jsp_play_gives_the_python_paths_clip_and_its_crcs(tmp_path, option, bits, tight):
    clip = cc.tight(bits) if tight else cc.seams(bits, cc.WHOLE)
    frames, keys, pal = clip.frames, clip.keys, palette(bits)
    path, out = tmp_path / "clip.avi", tmp_path / "out.avi"
    path.write_bytes(avi.write_avi(cc.W, cc.H, frames, fourcc=b"CRAM", bpp=bits, fps=15.0, palette=pal, key_flags=keys))
    first, count, stride = 1, 4, 2
    keep = [first + k * stride for k in range(count)]
    order = keep[::-1] if option == "--reverse" else keep + keep[-2::-1]
    rc, lines, err = run(path, option, [f"{first}:{count}:{stride}" + (":tight" if tight else ""), str(out)])
    assert rc == 0, err
    assert lines[0] == [option[2:], "blocks", "0", "0", "48", "48", "display", "0", "0", "192", "192"]
    assert [l[0] for l in lines[1:]] == [str(k) for k in order]
    assert all(len(l) == 3 and l[1] == l[2] for l in lines[1:]), lines
    assert len({l[1] for l in lines[1:]}) == count                # four different pictures
    if option == "--boomerang":
        assert lines[1][1] == lines[-1][1]                        # the last picture is the first: the file loops
    vi, got, got_keys = avi.read_avi_indexed(out.read_bytes())
    assert (vi.X, vi.Y, vi.bpp, vi.nframes) == (cc.W, cc.H, bits, len(order))
    dec = make_gpu(bits, cc.W, cc.H, pal)
    info = VideoInfo(X=cc.W, Y=cc.H, bpp=bits, fps=15.0, nframes=len(frames), codec=CODEC_MSVC16 if bits == 16 else CODEC_MSVC8, palette=pal,
                     riff_size=0)
    mgr = player.Manager(info, dec, lambda n: np.zeros(n, dtype=np.int32))
    with dec.BuildIndex(frames[:keep[-1] + 1], keys[:keep[-1] + 1]) as idx:
        mgr.attach_index(idx, 0)
        make, write = (mgr.reverse, mgr.write_reverse) if option == "--reverse" else (mgr.boomerang, mgr.write_boomerang)
        want, want_keys, shown = make(frames, keep, tight=tight)
        assert shown == (0, 0, cc.W, cc.H) and (want, want_keys) == mgr.sequence(frames, order, tight=tight)[:2]
        assert [bytes(f) for f in got] == [bytes(f) for f in want] and list(got_keys) == want_keys
        blob = write(frames, keep, tight=tight)
        if tight:
            assert sum(len(f) for f in want) < sum(len(f) for f in make(frames, keep)[0])
        # the same frames forward are CropFrames' own: what is new is the step back
        assert mgr.sequence(frames, keep, tight=tight)[:2] == mgr.crop(frames, (0, 0, cc.W, cc.H), keep, tight=tight)[:2]
    dec.StopAndClean()
    vi2, mine, mine_keys = avi.read_avi_indexed(blob)
    assert (vi2.X, vi2.Y, vi2.bpp) == (vi.X, vi.Y, vi.bpp) and [bytes(f) for f in mine] == want
    assert crcs_of(bits, vi2.X, vi2.Y, pal, mine, mine_keys) == [l[1] for l in lines[1:]]   # the Python path's clip: the example's CRCs
    if not tight and bits == 16 and option == "--reverse":
        # an unknown suffix; text behind :tight; an empty run; frames outside the clip; not alone; with --crop's rectangle; no file name
        for extra in (["1:2:2:loose", str(out)], ["1:tight:junk", str(out)], ["5:0", str(out)], ["1:2:2", str(out), "--step-back"], ["1:2"]):
            rc, bad, err = run(path, option, extra)
            assert rc != 0 and not [l for l in bad if l[0] != "reverse"], extra
        rc, bad, err = run(path, option, ["9:4:2", str(out)])
        assert rc != 0 and "not all in the clip" in err


def test_jsp_play_refuses_screenpressor_with_the_other_clip_options_sentence(tmp_path):
    chunks, keys, _ = sp_clip(3, 64, 48, 3, version=4)
    path = tmp_path / "sp.avi"
    path.write_bytes(avi.write_avi(64, 48, chunks, fourcc=b"SCPR", bpp=24, fps=15.0, key_flags=keys))
    said = {}
    for option, spec in (("--reverse", ["0:2:1"]), ("--boomerang", ["0:2:1"]), ("--crop", ["0:0:8:8", "0:2:1"])):
        res = subprocess.run([exe_path(), str(path), option] + spec + [str(tmp_path / "out.avi")], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                             timeout=120)
        assert res.returncode == 2 and not (tmp_path / "out.avi").exists()
        said[option] = res.stderr.decode().strip()
        assert said[option].startswith(option + ": MSVideo1 only")
    assert said["--reverse"][len("--reverse"):] == said["--boomerang"][len("--boomerang"):] == said["--crop"][len("--crop"):]
