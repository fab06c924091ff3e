"""examples/jsp_play --distance REF[:FIRST[:COUNT]] on a small written AVI of either codec: the totals it prints per frame, the frames
it lists at distance 0 and the CRC of the map are THE DEFINITION's (tests/index_distance_ref.py over the oracle's run, through
tests/index_distance_cases.py) — nothing of the truth comes from the GPU."""
import os
import subprocess
import zlib

import numpy as np
import pytest

import index_activity_ref as ar
import index_distance_cases as cs
import index_distance_ref as dr
from jsplayer_amd import avi

pytestmark = pytest.mark.gpu


def run(exe, path, extra):
    res = subprocess.run([exe, str(path)] + extra, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    return res.returncode, [l.split() for l in res.stdout.decode().splitlines()], res.stderr.decode()


def clip_of(kind):
    """(AVI bytes, w, h, frames, pictures P(-1) and P(0) .. P(n - 1), whole blocks only)"""
    if kind == "msvideo1":   # msv1_tight_clips.directed: frame 1 shows frame 0's picture, `back` (4) returns to it at the spots
        c = cs.msv1_directed(16, 128, 128)
        return avi.write_avi(c.w, c.h, c.frames, fourcc=b"CRAM", bpp=16, fps=15.0, key_flags=c.keys), c.w, c.h, c.n, c.p_before, c.p, True
    c = cs.sp_case("72x16")   # sp_activity_clips: the picture of frame 30 comes back, frame 40 repeats frame 39
    k = c.clip
    data = avi.write_avi(k.w, k.h, k.chunks, fourcc=b"SCPR", bpp=k.bpp, fps=15.0, key_flags=k.keys)
    return data, k.w, k.h, c.n, np.zeros(k.w * k.h, dtype=np.uint32), c.pictures, False


@pytest.mark.parametrize("kind", ["msvideo1", "screenpressor"])
def test_jsp_play_distance_prints_the_definitions_totals(tmp_path, kind):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "examples", "jsp_play")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-s", "-C", os.path.join(root, "examples")])
    data, w, h, n, p_before, p, blocks_only = clip_of(kind)
    path = tmp_path / "clip.avi"
    path.write_bytes(data)
    cols, rows = ar.grid(w, h)
    runs = {"msvideo1": (("1", 1, 0, n), ("4:2:5", 4, 2, 5), ("-1", -1, 0, n), ("%d:%d" % (n - 1, n - 1), n - 1, n - 1, 1)),
            "screenpressor": (("30", 30, 0, n), ("-1:3:10", -1, 3, 10), ("40:39:2", 40, 39, 2), ("0:%d" % (n - 1), 0, n - 1, 1))}[kind]
    seen_return = False
    for arg, ref, first, count in runs:
        rc, lines, err = run(exe, path, ["--distance", arg])
        assert rc == 0, (arg, err)
        want = dr.distance(p[first:first + count], p_before if ref < 0 else p[ref], w, h, blocks_only)
        totals = [int(v) for v in want.reshape(count, -1).sum(axis=1, dtype=np.int64)]
        assert len(lines) == count + 2, arg
        assert lines[:count] == [[str(first + k), str(totals[k])] for k in range(count)], arg
        zero = [str(first + k) for k in range(count) if totals[k] == 0]
        assert lines[count] == ["zero"] + zero, arg
        assert lines[-1] == ["map", f"{cols}x{rows}x{count}", "%08x" % zlib.crc32(want.tobytes())], arg
        seen_return = seen_return or len([z for z in zero if int(z) != ref]) > 0
        assert any(totals) or count <= 2
    assert seen_return, "no run finds the reference picture at another frame"
    for extra in (["--distance", "0:0:%d" % (n + 1)], ["--distance", "0:%d" % n], ["--distance", str(n)], ["--distance", "-2"],
                  ["--distance", "0:5:0"], ["--distance", "0", "--step-back"], ["--distance"], ["--distance", "1", "--activity"],
                  ["--activity", "--distance", "1"], ["--distance", "last"], ["--distance", "1x"], ["--distance", "1:"], ["--distance", "1:-2"]):
        # past the end; a reference outside the clip; an empty run; it goes alone, without --activity too; no REF; a REF that is no number
        rc, lines, err = run(exe, path, extra)
        assert rc != 0 and not [l for l in lines if l and l[0] in ("zero", "map")], extra
