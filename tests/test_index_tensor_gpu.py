"""Frames of an MSVideo1 seek index as a model-ready tensor batch (jsp_index_tensor, SeekIndex.Tensor, jsp_play --index-tensor) on an
MI355X.

Truth is the oracle, not the library: the pictures of test_index_present_gpu (the clip decoded frame by frame with OracleMSVideo1),
pushed through the numpy contract of Present (tests/index_present_ref.py) and then through the element rule and the layouts
(tests/index_tensor_ref.py).  Every comparison is of raw bytes: -0.0, ties and infinities count, and so does the poison behind the
tensor.  The cross-check on the device is Present into an int sheet followed by a table lookup with torch ops.

Shapes are those of test_index_present_gpu, whose fixtures are imported: a 134 x 98 picture, 72 frames behind 3 decoded ones and the
fresh-codec clip, 16 and 8 bit, both parse modes, the same picks."""
import os
import subprocess
import zlib

import numpy as np
import pytest

import index_present_cases as ic
import index_present_ref as ipr
import index_tensor_cases as tc
import index_tensor_ref as itr
import test_index_present_gpu as base
import view_ref as vr
from jsplayer_amd import CodecError, ScreenPressor
from jsplayer_amd import streamgen as sg

pytestmark = pytest.mark.gpu

FN = "index_tensor"
W, H, NF, PICKS = base.W, base.H, base.NF, base.PICKS


@pytest.fixture(autouse=True, params=["host", "gpu"])
def parse_mode(request):
    """Every test runs with the block tables of the host parser and of the on-GPU parse (base.Session reads base.PARSE)."""
    base.PARSE = request.param
    yield request.param
    base.PARSE = "host"


@pytest.mark.parametrize("before", [True, False], ids=["before", "fresh"])
@pytest.mark.parametrize("bits", [16, 8])
def test_every_dtype_layout_and_filter_matches_the_oracle(bits, before):
    s = base.Session(bits, before)
    what = f"{bits}-bit {'behind a picture' if before else 'fresh codec'} ({base.PARSE} parse)"
    tc.check_every_dtype_layout_and_filter(FN, s.gpu, s.idx, s.pictures, PICKS, W, H, vr.CANVAS, what)
    s.close()


@pytest.mark.parametrize("before", [True, False], ids=["before", "fresh"])
@pytest.mark.parametrize("bits", [16, 8])
def test_the_other_windows_and_the_scalar_path(bits, before):
    s = base.Session(bits, before)
    what = f"{bits}-bit {'behind a picture' if before else 'fresh codec'} ({base.PARSE} parse)"
    tc.check_the_other_windows(FN, s.gpu, s.idx, s.pictures, PICKS, W, H, vr.CANVAS, what)
    # the RGB15 conversion is taken as well (bytes 0, 1, 2 of its words are R, G, B too)
    k, dx, dy = vr.view_matrix(W, H, 100, 73, 0, 0.5, 0.5)
    tc.check(FN, s.gpu, s.idx, s.pictures, PICKS, W, H, 100, 73, k, dx, dy, vr.CANVAS_RGB15, ipr.AREA, itr.F16, itr.NHWC, what=what + " RGB15")
    s.close()


@pytest.mark.parametrize("bits", [16, 8])
def test_rounding(bits):
    s = base.Session(bits, True)
    tc.check_rounding(FN, s.gpu, s.idx, s.pictures, PICKS, W, H, vr.CANVAS, f"{bits}-bit ({base.PARSE} parse)")
    s.close()


@pytest.mark.parametrize("bits", [16, 8])
def test_tensor_is_present_plus_a_table_lookup_on_the_device(bits):
    s = base.Session(bits, True)
    tc.check_against_present_on_the_device(s.idx, PICKS, W, H, vr.CANVAS, f"{bits}-bit ({base.PARSE} parse)")
    # the defaults: PRESENT_AREA, float32, NCHW, v / 255
    k, dx, dy = vr.view_matrix(W, H, 50, 36, 0, 0.5, 0.5)
    got = s.idx.Tensor(PICKS[:3], 50, 36, k, dx, dy)
    want = itr.tensor([s.pictures[t] for t in PICKS[:3]], W, H, 50, 36, k, dx, dy, vr.CANVAS, ipr.AREA, 0xFF000000, itr.F32, itr.NCHW, (1 / 255,) * 3, (0,) * 3)
    assert tuple(got.shape) == (3, 3, 36, 50) and np.array_equal(got.cpu().numpy().view(np.uint32), want)
    s.close()


@pytest.mark.parametrize("bits", [16, 8])
def test_the_codec_is_only_lent(bits):
    """A session that asks for tensors and one that does not: the previous frame, the block-change counter and the next inter frame
    come out the same; poisoned pool buffers stay poisoned; the index grows by the frame list, not by a picture."""
    import torch
    runs = []
    for tensors in (True, False):
        s = base.Session(bits, True)
        prev = s.gpu.PreviousFrame()
        prev_pixels = prev.cpu().numpy().copy()
        free = [b for b in s.pool if b is not prev]
        for b in free:
            b.fill_(ic.POISON)
        dev0, _ = base.info(s.idx)
        if tensors:
            k, dx, dy = vr.view_matrix(W, H, 100, 73, 0, 0.5, 0.5)
            for f in ipr.FILTERS:
                s.idx.Tensor(PICKS, 100, 73, k, dx, dy, filter=f, dtype=torch.float16)
            s.idx.Tensor(list(range(NF)) * 3, 9, 7, 0.05, 0.0, 0.0, dtype=torch.uint8, layout="nhwc")
            dev1, _ = base.info(s.idx)
            assert 4 * 3 * NF <= dev1 - dev0 < W * H * 4
        assert s.gpu.PreviousFrame() is prev and np.array_equal(prev.cpu().numpy(), prev_pixels)
        for b in free:
            assert bool((b == ic.POISON).all()), "Tensor wrote a frame buffer"
        changes = s.gpu.counter("msv1_block_changes")
        nxt = free[0]
        nxt.copy_(prev)
        r = s.gpu.DecompressP(s.frames[s.start], nxt)
        runs.append((changes, s.gpu.counter("msv1_block_changes"), r.significant_changes, r.data_pnt is nxt, s.gpu.PreviousFrame().cpu().numpy().copy()))
        assert np.array_equal(runs[-1][4], s.pictures[0])
        s.close()
    a, b = runs
    assert a[:4] == b[:4] and np.array_equal(a[4], b[4])


def test_every_refusal_leaves_out_untouched_and_names_the_call():
    s = base.Session(16, True)
    a, idx = s.gpu, s.idx

    def in_flight():
        prev = a.PreviousFrame()
        ticket = a.DecompressP_async(s.frames[s.start], next(b for b in s.pool if b is not prev))
        return lambda: a.wait(ticket)

    other = base.make_gpu(16)
    sp = ScreenPressor(W, H, 24)
    tc.check_refusals(FN, a, idx, NF, "MSVideo1 only", in_flight, other, sp, "index: MSVideo1 only")
    sp.StopAndClean()
    other.StopAndClean()
    # and the call still works; a closed index / codec raise as Present does
    tc.check(FN, a, idx, s.pictures, [1, 0], W, H, 20, 10, 0.5, 0.0, 0.0, vr.CANVAS, ipr.BILINEAR, itr.F32, itr.NCHW)
    idx.close()
    with pytest.raises(CodecError, match="index is closed"):
        idx.Tensor([0], 20, 10, 0.5, 0, 0)
    idx2 = a.BuildIndex(s.frames[s.start:], s.keys[s.start:])
    a.StopAndClean()
    with pytest.raises(CodecError, match="codec is closed"):
        idx2.Tensor([0], 20, 10, 0.5, 0, 0)
    idx2.close()


def test_jsp_play_index_tensor_prints_the_crcs_of_the_python_path(tmp_path):
    import torch
    from jsplayer_amd import avi
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "examples", "jsp_play")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-s", "-C", os.path.join(root, "examples")])
    w, h, n = 320, 240, 40
    frames, keys, _ = sg.msv1_clip(97, w, h, n, p_mix=sg.msv1_p_mix(0.7, 6.0), key_every=16)
    path = tmp_path / "clip.avi"
    path.write_bytes(avi.write_avi(w, h, frames, fourcc=b"CRAM", bpp=16, fps=15.0, key_flags=keys))
    picks = [(i * n) // 9 for i in range(9)]
    g = base.make_gpu(16, w, h)
    with g.BuildIndex(frames, keys) as idx:
        for spec, arg, filter, dtype, layout in (("90x50", "9", 2, torch.float32, "nchw"), ("64x48", "9:1:f16:nhwc", 1, torch.float16, "nhwc"),
                                                 ("90x50", "9:0:u8", 0, torch.uint8, "nchw"), ("33x20", "9:2:bf16", 2, torch.bfloat16, "nchw")):
            ww, wh = (int(v) for v in spec.split("x"))
            res = subprocess.run([exe, str(path), "--index-tensor", spec, arg], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
            assert res.returncode == 0, res.stderr.decode()
            lines = [l.split() for l in res.stdout.decode().splitlines() if l and l[0].isdigit()]
            assert [int(l[0]) for l in lines] == picks
            k, dx, dy = vr.view_matrix(w, h, ww, wh, 0, 0.5, 0.5)
            got = idx.Tensor(picks, ww, wh, k, dx, dy, filter=filter, dtype=dtype, layout=layout)
            raw = got.view(torch.uint8).cpu().numpy().reshape(len(picks), -1)
            assert [l[1] for l in lines] == ["%08x" % (zlib.crc32(raw[i].tobytes()) & 0xFFFFFFFF) for i in range(len(picks))], spec + " " + arg
    g.StopAndClean()
    # the option goes alone and checks its arguments
    for extra in (["--index-tensor", "90x50", "0"], ["--index-tensor", "90x50", "4:3"], ["--index-tensor", "0x50", "4"], ["--index-tensor", "90x50:2", "4"],
                  ["--index-tensor", "90x50", "4:2:f64"], ["--index-tensor", "90x50", "4:2:f16:chwn"], ["--index-tensor", "90x50", "4", "--step-back"]):
        assert subprocess.run([exe, str(path)] + extra, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120).returncode == 2
