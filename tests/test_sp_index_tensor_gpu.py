"""Frames of a ScreenPressor seek index as a model-ready tensor batch (jsp_sp_index_tensor, SpScrubIndex.Tensor, jsp_play
--index-tensor) on an MI355X.

Truth: the oracle's pictures of test_sp_index_present_gpu (which are also the encoder's), pushed through the numpy contract of Present
(tests/index_present_ref.py) and then through the element rule and the layouts (tests/index_tensor_ref.py).  Every comparison is of raw
bytes, the poison behind the tensor included.  The cross-check on the device is Present into an int sheet followed by a table lookup
with torch ops.

Shapes are those of test_sp_index_present_gpu, whose fixtures are imported: its clips 0 (150 wide, 24 bpp) and 3 (148 wide, 16 bpp:
the RGB15 conversion and the 16-byte key-picture loads) and its picks."""
import os
import subprocess
import zlib

import numpy as np
import pytest

import index_present_cases as ic
import index_present_ref as ipr
import index_tensor_cases as tc
import index_tensor_ref as itr
import sp_index_ref as ref
import test_sp_index_present_gpu as base
import view_ref as vr
from jsplayer_amd import CodecError, MSVideo1_16bit, ScreenPressor
from jsplayer_amd import streamgen as sg

pytestmark = pytest.mark.gpu

FN = "sp_index_tensor"
H, PICKS = base.H, base.PICKS
CASES = [base.CLIPS[0], base.CLIPS[3]]
IDS = ["150wide_24bpp", "148wide_16bpp"]


def session(case):
    clip, pictures = base.get_clip(case)
    gpu = base.make_sp(clip)
    idx = gpu.BuildScrubIndex(clip.chunks, clip.keys, key_row=7)
    return clip, pictures, gpu, idx, (vr.CANVAS_RGB15 if clip.bpp == 16 else vr.CANVAS)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_every_dtype_layout_and_filter_matches_the_oracle(case):
    clip, pictures, gpu, idx, mode = session(case)
    tc.check_every_dtype_layout_and_filter(FN, gpu, idx, pictures, PICKS, clip.w, H, mode, clip.name)
    assert gpu.PreviousFrame() is None
    idx.close()
    gpu.StopAndClean()


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_the_other_windows_and_the_scalar_path(case):
    clip, pictures, gpu, idx, mode = session(case)
    tc.check_the_other_windows(FN, gpu, idx, pictures, PICKS, clip.w, H, mode, clip.name)
    idx.close()
    gpu.StopAndClean()


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_rounding(case):
    clip, pictures, gpu, idx, mode = session(case)
    tc.check_rounding(FN, gpu, idx, pictures, PICKS, clip.w, H, mode, clip.name)
    idx.close()
    gpu.StopAndClean()


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_tensor_is_present_plus_a_table_lookup_on_the_device(case):
    clip, pictures, gpu, idx, mode = session(case)
    tc.check_against_present_on_the_device(idx, PICKS, clip.w, H, mode, clip.name)
    # the defaults: PRESENT_AREA, float32, NCHW, v / 255, and the conversion that gives canvas pixels — RGB15 for 16 bpp
    k, dx, dy = vr.view_matrix(clip.w, H, 50, 36, 0, 0.5, 0.5)
    got = idx.Tensor(PICKS[:3], 50, 36, k, dx, dy)
    want = itr.tensor([pictures[t] for t in PICKS[:3]], clip.w, H, 50, 36, k, dx, dy, mode, ipr.AREA, 0xFF000000, itr.F32, itr.NCHW, (1 / 255,) * 3, (0,) * 3)
    assert tuple(got.shape) == (3, 3, 36, 50) and np.array_equal(got.cpu().numpy().view(np.uint32), want)
    idx.close()
    gpu.StopAndClean()


def test_the_codec_is_only_lent():
    """A codec half-way through ANOTHER clip builds an index and asks for tensors between its decodes: no frame buffer is written, and
    every later picture, verdict and data_pnt equals a twin's that never saw an index.  The index grows by the per-cell records, not by
    a picture."""
    import torch
    w, h = 100, 52
    own = ref.make_clip(81, w, h, 30, 24, 4, 9, 7)
    other = ref.make_clip(82, w, h, 41, 24, 4, 13, 7)
    gpu, twin = base.make_sp(own), base.make_sp(own)
    pool, tpool = [ic.dev_buf(w * h) for _ in range(3)], [ic.dev_buf(w * h) for _ in range(3)]
    a = base.sequential(gpu, own.chunks, own.keys, 0, 14, pool)
    b = base.sequential(twin, own.chunks, own.keys, 0, 14, tpool)
    idx = gpu.BuildScrubIndex(other.chunks, other.keys, key_row=7)
    dev0, _ = base.info(idx)
    k, dx, dy = vr.view_matrix(w, h, 64, 30, 0, 0.5, 0.5)
    for lo, hi in ((14, 15), (15, 22), (22, 30)):
        prev = gpu.PreviousFrame()
        pool_pics = [base.picture(p).copy() for p in pool]
        for f in ipr.FILTERS:
            idx.Tensor([40, 17, 3, 25, 0, 13], 64, 30, k, dx, dy, filter=f, dtype=torch.bfloat16)
        idx.Tensor(list(range(idx.frames)) * 2, 9, 5, 0.05, 0.0, 0.0, dtype=torch.uint8, layout="nhwc")
        assert gpu.PreviousFrame() is prev
        for p, pic in zip(pool, pool_pics):
            assert np.array_equal(base.picture(p), pic), "Tensor wrote a frame buffer"
        a += base.sequential(gpu, own.chunks, own.keys, lo, hi, pool)
        b += base.sequential(twin, own.chunks, own.keys, lo, hi, tpool)
    dev1, _ = base.info(idx)
    assert 24 * 82 <= dev1 - dev0 < w * h * 4
    for i, (x, y) in enumerate(zip(a, b)):
        assert np.array_equal(x[0], y[0]) and x[1] == y[1] and x[2] == y[2], f"frame {i} after Tensor differs from the twin's"
        assert np.array_equal(x[0], own.frames[i]), f"frame {i}: not the encoder's picture"
    idx.close()
    gpu.StopAndClean()
    twin.StopAndClean()


def test_every_refusal_leaves_out_untouched_and_names_the_call():
    w, h = 64, 48
    clip = ref.make_clip(85, w, h, 41, 24, 4, 13, 36)
    pictures, _ = ref.oracle_run(clip)
    gpu = base.make_sp(clip)
    pool = [ic.dev_buf(w * h) for _ in range(3)]
    base.sequential(gpu, clip.chunks, clip.keys, 0, 5, pool)
    idx = gpu.BuildScrubIndex(clip.chunks, clip.keys)

    def in_flight():
        prev = gpu.PreviousFrame()
        ticket = gpu.DecompressP_async(clip.chunks[5], next(b for b in pool if b is not prev))
        return lambda: gpu.wait(ticket)

    other = base.make_sp(clip)
    msv = MSVideo1_16bit(w, h)
    tc.check_refusals(FN, gpu, idx, idx.frames, "ScreenPressor only", in_flight, other, msv, "sp_index: ScreenPressor only")
    msv.StopAndClean()
    other.StopAndClean()
    # and the call still works, the codec's stream goes on; a closed index / codec raise as Present does
    tc.check(FN, gpu, idx, pictures, [1, 0], w, h, 20, 10, 0.5, 0.0, 0.0, vr.CANVAS, ipr.BILINEAR, itr.F32, itr.NCHW)
    after = base.sequential(gpu, clip.chunks, clip.keys, 6, 12, pool)
    for i, got in enumerate(after, start=6):
        assert np.array_equal(got[0], pictures[i]), f"frame {i} after the refusals"
    idx.close()
    with pytest.raises(CodecError, match="index is closed"):
        idx.Tensor([0], 20, 10, 0.5, 0, 0)
    idx2 = gpu.BuildScrubIndex(clip.chunks, clip.keys)
    gpu.StopAndClean()
    with pytest.raises(CodecError, match="codec is closed"):
        idx2.Tensor([0], 20, 10, 0.5, 0, 0)
    idx2.close()


def test_jsp_play_index_tensor_on_a_screenpressor_avi(tmp_path):
    import torch
    from jsplayer_amd import avi
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "examples", "jsp_play")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-s", "-C", os.path.join(root, "examples")])
    w, h, n = 320, 240, 40
    chunks, keys, frames = sg.sp_clip(97, w, h, n, bpp=16, version=4, key_every=12, unchanged_at=(5,))
    path = tmp_path / "clip.avi"
    path.write_bytes(avi.write_avi(w, h, chunks, fourcc=b"SCPR", bpp=16, fps=15.0, key_flags=keys))
    picks = [(i * n) // 9 for i in range(9)]
    gpu = ScreenPressor(w, h, 16)
    gpu.Preinit(36)
    idx = gpu.BuildScrubIndex(chunks, keys)
    for spec, arg, filter, dtype, layout in (("90x50", "9", 2, torch.float32, "nchw"), ("64x48", "9:1:f16:nhwc", 1, torch.float16, "nhwc"),
                                             ("90x50", "9:0:u8:nhwc", 0, torch.uint8, "nhwc")):
        ww, wh = (int(v) for v in spec.split("x"))
        res = subprocess.run([exe, str(path), "--index-tensor", spec, arg], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
        assert res.returncode == 0, res.stderr.decode()
        lines = [l.split() for l in res.stdout.decode().splitlines() if l and l[0].isdigit()]
        assert [int(l[0]) for l in lines] == picks
        k, dx, dy = vr.view_matrix(w, h, ww, wh, 0, 0.5, 0.5)
        got = idx.Tensor(picks, ww, wh, k, dx, dy, filter=filter, dtype=dtype, layout=layout)      # 16 bpp: the RGB15 conversion by default
        raw = got.view(torch.uint8).cpu().numpy().reshape(len(picks), -1)
        assert [l[1] for l in lines] == ["%08x" % (zlib.crc32(raw[i].tobytes()) & 0xFFFFFFFF) for i in range(len(picks))], spec + " " + arg
    idx.close()
    gpu.StopAndClean()
    for extra in (["--index-tensor", "90x50", "0"], ["--index-tensor", "90x50", "4:2:u16"], ["--index-tensor", "90x50", "4", "--filmstrip", "3"]):
        assert subprocess.run([exe, str(path)] + extra, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120).returncode == 2
