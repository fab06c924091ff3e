"""The activity map of a ScreenPressor seek index (jsp_sp_index_activity / SpScrubIndex.Activity) on an MI355X.

Truth: THE DEFINITION (tests/index_activity_ref.py: changed pixels per 16 x 16 block between whole pictures) over the encoder's
pictures, which test_sp_index_gpu pins to the oracle's sequential run, and over the oracle's run itself for the painted clips —
nothing of it comes from the GPU.  Every case compares the WHOLE array, exactly."""
import ctypes as C

import numpy as np
import pytest

import index_activity_ref as ar
import sp_directed_clips as dc
import sp_index_ref as ref
from jsplayer_amd import CodecError, ScreenPressor
from jsplayer_amd import _native as N
from test_sp_index_gpu import CLIPS, POISON, clip_id, dev_buf, make_sp, picture, sequential

pytestmark = pytest.mark.gpu


def whole_map(pictures, w, h):
    return ar.activity(pictures, np.zeros(w * h, dtype=np.uint32), w, h)


def check(idx, want, first, n, where):
    got = idx.Activity(first, n)
    assert tuple(got.shape) == (n,) + want.shape[1:] and str(got.dtype) == "torch.int16"
    got = got.cpu().numpy().view(np.uint16)
    assert np.array_equal(got, want[first:first + n]), f"{where} first={first} n={n}"
    return got


@pytest.mark.parametrize("case", CLIPS, ids=clip_id)
def test_generated_clips(case):
    cfg, w, h, n, bpp, version, key_every, key_row, _ = case
    clip = ref.make_clip(cfg, w, h, n, bpp, version, key_every, key_row)
    want = whole_map(clip.frames, w, h)
    gpu = make_sp(clip)
    idx = gpu.BuildScrubIndex(clip.chunks, clip.keys, key_row=key_row)
    assert idx.ActivitySize() == ar.grid(w, h)
    keys_at = [t for t in range(1, n) if clip.keys[t]]
    runs = [(0, n), (1, 1), (31, 3), (n - 1, 1), (5, n - 9)]
    runs += [(k, min(4, n - k)) for k in keys_at[:3]] + [(k + 1, min(4, n - k - 1)) for k in keys_at[:3] if k + 1 < n]
    whole = None
    for first, count in runs:
        got = check(idx, want, first, count, clip.name)
        whole = got if (first, count) == (0, n) else whole
    # unchanged frames are all zeros; a set bit is not a change: some rectangle covers pixels that stay
    assert any(not want[t].any() for t in range(1, n))
    if case is CLIPS[0]:   # (one clip's host-stage records are enough: literalised motion rewrites pixels as they were)
        comp = ref.Composer(clip)
        before = np.zeros(w * h, dtype=np.uint32)
        slack = []             # (frame, block row, block column, the rectangle's pixels there)
        for t in range(n):
            if t in comp.mask:
                stays = ar.cell_sums(comp.mask[t] & (clip.frames[t] == before).reshape(h, w), w, h)
                area = ar.cell_sums(comp.mask[t], w, h)
                slack += [(t, r, q, int(area[r, q])) for r, q in zip(*np.nonzero(stays))]
            before = clip.frames[t]
        assert slack, f"{clip.name}: every rectangle is all change"
        for t, r, q, area in slack:
            assert whole[t, r, q] < area, f"{clip.name} frame {t} block ({r}, {q}): the rectangle's area is not the count"
    assert gpu.PreviousFrame() is None
    idx.close()
    gpu.StopAndClean()


@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_painted_clips(name):
    clip = dc.clip(name)
    w, h, n = clip.w, clip.h, dc.N
    pictures, _ = dc.oracle(name)
    want = whole_map(pictures, w, h)
    gpu = make_sp(clip, lines=dc.KEY_ROW)
    idx = gpu.BuildScrubIndex(clip.chunks, clip.keys, key_row=dc.KEY_ROW)
    keys_at = [t for t in range(1, n) if clip.keys[t]]
    runs = [(0, n), (1, 1), (31, 3), (33, 64), (n - 1, 1)] + [(k, 3) for k in keys_at] + [(k + 1, 3) for k in keys_at]
    for first, count in runs:
        check(idx, want, first, count, clip.name)
    # every painted pixel differs from the frame before: the counts follow by hand from regions()
    got = check(idx, want, 0, n, clip.name).reshape(n, -1)
    for t in range(n):
        if clip.keys[t]:
            continue
        assert got[t, 0] == 1, f"{clip.name} frame {t}: block role 0 paints one pixel in every inter frame"
        areas = {b: (x2 - x1) * (y2 - y1) for b, (x1, y1, x2, y2) in dc.regions(t, w, h).items()}
        assert {b: int(v) for b, v in enumerate(got[t]) if v} == areas, f"{clip.name} frame {t}"
    for t in dc.REPAINTS:
        assert got[t, 4] == 256, f"{clip.name} frame {t}: block role 4 is the whole block"
    idx.close()
    gpu.StopAndClean()


def test_nothing_else_is_written_and_the_codec_is_only_lent():
    """A sentinel behind n * rows * cols and an unrelated frame buffer stay intact; `out=` is taken; the index grows by nothing the
    size of a picture; a codec half-way through ANOTHER clip goes on exactly as a twin that never saw the call."""
    import torch
    w, h = 100, 52
    own = ref.make_clip(61, w, h, 30, 24, 4, 9, 7)
    other = ref.make_clip(62, w, h, 41, 24, 4, 13, 7)
    want = whole_map(other.frames, w, h)
    gpu, twin = make_sp(own), make_sp(own)
    pool, tpool = [dev_buf(w * h) for _ in range(3)], [dev_buf(w * h) for _ in range(3)]
    a = sequential(gpu, own.chunks, own.keys, 0, 14, pool)
    b = sequential(twin, own.chunks, own.keys, 0, 14, tpool)
    idx = gpu.BuildScrubIndex(other.chunks, other.keys, key_row=7)
    cols, rows = idx.ActivitySize()
    cell = rows * cols
    first, n = 3, 30
    raw = torch.full((n * cell + 64,), 0x7BCD, dtype=torch.int16, device="cuda")
    bystander = dev_buf(w * h)
    prev = gpu.PreviousFrame()
    prev_pic = picture(prev).copy()
    dev_before = idx.device_bytes
    lib = N.lib()
    assert lib.jsp_sp_index_activity(gpu._h, idx._h, first, n, C.c_void_p(raw.data_ptr()), n * cell) == 0, N.last_error()
    host = raw.cpu().numpy()
    assert np.array_equal(host[:n * cell].view(np.uint16).reshape(n, rows, cols), want[first:first + n])
    assert np.all(host[n * cell:] == 0x7BCD), "written behind n * rows * cols"
    assert np.all(picture(bystander) == POISON)
    idx._info()
    assert idx.device_bytes - dev_before <= 16 * idx.frames + 4 * ((idx.frames + 31) // 32) + 16, "the per-frame table of Play, no more"
    out = torch.full((n, rows, cols), 0x7BCD, dtype=torch.int16, device="cuda")
    assert idx.Activity(first, n, out=out) is out and np.array_equal(out.cpu().numpy().view(np.uint16), want[first:first + n])
    with pytest.raises(CodecError):
        idx.Activity(first, n, out=out.to(torch.int32))
    assert gpu.PreviousFrame() is prev and np.array_equal(picture(prev), prev_pic)
    for lo, hi in ((14, 15), (15, 22), (22, 30)):
        check(idx, want, 0, 41, other.name)
        a += sequential(gpu, own.chunks, own.keys, lo, hi, pool)
        b += sequential(twin, own.chunks, own.keys, lo, hi, tpool)
    for i, (x, y) in enumerate(zip(a, b)):
        assert np.array_equal(x[0], y[0]) and x[1] == y[1] and x[2] == y[2], f"frame {i} after Activity differs from the twin's"
    idx.close()
    gpu.StopAndClean()
    twin.StopAndClean()
