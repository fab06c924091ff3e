"""jsp_display_present_area (a frame in a window, area-averaged: conversion, row flip, crop and box filter in one launch) and
Manager.present(filter=PRESENT_AREA) on an MI355X.

Truth: tests/view_area_ref.py — the rule of include/jsplayer_amd.h restated in numpy.  Every comparison is bit-exact."""
import math

import numpy as np
import pytest

import view_area_ref as ar
import view_ref as vr
from jsplayer_amd import MSVideo1_16bit, ScreenPressor, _native as N, player
from jsplayer_amd import codec as cm
from jsplayer_amd import streamgen as sg

pytestmark = pytest.mark.gpu

CANARY = 0x5A5A5A5A
PARTS = ["views", "edges", "modes", "large", "taps", "seams"]


def random_frame(w, h, seed, bits=24):
    return np.random.default_rng(seed).integers(0, 1 << bits, size=w * h, dtype=np.uint64).astype(np.uint32)


def to_dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).cuda()


def dev_full(n, fill=CANARY):
    import torch
    return torch.full((n,), fill, dtype=torch.int32, device="cuda")


def host(t):
    return t.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("part", PARTS)
def test_every_case_of_the_shared_list_is_the_reference(part):
    cases = [c for c in ar.CASES if c.part == part]
    assert cases
    frames = {}                                                # one upload per distinct frame
    for i, c in enumerate(cases):
        (fw, fh), (ww, wh) = c.frame, c.window
        key = (c.frame, c.pixels, c.seed, c.mode in ar.RGB15)
        if key not in frames:
            src = ar.frame_words(c)
            frames[key] = (src, to_dev(src))
        src, d_src = frames[key]
        bg = 0xFF000000 if i % 2 else 0x00123456
        out = dev_full(ww * wh + 4)
        cm.display_present_area(d_src, fw, fh, out, ww, wh, c.k, c.dx, c.dy, mode=c.mode, background=bg)
        want = ar.present_area(src, fw, fh, ww, wh, c.k, c.dx, c.dy, c.mode, bg)
        got = host(out)
        assert np.all(got[ww * wh:] == CANARY), c
        got = got[:ww * wh].reshape(wh, ww)
        bad = np.argwhere(got != want)
        assert len(bad) == 0, f"{c}: {len(bad)} pixels differ, first at {tuple(bad[0])}: {got[tuple(bad[0])]:08x} != {want[tuple(bad[0])]:08x}"
    for (src, d_src) in frames.values():
        assert np.array_equal(host(d_src), src)                # the frame is only read


def test_white_frames_stay_white_where_the_sum_passes_32_bits():
    for (fw, fh, ww, wh, k) in [(130, 130, 2, 2, 1 / 64), (200, 120, 10, 6, 0.05)]:
        d_src = to_dev(np.full(fw * fh, 0xFFFFFF, dtype=np.uint32))
        out = dev_full(ww * wh)
        cm.display_present_area(d_src, fw, fh, out, ww, wh, k, 0.0, 0.0, mode=cm.DISPLAY_CANVAS, background=0)
        assert np.all(host(out) == 0xFFFFFFFF), (fw, fh)


def test_pitch_padding_and_memory_behind_the_window_are_untouched():
    fw, fh, ww, wh = 100, 52, 33, 17
    src = random_frame(fw, fh, 11)
    d_src = to_dev(src)
    k, dx, dy = 1 / 3, 0.5, 0.25
    want = ar.present_area(src, fw, fh, ww, wh, k, dx, dy)
    for pitch in (ww + 3, ww + 4, ww + 7):                      # 36, 40: every row on a 16-byte boundary; 37: rows on every remainder
        out = dev_full(wh * pitch + 9)
        cm.display_present_area(d_src, fw, fh, out, ww, wh, k, dx, dy, out_pitch=pitch)
        got = host(out)
        rows = got[:wh * pitch].reshape(wh, pitch)
        assert np.array_equal(rows[:, :ww], want), pitch
        assert np.all(rows[:, ww:] == CANARY), f"pitch {pitch}: padding written"
        assert np.all(got[wh * pitch:] == CANARY), f"pitch {pitch}: written behind the window"
    # an `out` that holds exactly (win_h - 1) * pitch + win_w ints
    pitch = ww + 7
    out = dev_full((wh - 1) * pitch + ww + 4)
    cm.display_present_area(d_src, fw, fh, out[:(wh - 1) * pitch + ww], ww, wh, k, dx, dy, out_pitch=pitch)
    got = host(out)
    assert np.all(got[(wh - 1) * pitch + ww:] == CANARY)
    assert np.array_equal(got[(wh - 1) * pitch:(wh - 1) * pitch + ww], want[-1])


def test_an_out_shifted_by_one_int_matches():
    fw, fh, ww, wh = 600, 40, 300, 20
    src = random_frame(fw, fh, 12)
    d_src = to_dev(src)
    k, dx, dy = 0.5, 0.0, 0.0
    aligned = dev_full(ww * wh + 8)
    assert aligned.data_ptr() % 16 == 0
    cm.display_present_area(d_src, fw, fh, aligned, ww, wh, k, dx, dy)
    shifted = dev_full(ww * wh + 8)
    cm.display_present_area(d_src, fw, fh, shifted[1:], ww, wh, k, dx, dy)
    a, s = host(aligned), host(shifted)
    assert np.array_equal(a[:ww * wh], s[1:1 + ww * wh])
    assert np.array_equal(a[:ww * wh].reshape(wh, ww), ar.present_area(src, fw, fh, ww, wh, k, dx, dy))
    assert s[0] == CANARY and np.all(s[1 + ww * wh:] == CANARY) and np.all(a[ww * wh:] == CANARY)


def test_a_non_default_stream_is_honoured():
    import torch
    fw, fh, ww, wh = 64, 48, 21, 16
    src = random_frame(fw, fh, 13)
    d_src = to_dev(src)
    out = dev_full(ww * wh)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        handle = torch.cuda.current_stream().cuda_stream
        assert handle != 0
        cm.display_present_area(d_src, fw, fh, out, ww, wh, 1 / 3, 1.5, 2.5, stream=handle)
    side.synchronize()
    assert np.array_equal(host(out).reshape(wh, ww), ar.present_area(src, fw, fh, ww, wh, 1 / 3, 1.5, 2.5))


@pytest.mark.parametrize("mode", ar.MODES)
def test_k1_with_integral_offsets_is_a_slice_of_display_convert(mode):
    import torch
    fw, fh, ww, wh, dx, dy = 37, 23, 16, 8, 5, 3
    src = random_frame(fw, fh, 14, 15 if mode in ar.RGB15 else 24)
    d_src = to_dev(src)
    full = torch.empty_like(d_src)
    cm.display_convert(d_src, full, fw, fh, mode, True)
    want = host(full).reshape(fh, fw)[fh - wh - dy:fh - dy, dx:dx + ww]
    out = dev_full(ww * wh)
    cm.display_present_area(d_src, fw, fh, out, ww, wh, 1.0, float(dx), float(dy), mode=mode)
    assert np.array_equal(host(out).reshape(wh, ww), want)


def test_every_refusal_leaves_out_alone():
    import torch
    lib = N.lib()
    fw, fh, ww, wh = 20, 12, 16, 8
    d_src = to_dev(random_frame(fw, fh, 15))
    out = dev_full(ww * wh + 64)
    f, o = d_src.data_ptr(), out.data_ptr()
    good = dict(frame=f, fw=fw, fh=fh, out=o, ww=ww, wh=wh, pitch=ww, k=1.0, dx=0.0, dy=0.0, mode=0)
    bad = [dict(frame=None), dict(out=None),
           dict(fw=0), dict(fw=-1), dict(fw=16385), dict(fh=0), dict(fh=16385),
           dict(ww=0), dict(ww=16385, pitch=16385), dict(wh=0), dict(wh=-2), dict(wh=16385),
           dict(k=1.0 / 65), dict(k=64.5), dict(k=0.0), dict(k=-1.0), dict(k=math.nan), dict(k=math.inf),
           dict(dx=math.nan), dict(dx=math.inf), dict(dy=math.nan), dict(dy=-math.inf),
           dict(pitch=ww - 1), dict(pitch=0),
           dict(mode=-1), dict(mode=4)]
    for change in bad:
        a = dict(good, **change)
        rc = lib.jsp_display_present_area(a["frame"], a["fw"], a["fh"], a["out"], a["ww"], a["wh"], a["pitch"], a["k"], a["dx"], a["dy"],
                                          a["mode"], 0xFF000000, None)
        assert rc == N.JSP_ERROR_OCCURED, change
        assert N.last_error().startswith("display_present_area:"), (change, N.last_error())
    torch.cuda.synchronize()
    assert np.all(host(out) == CANARY)
    with pytest.raises(cm.CodecError, match="^display_present_area:"):
        cm.display_present_area(d_src, fw, fh, out, ww, wh, 100.0, 0.0, 0.0)
    with pytest.raises(cm.CodecError, match="^display_present_area:"):
        cm.display_present_area(host(d_src), fw, fh, out, ww, wh, 1.0, 0.0, 0.0)      # a host array
    assert np.all(host(out) == CANARY)
    # the bounds themselves are accepted: k = 1/64 and k = 64, a far-away finite dx (all background)
    for k in (1.0 / 64, 64.0):
        cm.display_present_area(d_src, fw, fh, out, ww, wh, k, 0.0, 0.0)
        assert np.array_equal(host(out)[:ww * wh].reshape(wh, ww), ar.present_area(host(d_src), fw, fh, ww, wh, k, 0.0, 0.0)), k
    for far in (1e300, -1e300, 1e15, -1e15):
        cm.display_present_area(d_src, fw, fh, out, ww, wh, 1.0, far, 0.0, background=0x01020304)
        assert np.all(host(out)[:ww * wh] == 0x01020304), far
        cm.display_present_area(d_src, fw, fh, out, ww, wh, 1.0, 0.0, far, background=0x04030201)
        assert np.all(host(out)[:ww * wh] == 0x04030201), far
    assert np.all(host(out)[ww * wh:] == CANARY)


def test_display_present_still_refuses_the_area_filter():
    """The other call's contract, restated: jsp_display_present takes filters 0 and 1 and nothing else."""
    import torch
    fw, fh, ww, wh = 20, 12, 16, 8
    d_src = to_dev(random_frame(fw, fh, 16))
    out = dev_full(ww * wh)
    rc = N.lib().jsp_display_present(d_src.data_ptr(), fw, fh, out.data_ptr(), ww, wh, ww, 1.0, 0.0, 0.0, 0, cm.PRESENT_AREA, 0xFF000000, None)
    assert rc == N.JSP_ERROR_OCCURED and N.last_error().startswith("display_present: unknown filter")
    with pytest.raises(cm.CodecError, match="^display_present: unknown filter"):
        cm.display_present(d_src, fw, fh, out, ww, wh, 1.0, 0.0, 0.0, filter=cm.PRESENT_AREA)
    torch.cuda.synchronize()
    assert np.all(host(out) == CANARY)


def _alloc(n):
    import torch
    return torch.zeros(n, dtype=torch.int32, device="cuda")


def test_manager_present_area_on_a_decoded_msvideo1_frame():
    from jsplayer_amd.avi import CODEC_MSVC16, VideoInfo
    w, h, n = 64, 48, 3
    frames, keys, _ = sg.msv1_clip(1, w, h, n, p_mix=sg.msv1_p_mix(0.7, 40.0))
    vi = VideoInfo(X=w, Y=h, bpp=16, fps=15.0, nframes=n, codec=CODEC_MSVC16, palette=None, riff_size=0)
    dec = MSVideo1_16bit(w, h)
    mgr = player.Manager(vi, dec, _alloc)
    mgr.play(frames, key_flags=keys)
    slot = mgr.log[-1].buffer_index
    pic = host(mgr.buffers[slot])
    assert len(np.unique(pic)) > 16
    ww, wh = 21, 16
    out = dev_full(ww * wh)
    mgr.present(slot, out, ww, wh, filter=cm.PRESENT_AREA)                          # Fit (k = 21/64), by slot number
    k, dx, dy = vr.view_matrix(w, h, ww, wh, 0, 0.5, 0.5)
    want = ar.present_area(pic, w, h, ww, wh, k, dx, dy, ar.CANVAS)
    assert np.array_equal(host(out).reshape(wh, ww), want)
    mgr.present(slot, out, ww, wh)                                                  # the default stays bilinear
    bil = vr.present(pic, w, h, ww, wh, k, dx, dy, vr.CANVAS, vr.BILINEAR)
    assert np.array_equal(host(out).reshape(wh, ww), bil) and not np.array_equal(bil, want)
    mgr.present(mgr.buffers[slot], out, ww, wh, filter=cm.PRESENT_AREA, background=0x11223344)   # by buffer
    assert np.array_equal(host(out).reshape(wh, ww), ar.present_area(pic, w, h, ww, wh, k, dx, dy, ar.CANVAS, 0x11223344))
    with pytest.raises(ValueError):
        mgr.present(_alloc(w * h), out, ww, wh, filter=cm.PRESENT_AREA)
    assert np.array_equal(host(mgr.buffers[slot]), pic)
    dec.StopAndClean()


def test_manager_present_area_on_a_decoded_screenpressor_16bpp_frame():
    """16-bpp ScreenPressor frames hold 5-bit components: the Manager picks JSP_DISPLAY_CANVAS_RGB15 (Manager.hx:121, 370)."""
    from jsplayer_amd.avi import CODEC_SCREENPRESSOR, VideoInfo
    w, h, n = 64, 48, 3
    chunks, keys, frames = sg.sp_clip(3, w, h, n, bpp=16, version=4)
    vi = VideoInfo(X=w, Y=h, bpp=16, fps=15.0, nframes=n, codec=CODEC_SCREENPRESSOR, palette=None, riff_size=0)
    dec = ScreenPressor(w, h, 16)
    mgr = player.Manager(vi, dec, _alloc)
    mgr.play(chunks, key_flags=keys)
    slot = mgr.log[-1].buffer_index
    pic = host(mgr.buffers[slot])
    assert np.array_equal(pic, frames[-1].astype(np.uint32))
    ww, wh = 30, 30
    out = dev_full(ww * wh)
    mgr.present(slot, out, ww, wh, filter=cm.PRESENT_AREA)                          # Fit with background bars
    k, dx, dy = vr.view_matrix(w, h, ww, wh, 0, 0.5, 0.5)
    want = ar.present_area(pic, w, h, ww, wh, k, dx, dy, ar.CANVAS_RGB15)
    assert not np.array_equal(want, ar.present_area(pic, w, h, ww, wh, k, dx, dy, ar.CANVAS))   # (the mode matters here)
    assert np.array_equal(host(out).reshape(wh, ww), want)
    dec.StopAndClean()


@pytest.mark.parametrize("what", ["msvc16", "screenpressor16"])
def test_jsp_play_present_area_prints_the_windows_crc(what, tmp_path):
    """examples/jsp_play --present-area WxH:zoom:hpos:vpos: the plain run's lines, each with the CRC-32 of the window the frame shown
    gives under jsp_view_matrix + jsp_display_present_area (the mode Manager.hx:121 picks)."""
    import os
    import subprocess
    import zlib
    from jsplayer_amd import avi
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "examples", "jsp_play")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-s", "-C", os.path.join(root, "examples")])
    w, h, n = 64, 48, 4
    if what == "msvc16":
        frames, keys, _ = sg.msv1_clip(1, w, h, n, p_mix=sg.msv1_p_mix(0.7, 40.0))
        blob = avi.write_avi(w, h, frames, fourcc=b"CRAM", bpp=16, fps=15.0, key_flags=keys)
        mode = ar.CANVAS
    else:
        frames, keys, _ = sg.sp_clip(3, w, h, n, bpp=16, version=4)
        blob = avi.write_avi(w, h, frames, fourcc=b"SCPR", bpp=16, key_flags=keys)
        mode = ar.CANVAS_RGB15
    path = tmp_path / "clip.avi"
    path.write_bytes(blob)
    plain = subprocess.run([exe, str(path)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert plain.returncode == 0, plain.stderr.decode()
    vi, got, got_keys = avi.read_avi_indexed(blob)
    mgr = player.Manager(vi, player.make_decoder(vi, (MSVideo1_16bit, None, ScreenPressor)), _alloc)
    pictures = []
    mgr.play(got, on_frame=lambda d, buf: pictures.append(host(buf).copy()), key_flags=got_keys)
    for spec, (ww, wh, zoom, hor, ver) in [("21x16", (21, 16, 0, 0.5, 0.5)), ("16x12:0.25:0.3:0.7", (16, 12, 0.25, 0.3, 0.7)), ("30x30", (30, 30, 0, 0.5, 0.5))]:
        res = subprocess.run([exe, str(path), "--present-area", spec], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
        assert res.returncode == 0, res.stderr.decode()
        lines = [l.split() for l in res.stdout.decode().splitlines()]
        assert [l[:5] for l in lines] == [l.split() for l in plain.stdout.decode().splitlines()] and len(lines) == n
        k, dx, dy = vr.view_matrix(w, h, ww, wh, zoom, hor, ver)
        for ln, pic in zip(lines, pictures):
            assert int(ln[4], 16) == zlib.crc32(pic.tobytes()), ln
            assert int(ln[5], 16) == zlib.crc32(ar.present_area(pic, w, h, ww, wh, k, dx, dy, mode).tobytes()), (spec, ln)
    assert subprocess.run([exe, str(path), "--present-area", "0x9"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60).returncode == 2
    mgr.decoder.StopAndClean()
