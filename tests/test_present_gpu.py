"""jsp_display_present (a frame in a window: conversion, row flip, crop and resampling in one launch) and Manager.present on an MI355X.

Truth: tests/view_ref.py — the rule of include/jsplayer_amd.h restated in numpy.  Every comparison is bit-exact."""
import ctypes as C
import math

import numpy as np
import pytest

import view_ref as vr
from jsplayer_amd import MSVideo1_16bit, ScreenPressor, _native as N, player
from jsplayer_amd import codec as cm
from jsplayer_amd import streamgen as sg

pytestmark = pytest.mark.gpu

CANARY = 0x5A5A5A5A
FRAMES = [(20, 12), (37, 23), (64, 36)]                       # 37 x 23: odd, rows that start on no 16-byte boundary
WINDOWS = [(16, 8), (33, 19), (15, 9), (128, 72), (64, 64)]   # 15 x 9: half-pixel offsets; 64 x 64: background, the fit() quirk
POSITIONS = [0.0, 0.3, 0.5, 1.0]
ZOOMS = [1.0, 2.0, 0.37, 3.5]
MODES = [cm.DISPLAY_CANVAS, cm.DISPLAY_CANVAS_RGB15, cm.DISPLAY_SETPIXELS, cm.DISPLAY_SETPIXELS_RGB15]
FILTERS = [cm.PRESENT_NEAREST, cm.PRESENT_BILINEAR]
RGB15 = (cm.DISPLAY_CANVAS_RGB15, cm.DISPLAY_SETPIXELS_RGB15)


def random_frame(w, h, mode, seed):
    """24-bit pixels; 5-bit components (15 bits) for the RGB15 modes."""
    bits = 15 if mode in RGB15 else 24
    return np.random.default_rng(seed).integers(0, 1 << bits, size=w * h, dtype=np.uint64).astype(np.uint32)


def to_dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).cuda()


def dev_full(n, fill=CANARY):
    import torch
    return torch.full((n,), fill, dtype=torch.int32, device="cuda")


def host(t):
    return t.cpu().numpy().view(np.uint32)


def views(fw, fh, ww, wh):
    """Fit, then 100 %, 200 %, k = 0.37 and k = 3.5 at every pair of view positions: (k, dx, dy) from the reference geometry."""
    out = [vr.view_matrix(fw, fh, ww, wh, 0, 0.5, 0.5)]
    for z in ZOOMS:
        for hor in POSITIONS:
            for ver in POSITIONS:
                out.append(vr.view_matrix(fw, fh, ww, wh, z, hor, ver))
    return out


@pytest.mark.parametrize("filt", FILTERS, ids=["nearest", "bilinear"])
@pytest.mark.parametrize("frame", FRAMES, ids=lambda f: f"{f[0]}x{f[1]}")
def test_every_view_of_small_frames_is_the_reference(frame, filt):
    import torch
    fw, fh = frame
    checked = quirk = partly = 0
    for mode in MODES:
        src = random_frame(fw, fh, mode, 100 + mode)
        d_src = to_dev(src)
        for (ww, wh) in WINDOWS:
            out = dev_full(ww * wh)
            for (k, dx, dy) in views(fw, fh, ww, wh):
                bg = 0xFF000000 if checked % 2 else 0x00123456
                cm.display_present(d_src, fw, fh, out, ww, wh, k, dx, dy, mode=mode, filter=filt, background=bg)
                want = vr.present(src, fw, fh, ww, wh, k, dx, dy, mode, filt, bg)
                got = host(out).reshape(wh, ww)
                bad = np.argwhere(got != want)
                assert len(bad) == 0, f"{frame} -> {ww}x{wh} k={k} dx={dx} dy={dy} mode={mode}: {len(bad)} pixels differ, first at {tuple(bad[0])}: {got[tuple(bad[0])]:08x} != {want[tuple(bad[0])]:08x}"
                checked += 1
                quirk += dx < 0 or dy < 0
                partly += bool(np.any(want == bg)) and bool(np.any(want != bg))
        assert np.array_equal(host(d_src), src)                # the frame is only read
    torch.cuda.synchronize()
    assert checked == len(MODES) * len(WINDOWS) * 65 and quirk > 0 and partly > 0


@pytest.mark.parametrize("filt", FILTERS, ids=["nearest", "bilinear"])
def test_windows_wider_and_taller_than_one_workgroup(filt):
    """More than one workgroup in x and in y, each with a remainder that is no multiple of a lane's run of 4 pixels (with the
    kernel's constants: a 520 x 6 frame at k = 2 into 1037 x 11)."""
    span, band = cm.PRESENT_SPAN_X, cm.PRESENT_BAND_ROWS
    ww, wh = 4 * span + 13, band + 3
    fw, fh = (ww + 1) // 2 + 1, (wh + 1) // 2
    src = random_frame(fw, fh, cm.DISPLAY_CANVAS, 7)
    d_src = to_dev(src)
    for (k, dx, dy, w, h) in [(2.0, 0.0, 0.0, ww, wh), (2.0, 3.0, 1.0, ww, wh), (1.0, 0.0, 0.0, fw, fh), (3.5, 10.5, 2.25, ww, 3 * band + 1), (0.37, 0.0, 0.0, span + 1, band + 1)]:
        out = dev_full(w * h)
        cm.display_present(d_src, fw, fh, out, w, h, k, dx, dy, filter=filt)
        want = vr.present(src, fw, fh, w, h, k, dx, dy, vr.CANVAS, filt)
        assert np.array_equal(host(out).reshape(h, w), want), (k, dx, dy, w, h)


@pytest.mark.parametrize("filt", FILTERS, ids=["nearest", "bilinear"])
def test_pitch_padding_and_memory_behind_the_window_are_untouched(filt):
    fw, fh, ww, wh = 37, 23, 33, 19
    src = random_frame(fw, fh, cm.DISPLAY_CANVAS, 11)
    d_src = to_dev(src)
    k, dx, dy = vr.view_matrix(fw, fh, ww, wh, 2, 0.3, 0.5)
    want = vr.present(src, fw, fh, ww, wh, k, dx, dy, vr.CANVAS, filt)
    for pitch in (ww + 3, ww + 4, ww + 7):                      # 36, 40: every row on a 16-byte boundary (vector stores); 37: scalar stores
        out = dev_full(wh * pitch + 9)
        cm.display_present(d_src, fw, fh, out, ww, wh, k, dx, dy, filter=filt, out_pitch=pitch)
        got = host(out)
        rows = got[:wh * pitch].reshape(wh, pitch)
        assert np.array_equal(rows[:, :ww], want), pitch
        assert np.all(rows[:, ww:] == CANARY), f"pitch {pitch}: padding written"
        assert np.all(got[wh * pitch:] == CANARY), f"pitch {pitch}: written behind the window"
    # an `out` that holds exactly (win_h - 1) * pitch + win_w ints
    pitch = ww + 7
    out = dev_full((wh - 1) * pitch + ww + 4)
    cm.display_present(d_src, fw, fh, out[:(wh - 1) * pitch + ww], ww, wh, k, dx, dy, filter=filt, out_pitch=pitch)
    got = host(out)
    assert np.all(got[(wh - 1) * pitch + ww:] == CANARY)
    assert np.array_equal(got[(wh - 1) * pitch:(wh - 1) * pitch + ww], want[-1])


@pytest.mark.parametrize("filt", FILTERS, ids=["nearest", "bilinear"])
def test_an_unaligned_out_takes_the_scalar_path_and_matches(filt):
    fw, fh, ww, wh = 64, 36, 128, 72
    src = random_frame(fw, fh, cm.DISPLAY_CANVAS, 12)
    d_src = to_dev(src)
    k, dx, dy = 2.0, 0.0, 0.0
    aligned = dev_full(ww * wh + 8)
    assert aligned.data_ptr() % 16 == 0
    cm.display_present(d_src, fw, fh, aligned, ww, wh, k, dx, dy, filter=filt)
    shifted = dev_full(ww * wh + 8)
    cm.display_present(d_src, fw, fh, shifted[1:], ww, wh, k, dx, dy, filter=filt)
    a, s = host(aligned), host(shifted)
    assert np.array_equal(a[:ww * wh], s[1:1 + ww * wh])
    assert np.array_equal(a[:ww * wh].reshape(wh, ww), vr.present(src, fw, fh, ww, wh, k, dx, dy, vr.CANVAS, filt))
    assert s[0] == CANARY and np.all(s[1 + ww * wh:] == CANARY) and np.all(a[ww * wh:] == CANARY)


def test_a_non_default_stream_is_honoured():
    import torch
    fw, fh, ww, wh = 64, 36, 33, 19
    src = random_frame(fw, fh, cm.DISPLAY_CANVAS, 13)
    d_src = to_dev(src)
    out = dev_full(ww * wh)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        handle = torch.cuda.current_stream().cuda_stream
        assert handle != 0
        cm.display_present(d_src, fw, fh, out, ww, wh, 0.37, 1.5, 2.5, stream=handle)
    side.synchronize()
    assert np.array_equal(host(out).reshape(wh, ww), vr.present(src, fw, fh, ww, wh, 0.37, 1.5, 2.5))


@pytest.mark.parametrize("mode", MODES)
def test_k1_with_integral_offsets_is_a_slice_of_display_convert(mode):
    """Ties the new call to the old one: at k = 1 with integral dx, dy both filters show rows fh - win_h - dy .. of the flipped
    jsp_display_convert picture, columns dx .. dx + win_w."""
    import torch
    fw, fh, ww, wh, dx, dy = 37, 23, 16, 8, 5, 3
    src = random_frame(fw, fh, mode, 14)
    d_src = to_dev(src)
    full = torch.empty_like(d_src)
    cm.display_convert(d_src, full, fw, fh, mode, True)
    want = host(full).reshape(fh, fw)[fh - wh - dy:fh - dy, dx:dx + ww]
    for filt in FILTERS:
        out = dev_full(ww * wh)
        cm.display_present(d_src, fw, fh, out, ww, wh, 1.0, float(dx), float(dy), mode=mode, filter=filt)
        assert np.array_equal(host(out).reshape(wh, ww), want), filt


def test_every_refusal_leaves_out_alone():
    import torch
    lib = N.lib()
    fw, fh, ww, wh = 20, 12, 16, 8
    d_src = to_dev(random_frame(fw, fh, 0, 15))
    out = dev_full(ww * wh + 64)
    f, o = d_src.data_ptr(), out.data_ptr()
    good = dict(frame=f, fw=fw, fh=fh, out=o, ww=ww, wh=wh, pitch=ww, k=1.0, dx=0.0, dy=0.0, mode=0, filter=1)
    bad = [dict(frame=None), dict(out=None),
           dict(fw=0), dict(fw=-1), dict(fw=16385), dict(fh=0), dict(fh=16385),
           dict(ww=0), dict(ww=16385, pitch=16385), dict(wh=0), dict(wh=-2), dict(wh=16385),
           dict(k=1.0 / 65), dict(k=64.5), dict(k=0.0), dict(k=-1.0), dict(k=math.nan), dict(k=math.inf),
           dict(dx=math.nan), dict(dx=math.inf), dict(dy=math.nan), dict(dy=-math.inf),
           dict(pitch=ww - 1), dict(pitch=0),
           dict(mode=-1), dict(mode=4), dict(filter=-1), dict(filter=2)]
    for change in bad:
        a = dict(good, **change)
        rc = lib.jsp_display_present(a["frame"], a["fw"], a["fh"], a["out"], a["ww"], a["wh"], a["pitch"], a["k"], a["dx"], a["dy"],
                                     a["mode"], a["filter"], 0xFF000000, None)
        assert rc == N.JSP_ERROR_OCCURED, change
        assert N.last_error().startswith("display_present:"), (change, N.last_error())
    torch.cuda.synchronize()
    assert np.all(host(out) == CANARY)
    with pytest.raises(cm.CodecError, match="^display_present:"):
        cm.display_present(d_src, fw, fh, out, ww, wh, 100.0, 0.0, 0.0)
    # the bounds themselves are accepted: k = 1/64 and k = 64, a far-away finite dx (all background)
    for k in (1.0 / 64, 64.0):
        cm.display_present(d_src, fw, fh, out, ww, wh, k, 0.0, 0.0)
        assert np.array_equal(host(out)[:ww * wh].reshape(wh, ww), vr.present(host(d_src), fw, fh, ww, wh, k, 0.0, 0.0)), k
    for far in (1e300, -1e300, 1e15, -1e15):
        cm.display_present(d_src, fw, fh, out, ww, wh, 1.0, far, 0.0, background=0x01020304)
        assert np.all(host(out)[:ww * wh] == 0x01020304), far
        cm.display_present(d_src, fw, fh, out, ww, wh, 1.0, 0.0, far, background=0x04030201)
        assert np.all(host(out)[:ww * wh] == 0x04030201), far
    assert np.all(host(out)[ww * wh:] == CANARY)


def _alloc(n):
    import torch
    return torch.zeros(n, dtype=torch.int32, device="cuda")


def test_manager_present_on_a_decoded_msvideo1_frame():
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
    ww, wh = 33, 19
    out = dev_full(ww * wh)
    mgr.present(slot, out, ww, wh)                                                  # Fit, bilinear, by slot number
    k, dx, dy = vr.view_matrix(w, h, ww, wh, 0, 0.5, 0.5)
    assert np.array_equal(host(out).reshape(wh, ww), vr.present(pic, w, h, ww, wh, k, dx, dy, vr.CANVAS, vr.BILINEAR))
    mgr.view.zoom_in()
    mgr.view.zoom_in()
    mgr.view.key(39)
    mgr.view.key(40)
    k, dx, dy = vr.view_matrix(w, h, ww, wh, 2, 0.5 + 0.1, 0.5 + 0.1)
    assert mgr.view.matrix(w, h, ww, wh) == (k, dx, dy)
    mgr.present(mgr.buffers[slot], out, ww, wh, filter=cm.PRESENT_NEAREST, background=0x11223344)   # by buffer
    assert np.array_equal(host(out).reshape(wh, ww), vr.present(pic, w, h, ww, wh, k, dx, dy, vr.CANVAS, vr.NEAREST, 0x11223344))
    with pytest.raises(ValueError):
        mgr.present(_alloc(w * h), out, ww, wh)
    assert np.array_equal(host(mgr.buffers[slot]), pic)
    dec.StopAndClean()


def test_manager_present_on_a_decoded_screenpressor_16bpp_frame():
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
    ww, wh = 128, 72
    out = dev_full(ww * wh)
    mgr.view.zoom_in()
    mgr.view.scroll(True, 0.3)
    mgr.present(slot, out, ww, wh)
    k, dx, dy = vr.view_matrix(w, h, ww, wh, 1, 0.3, 0.5)
    want = vr.present(pic, w, h, ww, wh, k, dx, dy, vr.CANVAS_RGB15, vr.BILINEAR)
    assert not np.array_equal(want, vr.present(pic, w, h, ww, wh, k, dx, dy, vr.CANVAS, vr.BILINEAR))   # (the mode matters here)
    assert np.array_equal(host(out).reshape(wh, ww), want)
    dec.StopAndClean()


@pytest.mark.parametrize("what", ["msvc16", "screenpressor16"])
def test_jsp_play_present_prints_the_windows_crc(what, tmp_path):
    """examples/jsp_play --present WxH:zoom:hpos:vpos: the plain run's lines, each with the CRC-32 of the window the frame shown
    gives under jsp_view_matrix + jsp_display_present (bilinear, the mode Manager.hx:121 picks)."""
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
        mode = vr.CANVAS
    else:
        frames, keys, _ = sg.sp_clip(3, w, h, n, bpp=16, version=4)
        blob = avi.write_avi(w, h, frames, fourcc=b"SCPR", bpp=16, key_flags=keys)
        mode = vr.CANVAS_RGB15
    path = tmp_path / "clip.avi"
    path.write_bytes(blob)
    plain = subprocess.run([exe, str(path)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert plain.returncode == 0, plain.stderr.decode()
    vi, got, got_keys = avi.read_avi_indexed(blob)
    mgr = player.Manager(vi, player.make_decoder(vi, (MSVideo1_16bit, None, ScreenPressor)), _alloc)
    pictures = []
    mgr.play(got, on_frame=lambda d, buf: pictures.append(host(buf).copy()), key_flags=got_keys)
    for spec, (ww, wh, zoom, hor, ver) in [("33x19:2:0.3:0.7", (33, 19, 2, 0.3, 0.7)), ("128x72", (128, 72, 0, 0.5, 0.5)), ("15x9:1", (15, 9, 1, 0.5, 0.5))]:
        res = subprocess.run([exe, str(path), "--present", spec], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
        assert res.returncode == 0, res.stderr.decode()
        lines = [l.split() for l in res.stdout.decode().splitlines()]
        assert [l[:5] for l in lines] == [l.split() for l in plain.stdout.decode().splitlines()] and len(lines) == n
        k, dx, dy = vr.view_matrix(w, h, ww, wh, zoom, hor, ver)
        for ln, pic in zip(lines, pictures):
            assert int(ln[4], 16) == zlib.crc32(pic.tobytes()), ln
            assert int(ln[5], 16) == zlib.crc32(vr.present(pic, w, h, ww, wh, k, dx, dy, mode, vr.BILINEAR).tobytes()), (spec, ln)
    assert subprocess.run([exe, str(path), "--present", "0x9"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60).returncode == 2
    mgr.decoder.StopAndClean()
