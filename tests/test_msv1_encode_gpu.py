"""The MSVideo1 16-bit encoder (jsp_msv1_encode_frames / Msv1Encoder / Manager.transcode, proxy) on an MI355X.

Truth: tests/msv1_encode_ref.py, the rule in plain Python, which test_msv1_encode_ref_cpu.py pins to the oracle — nothing of it comes
from the GPU.  Every case compares BYTES, exactly; the round trips compare pictures, exactly."""
import ctypes as C
import functools

import numpy as np
import pytest

import msv1_encode_ref as er
from index_delta_ref import skip_word, walk
from jsplayer_amd import CodecError, MSVideo1_16bit, Msv1Encoder, ScreenPressor, player
from jsplayer_amd import _native as N
from jsplayer_amd import streamgen as sg
from jsplayer_amd.avi import CODEC_MSVC16, CODEC_SCREENPRESSOR, VideoInfo
from oracle_binding import OracleMSVideo1

pytestmark = pytest.mark.gpu

POISON = 0x5A5A5A5A
FILL = 0xA5
SLICE = 16          # kEncodeMaxSlice (msv1_encode.cpp): pictures a slice at most; small pictures get exactly this
WG_BLOCKS = 1024    # MSV1_KEYFRAME_WG_BLOCKS (msv1_seek.h)
SIZES = [(4, 4), (22, 9), (128, 128), (256, 128), (260, 132)]
LAYOUTS = ("aligned", "off4", "sheet", "negative")


def torch():
    import torch as t
    return t


def runs(nb):
    """Sets of coded blocks whose skip runs fall on the seams of the workgroups and of the 1023s, each there by construction where
    the picture has the blocks for it; block numbers past nb are dropped."""
    every = set(range(nb))
    named = {
        "run_ends_at_wg_last": every - set(range(1000, WG_BLOCKS)),              # blocks 1000 .. 1023 skipped, 1024 coded
        "run_starts_at_wg_first": every - set(range(WG_BLOCKS, WG_BLOCKS + 7)),  # 1023 coded, 1024 .. 1030 skipped
        "run_crosses_seam_cut_at_1023": every - set(range(900, 1200)),           # heads at 900 (count 123) and 1023
        "run_1022_next_in_wg_plus_2": {1023, 2050},                              # head 1024: count 1022, cut at 2046; head 2046 -> 2050
        "nothing_in_next_wg": {500, 2050},                                       # head 501 finds nothing in workgroup 1, is cut at 1023
        "run_reaches_nblocks": {5},
        "nothing": set(),
        "last_block_only": {nb - 1},
        "wg_first_blocks": {0, WG_BLOCKS, 2 * WG_BLOCKS},
    }
    return {k: sorted(b for b in v if b < nb) for k, v in named.items()}


@functools.lru_cache(maxsize=None)
def case(w, h):
    """(pictures, previous as indices or None, the reference's frames) of one size — computed once, never changed."""
    rng = np.random.default_rng(w * 131 + h)
    nb = (w >> 2) * (h >> 2)
    base = er.lossy_picture(rng, w, h)
    pics = [er.exact_picture(rng, w, h), er.lossy_picture(rng, w, h), er.directed_picture(w, h), base]
    prev = [None, 0, None, None]
    for blocks in runs(nb).values():
        pics.append(er.change_blocks(rng, base, w, blocks))
        prev.append(3)
    pics.append(er.change_blocks(rng, base, w, range(nb), dropped_bits_only=True))   # only bits q drops: nothing coded
    prev.append(3)
    for p in pics:
        p.setflags(write=False)
    want = er.encode(pics, [None if j is None else pics[j] for j in prev], w, h)
    names = list(runs(nb))
    if nb > 2050:   # the seams are where they are said to be
        heads = lambda f: [(b, c) for b, c in walk(16, f)[1]]
        assert (1000, 23) in heads(want[4 + names.index("run_ends_at_wg_last")]) and (1023, 1) in heads(want[4 + names.index("run_ends_at_wg_last")])
        assert heads(want[4 + names.index("run_starts_at_wg_first")]) == [(1024, 7)]
        assert heads(want[4 + names.index("run_crosses_seam_cut_at_1023")]) == [(900, 123), (1023, 177)]
        assert heads(want[4 + names.index("run_1022_next_in_wg_plus_2")]) == [(0, 1023), (1024, 1022), (2046, 4), (2051, nb - 2051)]
        assert heads(want[4 + names.index("nothing_in_next_wg")])[1] == (501, 522)
    assert want[-1] == b"".join(skip_word(min(1023, nb - at)) for at in range(0, nb, 1023))
    return pics, prev, want


class Laid:
    """Pictures on the device in one of the LAYOUTS: ptrs[i] and the pitch to hand to the encoder, and the memory they lie in."""

    def __init__(self, pics, w, h, layout):
        t = torch()
        self.w, self.h = w, h
        if layout == "sheet":            # cells of a poisoned sheet, pitch > width and a multiple of 4: 16-byte rows also for an odd width
            self.pitch = ((w + 7) // 4) * 4 + 4
            rowlen, rows = self.pitch, h
        else:
            self.pitch = -w if layout == "negative" else w
            rowlen, rows = w, h
        off = 1 if layout == "off4" else 0     # 4 bytes off: scalar loads
        host = np.full((len(pics), (rows * rowlen + 4 + 3) // 4 * 4), POISON, dtype=np.uint32)   # (every picture's memory 16-byte aligned)
        for i, p in enumerate(pics):
            body = host[i, off:off + rows * rowlen].reshape(rows, rowlen)
            body[:, :w] = p[::-1] if layout == "negative" else p
        self.host = host
        self.mem = t.from_numpy(host.view(np.int32)).cuda()
        assert self.mem.data_ptr() % 16 == 0 and (host.shape[1] * 4) % 16 == 0
        first = (rows - 1) * rowlen if layout == "negative" else 0
        self.ptrs = [self.mem.data_ptr() + 4 * (i * host.shape[1] + off + first) for i in range(len(pics))]
        self.vec = off == 0 and self.pitch % 4 == 0

    def unchanged(self):
        return np.array_equal(self.mem.cpu().numpy().view(np.uint32), self.host)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_bytes_equal_the_reference(size, layout):
    w, h = size
    pics, prev, want = case(w, h)
    laid = Laid(pics, w, h, layout)
    with Msv1Encoder(w, h) as enc:
        assert enc.Bound() == (w >> 2) * (h >> 2) * 18
        got = enc.EncodeFrames(laid.ptrs, [None if j is None else laid.ptrs[j] for j in prev], pitch=laid.pitch)
    for j, (g, x) in enumerate(zip(got, want)):
        assert g == x, f"{w}x{h} {layout}: frame {j} (against {prev[j]}) differs from the reference"
    assert laid.unchanged(), "the pictures, or the memory around them, changed"


def test_both_load_forms_run_and_agree():
    """By construction of Laid: aligned with a width that is a multiple of 4 and the sheet move 16-byte rows, 4 bytes off moves words."""
    w, h = 256, 128
    pics, prev, want = case(w, h)
    forms = {layout: Laid(pics, w, h, layout) for layout in LAYOUTS}
    assert [forms[k].vec for k in LAYOUTS] == [True, False, True, True]
    assert not Laid(case(22, 9)[0][:1], 22, 9, "aligned").vec and Laid(case(22, 9)[0][:1], 22, 9, "sheet").vec
    with Msv1Encoder(w, h) as enc:
        got = {k: enc.EncodeFrames(v.ptrs, [None if j is None else v.ptrs[j] for j in prev], pitch=v.pitch) for k, v in forms.items()}
    assert got["aligned"] == got["off4"] == got["sheet"] == got["negative"] == want


def test_more_pictures_than_a_slice_equal_one_per_call():
    w, h = 22, 9
    rng = np.random.default_rng(77)
    n = 2 * SLICE + 3
    pics = [er.lossy_picture(rng, w, h)]
    for _ in range(n - 1):
        pics.append(er.change_blocks(rng, pics[-1], w, sorted(set(int(b) for b in rng.integers(0, 10, size=3)))))
    prev = [None] + list(range(n - 1))
    prev[SLICE] = None                      # a key frame in the middle, first of the second slice
    want = er.encode(pics, [None if j is None else pics[j] for j in prev], w, h)
    laid = Laid(pics, w, h, "aligned")
    with Msv1Encoder(w, h) as enc:
        together = enc.EncodeFrames(laid.ptrs, [None if j is None else laid.ptrs[j] for j in prev])
        alone = [enc.EncodeFrames([laid.ptrs[i]], [None if prev[i] is None else laid.ptrs[prev[i]]])[0] for i in range(n)]
    assert together == want and alone == want


def raw(enc, n, pics, prevs, pitch, cap, guard=32):
    """The C call into a host array of FILL: (rc, lens, total, the array — `guard` bytes longer than cap)."""
    out = np.full(cap + guard, FILL, dtype=np.uint8)
    lens, total = (C.c_size_t * max(n, 1))(*([777] * max(n, 1))), C.c_size_t(12345)
    pa = (C.c_void_p * max(len(pics), 1))(*pics) if pics is not None else None
    pb = (C.c_void_p * max(len(prevs), 1))(*prevs) if prevs is not None else None
    rc = N.lib().jsp_msv1_encode_frames(enc._h if enc is not None else None, n, pa, pb, pitch, C.c_void_p(out.ctypes.data), cap, lens,
                                        C.byref(total), None)
    return rc, list(lens)[:max(n, 0)], total.value, out


def test_a_short_cap_sets_the_lengths_and_writes_nothing():
    w, h = 22, 9
    pics, prev, want = case(w, h)
    laid = Laid(pics, w, h, "off4")
    prevs = [None if j is None else laid.ptrs[j] for j in prev]
    n, full = len(pics), sum(len(f) for f in want)
    with Msv1Encoder(w, h) as enc:
        rc, lens, total, out = raw(enc, n, laid.ptrs, prevs, w, full - 1)
        assert rc != 0 and N.last_error().startswith("msv1_encode: cap is smaller")
        assert lens == [len(f) for f in want] and total == full and np.all(out == FILL)
        rc, lens, total, out = raw(enc, n, laid.ptrs, prevs, w, 0)
        assert rc != 0 and lens == [len(f) for f in want] and total == full and np.all(out == FILL)
        rc, lens, total, out = raw(enc, n, laid.ptrs, prevs, w, full)
        assert rc == 0 and lens == [len(f) for f in want] and total == full
        assert out[:full].tobytes() == b"".join(want) and np.all(out[full:] == FILL), "written behind the frames"
    assert laid.unchanged()


def test_refusals_come_before_anything_is_queued():
    w, h = 22, 9
    pics, prev, want = case(w, h)
    laid = Laid(pics[:2], w, h, "aligned")
    with Msv1Encoder(w, h) as enc:
        for kw in (dict(enc=None), dict(pics=None), dict(pitch=w - 1), dict(pitch=-(w - 1)), dict(n=0), dict(n=4097), dict(n=-1),
                   dict(pics=[laid.ptrs[0], None])):
            a = dict(enc=enc, n=2, pics=laid.ptrs, prevs=[None, laid.ptrs[0]], pitch=w, cap=2 * enc.Bound())
            a.update(kw)
            rc, lens, total, out = raw(**a)
            assert rc != 0 and N.last_error().startswith("msv1_encode:"), kw
            assert total == 0 and all(v == 0 for v in lens[:2] if 1 <= a["n"] <= 4096) and np.all(out == FILL), kw
        rc, lens, total, out = raw(enc, 2, laid.ptrs, None, w, 2 * enc.Bound())      # previous may be null: key frames
        assert rc == 0 and out[:total].tobytes() == want[0] + er.key(pics[1], w, h)
    with pytest.raises(CodecError, match="^msv1_encode:"):
        Msv1Encoder(3, 8)
    assert laid.unchanged()


def decode_on_device(w, h, frames):
    """The pictures a fresh GPU codec shows after a key frame and the inter frames behind it (covered pixels)."""
    t = torch()
    gpu = MSVideo1_16bit(w, h)
    gpu.Preinit(0)
    pool = [t.full((w * h,), POISON, dtype=t.int32, device="cuda") for _ in range(3)]
    out = []
    for i, data in enumerate(frames):
        dst = next(b for b in pool if b is not gpu.PreviousFrame())
        if i == 0:
            assert gpu.IsKeyFrame(data) and gpu.DecompressI(data, dst) == 0
            shown = dst
        else:
            shown = gpu.DecompressP(data, dst).data_pnt
        out.append(covered(shown.cpu().numpy().view(np.uint32), w, h).copy())
    gpu.StopAndClean()
    return out


def covered(pic, w, h):
    return np.asarray(pic).reshape(h, w)[:(h >> 2) * 4, :(w >> 2) * 4]


def D(w, h, pic):
    """The oracle's decode of the REFERENCE's key frame of a picture."""
    orc = OracleMSVideo1(16, w, h)
    dst = np.zeros(w * h, dtype=np.int32)
    assert orc.DecompressI(er.key(pic, w, h), dst) == 0
    return covered(dst.view(np.uint32), w, h).copy()


@pytest.mark.parametrize("size", [(22, 9), (260, 132)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_round_trip_on_the_device_gives_D_of_every_picture(size):
    w, h = size
    rng = np.random.default_rng(9)
    nb = (w >> 2) * (h >> 2)
    pics = [er.lossy_picture(rng, w, h)]
    pics.append(pics[0].copy())                                                       # a gap that changes nothing
    pics.append(er.change_blocks(rng, pics[1], w, range(0, nb, 3)))
    pics.append(er.exact_picture(rng, w, h))                                          # every block changes
    pics.append(er.change_blocks(rng, pics[3], w, range(nb), dropped_bits_only=True))
    laid = Laid(pics, w, h, "aligned")
    with Msv1Encoder(w, h) as enc:
        frames = enc.EncodeFrames(laid.ptrs, [None] + laid.ptrs[:-1])
    shown = decode_on_device(w, h, frames)
    for i, p in enumerate(pics):
        assert np.array_equal(shown[i], D(w, h, p)), f"picture {i}"
    assert np.array_equal(shown[3], covered(pics[3], w, h) & 0x00F8F8F8)              # an exact picture comes back as it is


def msv1_index(w, h, n, seed=3):
    frames, keys, _ = sg.msv1_clip(seed, w, h, n, p_mix=sg.msv1_p_mix(0.7, 40.0))
    gpu = MSVideo1_16bit(w, h)
    gpu.Preinit(player.INSIGNIFICANT_LINES)
    idx = gpu.BuildIndex(frames, keys)
    return gpu, idx, frames, keys


def shown_pictures(idx, w, h, picks):
    t = torch()
    out = []
    for f in picks:
        dst = t.full((w * h,), POISON, dtype=t.int32, device="cuda")
        idx.Show(f, dst, adopt=False)
        out.append(dst.cpu().numpy().view(np.uint32).reshape(h, w).copy())
    return out


def test_pictures_shown_from_an_msvideo1_index_come_back_as_they_are():
    w, h, n = 64, 48, 12
    gpu, idx, frames, keys = msv1_index(w, h, n)
    picks = [0, 5, 6, 11, 2]
    t = torch()
    bufs = [t.full((w * h,), POISON, dtype=t.int32, device="cuda") for _ in picks]
    for f, b in zip(picks, bufs):
        idx.Show(f, b, adopt=False)
    with Msv1Encoder(w, h) as enc:
        out = enc.EncodeFrames(bufs, [None] + bufs[:-1])
    shown = decode_on_device(w, h, out)
    for i, b in enumerate(bufs):
        assert np.array_equal(shown[i], covered(b.cpu().numpy().view(np.uint32), w, h)), f"frame {picks[i]}"
    idx.close()
    gpu.StopAndClean()


def test_manager_transcode_of_an_msvideo1_index_is_exact():
    w, h, n = 64, 48, 14
    gpu, idx, frames, keys = msv1_index(w, h, n, seed=4)
    vi = VideoInfo(X=w, Y=h, bpp=16, fps=15.0, nframes=n, codec=CODEC_MSVC16, palette=None, riff_size=0)
    t = torch()
    mgr = player.Manager(vi, gpu, lambda k: t.zeros(k, dtype=t.int32, device="cuda"), num_buffers=3)   # runs of 4: keep spans several
    with pytest.raises(ValueError, match="no seek index"):
        mgr.transcode([0])
    mgr.attach_index(idx, first=0)
    keep = [1, 2, 3, 7, 7, 13, 4, 0, 9, 10, 11]
    out, flags = mgr.transcode(keep)
    assert flags == [True] + [False] * (len(keep) - 1) and len(out) == len(keep)
    want = shown_pictures(idx, w, h, keep)
    shown = decode_on_device(w, h, out)
    for i, f in enumerate(keep):
        assert np.array_equal(shown[i], covered(want[i], w, h)), f"entry {i} (frame {f})"
    assert out[4] == skip_word((w >> 2) * (h >> 2))                                   # frame 7 after frame 7: nothing changed
    from jsplayer_amd import avi
    data = mgr.write_transcode(keep[:3])
    info, avi_frames, avi_keys = avi.read_avi_indexed(data)
    assert (info.X, info.Y, info.bpp, info.codec) == (w, h, 16, CODEC_MSVC16) and list(avi_frames) == out[:3]
    assert [bool(k) for k in avi_keys] == [True, False, False]
    with pytest.raises(ValueError, match="not in the attached seek index"):
        mgr.transcode([n])
    with pytest.raises(ValueError, match="keep is empty"):
        mgr.transcode([])
    idx.close()
    gpu.StopAndClean()


def sp_index(w, h, n, bpp=24):
    chunks, keys, frames = sg.sp_clip(11, w, h, n, bpp=bpp, version=4)
    gpu = ScreenPressor(w, h, bpp)
    gpu.Preinit(player.INSIGNIFICANT_LINES)
    idx = gpu.BuildScrubIndex(chunks, keys)
    vi = VideoInfo(X=w, Y=h, bpp=bpp, fps=15.0, nframes=n, codec=CODEC_SCREENPRESSOR, palette=None, riff_size=0)
    t = torch()
    mgr = player.Manager(vi, gpu, lambda k: t.zeros(k, dtype=t.int32, device="cuda"), num_buffers=2)
    mgr.attach_index(idx, first=0)
    return gpu, idx, mgr


def test_manager_transcode_of_a_screenpressor_index_gives_D_of_its_pictures():
    w, h, n = 64, 48, 8
    gpu, idx, mgr = sp_index(w, h, n)
    keep = [0, 1, 2, 3, 6, 5, 4]
    out, flags = mgr.transcode(keep)
    want = shown_pictures(idx, w, h, keep)
    assert out == er.encode(want, [None] + want[:-1], w, h)
    shown = decode_on_device(w, h, out)
    for i, f in enumerate(keep):
        assert np.array_equal(shown[i], D(w, h, want[i])), f"entry {i} (frame {f})"
    idx.close()
    gpu.StopAndClean()


def test_a_16_bpp_screenpressor_index_and_odd_windows_are_refused():
    w, h, n = 64, 48, 3
    gpu, idx, mgr = sp_index(w, h, n, bpp=16)
    with pytest.raises(ValueError, match="16-bpp ScreenPressor"):
        mgr.transcode([0])
    with pytest.raises(ValueError, match="16-bpp ScreenPressor"):
        mgr.proxy([0], 32, 24)
    idx.close()
    gpu.StopAndClean()
    gpu, idx, mgr = sp_index(w, h, n)
    for ww, wh in ((30, 24), (32, 22), (0, 0)):
        with pytest.raises(ValueError, match="multiple of 4"):
            mgr.proxy([0], ww, wh)
    mgr.attach_index(None)
    with pytest.raises(ValueError, match="no seek index"):
        mgr.proxy([0], 32, 24)
    idx.close()
    gpu.StopAndClean()


@pytest.mark.parametrize("codec", ["msvideo1", "screenpressor"])
def test_proxy_decodes_to_D_of_the_presented_windows_upright(codec):
    from jsplayer_amd.codec import DISPLAY_SETPIXELS, PRESENT_AREA, view_matrix
    w, h, n, ww, wh = 64, 48, 8, 32, 24
    if codec == "msvideo1":
        gpu, idx, frames, keys = msv1_index(w, h, n, seed=6)
        vi = VideoInfo(X=w, Y=h, bpp=16, fps=15.0, nframes=n, codec=CODEC_MSVC16, palette=None, riff_size=0)
        t = torch()
        mgr = player.Manager(vi, gpu, lambda k: t.zeros(k, dtype=t.int32, device="cuda"), num_buffers=2)
        mgr.attach_index(idx, first=0)
    else:
        gpu, idx, mgr = sp_index(w, h, n)
    keep = [0, 2, 4, 6, 7, 1, 3]
    out, flags = mgr.proxy(keep, ww, wh)
    k, dx, dy = view_matrix(w, h, ww, wh, 0.0)
    sheet = idx.Present(keep, ww, wh, k, dx, dy, mode=DISPLAY_SETPIXELS, filter=PRESENT_AREA, cols=1).cpu().numpy().view(np.uint32)
    windows = [sheet[i * wh:(i + 1) * wh] for i in range(len(keep))]                  # top row first
    assert all(np.all(win >> 24 == 0xFF) for win in windows)
    bottom_up = [win[::-1] for win in windows]                                        # a frame buffer holds the bottom row first
    assert out == er.encode(bottom_up, [None] + bottom_up[:-1], ww, wh)
    shown = decode_on_device(ww, wh, out)
    for i in range(len(keep)):
        assert np.array_equal(shown[i][::-1], D(ww, wh, bottom_up[i])[::-1]), f"entry {i}"   # flipped back: the window, upright
    idx.close()
    gpu.StopAndClean()


@pytest.mark.parametrize("codec", ["msvideo1", "screenpressor"])
def test_jsp_play_transcode_and_proxy_write_the_managers_clips(tmp_path, codec):
    """examples/jsp_play --transcode / --proxy: the file holds the frames Manager.transcode / proxy give, and for an MSVideo1 clip
    every CRC pair --transcode prints (OUT.avi played back beside the clip's own pictures) is equal."""
    import subprocess
    from jsplayer_amd import avi
    from test_jsp_play_thin_gpu import exe_path
    w, h, n = 64, 48, 14
    if codec == "msvideo1":
        gpu, idx, frames, keys = msv1_index(w, h, n, seed=4)
        vi = VideoInfo(X=w, Y=h, bpp=16, fps=15.0, nframes=n, codec=CODEC_MSVC16, palette=None, riff_size=0)
        fourcc, bpp = b"CRAM", 16
    else:
        frames, keys, _ = sg.sp_clip(11, w, h, n, bpp=24, version=4)
        gpu = ScreenPressor(w, h, 24)
        gpu.Preinit(player.INSIGNIFICANT_LINES)
        idx = gpu.BuildScrubIndex(frames, keys)
        vi = VideoInfo(X=w, Y=h, bpp=24, fps=15.0, nframes=n, codec=CODEC_SCREENPRESSOR, palette=None, riff_size=0)
        fourcc, bpp = b"SCPR", 24
    t = torch()
    mgr = player.Manager(vi, gpu, lambda k: t.zeros(k, dtype=t.int32, device="cuda"))
    mgr.attach_index(idx, first=0)
    path = tmp_path / "clip.avi"
    path.write_bytes(avi.write_avi(w, h, frames, fourcc=fourcc, bpp=bpp, fps=15.0, key_flags=keys))
    keep = list(range(1, n, 1))[:11]                      # 11 frames: the example's runs of 8 carry a picture over
    for extra, (want, flags), size in ((["--transcode", "1:11:1"], mgr.transcode(keep), (w, h)),
                                       (["--proxy", "32x24", "1:11:1"], mgr.proxy(keep, 32, 24), (32, 24))):
        out = tmp_path / (extra[0][2:] + ".avi")
        res = subprocess.run([exe_path(), str(path)] + extra + [str(out)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
        assert res.returncode == 0, res.stderr.decode()
        rows = [l.split() for l in res.stdout.decode().splitlines()]
        assert [int(r[0]) for r in rows] == keep and [int(r[1]) for r in rows] == [len(f) for f in want]
        if codec == "msvideo1" and extra[0] == "--transcode":
            assert all(len(r) == 4 and r[2] == r[3] for r in rows)
        info, got, got_keys = avi.read_avi_indexed(out.read_bytes())
        assert (info.X, info.Y, info.bpp, info.codec) == size + (16, CODEC_MSVC16)
        assert [bytes(f)[:len(x)] for f, x in zip(got, want)] == want and [bool(k) for k in got_keys] == flags
    idx.close()
    gpu.StopAndClean()
