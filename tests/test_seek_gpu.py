"""jsp_seek / Seek / Manager.seek on an MI355X against the oracle.

Truth: OracleMSVideo1 driven frame by frame where, before each frame of the sought range, its destination is np.copyto'd
with the picture before it — the contract's equivalence (include/jsplayer_amd.h, jsp_seek).  For well-formed clips that is a
plain oracle run."""
import os
import subprocess

import numpy as np
import pytest

from jsplayer_amd import CodecError, MSVideo1_16bit, MSVideo1_8bit, ScreenPressor, player
from jsplayer_amd import streamgen as sg
from oracle_binding import OracleAbort, OracleMSVideo1, OracleScreenPressor

pytestmark = pytest.mark.gpu

POISON = 0x5A5A5A5A
PARSE = "host"


@pytest.fixture(autouse=True, params=["host", "gpu"])
def parse_mode(request):
    """Every test runs with the block tables of the host parser and of the on-GPU parse."""
    global PARSE
    PARSE = request.param
    yield request.param
    PARSE = "host"


def dev_buf(n, fill=POISON, misalign=False):
    import torch
    if misalign:
        return torch.full((n + 4,), fill, dtype=torch.int32, device="cuda")[1:1 + n]
    return torch.full((n,), fill, dtype=torch.int32, device="cuda")


def make_gpu(bits, w, h, pal=None, lines=36):
    c = MSVideo1_16bit(w, h) if bits == 16 else MSVideo1_8bit(w, h, pal or b"")
    c.set_option("msv1_parse", PARSE)
    c.Preinit(lines)
    return c


class Truth:
    """The oracle, frame by frame; `inplace` frames start from a copy of the picture before them."""

    def __init__(self, bits, w, h, pal, lines=36):
        self.o = OracleMSVideo1(bits, w, h, pal)
        self.o.Preinit(lines)
        self.n = w * h
        self.bufs = [np.full(self.n, POISON, dtype=np.int32) for _ in range(3)]

    def picture(self):
        p = self.o.PreviousFrame()
        return None if p is None else p.copy()

    def step(self, src, key, inplace=False):
        """(adopted, significant) of one frame."""
        prev = self.o.PreviousFrame()
        dst = next(b for b in self.bufs if b is not prev)
        if inplace:
            if prev is not None:
                np.copyto(dst, prev)
            else:
                dst.fill(POISON)
        if key:
            rc = self.o.DecompressI(src, dst)
            if rc != 0:
                raise OracleAbort()
            return self.o.PreviousFrame() is dst, False
        data, sig = self.o.DecompressP(src, dst)
        return data is dst, sig


def gpu_sequential(gpu, frames, keys, upto, w, h):
    """Frames [0, upto) through DecompressI / DecompressP into a small pool; returns the pool."""
    pool = [dev_buf(w * h) for _ in range(3)]
    for i in range(upto):
        dst = next(b for b in pool if b is not gpu.PreviousFrame())
        if keys[i]:
            assert gpu.DecompressI(frames[i], dst) == 0
        else:
            gpu.DecompressP(frames[i], dst)
    return pool


def check_seek(bits, w, h, pal, frames, keys, start, target, lines=36, misalign=False, continue_frames=0, chunk=None):
    """Frames [0, start) sequentially on both sides, then seek over [start, target], then `continue_frames` more."""
    truth = Truth(bits, w, h, pal, lines)
    for i in range(start):
        truth.step(frames[i], keys[i])
    before = truth.picture()
    adopted, sig = False, False
    for i in range(start, target + 1):
        a, sig = truth.step(frames[i], keys[i], inplace=True)
        adopted |= a
    gpu = make_gpu(bits, w, h, pal, lines)
    if chunk:
        gpu.set_option("msv1_seek_chunk_frames", str(chunk))
    pool = gpu_sequential(gpu, frames, keys, start, w, h)
    old_prev = gpu.PreviousFrame()
    dst = dev_buf(w * h, misalign=misalign)
    res = gpu.Seek(frames[start:target + 1], dst, keys[start:target + 1])
    got = dst.cpu().numpy()
    where = f"{bits}-bit {w}x{h} seek {start}..{target} ({PARSE} parse)"
    if adopted:
        assert res.data_pnt is dst and gpu.PreviousFrame() is dst, where
        assert np.array_equal(got, truth.picture()), where
    else:
        assert res.data_pnt is old_prev and gpu.PreviousFrame() is old_prev, where
        assert np.all(got == POISON), where + ": dst touched"
        if before is not None:
            assert np.array_equal(old_prev.cpu().numpy(), before), where
    assert res.significant_changes == (False if keys[target] else sig), where
    if continue_frames:
        # the next frames through a pool, exactly as after a sequential decode (block_changes, previous frame)
        cx, cy = (w // 4) * 4, (h // 4) * 4
        pool = [p for p in pool if p is not gpu.PreviousFrame()] + [dst]
        for i in range(target + 1, min(target + 1 + continue_frames, len(frames))):
            prev = gpu.PreviousFrame()
            gdst = next(b for b in pool if b is not prev)
            a, s = truth.step(frames[i], keys[i])
            if keys[i]:
                assert gpu.DecompressI(frames[i], gdst) == 0
            else:
                r = gpu.DecompressP(frames[i], gdst)
                assert r.significant_changes == s, f"{where}: frame {i} significance"
                assert (r.data_pnt is gdst) == a, f"{where}: frame {i} adoption"
            pic = gpu.PreviousFrame().cpu().numpy().reshape(h, w)[:cy, :cx]
            assert np.array_equal(pic, truth.picture().reshape(h, w)[:cy, :cx]), f"{where}: frame {i} after the seek"
    gpu.StopAndClean()
    return res


def clip(bits, w, h, n=20, cfg=0):
    return sg.msv1_clip(900 + cfg + bits, w, h, n, bits=bits, p_mix=sg.msv1_p_mix(0.7, 6.0), key_every=5)


@pytest.mark.parametrize("bits", [16, 8])
@pytest.mark.parametrize("size", [(4, 4), (37, 23), (100, 52), (320, 240), (1920, 1080)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_seek_from_nearest_key_frame(bits, size):
    w, h = size
    n = 20
    frames, keys, pal = clip(bits, w, h, n)
    for target in (0, 1, 8, n - 1, 5, 6):
        start = player.nearest_key_frame(keys, target)
        check_seek(bits, w, h, pal, frames, keys, start, target, continue_frames=8 if w <= 320 else 2)


@pytest.mark.parametrize("bits", [16, 8])
def test_forward_seek_inside_an_interval(bits):
    w, h = 37, 23
    frames, keys, pal = clip(bits, w, h, 20, cfg=1)
    check_seek(bits, w, h, pal, frames, keys, 7, 9, continue_frames=8)
    check_seek(bits, w, h, pal, frames, keys, 11, 14, continue_frames=4)
    w, h = 320, 240
    frames, keys, pal = clip(bits, w, h, 20, cfg=2)
    check_seek(bits, w, h, pal, frames, keys, 2, 4, continue_frames=8)


@pytest.mark.parametrize("bits", [16, 8])
def test_all_skip_range_leaves_dst_alone(bits):
    w, h = 64, 32
    frames, _, pal = sg.msv1_clip(81, w, h, 1, bits=bits)
    short = bytes([0x10, 0x84])                    # (16-bit: shorter than size_of_just_skips, the early-out)
    allskip = bytes([0x10, 0x84] * 8)              # 128 blocks, all skipped: nothing adopted
    res = check_seek(bits, w, h, pal, [frames[0], short, allskip, allskip], [True, False, False, False], 1, 3)
    assert res.significant_changes is False


@pytest.mark.parametrize("bits", [16, 8])
def test_damaged_streams_in_the_range(bits):
    w, h = 32, 16
    frames, keys, pal = sg.msv1_clip(70 + bits, w, h, 2, bits=bits, p_mix=sg.msv1_p_mix(0.4, 5.0))
    rng = np.random.default_rng(11)
    full = frames[1]
    srcs, ks = [frames[0]], [True]
    for cut in [0, 1, 2, 3, 5, 8, 13, 21, len(full) // 2, len(full) - 1]:
        srcs.append(full[:cut])
        ks.append(False)
    for _ in range(6):
        srcs.append(rng.integers(0, 256, size=int(rng.integers(1, 200)), dtype=np.uint8).tobytes())
        ks.append(False)
    if bits == 8:
        srcs.append(full[:20] + b"\x00\x00" + full[22:])      # end marker mid-frame
    else:
        srcs.append(bytes([0x1F, 0x80, 0x00, 0x84] + [0] * 20))   # negative skip
    ks.append(False)
    srcs.append(full + b"\x07")                                # odd trailing byte
    ks.append(False)
    for target in range(1, len(srcs)):
        check_seek(bits, w, h, pal, srcs, ks, 0, target, lines=4)
        check_seek(bits, w, h, pal, srcs, ks, max(1, target - 3), target, lines=4)


def test_skip_with_no_previous_picture_raises():
    w, h = 16, 8
    bad = bytes([0x00, 0xFC, 0x01, 0x84] + [0] * 8)
    frames, _, _ = sg.msv1_clip(83, w, h, 1)
    gpu = make_gpu(16, w, h, lines=0)
    dst = dev_buf(w * h)
    with pytest.raises(CodecError, match="frame 0"):
        gpu.Seek([bad, frames[0]], dst, [False, True])
    assert gpu.PreviousFrame() is None
    other = dev_buf(w * h)
    assert gpu.DecompressI(frames[0], other) == 0
    orc = OracleMSVideo1(16, w, h)
    orc.Preinit(0)
    ref = np.zeros(w * h, dtype=np.int32)
    assert orc.DecompressI(frames[0], ref) == 0
    assert np.array_equal(other.cpu().numpy(), ref)
    assert gpu.PreviousFrame() is other


def test_chunks_give_the_one_chunk_result():
    w, h = 320, 240
    frames, keys, pal = sg.msv1_clip(91, w, h, 14, p_mix=sg.msv1_p_mix(0.7, 6.0))
    for chunk in (1, 3, 4):
        for target in (6, 9, 13):   # 7 frames in chunks of 3: the last frame opens its chunk
            a = check_seek(16, w, h, None, frames, keys, 0, target, chunk=chunk, continue_frames=0)
            b = check_seek(16, w, h, None, frames, keys, 0, target)
            assert a.significant_changes == b.significant_changes
    # and one from inside the clip, with the compare of the last frame depending on the chunk before
    check_seek(16, w, h, None, frames, keys, 4, 10, chunk=3, continue_frames=3)


def test_full_size_inter70_seek_to_the_last_frame():
    import torch
    from jsplayer_amd import workloads as wl
    name = "msvideo1_16_1080p_inter70"
    c = wl.build_clips(name)[0]
    gpu = wl.make_codec(name, options={"msv1_parse": PARSE})
    pool = [dev_buf(wl.W * wl.H) for _ in range(3)]
    for i, f in enumerate(c.frames):
        dst = next(b for b in pool if b is not gpu.PreviousFrame())
        if c.keys[i]:
            assert gpu.DecompressI(f, dst) == 0
        else:
            gpu.DecompressP(f, dst)
    want = wl.digest(gpu.PreviousFrame().cpu().numpy())
    gpu.StopAndClean()
    seeker = wl.make_codec(name, options={"msv1_parse": PARSE})
    dst = dev_buf(wl.W * wl.H)
    res = seeker.Seek(c.frames, dst, c.keys)
    torch.cuda.synchronize()
    assert res.data_pnt is dst
    assert wl.digest(dst.cpu().numpy()) == want
    seeker.StopAndClean()


@pytest.mark.parametrize("bits", [16, 8])
def test_dst_not_16_byte_aligned(bits):
    for (w, h) in [(64, 48), (320, 240)]:
        frames, keys, pal = clip(bits, w, h, 12, cfg=3)
        for target in (3, 7, 11):
            check_seek(bits, w, h, pal, frames, keys, player.nearest_key_frame(keys, target), target, misalign=True, continue_frames=3)


def test_refusals_change_nothing():
    w, h = 64, 48
    chunks, keys, _ = sg.sp_clip(3, w, h, 6, version=4)
    sp, so = ScreenPressor(w, h, 24), OracleScreenPressor(w, h, 24)
    sp.Preinit(36)
    so.Preinit(36)
    bufs = [dev_buf(w * h, 0) for _ in range(3)]
    obufs = [np.zeros(w * h, dtype=np.int32) for _ in range(3)]
    for i, (src, key) in enumerate(zip(chunks, keys)):
        if i == 3:
            before = sp.PreviousFrame()
            with pytest.raises(CodecError, match="MSVideo1 only"):
                sp.Seek(chunks[:4], next(b for b in bufs if b is not before), keys[:4])
            assert sp.PreviousFrame() is before
        k = next(j for j in range(3) if bufs[j] is not sp.PreviousFrame())
        if key:
            assert sp.DecompressI(src, bufs[k]) == 0 and so.DecompressI(src, obufs[k]) == 0
        else:
            sp.DecompressP(src, bufs[k])
            so.DecompressP(src, obufs[k])
        assert np.array_equal(sp.PreviousFrame().cpu().numpy(), so.PreviousFrame()), f"ScreenPressor frame {i}"
    sp.StopAndClean()
    # MSVideo1: an asynchronous frame in flight, a host buffer, the current previous frame
    frames, keys, _ = clip(16, 64, 48, 6, cfg=4)
    gpu = make_gpu(16, 64, 48)
    a, b, c = dev_buf(64 * 48), dev_buf(64 * 48), dev_buf(64 * 48)
    assert gpu.DecompressI(frames[0], a) == 0
    t = gpu.DecompressP_async(frames[1], b)
    with pytest.raises(CodecError, match="in flight"):
        gpu.Seek(frames[:3], c, keys[:3])
    gpu.wait(t)
    prev = gpu.PreviousFrame()
    with pytest.raises(CodecError, match="previous frame"):
        gpu.Seek(frames[:3], prev, keys[:3])
    with pytest.raises(CodecError, match="device"):
        gpu.Seek(frames[:3], np.zeros(64 * 48, dtype=np.int32), keys[:3])
    assert gpu.PreviousFrame() is prev
    assert np.all(c.cpu().numpy() == POISON)
    gpu.StopAndClean()


class _Res:
    def __init__(self, data, sig):
        self.data_pnt, self.significant_changes = data, sig


class _Orc:
    def __init__(self, o):
        self.o = o

    def __getattr__(self, k):
        return getattr(self.o, k)

    def DecompressP(self, src, dst):
        return _Res(*self.o.DecompressP(src, dst))


@pytest.mark.parametrize("bits", [16, 8])
def test_manager_seek_against_the_reference_way(bits):
    import torch
    from jsplayer_amd.avi import CODEC_MSVC16, CODEC_MSVC8, VideoInfo
    w, h, n = 320, 240, 30
    frames, keys, pal = sg.msv1_clip(95 + bits, w, h, n, bits=bits, p_mix=sg.msv1_p_mix(0.7, 6.0), key_every=10)
    vi = VideoInfo(X=w, Y=h, bpp=bits, fps=15.0, nframes=n, codec=CODEC_MSVC16 if bits == 16 else CODEC_MSVC8, palette=pal, riff_size=0)
    cpu = player.Manager(vi, _Orc(OracleMSVideo1(bits, w, h, pal)), lambda k: np.zeros(k, dtype=np.int32))
    dec = MSVideo1_16bit(w, h) if bits == 16 else MSVideo1_8bit(w, h, pal)
    dec.set_option("msv1_parse", PARSE)
    gpu = player.Manager(vi, dec, lambda k: torch.zeros(k, dtype=torch.int32, device="cuda"))
    def show(mgr, i):   # what a player does for frame i: worker() when it is the next frame to decode, else the seek branch
        d = mgr.worker(frames[i], i, None, keys[i]) if mgr.next_frame_to_decode == i else mgr.seek(frames, i, keys)
        return mgr.buffers[d.buffer_index]

    for target in (17, 3, 12, 13, 25, 0, 9, 29, 15, 14):   # backwards, forwards inside an interval, held frames
        dc, dg = cpu.seek(frames, target, keys), gpu.seek(frames, target, keys)
        assert np.array_equal(gpu.buffers[dg.buffer_index].cpu().numpy(), cpu.buffers[dc.buffer_index]), f"seek to {target}"
        for i in range(target + 1, min(target + 4, n)):
            assert np.array_equal(show(gpu, i).cpu().numpy(), show(cpu, i)), f"frame {i} after the seek to {target}"
    dec.StopAndClean()


def test_jsp_play_seek_matches_the_plain_run(tmp_path):
    from jsplayer_amd import avi
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "examples", "jsp_play")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-s", "-C", os.path.join(root, "examples")])
    frames, keys, _ = sg.msv1_clip(97, 320, 240, 40, p_mix=sg.msv1_p_mix(0.7, 6.0), key_every=16)
    path = tmp_path / "clip.avi"
    path.write_bytes(avi.write_avi(320, 240, frames, fourcc=b"CRAM", bpp=16, fps=15.0, key_flags=keys))

    def lines(extra):
        res = subprocess.run([exe, str(path)] + extra, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
        assert res.returncode == 0, res.stderr.decode()
        return [(l.split()[0], l.split()[1], l.split()[-1]) for l in res.stdout.decode().splitlines() if l and l[0].isdigit()]

    plain = lines([])
    assert len(plain) == 40
    for n in (0, 7, 16, 23, 39):
        got = lines(["--seek", str(n)])
        assert got == plain[n:], f"--seek {n}"
