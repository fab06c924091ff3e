"""Seek index (jsp_index_* / BuildIndex / SeekIndex.Show / Manager.attach_index) on an MI355X.

Truth: a twin codec brought to the build-time state (same prefix, decoded frame by frame) running Seek(frames[0..t]) — the index's
contract (include/jsplayer_amd.h, jsp_index_show) — and, for the Manager and the full-size clip, the oracle."""
import os
import subprocess

import numpy as np
import pytest

from jsplayer_amd import CodecError, MSVideo1_16bit, MSVideo1_8bit, ScreenPressor, player
from jsplayer_amd import streamgen as sg
from oracle_binding import OracleMSVideo1

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


def dev_buf(n, fill=POISON):
    import torch
    return torch.full((n,), fill, dtype=torch.int32, device="cuda")


def make_gpu(bits, w, h, pal=None, lines=36, chunk=None):
    c = MSVideo1_16bit(w, h) if bits == 16 else MSVideo1_8bit(w, h, pal or b"")
    c.set_option("msv1_parse", PARSE)
    if chunk:
        c.set_option("msv1_seek_chunk_frames", str(chunk))
    c.Preinit(lines)
    return c


def sequential(gpu, frames, keys, lo, hi, pool):
    """Frames [lo, hi) through DecompressI / DecompressP into `pool`; [(adopted, significance)] of each."""
    out = []
    for i in range(lo, hi):
        prev = gpu.PreviousFrame()
        dst = next(b for b in pool if b is not prev)
        if keys[i]:
            assert gpu.DecompressI(frames[i], dst) == 0
            out.append((gpu.PreviousFrame() is dst, None))
        else:
            r = gpu.DecompressP(frames[i], dst)
            out.append((r.data_pnt is dst, r.significant_changes))
    return out


def mixed_clip(bits, w, h, seed=0):
    """A key frame, inter frames with skips, all-skip frames, early-outs, an 8-bit end marker, a truncated frame, key frames
    mid-range."""
    frames, keys, pal = sg.msv1_clip(600 + seed + bits, w, h, 14, bits=bits, p_mix=sg.msv1_p_mix(0.6, 5.0), key_every=6)
    nb = (w // 4) * (h // 4)
    allskip = b"".join(bytes([min(nb - k, 255), 0x84]) for k in range(0, nb, 255))
    out, ks = list(frames[:4]), list(keys[:4])
    out += [allskip, bytes([0x10, 0x84]), frames[4]]                 # all-skip; 16-bit early-out (short); a real frame
    ks += [False, False, keys[4]]
    full = frames[5] if not keys[5] else frames[4]
    out.append(full[: max(2, len(full) // 2)])                          # truncated
    ks.append(False)
    if bits == 8:
        out.append(full[:10] + b"\x00\x00" + full[12:])                 # end marker part-way
    else:
        out.append(full + b"\x07")                                      # odd trailing byte
    ks.append(False)
    out += list(frames[5:])
    ks += list(keys[5:])
    out.append(allskip)
    ks.append(False)
    return out, ks, pal


class Twin:
    """A codec brought to the build-time state: `start` frames decoded one by one."""

    def __init__(self, bits, w, h, pal, frames, keys, start, lines=36, chunk=None):
        self.args = (bits, w, h, pal, lines, chunk)
        self.frames, self.keys, self.start, self.w, self.h = frames, keys, start, w, h

    def make(self):
        bits, w, h, pal, lines, chunk = self.args
        g = make_gpu(bits, w, h, pal, lines, chunk)
        pool = [dev_buf(w * h) for _ in range(3)]
        sequential(g, self.frames, self.keys, 0, self.start, pool)
        return g, pool

    def seek(self, t):
        """(picture, data_pnt is dst, data_pnt is the old previous frame, significance) of Seek(range[0..t]) on a fresh twin."""
        g, pool = self.make()
        old = g.PreviousFrame()
        dst = dev_buf(self.w * self.h)
        s = self.start
        r = g.Seek(self.frames[s:s + t + 1], dst, self.keys[s:s + t + 1])
        out = (dst.cpu().numpy(), r.data_pnt is dst, old is not None and r.data_pnt is old, r.significant_changes)
        g.StopAndClean()
        return out


def show(idx, t, w, h, adopt=False):
    dst = dev_buf(w * h)
    old = idx._codec.PreviousFrame()
    r = idx.Show(t, dst, adopt=adopt)
    return dst.cpu().numpy(), r.data_pnt is dst, old is not None and r.data_pnt is old, r.significant_changes


def where(bits, w, h, t):
    return f"{bits}-bit {w}x{h} t={t} ({PARSE} parse)"


@pytest.mark.parametrize("bits", [16, 8])
@pytest.mark.parametrize("size", [(4, 4), (13, 9), (64, 48), (256, 144)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_every_t_matches_the_twin_seek(bits, size):
    w, h = size
    frames, keys, pal = mixed_clip(bits, w, h)
    for start in (0, 3):   # from no picture at all, and from inside the clip (the index starts at an inter frame)
        twin = Twin(bits, w, h, pal, frames, keys, start)
        a, _ = twin.make()
        with a.BuildIndex(frames[start:], keys[start:]) as idx:
            assert idx.frames == len(frames) - start and idx.device_bytes > 0
            for t in range(idx.frames):
                got, want = show(idx, t, w, h), twin.seek(t)
                assert np.array_equal(got[0], want[0]), where(bits, w, h, t) + f" start={start}"
                assert got[1:] == want[1:], where(bits, w, h, t) + f" start={start}"
        a.StopAndClean()


@pytest.mark.parametrize("bits", [16, 8])
def test_order_independence_and_no_trace_without_adopt(bits):
    w, h = 64, 48
    frames, keys, pal = mixed_clip(bits, w, h, seed=1)
    start = 2
    twin = Twin(bits, w, h, pal, frames, keys, start)
    a, pool = twin.make()
    idx = a.BuildIndex(frames[start:], keys[start:])
    n = idx.frames
    first = {t: show(idx, t, w, h) for t in range(n)}
    rng = np.random.default_rng(5)
    for t in list(range(n - 1, -1, -1)) + [int(x) for x in rng.permutation(n)]:
        got = show(idx, t, w, h)
        assert np.array_equal(got[0], first[t][0]) and got[1:] == first[t][1:], where(bits, w, h, t)
    # the codec is as it was: the next frames decode exactly as on the twin that saw no show
    b, bpool = twin.make()
    assert sequential(a, frames, keys, start, len(frames), pool) == sequential(b, frames, keys, start, len(frames), bpool)
    cx, cy = (w // 4) * 4, (h // 4) * 4
    pa, pb = a.PreviousFrame().cpu().numpy().reshape(h, w), b.PreviousFrame().cpu().numpy().reshape(h, w)
    assert np.array_equal(pa[:cy, :cx], pb[:cy, :cx])
    idx.close()
    a.StopAndClean()
    b.StopAndClean()


@pytest.mark.parametrize("bits", [16, 8])
def test_adopt_then_play_on(bits):
    w, h = 64, 48
    frames, keys, pal = mixed_clip(bits, w, h, seed=2)
    n = len(frames)
    # right after the truncated frame (7) and the frame after it, after an all-skip (4) and an early-out (5), a key frame, the end
    cx, cy = (w // 4) * 4, (h // 4) * 4
    for t in (0, 4, 5, 7, 8, 10, n - 2):
        twin = Twin(bits, w, h, pal, frames, keys, 0)
        a, apool = twin.make()
        idx = a.BuildIndex(frames, keys)
        dst = dev_buf(w * h)
        r = idx.Show(t, dst, adopt=True)
        b, bpool = twin.make()
        bdst = dev_buf(w * h)
        rb = b.Seek(frames[:t + 1], bdst, keys[:t + 1])
        assert (r.data_pnt is dst) == (rb.data_pnt is bdst) and r.significant_changes == rb.significant_changes
        assert (a.PreviousFrame() is dst) == (b.PreviousFrame() is bdst)
        apool, bpool = apool + [dst], bpool + [bdst]
        for i in range(t + 1, n):
            ra, rb2 = sequential(a, frames, keys, i, i + 1, apool), sequential(b, frames, keys, i, i + 1, bpool)
            assert ra == rb2, where(bits, w, h, t) + f": frame {i}"
            if a.PreviousFrame() is not None:
                pa = a.PreviousFrame().cpu().numpy().reshape(h, w)[:cy, :cx]
                pb = b.PreviousFrame().cpu().numpy().reshape(h, w)[:cy, :cx]
                assert np.array_equal(pa, pb), where(bits, w, h, t) + f": frame {i}"
        idx.close()
        a.StopAndClean()
        b.StopAndClean()


@pytest.mark.parametrize("chunk", [1, 3, 7])
def test_chunks_give_the_one_chunk_result(chunk):
    for bits in (16, 8):
        w, h = 64, 48
        frames, keys, pal = mixed_clip(bits, w, h, seed=3)
        one = make_gpu(bits, w, h, pal)
        split = make_gpu(bits, w, h, pal, chunk=chunk)
        i1, i2 = one.BuildIndex(frames, keys), split.BuildIndex(frames, keys)
        assert i1.significance == i2.significance
        for t in range(i1.frames):
            g1, g2 = show(i1, t, w, h), show(i2, t, w, h)
            assert np.array_equal(g1[0], g2[0]) and g1[1:] == g2[1:], f"{bits}-bit chunk {chunk} t={t}"
        i1.close()
        i2.close()
        one.StopAndClean()
        split.StopAndClean()


@pytest.mark.parametrize("bits", [16, 8])
def test_significance_is_what_the_worker_records_and_find_change_judges(bits):
    from jsplayer_amd.avi import CODEC_MSVC16, CODEC_MSVC8, VideoInfo
    w, h = 64, 48
    frames, keys, pal = sg.msv1_clip(640 + bits, w, h, 30, bits=bits, p_mix=sg.msv1_p_mix(0.5, 4.0), key_every=7)
    vi = VideoInfo(X=w, Y=h, bpp=bits, fps=15.0, nframes=len(frames), codec=CODEC_MSVC16 if bits == 16 else CODEC_MSVC8,
                   palette=pal, riff_size=0)
    dec = make_gpu(bits, w, h, pal)
    mgr = player.Manager(vi, dec, lambda n: dev_buf(n))
    log = mgr.play(frames, key_flags=keys)
    fresh = make_gpu(bits, w, h, pal, lines=player.INSIGNIFICANT_LINES)
    idx = fresh.BuildIndex(frames, keys)
    assert idx.significance == [bool(d.significant_changes) for d in log]
    res = fresh.FindChange(frames, dev_buf(w * h), keys, first=1)
    judged = [(j, s) for j, s in enumerate(res.significance) if s is not None]
    assert judged and all(s == idx.significance[j] for j, s in judged)
    idx.close()
    dec.StopAndClean()
    fresh.StopAndClean()


def test_range_starting_at_an_inter_frame_owns_its_picture_before():
    w, h = 64, 48
    frames, keys, _ = sg.msv1_clip(650, w, h, 12, p_mix=sg.msv1_p_mix(0.7, 5.0), key_every=12)
    twin = Twin(16, w, h, None, frames, keys, 4)
    a, pool = twin.make()
    old = a.PreviousFrame()
    idx = a.BuildIndex(frames[4:], keys[4:])
    import torch
    for b in pool:
        b.fill_(0x1234567)   # the caller reuses every buffer, the old previous frame among them
    torch.cuda.synchronize()
    for t in range(idx.frames):
        got, want = show(idx, t, w, h), twin.seek(t)
        assert np.array_equal(got[0], want[0]), f"t={t}"
    assert old is a.PreviousFrame()
    idx.close()
    a.StopAndClean()


def test_refusals_change_nothing():
    w, h = 64, 48
    frames, keys, _ = sg.msv1_clip(660, w, h, 8, p_mix=sg.msv1_p_mix(0.7, 5.0), key_every=8)
    sp = ScreenPressor(w, h, 24)
    with pytest.raises(CodecError, match="MSVideo1 only"):
        sp.BuildIndex(frames, keys)
    sp.StopAndClean()
    a = make_gpu(16, w, h)
    pool = [dev_buf(w * h) for _ in range(3)]
    sequential(a, frames, keys, 0, 2, pool)
    prev = a.PreviousFrame()
    prev_pic = prev.cpu().numpy().copy()
    idx = a.BuildIndex(frames[2:], keys[2:])
    assert a.PreviousFrame() is prev
    dst = dev_buf(w * h)
    for bad in (-1, idx.frames):
        with pytest.raises(CodecError, match="outside"):
            idx.Show(bad, dst)
    with pytest.raises(CodecError, match="device"):
        idx.Show(0, np.zeros(w * h, dtype=np.int32))
    with pytest.raises(CodecError, match="previous frame"):
        idx.Show(0, prev)
    ticket = a.DecompressP_async(frames[2], pool[2] if pool[2] is not prev else pool[1])
    with pytest.raises(CodecError, match="in flight"):
        idx.Show(1, dst)
    with pytest.raises(CodecError, match="in flight"):
        a.BuildIndex(frames[3:], keys[3:])
    a.wait(ticket)
    other = make_gpu(16, w, h)
    foreign = other.BuildIndex(frames, keys)
    foreign._codec = a            # (the index of one codec handed to another)
    with pytest.raises(CodecError, match="another codec"):
        foreign.Show(0, dst)
    foreign._codec = other
    foreign.close()
    assert np.all(dst.cpu().numpy() == POISON)
    # a range with a frame the reference raises on (a skip with no previous picture): the error names it, nothing changes
    bad = bytes([0x00, 0xFC, 0x01, 0x84] + [0] * 8)
    fresh = make_gpu(16, w, h)
    with pytest.raises(CodecError, match="frame 0"):
        fresh.BuildIndex([bad] + frames[1:3], [False, False, False])
    assert fresh.PreviousFrame() is None
    ok = dev_buf(w * h)
    assert fresh.DecompressI(frames[0], ok) == 0 and fresh.PreviousFrame() is ok
    # destroyed after its codec
    late = fresh.BuildIndex(frames[1:], keys[1:])
    fresh.StopAndClean()
    late.close()
    other.StopAndClean()
    idx.close()
    a.StopAndClean()
    assert np.array_equal(prev_pic, prev.cpu().numpy())


def test_full_size_inter70():
    import torch
    from jsplayer_amd import workloads as wl
    name = "msvideo1_16_1080p_inter70"
    c = wl.build_clips(name)[0]
    golden = wl.golden_digests(name, 0)
    if golden is None:
        pytest.fail("tests/golden/bench_digests.json has no digests for " + name)
    want = golden[0]
    assert len(want) == len(c.frames) == 512
    codec = wl.make_codec(name, options={"msv1_parse": PARSE})
    idx = codec.BuildIndex(c.frames, c.keys)
    bufs = [dev_buf(wl.W * wl.H) for _ in range(2)]
    rng = np.random.default_rng(7)
    for k, t in enumerate([0, 1, 255, 511] + [int(x) for x in rng.integers(0, 512, size=32)]):
        r = idx.Show(t, bufs[k & 1], adopt=False)
        assert r.data_pnt is bufs[k & 1]
        assert wl.digest(bufs[k & 1].cpu().numpy()) == want[t], f"frame {t}"
    for t in range(511, -1, -1):   # the full step back, adopting as the Manager does
        dst = bufs[t & 1]
        idx.Show(t, dst, adopt=True)
        torch.cuda.synchronize()
        assert wl.digest(dst.cpu().numpy()) == want[t], f"step back: frame {t}"
    idx.close()
    codec.StopAndClean()


class _Spy:
    """A decoder that forwards everything and logs the decoding calls."""

    def __init__(self, d):
        self.d, self.calls = d, []

    def __getattr__(self, k):
        v = getattr(self.d, k)
        if k in ("Seek", "FindChange", "DecompressI", "DecompressP", "BuildIndex"):
            def logged(*a, **kw):
                self.calls.append(k)
                return v(*a, **kw)
            return logged
        return v


@pytest.mark.parametrize("bits", [16, 8])
def test_manager_step_back_and_skip_stills_inside_the_index(bits):
    from jsplayer_amd.avi import CODEC_MSVC16, CODEC_MSVC8, VideoInfo
    w, h = 64, 48
    frames, keys, pal = sg.msv1_clip(670 + bits, w, h, 30, bits=bits, p_mix=sg.msv1_p_mix(0.4, 4.0), key_every=10)
    o = OracleMSVideo1(bits, w, h, pal)
    o.Preinit(player.INSIGNIFICANT_LINES)
    pics, buf = [], [np.zeros(w * h, dtype=np.int32) for _ in range(3)]
    for i, f in enumerate(frames):
        dst = next(b for b in buf if b is not o.PreviousFrame())
        if keys[i]:
            o.DecompressI(f, dst)
        else:
            o.DecompressP(f, dst)
        pics.append(o.PreviousFrame().copy())
    vi = VideoInfo(X=w, Y=h, bpp=bits, fps=15.0, nframes=len(frames), codec=CODEC_MSVC16 if bits == 16 else CODEC_MSVC8,
                   palette=pal, riff_size=0)
    dec = make_gpu(bits, w, h, pal)
    spy = _Spy(dec)
    mgr = player.Manager(vi, spy, lambda n: dev_buf(n))
    idx = dec.BuildIndex(frames, keys)
    mgr.attach_index(idx, 0)
    d = mgr.seek(frames, len(frames) - 1, keys)
    assert np.array_equal(mgr.buffers[d.buffer_index].cpu().numpy(), pics[-1])
    for t in range(len(frames) - 2, -1, -1):
        d = mgr.prev_frame(frames, keys)
        assert d.index == t and np.array_equal(mgr.buffers[d.buffer_index].cpu().numpy(), pics[t]), f"frame {t}"
    while d.index < len(frames) - 1:
        d = mgr.skip_stills(frames, keys)
        assert np.array_equal(mgr.buffers[d.buffer_index].cpu().numpy(), pics[d.index]), f"skip to {d.index}"
    assert spy.calls == [], spy.calls
    # and the play goes on from the frame shown as after a sequential decode
    mgr.seek(frames, 12, keys)
    for i in range(13, 16):
        d = mgr.worker(frames[i], i, None, keys[i])
        assert np.array_equal(mgr.buffers[d.buffer_index].cpu().numpy(), pics[i]), f"frame {i} after the show"
    idx.close()
    dec.StopAndClean()


def test_jsp_play_step_back_matches_the_plain_run(tmp_path):
    from jsplayer_amd import avi
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "examples", "jsp_play")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-s", "-C", os.path.join(root, "examples")])
    frames, keys, _ = sg.msv1_clip(97, 320, 240, 40, p_mix=sg.msv1_p_mix(0.7, 6.0), key_every=16)
    path = tmp_path / "clip.avi"
    path.write_bytes(avi.write_avi(320, 240, frames, fourcc=b"CRAM", bpp=16, fps=15.0, key_flags=keys))

    def run(extra):
        res = subprocess.run([exe, str(path)] + extra, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
        assert res.returncode == 0, res.stderr.decode()
        return [l.split() for l in res.stdout.decode().splitlines() if l and l[0].isdigit()]

    plain = sorted((int(l[0]), l[1], int(l[3]), l[-1]) for l in run([]))
    back = run(["--step-back"])
    assert [int(l[0]) for l in back] == list(range(39, -1, -1))
    assert sorted((int(l[0]), l[1], int(l[2]), l[-1]) for l in back) == plain
