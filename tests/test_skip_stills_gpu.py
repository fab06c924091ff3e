"""jsp_find_change / FindChange / Manager.skip_stills on an MI355X against the oracle.

Truth: OracleMSVideo1 stepped frame by frame, each destination first copied from the picture before it (the `Truth` pattern of
test_seek_gpu.py, the contract's equivalence); key frames get the Manager's frames_differ_significantly computed in numpy.
The clips are built here by hand: a key frame of solid blocks, then idle stretches of the kinds screen recordings are made of
(all-skip frames of both early-out sizes and longer, blocks recoded with the colour they already hold — solid, 2-colour and
8-colour codes —, changes only above the insignificant lines or only in the block row that straddles them), real changes, and
key frames that repeat the one before or repaint the same picture."""
import os
import subprocess

import numpy as np
import pytest

from jsplayer_amd import CodecError, MSVideo1_16bit, MSVideo1_8bit, ScreenPressor, player
from jsplayer_amd import streamgen as sg
from msv1_range_clips import Idle, expected_landing, truth_run
from msv1_range_clips import walk as _walk
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


def dev_buf(n, fill=POISON, misalign=False):
    import torch
    if misalign:
        return torch.full((n + 4,), fill, dtype=torch.int32, device="cuda")[1:1 + n]
    return torch.full((n,), fill, dtype=torch.int32, device="cuda")


def make_gpu(bits, w, h, pal=None, lines=36, chunk=None):
    c = MSVideo1_16bit(w, h) if bits == 16 else MSVideo1_8bit(w, h, pal or b"")
    c.set_option("msv1_parse", PARSE)
    if chunk:
        c.set_option("msv1_seek_chunk_frames", str(chunk))
    c.Preinit(lines)
    return c


# ---- clips (Idle: msv1_range_clips) -------------------------------------------------------------------------------------
def idle_clip(bits, w, h, seed=1, lines=36, stretches=(3, 1, 5, 2, 0, 4), with_keys=True):
    """(frames, keys, palette): a key frame, then idle stretches of the given lengths each ending in a real change, mixed
    with key frames that repeat the one before (bytes) or repaint the same picture."""
    g = Idle(bits, w, h, seed)
    pal = sg.msv1_clip(5, 8, 8, 1, bits=8)[2] if bits == 8 else None
    frames, keys = [g.key()], [True]
    insig_rows = max(0, lines // 4)
    kinds = ["empty", "short", "long", "repaint", "top", "edge"]
    for si, n in enumerate(stretches):
        for j in range(n):
            kind = kinds[(si + j) % len(kinds)]
            if kind in ("empty", "short", "long"):
                f = g.all_skip(kind)
            elif kind == "repaint":
                f = g.recode([int(b) for b in g.rng.choice(g.nb, size=max(1, g.nb // 5), replace=False)])
            elif kind == "top":
                f = g.change(g.row_of(min(insig_rows, g.nby) - 1)) if insig_rows >= 1 else g.recode(g.row_of(0))
            else:
                f = g.recode(g.row_of(min(insig_rows, g.nby - 1)), how="two")
            frames.append(f)
            keys.append(False)
        if with_keys and si % 3 == 1:
            frames.append(g.key(same=True, how="two"))   # a key frame that repaints the picture as it is, in other bytes
            keys.append(True)
            frames.append(frames[-1])                                      # ... and one byte-identical to it
            keys.append(True)
        frames.append(g.change([int(g.rng.integers(0, g.nb))] + g.row_of(g.nby - 1, 1)))
        keys.append(False)
    if with_keys:
        frames.append(g.key())
        keys.append(True)
    frames.append(g.recode(list(range(g.nb))))            # an idle tail
    keys.append(False)
    frames.append(g.all_skip("long"))
    keys.append(False)
    return frames, keys, pal


# ---- the walk (truth_run, expected_landing, walk: msv1_range_clips) ------------------------------------------------------------
def walk(bits, w, h, pal, frames, keys, lines=36, chunk=None, misalign=False, step=True):
    """msv1_range_clips.walk with this module's parse mode."""
    return _walk(bits, w, h, pal, frames, keys, lines=lines, chunk=chunk, misalign=misalign, step=step, parse=PARSE)


@pytest.mark.parametrize("bits", [16, 8])
@pytest.mark.parametrize("size,lines", [((4, 4), 0), ((37, 23), 8), ((64, 48), 20), ((320, 240), 36)],
                         ids=lambda v: f"{v[0]}x{v[1]}" if isinstance(v, tuple) else str(v))
def test_walk_lands_where_the_oracle_changes(bits, size, lines):
    w, h = size
    frames, keys, pal = idle_clip(bits, w, h, seed=w + bits, lines=lines)
    for step in (False, True):
        landings, truth = walk(bits, w, h, pal, frames, keys, lines=lines, step=step)
        if not step:   # skipping from frame 0 to the end: the significant candidates, then the last frame of the idle tail
            want = [k for k in range(1, len(frames)) if truth[k][1]]
            if not want or want[-1] != len(frames) - 1:
                want.append(len(frames) - 1)
            assert landings == want
        if bits == 8:  # an 8-bit inter frame with a previous picture is never significant: landings are key frames or the end
            assert all(keys[f] or f == len(frames) - 1 for f in landings)


@pytest.mark.parametrize("bits", [16, 8])
def test_line_vs_block_row_granularity(bits):
    """Preinit(37) / (38): changes on the first pixel line of the block row that straddles the insignificant lines."""
    w, h = 32, 64
    for lines in (36, 37, 38, 40):
        g = Idle(bits, w, h, seed=lines)
        pal = sg.msv1_clip(5, 8, 8, 1, bits=8)[2] if bits == 8 else None
        frames, keys = [g.key()], [True]
        for by in (8, 9, 10):
            frames += [g.first_line_only(by), g.recode(g.row_of(by, 3), how="eight"), g.all_skip("long")]
            keys += [False] * 3
        walk(bits, w, h, pal, frames, keys, lines=lines, step=False)
        walk(bits, w, h, pal, frames, keys, lines=lines, step=True)


@pytest.mark.parametrize("bits", [16, 8])
def test_full_hd_and_unaligned_buffers(bits):
    w, h = 1920, 1080
    frames, keys, pal = idle_clip(bits, w, h, seed=3, stretches=(6, 0, 9), with_keys=True)
    walk(bits, w, h, pal, frames, keys, step=True)
    frames, keys, pal = idle_clip(bits, 100, 52, seed=4, lines=12)
    walk(bits, 100, 52, pal, frames, keys, lines=12, misalign=True, step=True)


@pytest.mark.parametrize("chunk", [1, 3])
def test_chunks_give_the_one_chunk_result(chunk):
    w, h = 64, 48
    for seed in range(3):
        frames, keys, pal = idle_clip(16, w, h, seed=seed, lines=20, stretches=(2, 3, 1, 4, 5))
        a, _ = walk(16, w, h, pal, frames, keys, lines=20, chunk=chunk, step=False)
        b, _ = walk(16, w, h, pal, frames, keys, lines=20, step=False)
        assert a == b
        walk(16, w, h, pal, frames, keys, lines=20, chunk=chunk, step=True)


@pytest.mark.parametrize("bits", [16, 8])
def test_damaged_frames_inside_idle_stretches(bits):
    w, h = 32, 48
    g = Idle(bits, w, h, seed=9)
    pal = sg.msv1_clip(5, 8, 8, 1, bits=8)[2] if bits == 8 else None
    frames, keys = [g.key()], [True]
    change = g.change(g.row_of(10) + g.row_of(11))
    for cut in (1, 3, 5, len(change) // 2, len(change) - 1):
        frames += [g.recode(g.row_of(9)), change[:cut], g.all_skip("long")]
        keys += [False] * 3
    if bits == 8:
        body = g.recode(g.row_of(10) + g.row_of(11), how="solid")
        frames.append(body[:4] + b"\x00\x00" + body[4:])   # end marker inside a repaint
        keys.append(False)
        frames.append(g.change(g.row_of(11))[:6] + b"\x00\x00")
        keys.append(False)
    frames.append(change + b"\x07")                          # odd trailing byte
    keys.append(False)
    frames.append(g.all_skip("short"))
    keys.append(False)
    walk(bits, w, h, pal, frames, keys, lines=36, step=False)
    walk(bits, w, h, pal, frames, keys, lines=36, step=True)


def test_first_past_zero_and_key_before():
    w, h = 64, 48
    frames, keys, pal = idle_clip(16, w, h, seed=21, lines=20)
    n = len(frames)
    for first in (1, 4, 9, n - 1):
        truth = truth_run(16, w, h, pal, frames, keys, lines=20, key_row=20)
        gpu = make_gpu(16, w, h, lines=20)
        dst = dev_buf(w * h)
        res = gpu.FindChange(frames, dst, keys, first=first, key_row=20)
        want = expected_landing(truth, first)
        assert res.index == want and res.changed == truth[want][1]
        assert all(s is None for s in res.significance[:first])
        assert np.array_equal(gpu.PreviousFrame().cpu().numpy(), truth[want][0])
        gpu.StopAndClean()
    # a range opening with a key frame: key_before names the key frame in front of it (bytes compared), or not (pixels compared)
    g = Idle(16, w, h, seed=5)
    k0 = g.key()
    same, other = g.key(same=True, how="two"), g.key()
    for kb, opener in ((k0, k0), (k0, same), (None, same), (None, k0), (None, other)):
        o = OracleMSVideo1(16, w, h)
        o.Preinit(20)
        ref = np.full(w * h, POISON, dtype=np.int32)
        assert o.DecompressI(k0, ref) == 0
        gpu = make_gpu(16, w, h, lines=20)
        a = dev_buf(w * h)
        assert gpu.DecompressI(k0, a) == 0
        res = gpu.FindChange([opener, other], dev_buf(w * h), [True, True], 0, kb, 20)
        pic = ref.copy()
        o2 = OracleMSVideo1(16, w, h)
        o2.Preinit(20)
        assert o2.DecompressI(opener, pic) == 0
        want0 = (bytes(kb) != bytes(opener)) if kb is not None else bool(np.any(pic[20 * w:] != ref[20 * w:]))
        assert res.significance[0] == want0, (kb is not None, opener is k0)
        assert res.index == (0 if want0 else 1)
        gpu.StopAndClean()


def test_refusals_change_nothing():
    w, h = 64, 48
    chunks, keys, _ = sg.sp_clip(3, w, h, 4, version=4)
    sp = ScreenPressor(w, h, 24)
    sp.Preinit(36)
    a = dev_buf(w * h, 0)
    assert sp.DecompressI(chunks[0], a) == 0
    with pytest.raises(CodecError, match="MSVideo1 only"):
        sp.FindChange(chunks[1:], dev_buf(w * h), keys[1:])
    assert sp.PreviousFrame() is a
    assert not ScreenPressor.FINDS_CHANGES and MSVideo1_16bit.FINDS_CHANGES and MSVideo1_8bit.FINDS_CHANGES
    sp.StopAndClean()
    frames, keys, _ = idle_clip(16, w, h, seed=2, lines=20)
    gpu = make_gpu(16, w, h, lines=20)
    a, b, c = dev_buf(w * h), dev_buf(w * h), dev_buf(w * h)
    assert gpu.DecompressI(frames[0], a) == 0
    t = gpu.DecompressP_async(frames[1], b)
    with pytest.raises(CodecError, match="in flight"):
        gpu.FindChange(frames[2:], c, keys[2:])
    gpu.wait(t)
    prev = gpu.PreviousFrame()
    with pytest.raises(CodecError, match="previous frame"):
        gpu.FindChange(frames[2:], prev, keys[2:])
    with pytest.raises(CodecError, match="device"):
        gpu.FindChange(frames[2:], np.zeros(w * h, dtype=np.int32), keys[2:])
    for bad in (-1, len(frames) - 2):
        with pytest.raises(CodecError, match="first"):
            gpu.FindChange(frames[2:], c, keys[2:], first=bad)
    assert gpu.PreviousFrame() is prev
    assert np.all(c.cpu().numpy() == POISON)
    # the codec goes on as if nothing had been asked: the next frame against the oracle
    truth = truth_run(16, w, h, None, frames[:3], keys[:3], lines=20)
    c.copy_(prev)
    r = gpu.DecompressP(frames[2], c)
    assert r.significant_changes == truth[2][1]
    assert np.array_equal(gpu.PreviousFrame().cpu().numpy(), truth[2][0])
    gpu.StopAndClean()
    # a skip code with no picture: the error names the range index, the previous frame is gone
    bad = bytes([0x00, 0xFC, 0x01, 0x84] + [0] * 8)
    gpu = make_gpu(16, 16, 8, lines=0)
    with pytest.raises(CodecError, match="frame 1"):
        gpu.FindChange([b"", bad, frames[0]], dev_buf(16 * 8), [False, False, True])
    assert gpu.PreviousFrame() is None
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
def test_manager_skip_stills_against_the_oracle_manager(bits):
    import torch
    from jsplayer_amd.avi import CODEC_MSVC16, CODEC_MSVC8, VideoInfo
    w, h = 320, 240
    frames, keys, pal = idle_clip(bits, w, h, seed=40 + bits, stretches=(4, 2, 7, 0, 3))
    n = len(frames)
    vi = VideoInfo(X=w, Y=h, bpp=bits, fps=15.0, nframes=n, codec=CODEC_MSVC16 if bits == 16 else CODEC_MSVC8, palette=pal, riff_size=0)
    cpu = player.Manager(vi, _Orc(OracleMSVideo1(bits, w, h, pal)), lambda k: np.zeros(k, dtype=np.int32))
    dec = make_gpu(bits, w, h, pal)
    gpu = player.Manager(vi, dec, lambda k: torch.zeros(k, dtype=torch.int32, device="cuda"))
    dc, dg = cpu.worker(frames[0], 0, None, True), gpu.worker(frames[0], 0, None, True)
    landings = []
    while dg.index < n - 1:
        dc, dg = cpu.skip_stills(frames, keys), gpu.skip_stills(frames, keys)
        assert dg.index == dc.index
        assert np.array_equal(gpu.buffers[dg.buffer_index].cpu().numpy(), cpu.buffers[dc.buffer_index]), f"landing {dg.index}"
        assert gpu.frame_of_interest == dg.index and gpu.next_frame_to_decode == dg.index + 1
        landings.append(dg.index)
        if dg.index < n - 1:   # the frame after, the way a player shows it
            i = dg.index + 1
            a, b = cpu.worker(frames[i], i, None, keys[i]), gpu.worker(frames[i], i, None, keys[i])
            assert np.array_equal(gpu.buffers[b.buffer_index].cpu().numpy(), cpu.buffers[a.buffer_index]), f"frame {i}"
            if not keys[i]:
                assert a.significant_changes == b.significant_changes
            dg = b
    assert dg.index == n - 1
    # back to the start and skip again: every landing is served from what the first pass judged, through seek()
    first = landings[0]
    for mgr in (cpu, gpu):
        mgr.seek(frames, 0, keys)
    calls = []
    orig = dec.FindChange
    dec.FindChange = lambda *a, **k: calls.append(1) or orig(*a, **k)
    d = gpu.skip_stills(frames, keys)
    assert d.index == first and calls == []
    assert np.array_equal(gpu.buffers[d.buffer_index].cpu().numpy(), cpu.buffers[cpu.skip_stills(frames, keys).buffer_index])
    dec.StopAndClean()


def test_jsp_play_skip_stills_matches_the_plain_run(tmp_path):
    from jsplayer_amd import avi
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "examples", "jsp_play")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-s", "-C", os.path.join(root, "examples")])
    w, h = 320, 240
    frames, keys, _ = idle_clip(16, w, h, seed=77, stretches=(5, 3, 8, 1))
    path = tmp_path / "clip.avi"
    path.write_bytes(avi.write_avi(w, h, frames, fourcc=b"CRAM", bpp=16, fps=15.0, key_flags=keys))

    def lines(extra):
        res = subprocess.run([exe, str(path)] + extra, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
        assert res.returncode == 0, res.stderr.decode()
        return [l.split() for l in res.stdout.decode().splitlines() if l and l[0].isdigit()]

    plain = {int(l[0]): l[-1] for l in lines([])}
    assert len(plain) == len(frames)
    got = lines(["--skip-stills"])
    truth = truth_run(16, w, h, None, frames, keys)
    want, shown = [], 0
    while shown < len(frames) - 1:
        shown = expected_landing(truth, shown + 1)
        want.append(shown)
    assert [int(l[0]) for l in got] == want
    for l in got:
        assert l[-1] == plain[int(l[0])], f"frame {l[0]}: CRC"
