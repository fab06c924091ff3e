"""The motion branch of sp_pframe_kernel — the one place on the GPU that reads the picture before away from the pixel's own position —
and everything that carries moved blocks around it (the host stage's literalise_motion and quarter rule, the group kernels, the
three seek-index kernels, the Manager's frame-by-frame seek) on the directed clips of tests/sp_motion_clips.py, on an MI355X: sources
at index -1 and X*Y, above and below the picture, wrapped into the neighbouring row, at -256 and +255, sub-rectangles off the
4-pixel grid, a scroll whose every source is rewritten in the same frame, the scalar arm on a picture 75 wide and through buffers 4
bytes into their allocation (tests/test_sp_motion_clips_cpu.py asserts that the clips hold all of that).

Truth: the painted pictures, which are also the oracle's sequential run; its significant_changes and adoption alongside.  Everything
is bit-exact.  Every destination is filled with a poison word before each call and lies inside a larger poisoned allocation whose
words around it must keep the poison; the buffer of the picture before must still hold that picture.  (The asynchronous calls go
through test_async_gpu.drive, which reuses its buffers from frame to frame without refilling them: there the destinations are
guarded allocations too, and the guard words of all of them are checked once the last frame has been collected.)"""
import numpy as np
import pytest

import sp_motion_clips as mc
from jsplayer_amd import DecoderState, ScreenPressor, player
from oracle_binding import OracleScreenPressor

pytestmark = pytest.mark.gpu

POISON = 0x5A5A5A5A
PAD = 64                                   # poisoned words on either side of a destination


class Guarded:
    """A frame buffer inside a larger poisoned allocation; `misalign`: it starts 4 bytes off a 16-byte boundary; `host`: numpy."""

    def __init__(self, n, misalign=False, host=False):
        import torch
        off = PAD + (1 if misalign else 0)
        self.host = host
        self.slab = np.full(n + 2 * PAD + 4, POISON, dtype=np.int32) if host else torch.full((n + 2 * PAD + 4,), POISON, dtype=torch.int32, device="cuda")
        self.buf = self.slab[off:off + n]
        self.off, self.n = off, n
        if not host:
            assert self.buf.data_ptr() % 16 == (4 if misalign else 0)

    def poison(self):
        if self.host:
            self.buf[:] = POISON
        else:
            self.buf.fill_(POISON)

    def whole(self):
        return (self.slab if self.host else self.slab.cpu().numpy()).view(np.uint32)

    def picture(self):
        return self.whole()[self.off:self.off + self.n]

    def check_guards(self, what):
        s = self.whole()
        assert np.all(s[:self.off] == POISON) and np.all(s[self.off + self.n:] == POISON), f"{what}: written outside the destination"


def codec(c):
    gpu = ScreenPressor(c.w, c.h, c.bpp)
    gpu.Preinit(mc.KEY_ROW)
    return gpu


def exact(c, got, t, what):
    assert np.array_equal(got, c.frames[t]), f"{c.name} {what} frame {t} ({mc.role_at(c, t)}): " + mc.describe_mismatch(got, c.frames[t], c.w, c.h)


# ------------------------------------------------------------------------------------------------------- a, b: synchronous calls

def run_sync(name, nbuf, misalign=False, host=False):
    """The clip call by call through a pool used in rotation, as a player uses it: the destination is the buffer after the one
    adopted last (never the previous frame; with three buffers never the one before that either), and a frame that changes nothing
    takes none.  At the end every buffer has been a destination and holds the last picture decoded into it."""
    c = mc.clip(name)
    plan = mc.plan(name)
    _, verdicts = mc.oracle(name)
    gpu = codec(c)
    pool = [Guarded(c.w * c.h, misalign, host) for _ in range(nbuf)]
    holds = [None] * nbuf                                         # the frame whose picture each buffer holds; None: poison
    taken = [0] * nbuf                                            # how often each buffer was adopted
    k, prev = 0, None                                             # adopted frames so far; the pool index of the picture before
    what = f"{nbuf} buffers{', misaligned' if misalign else ''}{', host pointers' if host else ''},"
    for t, (src, key) in enumerate(zip(c.chunks, c.keys)):
        at = k % nbuf
        dst = pool[at]
        assert at != prev and dst.buf is not gpu.PreviousFrame()
        dst.poison()
        holds[at] = None
        if key:
            assert gpu.DecompressI(src, dst.buf) == DecoderState.zero_state, t
        else:
            res = gpu.DecompressP(src, dst.buf)
            assert res.significant_changes == verdicts[t], f"{c.name} {what} frame {t}: verdict"
            if plan[t]["kind"] == "none":
                assert res.data_pnt is pool[prev].buf and gpu.PreviousFrame() is pool[prev].buf, f"{c.name} {what} frame {t}: nothing changes, the picture before stays"
            else:
                assert res.data_pnt is dst.buf, f"{c.name} {what} frame {t}: not adopted"
        if plan[t]["kind"] != "none":
            assert gpu.PreviousFrame() is dst.buf
            holds[at], prev, k = t, at, k + 1
            taken[at] += 1
        for i, g in enumerate(pool):                              # the destination, the picture before, and whatever else the pool holds
            g.check_guards(f"{c.name} {what} frame {t}")
            if holds[i] is None:
                assert np.all(g.picture() == POISON), f"{c.name} {what} frame {t}: buffer {i} was written"
            else:
                exact(c, g.picture(), holds[i], what + f" buffer {i} after frame {t},")
    assert all(n > 0 for n in taken) and len({n for n in taken}) <= 2, f"{c.name} {what} the rotation left a buffer out: {taken}"
    assert sorted(h for h in holds if h is not None)[-1] == max(t for t, p in enumerate(plan) if p["kind"] != "none")
    gpu.StopAndClean()


@pytest.mark.parametrize("nbuf", [2, 3])
@pytest.mark.parametrize("name", mc.NAMES)
def test_synchronous_calls(name, nbuf):
    run_sync(name, nbuf)


@pytest.mark.parametrize("name", ["M", "H", "Q"])
def test_synchronous_calls_through_buffers_4_bytes_into_their_allocation(name):
    """M, H and Q would take 16-byte loads and stores: here the scalar arm at a width that vectorises."""
    run_sync(name, 3, misalign=True)


@pytest.mark.parametrize("name", mc.NAMES)
def test_synchronous_calls_through_host_pointers(name):
    run_sync(name, 2, host=True)


# ---------------------------------------------------------------------------------------------------------- c: asynchronous calls

@pytest.mark.parametrize("threads", [None, "4"], ids=["default-threads", "worker-threads"])
@pytest.mark.parametrize("name", mc.NAMES)
def test_asynchronous_calls(name, threads):
    """test_async_gpu.drive: frames in flight, every result, buffer identity and picture as the oracle's — whose pictures are the
    painted ones."""
    from test_async_gpu import drive
    c = mc.clip(name)
    pictures, _ = mc.oracle(name)
    assert all(np.array_equal(p, f) for p, f in zip(pictures, c.frames))
    gpu = ScreenPressor(c.w, c.h, c.bpp)
    if threads is not None:
        gpu.set_option("sp_async_threads", threads)
    slabs = []

    def alloc(n):
        slabs.append(Guarded(n))
        return slabs[-1].buf

    def guards(_):
        assert len(slabs) > 3
        for i, g in enumerate(slabs):
            g.check_guards(f"{c.name} asynchronous calls, buffer {i}")
    drive(gpu, OracleScreenPressor(c.w, c.h, c.bpp), c.w, c.h, c.chunks, c.keys, lines=mc.KEY_ROW, before_close=guards, alloc=alloc)


# -------------------------------------------------------------------------------------------------------------- d: staged batches

@pytest.mark.parametrize("fusion", ["on", "off"])
@pytest.mark.parametrize("name,misalign", [("M", False), ("M", True), ("U", False), ("H", False), ("Q", False)],
                         ids=["M", "M-misaligned", "U", "H", "Q"])
def test_staged_batch_a_buffer_per_frame_replayed(name, misalign, fusion):
    """With the fusion the frames that move at most a quarter of their pixels ride in group launches, literalised; the edges, scroll
    and heavy frames and Q's second keep their motion blocks and take a launch of sp_pframe_kernel each, ending a run."""
    c = mc.clip(name)
    plan = mc.plan(name)
    n = len(plan)
    _, verdicts = mc.oracle(name)
    gpu = codec(c)
    gpu.set_option("sp_inter_fusion", fusion)
    dsts = [Guarded(c.w * c.h, misalign) for _ in range(n)]
    extra = Guarded(c.w * c.h, misalign)                              # never listed: must stay as it is
    st = gpu.stage_batch(c.chunks, [g.buf for g in dsts], is_key=c.keys)
    assert mc.kept(name), "no frame keeps its motion blocks"
    assert "sp_pframe_kernel" in st.kernels(), st.kernels()
    assert ("group" in st.kernels()) == (fusion == "on"), st.kernels()
    assert st.info()["kernel_launches"] == mc.launches(name, fused=fusion == "on"), (st.info()["kernel_launches"], st.kernels())
    for replay in range(2):
        for g in dsts:
            g.poison()
        st.decode()
        gpu.sync()
        status, adopted, signif = st.results()
        assert status == [0] * n
        assert [bool(a) for a in adopted] == [p["kind"] != "none" for p in plan]
        assert [bool(s) for s, k in zip(signif, c.keys) if not k] == [v for v, k in zip(verdicts, c.keys) if not k]
        for t, g in enumerate(dsts):
            what = f"staged batch, fusion {fusion}, pass {replay},"
            g.check_guards(f"{c.name} {what} frame {t}")
            if adopted[t]:
                exact(c, g.picture(), t, what)
            else:
                assert np.all(g.picture() == POISON), f"{c.name} {what} frame {t} changes nothing, its buffer was written"
        assert np.all(extra.whole() == POISON), f"{c.name}: a buffer that was not listed was written"
    st.close()
    gpu.StopAndClean()


@pytest.mark.parametrize("name", mc.NAMES)
def test_staged_in_pieces_every_kept_frame_takes_the_single_frame_kernel(name):
    """kernels() names a batch's kernels, not a frame's: here the clip goes through the codec in batches cut so that every kept
    frame (edges, scroll, heavy, Q's second) shares a batch with exactly one literalised frame — two launches, both names — and
    the pieces between them hold literalised runs only.  A frame that took the other path changes its piece's count or names."""
    c = mc.clip(name)
    plan = mc.plan(name)
    gpu = codec(c)
    dsts = [Guarded(c.w * c.h) for _ in range(len(plan))]
    seen_kept = []
    for lo, hi in mc.pieces(name):
        st = gpu.stage_batch(c.chunks[lo:hi], [g.buf for g in dsts[lo:hi]], is_key=c.keys[lo:hi])
        single, group = mc.launch_kinds(name, True, lo, hi)
        what = f"{c.name} frames {lo}..{hi - 1}: {st.kernels()}"
        assert ("sp_pframe_kernel" in st.kernels()) == single and ("group" in st.kernels()) == group, what
        assert st.info()["kernel_launches"] == mc.launches(name, True, lo, hi), what
        kept_here = [t for t in mc.kept(name) if lo <= t < hi]
        if kept_here:
            assert hi - lo == 2 and single and group and st.info()["kernel_launches"] == 2, what
            seen_kept += kept_here
        st.decode()
        gpu.sync()
        status, adopted, _ = st.results()
        assert status == [0] * (hi - lo)
        for t in range(lo, hi):
            dsts[t].check_guards(f"{c.name} staged in pieces, frame {t}")
            if adopted[t - lo]:
                exact(c, dsts[t].picture(), t, "staged in pieces,")
            else:
                assert plan[t]["kind"] == "none" and np.all(dsts[t].picture() == POISON)
        st.close()
    assert seen_kept == mc.kept(name)
    for t, g in enumerate(dsts):                                      # nothing a later piece did reached an earlier frame's buffer
        if plan[t]["kind"] != "none":
            exact(c, g.picture(), t, "staged in pieces, at the end,")
    gpu.StopAndClean()


# ------------------------------------------------------------------------------------------------------------------ e: seek index

class Indexed:
    """A motion clip, a codec and ONE index of the clip (what test_sp_index_directed_gpu.check_sheet asks of its `x`)."""

    def __init__(self, name):
        self.clip = c = mc.clip(name)
        _, self.verdicts = mc.oracle(name)
        self.n, self.size = len(c.keys), c.w * c.h
        self.gpu = codec(c)
        self.idx = self.gpu.BuildScrubIndex(c.chunks, c.keys, key_row=mc.KEY_ROW)
        assert self.idx.frames == self.n and self.idx.significance == self.verdicts
        self.extra = Guarded(self.size)

    def untouched(self, what):
        assert np.all(self.extra.whole() == POISON), f"{self.clip.name} {what}: a buffer that was not listed was written"

    def close(self):
        assert self.gpu.PreviousFrame() is None
        self.idx.close()
        self.gpu.StopAndClean()


@pytest.mark.parametrize("name", mc.NAMES)
def test_index_show_play_and_thumbs(name):
    """The index stages every inter frame literalised, the scroll and heavy frames too: no block reads the picture before away from
    its own position any more, and the pictures are the painted ones all the same."""
    from test_sp_index_directed_gpu import check_sheet
    x = Indexed(name)
    c = x.clip
    for misalign in (False, True):
        dst = Guarded(x.size, misalign)
        for t in range(x.n - 1, -1, -1):
            dst.poison()
            r = x.idx.Show(t, dst.buf)
            what = f"Show into the {'misaligned' if misalign else 'aligned'} buffer,"
            assert r.data_pnt is dst.buf and r.significant_changes == x.verdicts[t], f"{c.name} {what} frame {t}"
            exact(c, dst.picture(), t, what)
            dst.check_guards(f"{c.name} {what} frame {t}")
    bufs = [Guarded(x.size) for _ in range(x.n)]
    for first, count, stride in ((0, x.n, 1), (0, (x.n + 2) // 3, 3), (1, (x.n + 1) // 3, 3)):
        what = f"Play({first}, {count}, stride {stride}),"
        for g in bufs:
            g.poison()
        res = x.idx.Play(first, [g.buf for g in bufs[:count]], stride)
        assert len(res) == count
        for k, (r, g) in enumerate(zip(res, bufs)):
            t = first + k * stride
            assert r.data_pnt is g.buf and r.significant_changes == x.verdicts[t], f"{c.name} {what} frame {t}"
            exact(c, g.picture(), t, what)
        for g in bufs:
            g.check_guards(f"{c.name} {what}")
        assert all(np.all(g.picture() == POISON) for g in bufs[count:]), f"{c.name} {what}: a buffer that was not listed was written"
    check_sheet(x, list(range(x.n)), 4, 4, "Thumbs of every frame, scale 4, 4 to a row")
    x.untouched("Show, Play, Thumbs")
    x.close()


# -------------------------------------------------------------------------------------------------------------- f: fallback seek

def test_manager_seeks_the_last_frame_of_m_frame_by_frame():
    """No index attached and no Seek on this codec: Manager.seek decodes from the nearest key frame through worker(), frame by
    frame — the chain behind the second key frame, its light, heavy and light motion frames one on top of the other."""
    from jsplayer_amd.avi import CODEC_SCREENPRESSOR, VideoInfo
    c = mc.clip("M")
    n = len(c.keys)
    vi = VideoInfo(X=c.w, Y=c.h, bpp=c.bpp, fps=15.0, nframes=n, codec=CODEC_SCREENPRESSOR, palette=None, riff_size=0)
    dec = codec(c)
    slabs = []

    def alloc(k):
        slabs.append(Guarded(k))
        return slabs[-1].buf
    mgr = player.Manager(vi, dec, alloc)
    for t in (mc.frames_of("M", "scroll")[0], n - 1):
        out = mgr.seek(c.chunks, t, c.keys)
        assert out.index == t                  # (the Manager sets its own insignificant lines: the verdicts are not the oracle run's)
        g = next(s for s in slabs if s.buf is mgr.buffers[out.buffer_index])
        exact(c, g.picture(), t, "Manager.seek,")
        for s in slabs:
            s.check_guards(f"Manager.seek({t})")
    assert [d.index for d in mgr.log] == list(range(0, mc.frames_of("M", "scroll")[0] + 1)) + list(range(mc.frames_of("M", "key")[1], n))
    dec.StopAndClean()
