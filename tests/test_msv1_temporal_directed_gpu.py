"""The directed inter-frame groups of tests/msv1_temporal_clips.py through msv1_blocks_temporal_kernel on an MI355X (run with
-m gpu): every clip staged as one batch with msv1_parse=host and =gpu, msv1_scrub_tables on, decoded once and replayed twice
with the buffers refilled between the runs — every buffer bit-equal to the CPU oracle's, status, adoption and significance the
oracle's, after every run.

No clip may pass by quietly taking another path: the kernels the batch launches are the ones the clip was built for
(msv1_blocks_temporal_kernel; with it msv1_edge_compare_kernel where Y % 4 != 0 and the frames compare; msv1_blocks_kernel
instead where X % 4 != 0), no look-back fall-back is taken, and the on-GPU parse hands to the host parser exactly the frames
the model says it must (truncated frames, and 16-bit frames shorter than size_of_just_skips).  What each clip pins, and that a
kernel with one of twelve named mistakes would fail on it, is shown without a GPU in tests/test_msv1_temporal_clips_cpu.py."""
import numpy as np
import pytest

import msv1_directed_streams as D
import msv1_temporal_clips as K
import msv1_temporal_plan as P
import test_msv1_temporal_clips_cpu as T
from jsplayer_amd import MSVideo1_16bit, MSVideo1_8bit
from oracle_binding import OracleMSVideo1

pytestmark = pytest.mark.gpu

NAMES = T.NAMES


def make_gpu(c, parse):
    g = MSVideo1_16bit(c.w, c.h) if c.bits == 16 else MSVideo1_8bit(c.w, c.h, D.palette(c.bits))
    g.set_option("msv1_parse", parse)
    g.Preinit(c.lines)
    return g


def device_buffers(c):
    import torch
    assert all(0 <= v < 2 ** 31 for v in c.prefills)
    return [torch.full((c.w * c.h,), v, dtype=torch.int32, device="cuda") for v in c.prefills]


def refill(c, bufs, upto):
    for k in range(upto):
        bufs[k].fill_(c.prefills[k])


@pytest.mark.parametrize("parse", ["host", "gpu"])
@pytest.mark.parametrize("name", NAMES)
def test_staged_and_replayed(name, parse):
    c = K.by_name(name)
    obufs, oadopted, osignif = T.oracle_run(name)
    staged = T.model_run(c, P.GPU_ALIGN if parse == "gpu" else P.HOST_ALIGN)[3]
    n = len(c.frames)
    where = f"{name} ({parse} parse)"
    gpu = make_gpu(c, parse)
    gpu.set_option("msv1_scrub_tables", "1")
    bufs = device_buffers(c)
    if c.start == "sync":
        assert gpu.DecompressI(c.sync_key, bufs[c.nbuf]) == 0, where
    before = gpu.counter("host_parsed_frames")
    st = gpu.stage_batch([f for f, _ in c.frames], [bufs[d] for d in c.dsts], is_key=[k for _, k in c.frames])
    kernels = st.kernels()
    assert "fallback" not in kernels, f"{where}: {kernels}"
    if c.kernel == "msv1_blocks_temporal_kernel":
        assert "msv1_blocks_temporal_kernel" in kernels and "msv1_blocks_kernel" not in kernels, f"{where}: {kernels}"
    else:
        assert "msv1_blocks_kernel" in kernels and "msv1_blocks_temporal_kernel" not in kernels, f"{where}: {kernels}"
    assert ("msv1_edge_compare_kernel" in kernels) == c.edge, f"{where}: {kernels}"
    handed_over = sum(a.host for a in staged.frames) if parse == "gpu" else 0
    assert gpu.counter("host_parsed_frames") - before == handed_over, where + ": frames handed to the host parser"
    upto = c.nbuf if c.start == "sync" else len(bufs)           # (the synchronous key frame's buffer is not the batch's to write)
    for run in range(3):
        refill(c, bufs, upto)
        st.decode()
        gpu.sync()
        status, adopted, signif = st.results()
        at = f"{where}, run {run}"
        assert status == [0] * n, at
        assert [bool(a) for a in adopted] == oadopted, at + ": adoption"
        assert [bool(s) for s in signif] == osignif, at + ": significant_changes"
        for k, want in enumerate(obufs):
            got = bufs[k].cpu().numpy().view(np.uint32)
            if not np.array_equal(got, want):
                bad = np.nonzero(got != want)[0]
                y, x = divmod(int(bad[0]), c.w)
                raise AssertionError(f"{at}: buffer {k} differs in {bad.size} pixels, first at ({x}, {y}), block {(y // 4) * (c.w // 4) + x // 4}")
    assert gpu.counter("lookback_fallbacks") == 0, where
    assert gpu.counter("host_parsed_frames") - before == handed_over, where
    st.close()
    gpu.StopAndClean()


@pytest.mark.parametrize("parse", ["host", "gpu"])
@pytest.mark.parametrize("name", ["code_cut_16", "tails_8"])
def test_the_same_clip_through_the_synchronous_calls(name, parse):
    """The cross-check: DecompressI / DecompressP frame by frame into the clip's buffers, the oracle in step."""
    c = K.by_name(name)
    gpu = make_gpu(c, parse)
    orc = OracleMSVideo1(c.bits, c.w, c.h, D.palette(c.bits))
    orc.Preinit(c.lines)
    obufs = [b.view(np.int32) for b in T.fresh_buffers(c)]
    gbufs = device_buffers(c)
    if c.start == "sync":
        assert orc.DecompressI(c.sync_key, obufs[c.nbuf]) == 0 and gpu.DecompressI(c.sync_key, gbufs[c.nbuf]) == 0
    for i, ((src, key), d) in enumerate(zip(c.frames, c.dsts)):
        at = f"{name} ({parse} parse) frame {i}"
        if key:
            assert orc.DecompressI(src, obufs[d]) == 0 and gpu.DecompressI(src, gbufs[d]) == 0, at
        else:
            odata, osig = orc.DecompressP(src, obufs[d])
            res = gpu.DecompressP(src, gbufs[d])
            assert res.significant_changes == osig, at
            assert (res.data_pnt is gbufs[d]) == (odata is obufs[d]), at
        assert np.array_equal(obufs[d], gbufs[d].cpu().numpy()), at + ": pixels"
    final, _, _ = T.oracle_run(name)
    for k, want in enumerate(final):
        assert np.array_equal(gbufs[k].cpu().numpy().view(np.uint32), want), f"{name} ({parse} parse): buffer {k}"
    gpu.StopAndClean()
