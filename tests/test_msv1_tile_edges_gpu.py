"""The directed tile-boundary catalogue (tests/msv1_directed_streams.py) through every MSVideo1 decode path on an MI355X
(run with -m gpu), bit-exact against the CPU oracle: every buffer's pixels, significant_changes, adoption, raised-or-not.

  a. DecompressI / DecompressP with msv1_parse=host;
  b. the same calls with msv1_parse=gpu;
  c. stage_batch of the key-frame cases (the fused batch form, 16 KiB tiles);
  d. stage_batch of the inter-frame cases (the table-writing form, 8 KiB tiles, plus the temporal kernel), replayed twice
     with msv1_scrub_tables on;
  e. c and d again with msv1_inject_fault=1 (the three-kernel descriptor parse);
  f. the asynchronous calls in every msv1_async form, msv1_async_pairs on and off (one-frame launches, 8 KiB tiles);
  g. one directed clip through Seek, FindChange and BuildIndex -> Show against the frame-by-frame truth.

No path may pass by quietly taking another one: the catalogue says for every frame whether the on-GPU parse settles it or
hands it to the host parser (by design only the malformed ones: too short, an 8-bit end marker on the chain, a skip code
with no previous frame), and the tests hold the product to that through jsp_counter ("host_parsed_frames", "async_reruns",
"lookback_fallbacks") and StagedBatch.kernels() / info()."""
import functools

import numpy as np
import pytest

import msv1_directed_streams as D
import msv1_range_clips as R
from jsplayer_amd import CodecError, MSVideo1_16bit, MSVideo1_8bit
from oracle_binding import OracleAbort, OracleMSVideo1
from test_async_gpu import drive

pytestmark = pytest.mark.gpu

LINES = 36


def dev_buf(n, fill=D.PREFILL):
    import torch
    return torch.full((n,), fill, dtype=torch.int32, device="cuda")


def make_gpu(bits, w, h, parse):
    c = MSVideo1_16bit(w, h) if bits == 16 else MSVideo1_8bit(w, h, D.palette(bits))
    c.set_option("msv1_parse", parse)
    return c


def geometries(bits):
    return sorted({(c.w, c.h) for c in D.catalogue(bits)})


@functools.lru_cache(maxsize=None)
def clips(bits, w, h):
    """The cases of one geometry as two long clips — the ones the GPU settles alone, and the ones with a frame it hands to the
    host parser (the case the reference raises on first: it needs a codec with no previous frame) — as (names, frames, keys,
    host flags) each."""
    out = []
    for host in (False, True):
        cs = [c for c in D.catalogue(bits) if (c.w, c.h) == (w, h) and c.any_host == host]
        cs.sort(key=lambda c: not c.raises)                    # (stable: the raising case first)
        names, frames, keys, hosts = [], [], [], []
        for c in cs:
            for i, (src, key) in enumerate(c.frames):
                names.append(f"{c.name}[{i}]")
                frames.append(src)
                keys.append(key)
                hosts.append(c.host[i])
        out.append((names, frames, keys, hosts))
    return out


# (bits, w, h) of every geometry of the catalogue.  Stated here, not derived at import: building the catalogue takes seconds,
# and every collection of the suite would pay for it.
GEOMETRIES = [(16,) + D.SIZES[16], (16,) + D.BIG, (8,) + D.SIZES[8], (8,) + D.BIG]
GEOMETRY_IDS = [f"{b}-{w}x{h}" for b, w, h in GEOMETRIES]


def test_the_geometries_named_here_are_the_catalogue_s():
    assert sorted(GEOMETRIES) == sorted((bits, w, h) for bits in (16, 8) for (w, h) in geometries(bits))


# ---- a, b: the synchronous calls -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("parse", ["host", "gpu"])
@pytest.mark.parametrize("bits,w,h", GEOMETRIES, ids=GEOMETRY_IDS)
def test_synchronous_calls(bits, w, h, parse):
    """Manager's buffer protocol, oracle and HIP path in step (as drive_pair of test_msvideo1_gpu.py), and after every frame
    what the counters say about who settled it."""
    nbuf = 3
    for names, frames, keys, hosts in clips(bits, w, h):
        if not frames:
            continue
        orc = OracleMSVideo1(bits, w, h, D.palette(bits))
        gpu = make_gpu(bits, w, h, parse)
        orc.Preinit(LINES)
        gpu.Preinit(LINES)
        obufs = [np.full(w * h, D.PREFILL, dtype=np.int32) for _ in range(nbuf)]
        gbufs = [dev_buf(w * h) for _ in range(nbuf)]
        for i, (src, key) in enumerate(zip(frames, keys)):
            where = f"{bits}-bit {w}x{h} {names[i]} ({parse} parse)"
            oprev, gprev = orc.PreviousFrame(), gpu.PreviousFrame()
            oi = next(k for k in range(nbuf) if obufs[k] is not oprev)
            gi = next(k for k in range(nbuf) if gbufs[k] is not gprev)
            assert oi == gi, where + ": buffer choice diverged"
            assert gpu.IsKeyFrame(src) == orc.IsKeyFrame(src), where
            before = (gpu.counter("host_parsed_frames"), gpu.counter("async_reruns"))
            if key:
                assert orc.DecompressI(src, obufs[oi]) == 0
                assert gpu.DecompressI(src, gbufs[gi]) == 0, where
            else:
                try:
                    odata, osig = orc.DecompressP(src, obufs[oi])
                except OracleAbort:
                    with pytest.raises(CodecError):
                        gpu.DecompressP(src, gbufs[gi])
                else:
                    res = gpu.DecompressP(src, gbufs[gi])
                    assert res.significant_changes == osig, where + ": significant_changes"
                    assert (res.data_pnt is gbufs[gi]) == (odata is obufs[oi]), where + ": data_pnt identity"
                    assert (res.data_pnt is None) == (odata is None), where
            onow, gnow = orc.PreviousFrame(), gpu.PreviousFrame()
            assert [k for k in range(nbuf) if obufs[k] is onow] == [k for k in range(nbuf) if gbufs[k] is gnow], where
            for k in range(nbuf):
                assert np.array_equal(obufs[k], gbufs[k].cpu().numpy()), where + f": buffer {k} differs"
            settled_by_host = gpu.counter("host_parsed_frames") - before[0]
            reruns = gpu.counter("async_reruns") - before[1]
            if parse == "gpu":
                assert settled_by_host == (1 if hosts[i] else 0), where + ": who settled the frame"
                assert reruns <= settled_by_host, where + ": a frame the GPU settles was re-run"
            else:
                assert settled_by_host == 0 and reruns == 0, where
        gpu.StopAndClean()


# ---- c, d, e: staged batches ---------------------------------------------------------------------------------------------------
def batch_frames(bits, w, h, keys_only):
    """(names, frames, keys, host flags, consumed, coded) of the batch of one geometry: the directed key frames, or the clips of
    every other case one after the other (the case the reference raises on first)."""
    rows = [(f"{c.name}[{i}]", c.frames[i][0], c.frames[i][1], c.host[i], c.consumed[i], c.coded[i], c.raises and i == c.directed, c.name)
            for c in batch_cases(bits, w, h, keys_only) for i in range(len(c.frames))]
    return rows


def batch_cases(bits, w, h, keys_only):
    cs = [c for c in D.catalogue(bits) if (c.w, c.h) == (w, h) and c.key_case == keys_only]
    cs.sort(key=lambda c: not c.raises)
    return cs


def oracle_batch(bits, w, h, rows):
    """Every frame into a buffer of its own -> (buffers, per frame: raised, significance, adopted)."""
    orc = OracleMSVideo1(bits, w, h, D.palette(bits))
    orc.Preinit(LINES)
    obufs = [np.full(w * h, D.PREFILL, dtype=np.int32) for _ in rows]
    verdicts = []
    for i, row in enumerate(rows):
        if row[2]:
            assert orc.DecompressI(row[1], obufs[i]) == 0
            verdicts.append((False, None, True))
            continue
        try:
            data, sig = orc.DecompressP(row[1], obufs[i])
            verdicts.append((False, sig, data is obufs[i]))
        except OracleAbort:
            verdicts.append((True, None, False))
    return obufs, verdicts


@pytest.mark.parametrize("inject", [False, True], ids=["look-back", "injected-fault"])
@pytest.mark.parametrize("keys_only", [True, False], ids=["key-frames", "inter-frames"])
@pytest.mark.parametrize("bits,w,h", GEOMETRIES, ids=GEOMETRY_IDS)
def test_staged_batches(bits, w, h, keys_only, inject):
    rows = batch_frames(bits, w, h, keys_only)
    assert rows
    n = len(rows)
    nb = (w // 4) * (h // 4)
    where = f"{bits}-bit {w}x{h} {'key' if keys_only else 'inter'}-frame batch of {n}" + (", fault injected" if inject else "")
    obufs, verdicts = oracle_batch(bits, w, h, rows)
    frames, keys = [r[1] for r in rows], [r[2] for r in rows]
    # what the host parser makes of the same batch: the accounting must not depend on who parsed
    ref = make_gpu(bits, w, h, "host")
    ref.Preinit(LINES)
    dsts = [dev_buf(w * h) for _ in range(n)]
    st = ref.stage_batch(frames, dsts, is_key=keys)
    want_info = st.info()
    st.close()
    ref.StopAndClean()

    gpu = make_gpu(bits, w, h, "gpu")
    gpu.Preinit(LINES)
    gpu.set_option("msv1_scrub_tables", "1")
    if inject:
        gpu.set_option("msv1_inject_fault", "1")
    st = gpu.stage_batch(frames, dsts, is_key=keys)
    n_host = sum(1 for r in rows if r[3])
    assert gpu.counter("host_parsed_frames") == n_host, where + ": frames handed to the host parser"
    info = st.info()
    for k in ("frames", "units_coded", "units_copied", "stream_bytes", "algorithmic_bytes"):
        assert info[k] == want_info[k], f"{where}: info()['{k}'] differs from the host parser's"
    if n_host == 0:       # ... and is what the catalogue says by construction
        assert info["stream_bytes"] == sum(r[4] for r in rows), where + ": bytes consumed"
        assert info["units_coded"] == sum(r[5] for r in rows) and info["units_copied"] == n * nb - info["units_coded"], where
    else:                 # ... and so is what the well-formed frames of the batch add to it, staged without the others
        good = {c.name for c in batch_cases(bits, w, h, keys_only) if not c.any_host}
        good_rows = [r for r in rows if r[7] in good]
        alone = make_gpu(bits, w, h, "gpu")
        alone.Preinit(LINES)
        sub = alone.stage_batch([r[1] for r in good_rows], dsts[:len(good_rows)], is_key=[r[2] for r in good_rows])
        sub_info = sub.info()
        sub.close()
        assert alone.counter("host_parsed_frames") == 0, where + ": a well-formed frame was handed to the host parser"
        alone.StopAndClean()
        assert sub_info["stream_bytes"] == sum(r[4] for r in good_rows), where + ": bytes consumed by the well-formed frames"
        assert sub_info["units_coded"] == sum(r[5] for r in good_rows), where + ": blocks coded by the well-formed frames"
        assert sub_info["units_copied"] == len(good_rows) * nb - sub_info["units_coded"], where
    kernels = st.kernels()
    assert "fallback" not in kernels
    if keys_only:
        assert kernels == "msv1_fused_kernel", f"{where}: {kernels}"
    else:
        assert "msv1_blocks_temporal_kernel" in kernels and "msv1_fused_kernel" in kernels, f"{where}: {kernels}"
    for run in range(1 if keys_only else 3):                       # (the replays rebuild their scrubbed block tables)
        for d in dsts:
            d.fill_(D.PREFILL)
        st.decode()
        gpu.sync()
        status, adopted, signif = st.results()
        for i, (raised, sig, ad) in enumerate(verdicts):
            at = f"{where}, run {run}, {rows[i][0]}"
            assert (status[i] != 0) == raised, at + ": raised or not"
            if not raised:
                assert bool(adopted[i]) == ad, at + ": adoption"
                if sig is not None:
                    assert bool(signif[i]) == sig, at + ": significant_changes"
            assert np.array_equal(obufs[i], dsts[i].cpu().numpy()), at + ": pixels"
        if inject:
            assert "look-back fallback" in st.kernels(), where
    assert gpu.counter("lookback_fallbacks") == (1 if inject else 0), where
    assert gpu.counter("host_parsed_frames") == n_host, where
    st.close()
    gpu.StopAndClean()


@pytest.mark.parametrize("bits,w,h", GEOMETRIES, ids=GEOMETRY_IDS)
def test_staged_batches_hand_exactly_the_malformed_frames_to_the_host_parser(bits, w, h):
    """The total of test_staged_batches would also come out with a well-formed frame handed over and a malformed one kept.
    Here every case with a malformed frame is staged as a batch of its own (its clip: nothing in it depends on the batch
    around it) and must hand over exactly its malformed frames, and the batch of all the other cases none."""
    cs = batch_cases(bits, w, h, False)
    gpu = make_gpu(bits, w, h, "gpu")
    gpu.Preinit(LINES)
    dsts = [dev_buf(w * h) for _ in range(max(len(c.frames) for c in cs))]

    def handed_over(frames):
        before = gpu.counter("host_parsed_frames")
        while len(dsts) < len(frames):
            dsts.append(dev_buf(w * h))
        st = gpu.stage_batch([f[0] for f in frames], dsts[:len(frames)], is_key=[f[1] for f in frames])
        st.close()
        return gpu.counter("host_parsed_frames") - before

    for c in cs:
        if c.any_host:
            assert handed_over(c.frames) == sum(c.host), f"{bits}-bit {w}x{h} {c.name}: {c.why_host}"
    good = [f for c in cs if not c.any_host for f in c.frames]
    assert good and handed_over(good) == 0, f"{bits}-bit {w}x{h}: a well-formed frame was handed to the host parser"
    gpu.StopAndClean()


# ---- f: the asynchronous calls -------------------------------------------------------------------------------------------------
def expected_reruns(hosts, depth):
    """async_reruns after drive(): frame f is waited for with the frames up to f + depth - 1 submitted behind it (fewer at the
    end of the clip); if the GPU cannot settle f, it and everything submitted behind it is re-run through the synchronous
    path, once, whoever settles those frames there.  Nothing else is re-run."""
    n, total, done = len(hosts), 0, 0
    for f, host in enumerate(hosts):
        if host and f >= done:
            done = min(f + depth, n)
            total += done - f
    return total


@pytest.mark.parametrize("pairs", ["on", "off"])
@pytest.mark.parametrize("form", ["one_launch_dma", "one_launch", "two_launches"])
@pytest.mark.parametrize("bits,w,h", GEOMETRIES, ids=GEOMETRY_IDS)
def test_asynchronous_calls(bits, w, h, form, pairs):
    """drive() of test_async_gpu.py: four frames in flight, the compressed frames in pinned memory.  The frames the GPU settles
    alone must all be settled there (no re-run, no host parse); of the others exactly the malformed ones reach the host parser
    (whatever was in flight behind one is re-run with it, and parsed on the GPU again)."""
    for names, frames, keys, hosts in clips(bits, w, h):
        if not frames:
            continue
        gpu = make_gpu(bits, w, h, "gpu")
        gpu.set_option("msv1_async", form)
        gpu.set_option("msv1_async_pairs", pairs)
        seen = {}
        drive(gpu, OracleMSVideo1(bits, w, h, D.palette(bits)), w, h, frames, keys, depth=4, pinned=True, lines=LINES,
              before_close=lambda g: seen.update(host=g.counter("host_parsed_frames"), reruns=g.counter("async_reruns"),
                                                 paired=g.counter("paired_frames")))
        where = f"{bits}-bit {w}x{h} msv1_async={form} pairs={pairs}: {seen}"
        n_host = sum(hosts)
        assert seen["host"] == n_host, where
        if n_host == 0:
            if form != "two_launches":
                assert (seen["paired"] > 0) == (pairs == "on"), where
        assert seen["reruns"] == expected_reruns(hosts, 4), where


# ---- g: the range calls --------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def range_clip(bits):
    """A key frame and a dozen directed inter frames from the skip, trailing-bytes and straddle groups, and the truth."""
    w, h = D.SIZES[bits]
    pick = [c for c in D.catalogue(bits) if (c.w, c.h) == (w, h) and not c.key_case and not c.any_host
            and c.group.split("+")[0] in ("skip", "trailing", "straddle")]
    by_group = {g: [c for c in pick if c.group.split("+")[0] == g] for g in ("skip", "trailing", "straddle")}
    chosen = by_group["skip"][:4] + by_group["trailing"][:4] + by_group["straddle"][::max(1, len(by_group["straddle"]) // 4)][:4]
    assert len(chosen) == 12
    frames = [D.key_frame(bits, w, h).data] + [c.frames[-1][0] for c in chosen]
    keys = [True] + [False] * len(chosen)
    truth = R.truth_run(bits, w, h, D.palette(bits), frames, keys, LINES, key_row=LINES)
    assert all(t is not None and t[0] is not None for t in truth)
    return frames, keys, truth


@pytest.mark.parametrize("parse", ["host", "gpu"])
@pytest.mark.parametrize("bits", [16, 8])
def test_range_calls_on_a_directed_clip(bits, parse):
    w, h = D.SIZES[bits]
    pal = D.palette(bits)
    frames, keys, truth = range_clip(bits)
    n = len(frames)
    where = f"{bits}-bit {w}x{h} ({parse} parse)"
    # Seek from the key frame
    for t in (1, n // 2, n - 1):
        gpu = R.make_gpu(bits, w, h, pal, LINES, None, parse)
        dst = R.dev_buf(w * h)
        res = gpu.Seek(frames[:t + 1], dst, keys[:t + 1])
        assert res.data_pnt is dst and gpu.PreviousFrame() is dst, f"{where} seek 0..{t}"
        assert np.array_equal(dst.cpu().numpy(), truth[t][0]), f"{where} seek 0..{t}: picture"
        assert res.significant_changes == truth[t][1], f"{where} seek 0..{t}"
        gpu.StopAndClean()
    # FindChange, landing after landing
    R.walk(bits, w, h, pal, frames, keys, lines=LINES, parse=parse, truth=truth)
    # BuildIndex -> Show
    gpu = R.make_gpu(bits, w, h, pal, LINES, None, parse)
    idx = gpu.BuildIndex(frames, keys, key_row=LINES)
    assert idx.frames == n and idx.significance == [t[1] for t in truth], where
    dst = R.dev_buf(w * h)
    for t in range(n):
        dst.fill_(R.POISON)
        r = idx.Show(t, dst, adopt=False)
        assert r.data_pnt is dst, f"{where} show({t})"
        assert np.array_equal(dst.cpu().numpy(), truth[t][0]), f"{where} show({t}): picture"
        assert r.significant_changes == (False if keys[t] else truth[t][1]), f"{where} show({t})"
    if parse == "gpu":
        assert gpu.counter("host_parsed_frames") == 0, where
    idx.close()
    gpu.StopAndClean()
