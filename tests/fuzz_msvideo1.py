#!/usr/bin/env python3
"""Randomised GPU campaign for MSVideo1 against the oracle (it lives under tests/ because it uses the oracle):
random geometry (multiples of 4 or not), depth, clip structure, skip mixes, mutated / truncated / random frames, host and
on-GPU parse, device / host / misaligned buffers, per-call API and staged batches; and `range` clips of up to 300 frames for the
range calls (Seek, FindChange, BuildIndex / Show).  Not collected by pytest.

    python tests/fuzz_msvideo1.py [seconds] [seed]
"""
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)


def main():
    budget = float(sys.argv[1]) if len(sys.argv) > 1 else 60.0
    seed = int(sys.argv[2]) if len(sys.argv) > 2 else 1
    import test_msvideo1_gpu as T
    from jsplayer_amd import streamgen as sg
    from oracle_binding import OracleMSVideo1
    rng = np.random.default_rng(seed)
    t0, clips, nframes, bad = time.time(), 0, 0, 0
    while time.time() - t0 < budget:
        if rng.random() < 0.3:   # range: Seek / FindChange / BuildIndex + Show on a clip of up to 300 frames
            info = []
            try:
                tag, n = drive_range(rng, info)
            except AssertionError as e:
                print("BAD", "range", " ".join(info), e, flush=True)
                bad += 1
                if bad >= 10:
                    return 1
                continue
            print("ok ", "range", tag, flush=True)
            clips += 1
            nframes += n
            continue
        w = int(rng.choice([int(rng.integers(1, 120)) * 4, int(rng.integers(4, 500)), int(rng.integers(100, 481)) * 4]))
        h = int(rng.choice([int(rng.integers(1, 70)) * 4, int(rng.integers(4, 300)), int(rng.integers(60, 271)) * 4]))   # up to 1920x1080: dozens of 16 KiB tiles per frame
        bits = int(rng.choice([16, 8]))
        n = int(rng.integers(2, 12))
        p_mix = sg.msv1_p_mix(float(rng.choice([0.0, 0.3, 0.7, 0.95, 1.0])), float(rng.choice([1.5, 8.0, 40.0, 300.0])))
        key_every = int(rng.choice([0, 1, 3, 5]))
        cfg = int(rng.integers(0, 1 << 30))
        frames, keys, pal = sg.msv1_clip(cfg, w, h, n, bits=bits, p_mix=None if key_every == 1 else p_mix, key_every=key_every)
        frames = list(frames)
        for i in range(1, n):                       # mutate some frames (never frame 0: later frames need a previous one)
            r = rng.random()
            b = bytearray(frames[i])
            if r < 0.10 and b:
                b = b[: int(rng.integers(0, len(b)))]
            elif r < 0.20 and b:
                b[int(rng.integers(0, len(b)))] = int(rng.integers(0, 256))
            elif r < 0.25:
                b = bytearray(rng.integers(0, 256, size=int(rng.integers(0, 200)), dtype=np.uint8).tobytes())
            elif r < 0.30:
                b = b + b"\x07"
            frames[i] = bytes(b)
        mode = str(rng.choice(["host", "gpu", "gpu", "async", "staged"]))   # async: jsp_decompress_*_async / jsp_wait with the on-GPU parse; staged: the whole clip as ONE batch, replayed
        host_buffers, misalign = rng.random() < 0.15, rng.random() < 0.15
        lines = int(rng.integers(0, 60))
        depth = int(rng.choice([1, 2, 4, 8]))
        form = str(rng.choice(["one_launch_dma", "one_launch", "two_launches"]))   # how the asynchronous path runs a frame
        tag = f"{w}x{h} {bits}bit n={n} key_every={key_every} parse={mode} host={host_buffers} misalign={misalign} lines={lines} cfg={cfg}" + (f" depth={depth} form={form}" if mode == "async" else "")
        try:
            if mode == "async":
                import test_async_gpu as A
                from jsplayer_amd import MSVideo1_16bit, MSVideo1_8bit
                gpu = MSVideo1_16bit(w, h) if bits == 16 else MSVideo1_8bit(w, h, pal)
                gpu.set_option("msv1_parse", "gpu")
                gpu.set_option("msv1_async", form)
                # (a third of the asynchronous clips: the arena goes up in ranges of a few frames ahead of them, jsp_prefetch — some ranges
                # stop short of their last frame, and halfway every range is given up once)
                ranges = int(rng.integers(1, 5)) if rng.random() < 0.33 else 0
                A.drive(gpu, OracleMSVideo1(bits, w, h, pal), w, h, frames, keys, depth=depth, pinned=bool(ranges) or bool(rng.random() < 0.5), lines=lines,
                        prefetch=ranges, drop_ranges_at=(n // 2 if ranges and rng.random() < 0.5 else None))
            elif mode == "staged":
                opts = dict(msv1_parse_ahead=str(rng.choice(["on", "off"])), msv1_scrub_tables="1")
                tag += " " + " ".join(f"{k}={v}" for k, v in opts.items())
                drive_staged(T, bits, w, h, frames, keys, pal, lines, int(rng.integers(2, 6)), int(rng.integers(1, 4)), opts)
            else:
                drive(T, bits, w, h, frames, keys, pal, lines, mode, host_buffers, misalign)
        except AssertionError as e:
            print("BAD", tag, e, flush=True)
            bad += 1
            if bad >= 10:
                return 1
            continue
        print("ok ", tag, flush=True)
        clips += 1
        nframes += n
    print(f"fuzz finished: {clips} clips, {nframes} frames, {bad} BAD, {time.time() - t0:.0f} s, seed {seed}")
    return 1 if bad else 0


def drive(T, bits, w, h, frames, keys, pal, lines, mode, host_buffers, misalign):
    """test_msvideo1_gpu.drive_pair with the parse mode its make_gpu() applies."""
    T.PARSE_MODE = mode
    T.drive_pair(bits, w, h, frames, keys, pal, lines=lines, host=host_buffers, misalign=misalign and not host_buffers)


def drive_staged(T, bits, w, h, frames, keys, pal, lines, nbuf, replays, opts):
    """The clip as ONE staged batch into `nbuf` rotating buffers, decoded and replayed `replays` times back to back (round 6: the next replay's
    parse beside this one, tables poisoned before every parse) — mutated, truncated and random frames included, so that
    frames the host parser has to settle sit between the GPU-parsed ones.  Statuses, adoption, significance and every buffer against the oracle."""
    from jsplayer_amd import MSVideo1_16bit, MSVideo1_8bit
    from oracle_binding import OracleAbort, OracleMSVideo1
    n = len(frames)
    orc = OracleMSVideo1(bits, w, h, pal)
    orc.Preinit(lines)
    obufs = [np.full(w * h, 5, dtype=np.int32) for _ in range(nbuf)]
    want, where = [], []                        # per frame: None (the reference raises) or (adopted, significant or None for a key frame); the buffer it goes to
    for i in range(n):
        k = next(j for j in range(nbuf) if obufs[j] is not orc.PreviousFrame())   # the Manager's rule: any buffer but the previous frame's
        where.append(k)
        if keys[i]:
            assert orc.DecompressI(frames[i], obufs[k]) == 0
            want.append((True, None))
        else:
            try:
                data, sig = orc.DecompressP(frames[i], obufs[k])
                want.append((data is obufs[k], sig))
            except OracleAbort:
                want.append(None)
    gpu = MSVideo1_16bit(w, h) if bits == 16 else MSVideo1_8bit(w, h, pal)
    gpu.Preinit(lines)
    gpu.set_option("msv1_parse", "gpu")
    for k, v in opts.items():
        gpu.set_option(k, v)
    dsts = [T.dev_buf(w * h, 5) for _ in range(nbuf)]
    st = gpu.stage_batch(frames, [dsts[where[i]] for i in range(n)], is_key=keys)
    for run in range(2):
        for d in dsts:
            d.fill_(5)
        for _ in range(replays if run else 1):
            st.decode()
        gpu.sync()
        status, adopted, signif = st.results()
        for i in range(n):
            if want[i] is None:
                assert status[i] != 0, f"run {run} frame {i}: the reference raises here"
                continue
            assert status[i] == 0, f"run {run} frame {i}: status {status[i]}"
            if not keys[i]:
                assert bool(adopted[i]) == want[i][0], f"run {run} frame {i}: adoption"
                assert bool(signif[i]) == want[i][1], f"run {run} frame {i}: significant_changes"
        if all(x is not None for x in want):    # (a frame at which the reference raises leaves the later ones undefined there)
            for k in range(nbuf):
                assert np.array_equal(obufs[k], T.to_np(dsts[k])), f"run {run}: buffer {k} differs"
    st.close()
    gpu.StopAndClean()


def range_clip(rng, bits, w, h, n):
    """A long_clip schedule, or a generated clip with mutated, truncated and random frames; sometimes opening with frames that
    adopt nothing and a skip code with no picture before it (the reference raises there)."""
    import msv1_range_clips as R
    from jsplayer_amd import streamgen as sg
    if n >= 96 and rng.random() < 0.5:
        frames, keys, pal, plan = R.long_clip(bits, w, h, int(rng.integers(0, 1 << 30)), n=n)
        return list(frames), list(keys), pal, plan["lines"]
    p_mix = sg.msv1_p_mix(float(rng.choice([0.3, 0.7, 0.95])), float(rng.choice([1.5, 8.0, 40.0])))
    frames, keys, pal = sg.msv1_clip(int(rng.integers(0, 1 << 30)), w, h, n, bits=bits, p_mix=p_mix, key_every=int(rng.choice([0, 5, 40, 97])))
    frames, keys = list(frames), list(keys)
    for i in range(1, n):
        r, b = rng.random(), bytearray(frames[i])
        if r < 0.05 and b:
            b = b[: int(rng.integers(0, len(b)))]
        elif r < 0.08:
            b = bytearray(rng.integers(0, 256, size=int(rng.integers(0, 200)), dtype=np.uint8).tobytes())
        elif r < 0.10:
            b = b + b"\x07"
        frames[i] = bytes(b)
    if rng.random() < 0.15:
        lead = int(rng.integers(0, min(3, n - 1)))
        for i in range(lead):   # nothing coded: an all-skip 16-bit early-out, an 8-bit end marker on the first block
            frames[i], keys[i] = (b"" if bits == 16 else b"\x00\x00"), False
        frames[lead], keys[lead] = bytes([0x01, 0x84]) + frames[lead], False
    return frames, keys, pal, int(rng.integers(0, 60))


def drive_range(rng, info):
    """One clip, random range queries against the oracle's frame-by-frame run (msv1_range_clips.truth_run): Seek from the nearest
    key frame, FindChange from a shown frame, BuildIndex then every Show and one adopting Show played on.  A range that reaches a
    frame the oracle raises on must raise naming it and leave no previous frame."""
    import msv1_range_clips as R
    from jsplayer_amd import CodecError, player
    bits = int(rng.choice([16, 8]))
    w = int(rng.choice([int(rng.integers(1, 17)) * 4, int(rng.integers(4, 70))]))
    h = int(rng.choice([int(rng.integers(1, 13)) * 4, int(rng.integers(4, 50))]))
    n = int(rng.integers(2, 301))
    frames, keys, pal, lines = range_clip(rng, bits, w, h, n)
    chunk = rng.choice([None, None, 1, 3, 5, 7, 31, 32, 33, int(rng.integers(1, 80))])
    chunk = None if chunk is None else int(chunk)
    parse = str(rng.choice(["host", "gpu"]))
    tag = f"{w}x{h} {bits}bit n={n} chunk={chunk} parse={parse} lines={lines}"
    info.append(tag)
    truth = R.truth_run(bits, w, h, pal, frames, keys, lines, key_row=lines)
    raise_at = next((i for i, x in enumerate(truth) if x is None), n)
    coded = R.make_plan(bits, w, h, frames[:raise_at], keys[:raise_at], lines)["coded"].any(axis=1) if raise_at else np.zeros(0, bool)

    def fresh(upto):
        g = R.make_gpu(bits, w, h, pal, lines, chunk, parse)
        pool = [R.dev_buf(w * h) for _ in range(3)]
        for i in range(upto):
            d = next(b for b in pool if b is not g.PreviousFrame())
            if g.PreviousFrame() is not None:   # (as truth_run: each destination starts as the picture before it)
                d.copy_(g.PreviousFrame())
            if keys[i]:
                assert g.DecompressI(frames[i], d) == 0
            else:
                g.DecompressP(frames[i], d)
        return g, pool

    def raised(call, k):
        try:
            call()
        except CodecError as e:
            assert f"frame {k} " in str(e) or str(e).endswith(f"frame {k}"), f"error names another frame: {e}"
            return
        raise AssertionError(f"no error for the frame the oracle raises on ({k} of the range)")

    # Seek
    t = int(rng.integers(0, n))
    s = player.nearest_key_frame(keys, t)
    if s <= raise_at:
        g, pool = fresh(s)
        old, dst = g.PreviousFrame(), R.dev_buf(w * h, misalign=bool(rng.random() < 0.2))
        if t >= raise_at:
            raised(lambda: g.Seek(frames[s:t + 1], dst, keys[s:t + 1]), raise_at - s)
            assert g.PreviousFrame() is None, "seek: previous frame after the raise"
        else:
            r = g.Seek(frames[s:t + 1], dst, keys[s:t + 1])
            if coded[s:t + 1].any():
                assert r.data_pnt is dst and np.array_equal(dst.cpu().numpy(), truth[t][0]), f"seek {s}..{t}: picture"
            else:
                assert r.data_pnt is old, f"seek {s}..{t}: data_pnt"
            assert r.significant_changes == (False if keys[t] else truth[t][1]), f"seek {s}..{t}: significance"
        g.StopAndClean()
    # FindChange from a shown frame
    if raise_at > 1:
        k = int(rng.integers(0, min(raise_at, n - 1)))
        g, pool = fresh(k + 1)
        dst = next(b for b in pool if b is not g.PreviousFrame())
        want = R.expected_landing(truth, k + 1)
        kb = frames[k] if keys[k] else None
        call = lambda: g.FindChange(frames[k + 1:], dst, keys[k + 1:], 0, kb, lines)
        if want is None:
            raised(call, raise_at - k - 1)
            assert g.PreviousFrame() is None, "find_change: previous frame after the raise"
        else:
            res = call()
            f = k + 1 + res.index
            assert f == want, f"find_change from {k}: landed on {f}, the oracle on {want}"
            assert res.changed == truth[f][1]
            assert res.significance == [truth[j][1] if j <= f else None for j in range(k + 1, n)], f"find_change from {k}: significance"
            if g.PreviousFrame() is not None:
                assert np.array_equal(g.PreviousFrame().cpu().numpy(), truth[f][0]), f"find_change from {k}: picture"
        g.StopAndClean()
    # BuildIndex, every Show, one adopting Show played on
    start = int(rng.integers(0, max(1, min(raise_at, n))))
    g, pool = fresh(start)
    old = g.PreviousFrame()
    if raise_at < n:
        raised(lambda: g.BuildIndex(frames[start:], keys[start:], key_row=lines), raise_at - start)
        assert g.PreviousFrame() is old, "index: the codec changed on a refused build"
        g.StopAndClean()
        return tag + " raises at %d" % raise_at, n
    idx = g.BuildIndex(frames[start:], keys[start:], key_row=lines)
    for j in range(start, n):
        if j > start or not (keys[j] and j > 0 and keys[j - 1]):   # (the range's first key frame is judged by its pixels)
            assert idx.significance[j - start] == truth[j][1], f"index from {start}: significance of {j}"
    dst = R.dev_buf(w * h)
    for j in range(start, n):
        dst.fill_(R.POISON)
        r = idx.Show(j - start, dst, adopt=False)
        if coded[start:j + 1].any():
            assert r.data_pnt is dst and np.array_equal(dst.cpu().numpy(), truth[j][0]), f"index from {start}: show {j}"
        else:
            assert r.data_pnt is old, f"index from {start}: show {j} data_pnt"
    j = int(rng.integers(start, n))
    d = next(b for b in pool if b is not g.PreviousFrame())
    idx.Show(j - start, d, adopt=True)
    cx, cy = (w // 4) * 4, (h // 4) * 4
    for i in range(j + 1, min(n, j + 4)):
        d = next(b for b in pool if b is not g.PreviousFrame())
        if g.PreviousFrame() is not None:
            d.copy_(g.PreviousFrame())
        if keys[i]:
            assert g.DecompressI(frames[i], d) == 0
        else:
            assert g.DecompressP(frames[i], d).significant_changes == truth[i][1], f"play on from show {j}: frame {i} significance"
        if g.PreviousFrame() is not None:
            got = g.PreviousFrame().cpu().numpy().reshape(h, w)[:cy, :cx]
            assert np.array_equal(got, truth[i][0].reshape(h, w)[:cy, :cx]), f"play on from show {j}: frame {i}"
    idx.close()
    g.StopAndClean()
    return tag, n


if __name__ == "__main__":
    sys.exit(main())
