"""Scrubbing latency with the ScreenPressor seek index (jsp_sp_index_build / jsp_sp_index_show) on clip 0 of
screenpressor_v4_1080p_pclip300 (ONE key frame, 299 inter frames, 1080p):

  build       BuildScrubIndex over the whole clip (host entropy stage once, records up, key pictures, verdicts), and what stays in
              HBM: tables, literal payload, bitmap, key pictures;
  show        Show(t) of ONE frame at distance t from the key frame, against
  fallback    what the Manager falls back to for the same click without an index: DecompressI + t x DecompressP from the key frame,
  staged      and against the fastest existing way, host stage included: frames 0..t staged as one batch into a scratch pool
              (stage_batch + decode), for t in {1, 16, 64, 150, 299};
  step back   299 -> 284, one Show per step against one fallback per step (sixteen steps; the fallback's full walk back through the
              clip is minutes and is EXTRAPOLATED from the per-frame cost of the sixteen: said so in the output);

each measured with a host clock around a call that ends synchronised, in one process, the forms alternating, medians of --reps.
Every timed picture is first checked against the golden digests of the sequential decode.  Prints one JSON line per measurement.

  --volumes   no GPU needed: from the host stage's tables (tests/hoststage_binding.py), the bytes the show kernel must read for
              frame t — bitmap words walked, records and literals of the last writers, the key picture — and what a forward walk
              (every record of k + 1 .. t) would read instead.
  --kernel-only T   just a few Show(T) calls: the program to put behind `rocprofv3 --kernel-trace --stats --`.

    python tools/sp_scrub_latency.py [--reps 5] [--distances 1,16,64,150,299] [--out profiles/sp_scrub_latency.json]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NAME = "screenpressor_v4_1080p_pclip300"


def read_volumes(frames, keys, targets):
    """Per target frame t: what the backward walk of sp_index_show_kernel reads, simulated per pixel from the literalised tables,
    and what the forward form would read.  Host stage only."""
    import numpy as np
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import hoststage_binding as hb
    from jsplayer_amd import workloads as wl
    w, h = wl.W, wl.H
    nbx, nby = (w + 15) // 16, (h + 15) // 16
    nb = nbx * nby
    hs = hb.HostStage(w, h, 24)
    hs.preinit(36)
    rects, lit_words = {}, {}
    last = max(targets)
    for t in range(last + 1):
        d = hs.decode(bool(keys[t]), frames[t])
        assert d["status"] == 0, (t, d["error"])
        if d["kind"] != hb.KIND_INTER:
            continue
        d = hs.literalise_motion(d)
        b = d["blocks"]
        rects[t] = (b[:, 0] != 0, b[:, 1].astype(np.int16), b[:, 2].astype(np.int16), b[:, 3].astype(np.int16), b[:, 4].astype(np.int16))
        lit_words[t] = int(d["payload"].size)
    hs.close()
    px = np.arange(16, dtype=np.int16)
    out = []
    for t in targets:
        k = max(i for i in range(t + 1) if keys[i])
        uncovered = np.ones((nb, 16, 16), bool)
        by, bx = np.divmod(np.arange(nb), nbx)
        uncovered &= ((by[:, None] * 16 + px[None, :]) < h)[:, :, None] & ((bx[:, None] * 16 + px[None, :]) < w)[:, None, :]
        records = literals = 0
        words = np.zeros(nb, np.int64)
        is_open = np.ones(nb, bool)
        for wd in range(t >> 5, ((k + 1) >> 5) - 1, -1):
            if t == k:
                break
            words += is_open                                   # a wave still walking reads this word of its block
            for f in range(min(t, wd * 32 + 31), max(k, wd * 32 - 1), -1):
                if f not in rects:
                    continue
                ch, x1, y1, x2, y2 = rects[f]
                visit = ch & is_open
                if not visit.any():
                    continue
                rect = ((px[None, :] >= y1[:, None]) & (px[None, :] < y2[:, None]))[:, :, None] & \
                       ((px[None, :] >= x1[:, None]) & (px[None, :] < x2[:, None]))[:, None, :]
                take = rect & uncovered & visit[:, None, None]
                records += int(visit.sum())
                literals += int(take.sum())
                uncovered &= ~take
                is_open = uncovered.any(axis=(1, 2))
        picture = w * h * 4
        backward = dict(bitmap_bytes=int(words.sum()) * 4, record_bytes=records * 16, literal_bytes=literals * 4, key_picture_bytes=picture)
        backward["read_bytes"] = sum(backward.values())
        forward = dict(record_bytes=sum(1 for f in rects if k < f <= t) * nb * 16,
                       literal_bytes=sum(4 * lit_words[f] for f in rects if k < f <= t), key_picture_bytes=picture)
        forward["read_bytes"] = sum(forward.values())
        out.append(dict(frame=t, key_frame=k, written_bytes=picture, backward=backward, forward=forward))
    return out


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--distances", default="1,16,64,150,299")
    ap.add_argument("--volumes", action="store_true")
    ap.add_argument("--kernel-only", type=int, default=-1)
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    from jsplayer_amd import workloads as wl
    clip = wl.build_clips(NAME)[0]
    frames, keys = clip.frames, clip.keys
    nf = len(frames)
    distances = [min(int(d), nf - 1) for d in args.distances.split(",")]
    lines = []

    def say(rec):
        lines.append(rec)
        print(json.dumps(rec), flush=True)

    if args.volumes:
        for rec in read_volumes(frames, keys, distances):
            say(rec)
        if args.out:
            with open(args.out, "w") as f:
                json.dump(lines, f, indent=1)
        return 0

    import torch
    if not torch.cuda.is_available():
        print("sp_scrub_latency: no GPU", file=sys.stderr)
        return 2
    n = wl.W * wl.H
    want = list(wl.golden_digests(NAME, 0)[0])
    for t in range(1, nf):
        if want[t] == "-":
            want[t] = want[t - 1]

    shower = wl.make_codec(NAME)
    dst = [torch.zeros(n, dtype=torch.int32, device="cuda") for _ in range(2)]

    def build():
        t0 = time.perf_counter()
        idx = shower.BuildScrubIndex(frames, keys)
        return (time.perf_counter() - t0) * 1e3, idx

    def show(idx, t):
        d = dst[t & 1]
        t0 = time.perf_counter()
        idx.Show(t, d)                       # (returns synchronised)
        return (time.perf_counter() - t0) * 1e3, d

    if args.kernel_only >= 0:
        _, idx = build()
        for _ in range(20):
            show(idx, args.kernel_only)
        ok = wl.digest(dst[args.kernel_only & 1].cpu().numpy()) == want[args.kernel_only]
        say({"kernel_only": args.kernel_only, "digest_matches": ok})
        idx.close()
        shower.StopAndClean()
        return 0 if ok else 1

    seq_bufs = [torch.zeros(n, dtype=torch.int32, device="cuda") for _ in range(3)]
    pool = torch.zeros(nf * n, dtype=torch.int32, device="cuda")
    pool_frames = [pool[i * n:(i + 1) * n] for i in range(nf)]

    def fallback(t):
        """The Manager's seek branch without an index: a decoder restarted at the key frame, frame by frame up to t."""
        c = wl.make_codec(NAME)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(t + 1):
            d = next(b for b in seq_bufs if b is not c.PreviousFrame())
            if keys[i]:
                c.DecompressI(frames[i], d)
            else:
                c.DecompressP(frames[i], d)
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3
        pic = c.PreviousFrame()
        c.StopAndClean()
        return ms, pic

    def staged(t):
        c = wl.make_codec(NAME)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        st = c.stage_batch(frames[:t + 1], pool_frames[:t + 1], is_key=keys[:t + 1])
        st.decode()
        c.sync()
        ms = (time.perf_counter() - t0) * 1e3
        pic = c.PreviousFrame()
        st.close()
        c.StopAndClean()
        return ms, pic

    ok_all = True
    _, idx = build()                          # warm-up
    idx.close()
    builds = []
    for r in range(args.reps):
        ms, idx = build()
        builds.append(ms)
        if r + 1 < args.reps:
            idx.close()
    nblocks = ((wl.W + 15) // 16) * ((wl.H + 15) // 16)
    nkeys = sum(1 for k in keys if k)
    tables = (nf - nkeys) * nblocks * 16
    bitmap = ((nf + 31) // 32) * nblocks * 4
    key_pics = nkeys * ((n + 3) & ~3) * 4
    say({"frames": nf, "build_ms": round(statistics.median(builds), 2), "build_ms_min": round(min(builds), 2),
         "device_bytes": idx.device_bytes, "host_bytes": idx.host_bytes, "table_bytes": tables, "bitmap_bytes": bitmap,
         "key_picture_bytes": key_pics, "payload_bytes": idx.device_bytes - tables - bitmap - key_pics})

    for t in distances:
        times = {"show": [], "fallback": [], "staged": []}
        ok = True
        for _ in range(args.reps):
            for form, fn in (("show", lambda: show(idx, t)), ("fallback", lambda: fallback(t)), ("staged", lambda: staged(t))):
                ms, pic = fn()
                times[form].append(ms)
                ok &= wl.digest(pic.cpu().numpy()) == want[t]
        ok_all &= ok
        say({"frame": t, **{f"{m}_ms": round(statistics.median(v), 4) for m, v in times.items()},
             **{f"{m}_ms_min": round(min(v), 4) for m, v in times.items()}, "digests_match": ok})

    steps = list(range(nf - 1, nf - 17, -1))
    back = {"show": [], "fallback": []}
    ok = True
    for _ in range(args.reps):
        total = 0.0
        for t in steps:
            ms, pic = show(idx, t)
            total += ms
            ok &= wl.digest(pic.cpu().numpy()) == want[t]
        back["show"].append(total)
        total = 0.0
        for t in steps:
            ms, pic = fallback(t)
            total += ms
            ok &= wl.digest(pic.cpu().numpy()) == want[t]
        back["fallback"].append(total)
    ok_all &= ok
    fb = statistics.median(back["fallback"])
    per_frame = fb / sum(t + 1 for t in steps)            # the fallback's cost per frame it decodes
    say({"step_back_from": steps[0], "step_back_to": steps[-1], "steps": len(steps),
         "show_total_ms": round(statistics.median(back["show"]), 3), "fallback_total_ms": round(fb, 1),
         "fallback_ms_per_decoded_frame": round(per_frame, 3),
         "fallback_full_walk_ms_EXTRAPOLATED": round(per_frame * nf * (nf + 1) / 2, 0),
         "show_full_walk_ms_EXTRAPOLATED": round(statistics.median(back["show"]) / len(steps) * nf, 1), "digests_match": ok})
    say({"reps": args.reps, "device": torch.cuda.get_device_name(0), "all_digests_match": ok_all})
    idx.close()
    shower.StopAndClean()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(lines, f, indent=1)
    return 0 if ok_all else 1


if __name__ == "__main__":
    sys.exit(main())
