"""Seek latency on the msvideo1_16_1080p_inter70 workload (512 frames at 1080p, frame 0 key, 70 % of the blocks skipped):
the wall time of reaching frame N from frame 0 by

  seek        ONE Seek call (jsp_seek: the range staged as one batch, one launch writes the picture);
  sequential  per-frame DecompressI / DecompressP calls into a three-buffer pool;
  pipelined   Manager.play_pipelined with 4 frames in flight;

each measured with a host clock around a call that ends synchronised, in one process, the three alternating, for N in
{1, 16, 64, 256, 511}.  The sought picture's digest must equal the sequential one.  Prints one JSON line per N and a summary.

    python tools/seek_latency.py [--reps 5] [--targets 1,16,64,256,511]
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


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--targets", default="1,16,64,256,511")
    ap.add_argument("--parse", default="gpu", choices=["gpu", "host"])
    args = ap.parse_args()

    import torch
    from jsplayer_amd import player
    from jsplayer_amd import workloads as wl
    from jsplayer_amd.avi import CODEC_MSVC16, VideoInfo

    name = "msvideo1_16_1080p_inter70"
    clip = wl.build_clips(name)[0]
    frames, keys = clip.frames, clip.keys
    n = wl.W * wl.H
    targets = [int(t) for t in args.targets.split(",")]
    opts = {"msv1_parse": args.parse}

    seeker = wl.make_codec(name, options=opts)
    seek_bufs = [torch.zeros(n, dtype=torch.int32, device="cuda") for _ in range(2)]
    seq = wl.make_codec(name, options=opts)
    seq_bufs = [torch.zeros(n, dtype=torch.int32, device="cuda") for _ in range(3)]
    vi = VideoInfo(X=wl.W, Y=wl.H, bpp=16, fps=15.0, nframes=len(frames), codec=CODEC_MSVC16, palette=None, riff_size=0)
    pipe_dec = wl.make_codec(name, options=opts)
    mgr = player.Manager(vi, pipe_dec, lambda k: torch.zeros(k, dtype=torch.int32, device="cuda"), num_buffers=player.NUM_BUFFERS + 4)

    def run_seek(t):
        dst = next(b for b in seek_bufs if b is not seeker.PreviousFrame())
        t0 = time.perf_counter()
        res = seeker.Seek(frames[:t + 1], dst, keys[:t + 1])
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3
        return ms, res.data_pnt

    def run_sequential(t):
        t0 = time.perf_counter()
        for i in range(t + 1):
            dst = next(b for b in seq_bufs if b is not seq.PreviousFrame())
            if keys[i]:
                seq.DecompressI(frames[i], dst)
            else:
                seq.DecompressP(frames[i], dst)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, seq.PreviousFrame()

    def run_pipelined(t):
        mgr.holds = [None] * len(mgr.buffers)
        mgr.log = []
        t0 = time.perf_counter()
        log = mgr.play_pipelined(frames[:t + 1], depth=4, key_flags=keys[:t + 1])
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, mgr.buffers[log[-1].buffer_index]

    # warm-up: every path's buffers reach their size (the seek's staging buffers for the longest range)
    run_seek(max(targets))
    run_sequential(16)
    run_pipelined(16)

    rows = []
    for t in targets:
        times = {"seek": [], "sequential": [], "pipelined": []}
        digests = {}
        for _ in range(args.reps):
            for mode, fn in (("seek", run_seek), ("sequential", run_sequential), ("pipelined", run_pipelined)):
                ms, pic = fn(t)
                times[mode].append(ms)
                digests.setdefault(mode, set()).add(wl.digest(pic.cpu().numpy()))
        ok = len(digests["seek"]) == 1 and digests["seek"] == digests["sequential"] == digests["pipelined"]
        row = {"target": t, "frames_in_range": t + 1, "range_stream_bytes": sum(len(f) for f in frames[:t + 1]),
               **{f"{m}_ms": round(statistics.median(v), 3) for m, v in times.items()},
               **{f"{m}_ms_min": round(min(v), 3) for m, v in times.items()},
               "digest": sorted(digests["seek"])[0], "digest_matches_sequential": ok}
        rows.append(row)
        print(json.dumps(row), flush=True)
    print(json.dumps({"workload": name, "parse": args.parse, "reps": args.reps, "device": torch.cuda.get_device_name(0),
                      "all_digests_match": all(r["digest_matches_sequential"] for r in rows)}), flush=True)
    for c in (seeker, seq, pipe_dec):
        c.StopAndClean()
    return 0 if all(r["digest_matches_sequential"] for r in rows) else 1


if __name__ == "__main__":
    sys.exit(main())
