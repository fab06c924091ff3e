"""Scrubbing latency with a seek index (jsp_index_build / jsp_index_show) on two 512-frame 1080p clips, 16-bit MSVideo1:
msvideo1_16_1080p_inter70 (frame 0 key, 70 % of the blocks skipped per frame) and the idle clip of tools/skip_stills_latency.py
(a key frame, 502 idle frames, a change, 8 idle frames).  Per clip:

  build       BuildIndex over the whole clip (staging, judging every frame, the coded-block bitmap);
  show        Show(t) of ONE frame at distance t from the key frame, against
  seek        Seek(frames[0..t]) to the same frame (jsp_seek: the range staged again, one launch), for t in {1, 16, 64, 256, 511};
  step back   every frame from the last down to 0, one Show(adopt=True) per step, against one Seek per step (Main.on_prevframe
              in the reference restarts at the key frame every time);

each measured with a host clock around a call that ends synchronised, in one process, the forms alternating.  Every picture
shown — every frame of the step back included — must equal the digest of a sequential decode.  Prints one JSON line per
measurement and a summary.

    python tools/scrub_latency.py [--reps 5] [--parse gpu|host] [--clips inter70,idle]
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
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--parse", default="gpu", choices=["gpu", "host"])
    ap.add_argument("--clips", default="inter70,idle")
    ap.add_argument("--distances", default="1,16,64,256,511")
    args = ap.parse_args()

    import torch
    from jsplayer_amd import MSVideo1_16bit, player
    from jsplayer_amd import workloads as wl
    from skip_stills_latency import idle_clip

    n = wl.W * wl.H
    distances = [int(d) for d in args.distances.split(",")]

    def codec():
        c = MSVideo1_16bit(wl.W, wl.H)
        c.set_option("msv1_parse", args.parse)
        c.Preinit(player.INSIGNIFICANT_LINES)
        return c

    def clips():
        for name in args.clips.split(","):
            if name == "inter70":
                c = wl.build_clips("msvideo1_16_1080p_inter70")[0]
                yield name, c.frames, c.keys
            else:
                frames, keys = idle_clip(502)
                yield name, frames, keys

    ok_all = True
    for name, frames, keys in clips():
        nf = len(frames)
        # the truth: a sequential decode, every frame's digest
        seq = codec()
        bufs = [torch.zeros(n, dtype=torch.int32, device="cuda") for _ in range(3)]
        want = []
        for i, f in enumerate(frames):
            dst = next(b for b in bufs if b is not seq.PreviousFrame())
            if keys[i]:
                seq.DecompressI(f, dst)
            else:
                seq.DecompressP(f, dst)
            want.append(wl.digest(seq.PreviousFrame().cpu().numpy()))
        seq.StopAndClean()

        shower, seeker = codec(), codec()
        show_bufs = [torch.zeros(n, dtype=torch.int32, device="cuda") for _ in range(2)]
        seek_bufs = [torch.zeros(n, dtype=torch.int32, device="cuda") for _ in range(2)]

        def build():
            t0 = time.perf_counter()
            idx = shower.BuildIndex(frames, keys)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3, idx

        def show(idx, t, adopt=False):
            dst = next(b for b in show_bufs if b is not shower.PreviousFrame())
            t0 = time.perf_counter()
            r = idx.Show(t, dst, adopt=adopt)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3, r.data_pnt

        def seek(t):
            k = player.nearest_key_frame(keys, t)
            dst = next(b for b in seek_bufs if b is not seeker.PreviousFrame())
            t0 = time.perf_counter()
            r = seeker.Seek(frames[k:t + 1], dst, keys[k:t + 1])
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3, r.data_pnt

        # warm-up: the seek's staging buffers at their largest, one build
        seek(nf - 1)
        build_ms, idx = build()
        idx.close()
        builds = []
        for _ in range(args.reps):
            ms, idx = build()
            builds.append(ms)
            if len(builds) < args.reps:
                idx.close()
        print(json.dumps({"clip": name, "frames": nf, "build_ms": round(statistics.median(builds), 3), "build_ms_min": round(min(builds), 3),
                          "index_device_bytes": idx.device_bytes, "index_host_bytes": idx.host_bytes}), flush=True)

        for d in distances:
            t = min(d, nf - 1)
            times = {"show": [], "seek": []}
            ok = True
            for _ in range(args.reps):
                ms, pic = show(idx, t)
                times["show"].append(ms)
                ok &= wl.digest(pic.cpu().numpy()) == want[t]
                ms, pic = seek(t)
                times["seek"].append(ms)
                ok &= wl.digest(pic.cpu().numpy()) == want[t]
            ok_all &= ok
            print(json.dumps({"clip": name, "frame": t, **{f"{m}_ms": round(statistics.median(v), 4) for m, v in times.items()},
                              **{f"{m}_ms_min": round(min(v), 4) for m, v in times.items()}, "digests_match": ok}), flush=True)

        # the step back: timed passes (no download inside), then one pass checking every frame's digest
        back = {"show": [], "seek": []}
        for _ in range(max(1, args.reps // 2)):
            total = 0.0
            for t in range(nf - 1, -1, -1):
                total += show(idx, t, adopt=True)[0]
            back["show"].append(total)
            total = 0.0
            for t in range(nf - 1, -1, -1):
                total += seek(t)[0]
            back["seek"].append(total)
        ok = True
        for t in range(nf - 1, -1, -1):
            ok &= wl.digest(show(idx, t, adopt=True)[1].cpu().numpy()) == want[t]
        ok_all &= ok
        print(json.dumps({"clip": name, "step_back_frames": nf, **{f"{m}_total_ms": round(statistics.median(v), 2) for m, v in back.items()},
                          "show_per_step_ms": round(statistics.median(back["show"]) / nf, 4),
                          "seek_per_step_ms": round(statistics.median(back["seek"]) / nf, 4), "digests_match": ok}), flush=True)
        idx.close()
        shower.StopAndClean()
        seeker.StopAndClean()
    print(json.dumps({"parse": args.parse, "reps": args.reps, "device": torch.cuda.get_device_name(0), "all_digests_match": ok_all}), flush=True)
    return 0 if ok_all else 1


if __name__ == "__main__":
    sys.exit(main())
