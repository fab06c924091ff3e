"""Filmstrip latency with a seek index (jsp_index_thumbs) on the two 512-frame 1080p clips of tools/scrub_latency.py, 16-bit
MSVideo1: msvideo1_16_1080p_inter70 and the idle clip of tools/skip_stills_latency.py.  One index over the whole clip, then
n frames spread evenly over it (frame (k * frames) // n), at each scale s:

  A   ONE Thumbs(frames, s) call: n thumbnails in one launch;
  B   what a caller can do without it: n x Show(t, scratch, adopt=False) — full-size pictures, NO downscale at all, so B is a
      lower bound of that path;
  C   B plus a torch downscale (the same box mean) of each scratch frame into the sheet — informative only;

and one hover-preview row: Thumbs([t], s) against one Show(t).  Each form is measured with a host clock around calls that end
synchronised, in one process, the forms alternating, medians of --reps.  Before anything is timed every result is checked: the
pictures Show writes against the digests of a sequential decode, the sheet of A against the sheet of C (exact).  Prints one JSON
line per measurement and a summary.

    python tools/filmstrip_latency.py [--reps 5] [--parse gpu|host] [--clips inter70,idle] [--n 64] [--scales 4,8,16]
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
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--scales", default="4,8,16")
    args = ap.parse_args()

    import torch
    from jsplayer_amd import MSVideo1_16bit, player
    from jsplayer_amd import workloads as wl
    from skip_stills_latency import idle_clip

    npix = wl.W * wl.H
    scales = [int(s) for s in args.scales.split(",")]

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

    def downscale(pic, s, tw, th, out):
        """The contract's box mean of a full-size picture, in torch: per channel, rounded half up."""
        shift = {4: 4, 8: 6, 16: 8}[s]
        v = pic.view(wl.H, wl.W)[: th * s, : tw * s]
        acc = None
        for pos in (16, 8, 0):
            c = ((v >> pos) & 0xFF).view(th, s, tw, s).sum(dim=(1, 3), dtype=torch.int32)
            c = ((c + (s * s) // 2) >> shift) << pos
            acc = c if acc is None else acc | c
        out.copy_(acc)

    ok_all = True
    for name, frames, keys in clips():
        nf = len(frames)
        picks = [(k * nf) // args.n for k in range(args.n)]
        # the truth for the pictures: a sequential decode, the digests of the frames picked
        seq = codec()
        bufs = [torch.zeros(npix, dtype=torch.int32, device="cuda") for _ in range(3)]
        want = {}
        for i, f in enumerate(frames):
            dst = next(b for b in bufs if b is not seq.PreviousFrame())
            if keys[i]:
                seq.DecompressI(f, dst)
            else:
                seq.DecompressP(f, dst)
            if i in picks:
                want[i] = wl.digest(seq.PreviousFrame().cpu().numpy())
        seq.StopAndClean()

        dec = codec()
        idx = dec.BuildIndex(frames, keys)
        scratch = torch.zeros(npix, dtype=torch.int32, device="cuda")

        def form_a(s, sheet, which):
            t0 = time.perf_counter()
            idx.Thumbs(which, scale=s, cols=1, out=sheet)
            return (time.perf_counter() - t0) * 1e3

        def form_b(which):
            t0 = time.perf_counter()
            for t in which:
                idx.Show(t, scratch, adopt=False)
            return (time.perf_counter() - t0) * 1e3

        def form_c(s, tw, th, sheet, which, check=False):
            cells = sheet.view(len(which), th, tw)
            ok = True
            t0 = time.perf_counter()
            for k, t in enumerate(which):
                idx.Show(t, scratch, adopt=False)
                if check:
                    ok &= wl.digest(scratch.cpu().numpy()) == want[t]
                downscale(scratch, s, tw, th, cells[k])
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3, ok

        for s in scales:
            tw, th = idx.ThumbSize(s)
            sheet_a = torch.zeros(args.n * th * tw, dtype=torch.int32, device="cuda")
            sheet_c = torch.zeros_like(sheet_a)
            # checked before it is timed (and the warm-up of every form)
            _, ok = form_c(s, tw, th, sheet_c, picks, check=True)
            form_a(s, sheet_a, picks)
            ok &= bool(torch.equal(sheet_a, sheet_c))
            form_b(picks)
            ok_all &= ok
            times = {"A": [], "B": [], "C": []}
            for _ in range(args.reps):
                times["A"].append(form_a(s, sheet_a, picks))
                times["B"].append(form_b(picks))
                times["C"].append(form_c(s, tw, th, sheet_c, picks)[0])
            ok &= bool(torch.equal(sheet_a, sheet_c))
            ok_all &= ok
            med = {m: statistics.median(v) for m, v in times.items()}
            print(json.dumps({"clip": name, "n": args.n, "scale": s, "thumb": [tw, th], **{f"{m}_ms": round(v, 4) for m, v in med.items()},
                              **{f"{m}_ms_min": round(min(v), 4) for m, v in times.items()}, "A_over_B": round(med["A"] / med["B"], 4),
                              "A_over_C": round(med["A"] / med["C"], 4), "A_faster_than_B": med["A"] < med["B"], "results_match": ok}), flush=True)

        # the hover preview: one thumbnail against one Show
        s, t = 8, picks[len(picks) // 2]
        tw, th = idx.ThumbSize(s)
        one_a = torch.zeros(th * tw, dtype=torch.int32, device="cuda")
        one_c = torch.zeros_like(one_a)
        _, ok = form_c(s, tw, th, one_c, [t], check=True)
        form_a(s, one_a, [t])
        ok &= bool(torch.equal(one_a, one_c))
        ok_all &= ok
        times = {"A": [], "B": []}
        for _ in range(args.reps):
            times["A"].append(form_a(s, one_a, [t]))
            times["B"].append(form_b([t]))
        print(json.dumps({"clip": name, "n": 1, "scale": s, "frame": t, "A_ms": round(statistics.median(times["A"]), 4),
                          "B_ms": round(statistics.median(times["B"]), 4), "A_ms_min": round(min(times["A"]), 4),
                          "B_ms_min": round(min(times["B"]), 4), "results_match": ok}), flush=True)
        idx.close()
        dec.StopAndClean()
    print(json.dumps({"parse": args.parse, "reps": args.reps, "device": torch.cuda.get_device_name(0), "all_results_match": ok_all}), flush=True)
    return 0 if ok_all else 1


if __name__ == "__main__":
    sys.exit(main())
