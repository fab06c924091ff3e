"""Filmstrip latency with the ScreenPressor seek index (jsp_sp_index_thumbs) on clip 0 of screenpressor_v4_1080p_pclip300 (ONE
key frame, 299 inter frames, 1080p).  One index over the whole clip, then n frames spread evenly over it (frame
(k * frames) // n), at each scale s:

  A   ONE Thumbs(frames, s) call: n thumbnails in one launch;
  B   what a caller could do before: n x Show(t, scratch) — full-size pictures, NO downscale at all, so B is a lower bound of
      that path;
  C   B plus a torch downscale (the same box mean) of each scratch frame into the sheet — informative only;

and one hover-preview row: Thumbs([t], s) against one Show(t).  Each form is measured with a host clock around calls that end
synchronised, in one process, the forms alternating, medians of --reps.  Before anything is timed every result is checked: the
pictures Show writes against the committed golden digests of the sequential decode, the sheet of A against the sheet of C
(exact).  Also printed: what the index holds in HBM before and after its first Thumbs call.  One JSON line per measurement and an
`all_results_match` line; the exit status is non-zero if anything differs.

    python tools/sp_filmstrip_latency.py [--reps 5] [--n 64] [--scales 4,8,16] [--out profiles/sp_filmstrip_latency.json]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NAME = "screenpressor_v4_1080p_pclip300"


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--scales", default="4,8,16")
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import torch
    from jsplayer_amd import workloads as wl
    if not torch.cuda.is_available():
        print("sp_filmstrip_latency: no GPU", file=sys.stderr)
        return 2

    npix = wl.W * wl.H
    scales = [int(s) for s in args.scales.split(",")]
    clip = wl.build_clips(NAME)[0]
    frames, keys = clip.frames, clip.keys
    nf = len(frames)
    picks = [(k * nf) // args.n for k in range(args.n)]
    want = list(wl.golden_digests(NAME, 0)[0])
    for t in range(1, nf):          # "-": an unchanged frame — the picture before it stays
        if want[t] == "-":
            want[t] = want[t - 1]
    lines = []

    def say(rec):
        lines.append(rec)
        print(json.dumps(rec), flush=True)

    def downscale(pic, s, tw, th, out):
        """The contract's box mean of a full-size picture, in torch: per byte, rounded half up."""
        shift = {4: 4, 8: 6, 16: 8}[s]
        v = pic.view(wl.H, wl.W)[: th * s, : tw * s]
        acc = None
        for pos in (16, 8, 0):
            c = ((v >> pos) & 0xFF).reshape(th, s, tw, s).sum(dim=(1, 3), dtype=torch.int32)
            c = ((c + (s * s) // 2) >> shift) << pos
            acc = c if acc is None else acc | c
        out.copy_(acc)

    dec = wl.make_codec(NAME)
    idx = dec.BuildScrubIndex(frames, keys)
    scratch = torch.zeros(npix, dtype=torch.int32, device="cuda")

    def device_bytes():
        n, dev, host = C.c_int(0), C.c_uint64(0), C.c_uint64(0)
        idx._lib.jsp_sp_index_info(idx._h, C.byref(n), C.byref(dev), C.byref(host))
        return dev.value

    def form_a(s, sheet, which):
        t0 = time.perf_counter()
        idx.Thumbs(which, scale=s, cols=1, out=sheet)
        return (time.perf_counter() - t0) * 1e3

    def form_b(which):
        t0 = time.perf_counter()
        for t in which:
            idx.Show(t, scratch)
        return (time.perf_counter() - t0) * 1e3

    def form_c(s, tw, th, sheet, which, check=False):
        cells = sheet.view(len(which), th, tw)
        ok = True
        t0 = time.perf_counter()
        for k, t in enumerate(which):
            idx.Show(t, scratch)
            if check:
                ok &= wl.digest(scratch.cpu().numpy()) == want[t]
            downscale(scratch, s, tw, th, cells[k])
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, ok

    ok_all = True
    before = device_bytes()
    for s in scales:
        tw, th = idx.ThumbSize(s)
        sheet_a = torch.zeros(args.n * th * tw, dtype=torch.int32, device="cuda")
        sheet_c = torch.zeros_like(sheet_a)
        # checked before it is timed (and the warm-up of every form)
        _, ok = form_c(s, tw, th, sheet_c, picks, check=True)
        form_a(s, sheet_a, picks)
        if s == scales[0]:
            say({"frames": nf, "device_bytes_before_first_thumbs": before, "device_bytes_after_first_thumbs": device_bytes()})
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
        say({"clip": NAME, "n": args.n, "scale": s, "thumb": [tw, th], **{f"{m}_ms": round(v, 4) for m, v in med.items()},
             **{f"{m}_ms_min": round(min(v), 4) for m, v in times.items()}, "A_over_B": round(med["A"] / med["B"], 4),
             "A_over_C": round(med["A"] / med["C"], 4), "A_faster_than_B": med["A"] < med["B"], "results_match": ok})

    # the hover preview: one thumbnail against one Show
    t = picks[len(picks) // 2]
    for s in scales:
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
        say({"clip": NAME, "n": 1, "scale": s, "frame": t, "A_ms": round(statistics.median(times["A"]), 4),
             "B_ms": round(statistics.median(times["B"]), 4), "A_ms_min": round(min(times["A"]), 4),
             "B_ms_min": round(min(times["B"]), 4), "results_match": ok})
    idx.close()
    dec.StopAndClean()
    say({"reps": args.reps, "device": torch.cuda.get_device_name(0), "all_results_match": ok_all})
    if args.out:
        with open(args.out, "w") as f:
            json.dump(lines, f, indent=1)
    return 0 if ok_all else 1


if __name__ == "__main__":
    sys.exit(main())
