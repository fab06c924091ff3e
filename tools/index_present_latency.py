"""Latency of presenting straight from a seek index (jsp_index_present / jsp_sp_index_present) on clip 0 of the 1080p bench clips
msvideo1_16_1080p_inter70 (512 frames) and screenpressor_v4_1080p_pclip300 (300 frames).  One index over the whole clip, then per
window and filter (0 nearest, 1 bilinear, 2 area):

  F   ONE Present([t], window) call: the fused launch, no full-size picture;
  P   the pair that existed before: Show(t) into a scratch frame buffer, then display_present / display_present_area of it,
      synchronised;

on the windows 320x180 Fit, 1280x720 Fit, 1920x1080 at 100 % and 3840x2160 Fit; and a contact sheet of --n cells of 240x135 (Fit):

  F   ONE Present(frames, 240x135, cols=8) call;
  P   n pairs, each window into its cell's own buffer;
  T   ONE Thumbs(frames, scale 8) call — the same cell size, but a box mean only: no conversion, no filter choice, less work.

Each form is measured with a host clock around calls that end synchronised, in one process, the forms alternating over several
frames of the index, medians of --reps passes.  Before anything is timed the fused result is checked against the pair's (exact).
One JSON line per measurement and an `all_results_match` line; the exit status is non-zero if anything differs.  Kernel times come
from a profiler trace of a run of its own (--reps 2 under the profiler); this script only names what it launches.

    python tools/index_present_latency.py [--reps 7] [--n 64] [--clips msv1,sp] [--out profiles/index_present_latency.json]
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

CLIPS = {"msv1": "msvideo1_16_1080p_inter70", "sp": "screenpressor_v4_1080p_pclip300"}
WINDOWS = (("320x180 fit", 320, 180, 0), ("1280x720 fit", 1280, 720, 0), ("1920x1080 100%", 1920, 1080, 1), ("3840x2160 fit", 3840, 2160, 0))
FILTERS = (("nearest", 0), ("bilinear", 1), ("area", 2))


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--clips", default="msv1,sp")
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import torch
    from jsplayer_amd import workloads as wl
    from jsplayer_amd.codec import DISPLAY_CANVAS, PRESENT_AREA, display_present, display_present_area, view_matrix
    if not torch.cuda.is_available():
        print("index_present_latency: no GPU", file=sys.stderr)
        return 2

    W, H = wl.W, wl.H
    lines = []
    ok_all = True

    def say(rec):
        lines.append(rec)
        print(json.dumps(rec), flush=True)

    for tag in args.clips.split(","):
        name = CLIPS[tag]
        clip = wl.build_clips(name)[0]
        dec = wl.make_codec(name)
        sp = tag == "sp"
        idx = dec.BuildScrubIndex(clip.frames, clip.keys) if sp else dec.BuildIndex(clip.frames, clip.keys)
        nf = idx.frames
        scratch = torch.zeros(W * H, dtype=torch.int32, device="cuda")
        probes = [(j * nf) // 5 + 3 for j in range(5)]                 # the frames a measurement alternates over

        def show(t):
            if sp:
                idx.Show(t, scratch)
            else:
                idx.Show(t, scratch, adopt=False)

        def pair(t, out, ww, wh, k, dx, dy, f):
            show(t)
            if f == PRESENT_AREA:
                display_present_area(scratch, W, H, out, ww, wh, k, dx, dy, mode=DISPLAY_CANVAS)
            else:
                display_present(scratch, W, H, out, ww, wh, k, dx, dy, mode=DISPLAY_CANVAS, filter=f)

        def timed(fn):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3

        for wname, ww, wh, zoom in WINDOWS:
            k, dx, dy = view_matrix(W, H, ww, wh, zoom)
            out_f = torch.zeros(ww * wh, dtype=torch.int32, device="cuda")
            out_p = torch.zeros_like(out_f)
            for fname, f in FILTERS:
                ok = True
                for t in probes:                                       # checked before it is timed (and the warm-up of both forms)
                    idx.Present([t], ww, wh, k, dx, dy, mode=DISPLAY_CANVAS, filter=f, out=out_f)
                    pair(t, out_p, ww, wh, k, dx, dy, f)
                    torch.cuda.synchronize()
                    ok &= bool(torch.equal(out_f, out_p))
                ok_all &= ok
                tf, tp = [], []
                for _ in range(args.reps):
                    for t in probes:
                        tf.append(timed(lambda: idx.Present([t], ww, wh, k, dx, dy, mode=DISPLAY_CANVAS, filter=f, out=out_f)))
                        tp.append(timed(lambda: pair(t, out_p, ww, wh, k, dx, dy, f)))
                mf, mp = statistics.median(tf), statistics.median(tp)
                say({"clip": name, "window": wname, "k": round(k, 5), "filter": fname, "fused_ms": round(mf, 4), "pair_ms": round(mp, 4),
                     "fused_ms_min": round(min(tf), 4), "pair_ms_min": round(min(tp), 4), "fused_over_pair": round(mf / mp, 3),
                     "fused_faster": mf < mp, "samples": len(tf), "results_match": ok})

        # the contact sheet: n cells of 240 x 135, 8 to a row
        n, cw, ch, cols = args.n, 240, 135, 8
        picks = [(j * nf) // n for j in range(n)]
        k, dx, dy = view_matrix(W, H, cw, ch, 0)
        rows = -(-n // cols)
        sheet = torch.zeros(rows * ch * cols * cw, dtype=torch.int32, device="cuda")
        cells = torch.zeros(n, ch * cw, dtype=torch.int32, device="cuda")
        tw, th = idx.ThumbSize(8)
        thumbs = torch.zeros(rows * th * cols * tw, dtype=torch.int32, device="cuda")
        for fname, f in FILTERS:
            def fused():
                idx.Present(picks, cw, ch, k, dx, dy, mode=DISPLAY_CANVAS, filter=f, cols=cols, out=sheet)

            def pairs():
                for j, t in enumerate(picks):
                    pair(t, cells[j], cw, ch, k, dx, dy, f)

            def strip():
                idx.Thumbs(picks, scale=8, cols=cols, out=thumbs)

            fused()
            pairs()
            strip()
            torch.cuda.synchronize()
            got = sheet.view(rows, ch, cols, cw)
            ok = all(bool(torch.equal(got[j // cols, :, j % cols, :], cells[j].view(ch, cw))) for j in range(n))
            ok_all &= ok
            tf, tp, tt = [], [], []
            for _ in range(args.reps):
                tf.append(timed(fused))
                tp.append(timed(pairs))
                tt.append(timed(strip))
            mf, mp, mt = statistics.median(tf), statistics.median(tp), statistics.median(tt)
            say({"clip": name, "sheet": f"{n} x {cw}x{ch}", "filter": fname, "fused_ms": round(mf, 4), "pairs_ms": round(mp, 4),
                 "thumbs8_ms": round(mt, 4), "fused_ms_min": round(min(tf), 4), "pairs_ms_min": round(min(tp), 4),
                 "thumbs8_ms_min": round(min(tt), 4), "fused_over_pairs": round(mf / mp, 3), "fused_over_thumbs8": round(mf / mt, 3),
                 "samples": len(tf), "results_match": ok})
        idx.close()
        dec.StopAndClean()
    say({"reps": args.reps, "device": torch.cuda.get_device_name(0), "all_results_match": ok_all})
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(lines, fh, indent=1)
    return 0 if ok_all else 1


if __name__ == "__main__":
    sys.exit(main())
