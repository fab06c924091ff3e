"""Latency of a model-ready tensor batch straight from a seek index (jsp_index_tensor / jsp_sp_index_tensor) on clip 0 of the 1080p
bench clips msvideo1_16_1080p_inter70 (512 frames) and screenpressor_v4_1080p_pclip300 (300 frames).  One index over the whole clip,
then per model input size (224x224 and 384x216, each Fit, area filter), batch (--batches frames spread evenly over the index) and
output (float16 NCHW, float32 NCHW, uint8 NHWC; scale 1 / 255, bias 0):

  F   ONE Tensor(frames, ...) call: the fused launch, no sheet of packed pixels;
  P   the pair it replaces: ONE Present(frames, ..., cols=1) call into an int sheet, then the torch ops that turn the sheet into the
      same tensor — three shift-and-mask unpacks stacked along the channel axis, a cast, a multiply, an add, a cast.

Both are measured with a host clock around calls that end synchronised, in one process, alternating, medians of --reps passes.  Before
anything is timed the fused result is checked against the pair's (exact: with this scale and bias float32 arithmetic gives the bits of
the contract's rule).  One JSON line per measurement with the tensor's bytes, and an `all_results_match` line; the exit status is
non-zero if anything differs.  Kernel times come from a profiler trace of a run of its own (--reps 2 under the profiler: per case the
fused kernel is launched three times, in the order of the JSON lines); this script only names what it launches.

    python tools/index_tensor_latency.py [--reps 7] [--batches 64,256] [--clips msv1,sp] [--out profiles/index_tensor_latency.json]
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
SIZES = ((224, 224), (384, 216))
OUTPUTS = (("float16", "nchw"), ("float32", "nchw"), ("uint8", "nhwc"))


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--batches", default="64,256")
    ap.add_argument("--clips", default="msv1,sp")
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import torch
    from jsplayer_amd import workloads as wl
    from jsplayer_amd.codec import DISPLAY_CANVAS, PRESENT_AREA, view_matrix
    if not torch.cuda.is_available():
        print("index_tensor_latency: no GPU", file=sys.stderr)
        return 2

    W, H = wl.W, wl.H
    lines = []
    ok_all = True

    def say(rec):
        lines.append(rec)
        print(json.dumps(rec), flush=True)

    def timed(fn):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    for tag in args.clips.split(","):
        name = CLIPS[tag]
        clip = wl.build_clips(name)[0]
        dec = wl.make_codec(name)
        idx = dec.BuildScrubIndex(clip.frames, clip.keys) if tag == "sp" else dec.BuildIndex(clip.frames, clip.keys)
        nf = idx.frames
        for ww, wh in SIZES:
            k, dx, dy = view_matrix(W, H, ww, wh, 0.0)
            for n in (int(v) for v in args.batches.split(",")):
                picks = [(j * nf) // n for j in range(n)]
                sheet = torch.zeros(n * wh * ww, dtype=torch.int32, device="cuda")
                for dname, layout in OUTPUTS:
                    dtype = getattr(torch, dname)
                    nchw = layout == "nchw"
                    shape = (1, 3, 1, 1) if nchw else (3,)
                    scale = torch.full(shape, 1.0 / 255, dtype=torch.float32, device="cuda")
                    bias = torch.zeros(shape, dtype=torch.float32, device="cuda")
                    out = torch.empty(n * 3 * wh * ww, dtype=dtype, device="cuda")
                    result = {}

                    def fused():
                        result["f"] = idx.Tensor(picks, ww, wh, k, dx, dy, mode=DISPLAY_CANVAS, filter=PRESENT_AREA, dtype=dtype, layout=layout, out=out)

                    def pair():
                        words = idx.Present(picks, ww, wh, k, dx, dy, mode=DISPLAY_CANVAS, filter=PRESENT_AREA, cols=1, out=sheet).view(n, wh, ww)
                        ch = torch.stack([(words >> s) & 0xFF for s in (0, 8, 16)], dim=1 if nchw else -1)
                        result["p"] = ch.to(torch.uint8) if dtype == torch.uint8 else (ch.to(torch.float32) * scale + bias).to(dtype)

                    fused()                                            # checked before it is timed (and the warm-up of both forms)
                    pair()
                    torch.cuda.synchronize()
                    ok = result["f"].shape == result["p"].shape and bool(torch.equal(result["f"], result["p"]))
                    ok_all &= ok
                    tf, tp = [], []
                    for _ in range(args.reps):
                        tf.append(timed(fused))
                        tp.append(timed(pair))
                    mf, mp = statistics.median(tf), statistics.median(tp)
                    say({"clip": name, "size": f"{ww}x{wh}", "k": round(k, 5), "n": n, "dtype": dname, "layout": layout,
                         "tensor_bytes": out.numel() * out.element_size(), "fused_ms": round(mf, 4), "pair_ms": round(mp, 4),
                         "fused_ms_min": round(min(tf), 4), "pair_ms_min": round(min(tp), 4), "fused_over_pair": round(mf / mp, 3),
                         "fused_faster": mf < mp, "samples": len(tf), "results_match": ok})
        idx.close()
        dec.StopAndClean()
    say({"reps": args.reps, "device": torch.cuda.get_device_name(0), "all_results_match": ok_all})
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(lines, fh, indent=1)
    return 0 if ok_all else 1


if __name__ == "__main__":
    sys.exit(main())
