"""What presenting a frame in a window costs (jsp_display_present: conversion, row flip, crop and resampling in one launch) on one
MI355X: one 1080p frame of random 24-bit pixels in a pool buffer, presented into five windows —

  1280x720 Fit, 1920x1080 at 100 %, 1920x1080 at 200 % in the middle of the picture, 3840x2160 Fit, 640x360 Fit

— with both filters, and in the same process what there is to compare with: jsp_display_convert of the same frame (the full-size
one-to-one pass a caller had before) and the plain fill rate over the window's bytes (jsp_measure_fill: one 16-byte store per lane,
nothing read).  Every form is warmed up, then timed with device events around --launches back-to-back launches on one stream,
--rounds times with the forms taking turns; the median per-launch time is reported, and as a fraction of the fill rate the time
the fill would need for max(window bytes, frame bytes the window reads).  The frame and every window fit the 256 MiB Infinity
Cache, for the present, the convert and the fill alike.  Each window is first checked against tests/view_ref.py.

The event times include what it takes to queue a launch from Python (a few microseconds, the floor every form of a few megabytes
sits on), so the kernels' own durations come from a profiler run of its own:

  --kernel-only   every form launched --kernel-launches times in a fixed order, nothing else: the program to put behind
                  `rocprofv3 --kernel-trace --output-format csv -d DIR --`; writes the order to --plan.
  --reduce DIR    no GPU needed: reads the kernel trace under DIR and the plan, and adds each form's kernel time (median, min, max of
                  its dispatches, the first three dropped) and its fraction of the fill KERNEL's time over max(window bytes, bytes
                  read) to the records of --out.

  --area          the area-averaged call instead (jsp_display_present_area): the windows a shrunk picture goes into —
                  1280x720 Fit, 640x360 Fit, 480x270 Fit and 30x17 at k = 1/64 — each as area, nearest and bilinear, beside the same
                  jsp_display_convert (which reads the same 8.3 MB once: the floor for a kernel that reads the whole frame) and fills;
                  each area window is first checked against tests/view_area_ref.py.  Goes with the three forms above; --out defaults
                  to profiles/present_area_latency.json, --plan to present_area_kernel_plan.json beside it.

    python tools/present_latency.py [--area] [--launches 200] [--rounds 7] [--out profiles/present_latency.json]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

FW, FH = 1920, 1080
# (name, window, zoom, hor, ver)
CASES = [("1280x720 fit", (1280, 720), 0, 0.5, 0.5),
         ("1920x1080 100%", (1920, 1080), 1, 0.5, 0.5),
         ("1920x1080 200% centre", (1920, 1080), 2, 0.5, 0.5),
         ("3840x2160 fit", (3840, 2160), 0, 0.5, 0.5),
         ("640x360 fit", (640, 360), 0, 0.5, 0.5)]
AREA_CASES = [("1280x720 fit", (1280, 720), 0, 0.5, 0.5),
              ("640x360 fit", (640, 360), 0, 0.5, 0.5),
              ("480x270 fit", (480, 270), 0, 0.5, 0.5),
              ("30x17 k=1/64", (30, 17), 1.0 / 64, 0.5, 0.5)]


def bytes_read(ww, wh, k, dx, dy):
    """Bytes of the frame under the window: the source rectangle the display matrix maps onto it, clipped to the picture."""
    x_lo, x_hi = max(0.0, dx / k), min(float(FW), (ww + dx) / k)
    y_lo, y_hi = max(0.0, dy / k), min(float(FH), (wh + dy) / k)
    return int(max(0.0, x_hi - x_lo) * max(0.0, y_hi - y_lo)) * 4


KERNELS = {"present": "display_present_kernel", "present_area": "display_present_area_kernel", "display_convert": "display_convert_kernel", "fill": "ceiling_fill_kernel"}
DROP = 3      # dispatches of each form that count as warm-up in the kernel trace


def reduce_trace(trace_dir, plan_path, out_path) -> int:
    """Kernel durations per form from a rocprofv3 kernel trace of a --kernel-only run."""
    import csv
    import glob
    plan = json.load(open(plan_path))
    files = sorted(glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True))
    if len(files) != 1:
        print(f"present_latency --reduce: expected one *kernel_trace.csv under {trace_dir}, found {len(files)}", file=sys.stderr)
        return 1
    rows = [r for r in csv.DictReader(open(files[0])) if any(k in r["Kernel_Name"] for k in KERNELS.values())]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    at, kernel_us = 0, {}
    for step in plan["order"]:
        mine = rows[at:at + step["count"]]
        at += step["count"]
        if len(mine) != step["count"] or any(KERNELS[step["kind"]] not in r["Kernel_Name"] for r in mine):
            print(f"present_latency --reduce: the trace does not follow the plan at {step['form']}", file=sys.stderr)
            return 1
        ns = [int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in mine[DROP:]]
        kernel_us[step["form"]] = {"median": statistics.median(ns) / 1000.0, "min": min(ns) / 1000.0, "max": max(ns) / 1000.0, "dispatches": len(ns)}
    if at != len(rows):
        print(f"present_latency --reduce: {len(rows) - at} dispatches more than the plan holds", file=sys.stderr)
        return 1
    doc = json.load(open(out_path)) if os.path.exists(out_path) else {"results": [{"form": f, "window": f} for f in kernel_us if not f.startswith("fill ")]}
    for rec in doc["results"]:
        form = rec.get("form") or (f"{rec['window']} {rec['filter']}" if rec.get("filter") else "display_convert 1920x1080")
        ku = kernel_us[form]
        fill = kernel_us["fill " + (rec["window"] if rec.get("filter") else "1920x1080 one-to-one")]
        rec.update({"kernel_us_median": round(ku["median"], 3), "kernel_us_min": round(ku["min"], 3), "kernel_us_max": round(ku["max"], 3),
                    "kernel_dispatches": ku["dispatches"], "fill_kernel_us_over_window": round(fill["median"], 3)})
        if "window_bytes" in rec:
            fill_us = fill["median"] * max(rec["window_bytes"], rec["bytes_read"]) / rec["window_bytes"]
            rec.update({"fill_kernel_us_for_max_bytes": round(fill_us, 3), "kernel_fraction_of_fill": round(fill_us / ku["median"], 4)})
        print(json.dumps(rec))
    doc["kernel_method"] = "rocprofv3 --kernel-trace, a run of its own (--kernel-only): dispatch durations per form, the first %d dropped" % DROP
    with open(out_path, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    return 0


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--area", action="store_true")
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernel-only", action="store_true")
    ap.add_argument("--kernel-launches", type=int, default=23)
    ap.add_argument("--plan", default=None)
    ap.add_argument("--reduce", default=None, metavar="DIR")
    args = ap.parse_args()
    args.out = args.out or os.path.join(ROOT, "profiles", "present_area_latency.json" if args.area else "present_latency.json")
    plan_path = args.plan or os.path.join(os.path.dirname(args.out), "present_area_kernel_plan.json" if args.area else "present_kernel_plan.json")
    if args.reduce:
        return reduce_trace(args.reduce, plan_path, args.out)

    import numpy as np
    import torch
    if not torch.cuda.is_available():
        print("present_latency: needs a GPU (nothing is measured without one)", file=sys.stderr)
        return 1
    import view_area_ref as ar
    import view_ref as vr
    from jsplayer_amd import _native as N
    from jsplayer_amd import codec as cm

    lib = N.lib()
    pool = cm.FramePool(FW, FH, 2)
    frame, full = pool.frames
    pixels = np.random.default_rng(1).integers(0, 1 << 24, size=FW * FH, dtype=np.uint64).astype(np.uint32)
    frame.copy_(torch.from_numpy(pixels.view(np.int32)))
    stream = torch.cuda.Stream()
    handle = stream.cuda_stream

    forms = {}      # name -> (callable queuing ONE launch on `stream`, record)
    fills = {}      # window name -> the tensor the fill is measured over
    AREA = "area"       # (no filter value of jsp_display_present: the call of its own)
    filters = ((cm.PRESENT_NEAREST, "nearest"), (cm.PRESENT_BILINEAR, "bilinear"))

    def present(out, ww, wh, k, dx, dy, filt):
        if filt == AREA:
            cm.display_present_area(frame, FW, FH, out, ww, wh, k, dx, dy, stream=handle)
        else:
            cm.display_present(frame, FW, FH, out, ww, wh, k, dx, dy, filter=filt, stream=handle)

    for name, (ww, wh), zoom, hor, ver in (AREA_CASES if args.area else CASES):
        k, dx, dy = cm.view_matrix(FW, FH, ww, wh, zoom, hor, ver)
        out = torch.empty(max(ww * wh, 1024), dtype=torch.int32, device="cuda")    # (jsp_measure_fill takes 4096 bytes or more: the fill of the 30x17 window is over 4096)
        rate = C.c_double(0)
        torch.cuda.synchronize()
        fills[name] = out
        if not args.kernel_only and lib.jsp_measure_fill(C.c_void_p(out.data_ptr()), C.c_size_t(out.numel() * 4), 50, C.byref(rate), C.c_void_p(handle)) != 0:
            raise RuntimeError(N.last_error())
        for filt, fname in (((AREA, "area"),) + filters if args.area else filters):
            what = "present_area" if filt == AREA else "present"
            if args.kernel_only:
                forms[f"{name} {fname}"] = (lambda out=out, ww=ww, wh=wh, k=k, dx=dx, dy=dy, filt=filt: present(out, ww, wh, k, dx, dy, filt), {"what": what})
                continue
            present(out, ww, wh, k, dx, dy, filt)
            stream.synchronize()
            want = ar.present_area(pixels, FW, FH, ww, wh, k, dx, dy, ar.CANVAS) if filt == AREA else vr.present(pixels, FW, FH, ww, wh, k, dx, dy, vr.CANVAS, filt)
            if not np.array_equal(out.cpu().numpy().view(np.uint32)[:ww * wh].reshape(wh, ww), want):
                raise RuntimeError(f"{name} {fname}: the window differs from the reference")
            rec = {"what": what, "window": name, "filter": fname, "k": k, "dx": dx, "dy": dy, "window_bytes": ww * wh * 4,
                   "bytes_read": bytes_read(ww, wh, k, dx, dy), "fill_gbps_over_window": rate.value}
            forms[f"{name} {fname}"] = (lambda out=out, ww=ww, wh=wh, k=k, dx=dx, dy=dy, filt=filt: present(out, ww, wh, k, dx, dy, filt), rec)
    rate = C.c_double(0)
    fills["1920x1080 one-to-one"] = full
    if not args.kernel_only and lib.jsp_measure_fill(C.c_void_p(full.data_ptr()), C.c_size_t(FW * FH * 4), 50, C.byref(rate), C.c_void_p(handle)) != 0:
        raise RuntimeError(N.last_error())
    forms["display_convert 1920x1080"] = (lambda: cm.display_convert(frame, full, FW, FH, cm.DISPLAY_CANVAS, True, stream=handle),
                                          {"what": "display_convert", "window": "1920x1080 one-to-one", "filter": None, "window_bytes": FW * FH * 4,
                                           "bytes_read": FW * FH * 4, "fill_gbps_over_window": rate.value})

    if args.kernel_only:
        order = []
        for name, (queue, rec) in forms.items():
            for _ in range(args.kernel_launches):
                queue()
            stream.synchronize()
            order.append({"form": name, "kind": rec["what"], "count": args.kernel_launches})
        for name, t in fills.items():     # (jsp_measure_fill: three passes of `reps` launches)
            if lib.jsp_measure_fill(C.c_void_p(t.data_ptr()), C.c_size_t(t.numel() * 4), args.kernel_launches, C.byref(rate), C.c_void_p(handle)) != 0:
                raise RuntimeError(N.last_error())
            order.append({"form": "fill " + name, "kind": "fill", "count": 3 * args.kernel_launches})
        os.makedirs(os.path.dirname(plan_path) or ".", exist_ok=True)
        with open(plan_path, "w") as f:
            json.dump({"order": order}, f, indent=1)
        pool.close()
        return 0

    times = {name: [] for name in forms}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(stream):
        for name, (queue, _) in forms.items():
            for _ in range(args.warmup):
                queue()
        stream.synchronize()
        for _ in range(args.rounds):
            for name, (queue, _) in forms.items():
                e0.record(stream)
                for _ in range(args.launches):
                    queue()
                e1.record(stream)
                e1.synchronize()
                times[name].append(e0.elapsed_time(e1) * 1000.0 / args.launches)

    results = []
    for name, (_, rec) in forms.items():
        us = statistics.median(times[name])
        moved = max(rec["window_bytes"], rec["bytes_read"])
        fill_us = moved / (rec["fill_gbps_over_window"] * 1e3)
        rec.update({"us_per_launch_median": round(us, 3), "us_per_launch_min": round(min(times[name]), 3),
                    "us_per_launch_max": round(max(times[name]), 3), "launches": args.launches, "rounds": args.rounds,
                    "fill_us_for_max_bytes": round(fill_us, 3), "fraction_of_fill": round(fill_us / us, 4)})
        results.append(rec)
        print(json.dumps(rec))
    doc = {"device": torch.cuda.get_device_name(0), "frame": [FW, FH], "method": "device events around back-to-back launches on one stream (launch overhead included), forms taking turns, median of rounds",
           "results": results}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    pool.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
