"""The distance map of a seek index (jsp_index_distance / jsp_sp_index_distance) against the Shows and the compare pass it replaces,
on the clips of tools/index_activity_latency.py — the two 512-frame 1080p MSVideo1 clips (msvideo1_16_1080p_inter70 and the idle clip)
and the 300-frame ScreenPressor bench clip screenpressor_v4_1080p_pclip300:

  A   ONE Distance(ref, first, n): the reference's block and the block of frame `first` composed once, the reference kept in
      registers, every writer of the run decoded once and counted against it, n * rows * cols counts written — every one, no memset;
  B   Show(ref) into one buffer of a FramePool, then the n Show(first .. first + n - 1) calls into another and, per frame, the torch
      `!=` and pool that give the same array: every picture written in full and read back;

for (first, n) = (1, 8), (256, 64) — the last 64 frames of a clip shorter than 320 —, (0, all frames); the reference is the clip's middle frame.  A
and B alternate in one process, each measured with a host clock around calls that end synchronised; medians of --reps.  Every A is
first checked equal to its B.  One JSON line per measurement.  For "the same walk with another last step" run
tools/index_activity_latency.py beside it: its rows are the same runs.

  --volumes   no GPU needed (MSVideo1 clips): from the clip's bytes (which frame codes which block), the bytes A and B read and
              write per row — bitmap words, table entries, code bytes and records per decode, pictures, the map.
  --kernel-only ROW   just a few Distance calls of row ROW (0 .. 2) on --clips' first clip: the program to put behind
              `rocprofv3 --kernel-trace --stats --`.

    python tools/index_distance_latency.py [--reps 5] [--clips inter70,idle,sp] [--parse gpu|host] [--out profiles/index_distance_latency.json]
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

from index_activity_latency import SP_CLIP, load_clips   # noqa: E402
from index_play_latency import CODE_BYTES, RECORD_BYTES, SCAN, coded_mask   # noqa: E402


def rows_of(nf):
    """(first, n): 8 frames, 64 frames (from frame 256, or the last 64 of a shorter clip), the whole clip."""
    rows = [(1, 8), (min(256, nf - 64), 64), (0, nf)]
    return [(first, n) for first, n in rows if first >= 0 and first + n <= nf]


def volumes(frames, rows, w, h, ref):
    """Per row: the bytes ONE Distance reads and writes and the bytes the n + 1 Shows and n compares read and write (MSVideo1)."""
    import numpy as np
    nb = (w // 4) * (h // 4)
    cells = ((w + 15) // 16) * ((h + 15) // 16)
    picture = w * h * 4
    nf = len(frames)
    coded = np.zeros((nf, nb), dtype=bool)
    last = np.full((nf, nb), -1, dtype=np.int16)      # last[t][b]: the last frame <= t that codes block b
    cur = np.full(nb, -1, dtype=np.int16)
    for t, f in enumerate(frames):
        coded[t] = coded_mask(nb, bytes(f))
        cur = np.where(coded[t], np.int16(t), cur)
        last[t] = cur

    def show_read(t):
        """(bitmap words, decodes) of composing frame t: word t / 32, then SCAN words per step down to the writer's."""
        L = last[t].astype(np.int64)
        wt = t >> 5
        target = np.where(L >= 0, L >> 5, 0)
        steps = -(-(wt - target) // SCAN)
        words = 1 + np.minimum(SCAN * steps, wt)
        return int(words.sum()), int((L >= 0).sum())

    per_decode = 4 + CODE_BYTES + RECORD_BYTES
    out = []
    for first, n in rows:
        rw, rd = show_read(ref)
        fw, fd = show_read(first)
        aw = rw + fw + ((first + n - 1) // 32 - (first + 1) // 32 + 1) * nb * (1 if n > 1 else 0)
        ad = rd + fd + int(coded[first + 1:first + n].sum())
        a = dict(read_bytes=aw * 4 + ad * per_decode, written_bytes=n * cells * 2)
        bw, bd = rw, rd
        for t in range(first, first + n):
            words, dec = show_read(t)
            bw += words
            bd += dec
        b = dict(read_bytes=bw * 4 + bd * per_decode + 2 * n * picture, written_bytes=(n + 1) * picture + n * cells * 2)
        out.append(dict(first=first, n=n, ref=ref, distance=a, shows_and_compare=b, decodes_distance=ad, decodes_shows=bd,
                        bytes_moved_b_over_a=round((b["read_bytes"] + b["written_bytes"]) / max(a["read_bytes"] + a["written_bytes"], 1), 1)))
    return out


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--parse", default="gpu", choices=["gpu", "host"])
    ap.add_argument("--clips", default="inter70,idle,sp")
    ap.add_argument("--volumes", action="store_true")
    ap.add_argument("--kernel-only", type=int, default=-1)
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    from jsplayer_amd import workloads as wl
    lines = []

    def say(rec):
        lines.append(rec)
        print(json.dumps(rec), flush=True)

    def save():
        if args.out:
            with open(args.out, "w") as f:
                json.dump(lines, f, indent=1)

    if args.volumes:
        for name, frames, _ in load_clips(",".join(c for c in args.clips.split(",") if c != "sp")):
            for rec in volumes(frames, rows_of(len(frames)), wl.W, wl.H, len(frames) // 2):
                say({"clip": name, **rec})
        save()
        return 0

    import torch
    if not torch.cuda.is_available():
        print("index_distance_latency: no GPU", file=sys.stderr)
        return 2
    from jsplayer_amd import FramePool, MSVideo1_16bit, player
    W, H = wl.W, wl.H
    assert W % 4 == 0 and H % 4 == 0, "form B compares whole pictures: an MSVideo1 picture with remainder pixels needs a mask"
    cols, rows = (W + 15) // 16, (H + 15) // 16
    pool = FramePool(W, H, 4)
    ok_all = True
    for name, frames, keys in load_clips(args.clips):
        sp = name == "sp"
        if sp:
            c = wl.make_codec(SP_CLIP)
            idx = c.BuildScrubIndex(frames, keys)
        else:
            c = MSVideo1_16bit(W, H)
            c.set_option("msv1_parse", args.parse)
            c.Preinit(player.INSIGNIFICANT_LINES)
            idx = c.BuildIndex(frames, keys)
        assert idx.ActivitySize() == (cols, rows)
        nf = idx.frames
        ref = nf // 2
        ref_buf, cur_buf = [b for b in pool.frames[:4] if b is not c.PreviousFrame()][:2]

        def show(t, dst):
            if sp:
                idx.Show(t, dst)
            else:
                idx.Show(t, dst, adopt=False)

        def pooled(cur, other):
            d = (cur != other).view(H, W)
            d = torch.nn.functional.pad(d, (0, cols * 16 - W, 0, rows * 16 - H))
            return d.view(rows, 16, cols, 16).sum(dim=(1, 3), dtype=torch.int32).to(torch.int16)

        def form_a(first, n, out):
            t0 = time.perf_counter()
            idx.Distance(ref, first, n, out=out)             # (returns synchronised)
            return (time.perf_counter() - t0) * 1e3

        def form_b(first, n, out):
            t0 = time.perf_counter()
            show(ref, ref_buf)
            for k in range(n):
                show(first + k, cur_buf)
                out[k] = pooled(cur_buf, ref_buf)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3

        todo = rows_of(nf)
        if args.kernel_only >= 0:
            first, n = todo[min(args.kernel_only, len(todo) - 1)]   # (a clip too short for a row has fewer: its last row is the whole clip)
            out = torch.empty((n, rows, cols), dtype=torch.int16, device="cuda")
            for _ in range(10):
                form_a(first, n, out)
            say({"clip": name, "kernel_only": [first, n], "ref": ref, "differing_pixels": int(out.to(torch.int64).sum())})
            idx.close()
            c.StopAndClean()
            pool.close()
            return 0

        for first, n in todo:
            out_a = torch.empty((n, rows, cols), dtype=torch.int16, device="cuda")
            out_b = torch.empty_like(out_a)
            for b in (ref_buf, cur_buf):
                b.zero_()
            form_a(first, n, out_a)
            form_b(first, n, out_b)
            ok = bool(torch.equal(out_a, out_b))
            ok_all &= ok
            ta, tb = [], []
            for _ in range(args.reps):
                ta.append(form_a(first, n, out_a))
                tb.append(form_b(first, n, out_b))
            a, b = statistics.median(ta), statistics.median(tb)
            say({"clip": name, "first": first, "n": n, "ref": ref, "distance_ms": round(a, 4), "shows_and_compare_ms": round(b, 4),
                 "distance_ms_min": round(min(ta), 4), "shows_and_compare_ms_min": round(min(tb), 4),
                 "distance_us_per_frame": round(a * 1e3 / n, 2), "b_over_a": round(b / a, 2), "a_below_b": a < b,
                 "differing_pixels": int(out_a.to(torch.int64).sum()), "nonzero_cells": int((out_a != 0).sum()),
                 "frames_at_distance_0": int((out_a.reshape(n, -1).to(torch.int64).sum(dim=1) == 0).sum()),
                 "map_bytes": n * rows * cols * 2, "pictures_written_by_b_bytes": (n + 1) * W * H * 4,
                 "index_device_bytes": idx.device_bytes, "results_match": ok})
        idx.close()
        c.StopAndClean()
    say({"parse": args.parse, "reps": args.reps, "device": torch.cuda.get_device_name(0), "all_results_match": ok_all})
    pool.close()
    save()
    return 0 if ok_all else 1


if __name__ == "__main__":
    sys.exit(main())
