"""The activity map of a seek index (jsp_index_activity / jsp_sp_index_activity) against the Shows and the compare pass it replaces,
on the two 512-frame 1080p MSVideo1 clips of tools/scrub_latency.py — msvideo1_16_1080p_inter70 and the idle clip — and the 300-frame
ScreenPressor bench clip screenpressor_v4_1080p_pclip300:

  A   ONE Activity(first, n): the picture before the run composed once per block, the pixels kept in registers, every writer of
      the run decoded once and compared, n * rows * cols counts written;
  B   the n + 1 Show(first - 1 .. first + n - 1) calls into two buffers of a FramePool used in turn (for first = 0 the picture
      before is the zeroed buffer: n Shows) and, per frame, the torch compare-and-pool that gives the same array: every picture
      written in full and read back twice;

for (first, n) = (1, 8), (256, 64) where the clip has that many frames, (0, all frames).  A and B alternate in one process, each measured with a host clock around calls
that end synchronised; medians of --reps.  Every A is first checked equal to its B.  One JSON line per measurement.

  --volumes   no GPU needed (MSVideo1 clips): from the clip's bytes (which frame codes which block), the bytes A and B read and
              write per row — bitmap words, table entries, code bytes and records per decode, pictures, the map.  For the
              ScreenPressor clip which block a frame changes is known only to the host stage: the GPU run reports the index's
              resident bytes, which bound what A reads, next to B's picture bytes.
  --kernel-only ROW   just a few Activity calls of row ROW (0 .. 2) on --clips' first clip: the program to put behind
              `rocprofv3 --kernel-trace --stats --`.

    python tools/index_activity_latency.py [--reps 5] [--clips inter70,idle,sp] [--parse gpu|host] [--out profiles/index_activity_latency.json]
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

from index_play_latency import CODE_BYTES, RECORD_BYTES, SCAN, coded_mask   # noqa: E402

ROWS = [(1, 8), (256, 64), (0, None)]   # (first, n); None: every frame of the clip
SP_CLIP = "screenpressor_v4_1080p_pclip300"


def load_clips(names):
    from jsplayer_amd import workloads as wl
    from skip_stills_latency import idle_clip
    for name in names.split(","):
        if name == "inter70":
            c = wl.build_clips("msvideo1_16_1080p_inter70")[0]
            yield name, c.frames, c.keys
        elif name == "sp":
            c = wl.build_clips(SP_CLIP)[0]
            yield name, c.frames, c.keys
        else:
            frames, keys = idle_clip(502)
            yield name, frames, keys


def rows_of(nf):
    return [(first, nf - first if n is None else n) for first, n in ROWS if first + (n or 1) <= nf]


def volumes(frames, rows, w, h):
    """Per row: the bytes ONE Activity reads and writes and the bytes the n + 1 Shows and n compares read and write (MSVideo1)."""
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
        aw, ad = show_read(first - 1) if first > 0 else (0, 0)
        aw += ((first + n - 1) // 32 - first // 32 + 1) * nb
        ad += int(coded[first:first + n].sum())
        a = dict(read_bytes=aw * 4 + ad * per_decode, written_bytes=n * cells * 2 * 2)   # (the memset and, at most, every count once more)
        bw = bd = 0
        shows = n + (1 if first > 0 else 0)
        for t in range(first - 1 if first > 0 else first, first + n):
            words, dec = show_read(t)
            bw += words
            bd += dec
        b = dict(read_bytes=bw * 4 + bd * per_decode + 2 * n * picture, written_bytes=shows * picture + n * cells * 2)
        out.append(dict(first=first, n=n, activity=a, shows_and_compare=b, decodes_activity=ad, decodes_shows=bd,
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
            for rec in volumes(frames, rows_of(len(frames)), wl.W, wl.H):
                say({"clip": name, **rec})
        save()
        return 0

    import torch
    if not torch.cuda.is_available():
        print("index_activity_latency: no GPU", file=sys.stderr)
        return 2
    from jsplayer_amd import FramePool, MSVideo1_16bit, player
    W, H = wl.W, wl.H
    cols, rows = (W + 15) // 16, (H + 15) // 16
    pool = FramePool(W, H, 3)
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
        two = [b for b in pool.frames[:3] if b is not c.PreviousFrame()][:2]

        def show(t, dst):
            if sp:
                idx.Show(t, dst)
            else:
                idx.Show(t, dst, adopt=False)

        def pooled(cur, prev):
            d = (cur != prev).view(H, W)
            d = torch.nn.functional.pad(d, (0, cols * 16 - W, 0, rows * 16 - H))
            return d.view(rows, 16, cols, 16).sum(dim=(1, 3), dtype=torch.int32).to(torch.int16)

        def form_a(first, n, out):
            t0 = time.perf_counter()
            idx.Activity(first, n, out=out)                  # (returns synchronised)
            return (time.perf_counter() - t0) * 1e3

        def form_b(first, n, out):
            t0 = time.perf_counter()
            if first > 0:
                show(first - 1, two[(first - 1) & 1])
            else:
                two[1].zero_()                               # P(-1) of these clips: nothing lies before frame 0
            for k in range(n):
                t = first + k
                show(t, two[t & 1])
                out[k] = pooled(two[t & 1], two[(t - 1) & 1])
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3

        todo = rows_of(nf)
        if args.kernel_only >= 0:
            first, n = todo[min(args.kernel_only, len(todo) - 1)]   # (a clip too short for a row has fewer: its last row is the whole clip)
            out = torch.empty((n, rows, cols), dtype=torch.int16, device="cuda")
            for _ in range(10):
                form_a(first, n, out)
            say({"clip": name, "kernel_only": [first, n], "changed_pixels": int(out.to(torch.int64).sum())})
            idx.close()
            c.StopAndClean()
            pool.close()
            return 0

        for first, n in todo:
            out_a = torch.empty((n, rows, cols), dtype=torch.int16, device="cuda")
            out_b = torch.empty_like(out_a)
            for b in two:
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
            say({"clip": name, "first": first, "n": n, "activity_ms": round(a, 4), "shows_and_compare_ms": round(b, 4),
                 "activity_ms_min": round(min(ta), 4), "shows_and_compare_ms_min": round(min(tb), 4),
                 "activity_us_per_frame": round(a * 1e3 / n, 2), "b_over_a": round(b / a, 2), "a_below_b": a < b,
                 "changed_pixels": int(out_a.to(torch.int64).sum()), "nonzero_cells": int((out_a != 0).sum()),
                 "map_bytes": n * rows * cols * 2, "pictures_written_by_b_bytes": (n + (1 if first > 0 else 0)) * W * H * 4,
                 "index_device_bytes": idx.device_bytes, "results_match": ok})
        idx.close()
        c.StopAndClean()
    say({"parse": args.parse, "reps": args.reps, "device": torch.cuda.get_device_name(0), "all_results_match": ok_all})
    pool.close()
    save()
    return 0 if ok_all else 1


if __name__ == "__main__":
    sys.exit(main())
