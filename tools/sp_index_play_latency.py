"""Playback from the ScreenPressor seek index (jsp_sp_index_play) against the Shows it replaces, on clip 0 of
screenpressor_v4_1080p_pclip300 (ONE key frame, 299 inter frames, 1080p):

  A   ONE Play(first, n, stride): frame `first` composed once, the pixels carried forward in registers, n pictures stored;
  B   the n Show(first + k * stride) calls that write the same pictures into the same buffers: n launches, n synchronises, the
      backward walk paid n times;

for (first, n, stride) = (1, 9, 1), (150, 9, 1), (1, 64, 1), (0, 300, 1), (0, 38, 8).  The destinations come from a FramePool.  A and
B alternate in one process, each measured with a host clock around calls that end synchronised; medians of --reps.  Every picture
of both forms is first checked against the golden digests of the sequential decode.  Prints one JSON line per row.

  --volumes   no GPU needed: from the host stage's tables (tests/hoststage_binding.py), the bytes A and B read and write per row —
              per block the bitmap words, records and literals of the backward walk (once for A, once per frame for B) and, for A,
              of the forward walk behind it.
  --kernel-only ROW   just a few Play calls of row ROW (0 .. 4): the program to put behind `rocprofv3 --kernel-trace --stats --`.

    python tools/sp_index_play_latency.py [--reps 5] [--out profiles/sp_index_play_latency.json]
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
ROWS = [(1, 9, 1), (150, 9, 1), (1, 64, 1), (0, 300, 1), (0, 38, 8)]


def volumes(frames, keys, rows):
    """Per row: the bytes ONE Play reads and writes, and the bytes the n Shows read and write, simulated per block from the
    literalised tables.  Host stage only."""
    import numpy as np
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import hoststage_binding as hb
    from jsplayer_amd import workloads as wl
    w, h = wl.W, wl.H
    nbx, nby = (w + 15) // 16, (h + 15) // 16
    nb = nbx * nby
    nf = len(frames)
    hs = hb.HostStage(w, h, 24)
    hs.preinit(36)
    writers = [[] for _ in range(nb)]     # per block: (frame, 16x16 mask of its rectangle inside the picture), ascending
    inside = np.zeros((nb, 16, 16), bool)
    px = np.arange(16)
    by, bx = np.divmod(np.arange(nb), nbx)
    inside[:] = ((by[:, None] * 16 + px[None, :]) < h)[:, :, None] & ((bx[:, None] * 16 + px[None, :]) < w)[:, None, :]
    for t in range(nf):
        d = hs.decode(bool(keys[t]), frames[t])
        assert d["status"] == 0, (t, d["error"])
        if d["kind"] != hb.KIND_INTER:
            continue
        d = hs.literalise_motion(d)
        blocks = d["blocks"]
        for b in np.nonzero(blocks[:, 0])[0]:
            x1, y1, x2, y2 = (int(v) for v in blocks[b, 1:5])
            m = np.zeros((16, 16), bool)
            m[y1:y2, x1:x2] = True
            writers[b].append((t, m & inside[b]))
    hs.close()
    key_of = []
    for t in range(nf):
        key_of.append(t if keys[t] else key_of[-1])
    picture = w * h * 4

    def backward(t):
        """What index_compose reads for frame t, all blocks: (bitmap words, records, literal pixels)."""
        k = key_of[t]
        if t == k:
            return 0, 0, 0
        wlo = (k + 1) >> 5
        words = records = literals = 0
        for b in range(nb):
            mine = [(f, m) for f, m in writers[b] if k < f <= t]
            if not mine:
                words += (t >> 5) - wlo + 1
                continue
            open_px = inside[b].copy()
            lowest_word = wlo
            for f, m in reversed(mine):
                records += 1
                take = m & open_px
                literals += int(take.sum())
                open_px &= ~take
                if not open_px.any():
                    lowest_word = f >> 5
                    break
            words += (t >> 5) - lowest_word + 1
        return words, records, literals

    back = {}
    out = []
    for first, n, stride in rows:
        last = first + (n - 1) * stride
        shown = [first + k * stride for k in range(n)]
        for t in shown:
            if t not in back:
                back[t] = backward(t)
        # B: n backward walks, each with the key picture underneath
        bw = sum(back[t][0] for t in shown)
        br = sum(back[t][1] for t in shown)
        bl = sum(back[t][2] for t in shown)
        b_read = dict(bitmap_bytes=bw * 4, record_bytes=br * 16, literal_bytes=bl * 4, key_picture_bytes=n * picture)
        b_read["read_bytes"] = sum(b_read.values())
        # A: one backward walk, then per block a bitmap word and a key-mask word per 32 frames, and per writer in (first, last] its
        # frame record, its block record and the literals inside the picture; a key frame inside the run reloads the key picture
        spanned = (last >> 5) - (first >> 5) + 1 if last > first else 0
        fr = fl = 0
        for b in range(nb):
            for f, m in writers[b]:
                if first < f <= last:
                    fr += 1
                    fl += int(m.sum())
        keys_inside = sum(1 for f in range(first + 1, last + 1) if keys[f])
        a_read = dict(bitmap_bytes=(back[first][0] + spanned * nb) * 4, key_mask_bytes=spanned * nb * 4,
                      record_bytes=back[first][1] * 16 + fr * 32 + nb * 16, literal_bytes=(back[first][2] + fl) * 4,
                      key_picture_bytes=(1 + keys_inside) * picture, destination_list_bytes=n * nb * 8)
        a_read["read_bytes"] = sum(a_read.values())
        out.append(dict(first=first, n=n, stride=stride, written_bytes=n * picture, play=a_read, shows=b_read,
                        read_ratio_shows_over_play=round(b_read["read_bytes"] / a_read["read_bytes"], 2)))
    return out


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--volumes", action="store_true")
    ap.add_argument("--kernel-only", type=int, default=-1)
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    from jsplayer_amd import workloads as wl
    clip = wl.build_clips(NAME)[0]
    frames, keys = clip.frames, clip.keys
    nf = len(frames)
    lines = []

    def say(rec):
        lines.append(rec)
        print(json.dumps(rec), flush=True)

    def save():
        if args.out:
            with open(args.out, "w") as f:
                json.dump(lines, f, indent=1)

    if args.volumes:
        for rec in volumes(frames, keys, ROWS):
            say(rec)
        save()
        return 0

    import torch
    if not torch.cuda.is_available():
        print("sp_index_play_latency: no GPU", file=sys.stderr)
        return 2
    from jsplayer_amd import FramePool
    want = list(wl.golden_digests(NAME, 0)[0])
    for t in range(1, nf):
        if want[t] == "-":
            want[t] = want[t - 1]
    codec = wl.make_codec(NAME)
    idx = codec.BuildScrubIndex(frames, keys)
    pool = FramePool(wl.W, wl.H, max(n for _, n, _ in ROWS))

    def play(first, n, stride):
        t0 = time.perf_counter()
        idx.Play(first, pool.frames[:n], stride)          # (returns synchronised)
        return (time.perf_counter() - t0) * 1e3

    def shows(first, n, stride):
        t0 = time.perf_counter()
        for k in range(n):
            idx.Show(first + k * stride, pool.frames[k])  # (each returns synchronised)
        return (time.perf_counter() - t0) * 1e3

    def exact(first, n, stride):
        return all(wl.digest(pool.frames[k].cpu().numpy()) == want[first + k * stride] for k in range(n))

    def poison(n):
        for b in pool.frames[:n]:
            b.fill_(0x5A5A5A5A)
        torch.cuda.synchronize()

    if args.kernel_only >= 0:
        first, n, stride = ROWS[args.kernel_only]
        for _ in range(10):
            play(first, n, stride)
        ok = exact(first, n, stride)
        say({"kernel_only": [first, n, stride], "digests_match": ok})
        idx.close()
        pool.close()
        codec.StopAndClean()
        return 0 if ok else 1

    ok_all = True
    for first, n, stride in ROWS:
        poison(n)
        play(first, n, stride)
        ok = exact(first, n, stride)
        poison(n)
        shows(first, n, stride)
        ok &= exact(first, n, stride)
        times = {"play": [], "shows": []}
        for _ in range(args.reps):
            times["play"].append(play(first, n, stride))
            times["shows"].append(shows(first, n, stride))
        ok_all &= ok
        a, b = statistics.median(times["play"]), statistics.median(times["shows"])
        say({"first": first, "n": n, "stride": stride, "play_ms": round(a, 4), "shows_ms": round(b, 4),
             "play_ms_min": round(min(times["play"]), 4), "shows_ms_min": round(min(times["shows"]), 4),
             "play_ms_per_frame": round(a / n, 4), "shows_ms_per_frame": round(b / n, 4), "shows_over_play": round(b / a, 2),
             "written_gb_per_s_play": round(n * wl.W * wl.H * 4 / (a * 1e-3) / 1e9, 1), "play_below_shows": a < b,
             "digests_match": ok})
    say({"reps": args.reps, "device": torch.cuda.get_device_name(0), "store_rate_pool_gb_per_s": round(pool.store_rate, 1),
         "all_digests_match": ok_all})
    idx.close()
    pool.close()
    codec.StopAndClean()
    save()
    return 0 if ok_all else 1


if __name__ == "__main__":
    sys.exit(main())
