"""Skip-stills latency on a generated 1080p idle clip (16-bit MSVideo1): a key frame, then an idle stretch of L frames — all-skip
frames of both early-out sizes and longer, blocks recoded with the colour they already hold (stage 1 says yes, only the pixel
compare says no), changes only above line 36 — then a real change and 8 idle frames more.  The wall time from "frame 0 is
shown" to "the change is shown" by

  find        ONE FindChange call over frames 1 .. the clip's end, as Manager.skip_stills makes it (jsp_find_change: the range
              staged, one scan launch, the prefix up to the change staged again for the codec state, one compose launch);
  find_exact  the same call over frames 1 .. the change only (the hit is the range's last frame: nothing is staged twice);
  sequential  per-frame DecompressP calls into a three-buffer pool until one reports significant_changes (Manager.worker);
  pipelined   Manager.play_pipelined with 4 frames in flight over frames 0..L+1 (frame 0 included);

each measured with a host clock around a call that ends synchronised, in one process, the four alternating, for L in
{16, 64, 256, 511}.  The landing picture's digest must equal the sequential one.  Prints one JSON line per L and a summary.

    python tools/skip_stills_latency.py [--reps 5] [--stretches 16,64,256,511] [--parse gpu|host]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W, H = 1920, 1080
NBX, NBY = W // 4, H // 4
NB = NBX * NBY


def _solid(v):
    return bytes([v & 0xFF, 0x80 | (v >> 8)])


def _encode(codes):
    out, run = bytearray(), 0
    for c in codes + [b""]:
        if c is None:
            run += 1
            continue
        while run:
            k = min(run, 1023)
            out += bytes([k & 0xFF, 0x84 + (k >> 8)])
            run -= k
        out += c
    return bytes(out)


def idle_clip(stretch, seed=0, tail=8):
    """Frame 0 key; frames 1..stretch idle; frame stretch + 1 a real change; `tail` idle frames after it.  Key flags alongside."""
    rng = np.random.default_rng(seed)
    col = [int(v) for v in rng.integers(0, 0x8000, size=NB)]
    col = [v if (v >> 10) != 1 else v ^ 0x0400 for v in col]   # (a solid code must not read as a skip code)
    frames = [_encode([_solid(v) for v in col])]
    for j in range(stretch):
        kind = j % 5
        if kind == 0:
            frames.append(b"")                                  # empty: early-out
        elif kind == 1:
            frames.append(bytes([0x10, 0x84]))                  # short all-skip: early-out
        elif kind == 2:
            frames.append(_encode([None] * NB))                 # all-skip covering the picture
        elif kind == 3:                                         # a repaint: 5 % of the blocks recoded with their own colour
            codes = [None] * NB
            for b in rng.choice(NB, size=NB // 20, replace=False):
                codes[int(b)] = _solid(col[int(b)])
            frames.append(_encode(codes))
        else:                                                   # a change above line 36 only (block rows 0..8)
            codes = [None] * NB
            for b in rng.choice(NBX * 9, size=64, replace=False):
                col[int(b)] = (col[int(b)] + 7) & 0x3FF
                codes[int(b)] = _solid(col[int(b)])
            frames.append(_encode(codes))
    codes = [None] * NB
    for b in range(NB - NBX, NB):                               # the change: the last block row
        col[b] = (col[b] + 9) & 0x3FF
        codes[b] = _solid(col[b])
    frames.append(_encode(codes))
    frames += [_encode([None] * NB)] * tail
    return frames, [True] + [False] * (len(frames) - 1)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--stretches", default="16,64,256,511")
    ap.add_argument("--parse", default="gpu", choices=["gpu", "host"])
    args = ap.parse_args()

    import torch
    from jsplayer_amd import MSVideo1_16bit, player
    from jsplayer_amd import workloads as wl
    from jsplayer_amd.avi import CODEC_MSVC16, VideoInfo

    n = W * H

    def codec():
        c = MSVideo1_16bit(W, H)
        c.set_option("msv1_parse", args.parse)
        c.Preinit(player.INSIGNIFICANT_LINES)
        return c

    finder, seq = codec(), codec()
    find_bufs = [torch.zeros(n, dtype=torch.int32, device="cuda") for _ in range(2)]
    seq_bufs = [torch.zeros(n, dtype=torch.int32, device="cuda") for _ in range(3)]

    def run_find(frames, keys, upto=None):
        finder.DecompressI(frames[0], find_bufs[0])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = finder.FindChange(frames[1:upto], find_bufs[1], keys[1:upto], key_before=frames[0])
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3
        assert res.changed and res.index == change - 1, res.index
        return ms, res.data_pnt

    def run_sequential(frames, keys):
        seq.DecompressI(frames[0], seq_bufs[0])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(1, len(frames)):
            dst = next(b for b in seq_bufs if b is not seq.PreviousFrame())
            if seq.DecompressP(frames[i], dst).significant_changes:
                break
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3
        assert i == change, i
        return ms, seq.PreviousFrame()

    def run_pipelined(frames, keys):
        frames, keys = frames[:change + 1], keys[:change + 1]
        vi = VideoInfo(X=W, Y=H, bpp=16, fps=15.0, nframes=len(frames), codec=CODEC_MSVC16, palette=None, riff_size=0)
        dec = codec()
        mgr = player.Manager(vi, dec, lambda k: torch.zeros(k, dtype=torch.int32, device="cuda"), num_buffers=player.NUM_BUFFERS + 4)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        log = mgr.play_pipelined(frames, depth=4, key_flags=keys)
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3
        assert [d.index for d in log[1:] if d.significant_changes] == [len(frames) - 1]
        pic = mgr.buffers[log[-1].buffer_index].clone()
        dec.StopAndClean()
        return ms, pic

    stretches = [int(s) for s in args.stretches.split(",")]
    clips = {s: idle_clip(s, seed=s) for s in stretches}
    change = max(stretches) + 1
    run_find(*clips[max(stretches)])          # warm-up: the staging buffers reach their size for the longest range
    change = min(stretches) + 1
    run_sequential(*clips[min(stretches)])
    run_pipelined(*clips[min(stretches)])

    rows = []
    for s in stretches:
        frames, keys = clips[s]
        change = s + 1
        times = {"find": [], "find_exact": [], "sequential": [], "pipelined": []}
        digests = {}
        for _ in range(args.reps):
            for mode, fn in (("find", run_find), ("find_exact", lambda f, k: run_find(f, k, change + 1)),
                             ("sequential", run_sequential), ("pipelined", run_pipelined)):
                ms, pic = fn(frames, keys)
                times[mode].append(ms)
                digests.setdefault(mode, set()).add(wl.digest(pic.cpu().numpy()))
        ok = len(digests["find"]) == 1 and digests["find"] == digests["find_exact"] == digests["sequential"] == digests["pipelined"]
        row = {"idle_frames": s, "landing": change, "range_frames": len(frames) - 1, "range_stream_bytes": sum(len(f) for f in frames[1:]),
               **{f"{m}_ms": round(statistics.median(v), 3) for m, v in times.items()},
               **{f"{m}_ms_min": round(min(v), 3) for m, v in times.items()},
               "digest": sorted(digests["find"])[0], "digest_matches_sequential": ok}
        rows.append(row)
        print(json.dumps(row), flush=True)
    print(json.dumps({"clip": "generated 1080p idle", "parse": args.parse, "reps": args.reps, "device": torch.cuda.get_device_name(0),
                      "all_digests_match": all(r["digest_matches_sequential"] for r in rows)}), flush=True)
    for c in (finder, seq):
        c.StopAndClean()
    return 0 if all(r["digest_matches_sequential"] for r in rows) else 1


if __name__ == "__main__":
    sys.exit(main())
