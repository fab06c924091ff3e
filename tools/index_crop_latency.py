"""Cropping a clip to a block rectangle of a seek index (jsp_index_crop_frames) against the full-picture call it is modelled on
(jsp_index_delta_frames), on the two 512-frame 1080p MSVideo1 clips of tools/scrub_latency.py — msvideo1_16_1080p_inter70 and the idle
clip — for a stride-8 time-lapse (frames 0, 8, 16, ...) of the 640 x 360 rectangle in the middle of the picture (160 x 90 of the
480 x 270 blocks):

  A   ONE CropFrames call for the gaps (8 k, 8 k + 8] of the rectangle (`crop_frames_*`), and one for the whole cropped clip, the key
      pair at frame 0 in front of them (`crop_clip_*`);
  B   ONE DeltaFrames call for the same gaps of the whole picture.  B produces a DIFFERENT, larger clip; it is what a region of a
      recording cost before: the whole picture or nothing.

A and B alternate in one process, each measured with a host clock around calls that end synchronised; medians of --reps — once
through the Python methods (which allocate the host bytes they return) and, in a loop of their own behind one untimed call, as the
C calls alone into one host buffer that is allocated and touched before the clock starts (`*_call_ms`).  A is first checked: a fresh
codec of the rectangle's size decodes its frames one after the other to that part of the pictures Show gives.  There is no pass mark
on time; a small rectangle can be SLOWER than the whole picture where launches and copies dominate, and the numbers say so.  One
JSON line per measurement.

  --volumes   no GPU needed: from the clip's bytes (which frame codes which block with a code of which length), the size of the
              cropped clip, of the full-picture thinned clip (DeltaFrames) and of the full-picture all-key clip.

    python tools/index_crop_latency.py [--reps 5] [--clips inter70,idle] [--stride 8] [--rect 640:360:640:360] [--parse gpu|host]
                                       [--out profiles/index_crop_latency.json]
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

from index_delta_latency import skip_words          # noqa: E402
from index_keyframe_latency import code_lengths    # noqa: E402
from index_play_latency import load_clips           # noqa: E402

KEY = -2   # JSP_CROP_KEY


def block_rect(rect, w, h):
    """Manager.crop_rect's arithmetic: the smallest block rectangle (table order) that contains the display rectangle."""
    x, y, rw, rh = rect
    nbx, nby = w // 4, h // 4
    x0, x1 = max(x, 0), min(x + rw, 4 * nbx)
    s0, s1 = max(h - (y + rh), 0), min(h - y, 4 * nby)
    if x0 >= x1 or s0 >= s1:
        raise SystemExit("index_crop_latency: nothing of the rectangle lies in the picture's blocks")
    bx, by = x0 // 4, s0 // 4
    return bx, by, (x1 + 3) // 4 - bx, (s1 + 3) // 4 - by


def volumes(frames, stride, w, h, blocks):
    """The cropped clip, the full-picture thinned clip and the full-picture all-key clip up to the last kept frame, in bytes."""
    import numpy as np
    nbx, nby = w // 4, h // 4
    nb = nbx * nby
    bx, by, bw, bh = blocks
    inside = (np.arange(by, by + bh)[:, None] * nbx + np.arange(bx, bx + bw)[None, :]).reshape(-1)   # src(j), j ascending
    keep = list(range(0, len(frames), stride))
    length = np.zeros(nb, dtype=np.int64)        # per block: the length of its last writer's code
    since = np.zeros(nb, dtype=bool)             # per block: written since the last kept frame
    crop = thinned = all_key = crop_words = 0
    for t, f in enumerate(frames[:keep[-1] + 1]):
        L = code_lengths(nb, bytes(f))
        length = np.where(L > 0, L, length)
        since |= L > 0
        if t % stride:
            continue
        all_key += int(length.sum())
        if t == 0:
            thinned += int(length.sum())
            crop += int(length[inside].sum())
        else:
            thinned += int(length[since].sum()) + 2 * skip_words(since)
            k = skip_words(since[inside])        # (run heads and multiples of 1023 in the rectangle's numbering)
            crop_words += k
            crop += int(length[inside][since[inside]].sum()) + 2 * k
        since[:] = False
    return dict(stride=stride, kept_frames=len(keep), rect_blocks=list(blocks), crop_bytes=crop, crop_skip_words=crop_words,
                thinned_bytes=thinned, all_key_bytes=all_key, thinned_over_crop=round(thinned / max(crop, 1), 2),
                all_key_over_crop=round(all_key / max(crop, 1), 2), area_over_crop_area=round(nb / (bw * bh), 2))


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--stride", type=int, default=8)
    ap.add_argument("--rect", default="640:360:640:360")
    ap.add_argument("--parse", default="gpu", choices=["gpu", "host"])
    ap.add_argument("--clips", default="inter70,idle")
    ap.add_argument("--volumes", action="store_true")
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    from jsplayer_amd import workloads as wl
    W, H = wl.W, wl.H
    blocks = block_rect(tuple(int(v) for v in args.rect.split(":")), W, H)
    bx, by, bw, bh = blocks
    lines = []

    def say(rec):
        lines.append(rec)
        print(json.dumps(rec), flush=True)

    def save():
        if args.out:
            with open(args.out, "w") as f:
                json.dump(lines, f, indent=1)

    if args.volumes:
        for name, frames, _ in load_clips(args.clips):
            say({"clip": name, **volumes(frames, args.stride, W, H, blocks)})
        save()
        return 0

    import ctypes as C

    import numpy as np
    import torch
    if not torch.cuda.is_available():
        print("index_crop_latency: no GPU", file=sys.stderr)
        return 2
    from jsplayer_amd import FramePool, MSVideo1_16bit, player
    from jsplayer_amd import _native as N
    pool = FramePool(W, H, 1)
    small = FramePool(4 * bw, 4 * bh, 2)
    ok_all = True
    for name, frames, keys in load_clips(args.clips):
        c = MSVideo1_16bit(W, H)
        c.set_option("msv1_parse", args.parse)
        c.Preinit(player.INSIGNIFICANT_LINES)
        idx = c.BuildIndex(frames, keys)
        keep = list(range(0, idx.frames, args.stride))
        gaps = list(zip(keep, keep[1:]))
        clip_pairs = [(KEY, keep[0])] + gaps

        def timed(fn):
            t0 = time.perf_counter()
            out = fn()
            return (time.perf_counter() - t0) * 1e3, out

        _, (cropped, flags) = timed(lambda: idx.CropFrames(blocks, clip_pairs))
        _, full = timed(lambda: idx.DeltaFrames(gaps))
        # the C calls alone, into a host buffer that exists before the clock starts
        lib = N.lib()
        room = np.full(max(sum(len(f) for f in cropped), sum(len(f) for f in full)) + 64, 0xA5, dtype=np.uint8)

        def arrays(pairs):
            n = len(pairs)
            return n, (C.c_int * n)(*[a for a, _ in pairs]), (C.c_int * n)(*[b for _, b in pairs]), (C.c_size_t * n)(), (C.c_int * n)()

        gap_args, clip_args = arrays(gaps), arrays(clip_pairs)
        total = C.c_size_t(0)

        def call_crop(a):
            n, frm, to, lens, ks = a
            t0 = time.perf_counter()
            rc = lib.jsp_index_crop_frames(c._h, idx._h, bx, by, bw, bh, n, frm, to, 0, C.c_void_p(room.ctypes.data), room.size, lens, ks,
                                           C.byref(total))
            ms = (time.perf_counter() - t0) * 1e3
            if rc != 0:
                raise RuntimeError(N.last_error())
            return ms

        def call_delta():
            n, frm, to, lens, _ = gap_args
            t0 = time.perf_counter()
            rc = lib.jsp_index_delta_frames(c._h, idx._h, n, frm, to, C.c_void_p(room.ctypes.data), room.size, lens, C.byref(total))
            ms = (time.perf_counter() - t0) * 1e3
            if rc != 0:
                raise RuntimeError(N.last_error())
            return ms

        call_crop(clip_args)
        same = room[:total.value].tobytes() == b"".join(cropped)
        call_delta()
        same = same and room[:total.value].tobytes() == b"".join(full)
        # the check: a fresh codec of the rectangle's size plays the cropped clip to that part of the pictures Show gives
        shown = pool.frames[0]
        a, b = small.frames[:2]
        fresh = MSVideo1_16bit(4 * bw, 4 * bh)
        fresh.Preinit(player.INSIGNIFICANT_LINES)
        ok = bool(fresh.IsKeyFrame(cropped[0])) and flags[0] and fresh.DecompressI(cropped[0], a) == 0
        for k, (t, data) in enumerate(zip(keep, cropped)):
            if k > 0:
                prev = fresh.PreviousFrame()
                dst = b if prev is a else a
                dst.copy_(prev)
                fresh.DecompressP(data, dst)
            idx.Show(t, shown, adopt=False)
            part = shown.view(H, W)[4 * by:4 * by + 4 * bh, 4 * bx:4 * bx + 4 * bw]
            ok = ok and bool(torch.equal(fresh.PreviousFrame().view(4 * bh, 4 * bw), part))
        fresh.StopAndClean()
        ok = ok and same                                             # (and the C calls alone gave the same bytes)
        ok_all &= ok
        tg, tc, td, cg, cc_, cd = [], [], [], [], [], []
        for _ in range(args.reps):                                   # the Python methods: A, A with its key pair, B
            tg.append(timed(lambda: idx.CropFrames(blocks, gaps))[0])
            tc.append(timed(lambda: idx.CropFrames(blocks, clip_pairs))[0])
            td.append(timed(lambda: idx.DeltaFrames(gaps))[0])
        call_crop(gap_args)                                          # (untimed: the first C call behind the methods' large host buffers)
        for _ in range(args.reps):                                   # the C calls alone, in a loop of their own
            cg.append(call_crop(gap_args))
            cc_.append(call_crop(clip_args))
            cd.append(call_delta())
        med = statistics.median
        say({"clip": name, "stride": args.stride, "kept_frames": len(keep), "rect_blocks": list(blocks),
             "crop_frames_call_ms": round(med(cg), 3), "crop_clip_call_ms": round(med(cc_), 3), "delta_frames_call_ms": round(med(cd), 3),
             "call_delta_over_crop": round(med(cd) / med(cg), 2),
             "crop_frames_ms": round(med(tg), 3), "crop_clip_ms": round(med(tc), 3), "delta_frames_ms": round(med(td), 3),
             "delta_over_crop": round(med(td) / med(tg), 2),
             "crop_frames_call_ms_min": round(min(cg), 3), "delta_frames_call_ms_min": round(min(cd), 3),
             "crop_clip_bytes": sum(len(f) for f in cropped), "delta_frames_bytes": sum(len(f) for f in full),
             "index_device_bytes": idx.device_bytes, "results_match": ok})
        idx.close()
        c.StopAndClean()
    say({"parse": args.parse, "reps": args.reps, "device": torch.cuda.get_device_name(0), "all_results_match": ok_all})
    pool.close()
    small.close()
    save()
    return 0 if ok_all else 1


if __name__ == "__main__":
    sys.exit(main())
