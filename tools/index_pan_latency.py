"""Panning a crop across a clip (jsp_index_pan_frames) on the two 512-frame 1080p MSVideo1 clips of tools/index_crop_latency.py —
msvideo1_16_1080p_inter70 and the idle clip — for a stride-8 time-lapse (frames 0, 8, 16, ...) of a 640 x 360 rectangle (160 x 90 of
the 480 x 270 blocks) on a path that moves at EVERY kept frame:

  bytes   the panned clip with JSP_CROP_TIGHT (a frame behind a move codes only the blocks that differ from the block that stood at
          the same place of the rectangle before) against the clip a caller had to write before: a rectangle key frame at every
          move (the same call without the flag);
  time    ONE C call for the whole panned clip, tight and not, into one host buffer that is allocated and touched before the clock
          starts; medians of --reps behind one untimed call;
  still   ONE jsp_index_pan_frames call of STILL pairs only — the 63 gaps of tools/index_crop_latency.py's rectangle in the middle
          of the picture, one origin throughout — beside jsp_index_crop_frames for the same pairs, alternating in one process
          (`pan_still_call_ms` / `crop_frames_call_ms`), and the same with JSP_CROP_TIGHT, the form a panned clip with still
          stretches runs (`pan_still_tight_call_ms` / `crop_frames_tight_call_ms`); the bytes of the two are compared.  The parent
          commit's figure for the plain pairs is `crop_frames_call_ms` of tools/index_crop_latency.py run there.

The panned clip is first checked: a fresh codec of the rectangle's size decodes its frames one after the other to the rectangles of
the pictures Show gives along the path.  There is no pass mark on time.  One JSON line per measurement.

    python tools/index_pan_latency.py [--reps 5] [--clips inter70,idle] [--stride 8] [--size 640x360] [--parse gpu|host]
                                      [--out profiles/index_pan_latency.json]
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

from index_crop_latency import block_rect           # noqa: E402
from index_play_latency import load_clips           # noqa: E402

KEY = -2   # JSP_CROP_KEY


def path_of(keep, nbx, nby, bw, bh):
    """An origin per kept frame that differs from the one before on both axes, inside the grid."""
    rx, ry = nbx - bw, nby - bh
    return [((37 * k) % (rx + 1), (23 * k) % (ry + 1)) for k in range(len(keep))]


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--stride", type=int, default=8)
    ap.add_argument("--size", default="640x360")
    ap.add_argument("--parse", default="gpu", choices=["gpu", "host"])
    ap.add_argument("--clips", default="inter70,idle")
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import ctypes as C

    import numpy as np
    import torch
    if not torch.cuda.is_available():
        print("index_pan_latency: no GPU", file=sys.stderr)
        return 2
    from jsplayer_amd import FramePool, MSVideo1_16bit, player
    from jsplayer_amd import _native as N
    from jsplayer_amd import workloads as wl
    W, H = wl.W, wl.H
    nbx, nby = W // 4, H // 4
    pw, ph = (int(v) for v in args.size.split("x"))
    bw, bh = min((pw + 3) // 4, nbx), min((ph + 3) // 4, nby)
    middle = block_rect((pw, ph, pw, ph), W, H)          # tools/index_crop_latency.py's rectangle, for the still pairs
    lines = []

    def say(rec):
        lines.append(rec)
        print(json.dumps(rec), flush=True)

    pool = FramePool(W, H, 1)
    small = FramePool(4 * bw, 4 * bh, 2)
    lib = N.lib()
    ok_all = True
    for name, frames, keys in load_clips(args.clips):
        c = MSVideo1_16bit(W, H)
        c.set_option("msv1_parse", args.parse)
        c.Preinit(player.INSIGNIFICANT_LINES)
        idx = c.BuildIndex(frames, keys)
        keep = list(range(0, idx.frames, args.stride))
        at = path_of(keep, nbx, nby, bw, bh)
        assert all(a != b for a, b in zip(at, at[1:]))
        pairs = [(KEY, keep[0], None, at[0])] + [(keep[k - 1], keep[k], at[k - 1], at[k]) for k in range(1, len(keep))]
        tight, tight_flags = idx.PanFrames((bw, bh), pairs, tight=True)
        loose, loose_flags = idx.PanFrames((bw, bh), pairs)
        # the check: a fresh codec of the rectangle's size plays the panned clip to the rectangles of the pictures Show gives
        shown = pool.frames[0]
        a, b = small.frames[:2]
        ok = all(loose_flags) and tight_flags[0]
        for clip in (tight, loose):
            fresh = MSVideo1_16bit(4 * bw, 4 * bh)
            fresh.Preinit(player.INSIGNIFICANT_LINES)
            ok = ok and fresh.DecompressI(clip[0], a) == 0
            for k, (t, data) in enumerate(zip(keep, clip)):
                if k > 0:
                    prev = fresh.PreviousFrame()
                    dst = b if prev is a else a
                    if fresh.IsKeyFrame(data):
                        ok = ok and fresh.DecompressI(data, dst) == 0
                    else:
                        dst.copy_(prev)
                        fresh.DecompressP(data, dst)
                idx.Show(t, shown, adopt=False)
                x, y = at[k]
                part = shown.view(H, W)[4 * y:4 * y + 4 * bh, 4 * x:4 * x + 4 * bw]
                ok = ok and bool(torch.equal(fresh.PreviousFrame().view(4 * bh, 4 * bw), part))
            fresh.StopAndClean()

        room = np.full(sum(len(f) for f in loose) + 64, 0xA5, dtype=np.uint8)
        total = C.c_size_t(0)

        def pan_args(ps):
            n = len(ps)
            flat = lambda k: (C.c_int * (2 * n))(*[v for p in ps for v in (p[k] if p[k] is not None else p[3])])   # noqa: E731
            return n, (C.c_int * n)(*[p[0] for p in ps]), (C.c_int * n)(*[p[1] for p in ps]), flat(2), flat(3), (C.c_size_t * n)(), (C.c_int * n)()

        def call_pan(a, flags):
            n, frm, to, fxy, txy, lens, ks = a
            t0 = time.perf_counter()
            rc = lib.jsp_index_pan_frames(c._h, idx._h, bw, bh, n, frm, to, fxy, txy, flags, C.c_void_p(room.ctypes.data), room.size, lens, ks,
                                          C.byref(total))
            ms = (time.perf_counter() - t0) * 1e3
            if rc != 0:
                raise RuntimeError(N.last_error())
            return ms

        gaps = list(zip(keep, keep[1:]))
        ng = len(gaps)
        crop_args = (ng, (C.c_int * ng)(*[g[0] for g in gaps]), (C.c_int * ng)(*[g[1] for g in gaps]), (C.c_size_t * ng)(), (C.c_int * ng)())

        def call_crop(flags=0):
            n, frm, to, lens, ks = crop_args
            t0 = time.perf_counter()
            rc = lib.jsp_index_crop_frames(c._h, idx._h, *middle, n, frm, to, flags, C.c_void_p(room.ctypes.data), room.size, lens, ks,
                                           C.byref(total))
            ms = (time.perf_counter() - t0) * 1e3
            if rc != 0:
                raise RuntimeError(N.last_error())
            return ms

        clip_args = pan_args(pairs)
        still_args = pan_args([(g[0], g[1], middle[:2], middle[:2]) for g in gaps])
        call_pan(clip_args, 1)
        ok = ok and room[:total.value].tobytes() == b"".join(tight)
        call_pan(still_args, 0)
        still_bytes = room[:total.value].tobytes()
        call_crop()
        ok = ok and room[:total.value].tobytes() == still_bytes
        call_pan(still_args, 1)
        still_tight_bytes = room[:total.value].tobytes()
        call_crop(1)
        ok = ok and room[:total.value].tobytes() == still_tight_bytes
        ok_all &= ok
        pt, pl, ps, cr, pst, crt = [], [], [], [], [], []
        for _ in range(args.reps):
            pt.append(call_pan(clip_args, 1))
            pl.append(call_pan(clip_args, 0))
        for _ in range(args.reps):                                   # still pairs through both calls, alternating
            ps.append(call_pan(still_args, 0))
            cr.append(call_crop())
        for _ in range(args.reps):                                   # the same with JSP_CROP_TIGHT: the sizes kernels that decode
            pst.append(call_pan(still_args, 1))
            crt.append(call_crop(1))
        med = statistics.median
        say({"clip": name, "stride": args.stride, "kept_frames": len(keep), "size_blocks": [bw, bh],
             "pan_tight_bytes": sum(len(f) for f in tight), "pan_key_at_every_move_bytes": sum(len(f) for f in loose),
             "key_over_tight": round(sum(len(f) for f in loose) / max(sum(len(f) for f in tight), 1), 2),
             "tight_frames_that_code_every_block": sum(tight_flags[1:]),
             "pan_tight_call_ms": round(med(pt), 3), "pan_loose_call_ms": round(med(pl), 3),
             "pan_still_call_ms": round(med(ps), 3), "crop_frames_call_ms": round(med(cr), 3),
             "pan_still_call_ms_all": [round(v, 3) for v in ps], "crop_frames_call_ms_all": [round(v, 3) for v in cr],
             "pan_still_tight_call_ms": round(med(pst), 3), "crop_frames_tight_call_ms": round(med(crt), 3),
             "pan_still_tight_call_ms_all": [round(v, 3) for v in pst], "crop_frames_tight_call_ms_all": [round(v, 3) for v in crt],
             "still_bytes": len(still_bytes), "still_tight_bytes": len(still_tight_bytes), "index_device_bytes": idx.device_bytes, "results_match": ok})
        idx.close()
        c.StopAndClean()
    say({"parse": args.parse, "reps": args.reps, "device": torch.cuda.get_device_name(0), "all_results_match": ok_all})
    pool.close()
    small.close()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(lines, f, indent=1)
    return 0 if ok_all else 1


if __name__ == "__main__":
    sys.exit(main())
