"""A clip played backwards out of a seek index (jsp_index_path_frames) against the same frames forward (jsp_index_crop_frames), on the
two 512-frame 1080p MSVideo1 clips of tools/scrub_latency.py — msvideo1_16_1080p_inter70 and the idle clip — for every 8th frame
(frames 0, 8, 16, ...) of the whole picture (480 x 270 blocks):

  A   ONE jsp_index_path_frames call for the steps back (8 k + 8 -> 8 k), loose and tight (`back_*`), and one for the whole reversed
      clip, the key pair at the last kept frame in front of them (`reverse_clip_*`);
  B   ONE jsp_index_crop_frames call for the same frames forward, the gaps (8 k, 8 k + 8], loose and tight (`forward_*`).

A and B alternate in one process, each measured with a host clock around C calls that end synchronised, into one host buffer that is
allocated and touched before the clock starts; medians of --reps behind one untimed call.  A is first checked: a fresh codec decodes
the reversed clip's frames one after the other to the pictures Show gives.  There is no pass mark on time: a step back walks the
writer bitmap twice per block and is expected to be slower than the step forward, and the numbers say so.  One JSON line per
measurement.

  --volumes   no GPU needed: from the clip's bytes (which frame codes which block with which code), the size of the reversed clip,
              loose and tight, of the same frames forward (DeltaFrames) and of the all-key clip of the same frames — today's only
              way to a reversed clip.

    python tools/index_path_latency.py [--reps 5] [--clips inter70,idle] [--stride 8] [--parse gpu|host]
                                       [--out profiles/index_path_latency.json]
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
from index_play_latency import load_clips           # noqa: E402
from index_tight_latency import parse, pixels       # noqa: E402

KEY = -2     # JSP_CROP_KEY
TIGHT = 1    # JSP_CROP_TIGHT


def volumes(frames, stride, w, h):
    """The reversed clip (loose, tight), the same frames forward and the all-key clip of the same frames, in bytes.  A step back from
    kept frame k to the one before it codes the blocks written in between with the codes they had at the EARLIER frame."""
    import numpy as np
    nb = (w // 4) * (h // 4)
    keep = list(range(0, len(frames), stride))
    length = np.zeros(nb, dtype=np.int64)             # per block: the length of its last writer's code ...
    code = np.zeros((nb, 18), dtype=np.uint8)         # ... and its bytes
    earlier = np.zeros(nb, dtype=np.int64)            # per block: that length at the last kept frame
    shown = np.zeros((nb, 16), dtype=np.int64)        # per block: its pixels at the last kept frame
    since = np.zeros(nb, dtype=bool)                  # per block: written since the last kept frame
    loose = tight = forward = all_key = touched = dropped = 0
    key = 0
    for t, f in enumerate(frames[:keep[-1] + 1]):
        src = np.frombuffer(bytes(f) + bytes(18), dtype=np.uint8)
        L, o = parse(nb, bytes(f))
        w_now = L > 0
        length = np.where(w_now, L, length)
        code[w_now] = src[o[w_now, None] + np.arange(18)]
        since |= w_now
        if t % stride:
            continue
        key = int(length.sum())
        all_key += key
        now = pixels(code[since], length[since])
        if t == 0:
            forward += key
        else:
            kept = since.copy()
            kept[since] = np.any(now != shown[since], axis=1)
            forward += int(length[since].sum()) + 2 * skip_words(since)
            loose += int(earlier[since].sum()) + 2 * skip_words(since)
            tight += int(earlier[kept].sum()) + 2 * skip_words(kept)
            touched += int(since.sum())
            dropped += int(since.sum() - kept.sum())
        shown[since] = now
        earlier = length.copy()
        since[:] = False
    loose += key                                      # the reversed clip starts with the key frame of the LAST kept frame
    tight += key
    return dict(stride=stride, kept_frames=len(keep), reverse_bytes=loose, reverse_tight_bytes=tight, forward_bytes=forward,
                all_key_bytes=all_key, touched_blocks=touched, dropped_blocks=dropped,
                all_key_over_reverse=round(all_key / max(loose, 1), 2), all_key_over_reverse_tight=round(all_key / max(tight, 1), 2),
                reverse_over_forward=round(loose / max(forward, 1), 4))


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--stride", type=int, default=8)
    ap.add_argument("--parse", default="gpu", choices=["gpu", "host"])
    ap.add_argument("--clips", default="inter70,idle")
    ap.add_argument("--volumes", action="store_true")
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    from jsplayer_amd import workloads as wl
    W, H = wl.W, wl.H
    bw, bh = W // 4, H // 4
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
            say({"clip": name, **volumes(frames, args.stride, W, H)})
        save()
        return 0

    import ctypes as C

    import numpy as np
    import torch
    if not torch.cuda.is_available():
        print("index_path_latency: no GPU", file=sys.stderr)
        return 2
    from jsplayer_amd import FramePool, MSVideo1_16bit, player
    from jsplayer_amd import _native as N
    pool = FramePool(W, H, 3)
    ok_all = True
    for name, frames, keys in load_clips(args.clips):
        c = MSVideo1_16bit(W, H)
        c.set_option("msv1_parse", args.parse)
        c.Preinit(player.INSIGNIFICANT_LINES)
        idx = c.BuildIndex(frames, keys)
        keep = list(range(0, idx.frames, args.stride))
        gaps = list(zip(keep, keep[1:]))
        backs = [(b, a) for a, b in gaps][::-1]
        clip_pairs = [(KEY, keep[-1])] + backs
        reversed_clip, flags = idx.PathFrames(None, clip_pairs)
        tight_clip, _ = idx.PathFrames(None, clip_pairs, tight=True)
        forward, _ = idx.CropFrames((0, 0, bw, bh), gaps)
        lib = N.lib()
        room = np.full(max(sum(len(f) for f in reversed_clip), sum(len(f) for f in forward)) + 64, 0xA5, dtype=np.uint8)
        total = C.c_size_t(0)

        def arrays(pairs):
            n = len(pairs)
            return n, (C.c_int * n)(*[a for a, _ in pairs]), (C.c_int * n)(*[b for _, b in pairs]), (C.c_size_t * n)(), (C.c_int * n)()

        def call(fn, a, flags):
            n, frm, to, lens, ks = a
            t0 = time.perf_counter()
            rc = fn(c._h, idx._h, 0, 0, bw, bh, n, frm, to, flags, C.c_void_p(room.ctypes.data), room.size, lens, ks, C.byref(total))
            ms = (time.perf_counter() - t0) * 1e3
            if rc != 0:
                raise RuntimeError(N.last_error())
            return ms

        gap_args, back_args, clip_args = arrays(gaps), arrays(backs), arrays(clip_pairs)
        call(lib.jsp_index_path_frames, clip_args, 0)
        same = room[:total.value].tobytes() == b"".join(reversed_clip)
        call(lib.jsp_index_path_frames, gap_args, 0)            # forward pairs through the path call: crop's bytes
        same = same and room[:total.value].tobytes() == b"".join(forward)
        # the check: a fresh codec plays the reversed clips, loose and tight, to the pictures Show gives
        shown, a, b = pool.frames[:3]
        ok = same and all(len(x) <= len(y) for x, y in zip(tight_clip, reversed_clip))
        for made in (reversed_clip, tight_clip):
            fresh = MSVideo1_16bit(4 * bw, 4 * bh)
            fresh.Preinit(player.INSIGNIFICANT_LINES)
            ok = ok and bool(fresh.IsKeyFrame(made[0])) and flags[0] and fresh.DecompressI(made[0], a) == 0
            for k, (t, data) in enumerate(zip(keep[::-1], made)):
                if k > 0:
                    prev = fresh.PreviousFrame()
                    dst = b if prev is a else a
                    dst.copy_(prev)
                    fresh.DecompressP(data, dst)
                idx.Show(t, shown, adopt=False)
                part = shown.view(H, W)[:4 * bh, :4 * bw]
                ok = ok and bool(torch.equal(fresh.PreviousFrame().view(4 * bh, 4 * bw), part))
            fresh.StopAndClean()
        ok_all &= ok
        t = {k: [] for k in ("back", "back_tight", "reverse_clip", "forward", "forward_tight")}
        for _ in range(args.reps):
            t["back"].append(call(lib.jsp_index_path_frames, back_args, 0))
            t["forward"].append(call(lib.jsp_index_crop_frames, gap_args, 0))
            t["back_tight"].append(call(lib.jsp_index_path_frames, back_args, TIGHT))
            t["forward_tight"].append(call(lib.jsp_index_crop_frames, gap_args, TIGHT))
            t["reverse_clip"].append(call(lib.jsp_index_path_frames, clip_args, 0))
        med = statistics.median
        say({"clip": name, "stride": args.stride, "kept_frames": len(keep), "pairs": len(gaps),
             "back_call_ms": round(med(t["back"]), 3), "forward_call_ms": round(med(t["forward"]), 3),
             "back_over_forward": round(med(t["back"]) / med(t["forward"]), 2),
             "back_tight_call_ms": round(med(t["back_tight"]), 3), "forward_tight_call_ms": round(med(t["forward_tight"]), 3),
             "back_tight_over_forward_tight": round(med(t["back_tight"]) / med(t["forward_tight"]), 2),
             "reverse_clip_call_ms": round(med(t["reverse_clip"]), 3),
             "back_call_ms_min": round(min(t["back"]), 3), "forward_call_ms_min": round(min(t["forward"]), 3),
             "reverse_clip_bytes": sum(len(f) for f in reversed_clip), "reverse_tight_clip_bytes": sum(len(f) for f in tight_clip),
             "forward_frames_bytes": sum(len(f) for f in forward), "index_device_bytes": idx.device_bytes, "results_match": ok})
        idx.close()
        c.StopAndClean()
    say({"parse": args.parse, "reps": args.reps, "device": torch.cuda.get_device_name(0), "all_results_match": ok_all})
    pool.close()
    save()
    return 0 if ok_all else 1


if __name__ == "__main__":
    sys.exit(main())
