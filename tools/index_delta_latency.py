"""Thinning a clip with the inter frames that span the gaps of a seek index (jsp_index_delta_frames) against the only stream-level
alternative there was before it, on the two 512-frame 1080p MSVideo1 clips of tools/scrub_latency.py — msvideo1_16_1080p_inter70 and
the idle clip — for a stride-8 time-lapse (frames 0, 8, 16, ...):

  A   KeyFrame(0) and ONE DeltaFrames call for every gap (8 k, 8 k + 8]: per pair and block the last writer in the gap and the length
      of its code, or a skip; the frames gathered in device scratch in slices of pairs and copied to the host;
  B   one KeyFrame call per kept frame: an all-key clip.  B produces a DIFFERENT, larger file; it is the alternative only in that both
      are clips a decoder plays to the same pictures.

A and B alternate in one process, each measured with a host clock around calls that end synchronised; medians of --reps — once
through the Python methods (which allocate the host bytes they return) and once as the C calls alone into one host buffer that is
allocated and touched before the clock starts (`*_call_ms`).  A is first checked: a fresh codec decodes its frames one after the
other to the pictures Show gives.  There is no pass mark on time.  One JSON line per measurement.

  --volumes   no GPU needed: from the clip's bytes (which frame codes which block with a code of which length), the size of the
              thinned clip A writes, of the all-key clip B writes, and of the original frames they replace.

    python tools/index_delta_latency.py [--reps 5] [--clips inter70,idle] [--stride 8] [--parse gpu|host] [--out profiles/index_delta_latency.json]
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

from index_keyframe_latency import code_lengths   # noqa: E402
from index_play_latency import load_clips          # noqa: E402

RUN = 1023   # a skip word's count has 10 bits: no skip word crosses a multiple of this


def skip_words(written):
    """The skip words of a frame whose blocks are written where `written` says so: a run head is block 0, a block behind a written
    one, or a multiple of 1023 (the rule: msv1_index_delta_kernels.hip)."""
    import numpy as np
    nb = len(written)
    i = np.arange(nb)
    before = np.concatenate(([True], written[:-1]))
    return int((~written & (before | (i % RUN == 0))).sum())


def volumes(frames, stride, w, h):
    """The thinned clip of A, the all-key clip of B and the original frames up to the last kept one, in bytes."""
    import numpy as np
    nb = (w // 4) * (h // 4)
    keep = list(range(0, len(frames), stride))
    length = np.zeros(nb, dtype=np.int64)        # per block: the length of its last writer's code
    since = np.zeros(nb, dtype=bool)             # per block: written since the last kept frame
    a_bytes = b_bytes = words = 0
    for t, f in enumerate(frames[:keep[-1] + 1]):
        L = code_lengths(nb, bytes(f))
        length = np.where(L > 0, L, length)
        since |= L > 0
        if t % stride:
            continue
        key = int(length.sum())
        b_bytes += key
        if t == 0:
            a_bytes += key
        else:
            k = skip_words(since)
            words += k
            a_bytes += int(length[since].sum()) + 2 * k
        since[:] = False
    original = sum(len(f) for f in frames[:keep[-1] + 1])
    return dict(stride=stride, kept_frames=len(keep), thinned_bytes=a_bytes, skip_words=words, all_key_bytes=b_bytes, original_bytes=original,
                all_key_over_thinned=round(b_bytes / max(a_bytes, 1), 2), original_over_thinned=round(original / max(a_bytes, 1), 2))


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
            say({"clip": name, **volumes(frames, args.stride, wl.W, wl.H)})
        save()
        return 0

    import ctypes as C

    import numpy as np
    import torch
    if not torch.cuda.is_available():
        print("index_delta_latency: no GPU", file=sys.stderr)
        return 2
    from jsplayer_amd import FramePool, MSVideo1_16bit, player
    from jsplayer_amd import _native as N
    W, H = wl.W, wl.H
    pool = FramePool(W, H, 3)
    ok_all = True
    for name, frames, keys in load_clips(args.clips):
        c = MSVideo1_16bit(W, H)
        c.set_option("msv1_parse", args.parse)
        c.Preinit(player.INSIGNIFICANT_LINES)
        idx = c.BuildIndex(frames, keys)
        keep = list(range(0, idx.frames, args.stride))
        pairs = list(zip(keep, keep[1:]))

        def form_a():
            t0 = time.perf_counter()
            out = [idx.KeyFrame(keep[0])] + idx.DeltaFrames(pairs)   # (both return synchronised, the bytes on the host)
            return (time.perf_counter() - t0) * 1e3, out

        def form_b():
            t0 = time.perf_counter()
            out = [idx.KeyFrame(t) for t in keep]
            return (time.perf_counter() - t0) * 1e3, out

        _, thinned = form_a()
        _, all_key = form_b()
        # the C calls alone, into a host buffer that exists before the clock starts
        lib = N.lib()
        bound = idx.KeyFrameBound()
        room = np.full(max(sum(len(f) for f in thinned), sum(len(f) for f in all_key)) + bound, 0xA5, dtype=np.uint8)
        frm, to = (C.c_int * len(pairs))(*[a for a, _ in pairs]), (C.c_int * len(pairs))(*[b for _, b in pairs])
        lens, total, one = (C.c_size_t * len(pairs))(), C.c_size_t(0), C.c_size_t(0)

        def call_a():
            t0 = time.perf_counter()
            rc = lib.jsp_index_key_frame(c._h, idx._h, keep[0], C.c_void_p(room.ctypes.data), bound, C.byref(one))
            rc |= lib.jsp_index_delta_frames(c._h, idx._h, len(pairs), frm, to, C.c_void_p(room.ctypes.data + one.value), room.size - one.value,
                                             lens, C.byref(total))
            ms = (time.perf_counter() - t0) * 1e3
            if rc != 0:
                raise RuntimeError(N.last_error())
            return ms

        def call_b():
            at = 0
            t0 = time.perf_counter()
            for t in keep:
                if lib.jsp_index_key_frame(c._h, idx._h, t, C.c_void_p(room.ctypes.data + at), bound, C.byref(one)) != 0:
                    raise RuntimeError(N.last_error())
                at += one.value
            return (time.perf_counter() - t0) * 1e3

        call_a()
        same = room[:one.value + total.value].tobytes() == b"".join(thinned)
        call_b()
        # the check: a fresh codec plays A's frames to the pictures Show gives
        shown, a, b = pool.frames[:3]
        fresh = MSVideo1_16bit(W, H)
        fresh.Preinit(player.INSIGNIFICANT_LINES)
        ok = bool(fresh.IsKeyFrame(thinned[0])) and fresh.DecompressI(thinned[0], a) == 0
        for t, data in zip(keep[1:], thinned[1:]):
            prev = fresh.PreviousFrame()
            dst = b if prev is a else a
            dst.copy_(prev)
            fresh.DecompressP(data, dst)
            idx.Show(t, shown, adopt=False)
            ok = ok and bool(torch.equal(fresh.PreviousFrame(), shown))
        fresh.StopAndClean()
        ok = ok and same                                             # (and the C calls alone gave the same bytes)
        ok_all &= ok
        ta, tb, ca, cb = [], [], [], []
        for _ in range(args.reps):
            ta.append(form_a()[0])
            tb.append(form_b()[0])
            ca.append(call_a())
            cb.append(call_b())
        ma, mb = statistics.median(ta), statistics.median(tb)
        say({"clip": name, "stride": args.stride, "kept_frames": len(keep), "delta_frames_ms": round(ma, 3), "key_frame_per_kept_frame_ms": round(mb, 3),
             "delta_frames_ms_min": round(min(ta), 3), "key_frame_per_kept_frame_ms_min": round(min(tb), 3), "b_over_a": round(mb / ma, 2),
             "delta_frames_call_ms": round(statistics.median(ca), 3), "key_frame_per_kept_frame_call_ms": round(statistics.median(cb), 3),
             "call_b_over_a": round(statistics.median(cb) / statistics.median(ca), 2),
             "thinned_bytes": sum(len(f) for f in thinned), "all_key_bytes": sum(len(f) for f in all_key),
             "original_bytes": sum(len(f) for f in frames[:keep[-1] + 1]), "index_device_bytes": idx.device_bytes, "results_match": ok})
        idx.close()
        c.StopAndClean()
    say({"parse": args.parse, "reps": args.reps, "device": torch.cuda.get_device_name(0), "all_results_match": ok_all})
    pool.close()
    save()
    return 0 if ok_all else 1


if __name__ == "__main__":
    sys.exit(main())
