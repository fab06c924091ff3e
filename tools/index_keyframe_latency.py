"""A key frame for any frame of a seek index (jsp_index_key_frame) against the start of the route it replaces, on the two 512-frame
1080p MSVideo1 clips of tools/scrub_latency.py — msvideo1_16_1080p_inter70 and the idle clip:

  A   ONE KeyFrame(t): per block the last writer <= t and the length of its code, the codes gathered in block order in device
      scratch, the frame's bytes copied to the host — two launches, no pixel decoded;
  B   Show(t) into a frame buffer and jsp_download of that picture: what a caller without A has to do before a CPU encoder can
      start.  B is only a LOWER BOUND of the alternative: it leaves out the encoder, which would have to guess codes from pixels,
      for a format whose encoder neither the reference nor this project has;

for t near the start, the middle and the end of the clip.  A and B alternate in one process, each measured with a host clock around
calls that end synchronised; medians of --reps.  Every A is first checked: a fresh codec decodes its bytes as a key frame to the
picture Show(t) gives.  A frame the index cannot cut is reported as such (its row has the library's text and no time of A).  One JSON
line per measurement.

  --volumes   no GPU needed: from the clip's bytes (which frame codes which block with a code of which length), the bytes A and B
              read, write and send over the bus per row.

    python tools/index_keyframe_latency.py [--reps 5] [--clips inter70,idle] [--parse gpu|host] [--out profiles/index_keyframe_latency.json]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from index_play_latency import CODE_BYTES, RECORD_BYTES, SCAN, load_clips   # noqa: E402

WG_BLOCKS = 1024   # blocks a workgroup of the two kernels owns (MSV1_KEYFRAME_WG_BLOCKS)


def picks(nf):
    return sorted({min(3, nf - 1), nf // 2, nf - 1})


def code_lengths(nb, src):
    """Per block of a 16-bit frame: the length of its code (2, 6 or 18), 0 where the frame does not code the block (the control flow
    of MSVideo1.hx:106-209; the bench clips have no damaged frame)."""
    import numpy as np
    out = np.zeros(nb, dtype=np.int8)
    n = len(src)
    si = blk = 0
    while blk < nb and si + 1 < n:
        a, b = src[si], src[si + 1]
        si += 2
        if (b & 0xFC) == 0x84:
            blk += max(((b - 0x84) << 8) + a, 1)
            continue
        if b < 0x80:
            eight = si + 1 < n and bool(src[si + 1] & 0x80)
            si += 16 if eight else 4
            out[blk] = 18 if eight else 6
        else:
            out[blk] = 2
        blk += 1
    return out


def volumes(frames, ts, w, h):
    """Per t: the bytes ONE KeyFrame reads, writes and sends to the host, and the bytes Show + download do."""
    import numpy as np
    nb = (w // 4) * (h // 4)
    picture = w * h * 4
    groups = -(-nb // WG_BLOCKS)
    last = np.full(nb, -1, dtype=np.int64)
    length = np.zeros(nb, dtype=np.int64)
    out = []
    for t, f in enumerate(frames[:max(ts) + 1]):
        L = code_lengths(nb, bytes(f))
        last = np.where(L > 0, t, last)
        length = np.where(L > 0, L, length)
        if t not in ts:
            continue
        wt = t >> 5
        steps = -(-(wt - np.where(last >= 0, last >> 5, 0)) // SCAN)
        words = int((1 + np.minimum(SCAN * steps, wt)).sum())
        have = int((last >= 0).sum())
        size = int(length.sum())
        a = dict(read_bytes=words * 4 + have * (4 + RECORD_BYTES + 4) + nb * 8 + have * (4 + RECORD_BYTES) + size + groups * 4 * (groups + 1) // 2 + size,
                 written_bytes=nb * 8 + groups * 4 + size + 8, to_host_bytes=size + 8)
        b = dict(read_bytes=words * 4 + have * (4 + CODE_BYTES + RECORD_BYTES) + picture, written_bytes=picture, to_host_bytes=picture)
        out.append(dict(t=t, key_frame_bytes=size, blocks_without_writer=nb - have, key_frame=a, show_and_download=b,
                        bytes_moved_b_over_a=round(sum(b.values()) / max(sum(a.values()), 1), 1)))
    return out


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
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
            for rec in volumes(frames, picks(len(frames)), wl.W, wl.H):
                say({"clip": name, **rec})
        save()
        return 0

    import numpy as np
    import torch
    if not torch.cuda.is_available():
        print("index_keyframe_latency: no GPU", file=sys.stderr)
        return 2
    from jsplayer_amd import CodecError, FramePool, MSVideo1_16bit, player
    from jsplayer_amd import _native as N
    W, H = wl.W, wl.H
    lib = N.lib()
    pool = FramePool(W, H, 3)
    host = np.empty(W * H, dtype=np.int32)
    ok_all = True
    for name, frames, keys in load_clips(args.clips):
        c = MSVideo1_16bit(W, H)
        c.set_option("msv1_parse", args.parse)
        c.Preinit(player.INSIGNIFICANT_LINES)
        idx = c.BuildIndex(frames, keys)
        dst, other = [b for b in pool.frames[:3] if b is not c.PreviousFrame()][:2]

        def form_a(t):
            t0 = time.perf_counter()
            kf = idx.KeyFrame(t)                               # (returns synchronised, the bytes on the host)
            return (time.perf_counter() - t0) * 1e3, kf

        def form_b(t):
            t0 = time.perf_counter()
            idx.Show(t, dst, adopt=False)
            if lib.jsp_download(C.c_void_p(dst.data_ptr()), C.c_void_p(host.ctypes.data), W * H) != 0:
                raise RuntimeError(N.last_error())
            return (time.perf_counter() - t0) * 1e3

        for t in picks(idx.frames):
            try:
                _, kf = form_a(t)
            except CodecError as e:
                say({"clip": name, "t": t, "refused": str(e), "show_and_download_ms": round(statistics.median(form_b(t) for _ in range(args.reps)), 4)})
                continue
            form_b(t)
            fresh = MSVideo1_16bit(W, H)                       # the check: the bytes are a key frame that decodes to Show's picture
            fresh.Preinit(player.INSIGNIFICANT_LINES)
            ok = bool(fresh.IsKeyFrame(kf)) and fresh.DecompressI(kf, other) == 0 and bool(torch.equal(other, dst))
            fresh.StopAndClean()
            ok_all &= ok
            ta, tb = [], []
            for _ in range(args.reps):
                ta.append(form_a(t)[0])
                tb.append(form_b(t))
            a, b = statistics.median(ta), statistics.median(tb)
            say({"clip": name, "t": t, "key_frame_ms": round(a, 4), "show_and_download_ms": round(b, 4), "key_frame_ms_min": round(min(ta), 4),
                 "show_and_download_ms_min": round(min(tb), 4), "b_over_a": round(b / a, 2), "a_below_b": a < b, "key_frame_bytes": len(kf),
                 "picture_bytes": W * H * 4, "index_device_bytes": idx.device_bytes, "results_match": ok})
        idx.close()
        c.StopAndClean()
    say({"parse": args.parse, "reps": args.reps, "device": torch.cuda.get_device_name(0), "all_results_match": ok_all})
    pool.close()
    save()
    return 0 if ok_all else 1


if __name__ == "__main__":
    sys.exit(main())
