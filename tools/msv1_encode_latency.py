"""The MSVideo1 16-bit encoder (jsp_msv1_encode_frames) on pictures of the two 512-frame 1080p MSVideo1 clips of
tools/scrub_latency.py — msvideo1_16_1080p_inter70 and the idle clip — for 1, 8 and 64 pictures a call, key frames and inter frames
(each picture against the one before it), beside two calls measured in the same run on the same frames:

  download   jsp_download of the same pictures: the floor of any host-side encoder, the picture bytes over the bus;
  key_frame  jsp_index_key_frame of the same frames: the gather-only call of the same two-launch shape (it reads codes, not pixels).

The pictures are frames first, first + 1, ... of the clip's seek index, shown into device buffers before the clock starts.  Every
call is measured with a host clock around calls that end synchronised, into host buffers that exist before the clock starts; medians
of --reps.  The encoder is first checked: a fresh codec decodes its frames, one after the other, to the shown pictures (an MSVideo1
picture comes back exactly).  There is no pass mark on time.  One JSON line per measurement.

  --volumes   no GPU needed: per row the bytes the encoder reads (64 per block and picture, twice that for an inter frame), the
              bytes a download moves over the bus, the frames' bound, and — from the clip's bytes — the key frames the gather writes.

    python tools/msv1_encode_latency.py [--reps 5] [--clips inter70,idle] [--counts 1,8,64] [--first 200] [--out profiles/msv1_encode_latency.json]
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


def volumes(frames, first, n, w, h):
    """Bytes per row: read by the encoder, moved by a download, the frames at their bound, the gathered key frames."""
    import numpy as np
    nb = (w // 4) * (h // 4)
    length = np.zeros(nb, dtype=np.int64)
    gathered = 0
    for t, f in enumerate(frames[:first + n]):
        L = code_lengths(nb, bytes(f))
        length = np.where(L > 0, L, length)
        if t >= first:
            gathered += int(length.sum())
    picture = w * h * 4
    return dict(first=first, pictures=n, picture_bytes=n * picture, encode_key_reads=n * nb * 64, encode_inter_reads=2 * n * nb * 64,
                download_bytes=n * picture, frames_bound=n * nb * 18, scratch_per_picture=nb * 24, key_frame_gather_bytes=gathered)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--clips", default="inter70,idle")
    ap.add_argument("--counts", default="1,8,64")
    ap.add_argument("--first", type=int, default=200)
    ap.add_argument("--volumes", action="store_true")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    counts = [int(v) for v in args.counts.split(",")]

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
            for n in counts:
                say({"clip": name, **volumes(frames, args.first, n, wl.W, wl.H)})
        save()
        return 0

    import ctypes as C

    import numpy as np
    import torch
    if not torch.cuda.is_available():
        print("msv1_encode_latency: no GPU", file=sys.stderr)
        return 2
    from jsplayer_amd import MSVideo1_16bit, Msv1Encoder, player
    from jsplayer_amd import _native as N
    W, H = wl.W, wl.H
    lib = N.lib()
    nmax = max(counts)
    bufs = [torch.zeros(W * H, dtype=torch.int32, device="cuda") for _ in range(nmax + 1)]
    enc = Msv1Encoder(W, H)
    bound = enc.Bound()
    room = np.full(nmax * bound + 64, 0xA5, dtype=np.uint8)
    host = np.zeros(nmax * W * H, dtype=np.int32)
    ok_all = True
    for name, frames, keys in load_clips(args.clips):
        c = MSVideo1_16bit(W, H)
        c.Preinit(player.INSIGNIFICANT_LINES)
        idx = c.BuildIndex(frames, keys)
        first = min(args.first, idx.frames - nmax - 1)
        for k in range(nmax + 1):                       # bufs[k] = the picture of frame first - 1 + k
            idx.Show(first - 1 + k, bufs[k], adopt=False)
        for n in counts:
            pics = (C.c_void_p * n)(*[bufs[1 + k].data_ptr() for k in range(n)])
            prevs = (C.c_void_p * n)(*[bufs[k].data_ptr() for k in range(n)])
            lens, total, one = (C.c_size_t * n)(), C.c_size_t(0), C.c_size_t(0)

            def encode(previous):
                t0 = time.perf_counter()
                rc = lib.jsp_msv1_encode_frames(enc._h, n, pics, previous, W, C.c_void_p(room.ctypes.data), room.size, lens, C.byref(total), None)
                ms = (time.perf_counter() - t0) * 1e3
                if rc != 0:
                    raise RuntimeError(N.last_error())
                return ms

            def download():
                t0 = time.perf_counter()
                for k in range(n):
                    if lib.jsp_download(C.c_void_p(bufs[1 + k].data_ptr()), C.c_void_p(host.ctypes.data + 4 * k * W * H), W * H) != 0:
                        raise RuntimeError(N.last_error())
                return (time.perf_counter() - t0) * 1e3

            def gather():
                at = 0
                t0 = time.perf_counter()
                for k in range(n):
                    if lib.jsp_index_key_frame(c._h, idx._h, first + k, C.c_void_p(room.ctypes.data + at), bound, C.byref(one)) != 0:
                        raise RuntimeError(N.last_error())
                    at += one.value
                return (time.perf_counter() - t0) * 1e3, at

            # the check: key frame of the first picture, then the inter frames, through a fresh codec
            encode(None)
            key_bytes = total.value
            first_key = room[:lens[0]].tobytes()
            encode(prevs)
            inter_bytes = total.value
            data, at = [first_key], lens[0]
            for k in range(1, n):
                data.append(room[at:at + lens[k]].tobytes())
                at += lens[k]
            fresh = MSVideo1_16bit(W, H)
            fresh.Preinit(player.INSIGNIFICANT_LINES)
            a, b = torch.zeros_like(bufs[0]), torch.zeros_like(bufs[0])
            ok = bool(fresh.IsKeyFrame(data[0])) and fresh.DecompressI(data[0], a) == 0 and bool(torch.equal(a, bufs[1]))
            for k in range(1, n):
                prev = fresh.PreviousFrame()
                ok = ok and bool(torch.equal(fresh.DecompressP(data[k], b if prev is a else a).data_pnt, bufs[1 + k]))
            fresh.StopAndClean()
            ok_all &= ok
            _, gathered = gather()
            tk, ti, td, tg = [], [], [], []
            for _ in range(args.reps):
                tk.append(encode(None))
                ti.append(encode(prevs))
                td.append(download())
                tg.append(gather()[0])
            med = lambda v: round(statistics.median(v), 3)
            say({"clip": name, "first": first, "pictures": n, "encode_key_ms": med(tk), "encode_inter_ms": med(ti), "download_ms": med(td),
                 "key_frame_gather_ms": med(tg), "encode_key_ms_min": round(min(tk), 3), "encode_inter_ms_min": round(min(ti), 3),
                 "download_ms_min": round(min(td), 3), "key_frame_gather_ms_min": round(min(tg), 3), "key_bytes": key_bytes,
                 "inter_bytes": inter_bytes, "gathered_bytes": gathered, "picture_bytes": n * W * H * 4, "results_match": ok})
        idx.close()
        c.StopAndClean()
    say({"reps": args.reps, "device": torch.cuda.get_device_name(0), "all_results_match": ok_all})
    enc.close()
    save()
    return 0 if ok_all else 1


if __name__ == "__main__":
    sys.exit(main())
