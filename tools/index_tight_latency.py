"""Thinning a clip TIGHTLY (jsp_index_tight_frames: a block whose pixels a gap did not change is dropped) against thinning it with
jsp_index_delta_frames (every block some frame of the gap codes is carried), on the two 512-frame 1080p MSVideo1 clips of
tools/scrub_latency.py — msvideo1_16_1080p_inter70 and the idle clip — for a stride-8 time-lapse (frames 0, 8, 16, ...: 63 gaps):

  A   ONE jsp_index_delta_frames call for the 63 pairs (8 k, 8 k + 8];
  B   ONE jsp_index_tight_frames call for the same pairs: its sizes launch decodes both ends of the gap of every written block.

A and B alternate in one process, each measured with a host clock around calls that end synchronised; medians of --reps — once
through the Python method (which allocates the host bytes it returns) and once as the C call alone into one host buffer that is
allocated and touched before the clock starts (`*_call_ms`).  B is checked first: a fresh codec decodes KeyFrame(0) and the 63 tight
frames one after the other to the pictures Show gives.  There is no pass mark on time.  One JSON line per measurement.

  --volumes   no GPU needed: from the clip's bytes alone (16-bit codes parsed and decoded with numpy), the size of the clip thinned
              tightly, thinned with Delta, all-key, and of the original frames they replace — for the two clips above and for
              `toggle`, a clip of this tool's own making in which a region of the picture toggles between two states with period 2
              (a blinking highlight) while a few blocks elsewhere change for good.

    python tools/index_tight_latency.py [--reps 5] [--clips inter70,idle] [--stride 8] [--parse gpu|host] [--out profiles/index_tight_latency.json]
    python tools/index_tight_latency.py --volumes [--clips inter70,idle,toggle] [--out profiles/index_tight_volumes.json]
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

from index_delta_latency import skip_words   # noqa: E402
from index_play_latency import load_clips    # noqa: E402

TOGGLE = dict(w=640, h=360, frames=128, region=(20, 10, 60, 40), drift=12)   # the toggling clip: blocks x0, y0, x1, y1 of the region


def toggle_clip():
    """(frames, keys, w, h): 16 bits.  Frame 0 is a key frame of solid blocks; every odd frame paints the region's blocks with their
    second colours, every even frame with their first ones again; every frame gives `drift` blocks outside the region a new colour."""
    import numpy as np
    w, h, n = TOGGLE["w"], TOGGLE["h"], TOGGLE["frames"]
    nbx, nb = w // 4, (w // 4) * (h // 4)
    rng = np.random.default_rng(7)

    def colours(k):   # (red == 1 would read as a skip code)
        v = rng.integers(0, 0x8000, size=k)
        return np.where((v >> 10) == 1, v ^ 0x0800, v)

    def encode(codes):   # {block: colour}: solid codes, skip words in between and up to the end of the picture
        out, at = bytearray(), 0
        for b in sorted(codes) + [nb]:
            run = b - at
            while run:
                k = min(run, 1023)
                out += bytes([k & 0xFF, 0x84 + (k >> 8)])
                run -= k
            if b < nb:
                out += bytes([codes[b] & 0xFF, 0x80 | (codes[b] >> 8)])
            at = b + 1
        return bytes(out)

    x0, y0, x1, y1 = TOGGLE["region"]
    region = [y * nbx + x for y in range(y0, y1) for x in range(x0, x1)]
    outside = np.array(sorted(set(range(nb)) - set(region)))
    first = colours(nb)
    second = colours(nb)
    frames = [encode({b: int(first[b]) for b in range(nb)})]
    for t in range(1, n):
        state = second if t % 2 else first
        codes = {b: int(state[b]) for b in region}
        for b, v in zip(rng.choice(outside, size=TOGGLE["drift"], replace=False), colours(TOGGLE["drift"])):
            codes[int(b)] = int(v)
        frames.append(encode(codes))
    return frames, [True] + [False] * (n - 1), w, h


def parse(nb, src):
    """Per block of a 16-bit frame: (length of its code — 2, 6 or 18, 0 where the frame does not code the block —, its offset).  The
    control flow of MSVideo1.hx:106-209; these clips have no damaged frame."""
    import numpy as np
    length, offset = np.zeros(nb, dtype=np.int64), np.zeros(nb, dtype=np.int64)
    n = len(src)
    si = blk = 0
    while blk < nb and si + 1 < n:
        a, b = src[si], src[si + 1]
        o = si
        si += 2
        if (b & 0xFC) == 0x84:
            blk += max(((b - 0x84) << 8) + a, 1)
            continue
        if b < 0x80:
            eight = si + 1 < n and bool(src[si + 1] & 0x80)
            si += 16 if eight else 4
            length[blk] = 18 if eight else 6
        else:
            length[blk] = 2
        offset[blk] = o
        blk += 1
    return length, offset


def pixels(code, length):
    """The 16 colours (15 bits each: what a frame buffer's word is made of) of every code: code (k, 18) bytes, length (k,)."""
    import numpy as np
    words = code[:, 0::2].astype(np.int64) | (code[:, 1::2].astype(np.int64) << 8)   # (k, 9): the flag word, then the colours
    flags, cols = words[:, 0], words[:, 1:] & 0x7FFF
    out = np.empty((len(code), 16), dtype=np.int64)
    for p in range(16):
        y, x = p >> 2, p & 3
        other = 1 - ((flags >> p) & 1)                            # a set flag bit takes the FIRST colour of the pair
        quad = np.where(length == 18, ((y & 2) << 1) + (x & 2), 0)
        out[:, p] = np.where(length == 2, flags & 0x7FFF, cols[np.arange(len(code)), quad + other])
    return out


def volumes(frames, stride, w, h):
    """The clip thinned tightly, thinned with Delta, all-key, and the original frames up to the last kept one, in bytes."""
    import numpy as np
    nb = (w // 4) * (h // 4)
    keep = list(range(0, len(frames), stride))
    length = np.zeros(nb, dtype=np.int64)             # per block: the length of its last writer's code ...
    code = np.zeros((nb, 18), dtype=np.uint8)         # ... and its bytes
    shown = np.zeros((nb, 16), dtype=np.int64)        # per block: its pixels at the last kept frame
    since = np.zeros(nb, dtype=bool)                  # per block: written since the last kept frame
    tight = delta = all_key = dropped = written = 0
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
            tight += key
            delta += key
        else:
            kept = since.copy()
            kept[since] = np.any(now != shown[since], axis=1)
            delta += int(length[since].sum()) + 2 * skip_words(since)
            tight += int(length[kept].sum()) + 2 * skip_words(kept)
            written += int(since.sum())
            dropped += int(since.sum() - kept.sum())
        shown[since] = now
        since[:] = False
    original = sum(len(f) for f in frames[:keep[-1] + 1])
    return dict(stride=stride, kept_frames=len(keep), tight_bytes=tight, delta_bytes=delta, all_key_bytes=all_key, original_bytes=original,
                written_blocks=written, dropped_blocks=dropped, tight_over_delta=round(tight / max(delta, 1), 4),
                tight_over_all_key=round(tight / max(all_key, 1), 4), delta_over_all_key=round(delta / max(all_key, 1), 4))


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--stride", type=int, default=8)
    ap.add_argument("--parse", default="gpu", choices=["gpu", "host"])
    ap.add_argument("--clips", default="")
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
        for name in (args.clips or "inter70,idle,toggle").split(","):
            if name == "toggle":
                frames, _, w, h = toggle_clip()
                say({"clip": name, "width": w, "height": h, "frames": len(frames), **volumes(frames, args.stride, w, h)})
            else:
                _, frames, _ = next(iter(load_clips(name)))
                say({"clip": name, "width": wl.W, "height": wl.H, "frames": len(frames), **volumes(frames, args.stride, wl.W, wl.H)})
        save()
        return 0

    import ctypes as C

    import numpy as np
    import torch
    if not torch.cuda.is_available():
        print("index_tight_latency: no GPU", file=sys.stderr)
        return 2
    from jsplayer_amd import FramePool, MSVideo1_16bit, player
    from jsplayer_amd import _native as N
    W, H = wl.W, wl.H
    pool = FramePool(W, H, 3)
    ok_all = True
    for name, frames, keys in load_clips(args.clips or "inter70,idle"):
        c = MSVideo1_16bit(W, H)
        c.set_option("msv1_parse", args.parse)
        c.Preinit(player.INSIGNIFICANT_LINES)
        idx = c.BuildIndex(frames, keys)
        keep = list(range(0, idx.frames, args.stride))
        pairs = list(zip(keep, keep[1:]))

        def form(tight):
            t0 = time.perf_counter()
            out = idx.DeltaFrames(pairs, tight=tight)             # (returns synchronised, the bytes on the host)
            return (time.perf_counter() - t0) * 1e3, out

        _, loose = form(False)
        _, thin = form(True)
        # the check of B: a fresh codec plays KeyFrame(0) and the tight frames to the pictures Show gives
        shown, a, b = pool.frames[:3]
        fresh = MSVideo1_16bit(W, H)
        fresh.Preinit(player.INSIGNIFICANT_LINES)
        first = idx.KeyFrame(keep[0])
        ok = bool(fresh.IsKeyFrame(first)) and fresh.DecompressI(first, a) == 0
        for t, data in zip(keep[1:], thin):
            prev = fresh.PreviousFrame()
            dst = b if prev is a else a
            dst.copy_(prev)
            fresh.DecompressP(data, dst)
            idx.Show(t, shown, adopt=False)
            ok = ok and bool(torch.equal(fresh.PreviousFrame(), shown))
        fresh.StopAndClean()
        ok = ok and all(len(x) <= len(y) for x, y in zip(thin, loose))
        # the C calls alone, into a host buffer that exists before the clock starts
        lib = N.lib()
        room = np.full(sum(len(f) for f in loose) + 64, 0xA5, dtype=np.uint8)
        frm, to = (C.c_int * len(pairs))(*[p for p, _ in pairs]), (C.c_int * len(pairs))(*[q for _, q in pairs])
        lens, total = (C.c_size_t * len(pairs))(), C.c_size_t(0)

        def call(fn):
            t0 = time.perf_counter()
            rc = fn(c._h, idx._h, len(pairs), frm, to, C.c_void_p(room.ctypes.data), room.size, lens, C.byref(total))
            ms = (time.perf_counter() - t0) * 1e3
            if rc != 0:
                raise RuntimeError(N.last_error())
            return ms

        call(lib.jsp_index_tight_frames)
        ok = ok and room[:total.value].tobytes() == b"".join(thin)   # (the C call alone gave the same bytes)
        call(lib.jsp_index_delta_frames)
        ok = ok and room[:total.value].tobytes() == b"".join(loose)
        ok_all &= ok
        ta, tb, ca, cb = [], [], [], []
        for _ in range(args.reps):
            ta.append(form(False)[0])
            tb.append(form(True)[0])
            ca.append(call(lib.jsp_index_delta_frames))
            cb.append(call(lib.jsp_index_tight_frames))
        ma, mb, mca, mcb = (statistics.median(x) for x in (ta, tb, ca, cb))
        say({"clip": name, "stride": args.stride, "pairs": len(pairs), "delta_frames_ms": round(ma, 3), "tight_frames_ms": round(mb, 3),
             "delta_frames_ms_min": round(min(ta), 3), "tight_frames_ms_min": round(min(tb), 3), "tight_over_delta": round(mb / ma, 2),
             "delta_frames_call_ms": round(mca, 3), "tight_frames_call_ms": round(mcb, 3), "call_tight_over_delta": round(mcb / mca, 2),
             "delta_bytes": sum(len(f) for f in loose), "tight_bytes": sum(len(f) for f in thin),
             "index_device_bytes": idx.device_bytes, "results_match": ok})
        idx.close()
        c.StopAndClean()
    say({"parse": args.parse, "reps": args.reps, "device": torch.cuda.get_device_name(0), "all_results_match": ok_all})
    pool.close()
    save()
    return 0 if ok_all else 1


if __name__ == "__main__":
    sys.exit(main())
