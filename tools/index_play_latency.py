"""Playback from the MSVideo1 seek index (jsp_index_play) against the Shows it replaces, on the two 512-frame 1080p clips of
tools/scrub_latency.py — msvideo1_16_1080p_inter70 (frame 0 key, 70 % of the blocks skipped per frame) and the idle clip (a key
frame, 502 idle frames, a change, 8 idle frames):

  A   ONE Play(first, n, stride): frame `first` composed once, the 16 pixels of a block kept in registers, per further frame only the
      last writer of the gap decoded, n pictures stored;
  B   the n Show(first + k * stride) calls that write the same pictures into the same buffers: n launches, n synchronises, the bitmap
      walked and every block of the picture decoded again n times;

for (first, n, stride) = (1, 8, 1), (256, 8, 1), (503, 8, 1) with the buffer list reversed (reverse play), (0, 64, 8), (0, 8, 64),
(0, 512, 1).  The destinations come from a FramePool.  A and B alternate in one process, each measured with a host clock around
calls that end synchronised; medians of --reps.  Every picture of both forms is first checked against the digest of a sequential
decode.  Each row is measured at option "msv1_index_play_segments" = 1, auto and n (n capped at the option's 64).  Then the step
back 511 -> 0: in batches of 8 buffers, ONE Play(adopt = 0) per batch, against one Show(adopt) per step.  One JSON line per
measurement.

  --volumes   no GPU needed: from the clip's bytes (which frame codes which block), the bytes A and B read and write per row — bitmap
              words, table entries, code bytes and records per decode, the destination list.
  --kernel-only ROW   just a few Play calls of row ROW (0 .. 5) on --clips' first clip: the program to put behind
              `rocprofv3 --kernel-trace --stats --`.

    python tools/index_play_latency.py [--reps 5] [--clips inter70,idle] [--parse gpu|host] [--out profiles/index_play_latency.json]
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

ROWS = [(1, 8, 1, False), (256, 8, 1, False), (503, 8, 1, True), (0, 64, 8, False), (0, 8, 64, False), (0, 512, 1, False)]
SCAN = 4            # bitmap words a lane has in flight per step of a walk (msv1_seek_kernels.hip)
CODE_BYTES = 24     # six aligned dwords per decoded code (decode_at)
RECORD_BYTES = 44   # per decode: frame_chunk[f], the chunk record, the frame's stream_end


def load_clips(names):
    from jsplayer_amd import workloads as wl
    from skip_stills_latency import idle_clip
    for name in names.split(","):
        if name == "inter70":
            c = wl.build_clips("msvideo1_16_1080p_inter70")[0]
            yield name, c.frames, c.keys
        else:
            frames, keys = idle_clip(502)
            yield name, frames, keys


def coded_mask(nb, src):
    """Which blocks a 16-bit frame codes (the control flow of MSVideo1.hx:106-209, code by code; skips cost one step per run)."""
    import numpy as np
    out = np.zeros(nb, dtype=bool)
    n = len(src)
    sojs = (nb // 1023) * 2 + 10
    if n == 0:
        return out
    if n < sojs:
        total, just = 0, True
        for si in range(0, n, 2):
            if si + 1 < n and (src[si + 1] & 0xFC) == 0x84:
                total += ((src[si + 1] - 0x84) << 8) + src[si]
                if total >= nb:
                    break
            else:
                just = False
                break
        if just:
            return out
    si = blk = 0
    while blk < nb:
        if si + 1 >= n:            # codes past the end read as missing, which paints the block
            out[blk:] = True
            break
        a, b = src[si], src[si + 1]
        si += 2
        if (b & 0xFC) == 0x84:
            blk += max(((b - 0x84) << 8) + a, 1)
            continue
        if b < 0x80:
            si += 16 if (si + 1 < n and src[si + 1] & 0x80) else 4
        out[blk] = True
        blk += 1
    return out


def volumes(frames, rows, w, h):
    """Per row: the bytes ONE Play reads and writes and the bytes the n Shows read and write, from which frame codes which block."""
    import numpy as np
    nb = (w // 4) * (h // 4)
    nf = len(frames)
    waves = (nb + 63) // 64
    picture = w * h * 4
    last = np.full((nf, nb), -1, dtype=np.int16)      # last[t][b]: the last frame <= t that codes block b
    cur = np.full(nb, -1, dtype=np.int16)
    for t, f in enumerate(frames):
        cur = np.where(coded_mask(nb, bytes(f)), np.int16(t), cur)
        last[t] = cur

    def show_read(t):
        """(bitmap words, decodes) of one Show / of composing frame t: word t / 32, then SCAN words per step down to the writer's."""
        L = last[t].astype(np.int64)
        wt = t >> 5
        target = np.where(L >= 0, L >> 5, 0)
        steps = -(-(wt - target) // SCAN)
        words = 1 + np.minimum(SCAN * steps, wt)
        return int(words.sum()), int((L >= 0).sum())

    out = []
    for first, n, stride, _ in rows:
        shown = [first + k * stride for k in range(n)]
        bw = bd = 0
        for t in shown:
            words, dec = show_read(t)
            bw += words
            bd += dec
        b_read = dict(bitmap_bytes=bw * 4, table_bytes=bd * 4, code_bytes=bd * CODE_BYTES, record_bytes=bd * RECORD_BYTES)
        b_read["read_bytes"] = sum(b_read.values())
        aw, ad = show_read(first)
        for tp, t in zip(shown, shown[1:]):
            L = last[t].astype(np.int64)
            wt, wb, pw = t >> 5, (tp + 1) >> 5, tp >> 5
            if wt != pw:
                aw += nb                                   # the top word, once per word the run's frames pass through
            if wt > wb:                                    # a span of several words: down from the top word to the writer's, or the bottom
                walk = (L >> 5) < wt
                target = np.maximum(np.where(L > tp, L >> 5, wb), wb)
                steps = -(-(wt - target) // SCAN)
                fetched = np.minimum(SCAN * steps, wt - wb) - (pw >= wb)
                aw += int(np.where(walk, np.maximum(fetched, 0), 0).sum())
            ad += int((L > tp).sum())
        a_read = dict(bitmap_bytes=aw * 4, table_bytes=ad * 4, code_bytes=ad * CODE_BYTES, record_bytes=ad * RECORD_BYTES,
                      destination_list_bytes=n * waves * 8)
        a_read["read_bytes"] = sum(a_read.values())
        out.append(dict(first=first, n=n, stride=stride, written_bytes=n * picture, play=a_read, shows=b_read,
                        decodes_play=ad, decodes_shows=bd, read_ratio_shows_over_play=round(b_read["read_bytes"] / max(a_read["read_bytes"], 1), 2)))
    return out


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--parse", default="gpu", choices=["gpu", "host"])
    ap.add_argument("--clips", default="inter70,idle")
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
        for name, frames, _ in load_clips(args.clips):
            for rec in volumes(frames, ROWS, wl.W, wl.H):
                say({"clip": name, **rec})
        save()
        return 0

    import torch
    if not torch.cuda.is_available():
        print("index_play_latency: no GPU", file=sys.stderr)
        return 2
    from jsplayer_amd import FramePool, MSVideo1_16bit, player
    npix = wl.W * wl.H

    def codec():
        c = MSVideo1_16bit(wl.W, wl.H)
        c.set_option("msv1_parse", args.parse)
        c.Preinit(player.INSIGNIFICANT_LINES)
        return c

    pool = FramePool(wl.W, wl.H, max(n for _, n, _, _ in ROWS) + 1)   # (one more: the decoder's previous frame is never a destination)
    ok_all = True
    for name, frames, keys in load_clips(args.clips):
        nf = len(frames)
        seq = codec()                                        # the truth: a sequential decode, every frame's digest
        bufs = [torch.zeros(npix, dtype=torch.int32, device="cuda") for _ in range(3)]
        want = []
        for i, f in enumerate(frames):
            dst = next(b for b in bufs if b is not seq.PreviousFrame())
            if keys[i]:
                seq.DecompressI(f, dst)
            else:
                seq.DecompressP(f, dst)
            want.append(wl.digest(seq.PreviousFrame().cpu().numpy()))
        seq.StopAndClean()
        c = codec()
        idx = c.BuildIndex(frames, keys)

        def dsts(n, rev):
            prev = c.PreviousFrame()
            d = [b for b in pool.frames[:n + 1] if b is not prev][:n]
            return d[::-1] if rev else d

        def play(first, n, stride, rev, adopt=None):
            d = dsts(n, rev)
            t0 = time.perf_counter()
            idx.Play(first, d, stride, adopt=adopt)          # (returns synchronised)
            return (time.perf_counter() - t0) * 1e3

        def shows(first, n, stride, rev, adopt=False):
            d = dsts(n, rev)
            t0 = time.perf_counter()
            for k in range(n):
                idx.Show(first + k * stride, d[k], adopt=adopt)   # (each returns synchronised)
            return (time.perf_counter() - t0) * 1e3

        def exact(first, n, stride, rev):
            d = dsts(n, rev)
            return all(wl.digest(d[k].cpu().numpy()) == want[first + k * stride] for k in range(n))

        def zero(n):   # (the sequential decode's buffers started as zeros)
            for b in pool.frames[:n + 1]:
                b.zero_()
            torch.cuda.synchronize()

        if args.kernel_only >= 0:
            first, n, stride, rev = ROWS[args.kernel_only]
            for _ in range(10):
                play(first, n, stride, rev)
            ok = exact(first, n, stride, rev)
            say({"clip": name, "kernel_only": [first, n, stride], "digests_match": ok})
            idx.close()
            c.StopAndClean()
            pool.close()
            return 0 if ok else 1

        for first, n, stride, rev in ROWS:
            zero(n)
            play(first, n, stride, rev)
            ok = exact(first, n, stride, rev)
            zero(n)
            shows(first, n, stride, rev)
            ok &= exact(first, n, stride, rev)
            ok_all &= ok
            for segs in ("1", "auto", str(min(n, 64))):
                c.set_option("msv1_index_play_segments", segs)
                play(first, n, stride, rev)
                times = {"play": [], "shows": []}
                for _ in range(args.reps):
                    times["play"].append(play(first, n, stride, rev))
                    times["shows"].append(shows(first, n, stride, rev))
                a, b = statistics.median(times["play"]), statistics.median(times["shows"])
                say({"clip": name, "first": first, "n": n, "stride": stride, "reversed": rev, "segments": segs,
                     "play_ms": round(a, 4), "shows_ms": round(b, 4), "play_ms_min": round(min(times["play"]), 4),
                     "shows_ms_min": round(min(times["shows"]), 4), "play_ms_per_frame": round(a / n, 4),
                     "shows_ms_per_frame": round(b / n, 4), "shows_over_play": round(b / a, 2),
                     "written_gb_per_s_play": round(n * npix * 4 / (a * 1e-3) / 1e9, 1), "play_below_shows": a < b, "digests_match": ok})
            c.set_option("msv1_index_play_segments", "auto")

        # the step back 511 -> 0: batches of 8 (the lowest frame first, the buffers reversed, frame 0 of the run adopted) against a Show per step
        back = {"play": [], "shows": []}
        for _ in range(max(1, args.reps // 2)):
            total = 0.0
            for hi in range(nf - 1, -1, -8):
                m = min(8, hi + 1)
                total += play(hi - m + 1, m, 1, True, adopt=0)
            back["play"].append(total)
            total = 0.0
            for t in range(nf - 1, -1, -1):
                dst = next(b for b in pool.frames[:2] if b is not c.PreviousFrame())
                t0 = time.perf_counter()
                idx.Show(t, dst, adopt=True)
                total += (time.perf_counter() - t0) * 1e3
            back["shows"].append(total)
        ok = True
        for hi in range(nf - 1, -1, -8):
            m = min(8, hi + 1)
            d = dsts(m, True)                                # d[j] shows frame hi - j
            idx.Play(hi - m + 1, d[::-1], 1, adopt=0)
            ok &= all(wl.digest(d[j].cpu().numpy()) == want[hi - j] for j in range(m))
        ok_all &= ok
        a, b = statistics.median(back["play"]), statistics.median(back["shows"])
        say({"clip": name, "step_back_frames": nf, "batch": 8, "play_total_ms": round(a, 3), "shows_total_ms": round(b, 3),
             "play_per_step_ms": round(a / nf, 4), "show_per_step_ms": round(b / nf, 4), "play_below_shows": a < b, "digests_match": ok})
        idx.close()
        c.StopAndClean()
    say({"parse": args.parse, "reps": args.reps, "device": torch.cuda.get_device_name(0), "store_rate_pool_gb_per_s": round(pool.store_rate, 1),
         "all_digests_match": ok_all})
    pool.close()
    save()
    return 0 if ok_all else 1


if __name__ == "__main__":
    sys.exit(main())
