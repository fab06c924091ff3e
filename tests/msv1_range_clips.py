"""Clips for the MSVideo1 range calls (jsp_seek, jsp_find_change, jsp_index_*) and the oracle's frame-by-frame truth for them.

A plain helper module (no tests of its own; the GPU parts import torch only when called):
  * Idle — MSVideo1 frames built code by code, keeping the solid colour of every block;
  * long_clip — 200-300 frames from a fixed schedule that reaches what only a long clip reaches in the range kernels
    (msv1_seek_kernels.hip): blocks left alone for more than 4 bitmap words, blocks first coded late, chunk boundaries inside
    bitmap words 1 and up, walk lists of hundreds of entries, 8-bit end markers around frames 32, 64 and 128;
  * coded_blocks — which blocks a frame's parse codes (the control flow of MSVideo1.hx:106-209 / 293-393, no pixels), from
    which `plan` derives last writers, walk lists and adoption in Python;
  * truth_run — the oracle frame by frame, each destination first copied from the picture before it;
  * walk — FindChange from the frame after the one shown to the end, again and again, against truth_run."""
import numpy as np

from jsplayer_amd import MSVideo1_16bit, MSVideo1_8bit
from jsplayer_amd import streamgen as sg
from oracle_binding import OracleAbort, OracleMSVideo1

POISON = 0x5A5A5A5A


def dev_buf(n, fill=POISON, misalign=False):
    import torch
    if misalign:
        return torch.full((n + 4,), fill, dtype=torch.int32, device="cuda")[1:1 + n]
    return torch.full((n,), fill, dtype=torch.int32, device="cuda")


def make_gpu(bits, w, h, pal=None, lines=36, chunk=None, parse="host"):
    c = MSVideo1_16bit(w, h) if bits == 16 else MSVideo1_8bit(w, h, pal or b"")
    c.set_option("msv1_parse", parse)
    if chunk:
        c.set_option("msv1_seek_chunk_frames", str(chunk))
    c.Preinit(lines)
    return c


def palette(bits):
    return sg.msv1_clip(5, 8, 8, 1, bits=8)[2] if bits == 8 else None


# ---- frames built code by code -------------------------------------------------------------------------------------------------
class Idle:
    """MSVideo1 frames built code by code.  The generator keeps the solid colour of every block (None once a block holds a
    pattern), so that it can recode a block with what it already shows."""

    def __init__(self, bits, w, h, seed):
        self.bits, self.w, self.h = bits, w, h
        self.nbx, self.nby = w // 4, h // 4
        self.nb = self.nbx * self.nby
        self.rng = np.random.default_rng(seed)
        self.col = [None] * self.nb

    def colour(self):
        if self.bits == 8:
            return int(self.rng.integers(1, 256))
        while True:   # a solid 16-bit code must not look like a skip code: red == 1 is left out
            v = int(self.rng.integers(0, 0x8000))
            if (v >> 10) != 1:
                return v

    def solid(self, v):
        return bytes([v, 0x80]) if self.bits == 8 else bytes([v & 0xFF, 0x80 | (v >> 8)])

    def two(self, v0, v1, flags=0x5A5A):
        if self.bits == 8:
            return bytes([flags & 0xFF, flags >> 8, v0, v1])
        return bytes([flags & 0xFF, flags >> 8, v0 & 0xFF, v0 >> 8, v1 & 0xFF, v1 >> 8])

    def eight(self, v):
        if self.bits == 8:
            return bytes([0x34, 0x92] + [v] * 8)
        return bytes([0x34, 0x12, v & 0xFF, (v >> 8) | 0x80] + [v & 0xFF, v >> 8] * 7)

    def encode(self, codes):
        """codes: one entry per block, None = skip."""
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

    def key(self, same=False, how="solid"):
        """A key frame of solid blocks; same: the colours the blocks hold (how="two": as 2-colour codes, other bytes)."""
        if not same:
            self.col = [self.colour() for _ in range(self.nb)]
        self.col = [0 if v is None else v for v in self.col]
        return self.encode([self.solid(v) if how == "solid" else self.two(v, v) for v in self.col])

    def recode_codes(self, blocks, how=None):
        codes = [None] * self.nb
        for b in blocks:
            v = self.col[b]
            if v is None:
                continue
            kind = how or ("solid", "two", "eight")[int(self.rng.integers(0, 3))]
            codes[b] = self.solid(v) if kind == "solid" else self.two(v, v) if kind == "two" else self.eight(v)
        return codes

    def recode(self, blocks, how=None):
        return self.encode(self.recode_codes(blocks, how))

    def change_codes(self, blocks):
        codes = [None] * self.nb
        for b in blocks:
            self.col[b] = self.colour()
            codes[b] = self.solid(self.col[b])
        return codes

    def change(self, blocks):
        return self.encode(self.change_codes(blocks))

    def row_of(self, by, n=None):
        bs = list(range(by * self.nbx, (by + 1) * self.nbx))
        return bs if n is None else bs[:n]

    def first_line_only(self, by):
        """The blocks of block row `by` change their first pixel line only (a 2-colour code: new colour where flags are set)."""
        codes = [None] * self.nb
        for b in self.row_of(by):
            if self.col[b] is None:
                continue
            codes[b] = self.two(self.colour(), self.col[b], flags=0x000F)
            self.col[b] = None
        return self.encode(codes)

    def all_skip(self, kind):
        if kind == "empty":
            return b""
        if kind == "short":
            return bytes([0x01, 0x84])
        if kind == "marker":   # (8-bit) an end marker on the first block
            return b"\x00\x00"
        return self.encode([None] * self.nb)


# ---- what a frame codes ------------------------------------------------------------------------------------------------------
def coded_blocks(bits, nbx, nby, src, have_prev=True):
    """(coded, stop, early_out, raises) of one frame's parse: coded[b] — the frame writes block b from its own bytes (codes
    past the end of the data included: they read as missing, which paints the block); stop — the block of an 8-bit end marker
    (None: none); early_out — a 16-bit early-out (nothing done); raises — a skip code with no previous picture."""
    src = bytes(src)
    nb = nbx * nby
    coded = np.zeros(nb, dtype=bool)
    n = len(src)
    if bits == 16:
        sojs = (nb // 1023) * 2 + 10
        if n == 0:
            return coded, None, True, False
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
                return coded, None, True, False
    si, skip = 0, 0
    for blk in range(nb):
        if skip != 0:
            skip -= 1
            if not have_prev:
                return coded, None, False, True
            continue
        a_ok, b_ok = si < n, si + 1 < n
        a, b = (src[si] if a_ok else 0), (src[si + 1] if b_ok else 0)
        if bits == 8 and b_ok and a == 0 and b == 0:
            return coded, blk, False, False
        si += 2
        if b_ok and (b & 0xFC) == 0x84:
            skip = ((b - 0x84) << 8) + a - 1
            if not have_prev:
                return coded, None, False, True
            continue
        if bits == 16:
            if b_ok and b < 0x80:
                si += 16 if (si + 1 < n and src[si + 1] & 0x80) else 4
        elif b_ok and b < 0x80:
            si += 2
        elif b_ok and b >= 0x90:
            si += 8
        coded[blk] = True
    return coded, None, False, False


# ---- the long clip -----------------------------------------------------------------------------------------------------------
KEYS_AT = (70, 131, 132)          # mid-clip key frames (132 repeats the bytes of 131); frame 0 is one too
MARKERS_AT = (31, 33, 63, 65, 127, 129)   # 8-bit end markers / 16-bit damage: both sides of frames 32, 64 and 128
ONCE_AT, LATE_AT, LATE_FROM = 5, 120, 75   # ONCE blocks change at 5; LATE blocks are left alone from LATE_FROM to LATE_AT
IDLE = (133, 231)                 # the long idle stretch (repaints, all-skips, insignificant changes); frame 231 ends it
SECOND_AT = 231                   # ... with a change of the TWICE blocks, repainted at IDLE[0] + 3 and coded by key 131 / 132


def straddle_lines(h):
    """Preinit lines for a clip of height h: 2 pixel lines into block row nby // 2 (that row straddles them)."""
    return 4 * ((h // 4) // 2) + 2


def long_clip(bits, w, h, seed, n=300, lines=None):
    """(frames, keys, pal, plan): n frames (200..300; fewer stop the schedule early) from a fixed schedule.

    Block roles (rng permutation of the blocks, every role non-empty from 6 blocks on):
      STATIC  coded by the key frames only (0, 70, 131, 132): alone for n - 133 frames at the end;
      ONCE    changed at frame 5 and then alone until key 70 (16-bit: but for the truncated frames, which paint the blocks past
              their end);
      LATE    changed at frame LATE_AT = 120 and alone from LATE_FROM = 75 until then: a range from frame 75 shows them as
              the picture before it until t = 45;
      TWICE   repainted at IDLE[0] + 3 and changed at SECOND_AT = 231: two writers in the 4-word group below t (t in words
              6 and 8), and the FindChange hit at the end of the idle stretch, its previous writer dozens of walk entries back;
      BUSY    the rest: changes and repaints outside the idle stretch, repaints inside it.
    Also: changes of the insignificant block rows and of the straddle row (stage 1 settles them, the pixels below `lines`
    change), first-pixel-line changes of the straddle row, every all-skip kind, 8-bit end markers on the first block of a
    row, the last block of a row and the first block of the last row at MARKERS_AT, 16-bit truncated frames and odd
    trailing bytes there.

    plan: dict with n, nb, nbx, nby, lines, keys, roles, coded (n x nb bool), stop (per frame: marker block or None),
    early_out, raises (frames the oracle raises on, with the clip decoded from frame 0), markers (frame -> block)."""
    assert 96 <= n <= 300
    g = Idle(bits, w, h, seed)
    pal = palette(bits)
    lines = straddle_lines(h) if lines is None else lines
    nbx, nby, nb = g.nbx, g.nby, g.nb
    srow = min(lines // 4, nby - 1)                      # the straddle row; rows below it are insignificant
    # (TWICE first from the significant rows, below the straddle row: its change at SECOND_AT is a 16-bit FindChange hit)
    perm = sorted((int(b) for b in g.rng.permutation(nb)), key=lambda b: 0 if b // nbx > srow else 1)
    k = max(1, nb // 6)
    roles = {"TWICE": perm[:k], "STATIC": perm[k:2 * k], "ONCE": perm[2 * k:3 * k], "LATE": perm[3 * k:4 * k], "BUSY": perm[4 * k:]}
    if nb < 5:
        roles = {"STATIC": perm, "ONCE": perm, "LATE": [], "TWICE": perm, "BUSY": perm}
    busy, late = roles["BUSY"], set(roles["LATE"])
    sig_busy = [b for b in busy if b // nbx > srow] or busy
    idle_kinds = ("empty", "short", "long") if bits == 16 else ("long", "marker")
    frames, keys, intent = [], [], []   # intent: the blocks the schedule codes (None: a damaged frame, see coded_blocks)

    def add(src, key=False, blocks=None):
        frames.append(src)
        keys.append(key)
        intent.append(blocks)

    def coded_of(codes):
        return sorted(b for b, c in enumerate(codes) if c is not None)

    for i in range(n):
        if i == 0 or i == KEYS_AT[1]:
            add(g.key(), True, list(range(nb)))
        elif i == KEYS_AT[0]:
            add(g.key(same=True, how="two"), True, list(range(nb)))   # repaints the picture as it is, in other bytes
        elif i == KEYS_AT[2]:
            add(frames[-1], True, list(range(nb)))                        # repeats the bytes of the key frame before it
        elif i == ONCE_AT:
            codes = g.change_codes(roles["ONCE"])
            add(g.encode(codes), False, coded_of(codes))
        elif i == LATE_AT:
            codes = g.change_codes(roles["LATE"])
            add(g.encode(codes), False, coded_of(codes))
        elif i == SECOND_AT:
            codes = g.change_codes(roles["TWICE"])
            add(g.encode(codes), False, coded_of(codes))
        elif i == IDLE[0] + 3:
            codes = g.recode_codes(roles["TWICE"] + sig_busy[:2], how="two")
            add(g.encode(codes), False, coded_of(codes))
        elif i in MARKERS_AT:
            j = MARKERS_AT.index(i)
            if bits == 8:   # an end marker on the first block of a row, the last block of a row, the first block of the last row
                at = (srow * nbx, srow * nbx + nbx - 1, (nby - 1) * nbx)[j % 3]
            else:           # truncated after block `at` (the rest reads as missing: solid black), or an odd trailing byte
                at = max(1, nb // 2) if j % 2 == 0 else nb
            pick = [b for b in busy if b < at and b not in late]
            blocks = [int(b) for b in g.rng.choice(pick, size=max(1, len(pick) // 2), replace=False)] if pick else []
            codes = g.change_codes(blocks)
            src = g.encode(codes[:at])
            if bits == 8:
                add(src + b"\x00\x00", False, coded_of(codes))
            elif j % 2 == 0:
                if j == 4 and at < nb:   # and the first byte of one more code: the block takes that byte as its colour
                    src += bytes([0x3C])
                    g.col[at] = 0x3C
                    at += 1
                for b in range(at, nb):
                    g.col[b] = 0
                add(src, False, None)
            else:
                add(src + b"\x07", False, coded_of(codes))
        elif IDLE[0] <= i < IDLE[1]:
            r = (i - IDLE[0]) % 9
            if r in (0, 4):
                add(g.all_skip(idle_kinds[(i // 9) % len(idle_kinds)]), False, [])
            elif r == 7 and srow > 0:                            # an insignificant row changes
                blocks = [b for b in g.row_of(int(g.rng.integers(0, srow))) if b not in roles["STATIC"] and b not in roles["TWICE"]]
                codes = g.change_codes(blocks)
                add(g.encode(codes), False, coded_of(codes))
            elif r == 8:                                         # the straddle row: stage 1 settles it, pixels below `lines` change
                blocks = [b for b in g.row_of(srow) if b not in roles["STATIC"] and b not in roles["TWICE"]]
                if (i // 9) % 2 == 0:                            # ... or only its first pixel line
                    codes = _first_line(g, blocks)
                else:
                    codes = g.change_codes(blocks)
                add(g.encode(codes), False, coded_of(codes))
            else:                                                # repaint busy blocks in significant rows with what they show
                pick = [b for b in sig_busy if g.col[b] is not None] or [b for b in busy if g.col[b] is not None]
                blocks = [int(b) for b in g.rng.choice(pick, size=max(1, len(pick) // 3), replace=False)] if pick else []
                codes = g.recode_codes(blocks)
                add(g.encode(codes), False, coded_of(codes))
        else:
            r = i % 5
            pick = [b for b in busy if not (b in late and LATE_FROM <= i < LATE_AT)]
            if i > IDLE[1]:
                pick = [b for b in pick if b not in roles["STATIC"] and b not in roles["TWICE"]]
            if r == 0 or not pick:
                add(g.all_skip(idle_kinds[(i // 5) % len(idle_kinds)]), False, [])
            elif r in (1, 3):
                codes = g.change_codes([int(b) for b in g.rng.choice(pick, size=max(1, len(pick) // 4), replace=False)])
                add(g.encode(codes), False, coded_of(codes))
            else:
                codes = g.recode_codes([int(b) for b in g.rng.choice(pick, size=max(1, len(pick) // 3), replace=False)])
                add(g.encode(codes), False, coded_of(codes))
    plan = make_plan(bits, w, h, frames, keys, lines)
    plan["roles"] = roles
    plan["intent"] = intent
    plan["srow"] = srow
    return frames, keys, pal, plan


def _first_line(g, blocks):
    """Codes that change the first pixel line of `blocks` only (a 2-colour code: a new colour where the flags are set)."""
    codes = [None] * g.nb
    for b in blocks:
        if g.col[b] is None:
            continue
        codes[b] = g.two(g.colour(), g.col[b], flags=0x000F)
        g.col[b] = None
    return codes


def make_plan(bits, w, h, frames, keys, lines, have_prev=False):
    """What the schedule does, frame by frame, worked out from coded_blocks (have_prev: a picture exists before frame 0)."""
    nbx, nby = w // 4, h // 4
    nb = nbx * nby
    n = len(frames)
    coded = np.zeros((n, nb), dtype=bool)
    stop, early, raises, markers = [None] * n, [False] * n, [], {}
    prev = have_prev
    for i, f in enumerate(frames):
        c, s, e, r = coded_blocks(bits, nbx, nby, f, prev)
        coded[i], stop[i], early[i] = c, s, e
        if s is not None:
            markers[i] = s
        if r:
            raises.append(i)
            break
        prev = prev or bool(c.any())
    return {"n": n, "nb": nb, "nbx": nbx, "nby": nby, "lines": lines, "keys": list(keys), "coded": coded, "stop": stop,
            "early_out": early, "raises": raises, "markers": markers}


def adopted(plan):
    """Per frame: it codes a block (its destination becomes the previous frame)."""
    return plan["coded"].any(axis=1)


def last_writer(plan, start, t, b):
    """The last frame in [start, t] whose parse codes block b (-1: none)."""
    col = np.nonzero(plan["coded"][start:t + 1, b])[0]
    return start + int(col[-1]) if len(col) else -1


def last_writers(plan, start, t):
    """last_writer for every block at once."""
    sub = plan["coded"][start:t + 1]
    any_ = sub.any(axis=0)
    last = sub.shape[0] - 1 - np.argmax(sub[::-1], axis=0)
    return np.where(any_, start + last, -1)


def walk_list(plan, start, upto):
    """The walk list jsp_find_change builds for a range from `start` judged up to frame `upto` (one chunk): the frames that code
    a block, in order (range indices are these minus start)."""
    ad = adopted(plan)
    return [f for f in range(start, upto + 1) if ad[f]]


def scan_segment(nblocks, nwalk):
    """Entries per segment of the change scan's walk list (scan_grid, msv1_seek_kernels.hip)."""
    waves = (nblocks + 63) // 64
    nseg = max(1, (8 * 1024 + waves - 1) // waves)
    nseg = min(nseg, max(1, (nwalk + 15) // 16), 65535)
    return (nwalk + nseg - 1) // nseg


# ---- truth -------------------------------------------------------------------------------------------------------------------
def truth_run(bits, w, h, pal, frames, keys, lines=36, key_row=36, key_before=None, rows=False, keep=None, start_as=None):
    """Per frame: (picture, significance as the Manager records it[, block_changes bits when rows]) — or None at the frame
    the reference raises on (the list ends there).  keep: the frames whose picture is kept (None: all; the others get None).
    start_as: k -> what buffer k of the three holds before it is first decoded into (None: the poison everywhere)."""
    o = OracleMSVideo1(bits, w, h, pal)
    o.Preinit(lines)
    start_as = start_as or (lambda k: np.full(w * h, POISON, dtype=np.int32))
    bufs = [np.array(start_as(k), dtype=np.int32) for k in range(3)]
    out = []
    for i, (src, key) in enumerate(zip(frames, keys)):
        prev = o.PreviousFrame()
        before = None if prev is None else prev.copy()
        dst = next(b for b in bufs if b is not prev)
        if prev is not None:
            np.copyto(dst, prev)
        else:
            np.copyto(dst, start_as(next(k for k in range(3) if bufs[k] is dst)))
        if key:
            if o.DecompressI(src, dst) != 0:
                raise OracleAbort()
            kb = frames[i - 1] if i > 0 and keys[i - 1] else (key_before if i == 0 else None)
            if kb is not None:
                sig = bytes(kb) != bytes(src)
            elif before is None:
                sig = True
            else:
                sig = bool(np.any(dst[key_row * w:] != before[key_row * w:]))
        else:
            try:
                data, sig = o.DecompressP(src, dst)
            except OracleAbort:
                out.append(None)
                return out
        pic = o.PreviousFrame()
        entry = (None if pic is None or (keep is not None and i not in keep) else pic.copy(), bool(sig))
        out.append(entry + (o.BlockChanges(),) if rows else entry)
    return out


def expected_landing(truth, first):
    for k in range(first, len(truth)):
        if truth[k] is None:
            return None
        if truth[k][1]:
            return k
    return len(truth) - 1


# ---- the walk ----------------------------------------------------------------------------------------------------------------
def walk(bits, w, h, pal, frames, keys, lines=36, chunk=None, misalign=False, step=True, parse="host", truth=None):
    """Frame 0 by DecompressI, then FindChange from the frame after the one shown to the end, again and again.  step: after
    each landing the next frame goes through DecompressI / DecompressP (its picture and significance against the oracle: the
    codec state FindChange left — previous frame, block_changes — is the sequential one) before the next skip."""
    truth = truth or truth_run(bits, w, h, pal, frames, keys, lines, key_row=lines)
    gpu = make_gpu(bits, w, h, pal, lines, chunk, parse)
    n = len(frames)
    first_buf = dev_buf(w * h, misalign=misalign)
    assert gpu.DecompressI(frames[0], first_buf) == 0
    pool = [first_buf] + [dev_buf(w * h, misalign=misalign) for _ in range(2)]
    shown, landings = 0, []
    where = f"{bits}-bit {w}x{h} lines={lines} chunk={chunk} ({parse} parse)"
    while shown < n - 1:
        start = shown + 1
        want = expected_landing(truth, start)
        prev = gpu.PreviousFrame()
        dst = next(b for b in pool if b is not prev)
        kb = frames[shown] if keys[shown] else None
        res = gpu.FindChange(frames[start:], dst, keys[start:], 0, kb, lines)
        f = start + res.index
        assert f == want, f"{where}: skip from {shown} landed on {f}, the oracle on {want}"
        assert res.changed == bool(truth[f][1]), where
        for k in range(start, n):
            s = res.significance[k - start]
            assert s == (truth[k][1] if k <= f else None), f"{where}: significance of frame {k}"
        got = gpu.PreviousFrame()
        assert res.data_pnt is got, where
        assert np.array_equal(got.cpu().numpy(), truth[f][0]), f"{where}: picture of frame {f}"
        landings.append(f)
        shown = f
        if step and shown < n - 1:
            i = shown + 1
            prev = gpu.PreviousFrame()
            d = next(b for b in pool if b is not prev)
            d.copy_(prev)
            if keys[i]:
                assert gpu.DecompressI(frames[i], d) == 0
            else:
                r = gpu.DecompressP(frames[i], d)
                assert r.significant_changes == truth[i][1], f"{where}: frame {i} after the landing on {f}: significance"
            assert np.array_equal(gpu.PreviousFrame().cpu().numpy(), truth[i][0]), f"{where}: frame {i} after the landing on {f}"
            shown = i
    gpu.StopAndClean()
    return landings, truth
