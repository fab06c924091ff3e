"""msv1_blocks_temporal_kernel (jsplayer_amd/csrc/msv1_kernels.hip) restated in numpy: which frames of an inter-frame group
each 256-block tile takes into which chunk (`plan`), and what the launch leaves in every destination buffer and in every
frame's significance word (`walk`) — with, on request, ONE of the mistakes the kernel could make (FAULTS).

A plain helper module (no tests of its own, numpy only):
  * parse / stage — msv1_host.cpp's walk and msv1_codec.cpp's decide_frames + plan_launches: the block tables (absolute
                    offsets into the batch's stream buffer, SKIP, UNTOUCHED), stream ends, no-op / uses-prev / cmp_row_lo
                    attributes, who is adopted, which frames a staged batch runs alone, and which the on-GPU parse hands
                    to the host parser;
  * plan          — the loader wave: per tile the chunks, per chunk the group frames it holds with lo, need, code_at, and
                    `next`;
  * walk          — loader and workers over a modelled pair of LDS chunk buffers that keep their bytes from chunk to
                    chunk, as the real ones do: what a worker decodes is what the model's buffer holds where the kernel
                    would read.

Frames start at multiples of 16 bytes with the host parse and of the 16 KiB parse tile with the on-GPU parse; both leave
`lo & ~15` a function of the offset inside the frame, so one model serves both (stage(..., align=)).

The modelled LDS starts as zeros (the real one is whatever the CU held): a fault that reads bytes nobody wrote can
therefore only be caught here where an EARLIER chunk of the same launch left non-zero bytes, which is what the catalogue
(tests/msv1_temporal_clips.py) arranges.  `quad_guard` is modelled by its mildest outcome: the blocks of the partial
quad are never written."""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

WG = 256                      # blocks per tile (a lane each)
T_NF = 16                     # frames per chunk, at most
T_CODE = 14 * 1024            # bytes of code stream per chunk
T_SLACK = 64                  # readable bytes behind a chunk's code bytes
SKIP = 0xFFFFFFFF
UNTOUCHED = 0xFFFFFFFE
NO_COMPARE = 0xFFFFFFFF
HOST_ALIGN, GPU_ALIGN = 16, 16384

FAULTS = ("swapped_buffer", "skip_after_cut", "slot_index", "sig_one_word", "first_lost_to_noop", "block_rows", "quad_guard",
          "stale_tail", "tail_byte_dropped", "hi_short", "lo_unrounded_at", "noop_takes_slot")
# Faults that change only the plan: none.  Each of the twelve can leave a wrong picture or flag, and the catalogue holds a clip
# on which it does (tests/test_msv1_temporal_clips_cpu.py: CATCHES).  Those that ALSO move the plan are named here, and the
# test holds them to that as well.
PLAN_ONLY = ()
MOVES_PLAN = ("skip_after_cut", "hi_short", "noop_takes_slot", "quad_guard", "lo_unrounded_at")

_QUAD = np.array([((y & 2) << 1) + (x & 2) for y in range(4) for x in range(4)])


def rgb555(c):
    c = np.asarray(c, dtype=np.int64)
    return ((c & 0x1F) << 3) | ((c & 0x3E0) << 6) | ((c & 0x7C00) << 9)


# ---- the host stage ---------------------------------------------------------------------------------------------------------
@dataclass
class Parsed:
    desc: np.ndarray          # per block: offset of its code inside the frame, SKIP or UNTOUCHED
    early_out: bool = False
    aborted: bool = False
    changes: bool = False
    s1: bool = False
    n_coded: int = 0
    n_skipped: int = 0
    n_untouched: int = 0
    short: bool = False       # the chain runs off the end of the (even part of the) data: the on-GPU parse hands it over
    end_marker: bool = False
    skip_codes: int = 0


def just_skips(data, nblocks):
    total = 0
    for si in range(0, len(data), 2):
        if si + 1 >= len(data) or (data[si + 1] & 0xFC) != 0x84:
            return False
        total += ((data[si + 1] - 0x84) << 8) + data[si]
        if total >= nblocks:
            return True
    return True


def parse(bits, nbx, nby, data, have_prev, insignificant_blocks, block_changes):
    """msv1_parse of msv1_host.cpp.  `block_changes`: the codec's persistent per-row list, updated in place."""
    nb = nbx * nby
    n = len(data)
    n_even = n & ~1
    out = Parsed(np.full(nb, UNTOUCHED, dtype=np.int64))
    if bits == 16 and (n == 0 or (n < (nb // 1023) * 2 + 10 and just_skips(data, nb))):
        out.early_out = True
        return out
    si = skip = blk = 0
    stop = False
    for by in range(nby):
        if stop:
            break
        block_changes[by] = 0
        row_coded = False
        for bx in range(nbx):
            if skip != 0:
                skip -= 1
                if not have_prev:
                    out.aborted = stop = True
                    break
                out.desc[blk] = SKIP
                out.n_skipped += 1
                blk += 1
                continue
            b_ok = si + 1 < n
            a = data[si] if si < n else 0
            b = data[si + 1] if b_ok else 0
            if bits == 8 and b_ok and a == 0 and b == 0:
                out.end_marker = stop = True
                break
            if si + 1 >= n_even:
                out.short = True
            at = si
            si += 2
            if b_ok and (b & 0xFC) == 0x84:
                skip = ((b - 0x84) << 8) + a - 1
                out.skip_codes += 1
                if not have_prev:
                    out.aborted = stop = True
                    break
                out.desc[blk] = SKIP
                out.n_skipped += 1
                blk += 1
                continue
            if bits == 16:
                if b_ok and b < 0x80:
                    si += 16 if (si + 1 < n and data[si + 1] & 0x80) else 4
            elif b_ok and b < 0x80:
                si += 2
            elif b_ok and b >= 0x90:
                si += 8
            out.desc[blk] = at
            out.n_coded += 1
            row_coded = True
            blk += 1
        if row_coded:
            block_changes[by] = 1
            out.changes = True
    out.n_untouched = nb - blk
    if not out.aborted and out.changes:
        out.s1 = any(block_changes[max(insignificant_blocks, 0):nby])
    return out


@dataclass
class FrameAttr:
    desc: np.ndarray          # absolute offsets into the stream buffer, SKIP, UNTOUCHED
    beg: int
    stream_end: int
    dst: int                  # index of the destination buffer
    prev: object              # index of the buffer that is the codec's previous frame when this one is staged (None: none)
    noop: bool
    uses_prev: bool
    cmp_row_lo: int
    special: bool
    dependent: bool
    adopted: bool
    significant: int          # 1, 0, or -1: the stage-2 compare decides
    status: int               # 0, or 2: the reference raises
    host: bool                # the on-GPU parse hands the frame to the host parser


@dataclass
class Staged:
    bits: int
    w: int
    h: int
    frames: list              # FrameAttr
    stream: np.ndarray        # the batch's stream buffer (uint8, zero padded; + 64)
    groups: list              # (first, count, kind): "temporal", "blocks" (per-frame kernel), "alone" (special)
    prev_after: object
    palette: object = None
    vec_ok: bool = True

    @property
    def nbx(self):
        return self.w // 4

    @property
    def nby(self):
        return self.h // 4

    @property
    def nblocks(self):
        return self.nbx * self.nby


def stage(bits, w, h, frames, keys, dsts, lines, prev, align=HOST_ALIGN, palette=None, block_changes=None):
    """decide_frames + plan_launches.  frames: bytes each; dsts: buffer index each; `prev`: index of the buffer holding the
    codec's previous frame before the batch (None: there is none); lines: what Preinit was given (None: never called)."""
    nbx, nby = w // 4, h // 4
    nb = nbx * nby
    insign_blocks = 0 if lines is None else (lines + 3) >> 2
    compares = bits == 16 and lines is not None
    block_changes = [0] * nby if block_changes is None else block_changes
    begs, total = [], 0
    for f in frames:
        begs.append(total)
        total += (len(f) + align - 1) // align * align
    stream = np.zeros(total + 64, dtype=np.uint8)
    attrs = []
    for i, f in enumerate(frames):
        stream[begs[i]:begs[i] + len(f)] = np.frombuffer(bytes(f), dtype=np.uint8)
        pr = parse(bits, nbx, nby, bytes(f), prev is not None, insign_blocks, block_changes)
        desc = np.where(pr.desc < UNTOUCHED, pr.desc + begs[i], pr.desc)
        dependent = pr.n_skipped != 0
        cmp_row_lo, sg, adopted, status = NO_COMPARE, 0, False, 0
        if pr.early_out:
            pass
        elif pr.aborted:
            status = 2
        else:
            if not pr.s1 or keys[i]:
                sg = 0
            elif prev is None:
                sg = 1
            else:
                sg = -1 if compares else 0
            if sg < 0:
                cmp_row_lo = max(lines, 0)
                dependent = True
            adopted = pr.changes
        tiny = bits == 16 and len(f) < (nb // 1023) * 2 + 10
        host = tiny or len(f) == 0 or pr.short or pr.end_marker or (pr.skip_codes > 0 and prev is None)
        attrs.append(FrameAttr(desc, begs[i], begs[i] + len(f), dsts[i], prev, pr.early_out, dependent and prev is not None, cmp_row_lo,
                               pr.aborted or (pr.n_untouched > 0 and not pr.early_out), dependent, adopted, sg, status, host))
        if adopted:
            prev = dsts[i]
    vec_ok = w % 4 == 0
    groups, i, n = [], 0, len(frames)
    while i < n:
        if attrs[i].special:
            groups.append((i, 1, "alone"))
            i += 1
            continue
        j = i
        while j < n and not attrs[j].special:
            j += 1
        if any(a.dependent for a in attrs[i:j]) and vec_ok:
            groups.append((i, j - i, "temporal"))
        else:
            groups.append((i, j - i, "blocks"))
        i = j
    return Staged(bits, w, h, attrs, stream, groups, prev, palette, vec_ok)


# ---- the loader ---------------------------------------------------------------------------------------------------------------
@dataclass
class Slot:
    frame: int                # index within the group
    lo: int
    need: int
    code_at: int
    end: int
    first_uses_prev: bool


@dataclass
class Chunk:
    rows: list                # the group frames whose table rows were fetched (at most T_NF)
    slots: list               # Slot, the frames kept
    next: int
    cut: bool                 # closed by the code area (a fetched row was left for the next chunk)
    over: int                 # used + need - T_CODE of the frame that was refused (cut), else of the last one admitted
    fits: list = field(default_factory=list)   # used + need - T_CODE per admitted frame


def tiles(nblocks):
    return (nblocks + WG - 1) // WG


def _extent(desc, end, fault):
    coded = desc[desc < UNTOUCHED]
    if coded.size == 0:
        return 0xFFFFFFF0, 0, 0, 0xFFFFFFFF
    raw_lo = int(coded.min())
    lo = raw_lo & ~15
    hi = int(coded.max()) + (2 if fault == "hi_short" else 18)
    hi = min(hi, end)
    length = hi - lo if hi > lo else 0
    return lo, (length + 15) & ~15, hi, raw_lo


def plan(group, nblocks, fault=None):
    """group: the FrameAttr of one temporal group, in order -> {tile: [Chunk]}."""
    n = len(group)
    out = {}
    for t in range(tiles(nblocks)):
        blk0 = t * WG
        live = min(nblocks - blk0, WG)
        if fault == "quad_guard":
            live = live // 4 * 4
        chunks, f, first = [], 0, True
        while f < n:
            rows, scan = [], f
            while scan < n and len(rows) < T_NF:
                if group[scan].noop and fault != "noop_takes_slot":
                    if fault == "first_lost_to_noop":
                        first = False
                else:
                    rows.append(scan)
                scan += 1
            used, slots, cut, over, fits = 0, [], False, 0, []
            for fi in rows:
                a = group[fi]
                lo, need, _, raw_lo = _extent(a.desc[blk0:blk0 + live], a.stream_end, fault)
                over = used + need - T_CODE
                if over > 0 and slots:
                    cut = True
                    break
                slots.append(Slot(fi, raw_lo if fault == "lo_unrounded_at" and need else lo, need, used, a.stream_end, first and a.uses_prev))
                fits.append(over)
                first = False
                used = (used + need + T_SLACK + 15) & ~15
            f = rows[len(slots)] if len(slots) < len(rows) and fault != "skip_after_cut" else scan
            chunks.append(Chunk(rows, slots, f, cut, over, fits))
        out[t] = chunks
    return out


def brief(plans):
    """A plan reduced to what can be compared: per tile and chunk the (frame, lo, need, code_at) kept, and next."""
    return {t: [([(s.frame, s.lo, s.need, s.code_at) for s in c.slots], c.next) for c in cs] for t, cs in plans.items()}


# ---- the workers --------------------------------------------------------------------------------------------------------------
def _decode(bits, L, p, avail, tail, at_end, pal):
    """The pixels of the blocks whose codes start at L[p] -> (len(p), 16).  avail: bytes up to the end of the frame's data;
    16-bit: tail = the odd last byte (0: none), at_end = the code starts exactly at the whole-word end."""
    p = np.clip(p, 0, L.size - 24)
    by = L[p[:, None] + np.arange(20)[None, :]].astype(np.int64)
    bit = ((by[:, 0] | (by[:, 1] << 8))[:, None] >> np.arange(16)[None, :]) & 1
    if bits == 16:
        wd = by[:, 0::2] | (by[:, 1::2] << 8)                      # code word, then the colours
        w0, cols = wd[:, 0], rgb555(wd[:, 1:9])
        pattern = w0 < 0x8000
        eight = pattern & ((wd[:, 1] & 0x8000) != 0)
        two = np.where(bit == 1, cols[:, 0:1], cols[:, 1:2])
        px8 = np.take_along_axis(cols, _QUAD[None, :] + (1 - bit), axis=1)
        px = np.where(eight[:, None], px8, np.where(pattern[:, None], two, rgb555(w0)[:, None]))
        px = np.where((avail == 0)[:, None], 0, px)
        if tail:
            px = np.where(at_end[:, None], rgb555(tail), px)
        return px
    b = by[:, 1]
    idx = np.where(avail[:, None] > 2 + np.arange(8)[None, :], pal[by[:, 2:10]], 0)
    two = np.where(bit == 1, idx[:, 0:1], idx[:, 1:2])
    px8 = np.take_along_axis(idx, _QUAD[None, :] + (1 - bit), axis=1)
    px = np.where((b < 0x80)[:, None], two, np.where((b >= 0x90)[:, None], px8, pal[by[:, 0]][:, None]))
    px = np.where((avail == 1)[:, None], pal[by[:, 0]][:, None], px)
    return np.where((avail == 0)[:, None], 0, px)


def walk(st, first, count, bufs, fault=None):
    """One launch of the temporal kernel over frames [first, first + count) of a staged batch, then msv1_edge_compare_kernel
    where Y % 4 != 0.  bufs: the buffers (flat uint32 arrays of w * h), changed in place -> significance flags (bool per
    frame of the group: the frame's signif word is non-zero)."""
    bits, w, h, nbx, nb = st.bits, st.w, st.h, st.nbx, st.nblocks
    group = st.frames[first:first + count]
    pal = None
    if bits == 8:
        pal = np.zeros(256, dtype=np.int64)
        v = np.frombuffer(bytes(st.palette or b""), dtype="<u4")[:256]
        pal[:len(v)] = v
    views = [b.reshape(h, w) for b in bufs]
    words = (count + 31) // 32
    signif = np.zeros(count, dtype=bool)
    plans = plan(group, nb, fault)
    for t, chunks in plans.items():
        blk0 = t * WG
        live = min(nb - blk0, WG)
        blks = blk0 + np.arange(live)
        brow, bcol = blks // nbx, blks % nbx
        yy = (brow[:, None] * 4 + np.arange(16)[None, :] // 4)
        xx = (bcol[:, None] * 4 + np.arange(16)[None, :] % 4)
        px = np.zeros((live, 16), dtype=np.int64)
        lds = [np.zeros(T_CODE + T_SLACK + 64, dtype=np.uint8) for _ in range(2)]
        sig = [0] * max(words, 1)
        if chunks and chunks[0].slots and chunks[0].slots[0].first_uses_prev:
            px = views[group[chunks[0].slots[0].frame].prev][yy, xx].astype(np.int64)
        filled = []                                            # per chunk: what the workers find in its buffer
        for c, ck in enumerate(chunks):
            L = lds[c & 1]
            tails = []
            for s in ck.slots:                                 # step 3: the requests; step 4: zero behind the end
                a = group[s.frame]
                lo = s.lo & ~15
                L[s.code_at:s.code_at + s.need] = st.stream[lo:lo + s.need]
                end = a.stream_end & ~1 if bits == 16 else a.stream_end
                tail = 0
                if s.need and lo + s.need + T_SLACK > end:
                    if bits == 16 and a.stream_end & 1 and a.stream_end > lo and a.stream_end - 1 - lo < s.need and fault != "tail_byte_dropped":
                        tail = int(L[s.code_at + a.stream_end - 1 - lo])
                    if fault != "stale_tail":
                        z0 = end - lo if end > lo else 0
                        L[s.code_at + z0:s.code_at + s.need + T_SLACK] = 0
                tails.append(tail)
            filled.append((ck, tails))
            rd, rtails = filled[c - 1] if fault == "swapped_buffer" and c >= 2 else (ck, tails)
            Lr = lds[(c & 1) ^ 1] if fault == "swapped_buffer" and c >= 2 else L
            for i, s in enumerate(rd.slots):
                a = group[s.frame]
                d = a.desc[blk0:blk0 + live].copy()
                if fault == "noop_takes_slot" and a.noop:
                    d[:] = SKIP
                if fault == "quad_guard":
                    d[live // 4 * 4:] = UNTOUCHED
                end = a.stream_end & ~1 if bits == 16 else a.stream_end
                coded = d < UNTOUCHED
                diff = False
                if coded.any():
                    o = d[coded]
                    avail = np.maximum(end - o, 0)
                    nx = _decode(bits, Lr, s.code_at + (o - s.lo), avail, rtails[i], o == end, pal)
                    if a.cmp_row_lo != NO_COMPARE:
                        rows = yy[coded]
                        lo_row = a.cmp_row_lo // 4 * 4 if fault == "block_rows" else a.cmp_row_lo
                        diff = bool(((nx != px[coded]) & (rows >= lo_row)).any())
                    px[coded] = nx
                wr = d != UNTOUCHED
                if wr.any():
                    views[a.dst][yy[wr], xx[wr]] = px[wr].astype(np.uint32)
                if diff:
                    k = i if fault == "slot_index" else s.frame
                    if fault == "sig_one_word":
                        sig[0] |= 1 << (k & 31)
                    elif k >> 5 < len(sig):
                        sig[k >> 5] |= 1 << (k & 31)
        for fi in range(count):
            if (sig[fi >> 5] >> (fi & 31)) & 1:
                signif[fi] = True
    cx, cy = nbx * 4, st.nby * 4
    if cy != h or cx != w:                                      # msv1_edge_compare_kernel: the pixels outside the block grid
        for fi, a in enumerate(group):
            if a.cmp_row_lo != NO_COMPARE:
                outside = np.ones((h, w), dtype=bool)
                outside[:cy, :cx] = False
                outside[:a.cmp_row_lo, :] = False
                if (views[a.dst][outside] != views[a.prev][outside]).any():
                    signif[fi] = True
    return signif


def run(st, bufs, fault=None):
    """Every launch of a staged batch -> (status, adopted, signif) per frame, as StagedBatch.results() reports them (signif:
    stage 1's answer, or the compare's).  Groups the product gives to the per-frame kernel are walked the same way: the pictures
    and flags do not depend on who paints them."""
    sig = [a.significant == 1 for a in st.frames]
    for first, count, kind in st.groups:
        assert kind != "alone", "the model walks no frame that the reference raises on or leaves partly written"
        got = walk(st, first, count, bufs, fault)
        for k in range(count):
            if st.frames[first + k].significant < 0:
                sig[first + k] = bool(got[k])
    return [a.status for a in st.frames], [a.adopted for a in st.frames], sig
