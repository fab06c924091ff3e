"""The two inter-frame group kernels of sp_kernels.hip restated in numpy (a helper module, no tests of its own): how a workgroup
cuts a group of inter frames into chunks (`plan`), and the pictures it leaves when it walks them (`walk`).

    form "loader"   sp_pframe_group_kernel:  a workgroup covers G2_BLOCKS = 8 blocks of a block row, a chunk holds at most G2_CF = 16
                    frames and G2_LW = 3072 literal words, every rectangle's literals are rounded up to four words, a lane carries
                    rows r and r + 8 of the block row.
    form "self"     sp_pframe_group1_kernel: 4 blocks, `chunk` = 32 frames, `lit_words` = 2048 words, no rounding, and with
                    `stagger` the first chunk of workgroup (wx, by) is cut to 1 + (5 wx + 3 by) % chunk frames.

In both forms a chunk takes frames while the literals up to and including a frame's last block fit; its first frame always does.
The next chunk starts at f0 + nf.

Input: the host stage's block records of the group's frames in decode order, one (nblocks, 16) uint8 table and one uint32 payload
per frame (hoststage_binding.HostStage).  Frames that change nothing have no table and are no frame of the group (sp_codec.cpp).

`walk(..., fault=...)` makes one mistake these kernels could make:

    skip_after_cut    after a chunk cut by the literal buffer the next chunk starts at f0 + nf_try
    dst_by_group      frame f of a chunk takes the destination at f0 + f of the chunk's own table (of which the chunk holds
                      nf_try entries; past them nothing is stored)
    dst_by_chunk      frame f of a chunk takes the destination of the group's frame f
    unrounded_test    loader: the capacity test adds unrounded sizes while the placement rounds; words past the capacity are lost
    stride_16         a rectangle's rows are taken 16 words apart, not its width
    no_minus_x1       the literal pointer is not moved back by x1
    row8_reads_row    loader: row r + 8 takes row r's literals
    stale_tail        a workgroup with fewer blocks than its width takes records for its missing blocks too: what the unguarded
                      fetch brings, the first blocks of the next block row (of the next frame behind the last row)
    one_frame_more    a chunk admits one frame more than its tables hold; that frame's records are not in the table
    stagger_always    self: every chunk is cut to the staggered length, not the first
    swapped_buffer    loader: from the third chunk on the workers read the other buffer's tables: chunk c - 2 is walked again

stale_tail and stagger_always change the PLAN only.  Whatever eight (four) records say, a chunk's first frame fits, every later
frame is tested, and the placement and the fetch follow the same scan: a cut that comes earlier leaves the same pictures.  `walk`
restates them all the same, and PLAN_ONLY names them, so that the tests assert what they do change.
"""
from __future__ import annotations

from collections import namedtuple
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

# sp_kernels.hip: the loader-wave form's constexprs, and the constexpr line of launch_pframe_group for the self-staging form
G2_BLOCKS, G2_CF, G2_LW = 8, 16, 3072
chunk, lit_words, stagger = 32, 2048, 1
SELF_BLOCKS = 4                    # sp_pframe_group1_kernel: kb = chunk >> 2 of 16 four-pixel chunks

FORMS = ("loader", "self")
Form = namedtuple("Form", "blocks cap words rounds stagger")
FORM = {"loader": Form(G2_BLOCKS, G2_CF, G2_LW, True, 0), "self": Form(SELF_BLOCKS, chunk, lit_words, False, stagger)}

FAULTS = {   # name: the forms it applies to
    "skip_after_cut": FORMS, "dst_by_group": FORMS, "dst_by_chunk": FORMS, "unrounded_test": ("loader",), "stride_16": FORMS,
    "no_minus_x1": FORMS, "row8_reads_row": ("loader",), "stale_tail": FORMS, "one_frame_more": FORMS, "stagger_always": ("self",),
    "swapped_buffer": ("loader",),
}
PLAN_ONLY = ("stale_tail", "stagger_always")

PB_DATA = 4
LOST = 0xDEADBEEF                  # what a literal read outside the chunk's buffer, or of a word that was never fetched, gives
UNWRITTEN = 0xFFFFFFFF             # a destination nobody stored to

# why a chunk ended
CAP, LITERALS, STAGGER, END = "frame cap", "literal buffer", "stagger", "end of group"

Chunk = namedtuple("Chunk", "f0 nf nf_try words unrounded why lit_at next_words next_unrounded")
# f0, nf            first frame (index in the group) and frames taken
# nf_try            frames the chunk fetched records for
# words, unrounded  literal words the nf frames take as placed, and the plain sum of their rectangle sizes
# lit_at            (nf_try, blocks) where each rectangle starts in the literal buffer
# next_words, next_unrounded   the same two sums with the first frame left out included (None at the end of the group)


def geometry(w: int, h: int) -> Tuple[int, int]:
    return (w + 15) // 16, (h + 15) // 16


def sizes(table: np.ndarray) -> np.ndarray:
    """Literal words of every block of one frame's table (0 where the block has no literal rectangle)."""
    t = table.astype(np.int64)
    return np.where(t[:, 0] & PB_DATA, (t[:, 3] - t[:, 1]) * (t[:, 4] - t[:, 2]), 0)


def offsets(table: np.ndarray) -> np.ndarray:
    return np.ascontiguousarray(table[:, 12:16]).view(np.uint32).reshape(-1).astype(np.int64)


def workgroups(form: str, nbx: int, nby: int) -> List[Tuple[int, int]]:
    nb = FORM[form].blocks
    return [(wx, by) for by in range(nby) for wx in range((nbx + nb - 1) // nb)]


def _need(form: str, records: Sequence[np.ndarray], nbx: int, nby: int, wx: int, by: int, stale: bool) -> np.ndarray:
    """(frames, blocks) literal words of the workgroup's blocks, unrounded; slots past the row's end are 0, or with `stale` what
    the unguarded fetch would bring."""
    nb = FORM[form].blocks
    out = np.zeros((len(records), nb), dtype=np.int64)
    nb_here = min(nb, nbx - wx * nb)
    for f, table in enumerate(records):
        sz = sizes(table)
        first = by * nbx + wx * nb
        out[f, :nb_here] = sz[first:first + nb_here]
        if stale:
            for k in range(nb_here, nb):
                at = f * nbx * nby + first + k                    # the tables of a group's frames follow each other
                ff, b = divmod(at, nbx * nby)
                if ff < len(records):
                    out[f, k] = sizes(records[ff])[b]
    return out


def plan_one(form: str, need: np.ndarray, wx: int, by: int, fault: Optional[str] = None) -> List[Chunk]:
    """The chunk list of one workgroup from its (frames, blocks) literal sizes."""
    F = FORM[form]
    nframes = len(need)
    placed = (need + 3) & ~3 if F.rounds else need
    tested = need if fault == "unrounded_test" else placed
    cap = F.cap + 1 if fault == "one_frame_more" else F.cap
    chunks = []
    f0 = 0
    while f0 < nframes:
        nf_try = min(nframes - f0, cap)
        short = False
        if F.stagger and (f0 == 0 or fault == "stagger_always"):
            first = 1 + (5 * wx + 3 * by) % F.cap
            short = first < nf_try
            nf_try = min(nf_try, first)
        per_frame = tested[f0:f0 + nf_try].sum(axis=1).cumsum()
        over = np.nonzero(per_frame[1:] > F.words)[0]
        nf = int(over[0]) + 1 if len(over) else nf_try
        flat = placed[f0:f0 + nf_try].reshape(-1)
        lit_at = (flat.cumsum() - flat).reshape(nf_try, F.blocks)
        if nf < nf_try:
            why = LITERALS
        elif f0 + nf == nframes:
            why = END
        else:
            why = STAGGER if short else CAP
        nxt = f0 + nf < nframes
        chunks.append(Chunk(f0, nf, nf_try, int(placed[f0:f0 + nf].sum()), int(need[f0:f0 + nf].sum()), why, lit_at,
                            int(placed[f0:f0 + nf + 1].sum()) if nxt else None, int(need[f0:f0 + nf + 1].sum()) if nxt else None))
        f0 += nf_try if fault == "skip_after_cut" and nf < nf_try else nf
    return chunks


def plan(form: str, records: Sequence[np.ndarray], nbx: int, nby: int, fault: Optional[str] = None) -> Dict[Tuple[int, int], List[Chunk]]:
    """Per workgroup (wx, by) the chunks it cuts the group into."""
    return {(wx, by): plan_one(form, _need(form, records, nbx, nby, wx, by, fault == "stale_tail"), wx, by, fault)
            for wx, by in workgroups(form, nbx, nby)}


def _gather(lits: np.ndarray, idx: np.ndarray) -> np.ndarray:
    ok = (idx >= 0) & (idx < len(lits))
    return np.where(ok, lits[np.where(ok, idx, 0)], np.uint32(LOST)).astype(np.uint32)


def walk(form: str, records: Sequence[np.ndarray], payloads: Sequence[np.ndarray], prev: np.ndarray, dsts: Sequence[int],
         fault: Optional[str] = None) -> Dict[int, np.ndarray]:
    """The pictures the kernel leaves: {buffer: (h, w) uint32}.  prev: the (h, w) picture before the group; dsts[f]: the buffer
    frame f of the group goes to (any hashable; a buffer named twice keeps what was stored last)."""
    assert fault is None or form in FAULTS[fault], (form, fault)
    F = FORM[form]
    h, w = prev.shape
    nbx, nby = geometry(w, h)
    assert len(records) == len(payloads) == len(dsts)
    out = {d: np.full((h, w), UNWRITTEN, dtype=np.uint32) for d in dsts}
    plans = plan(form, records, nbx, nby, fault)
    tables = [t.astype(np.int64) for t in records]
    offs = [offsets(t) for t in records]
    for (wx, by), chunks in plans.items():
        nb_here = min(F.blocks, nbx - wx * F.blocks)
        first = by * nbx + wx * F.blocks
        ys, xs = slice(by * 16, min(by * 16 + 16, h)), slice(wx * F.blocks * 16, min((wx * F.blocks + nb_here) * 16, w))
        px = prev[ys, xs].copy()                                  # the pixels the lanes carry from frame to frame
        rows_here, cols_here = px.shape
        held = []                                                 # (chunk, its literal buffer): what each chunk buffer was filled with
        for c, ck in enumerate(chunks):
            lits = np.full(F.words, LOST, dtype=np.uint32)
            for f in range(ck.nf):
                for k in range(nb_here):
                    t = tables[ck.f0 + f][first + k]
                    if t[0] & PB_DATA:
                        n = int((t[3] - t[1]) * (t[4] - t[2]))
                        at = int(ck.lit_at[f, k])
                        o = int(offs[ck.f0 + f][first + k])
                        take = max(0, min(n, F.words - at))           # (words past the buffer's end are lost)
                        lits[at:at + take] = payloads[ck.f0 + f][o:o + take]
            held.append((ck, lits))
            use, use_lits = (held[c - 2] if fault == "swapped_buffer" and c >= 2 else held[c])
            for f in range(use.nf):
                g = use.f0 + f                                    # the frame whose records are applied
                in_table = f < F.cap                              # (one_frame_more: the frame past the tables' end has no records there)
                for k in range(nb_here if in_table else 0):
                    t = tables[g][first + k]
                    if not t[0]:
                        continue
                    x1, y1, x2, y2 = (int(v) for v in t[1:5])
                    rw = x2 - x1
                    stride = 16 if fault == "stride_16" else rw
                    base = int(use.lit_at[f, k]) - (0 if fault == "no_minus_x1" else x1)
                    for ly in range(y1, min(y2, rows_here)):
                        src_row = ly - 8 if fault == "row8_reads_row" and ly >= 8 else ly
                        rx = np.arange(x1, min(x2, cols_here - k * 16))
                        px[ly, k * 16 + rx] = _gather(use_lits, base + (src_row - y1) * stride + rx)
                if fault == "dst_by_group":
                    at = use.f0 + f
                    d = dsts[use.f0 + at] if at < use.nf_try and use.f0 + at < len(dsts) else None
                elif fault == "dst_by_chunk":
                    d = dsts[f]
                else:
                    d = dsts[g]
                if d is not None:
                    out[d][ys, xs] = px
    return out
