"""A numpy model of msv1_index_play_kernel (jsplayer_amd/csrc/msv1_seek_kernels.hip) with the kernel's exact control flow, over a
plan of msv1_range_clips (which frame codes which block) — no GPU, no tests of its own.

  * bitmap words as the build lays them out (bit k of word w: frame 32 w + k codes the block);
  * index_last_writer: the top word masked to the frames <= t, then the words below it, SCAN in flight per step;
  * index_last_writer_span: the same with a lower bound — top word masked to <= t, bottom word to > t_{k-1}, stop at the bottom word,
    and the two cached words (the last top word fetched and the one before);
  * per segment of the run: compose the first frame, the `have` flag, a bounded last writer per further frame, null destinations
    before the first adopting frame, the remainder pixels from `before`.

A block's pixels as frame f codes them are taken from the oracle's picture after frame f (truth_run): the model is about WHICH
writer a lane decodes, not about the decode.  `wrong=` selects one of three deliberately broken walks that the tests must catch."""
import numpy as np

from msv1_range_clips import POISON

SCAN = 4
ALL = np.uint32(0xFFFFFFFF)


def bitmap_words(coded):
    """coded: (frames, nb) bool -> (words, nb) uint32."""
    n, nb = coded.shape
    nw = (n + 31) // 32
    bm = np.zeros((nw, nb), dtype=np.uint32)
    for f in range(n):
        bm[f >> 5] |= coded[f].astype(np.uint32) << np.uint32(f & 31)
    return bm


def _top_bit(m):
    """31 - clz(m) per lane (m != 0)."""
    return np.floor(np.log2(m.astype(np.float64))).astype(np.int64)


def index_last_writer(bm, t):
    """Per block: (m, w) — the word holding the last frame <= t that codes it, masked to the frames <= t, and its number; m = 0: none."""
    nb = bm.shape[1]
    w = np.full(nb, t >> 5, dtype=np.int64)
    m = bm[t >> 5] & (ALL >> np.uint32(31 - (t & 31)))
    lanes = np.arange(nb)
    while True:
        act = (m == 0) & (w > 0)
        if not act.any():
            return m, w
        step = np.full(nb, SCAN, dtype=np.int64)
        found = np.zeros(nb, dtype=np.uint32)
        for k in range(SCAN - 1, -1, -1):
            i = w - 1 - k
            e = np.where(i >= 0, bm[np.maximum(i, 0), lanes], 0).astype(np.uint32)
            hit = e != 0
            found = np.where(hit, e, found)
            step = np.where(hit, k + 1, step)
        m = np.where(act, found, m)
        w = np.where(act, w - step, w)


class SpanCache:
    def __init__(self):
        self.cw, self.pw, self.cv, self.pv = -1, -1, None, None
        self.fetches = 0   # top words fetched (one per word the run's frames pass through)


def index_last_writer_span(bm, tp, t, cache, wrong=None):
    """Per block: (m, w) for the last frame in (tp, t] that codes it."""
    nb = bm.shape[1]
    lo = tp + 1
    wb = lo >> 5
    mask_lo = ALL if wrong == "no_lower_mask" else np.uint32((0xFFFFFFFF << (lo & 31)) & 0xFFFFFFFF)
    wt = t >> 5
    if wt != cache.cw:
        cache.pw, cache.pv = cache.cw, cache.cv
        cache.cw, cache.cv = wt, bm[wt].copy()
        cache.fetches += 1
    w = np.full(nb, wt, dtype=np.int64)
    m = cache.cv & (ALL >> np.uint32(31 - (t & 31)))
    if wt == wb:
        return m & mask_lo, w
    if wrong == "top_word_only":
        return m, w
    lanes = np.arange(nb)
    while True:
        act = (m == 0) & (w > wb)
        if not act.any():
            return m, w
        step = np.full(nb, SCAN, dtype=np.int64)
        found = np.zeros(nb, dtype=np.uint32)
        for k in range(SCAN - 1, -1, -1):
            i = w - 1 - k
            e = np.where(i >= wb, bm[np.clip(i, 0, bm.shape[0] - 1), lanes], 0).astype(np.uint32)
            if cache.pv is not None:
                e = np.where(i == cache.pw, cache.pv, e).astype(np.uint32)   # (the same bits: the cache only saves the fetch)
                e = np.where(i >= wb, e, 0).astype(np.uint32)
            e = np.where(i == wb, e & mask_lo, e).astype(np.uint32)
            hit = e != 0
            found = np.where(hit, e, found)
            step = np.where(hit, k + 1, step)
        m = np.where(act, found, m)
        w = np.where(act, w - step, w)


def to_blocks(pic, w, h):
    """(h * w,) picture -> (nb, 16) block pixels (row-major inside the block), blocks in raster order."""
    nbx, nby = w // 4, h // 4
    p = np.asarray(pic).reshape(h, w)[:nby * 4, :nbx * 4]
    return p.reshape(nby, 4, nbx, 4).transpose(0, 2, 1, 3).reshape(nbx * nby, 16)


def put_blocks(pic, blocks, mask, w, h):
    """Store the blocks selected by mask into the (h * w,) picture."""
    nbx, nby = w // 4, h // 4
    view = pic.reshape(h, w)
    cur = to_blocks(pic, w, h)
    cur = np.where(mask[:, None], blocks, cur)
    view[:nby * 4, :nbx * 4] = cur.reshape(nby, nbx, 4, 4).transpose(0, 2, 1, 3).reshape(nby * 4, nbx * 4)


def remainder_mask(w, h):
    m = np.ones((h, w), dtype=bool)
    m[:(h // 4) * 4, :(w // 4) * 4] = False
    return m.reshape(-1)


def first_adopted(coded):
    any_ = coded.any(axis=1)
    return int(np.argmax(any_)) if any_.any() else coded.shape[0]


def segment_length(n, segs):
    segs = min(max(segs, 1), n)
    return (n + segs - 1) // segs


def play(coded, block_pics, w, h, first, n, stride, segs=1, before=None, wrong=None, fill=POISON):
    """The kernel's walk.  coded: (frames, nb) of the index's range; block_pics[f]: (nb, 16) pixels of the picture after frame f
    (a block frame f codes reads its code's pixels there); before: the (h * w,) picture before the range or None.
    Returns (dsts, stats): dsts[k] the (h * w,) buffer of frame first + k * stride, which held `fill` before."""
    bm = bitmap_words(coded)
    nb = coded.shape[1]
    fa = first_adopted(coded)
    dsts = [np.full(w * h, fill, dtype=np.int32) for _ in range(n)]
    null = [first + k * stride < fa for k in range(n)]
    rem = remainder_mask(w, h)
    seg = segment_length(n, segs)
    stats = {"top_fetches": 0, "decodes": 0}
    px = np.zeros((nb, 16), dtype=np.int32)
    have = np.zeros(nb, dtype=bool)
    t = first
    for k0 in range(0, n, seg):
        k1 = min(n, k0 + seg)
        if before is not None:   # the lanes past the last block
            for k in range(k0, k1):
                if not null[k]:
                    dsts[k][rem] = before[rem]
        carry = wrong == "carry_over_segment" and k0 > 0
        t = first + k0 * stride
        if not carry:   # compose the segment's first frame as Show does
            m, wd = index_last_writer(bm, t)
            found = m != 0
            px = np.zeros((nb, 16), dtype=np.int32)
            if found.any():
                f = 32 * wd[found] + _top_bit(m[found])
                px[found] = np.stack([block_pics[int(ff)][b] for ff, b in zip(f, np.nonzero(found)[0])])
                stats["decodes"] += int(found.sum())
            if before is not None:
                px[~found] = to_blocks(before, w, h)[~found]
                have = np.ones(nb, dtype=bool)
            else:
                have = found.copy()
        cache = SpanCache()
        k = k0
        while True:
            if not null[k]:
                put_blocks(dsts[k], px, have, w, h)
            k += 1
            if k >= k1:
                break
            tp, t = t, t + stride
            m, wd = index_last_writer_span(bm, tp, t, cache, wrong)
            found = m != 0
            if found.any():
                f = 32 * wd[found] + _top_bit(m[found])
                px[found] = np.stack([block_pics[int(ff)][b] for ff, b in zip(f, np.nonzero(found)[0])])
                have = have | found
                stats["decodes"] += int(found.sum())
        stats["top_fetches"] += cache.fetches
    return dsts, stats


def expected(truth_pics, coded, start, w, h, first, n, stride, fill=POISON):
    """What n Shows leave in buffers that held `fill`: the oracle's picture of each frame (truth_run of the whole clip from frame 0;
    the index covers clip frames start ..), nothing at all for a frame before the first adopting one."""
    fa = first_adopted(coded)
    out = []
    for k in range(n):
        t = first + k * stride
        out.append(np.full(w * h, fill, dtype=np.int32) if t < fa else np.asarray(truth_pics[start + t], dtype=np.int32))
    return out


# ---- the directed clip: a key frame cut short, then frames that code the blocks it left at different times -----------------------
def cut_short_clip(bits, w, h, seed=11):
    """(frames, keys, pal, at): frame 0 is a key frame cut short at block `at`, with no picture before it — 8-bit: an end marker there
    (the blocks from `at` on have no writer: they keep what the buffer held); 16-bit: the stream ends there (the reference paints the
    blocks whose codes are missing, so every block has frame 0 as its writer: there is no way to leave a 16-bit block without one).
    Frames 2, 3, 5, 8 and 9 then code parts of the blocks from `at` on, at different times; 1, 4, 6 and 7 code blocks before `at` or
    nothing."""
    from msv1_range_clips import Idle, palette
    g = Idle(bits, w, h, seed)
    nb = g.nb
    at = max(1, nb // 3)
    key = g.key()
    codes = [g.solid(v) for v in g.col]
    frame0 = g.encode(codes[:at]) + (b"\x00\x00" if bits == 8 else b"")
    late = list(range(at, nb))
    parts = [late[0::5], late[1::5], late[2::5], late[3::5], late[4::5]]
    early = list(range(0, at))
    frames, keys = [frame0], [True]
    plan = {1: early[::2], 2: parts[0], 3: parts[1], 4: [], 5: parts[2], 6: early[1::2], 7: [], 8: parts[3], 9: parts[4]}
    for i in range(1, 10):
        blocks = plan[i]
        frames.append(g.change(blocks) if blocks else g.all_skip("long"))
        keys.append(False)
    del key
    return frames, keys, palette(bits), at
