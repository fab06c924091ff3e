"""The directed clips of tests/sp_directed_clips.py, without a GPU: they are exact on the CPU, they contain what they were painted
for (a census, asserted), and deliberately wrong walks fail on them.

The census is taken from the host stage's own records (sp_index_ref.Composer), that is from what the index kernels are given,
not from what the painter meant.  `Walk` restates the two kernels' walks per block and per 32-frame bitmap word — backwards as
index_compose goes, forwards as sp_index_play_kernel goes — and must equal Composer.picture and sp_index_play_ref.play; its
`fault` argument makes one of six mistakes, in numpy only:

    a  the backward walk stops after 8 records (two steps of SHOW_AHEAD = 4)
    b  the records of one bitmap word are applied oldest first
    c  the key boundary is not applied in the key frame's own word
    d  the forward walk drops bit 31 of `range`
    e  the forward walk skips a key frame that sits at bit 0 of a word
    f  the forward walk keeps the record fetched ahead when a writer at bit 0 follows a writer at bit 31 of the word before

Every one gives a wrong frame on the directed clips (asserted).  What the random clips let through — the seven clips of
test_sp_index_ref_cpu.CASES, every frame shown, and played as (0, n, 1), (1, n - 1, 1), (n // 3, n // 2, 1), (0, (n + 1) // 2, 2)
— observed with `PYTHONPATH=. python tests/test_sp_directed_clips_cpu.py`, not asserted:

    fault   wrong frames on A / B / C     random clips that notice it (of 7)
    a       103 / 131 / 113               0
    b       123 / 136 / 127               6
    c       0 / 0 / 30                    6
    d       82 / 205 / 77                 1
    e       143 / 0 / 121                 0
    f       18 / 201 / 68                 0

(c shows on C alone, behind its flat key frame at 33: on A the frames behind a key frame never share a bitmap word with inter
frames before it — its key frames are at bit 31 and bit 0 — and B's only key frame is frame 0.)  The random clips let a, e and f
through whole, and d but for one clip.
"""
import numpy as np
import pytest

import sp_directed_clips as dc
import sp_index_play_ref as play_ref
import sp_index_ref as ref

SHOW_AHEAD = 4     # sp_index_kernels.hip
NAMES = ("A", "B", "C")
_composers = {}


def composer(name):
    if name not in _composers:
        _composers[name] = ref.Composer(dc.clip(name), preinit=dc.KEY_ROW)
    return _composers[name]


class Walk:
    """The index's tables as the kernels see them — bitmap[word][block], bit j: frame 32 word + j writes the block — and the two
    walks over them."""

    def __init__(self, comp):
        self.comp = comp
        c = comp.clip
        self.n = len(c.keys)
        self.nbx, self.nby = dc.geometry(c.w, c.h)
        self.nblocks = self.nbx * self.nby
        self.where = [(slice(by * 16, min(by * 16 + 16, c.h)), slice(bx * 16, min(bx * 16 + 16, c.w)))
                      for by in range(self.nby) for bx in range(self.nbx)]
        self.bitmap = [[0] * self.nblocks for _ in range((self.n + 31) // 32)]
        self.block_of = np.zeros((c.h, c.w), dtype=np.int32)
        for b, at in enumerate(self.where):
            self.block_of[at] = b
        for f, mask in comp.mask.items():
            for b, at in enumerate(self.where):
                if mask[at].any():
                    self.bitmap[f >> 5][b] |= 1 << (f & 31)

    def writers(self, b, lo, hi):
        """The frames of [lo, hi] that write block b."""
        return [f for f in range(max(lo, 0), hi + 1) if (self.bitmap[f >> 5][b] >> (f & 31)) & 1]

    def rect(self, f, b):
        """(x1, y1, x2, y2) of frame f's rectangle in block b, inside the block."""
        ys, xs = np.nonzero(self.comp.mask[f][self.where[b]])
        assert len(ys) == (ys.max() + 1 - ys.min()) * (xs.max() + 1 - xs.min()), "a block's changed pixels are one rectangle"
        return int(xs.min()), int(ys.min()), int(xs.max()) + 1, int(ys.max()) + 1

    def backward(self, t, fault=None, trace=None):
        """Frame t as index_compose makes it.  trace[b] = (records applied, the frame whose record completed the block or None)."""
        comp = self.comp
        k = comp.key_of[t]
        out = comp.key_pic[k].copy()
        if t <= k:
            return out.reshape(-1)
        wlo = (k + 1) >> 5
        for b, at in enumerate(self.where):
            need = np.ones(out[at].shape, bool)
            px = out[at]                      # (a view: the block's pixels of `out`)
            count, done = 0, None
            w = t >> 5
            m = self.bitmap[w][b] & (0xFFFFFFFF >> (31 - (t & 31)))
            is_open = True
            while is_open:
                if w == wlo and fault != "c":
                    m &= (0xFFFFFFFF << ((k + 1) & 31)) & 0xFFFFFFFF
                bits = [j for j in range(31, -1, -1) if (m >> j) & 1]
                if fault == "b":
                    bits.reverse()
                for j in bits:
                    f = 32 * w + j
                    take = comp.mask[f][at] & need
                    px[take] = comp.lit[f][at][take]
                    need &= ~comp.mask[f][at]
                    count += 1
                    if not need.any():
                        is_open, done = False, f
                    if fault == "a" and count == 2 * SHOW_AHEAD:
                        is_open = False
                    if not is_open:
                        break
                if w == wlo:
                    break
                w -= 1
                m = self.bitmap[w][b]
            if trace is not None:
                trace[b] = (count, done)
        return out.reshape(-1)

    def forward(self, first, n, stride=1, fault=None):
        """The run as sp_index_play_kernel makes it: frame `first` composed backwards, then one bitmap word and one key-mask word
        per 32 frames."""
        comp = self.comp
        keys = comp.clip.keys
        last = first + (n - 1) * stride
        assert n >= 1 and stride >= 1 and 0 <= first and last < self.n
        px = self.backward(first).reshape(comp.clip.h, comp.clip.w).copy()
        out = [px.reshape(-1).copy()]
        next_out = first + stride
        for w in range(first >> 5, (last >> 5) + 1):
            lo, hi = max(first + 1, 32 * w), min(last, 32 * w + 31)
            if lo > hi:
                continue
            in_range = (0xFFFFFFFF << (lo & 31)) & (0xFFFFFFFF >> (31 - (hi & 31))) & 0xFFFFFFFF
            if fault == "d":
                in_range &= 0x7FFFFFFF
            m = [self.bitmap[w][b] & in_range for b in range(self.nblocks)]
            km = sum(1 << (f & 31) for f in range(32 * w, min(32 * w + 32, self.n)) if keys[f]) & in_range
            if fault == "e":
                km &= ~1
            om = 0
            f = next_out
            while f <= hi:
                om |= 1 << (f & 31)
                f += stride
            for bit in range(32):
                f = 32 * w + bit
                blocks = [b for b in range(self.nblocks) if (m[b] >> bit) & 1]
                if fault == "f" and bit == 0 and f - 1 > first:
                    blocks = [b for b in blocks if not (self.bitmap[w - 1][b] >> 31) & 1]   # the stale record is applied again
                if blocks:
                    take = comp.mask[f] & np.isin(self.block_of, blocks)
                    px[take] = comp.lit[f][take]
                elif (km >> bit) & 1:
                    px = comp.key_pic[f].copy()
                if (om >> bit) & 1:
                    assert f == next_out
                    out.append(px.reshape(-1).copy())
                    next_out += stride
        return out


_walks = {}


def walk(name):
    if name not in _walks:
        _walks[name] = Walk(composer(name))
    return _walks[name]


# ------------------------------------------------------------------------------------------------------------------ exactness

@pytest.mark.parametrize("name", NAMES)
def test_every_pixel_names_its_last_writer(name):
    """writer_of of every painted pixel is the last frame whose region covers it, else the key frame — worked out from
    regions() alone."""
    w, h, bpp, _, coded, flat = dc.SPECS[name]
    clip = dc.clip(name)
    nbx, _ = dc.geometry(w, h)
    last = np.zeros((h, w), dtype=np.int64)
    decode = np.vectorize(lambda v: dc.writer_of(v, bpp))
    for t in range(dc.N):
        if t in coded or t in flat:
            last[:] = t
        else:
            for b, (x1, y1, x2, y2) in dc.regions(t, w, h).items():
                by, bx = divmod(b, nbx)
                last[by * 16 + y1:by * 16 + y2, bx * 16 + x1:bx * 16 + x2] = t
        assert np.array_equal(decode(clip.frames[t]).reshape(h, w), last), f"frame {t}"
    i = 9 * w + 9                                   # position (7 * 95) % 256 = 153 of block 0: frame 95's own pixel
    got = clip.frames[95].copy()
    got[i] = clip.frames[64][i]
    text = dc.describe_mismatch(got, clip.frames[95], w, h, bpp)
    stale = dc.writer_of(clip.frames[64][i], bpp)
    assert stale < 95 and "first in block 0, row 9, col 9: want writer frame 95, got frame %d " % stale in text, text
    assert dc.describe_mismatch(clip.frames[95], clip.frames[95], w, h, bpp) == ""


@pytest.mark.parametrize("name", NAMES)
def test_encoder_oracle_and_composition_equal_the_painting(name):
    clip = dc.clip(name)
    pictures, verdicts = dc.oracle(name)
    comp, wk = composer(name), walk(name)
    assert len(clip.chunks) == dc.N and clip.keys[0]
    for t in range(dc.N):
        want = clip.frames[t]
        for what, got in (("the encoder's picture", clip.encoder_frames[t]), ("the oracle's picture", pictures[t]),
                          ("Composer.picture", comp.picture(t)), ("the walk by words", wk.backward(t))):
            assert np.array_equal(got, want), f"{clip.name} frame {t}, {what}: " + dc.describe_mismatch(got, want, clip.w, clip.h, clip.bpp)
        if not clip.keys[t]:
            assert comp.verdict_p[t] == verdicts[t], f"frame {t}: host-stage verdict differs from DecompressP's"
    assert True in verdicts[1:] and False in verdicts[1:], "the verdicts tell nothing apart"


@pytest.mark.parametrize("name", NAMES)
def test_play_reference_equals_the_painting_on_every_run(name):
    clip = dc.clip(name)
    comp, wk = composer(name), walk(name)
    for first, count, stride in dc.play_runs():
        got = play_ref.play(comp, first, count, stride)
        for k, pic in enumerate(got):
            t = first + k * stride
            assert np.array_equal(pic, clip.frames[t]), f"{clip.name} play({first}, {count}, {stride}) frame {t}: " + \
                dc.describe_mismatch(pic, clip.frames[t], clip.w, clip.h, clip.bpp)
    for first, count, stride in [(0, dc.N, 1), (30, 40, 1), (31, 3, 1), (5, 5, 32), (33, 4, 31), (62, 3, 1), (1, 70, 2)]:
        for a, b in zip(wk.forward(first, count, stride), play_ref.play(comp, first, count, stride)):
            assert np.array_equal(a, b), f"{clip.name}: the walk by words differs from play_ref.play on ({first}, {count}, {stride})"


def test_saturated_clip_is_exact_and_saturated():
    import thumbs_ref as tr
    clip = dc.clip("S")
    pictures, _ = dc.oracle("S")
    comp = ref.Composer(clip, preinit=dc.KEY_ROW)
    for t in range(4):
        assert np.array_equal(pictures[t], clip.frames[t]) and np.array_equal(comp.picture(t), clip.frames[t])
        assert np.array_equal(clip.encoder_frames[t], clip.frames[t])
    for s in tr.SCALES:
        for t in (1, 2, 3):
            th = tr.thumbnail(clip.frames[t], clip.w, clip.h, s).view(np.uint32)
            for shift in (0, 8, 16):
                ch = (th >> shift) & 0xFF
                beside = ((ch[:, :-1] == 255) & (ch[:, 1:] == 0)) | ((ch[:, :-1] == 0) & (ch[:, 1:] == 255))
                assert beside.any(), f"scale {s} frame {t}: no cell of 255 beside a cell of 0 in the channel at bit {shift}"


# --------------------------------------------------------------------------------------------------------------------- census

_census = {}


def census(name, clip=None):
    """What the clip holds, from the host stage's records: a dict of the facts the tests below assert.  `clip`: a variant of the
    named clip, taken afresh."""
    if clip is None:
        if name not in _census:
            _census[name] = census(name, dc.clip(name))
        return _census[name]
    if clip is dc.clip(name):
        comp, wk = composer(name), walk(name)
    else:
        comp = ref.Composer(clip, preinit=dc.KEY_ROW)
        wk = Walk(comp)
    clip = comp.clip
    c = dict(popcount={}, depth=0, depth_at=None, early=[], early_raw=[], shapes=set(), bits=set(), motion=max(comp.motion_share.values()))
    for w, row in enumerate(wk.bitmap):
        for b, m in enumerate(row):
            c["popcount"][(w, b)] = bin(m).count("1")
            c["bits"] |= {j for j in range(32) if (m >> j) & 1}
    pw, ph = clip.w - 16 * (wk.nbx - 1), clip.h - 16 * (wk.nby - 1)
    for f in comp.mask:
        for b in range(wk.nblocks):
            if not (wk.bitmap[f >> 5][b] >> (f & 31)) & 1:
                continue
            x1, y1, x2, y2 = wk.rect(f, b)
            by, bx = divmod(b, wk.nbx)
            if (x2 - x1, y2 - y1) == (1, 1):
                c["shapes"].add("1x1")
            if (x1, x2) == (0, 16) and y2 - y1 == 1:
                c["shapes"].add("full row")
            if (x1, x2) == (0, 1) and y2 - y1 == 16:
                c["shapes"].add("column at x = 0")
            if (x1, x2) == (15, 16) and y2 - y1 == 16:
                c["shapes"].add("column at x = 15")
            if bx == wk.nbx - 1 and x2 == pw:
                c["shapes"].add("reaches the right edge of a block %d wide" % pw)
            if by == wk.nby - 1 and (y1, y2) == (ph - 2, ph):
                c["shapes"].add("the picture's last two rows")
    for t in range(len(clip.keys)):
        k = comp.key_of[t]
        if t == k:
            continue
        trace = {}
        wk.backward(t, trace=trace)
        for b, (count, done) in trace.items():
            if count > c["depth"]:
                c["depth"], c["depth_at"] = count, (t, b)
            if count == 16 and done is not None:
                below = wk.writers(b, k + 1, done - 1)
                same = [f for f in below if f >> 5 == done >> 5]
                if same and any(f >> 5 < done >> 5 for f in below):
                    c["early"].append((t, b))
                if same and any(wk.bitmap[w][b] for w in range(done >> 5)):
                    c["early_raw"].append((t, b))
    return c


def test_census_dense_words_and_deep_walks():
    a, b, c = census("A"), census("B"), census("C")
    assert a["popcount"][(2, 0)] == 32, "A: block 0 is not written in all 32 frames of word 2"
    assert max(b["popcount"].values()) == 32, "B: no block is written in all 32 frames of a word"
    trace = {}
    walk("A").backward(95, trace=trace)
    assert trace[0] == (32, None), "A: block 0 of frame 95 does not walk 32 records down to the key frame"
    for name, cs in (("A", a), ("B", b), ("C", c)):
        assert cs["depth"] >= 3 * SHOW_AHEAD + 1, f"{name}: no walk needs a fourth step"
    assert b["depth"] == 139, "B: block 0 of the last frame does not walk all 139 inter frames"
    assert b["popcount"][(1, 7)] == 9 and b["popcount"][(3, 7)] == 9 and b["popcount"][(2, 7)] == 0, "B: block 7 has no empty middle word"


def test_census_blocks_complete_with_writers_left_below():
    """A block complete after exactly 16 records while set bits stay unvisited below — in the same word and in an earlier one.
    On B and C those are writers of (key, t].  On A no run of inter frames allows that: its key frames at 31, 32, 63 and 96 are
    each wanted where they are, and the 43 frames behind 96 end in a word of 12, so a walk that completes with bits left in its
    word is in the key frame's own word; there the earlier word's set bits are those of frames before the key frame."""
    assert census("B")["early"] and census("C")["early"]
    assert census("A")["early_raw"]
    assert (139, 1) in census("B")["early"]


def test_census_word_boundaries():
    for name in NAMES:
        assert {0, 31} <= census(name)["bits"], f"{name}: no writer at bit 0 and bit 31 of a word"
        assert census(name)["motion"] == 0, f"{name}: a block is coded as motion"
    clip = dc.clip("A")
    kind = {t: clip.chunks[t][0] & 0xF for t in range(dc.N) if clip.keys[t]}      # 1: flat, 2: coded
    assert kind == {0: 2, 31: 2, 32: 2, 63: 1, 96: 2}
    comp = composer("A")
    assert all(f in comp.mask for f in range(64, 96)), "A: not a full word of inter frames before the key frame at 96"
    kind_c = {t: dc.clip("C").chunks[t][0] & 0xF for t in range(dc.N) if dc.clip("C").keys[t]}
    assert kind_c == {0: 2, 33: 1, 64: 2}
    assert sum(dc.clip("B").keys) == 1


def test_census_rectangle_shapes():
    want = {"1x1", "full row", "column at x = 0", "column at x = 15", "the picture's last two rows"}
    for name in NAMES:
        assert want <= census(name)["shapes"], f"{name}: missing {want - census(name)['shapes']}"
    assert "reaches the right edge of a block 3 wide" in census("B")["shapes"]
    assert "reaches the right edge of a block 4 wide" in census("A")["shapes"]


def test_the_census_notices_a_missing_role():
    """Without block 0's pixel per frame the dense word and the 1x1 rectangles are gone, without block 1's row per frame the
    blocks that complete with writers left below."""
    soft = census("A", dc.build("A", skip=(0,)))
    assert soft["popcount"][(2, 0)] == 0 and "1x1" not in soft["shapes"]
    soft = census("B", dc.build("B", skip=(1,)))
    assert not soft["early"] and "full row" not in soft["shapes"]


# ---------------------------------------------------------------------------------------------------------------- wrong walks

FAULT_RUNS = [(0, dc.N, 1), (30, 40, 1), (62, 3, 1), (1, 70, 2)]


def wrong_frames(wk, fault, runs, frames):
    """How many frames the faulty walk gets wrong: every frame shown for a, b, c; the frames of `runs` played for d, e, f."""
    if fault in "abc":
        return sum(1 for t in range(wk.n) if not np.array_equal(wk.backward(t, fault), frames[t]))
    bad = 0
    for first, count, stride in runs:
        got = wk.forward(first, count, stride, fault)
        bad += sum(1 for k, pic in enumerate(got) if not np.array_equal(pic, frames[first + k * stride]))
    return bad


@pytest.mark.parametrize("fault", list("abcdef"))
def test_a_wrong_walk_fails_on_the_directed_clips(fault):
    bad = {name: wrong_frames(walk(name), fault, FAULT_RUNS, dc.clip(name).frames) for name in NAMES}
    assert sum(bad.values()) > 0, f"fault {fault} passes every directed clip"
    if fault == "a":
        assert bad["B"] > 0, "the scalar clip does not notice a walk that stops after 8 records"


def observed_table():
    import test_sp_index_ref_cpu as old
    lines = []
    for fault in "abcdef":
        directed = " / ".join("%d" % wrong_frames(walk(name), fault, FAULT_RUNS, dc.clip(name).frames) for name in NAMES)
        noticed = 0
        for cfg, w, h, n, bpp, version, key_every, key_row in old.CASES:
            clip = ref.make_clip(cfg, w, h, n, bpp, version, key_every, key_row)
            wk = Walk(ref.Composer(clip))
            runs = [(0, n, 1), (1, n - 1, 1), (n // 3, n // 2, 1), (0, (n + 1) // 2, 2)]
            noticed += wrong_frames(wk, fault, runs, clip.frames) > 0
        lines.append("    %s       %-29s %d" % (fault, directed, noticed))
    return "\n".join(lines)


if __name__ == "__main__":
    print(observed_table())
