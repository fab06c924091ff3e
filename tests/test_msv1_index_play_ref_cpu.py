"""The numpy model of msv1_index_play_kernel (msv1_index_play_ref.play) against the oracle's frame-by-frame truth — no GPU.

The model has the kernel's control flow: compose the first frame, a bounded last writer per further frame, the `have` flag, null
destinations before the first adopting frame, segments.  Truth is truth_run: the oracle with each destination first copied from
the picture before it, poison where there is none.

Three deliberately wrong walks must be caught by the listed cases:
  * top_word_only       looks only at the top word of a span: wrong pictures;
  * carry_over_segment  keeps the registers of the segment before instead of composing a segment's first frame: wrong pictures;
  * no_lower_mask       forgets the lower-bound mask.  A coded block overwrites the whole block, so the writer such a walk finds
                        below the bound is the very one whose pixels the lane already holds: the pictures stay right, and what
                        fails is the work — codes decoded again.  The check is the count of decodes against the plan's count of
                        (block, frame) pairs with a writer in the gap."""
import functools

import numpy as np
import pytest

import msv1_index_play_ref as ref
from msv1_range_clips import POISON, long_clip, make_plan, truth_run

W, H = 24, 16
STRIDES = (1, 2, 31, 32, 33, 64, 100, 170)
STARTS = (0, 75, 133)   # no picture before; LATE blocks come from the picture before; the range begins with an all-skip frame


@functools.lru_cache(maxsize=None)
def clip(bits):
    frames, keys, pal, plan = long_clip(bits, W, H, seed=3)
    truth = truth_run(bits, W, H, pal, frames, keys, lines=plan["lines"], key_row=plan["lines"])
    pics = [t[0] for t in truth]
    blocks = [ref.to_blocks(p, W, H) for p in pics]
    return plan, pics, blocks


def cases(n_index):
    """(first, n, stride, segs) over an index of n_index frames: every stride, a `first` next to the word boundaries, the whole run."""
    out = []
    for stride in STRIDES:
        for first in (0, 1, 30, 31, 32, 33, 63, 65):
            if first >= n_index:
                continue
            n = (n_index - 1 - first) // stride + 1
            for segs in ((1, 2, 3, n) if first in (0, 31, 33) else (1, 3)):
                out.append((first, n, stride, segs))
    return out


def run_case(bits, start, first, n, stride, segs, wrong=None):
    """(pictures right, decodes right) of one run of the model."""
    plan, pics, blocks = clip(bits)
    coded = plan["coded"][start:]
    before = pics[start - 1] if start > 0 else None
    got, stats = ref.play(coded, blocks[start:], W, H, first, n, stride, segs, before, wrong)
    want = ref.expected(pics, coded, start, W, H, first, n, stride)
    same = all(np.array_equal(g, x) for g, x in zip(got, want))
    # decodes: per segment, the blocks with a writer <= its first frame, then per further frame the blocks coded in the gap
    seg = ref.segment_length(n, segs)
    count = 0
    for k in range(n):
        t = first + k * stride
        if k % seg == 0:
            count += int(coded[:t + 1].any(axis=0).sum())
        else:
            count += int(coded[t - stride + 1:t + 1].any(axis=0).sum())
    return same, stats["decodes"] == count, stats


@pytest.mark.parametrize("bits", [16, 8])
@pytest.mark.parametrize("start", STARTS)
def test_the_walk_shows_what_the_oracle_shows(bits, start):
    plan, _, _ = clip(bits)
    assert not plan["raises"]
    n_index = plan["n"] - start
    if start == 133:
        assert ref.first_adopted(plan["coded"][start:]) > 0, "the range should begin with frames that code nothing"
    for first, n, stride, segs in cases(n_index):
        same, exact, _ = run_case(bits, start, first, n, stride, segs)
        assert same, f"{bits}-bit start={start} first={first} n={n} stride={stride} segs={segs}: pictures"
        assert exact, f"{bits}-bit start={start} first={first} n={n} stride={stride} segs={segs}: decodes"


def test_a_word_is_fetched_once_while_the_run_stays_in_it():
    plan, _, _ = clip(16)
    for stride in (1, 2, 31, 32):
        n = (plan["n"] - 1) // stride + 1
        _, _, stats = run_case(16, 0, 0, n, stride, 1)
        words = len({(k * stride) >> 5 for k in range(1, n)})
        assert stats["top_fetches"] == words, stride


@pytest.mark.parametrize("wrong, what", [("top_word_only", "pictures"), ("carry_over_segment", "pictures"), ("no_lower_mask", "decodes")])
def test_each_wrong_walk_is_caught(wrong, what):
    caught = 0
    for bits in (16, 8):
        plan, _, _ = clip(bits)
        for first, n, stride, segs in cases(plan["n"]):
            same, exact, _ = run_case(bits, 0, first, n, stride, segs, wrong)
            caught += (not same) if what == "pictures" else (not exact)
            if wrong == "no_lower_mask":
                assert same, "a walk without the lower mask decodes too much, but what it decodes is what the lane holds"
    assert caught > 0, f"no listed case tells the {wrong} walk from the right one"


@pytest.mark.parametrize("bits", [16, 8])
def test_the_key_frame_cut_short(bits):
    frames, keys, pal, at = ref.cut_short_clip(bits, W, H)
    plan = make_plan(bits, W, H, frames, keys, 36)
    assert not plan["raises"]
    coded = plan["coded"]
    nb = plan["nb"]
    truth = truth_run(bits, W, H, pal, frames, keys)
    pics = [t[0] for t in truth]
    blocks = [ref.to_blocks(p, W, H) for p in pics]
    if bits == 8:
        # at least one block has no writer at `first`, and gets one inside the run — and they get theirs at different times
        none_at_first = ~coded[:1].any(axis=0)
        gets_one = coded[1:].any(axis=0)
        assert (none_at_first & gets_one).any()
        when = {int(np.argmax(coded[:, b])) for b in np.nonzero(none_at_first & gets_one)[0]}
        assert len(when) > 1, when
        assert np.all(ref.to_blocks(pics[0], W, H)[at:] == np.int32(POISON))
    else:
        # a 16-bit stream that ends early paints the blocks whose codes are missing (the reference reads the missing bytes as 0): every
        # block has frame 0 as its writer, and nothing the buffer held shows through
        assert coded[0].all() and not np.any(pics[0].reshape(H, W)[:H // 4 * 4, :W // 4 * 4] == np.int32(POISON))
    for first in range(len(frames)):
        for stride in (1, 2, 3):
            n = (len(frames) - 1 - first) // stride + 1
            for segs in (1, 2, 3, n):
                got, _ = ref.play(coded, blocks, W, H, first, n, stride, segs, None)
                want = ref.expected(pics, coded, 0, W, H, first, n, stride)
                assert all(np.array_equal(g, x) for g, x in zip(got, want)), (bits, first, stride, segs)
    if bits == 8:   # the early destinations keep the buffer's content in the blocks cut off, the later ones do not
        got, _ = ref.play(coded, blocks, W, H, 0, len(frames), 1, 1, None)
        assert np.any(ref.to_blocks(got[0], W, H)[at:] == np.int32(POISON))
        assert not np.any(ref.to_blocks(got[-1], W, H)[:nb] == np.int32(POISON))
