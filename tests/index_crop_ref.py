"""Reference for the frames of a block rectangle of a seek index (jsp_index_crop_frames / SeekIndex.CropFrames) — a helper module,
plain Python, no tests of its own.  Built on index_keyframe_ref.codes_of (WHOLE), index_delta_ref (written, the skip word, the 1023
rule) and index_tight_ref (kept).

THE RULE.  A rectangle is (bx, by, bw, bh) in 4x4 blocks in table order (block row 0 = stored rows 0 .. 3, the bottom of the picture
as displayed); nb = bw * bh; block j < nb of the rectangle is source block src(j) = (by + j // bw) * nbx + bx + j % bw.  The VIRTUAL
index has bw x bh blocks, and its block j is source block src(j): its codes_of tables are the source's, remapped through src.
  * a GAP pair (a, b], -1 <= a < b < nframes, is index_delta_ref.delta (tight: index_tight_ref.tight) of the virtual index —
    run heads, counts and the multiples of 1023 all in j;
  * a KEY pair (KEY, t) is the whole code of the last writer <= t of every block of the virtual index, in block order, no skip
    words: ("none", j) for the FIRST block without a writer or ("cut", j) for the first whose code is cut off, whichever block comes
    first.  tight does not touch it.
Blocks outside the rectangle never matter.

  * src, remap — the virtual index's tables;
  * Virtual — index_tight_ref.Pixels of the virtual index, over the Pixels of the source (block pixels from the oracle's pictures);
  * gap, key, crop — the bytes, or the refusal; flag — whether a frame codes every block of the rectangle;
  * `wrong` states one of four deliberately wrong variants (WRONG), each of which test_index_crop_ref_cpu.py shows to fail on a
    named clip."""
import index_delta_ref as dr
import index_tight_ref as tr

KEY = -2   # JSP_CROP_KEY
RUN = dr.RUN
WRONG = ("neighbour_in_source",       # the run-head test looks at source block src(j) - 1 instead of block j - 1 of the rectangle
         "run_in_source_numbering",   # the multiples of 1023 are taken in the picture's block numbers: src(j) % 1023
         "row_of_source",             # src takes the row as j // nbx instead of j // bw
         "key_skips_unwritten")       # a key pair skips a block without a writer instead of refusing


def src(nbx, rect, j, wrong=None):
    bx, by, bw, bh = rect
    assert 0 <= j < bw * bh
    row = j // nbx if wrong == "row_of_source" else j // bw
    return (by + row) * nbx + bx + j % bw


def remap(codes, nbx, rect, wrong=None):
    """codes_of tables of the virtual index: per frame, entry j = the source frame's entry src(j)."""
    order = [src(nbx, rect, j, wrong) for j in range(rect[2] * rect[3])]
    return [[c[i] for i in order] for c in codes]


class Virtual:
    """What index_tight_ref.tight and kept_set read of a Pixels, for the virtual index of `rect` over the source's `px`."""

    def __init__(self, px, nbx, rect, wrong=None):
        self.px, self.frames = px, px.frames
        self.order = [src(nbx, rect, j, wrong) for j in range(rect[2] * rect[3])]
        self.codes = [[c[i] for i in self.order] for c in px.codes]

    def block(self, t, j):
        return self.px.block(t, self.order[j])

    def code_bytes(self, f, j):
        return self.px.code_bytes(f, self.order[j])


def _emit(frames, vcodes, w, head, limit):
    """Delta's loop with the run-head test and the count's limit handed in (the wrong variants)."""
    nb = len(w)
    out = bytearray()
    for j in range(nb):
        if w[j] is not None:
            if vcodes[w[j]][j] == "cut":
                return ("cut", j)
            o, length = vcodes[w[j]][j]
            out += bytes(frames[w[j]])[o:o + length]
            continue
        if not head(j):
            continue
        nxt = next((k for k in range(j + 1, nb) if w[k] is not None), nb)
        out += dr.skip_word(max(1, min(min(nxt, limit(j), nb) - j, RUN)))
    return bytes(out)


def gap(bits, nbx, frames, rect, a, b, codes, tight=False, px=None, wrong=None):
    """codes: codes_of of every frame of the SOURCE index; px: index_tight_ref.Pixels of the source (tight only)."""
    assert wrong in (None,) + WRONG
    bx, by, bw, bh = rect
    nb = bw * bh
    if wrong in (None, "row_of_source", "key_skips_unwritten"):
        if tight:
            return tr.tight(Virtual(px, nbx, rect, wrong), a, b)
        return dr.delta(bits, bw, bh, frames, a, b, remap(codes, nbx, rect, wrong))
    vcodes = remap(codes, nbx, rect)
    if tight:
        kept = set(tr.kept_set(Virtual(px, nbx, rect), a, b)[1])
        w = [dr.writer(vcodes, a, b, j) if j in kept else None for j in range(nb)]
        full = set(tr.kept_set(px, a, b)[1])
    else:
        w = [dr.writer(vcodes, a, b, j) for j in range(nb)]
        full = set(i for i in range(len(codes[0])) if dr.writer(codes, a, b, i) is not None)
    if wrong == "neighbour_in_source":
        def head(j):
            s = src(nbx, rect, j)
            return j == 0 or s == 0 or s - 1 in full or j % RUN == 0
        return _emit(frames, vcodes, w, head, lambda j: (j // RUN + 1) * RUN)

    def head(j):   # run_in_source_numbering
        return j == 0 or w[j - 1] is not None or src(nbx, rect, j) % RUN == 0

    def limit(j):
        return next((k for k in range(j + 1, nb) if src(nbx, rect, k) % RUN == 0), nb)
    return _emit(frames, vcodes, w, head, limit)


def key(bits, nbx, frames, rect, t, codes, wrong=None):
    assert 0 <= t < len(frames) and wrong in (None,) + WRONG
    vcodes = remap(codes, nbx, rect, wrong)
    if wrong == "key_skips_unwritten":
        return dr.delta(bits, rect[2], rect[3], frames, -1, t, vcodes)
    out = bytearray()
    for j in range(rect[2] * rect[3]):
        f = dr.writer(vcodes, -1, t, j)
        if f is None:
            return ("none", j)
        if vcodes[f][j] == "cut":
            return ("cut", j)
        o, length = vcodes[f][j]
        out += bytes(frames[f])[o:o + length]
    return bytes(out)


def crop(bits, nbx, frames, rect, pair, codes, tight=False, px=None, wrong=None):
    a, b = pair
    if a == KEY:
        return key(bits, nbx, frames, rect, b, codes, wrong)
    return gap(bits, nbx, frames, rect, a, b, codes, tight, px, wrong)


def writer(codes, nbx, rect, pair, j):
    """The frame a ("cut", j) refusal of `pair` names: the last writer of src(j) up to the pair's frame."""
    a, b = pair
    return dr.writer(codes, -1 if a == KEY else a, b, src(nbx, rect, j))


def flag(bits, data, nb):
    """keys[] of a frame: it codes every block of the rectangle (its words are nb codes and no skip)."""
    codes, skips, blocks = dr.walk(bits, data)
    return len(codes) == nb and not skips
