"""Reference for the TIGHT inter frame that spans a gap of a seek index (jsp_index_tight_frames / SeekIndex.DeltaFrames(tight=True)) — a
helper module, plain Python, no tests of its own.  Built on index_delta_ref (written, the skip word, the 1023 rule) and
index_keyframe_ref.codes_of (WHOLE).

THE RULE.  P(t)[i] is the 16 frame-buffer words that the last frame <= t coding block i makes of it, else the block of the picture
before the index; P(a)[i] is DEFINED when one of the two exists (a = -1: only the picture before the index can define it).  Block i is
KEPT in (a, b] when it is written in (a, b] and either P(a)[i] is not defined or P(b)[i] != P(a)[i] in at least one of the 16 words;
every other block is DROPPED.  Tight(a, b) is index_delta_ref's rule with "written" replaced by "kept" everywhere: in the codes, in
the run-head test (is block i - 1 kept?) and in the counts.  Only a KEPT block whose last writer's code is cut refuses.

  * Pixels — where P(t)[i] comes from: the per-block decode of pyref_msv1 of the writer's whole code (nothing of the oracle), or whole
    pictures passed in (pictures[t] = the picture of index frame t; needed where a writer's code is cut: pyref decodes valid codes only);
  * kept_set — (written, kept) of a gap;
  * tight — the bytes, or ("cut", block) with the FIRST kept block that refuses.  `wrong` states one of four deliberately wrong
    variants (WRONG), each of which test_index_tight_ref_cpu.py shows to fail on a directed clip."""
import numpy as np

import index_delta_ref as dr
import pyref_msv1 as pyref

RUN = dr.RUN
WRONG = ("first_pixel_only",     # the compare looks at word 0 of the 16 only
         "bytes_not_pixels",     # a block is unchanged only if the two codes' bytes are equal
         "neighbour_written",    # the run-head test asks whether block i - 1 is WRITTEN instead of KEPT
         "dropped_refuses")      # a dropped block with a cut code refuses


class Pixels:
    """P(t)[i] of an index over `frames` (codes: codes_of of each): block(t, i) = a tuple of 16 words, or None where it is not
    defined.  before: the picture before the index (w * h words) or None.  pictures: whole pictures by index frame, or None for the
    per-block decode."""

    def __init__(self, bits, w, h, frames, codes, pal=None, before=None, pictures=None):
        self.bits, self.w, self.h, self.nbx = bits, w, h, w // 4
        self.frames, self.codes = frames, codes
        self.pal = pyref.palette_ints(pal) if bits == 8 else None
        self.before = None if before is None else np.asarray(before).reshape(h, w)
        self.pictures = pictures
        self._decoded, self._rows = {}, {}

    @staticmethod
    def _words(a):
        return tuple(int(v) & 0xFFFFFFFF for v in np.asarray(a).reshape(-1))

    def _of_picture(self, t, i):
        """Block i of pictures[t] (t = -1: of `before`); a picture's blocks are cut out once."""
        if t not in self._rows:
            pic = np.asarray(self.before if t < 0 else self.pictures[t]).reshape(self.h, self.w).astype(np.int64) & 0xFFFFFFFF
            nby = self.h // 4
            cut = pic[:4 * nby, :4 * self.nbx].reshape(nby, 4, self.nbx, 4).transpose(0, 2, 1, 3).reshape(-1, 16)
            self._rows[t] = [tuple(r) for r in cut.tolist()]
        return self._rows[t][i]

    def code_bytes(self, f, i):
        """The bytes of frame f's code of block i as far as the frame has them (a cut code: fewer than its length)."""
        c = self.codes[f][i]
        data = bytes(self.frames[f])
        if c == "cut":
            return None
        return data[c[0]:c[0] + c[1]]

    def block(self, t, i):
        f = dr.writer(self.codes, -1, t, i) if t >= 0 else None
        if f is None:
            return None if self.before is None else self._of_picture(-1, i)
        if self.pictures is not None:
            return self._of_picture(t, i)
        if (f, i) not in self._decoded:
            code = self.code_bytes(f, i)
            if code is None:
                raise ValueError(f"block {i}: the code of frame {f} is cut off; its pixels need whole pictures")
            self._decoded[(f, i)] = self._words(pyref.decode(self.bits, 4, 4, code, palette=self.pal)[0])
        return self._decoded[(f, i)]


def kept_set(px, a, b, wrong=None):
    """(written, kept): the blocks some frame of (a, b] codes, and those of them the rule keeps, both ascending."""
    codes = px.codes
    nb = len(codes[0])
    written, kept = [], []
    for i in range(nb):
        f = dr.writer(codes, a, b, i)
        if f is None:
            continue
        written.append(i)
        if wrong == "bytes_not_pixels":
            fa = dr.writer(codes, -1, a, i) if a >= 0 else None
            same = fa is not None and px.code_bytes(fa, i) is not None and px.code_bytes(fa, i) == px.code_bytes(f, i)
            if not same:
                kept.append(i)
            continue
        pa = px.block(a, i)
        if pa is None:
            kept.append(i)
            continue
        pb = px.block(b, i)
        if (pa[0] != pb[0]) if wrong == "first_pixel_only" else (pa != pb):
            kept.append(i)
    return written, kept


def tight(px, a, b, wrong=None):
    """px: Pixels of the index's range."""
    codes, frames = px.codes, px.frames
    assert -1 <= a < b < len(frames) and wrong in (None,) + WRONG
    nb = len(codes[0])
    written, kept = kept_set(px, a, b, wrong)
    ws, ks = set(written), set(kept)
    w = [dr.writer(codes, a, b, i) if i in ws else None for i in range(nb)]
    out = bytearray()
    for i in range(nb):
        if i in ks or (wrong == "dropped_refuses" and i in ws):
            if codes[w[i]][i] == "cut":
                return ("cut", i)
        if i in ks:
            o, length = codes[w[i]][i]
            out += bytes(frames[w[i]])[o:o + length]
            continue
        before = ws if wrong == "neighbour_written" else ks
        if not (i == 0 or i - 1 in before or i % RUN == 0):
            continue
        nxt = next((k for k in range(i + 1, nb) if k in ks), nb)
        out += dr.skip_word(min(nxt, (i // RUN + 1) * RUN, nb) - i)
    return bytes(out)
