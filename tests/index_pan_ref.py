"""Reference for the frames of a block rectangle THAT MOVES over a seek index (jsp_index_pan_frames / SeekIndex.PanFrames) — a helper
module, plain Python, no tests of its own.  Built on index_crop_ref (src, key, gap) and index_tight_ref.Pixels, whose block(t, i) is
P(t)[i] — the last writer's pixels, else the block of the picture before the range (also for t = -1), else None: not DEFINED.

THE RULE (PAN) is stated in jsplayer_amd/csrc/msv1_index_pan_kernels.hip.  A pair is (a, b, A, B): the rectangle of size = (bw, bh)
blocks stands at origin A = (bx, by) in the picture of frame a and at B in that of frame b.
  * KEY pair, a == KEY: index_crop_ref.key of rectangle B at b (A is None);
  * STILL pair, A == B: index_crop_ref.gap of that rectangle;
  * MOVED pair, A != B, -1 <= a <= b: without tight the KEY pair (B, b).  With tight block j is DROPPED when P(a)[srcA(j)] and
    P(b)[srcB(j)] are both defined and equal, else KEPT: the whole code of the last writer <= b of srcB(j); ("none", j) without one,
    ("cut", j) with a cut one — the FIRST such j.  Run heads and counts are Tight's in j.

  * kind, kept, pan — the kind of a pair, the kept blocks j of a moved tight pair, the bytes or the refusal;
  * writer — the frame a ("cut", j) refusal names;
  * `wrong` states one of four deliberately wrong variants (WRONG), each of which test_index_pan_ref_cpu.py shows to fail on a named
    clip."""
import index_crop_ref as cr
import index_delta_ref as dr

KEY = cr.KEY
RUN = dr.RUN
WRONG = ("movement_ignored",      # the compare takes srcB at `from` against srcB at `to`
         "gated_by_written",      # a block of srcB that no frame of the gap writes is skipped, whatever the pictures show
         "code_from_src_a",       # a kept block's code is that of the last writer of srcA(j)
         "dropped_refuses")       # a dropped block with a cut code, or without a writer, refuses


def rect_of(size, origin):
    return (origin[0], origin[1], size[0], size[1])


def kind(pair):
    a, b, A, B = pair
    return "key" if a == KEY else "still" if tuple(A) == tuple(B) else "moved"


def kept(px, nbx, size, pair, wrong=None):
    """The blocks j of a MOVED pair that the tight rule keeps, ascending."""
    a, b, A, B = pair
    nb = size[0] * size[1]
    out = []
    for j in range(nb):
        sa, sb = cr.src(nbx, rect_of(size, A), j), cr.src(nbx, rect_of(size, B), j)
        if wrong == "gated_by_written" and dr.writer(px.codes, a, b, sb) is None:
            continue
        pa = px.block(a, sb if wrong == "movement_ignored" else sa)
        pb = px.block(b, sb)
        if pa is None or pb is None or pa != pb:
            out.append(j)
    return out


def pan(bits, nbx, frames, size, pair, codes, tight=False, px=None, wrong=None):
    """codes: codes_of of every frame of the SOURCE index; px: index_tight_ref.Pixels of the source (tight only)."""
    assert wrong in (None,) + WRONG
    a, b, A, B = pair
    k = kind(pair)
    rect = rect_of(size, B)
    if k == "key" or (k == "moved" and not tight):
        assert 0 <= b < len(frames) and (k == "key" or -1 <= a <= b)
        return cr.key(bits, nbx, frames, rect, b, codes)
    if k == "still":
        return cr.gap(bits, nbx, frames, rect, a, b, codes, tight, px)
    assert -1 <= a <= b < len(frames) and b >= 0
    nb = size[0] * size[1]
    ks = set(kept(px, nbx, size, pair, wrong))
    out = bytearray()
    for j in range(nb):
        sb = cr.src(nbx, rect, j)
        take = cr.src(nbx, rect_of(size, A), j) if wrong == "code_from_src_a" else sb
        f = dr.writer(codes, -1, b, take)
        if j in ks or wrong == "dropped_refuses":
            if f is None:
                return ("none", j)
            if codes[f][take] == "cut":
                return ("cut", j)
        if j in ks:
            o, length = codes[f][take]
            out += bytes(frames[f])[o:o + length]
            continue
        if not (j == 0 or j - 1 in ks or j % RUN == 0):
            continue
        nxt = next((i for i in range(j + 1, nb) if i in ks), nb)
        out += dr.skip_word(min(nxt, (j // RUN + 1) * RUN, nb) - j)
    return bytes(out)


def writer(codes, nbx, size, pair, j):
    """The frame a ("cut", j) refusal of `pair` names: the last writer of srcB(j) up to the pair's frame."""
    return dr.writer(codes, -1, pair[1], cr.src(nbx, rect_of(size, pair[3]), j))


flag = cr.flag
