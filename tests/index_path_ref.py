"""Reference for the frames of a block rectangle of a seek index along ANY path through it (jsp_index_path_frames /
SeekIndex.PathFrames) — a helper module, plain Python, no tests of its own.  Built on index_crop_ref (src, the virtual index, the key
pair), index_delta_ref (the writer of a window, the skip word, the 1023 rule) and index_tight_ref (Pixels: P(t)[i]).

THE RULE.  The rectangle, src(j) and the virtual index are index_crop_ref's.  A pair (a, b) is
  * KEY, a == KEY: index_crop_ref.key;
  * FORWARD, -1 <= a < b < nframes; HOLD, 0 <= a == b < nframes; BACK, 0 <= b < a < nframes — ONE statement for the three, with
    lo = min(a, b), hi = max(a, b):
      block j is TOUCHED when some frame f, lo < f <= hi, codes it;
      a touched block is KEPT — with tight it is DROPPED instead when P(a)[j] and P(b)[j] are both defined and equal in all 16 words;
      a kept block gives the whole code of its last writer <= b; ("none", j) when it has none, ("cut", j) when that code is cut off
      — the FIRST such block of the rectangle decides;
      every other block is skipped under Delta's rule: a run head is j = 0, block j - 1 kept, or j % 1023 = 0; a count stops
      before the next kept block, before the next multiple of 1023 and at nb.

  * kind, kept, step, path — the kind of a pair, the kept blocks with their writers, the bytes or the refusal;
  * writer — the frame a ("cut", j) refusal names;
  * `wrong` states one of four deliberately wrong variants (WRONG), each of which test_index_path_ref_cpu.py shows to fail on a
    named clip."""
import index_crop_ref as cr
import index_delta_ref as dr

KEY = cr.KEY
RUN = dr.RUN
WRONG = ("code_of_from",             # a BACK pair takes the last writer <= a: the picture stays where it is
         "window_at_to",             # touched is computed over [b, a) instead of (b, a]
         "skips_no_writer",          # a kept block without a writer <= b is skipped instead of refused
         "tight_needs_written_to")   # tight drops only blocks whose P(b) comes from a code


def kind(pair):
    a, b = pair
    return "key" if a == KEY else "forward" if a < b else "hold" if a == b else "back"


def kept(nbx, rect, pair, codes, tight=False, px=None, wrong=None):
    """[(j, last writer <= b or None)] of the blocks a pair that is not KEY keeps, ascending."""
    a, b = pair
    back = a > b
    lo, hi = min(a, b), max(a, b)
    vcodes = cr.remap(codes, nbx, rect)
    v = cr.Virtual(px, nbx, rect) if tight else None
    out = []
    for j in range(rect[2] * rect[3]):
        if back and wrong == "window_at_to":
            touched = dr.writer(vcodes, lo - 1, hi - 1, j) is not None
        else:
            touched = dr.writer(vcodes, lo, hi, j) is not None
        if not touched:
            continue
        w = dr.writer(vcodes, -1, a if back and wrong == "code_of_from" else b, j)
        if tight:
            pa, pb = v.block(a, j), v.block(b, j)
            same = pa is not None and pb is not None and pa == pb
            if same and not (wrong == "tight_needs_written_to" and w is None):
                continue
        out.append((j, w))
    return out


def step(bits, nbx, frames, rect, pair, codes, tight=False, px=None, wrong=None):
    """A FORWARD, HOLD or BACK pair: the bytes, ("none", j) or ("cut", j)."""
    a, b = pair
    assert a >= -1 and 0 <= b < len(frames) and a < len(frames)
    nb = rect[2] * rect[3]
    vcodes = cr.remap(codes, nbx, rect)
    w = dict(kept(nbx, rect, pair, codes, tight, px, wrong))
    if wrong == "skips_no_writer":
        w = {j: f for j, f in w.items() if f is not None}
    out = bytearray()
    for j in range(nb):
        if j in w:
            if w[j] is None:
                return ("none", j)
            if vcodes[w[j]][j] == "cut":
                return ("cut", j)
            o, length = vcodes[w[j]][j]
            out += bytes(frames[w[j]])[o:o + length]
            continue
        if not (j == 0 or j - 1 in w or j % RUN == 0):
            continue
        nxt = next((k for k in range(j + 1, nb) if k in w), nb)
        out += dr.skip_word(min(nxt, (j // RUN + 1) * RUN, nb) - j)
    return bytes(out)


def path(bits, nbx, frames, rect, pair, codes, tight=False, px=None, wrong=None):
    """codes: codes_of of every frame of the SOURCE index; px: index_tight_ref.Pixels of the source (tight only)."""
    assert wrong in (None,) + WRONG
    if pair[0] == KEY:
        return cr.key(bits, nbx, frames, rect, pair[1], codes)
    return step(bits, nbx, frames, rect, pair, codes, tight, px, wrong)


def writer(codes, nbx, rect, pair, j):
    """The frame a ("cut", j) refusal of `pair` names: the last writer of src(j) up to the pair's `to`."""
    return dr.writer(codes, -1, pair[1], cr.src(nbx, rect, j))


def hold(nb):
    """A HOLD pair's frame: ceil(nb / 1023) skip words."""
    return b"".join(dr.skip_word(min(RUN, nb - j)) for j in range(0, nb, RUN))
