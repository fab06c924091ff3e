"""Reference for the inter frame that spans a gap of a seek index (jsp_index_delta_frames / SeekIndex.DeltaFrames) — a helper module,
plain Python, no tests of its own.  Built on index_keyframe_ref.codes_of, whose WHOLE is the definition used here.

THE RULE.  Block i is WRITTEN in (a, b] when some frame f with a < f <= b codes it (a = -1: from before the range).
Delta(a, b), -1 <= a < b < nframes = for blocks i = 0 .. nblocks-1 in table order:
  * i is written: the L bytes of the whole code of its last writer <= b;
  * i is not written and is a RUN HEAD — i = 0, or block i - 1 is written, or i % 1023 = 0: one skip word, bytes (count & 0xFF,
    0x84 + (count >> 8)), count = the consecutive unwritten blocks from i on, stopping before the next written block, before the
    next multiple of 1023 above i, and at nblocks: 1 <= count <= 1023;
  * otherwise: nothing.
A written block whose last writer's code is not whole ("cut") makes the pair uncuttable.  A block without a writer is skipped.

  * delta — the bytes, or ("cut", block) with the FIRST block that refuses.  `wrong` states one of three deliberately wrong
    variants (WRONG), each of which test_index_delta_ref_cpu.py shows to fail on a directed clip;
  * writer — the frame a ("cut", block) refusal names: the block's last writer <= b;
  * walk — a frame's words as the decoder takes them, without its early-outs: (codes, skips, blocks covered)."""

RUN = 1023   # a skip word's count has 10 bits
WRONG = ("chunks_from_run_start",     # a long run is cut into 1023s counted from its own start, not at the multiples of 1023
         "count_past_nblocks",        # the count is clipped by the multiple of 1023 only, not by nblocks
         "no_head_after_written")     # a run head is block 0 or a multiple of 1023 only: the run behind a written block gets no word


def writer(codes, a, b, blk):
    """The last frame in (a, b] that codes `blk`, or None."""
    return next((f for f in range(b, a, -1) if codes[f][blk] is not None), None)


def skip_word(count):
    assert 1 <= count <= RUN
    return bytes([count & 0xFF, 0x84 + (count >> 8)])


def delta(bits, nbx, nby, frames, a, b, codes, wrong=None):
    """frames: the index's range; codes: index_keyframe_ref.codes_of of every frame of it."""
    assert -1 <= a < b < len(frames) and wrong in (None,) + WRONG
    nb = nbx * nby
    w = [writer(codes, a, b, blk) for blk in range(nb)]
    out = bytearray()
    run_start = None
    for i in range(nb):
        if w[i] is not None:
            if codes[w[i]][i] == "cut":
                return ("cut", i)
            o, length = codes[w[i]][i]
            out += bytes(frames[w[i]])[o:o + length]
            continue
        if i == 0 or w[i - 1] is not None:
            run_start = i
        if wrong == "chunks_from_run_start":
            head = (i - run_start) % RUN == 0
        elif wrong == "no_head_after_written":
            head = i == 0 or i % RUN == 0
        else:
            head = i == 0 or w[i - 1] is not None or i % RUN == 0
        if not head:
            continue
        nxt = next((k for k in range(i + 1, nb) if w[k] is not None), nb)
        if wrong == "chunks_from_run_start":
            count = min(nxt, i + RUN) - i
        elif wrong == "count_past_nblocks":
            count = min(nxt if nxt < nb else 1 << 30, (i // RUN + 1) * RUN) - i
        else:
            count = min(nxt, (i // RUN + 1) * RUN, nb) - i
        out += skip_word(count)
    return bytes(out)


def walk(bits, data):
    """The words of a frame in stream order: ([(block, offset, length)] of its codes, [(block, count)] of its skip words, the
    blocks they cover together) — no early-out, no end marker, lengths by the first bytes as index_keyframe_ref.codes_of has them."""
    data = bytes(data)
    codes, skips, blk, si = [], [], 0, 0
    while si + 1 < len(data):
        a, b = data[si], data[si + 1]
        if (b & 0xFC) == 0x84:
            skips.append((blk, ((b - 0x84) << 8) + a))
            blk += skips[-1][1]
            si += 2
            continue
        if bits == 16:
            length = 2 if b >= 0x80 else (18 if si + 3 < len(data) and data[si + 3] & 0x80 else 6)
        else:
            length = 4 if b < 0x80 else (10 if b >= 0x90 else 2)
        codes.append((blk, si, length))
        blk += 1
        si += length
    assert si == len(data), "a frame ends inside a code"
    return codes, skips, blk
