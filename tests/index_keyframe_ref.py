"""Reference for the key frame of a seek index (jsp_index_key_frame / SeekIndex.KeyFrame) — a helper module, plain Python, no tests
of its own.

THE RULE.  Let e be the end of the writer's frame data (16-bit: rounded down to a whole word).  The code at offset o is WHOLE when
(1) its two-byte code word lies below e, (2) the bytes that settle its length lie below e — for a 16-bit code whose second byte is
below 0x80 that is the colour word at o + 2 — and (3) o + L <= e.  L follows MSVideo1.hx:135-181 (16-bit: 1-colour 2, 2-colour 6,
8-colour 18 bytes) and :319-364 (8-bit: 2, 4, 10).  KeyFrame(t) = for blocks 0 .. nblocks-1 in table order (which is stream order),
the L bytes of the whole code of the block's last writer <= t.  No skip codes, no end marker, nothing after the last block.  A block
with no writer <= t, or whose last writer's code is not whole, makes t uncuttable.

  * codes_of — one frame: per block (offset, length) of its whole code, "cut" for a code the frame's end cuts off, None for a block
    the frame does not code.  The control flow is msv1_range_clips.coded_blocks' (a block is coded exactly where that says so:
    test_index_keyframe_ref_cpu.py asserts it), with the offsets kept.
  * key_frame — the bytes, or ("none" | "cut", block) with the FIRST block that refuses;
  * cut_writer — the frame a ("cut", block) refusal names: the block's last writer <= t."""


def codes_of(bits, nbx, nby, src, have_prev=True):
    src = bytes(src)
    nb = nbx * nby
    out = [None] * nb
    n = len(src)
    e = n & ~1 if bits == 16 else n
    if bits == 16:   # the early-out: an empty frame, or a short one of skip codes only, does nothing
        sojs = (nb // 1023) * 2 + 10
        if n == 0:
            return out
        if n < sojs:
            total, just = 0, True
            for si in range(0, n, 2):
                if si + 1 < n and (src[si + 1] & 0xFC) == 0x84:
                    total += ((src[si + 1] - 0x84) << 8) + src[si]
                    if total >= nb:
                        break
                else:
                    just = False
                    break
            if just:
                return out
    si, skip = 0, 0
    for blk in range(nb):
        if skip != 0:
            skip -= 1
            if not have_prev:
                return out
            continue
        o = si
        a_ok, b_ok = si < n, si + 1 < n
        a, b = (src[si] if a_ok else 0), (src[si + 1] if b_ok else 0)
        if bits == 8 and b_ok and a == 0 and b == 0:
            return out                                      # the end marker: nothing from here on
        si += 2
        if b_ok and (b & 0xFC) == 0x84:
            skip = ((b - 0x84) << 8) + a - 1
            if not have_prev:
                return out
            continue
        # a coded block.  The parse goes on as the reference's does (missing bytes read as 0); the code is whole or cut by THE RULE
        length = 2
        settled = o + 2 <= e
        if bits == 16:
            if b_ok and b < 0x80:
                eight = si + 1 < n and bool(src[si + 1] & 0x80)
                si += 16 if eight else 4
                settled = settled and o + 4 <= e
                length = 18 if eight else 6
        elif b_ok and b < 0x80:
            si += 2
            length = 4
        elif b_ok and b >= 0x90:
            si += 8
            length = 10
        out[blk] = (o, length) if settled and o + length <= e else "cut"
    return out


def key_frame(bits, nbx, nby, frames, t, codes=None):
    """frames: the index's range; codes: codes_of of every frame, when the caller has them."""
    nb = nbx * nby
    if codes is None:
        codes = [codes_of(bits, nbx, nby, f) for f in frames[:t + 1]]
    out = bytearray()
    for blk in range(nb):
        f = next((f for f in range(t, -1, -1) if codes[f][blk] is not None), None)
        if f is None:
            return ("none", blk)
        if codes[f][blk] == "cut":
            return ("cut", blk)
        o, length = codes[f][blk]
        out += bytes(frames[f])[o:o + length]
    return bytes(out)


def cut_writer(codes, t, blk):
    """The frame whose code of `blk` is cut off when key_frame says ("cut", blk) at t: the last frame <= t that codes the block."""
    return next(f for f in range(t, -1, -1) if codes[f][blk] is not None)
