"""Directed clips for the lane arithmetic of the five range kernels of jsplayer_amd/csrc/msv1_seek_kernels.hip (msv1_seek_kernel,
msv1_change_scan_kernel, msv1_coded_bitmap_kernel, msv1_index_show_kernel, msv1_index_play_kernel) — a helper module, numpy only, no
tests of its own.

All five map work to lanes the same way: lane gid of the launch is 4x4 block gid in raster order (256 to a workgroup, 64 to a wave),
and the lanes past the last block are the pixels no block covers — first the strip [0, cy) x [cx, X), then the rows [cy, Y).  The
coded-bitmap kernel also folds the lanes of a block row into one word per row (a segmented OR inside the wave, one atomic per row
and wave) and finds the first untouched block of a frame (an atomic minimum per wave); the host turns both into the per-row
block_changes an adopted frame hands to the next DecompressP.  `sweep` is one short clip that says, frame by frame, which row flag
must be set and which must not; SIZES are the smallest pictures at which each piece of that arithmetic can go wrong without the
others:

  4x4, 8x4   1x1, 2x1 blocks    one block; one row of two
  68x16      17x4, 68 blocks    rows start at lanes 17, 34, 51 of one wave; the 64 seam cuts row 3, whose tail 64..67 is alone in wave 1
  70x18      the same           + 172 pixels no block covers (a strip 2x16, then 70x2) in workgroup 0 behind the blocks; X % 4 != 0
  260x24     65x6, 390 blocks   block 64, the last of row 0, is lane 0 of wave 1; the 256 seam lies inside row 3 (195..259); every wave
                                seam cuts a row at another column
  262x26     the same           + 572 uncovered pixels: they begin at lane 134 of workgroup 1 and fill workgroups 2 and 3 (no block at
                                all); the strip turns into rows at r = 48
  1028x8     257x2, 514 blocks  a row longer than a workgroup: five waves feed one row word; row 0 ends on lane 0 of workgroup 1
  1030x10    the same           + 2076 uncovered pixels, 11 workgroups; each of the two bottom rows (1030 pixels) is longer than four
                                workgroups
  20x248     5x62, 310 blocks   the most rows the test counter shows (62); 13 row segments in a wave; seams inside rows 12, 25, 38, 51
  22x250     the same           + 540 uncovered pixels, 496 of them a strip two pixels wide and 248 rows tall

The frames of sweep(bits, w, h), built on msv1_range_clips.Idle:
  0          a key frame of solid blocks
  MARK       one frame per marked block b, changing exactly block b.  Marked: the first and the last block of every block row, both
             sides of every 64-lane seam (s - 1 and s for s = 64, 128, ...: the 256 seams among them), block 0 and the last block
  STOP       two frames per marked block m > 0, taken as a cut: every block changes (every row flag is 1), then a frame that codes
             exactly one block c before the cut and ends at m — an 8-bit end marker on block m; a 16-bit stream that ends there
             (the reference paints the blocks from m on).  c = m - 1, or when m starts a row, m - nbx - 1 floored at 0: the last block
             of the row before the row before, so that the row before m is walked and codes nothing
Where nby > 12 only some rows are marked (marked_rows): row 0, the last row, every row that holds a 64-lane seam and the rows next
to it.  At 5x62 that is 34 marks and 33 cuts, 101 frames (all 62 rows would make 389)."""
import numpy as np

from msv1_range_clips import POISON, Idle, truth_run

SIZES = [(4, 4), (8, 4), (68, 16), (70, 18), (260, 24), (262, 26), (1028, 8), (1030, 10), (20, 248), (22, 250)]
WAVE, WG = 64, 256       # lanes of a wave, of a workgroup (the kernels' constants)
ROWS_SHOWN = 62          # block rows the test counter msv1_block_changes (and the oracle's BlockChanges) shows
MAX_FRAMES = 101


def marked_rows(nbx, nby):
    """The block rows whose ends are marked: all of them up to 12 rows, else row 0, the last row, the rows that hold a 64-lane seam
    and the rows next to those."""
    if nby <= 12:
        return list(range(nby))
    rows = {0, nby - 1}
    for s in range(WAVE, nbx * nby, WAVE):
        for b in (s - 1, s):
            rows |= {r for r in (b // nbx - 1, b // nbx, b // nbx + 1) if 0 <= r < nby}
    return sorted(rows)


def marked_blocks(nbx, nby):
    """The marked blocks, ascending, each once."""
    nb = nbx * nby
    out = {0, nb - 1}
    for r in marked_rows(nbx, nby):
        out |= {r * nbx, r * nbx + nbx - 1}
    for s in range(WAVE, nb, WAVE):
        out |= {s - 1, s}
    return sorted(out)


def coded_before(m, nbx):
    """The one block a STOP frame with its cut at block m codes."""
    return max(m - nbx - 1, 0) if m % nbx == 0 else m - 1


def sweep(bits, w, h, seed=7):
    """(frames, keys, marks, stops): the frames above, keys (frame 0 only), marks — (frame, block) per MARK frame —, stops —
    (frame, m, c) per STOP frame (the frame before it changes every block)."""
    g = Idle(bits, w, h, seed)
    every = list(range(g.nb))
    frames, marks, stops = [g.key()], [], []
    blocks = marked_blocks(g.nbx, g.nby)
    for b in blocks:
        marks.append((len(frames), b))
        frames.append(g.change([b]))
    for m in blocks:
        if m == 0:
            continue
        frames.append(g.change(every))
        c = coded_before(m, g.nbx)
        src = g.encode(g.change_codes([c])[:m])
        if bits == 8:
            src += b"\x00\x00"
        else:
            for b in range(m, g.nb):
                g.col[b] = 0
        stops.append((len(frames), m, c))
        frames.append(src)
    assert len(frames) <= MAX_FRAMES
    return frames, [True] + [False] * (len(frames) - 1), marks, stops


def with_idle_frame(bits, w, h, frames, keys, at):
    """The clip with one all-skip frame put in front of frame `at`: a range that starts there begins with a frame that codes
    nothing, so no frame of it has adopted a destination yet."""
    idle = Idle(bits, w, h, 0).all_skip("full")
    return frames[:at] + [idle] + frames[at:], keys[:at] + [False] + keys[at:]


# ---- painted pictures ----------------------------------------------------------------------------------------------------------
def uncovered(w, h):
    """Bool per pixel (flat): no 4x4 block covers it."""
    m = np.ones((h, w), dtype=bool)
    m[:(h // 4) * 4, :(w // 4) * 4] = False
    return m.reshape(-1)


def paint(w, h, k):
    """A buffer as the tests hand it to a codec for the first time: buffer number k (0..63) and the pixel's own index on the pixels
    no block covers — positive, never the poison, another word on every such pixel of every buffer —, the poison elsewhere."""
    assert 0 <= k < 64 and w * h < 1 << 24
    out = np.full(w * h, POISON, dtype=np.int32)
    at = np.flatnonzero(uncovered(w, h))
    out[at] = (0x40000000 | (k << 24) | at).astype(np.int32)
    return out


def painted_truth(bits, w, h, pal, frames, keys, lines):
    """truth_run (rows=True) with the oracle's three buffers painted: a decode writes no uncovered pixel, so every picture carries
    the paint of the buffer frame 0 went into."""
    return truth_run(bits, w, h, pal, frames, keys, lines, key_row=lines, rows=True, start_as=lambda k: paint(w, h, k))


def unpainted(picture, w, h):
    """The picture with the poison on the pixels no block covers: what a range with no picture before it leaves in a poisoned
    destination."""
    out = picture.copy()
    out[uncovered(w, h)] = np.int32(POISON)
    return out


def first_difference(got, want, w, h):
    """Where two whole buffers first differ, for a failure message ("" when they are equal)."""
    bad = np.flatnonzero(np.asarray(got) != np.asarray(want))
    if not len(bad):
        return ""
    i = int(bad[0])
    y, x = divmod(i, w)
    nbx = w // 4
    where = f"block {(y // 4) * nbx + x // 4} covers it" if not uncovered(w, h)[i] else "no block covers it"
    return (f"{len(bad)} pixels differ, the first is pixel {i} (x={x}, y={y}; {where}): "
            f"0x{int(got[i]) & 0xFFFFFFFF:08X}, wanted 0x{int(want[i]) & 0xFFFFFFFF:08X}")


# ---- what the clip promises ----------------------------------------------------------------------------------------------------
def check_census(truth, marks, stops, nbx, nby, bits):
    """What the sweep promises about block_changes (row r in bit r), asserted on the oracle's truth_run(..., rows=True) alone —
    before any answer of the code under test is looked at.  Every mark and every stop, no exemption."""
    assert nby <= ROWS_SHOWN
    full = (1 << nby) - 1
    assert all(x is not None for x in truth)
    for f, b in marks:
        assert truth[f][2] == 1 << (b // nbx), f"MARK frame {f} (block {b}): block_changes {truth[f][2]:#x}"
    for f, m, c in stops:
        assert truth[f - 1][2] == full, f"frame {f - 1} changes every block: block_changes {truth[f - 1][2]:#x}"
        rm, rc, got = m // nbx, c // nbx, truth[f][2]
        if bits == 16:   # the blocks from m on are painted: their rows are set; the rows walked before them hold c's flag alone
            want = (full >> rm << rm) | 1 << rc
        else:            # the rows past the marker's keep their 1, the marker's row and the rows before it are walked
            want = (full >> (rm + 1) << (rm + 1)) | 1 << rc
            assert (m % nbx == 0) == (rc != rm) and (got >> rm & 1) == (0 if m % nbx == 0 else 1), f"STOP frame {f}: row of block {m}"
            assert all(not (got >> r & 1) for r in range(rm) if r != rc), f"STOP frame {f}: a walked row that codes nothing keeps its flag"
        assert got == want, f"STOP frame {f} (cut at block {m}, block {c} coded): block_changes {got:#x}, by the rule {want:#x}"
