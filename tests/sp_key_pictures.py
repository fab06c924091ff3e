"""Directed key pictures for the two ScreenPressor key-frame kernels, sp_iframe_tile_kernel and sp_iframe_rows_search_kernel (a
helper module, no tests of its own): pictures PAINTED so that the run table the kernels compute with is fixed by construction, and
a census that says what a picture's tables hold.

The encoder (gen/sp_encoder.cpp) is deterministic: after the first X + 1 pixels, which are literals, it takes at every pixel the
longest run among "above", "repeat", "above-left" and "gradient" (ties in that order), at most 255 pixels, and a literal where none
matches.  Runs follow the LINEAR pixel index, so "above-left" of column 0 is pixel (X - 1, y - 2).

Most pictures are GROWN row by row: every column has a mode for a row, and the row is made from the row above by that mode, so the
encoder finds exactly that predictor there —
    A   the pixel above                                     -> an "above" run, addend 0
    L   the pixel above-left (linear index i - X - 1)       -> an "above-left" run
    G   the pixel above plus GRAD_ADD in every byte         -> a literal, then a "gradient" run: "above" with the addend GRAD_ADD
and single pixels are then overwritten with FRESH colours nothing predicts: each is a literal of its own, one constant record.
A run ends where the mode changes, so segments shorter than 255 pixels keep the 255-pixel cap from cutting runs at columns that
wander from row to row.  A QUIET row is one grown with the modes of the row above and no fresh pixel: it has as many records as the
row above.  A row with k fresh pixels at the start of a 256-column span has k constant records and then what is left of the quiet
layout.

What cannot be painted: a full 256-column span whose rows REPEAT (kRowRepeats: the records of the row above, column for column).  A
run holds at most 255 pixels, so every row of a full span has a run that starts inside it, and where it starts moves from row to
row: under the cap the start drifts, and an L segment behind an A segment takes the A segment's last colour one column further
every row, so the "above" run in front of it grows by one.  The ledger pictures' quiet rows therefore hold two records each, the
second one a column further right every row.  Rows that repeat — 64 and more in a row — are found in the last span of a picture 516
wide, which is one lane: a run starts inside those 4 columns once in about 86 rows (Q516).  A `direct` row, which needs more than
128 records, is for the same reason never next to a repeating row in its own tile; it is next to quiet ones (T256).

    name    size      bands  what it is
    D256    256x16    3      pure diagonal c[(x - y) mod 7]; 7 does not divide 257: a literal at the start of every row
    B256    256x16    5      diagonal broken by "above" columns, gradient blocks, fresh pixels at lane edges, 255 and X - 1
    Y256    256x16    4      byte arithmetic: gradient rows whose bytes wrap, constants of 0x00 / 0x7F / 0x80 / 0xFF bytes
    D260    260x12    5      pure diagonal, P = 9 divides 261: above-left runs straight through column 0; a last band of 2 rows
    B260    260x12    5      broken diagonal; the second span is one lane
    D516    516x16    4      pure diagonal, P = 11 divides 517
    B516    516x16    3      broken diagonal, fresh pixels at 255, 256 and X - 1
    W512    512x128   0      the window ledger (one band, capacity 442): span 0 windows of 62 (the lane limit), 61 and 5 rows,
                             span 1 windows of 1, 2, 16, 17 and 18 rows, two filled exactly, one that the next row overfills by one,
                             rows of 63, 64, 65, 128, 129 and 256 records, 64 and 65 both first in a window and later in one
    R512    512x128   24     W512's span 1 beside its span 0, in bands of 24 rows (capacity 510) — and another layout for the batch
    T256    256x200   0      one band of 200 rows (capacity 226): rows of 226, 227 and 256 records: the `direct` scatter between
                             windows of quiet rows.  (A span holds at most 256 records a row, and the capacity falls below 256
                             only from 191 rows a band on: no shorter picture has a `direct` row.)
    Q516    516x140   0, 61, 17   grown by L alone: span 2 (one lane) repeats for 28, 77 and 29 rows, cut by fresh pixels in rows 30 and
                             109: windows of 62 rows that begin on a repeating row; of 61 and 18 rows in bands of 61, of 17 in bands of 17
    D257, B257 (257x12), D259, B259 (259x12), D261, B261 (261x12), B2053 (2053x6)
                             the row kernel's widths: X % 4 = 1, 2, 3, and the second trip of its column loop
"""
from __future__ import annotations

from functools import lru_cache
from typing import Dict, List, Tuple

import numpy as np

import hoststage_binding as hb
from jsplayer_amd import streamgen as sg

SPAN = 256
GRAD_ADD = 0x90F0A5            # added byte by byte: every byte wraps within two rows
EDGE_BYTES = (0x00, 0x7F, 0x80, 0xFF)


def add_bytes(u, d):
    return hb._add_bytes(np.asarray(u, dtype=np.uint32), np.uint32(d))


def fresh_colours(seed: int, n: int) -> np.ndarray:
    """n distinct 24-bit colours, every byte in 1..254 (none a zeroed register's, none a saturated one)."""
    rng = np.random.default_rng(seed)
    out = np.zeros(0, dtype=np.uint32)
    while len(out) < n:
        b = rng.integers(1, 255, size=(2 * n + 16, 3)).astype(np.uint32)
        out = np.unique(np.concatenate([out, b[:, 0] | (b[:, 1] << 8) | (b[:, 2] << 16)]))
    return rng.permutation(out)[:n].astype(np.uint32)


def diagonal(w: int, h: int, p: int, seed: int) -> np.ndarray:
    c = fresh_colours(seed, p)
    y, x = np.mgrid[0:h, 0:w]
    return c[(x - y) % p]


def grow(w: int, h: int, modes, fresh, seed: int) -> np.ndarray:
    """modes(y) -> a string of w letters A / L / G (the module's docstring); fresh: {y: columns (or {column: colour})}."""
    pool = iter(fresh_colours(seed, w + 1 + sum(len(v) for v in fresh.values()) + h))
    pic = np.zeros((h, w), dtype=np.uint32)
    pic[0] = [next(pool) for _ in range(w)]
    for y in range(1, h):
        m = np.frombuffer(modes(y).encode(), dtype=np.uint8)
        assert len(m) == w
        up = pic[y - 1]
        left = np.empty(w, dtype=np.uint32)
        left[1:] = up[:-1]
        left[0] = pic[y - 2, w - 1] if y >= 2 else next(pool)
        pic[y] = np.where(m == ord("A"), up, np.where(m == ord("L"), left, add_bytes(up, GRAD_ADD)))
        cols = fresh.get(y, ())
        for x in cols:
            pic[y, x] = cols[x] if isinstance(cols, dict) else next(pool)
    assert int(pic.max()) <= 0xFFFFFF
    return pic


def segments(w: int, *cuts) -> str:
    """segments(w, "L", 10, "A", 14, "L"): L in columns 0..9, A in 10..13, L from 14 on."""
    out, at = "", 0
    for k in range(0, len(cuts), 2):
        end = cuts[k + 1] if k + 1 < len(cuts) else w
        out += cuts[k] * (min(end, w) - at)
        at = min(end, w)
    assert len(out) == w
    return out


def broken(w: int, h: int, seed: int) -> np.ndarray:
    """A diagonal broken by columns that copy the row above (4..5, 60..66, the three in front of the last), by a gradient block (columns
    24..43 from row 3 on; 2010..2029 as well in a wide picture, whose above-left runs cross x = 2048, the row kernel's second trip), and by fresh pixels at lane edges, at 255, 256
    and X - 1 and in front of and behind the A columns."""
    base = segments(w, "L", 4, "A", 6, "L", 24, "L", 44, "L", 60, "A", 67, "L", w - 4, "A", w - 1, "L")
    grad = segments(w, "L", 4, "A", 6, "L", 24, "G", 44, "L", 60, "A", 67, "L", w - 4, "A", w - 1, "L")
    if w > 2100:
        grad = grad[:2010] + "G" * 20 + grad[2030:]
    fresh = {2: [8, 11], 4: [w - 1], 5: [255, 12, 15], 6: [0, 100], 7: [7, 59, 67, 131, 136], 9: [w - 1, 3]}
    if w > 256:
        fresh[4] = [w - 1, 256]
        fresh[8] = [256, 255]
    fresh = {y: [x for x in xs if x < w] for y, xs in fresh.items() if y < h}
    return grow(w, h, lambda y: grad if y >= 3 else base, fresh, seed)


def byte_arithmetic(w: int, h: int, seed: int) -> np.ndarray:
    """Rows 1..: whole rows grown by G (every byte of every pixel gains GRAD_ADD's: each wraps within two rows), columns 200.. by A;
    rows 6 and 11 begin with the 64 colours whose bytes are all of 0x00, 0x7F, 0x80 and 0xFF."""
    edge = [a | (b << 8) | (c << 16) for a in EDGE_BYTES for b in EDGE_BYTES for c in EDGE_BYTES]
    rng = np.random.default_rng(seed)
    fresh = {6: {x: int(v) for x, v in enumerate(rng.permutation(edge))}, 11: {100 + x: int(v) for x, v in enumerate(rng.permutation(edge))}}
    return grow(w, h, lambda y: segments(w, "G", 200, "A"), fresh, seed)


QUIET = "A" * 128 + "L" * 128      # a span of the ledger pictures: two records a row, [above at 0, above-left at 128]


def fresh_for(records: int) -> int:
    """Fresh pixels at the start of a QUIET span that make a row of `records` records there."""
    return records - 2 if records <= 129 else (records - 1 if records < 256 else 256)


def ledger(h: int, *plans: Dict[int, int], seed: int) -> np.ndarray:
    """One QUIET span per plan, side by side; plan: {row: records that row holds in the span}.  Row 0 is all literals: 256 records."""
    w = SPAN * len(plans)
    fresh: Dict[int, List[int]] = {}
    for s, plan in enumerate(plans):
        for y, n in plan.items():
            assert 0 < y < h
            fresh.setdefault(y, []).extend(range(s * SPAN, s * SPAN + fresh_for(n)))
    return grow(w, h, lambda y: QUIET * len(plans), fresh, seed)


H = 256
# span 0: full rows at 0, 62 and 123, quiet rows between: windows of 62 (the lane limit), 61 and 5 rows
LEDGER_STRETCH = {62: H, 123: H}
# span 1 (capacity 442): windows of 1, 2, 16, 17, 18 rows between full rows; [54, 55] = 256 + 186 fills a window exactly; [56, 57] = 441 and
# row 58 brings 2; [58, 59] holds 192; [60..62] = 256 + 64 + 65 = 385; 67 (64 records) and 70 (65) begin windows; 63, 128, 129 at 73..75
LEDGER_WINDOWS = {1: H, 3: H, 19: H, 36: H, 54: H, 55: 186, 56: H, 57: 185, 59: 190, 60: H, 61: 64, 62: 65, 63: H, 64: H, 65: H, 66: 186,
                  67: 64, 68: H, 69: 122, 70: 65, 71: H, 72: H, 73: 63, 74: 128, 75: 129, 76: H}
# one band of 200 rows (capacity 226): full rows at 0, 40 and 150 are `direct`, 226 fits exactly, 227 does not
LEDGER_TALL = {40: H, 100: 226, 110: 227, 150: H}

# name: (painter, band_rows of its census and of the GPU tests)
PICTURES = {
    "D256": (lambda: diagonal(256, 16, 7, 11), 3),
    "B256": (lambda: broken(256, 16, 12), 5),
    "Y256": (lambda: byte_arithmetic(256, 16, 13), 4),
    "D260": (lambda: diagonal(260, 12, 9, 14), 5),
    "B260": (lambda: broken(260, 12, 15), 5),
    "D516": (lambda: diagonal(516, 16, 11, 16), 4),
    "B516": (lambda: broken(516, 16, 17), 3),
    "W512": (lambda: ledger(128, LEDGER_STRETCH, LEDGER_WINDOWS, seed=18), 0),
    "R512": (lambda: ledger(128, LEDGER_WINDOWS, LEDGER_STRETCH, seed=19), 24),
    "T256": (lambda: ledger(200, LEDGER_TALL, seed=20), 0),
    "Q516": (lambda: grow(516, 140, lambda y: "L" * 516, {30: [513], 109: [514, 515]}, 28), 0),
    "D257": (lambda: diagonal(257, 12, 6, 21), 5),       # 6 divides 258
    "B257": (lambda: broken(257, 12, 22), 5),
    "D259": (lambda: diagonal(259, 12, 7, 23), 4),       # 7 does not divide 260
    "B259": (lambda: broken(259, 12, 24), 3),
    "D261": (lambda: diagonal(261, 12, 131, 25), 5),     # 131 divides 262
    "B261": (lambda: broken(261, 12, 26), 4),
    "B2053": (lambda: broken(2053, 6, 27), 2),
}
ALIGNED = tuple(n for n in PICTURES if int(n[1:]) % 4 == 0)
ODD = tuple(n for n in PICTURES if int(n[1:]) % 4 != 0)


@lru_cache(maxsize=None)
def picture(name: str) -> np.ndarray:
    """(h, w) uint32, painted once a process; nobody changes it."""
    pic = np.ascontiguousarray(PICTURES[name][0](), dtype=np.uint32)
    pic.setflags(write=False)
    return pic


# further band heights at which a picture's census is taken and the GPU tests run it
MORE_BANDS = {"Q516": (61, 17)}


def band_rows_of(name: str) -> int:
    return PICTURES[name][1]


def bands_of(name: str) -> Tuple[int, ...]:
    return (PICTURES[name][1],) + MORE_BANDS.get(name, ())


@lru_cache(maxsize=None)
def chunk(name: str, version: int = 4) -> bytes:
    return encode(picture(name), version)


def encode(pic: np.ndarray, version: int = 4) -> bytes:
    h, w = pic.shape
    enc = sg.SpEncoder(w, h, 24, version)
    out = enc.encode_i(np.ascontiguousarray(pic))
    enc.close()
    return out


def host_tables(pic: np.ndarray, band_rows: int, version: int = 4, span: int = 0, src: bytes = None):
    """The host stage's tables for the picture: row-major (span 0) or tile layout."""
    h, w = pic.shape
    hs = hb.HostStage(w, h, 24)
    if span:
        hs.set_iframe_layout(band_rows, span)
    else:
        hs.set_band_rows(band_rows)
    d = hs.decode(True, src if src is not None else encode(pic, version))
    hs.close()
    assert d["status"] == 0 and d["kind"] == hb.KIND_INTRA, d["error"]
    return d


plan_windows = hb.plan_windows      # the restatement of plan_and_fetch, beside the tile model that also uses it


K_CONST, K_ABOVE, K_LEFT = 0, 1, 2          # the census's kinds, for both layouts
KIND_NAMES = ("constant", "above", "above-left")


class Census:
    """What the host stage's tables of a picture hold.  `runs`: the records of the row-major layout, `recs` those of the tile layout
    (X % 4 == 0 only) — rows of (y, x, end column, kind, value); kind_rows / kind_tiles: the kind of the record that covers each pixel;
    tile_rows: per (band, span, row of the band) (records, constants, above, above-left, repeats, first record's offset);
    windows: per (band, span) the plan_windows list."""


@lru_cache(maxsize=None)
def census_of(name: str, version: int = 4, band_rows: int = None) -> Census:
    return census(picture(name), band_rows_of(name) if band_rows is None else band_rows, version)


def census(pic: np.ndarray, band_rows: int, version: int = 4) -> Census:
    h, w = pic.shape
    c = Census()
    c.pic, c.w, c.h, c.band_rows = pic, w, h, band_rows
    c.rows_per = band_rows if 0 < band_rows < h else h
    c.nbands = -(-h // c.rows_per)
    src = encode(pic, version)
    d = host_tables(pic, band_rows, version, 0, src)
    assert np.array_equal(hb.expand_iframe(d, w, h).reshape(h, w), pic), "the row-major tables do not give the picture"
    starts, words = d["runs"][:, 0].astype(np.int64), d["runs"][:, 1]
    live = starts < w * h
    ends = np.append(starts[1:], w * h)[live]
    starts, words = starts[live], words[live]
    kinds = np.select([words >> 24 == hb.RUN_CONST, words >> 24 == hb.RUN_ABOVE], [K_CONST, K_ABOVE], K_LEFT)
    assert np.all(starts // w == (ends - 1) // w), "a row-major record crosses a row"
    c.runs = np.stack([starts // w, starts % w, (ends - 1) % w + 1, kinds, words & 0xFFFFFF], axis=1)
    c.kind_rows = np.repeat(kinds, ends - starts).reshape(h, w)
    c.recs = c.kind_tiles = None
    c.tile_rows, c.windows, c.cap = {}, {}, None
    if w % 4 == 0:
        t = host_tables(pic, band_rows, version, SPAN, src)
        assert np.array_equal(hb.expand_iframe_tiles(t, w, h).reshape(h, w), pic), "the tile tables do not give the picture"
        c.cap, _ = hb.tile_window(c.rows_per, SPAN)            # the product's figure for this band height
        idx, left, rec32 = t["tile_idx"], t["left"].reshape(-1, 2), t["runs"].reshape(-1)
        nspans = -(-w // SPAN)
        c.kind_tiles = np.full((h, w), -1, dtype=np.int64)
        recs = []
        for b in range(c.nbands):
            rows = min(c.rows_per, h - b * c.rows_per)
            for s in range(nspans):
                tl = b * nspans + s
                e = idx[tl * (c.rows_per + 1):(tl + 1) * (c.rows_per + 1)].astype(np.int64)
                off = e & 0x7FFFFFFF
                width = min(SPAN, w - s * SPAN)
                for r in range(rows):
                    y = b * c.rows_per + r
                    n = int(off[r + 1] - off[r])
                    rep = bool(e[r] >> 31)
                    if rep:
                        c.kind_tiles[y, s * SPAN:s * SPAN + width] = c.kind_tiles[y - 1, s * SPAN:s * SPAN + width]
                        c.tile_rows[(b, s, r)] = (0, 0, 0, 0, True, int(off[r]))
                        continue
                    counts = int(left[tl * c.rows_per + r, 1])
                    nc, na = counts & 0xFFFF, counts >> 16
                    c.tile_rows[(b, s, r)] = (n, nc, na, n - nc - na, False, int(off[r]))
                    rr = rec32[off[r]:off[r + 1]]
                    kk = np.concatenate([np.full(nc, K_CONST), np.full(na, K_ABOVE), np.full(n - nc - na, K_LEFT)])
                    order = np.argsort(rr >> 24, kind="stable")
                    cols = (rr >> 24).astype(np.int64)[order]
                    colend = np.append(cols[1:], width)
                    for x, xe, k, v in zip(cols, colend, kk[order], (rr & 0xFFFFFF)[order]):
                        if k == K_CONST:                       # the record carries the colour plus one in every byte
                            v = int(add_bytes(np.uint32(v), 0xFFFFFF))
                        recs.append((y, s * SPAN + x, s * SPAN + xe, k, int(v)))
                        c.kind_tiles[y, s * SPAN + x:s * SPAN + xe] = k
                c.windows[(b, s)] = plan_windows([int(v) for v in off[:rows + 1]], c.cap)
        c.recs = np.array(recs, dtype=np.int64)
        assert c.kind_tiles.min() >= 0
    return c


def conditions(c: Census) -> set:
    """The names of the conditions (tests/test_sp_key_pictures_cpu.py lists them) that the picture provides under its band height."""
    pic, w, h, rp = c.pic, c.w, c.h, c.rows_per
    flat = pic.reshape(-1)
    out = set()
    table = c.recs if c.recs is not None else c.runs
    for y, x, xe, k, v in table:
        if k == K_LEFT:
            i = y * w + x
            al, ab = int(flat[i - w - 1]), int(pic[y - 1, x])
            if al == ab or al == 0 or ab == 0:     # a record that a wrong start value would not show is not counted
                continue
            if x % SPAN == 0 and x > 0:
                out.add("al_span_start")
            if x == 0 and y >= 2 and pic[y - 2, w - 1] != 0:
                out.add("al_x0_wrap")
            if x % 4 == 0 and x % SPAN != 0:
                out.add("al_col_mult4")
            if x % 4:
                out.add("al_col_mod%d" % (x % 4))
            if xe == w:
                out.add("al_ends_last_column")
            if y >= rp and y % rp == 0:
                out.add("al_band_first_row")
            if y > rp and y % rp == 1:
                out.add("al_band_second_row")
        elif k == K_ABOVE and v:
            up = pic[y - 1, x:xe].astype(np.int64)
            if np.any((up & 0xFF) + (v & 0xFF) >= 256):            # a leaked carry would change byte 1, always
                out.add("grad_wrap_byte0")
            if np.any(((up >> 8) & 0xFF) + ((v >> 8) & 0xFF) >= 256):
                out.add("grad_wrap_byte1")
    consts = table[table[:, 3] == K_CONST][:, 4]
    if all(np.any(((consts >> s) & 0xFF) == b) for s in (0, 8, 16) for b in EDGE_BYTES):
        out.add("const_edge_bytes")
    if c.recs is None:
        return out
    if h % rp:
        out.add("last_band_short")
    for (b, s, r), (n, nc, na, nl, rep, off) in c.tile_rows.items():
        rows = min(rp, h - b * rp)
        if rep:
            if r == 1 and b > 0:
                out.add("rep_band_second_row")
            if r == rows - 1:
                out.add("rep_band_last_row")
            continue
        if min(nc, na, nl) >= 2:
            out.add("row_two_of_each")
        for k, (m, name) in enumerate(((nc, "const"), (na, "above"), (nl, "left"))):
            if m == n:
                out.add("row_only_" + name)
        if nc == 0 and nl > 0:
            out.add("row_left_no_const")
        if n in (63, 64, 65, 128, 129, 256):
            out.add("rec_%d" % n)
        if n == c.cap:
            out.add("rec_cap")
        if n == c.cap + 1:
            out.add("rec_cap_plus_1")
    for (b, s), wins in c.windows.items():
        rows = min(rp, h - b * rp)
        tr = [c.tile_rows[(b, s, r)] for r in range(rows)]
        end = tr[-1][5] + tr[-1][0]
        quiet = []
        run = 0
        for r in range(rows):
            run = run + 1 if tr[r][4] else 0
            if run >= 62:
                out.add("rep_stretch_62")
        for f, n, direct in wins:
            w0 = tr[f][5]
            held = (tr[f + n][5] if f + n < rows else end) - w0
            quiet.append(not direct and n >= 4 and all(t[0] <= 2 for t in tr[f + 2:f + n]))
            if not direct and n in (1, 2, 16, 17, 18, 61, 62):
                out.add("win_rows_%d" % n)
            out.add("win_offset_odd" if w0 & 1 else "win_offset_even")
            if not direct:
                for lo, hi in ((128, 256), (256, 384), (384, 510)):
                    if lo < held <= hi:
                        out.add("win_holds_%d_%d" % (lo + 1, hi))
                if held == c.cap:
                    out.add("win_exactly_full")
                if f + n < rows and held + tr[f + n][0] == c.cap + 1:
                    out.add("win_overfilled_by_one")
            if tr[f][4]:
                out.add("rep_window_first_row")
            for r in range(f, f + n):
                if tr[r][0] in (64, 65):
                    out.add("rec_%d_%s" % (tr[r][0], "first_of_window" if r == f else "later_in_window"))
        for k, (f, n, direct) in enumerate(wins):
            if direct and k + 1 < len(wins) and quiet[k + 1]:
                out.add("direct_before_quiet")
            if direct and k > 0 and quiet[k - 1]:
                out.add("direct_after_quiet")
    return out


def describe_mismatch(got, want, c: Census, tiles: bool) -> str:
    """'' when the pictures are equal, else the first wrong pixel: its row and column, its column inside the span, its lane (4 pixels a lane
    in both kernels; the row kernel's lanes take 2048 columns a trip) and the kind of the run that covers it."""
    got = np.asarray(got).reshape(-1).view(np.uint32)
    want = np.asarray(want).reshape(-1).view(np.uint32)
    bad = np.nonzero(got != want)[0]
    if len(bad) == 0:
        return ""
    y, x = divmod(int(bad[0]), c.w)
    kinds = c.kind_tiles if tiles and c.kind_tiles is not None else c.kind_rows
    lane = (x % SPAN) // 4 if tiles else (x % 2048) // 4
    return "%d pixels differ, first at row %d (row %d of band %d in the census's bands), column %d (column %d of span %d, lane %d, pixel %d of the lane), inside %s run: want 0x%08x, got 0x%08x" % (
        len(bad), y, y % c.rows_per, y // c.rows_per, x, x % SPAN, x // SPAN, lane, x % 4, KIND_NAMES[int(kinds[y, x])], int(want[bad[0]]), int(got[bad[0]]))
