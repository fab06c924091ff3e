"""The directed tile-boundary catalogue (tests/msv1_directed_streams.py) checked on the CPU.

  * every picture known by construction equals pyref_msv1.decode and OracleMSVideo1 (driven with the Manager's buffer
    protocol, as drive_pair of test_msvideo1_gpu.py does); for the malformed frames only the oracle speaks, and it must say
    the same twice;
  * every geometric claim — where a placed code starts, the tile it starts in, the slot at which the chain enters the next
    tile, the block span of every tile, the bytes consumed — is recomputed with a plain sequential walk over the bytes
    (the code-length rules of MSVideo1.hx:128-181 / 311-364, as in test_msv1_lanes_cpu.py);
  * every entry slot the format can produce occurs at a tile boundary for each tile size and bit depth (0..8 for 16-bit;
    0..4 for 8-bit, whose longest code is five slots: no well-formed chain enters a tile at slot 5..8);
  * which frames the on-GPU parse hands to the host parser is what frame_parse's three conditions (and the 16-bit early-out
    pre-check) say about the walk."""
from collections import Counter

import numpy as np
import pytest

import msv1_directed_streams as D
import pyref_msv1
from oracle_binding import OracleAbort, OracleMSVideo1

REST = 0xFFFFF


def walk(bits, data, nb):
    """The sequential walk: [(byte offset, slots, blocks covered, kind)] of every code on the chain, and how it ended:
    "covered" (every block has its code), "marker" (8-bit end marker) or "short" (the data ran out first)."""
    n = len(data) & ~1
    pos, blk, out = 0, 0, []
    while blk < nb:
        if pos >= n:
            return out, "short"
        a, b = data[pos], data[pos + 1]
        if (b & 0xFC) == 0x84:
            cnt = ((b - 0x84) << 8) + a
            out.append((pos, 1, cnt if cnt else REST, "skip"))
        elif bits == 16:
            if b < 0x80:
                eight = pos + 3 < len(data) and (data[pos + 3] & 0x80)
                out.append((pos, 9 if eight else 3, 1, "eight" if eight else "two"))
            else:
                out.append((pos, 1, 1, "solid"))
        elif a == 0 and b == 0:
            out.append((pos, 1, 0, "end"))
            return out, "marker"
        elif b < 0x80:
            out.append((pos, 2, 1, "two"))
        elif b >= 0x90:
            out.append((pos, 5, 1, "eight"))
        else:
            out.append((pos, 1, 1, "solid"))
        pos += 2 * out[-1][1]
        blk += out[-1][2]
    return out, "covered"


def walked_spans(chain, tile, nb):
    """[first block, end block) of the codes starting in each tile, and the slot at which the chain enters each tile."""
    ntiles = chain[-1][0] // tile + 1 if chain else 0
    spans, entries, blk, k = [], [], 0, 0
    for t in range(ntiles):
        first = min(blk, nb)
        entry = None
        while k < len(chain) and chain[k][0] < (t + 1) * tile:
            if entry is None:
                entry = (chain[k][0] - t * tile) // 2
            blk += chain[k][2]
            k += 1
        spans.append((first, min(blk, nb)))
        entries.append(entry)
    return spans, entries


def oracle_clip(case, lines=36, nbuf=3):
    """The clip through the oracle with the Manager's buffer protocol -> per frame (all buffers, significance, index of the
    buffer data_pnt is or None, raised)."""
    pal = D.palette(case.bits)
    orc = OracleMSVideo1(case.bits, case.w, case.h, pal)
    orc.Preinit(lines)
    bufs = [np.full(case.w * case.h, D.PREFILL, dtype=np.int32) for _ in range(nbuf)]
    out = []
    for src, key in case.frames:
        prev = orc.PreviousFrame()
        dst = next(b for b in bufs if b is not prev)
        sig, raised = None, False
        if key:
            assert orc.DecompressI(src, dst) == 0
        else:
            try:
                _, sig = orc.DecompressP(src, dst)
            except OracleAbort:
                raised = True
        now = orc.PreviousFrame()
        out.append(([b.copy() for b in bufs], sig, next((k for k in range(nbuf) if bufs[k] is now), None), raised,
                    next(k for k in range(nbuf) if bufs[k] is dst)))
    return out


@pytest.fixture(scope="module", params=[16, 8])
def cases(request):
    return D.catalogue(request.param)


def test_the_assembler_refuses_items_that_would_read_as_another_code():
    bad16 = [("solid", 0x0400), ("solid", 0x07FF), ("solid", 0x8000), ("two", 0x8000, 1, 2), ("two", 0x1234, 0x8001, 2),
             ("eight", 0x1234, (1,) * 8), ("eight", 0x9234, (0x8001,) * 8), ("skip", 1024), ("end",)]
    for item in bad16:
        with pytest.raises(D.Refused):
            D.assemble(16, 8, 8, [item])
    bad8 = [("two", 0, 1, 2), ("two", 0x8000, 1, 2), ("eight", 0x8FFF, (1,) * 8), ("eight", 0x9000, (1,) * 7), ("solid", 256), ("skip", -1)]
    for item in bad8:
        with pytest.raises(D.Refused):
            D.assemble(8, 8, 8, [item], palette=D.palette(8))
    with pytest.raises(D.Refused):                               # raw bytes only at the end; nothing but raw behind the last block
        D.assemble(16, 8, 4, [("raw", b"\x00\x80"), ("solid", 1)])
    with pytest.raises(D.Refused):
        D.assemble(16, 8, 4, [("solid", 1), ("solid", 2), ("solid", 3)])
    # 8-bit solid codes never get a skip code's high byte, whatever the index
    for c in range(256):
        assert not 0x84 <= D.encode_item(8, ("solid", c))[1] <= 0x87
    a = D.assemble(16, 8, 4, [("solid", 0x7FFF), ("two", 0x0001, 0x001F, 0x7C00), ("raw", b"\xAA")])
    assert a.consumed == 8 and len(a.data) == 9 and not a.short
    pic = a.picture.reshape(4, 8)
    assert (pic[:, :4] == 0xF8F8F8).all() and pic[0, 4] == 0x0000F8 and (pic[1:, 4:] == 0xF80000).all()


def test_pictures_by_construction_match_pyref_and_the_oracle(cases):
    n_valid = n_oracle_only = 0
    for case in cases:
        pal = D.palette(case.bits)
        pal_ints = pyref_msv1.palette_ints(pal) if pal else None
        first, second = oracle_clip(case), oracle_clip(case)
        prev_py = None
        for i, (src, key) in enumerate(case.frames):
            where = f"{case.bits}-bit {case.name} frame {i}"
            bufs, sig, now, raised, dst = first[i]
            bufs2, sig2, now2, raised2, dst2 = second[i]
            assert (sig, now, raised, dst) == (sig2, now2, raised2, dst2), where + ": the oracle disagrees with itself"
            assert all(np.array_equal(x, y) for x, y in zip(bufs, bufs2)), where
            assert raised == (case.raises and i == case.directed), where
            want = case.pictures[i]
            if want is None:
                n_oracle_only += 1
                prev_py = None
                continue
            n_valid += 1
            assert np.array_equal(bufs[dst].view(np.uint32), want), where + ": oracle against the picture by construction"
            exp, coded, nskips = pyref_msv1.decode(case.bits, case.w, case.h, src, None if prev_py is None else prev_py.reshape(case.h, case.w), pal_ints,
                                                   dst=np.full(case.w * case.h, D.PREFILL, dtype=np.int64))
            assert np.array_equal((exp & 0xFFFFFFFF).astype(np.uint32).ravel(), want), where + ": pyref against the picture by construction"
            prev_py = want.astype(np.int64) if coded else prev_py
            if coded:
                assert now == dst, where + ": a frame that codes a block becomes the previous frame"
    assert n_valid >= 100 and n_oracle_only >= 6


def test_every_claimed_geometry_is_where_the_bytes_say(cases):
    n_claims = 0
    for case in cases:
        nb = (case.w // 4) * (case.h // 4)
        for i, (src, key) in enumerate(case.frames):
            where = f"{case.bits}-bit {case.name} frame {i}"
            chain, ending = walk(case.bits, src, nb)
            layout = case.layouts[i]
            # the assembler's layout IS the chain (up to where the data, the blocks or a marker end it)
            got = [(o, s, c if k != "skip" or c < REST else REST, k) for o, s, c, k in chain]
            want = [(o, s, n, k) for o, b, n, k, s in layout]
            if ending == "covered":
                assert len(got) == len(want) and [g[:2] + g[3:] for g in got] == [x[:2] + x[3:] for x in want], where
                assert all(g[2] == x[2] or (g[3] == "skip" and g[2] >= x[2]) for g, x in zip(got, want)), where   # (a skip run is clipped to the frame)
                assert case.consumed[i] == chain[-1][0] + 2 * chain[-1][1], where + ": consumed"
            elif ending == "marker":
                assert [g[0] for g in got] == [x[0] for x in want] and case.consumed[i] == chain[-1][0] + 2, where
            else:
                assert case.consumed[i] == -1, where
            if ending != "short":
                for tile in D.TILES:
                    spans, _ = walked_spans(chain, tile, nb)
                    assert D.tile_spans(layout, tile, nb) == spans, f"{where}: block spans of the {tile}-byte tiles"
                    assert spans[0][0] == 0 and all(a[1] == b[0] for a, b in zip(spans, spans[1:])), where
                    assert ending == "marker" or spans[-1][1] == nb, where
            # what frame_parse decides from the parse's counters
            have_prev = i > 0
            host = ending in ("short", "marker") or (not have_prev and any(c[3] == "skip" for c in chain))
            host |= case.bits == 16 and len(src) < (nb // 1023) * 2 + 10
            assert case.host[i] == host, where + ": host-settled or not"
        # placements of the directed frame
        src = case.frames[case.directed][0]
        chain, _ = walk(case.bits, src, nb)
        starts = {c[0]: c for c in chain}
        for cl in case.claims:
            n_claims += 1
            where = f"{case.bits}-bit {case.name}: {cl['kind']} {cl['back']} slots before byte {cl['boundary']}"
            assert cl["at"] == cl["boundary"] - 2 * cl["back"] and cl["at"] in starts, where
            assert starts[cl["at"]][1] == cl["slots"] and starts[cl["at"]][3] == cl["kind"], where
            if cl["at"] == chain[-1][0]:            # (a rest-of-frame skip: the chain ends with the placed code)
                continue
            nxt = min(o for o in starts if o >= cl["boundary"])
            assert nxt == cl["boundary"] + 2 * cl["entry"], where + ": where the chain goes on behind the boundary"
            for tile in D.TILES:
                if cl["boundary"] % tile == 0:
                    k = cl["boundary"] // tile
                    _, entries = walked_spans(chain, tile, nb)
                    assert cl["at"] // tile == (k - 1 if cl["back"] else k), where + ": the tile the code starts in"
                    assert entries[k] == cl["entry"], where + f": entry slot into tile {k} of {tile} bytes"
    assert n_claims > 100


def test_every_entry_slot_occurs_at_a_tile_boundary(cases):
    bits = cases[0].bits
    longest = D.KIND_SLOTS[bits]["eight"]
    for tile in D.TILES:
        for keys_only in (True, False):         # the key-frame cases feed the fused batch form, the others the table-writing form
            hist = Counter()
            for case in cases:
                if case.key_case != keys_only or case.any_host:
                    continue
                nb = (case.w // 4) * (case.h // 4)
                chain, _ = walk(bits, case.frames[case.directed][0], nb)
                _, entries = walked_spans(chain, tile, nb)
                hist.update(e for e in entries[1:] if e is not None)
            assert set(hist) == set(range(longest)), (bits, tile, keys_only, sorted(hist.items()))
            assert all(hist[e] >= 2 for e in range(longest)), (bits, tile, keys_only, sorted(hist.items()))


def test_the_catalogue_holds_what_it_must(cases):
    bits = cases[0].bits
    groups = Counter(c.group.split("+")[0] for c in cases)
    need = {"straddle", "end", "trailing", "skip", "saturate", "window", "batch", "raise"} | ({"halo"} if bits == 16 else {"marker"})
    assert need <= set(groups), groups
    slots = D.KIND_SLOTS[bits]
    for kind in ("two", "eight"):
        for back in range(slots[kind]):
            for variant in ("key", "inter"):
                c = next(x for x in cases if x.name == f"straddle_{kind}_back{back}_{variant}")
                assert sorted(cl["boundary"] for cl in c.claims) == sorted(D.STRADDLE_BOUNDARIES)
                assert all(cl["back"] == back and cl["slots"] == slots[kind] for cl in c.claims)
                assert D.tile_count(len(c.frames[-1][0])) >= 3          # the frame spans three 16 KiB tiles
    # only deliberately malformed frames are left to the host parser
    assert all(c.why_host for c in cases if c.any_host)
    # one tile's block span past msv1_parse_emit's 8192-block staging buffer, and a two-window tile whose last block lies in either window
    big = [c for c in cases if (c.w, c.h) == D.BIG]
    nb = (D.BIG[0] // 4) * (D.BIG[1] // 4)
    assert any(max(b - a for a, b in D.tile_spans(c.layouts[-1], D.BATCH_TILE, nb)) > 8192 for c in big)
    rest = sorted(nb - D.tile_spans(c.layouts[-1], D.BATCH_TILE, nb)[1][0] for c in big if c.name.startswith("window_last"))
    assert rest and rest[0] <= 4096 < rest[-1] <= 8192, rest
    # lane-group and wave boundaries are not tile boundaries, tile sizes are what the catalogue was laid out for
    assert D.SMALL_TILE == D.LANES * 16 * 2 and D.BATCH_TILE == D.LANES * 32 * 2
    # every wave boundary and the lane groups at 10, 19 and 28 for either lane width, and a group and a wave boundary in a later tile
    for tile in D.TILES:
        lane = tile // D.LANES
        inside = {b % tile // lane for b in D.STRADDLE_BOUNDARIES if b % lane == 0}
        assert {10, 19, 28, 64, 128, 192} <= inside, (tile, sorted(inside))
        later = {b % tile // lane for b in D.STRADDLE_BOUNDARIES if b > tile and b % lane == 0}
        assert later & {10, 19, 28, 37, 46, 55} and later & {64, 128, 192}, (tile, sorted(later))
