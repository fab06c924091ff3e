"""The directed key pictures of tests/sp_key_pictures.py, without a GPU: that they are what was painted once encoded (truth), that they
hold every table feature the two key-frame kernels compute with (census), and that a kernel with one of the named mistakes would
get a pixel of them wrong (discrimination).  tests/test_sp_key_pictures_gpu.py runs the kernels on them."""
import numpy as np
import pytest

import hoststage_binding as hb
import sp_key_pictures as kp
from oracle_binding import OracleScreenPressor

BANDS = (0, 1, 2, 3, 4, 5, 24)
NAMES = tuple(kp.PICTURES)


# ---- truth ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("version", [2, 3, 4])
@pytest.mark.parametrize("name", NAMES)
def test_the_encoded_picture_is_the_painted_one(name, version):
    """The oracle's DecompressI of the chunk, and the host stage's tables expanded by the row model and by the tile model (span 256),
    at every band height: all give the painted picture, bit for bit."""
    pic = kp.picture(name)
    h, w = pic.shape
    assert pic.dtype == np.uint32 and int(pic.max()) <= 0xFFFFFF
    src = kp.chunk(name, version)
    orc = OracleScreenPressor(w, h, 24)
    orc.Preinit(36)
    out = np.full(w * h, 0x00A5A5A5, dtype=np.int32)
    assert orc.DecompressI(src, out) == 0
    assert np.array_equal(out.view(np.uint32).reshape(h, w), pic), "the oracle's picture"
    for rows in BANDS + kp.bands_of(name):
        d = kp.host_tables(pic, rows, version, 0, src)
        assert np.array_equal(hb.expand_iframe(d, w, h).reshape(h, w), pic), f"expand_iframe, bands of {rows}"
        t = kp.host_tables(pic, rows, version, kp.SPAN, src)
        assert np.array_equal(hb.expand_iframe_tiles(t, w, h).reshape(h, w), pic), f"expand_iframe_tiles, bands of {rows}"


def test_the_run_table_does_not_depend_on_the_stream_version():
    """The entropy coder changes with the version, the runs do not: one census serves all three."""
    for name in ("B260", "W512", "B259"):
        pic = kp.picture(name)
        a = kp.host_tables(pic, kp.band_rows_of(name), 4, kp.SPAN)
        for version in (2, 3):
            b = kp.host_tables(pic, kp.band_rows_of(name), version, kp.SPAN)
            for key in ("runs", "tile_idx", "left", "seeds"):
                assert np.array_equal(a[key], b[key]), (name, version, key)


# ---- census ---------------------------------------------------------------------------------------------------------------------
# condition: the picture that provides it (under the band height the GPU tests run it with; "name/rows": under that one of its heights)
TILE_PROVIDERS = {
    # above-left records (counted only where the pixel above-left differs from the pixel above and neither is 0)
    "al_span_start": "D260",             # at column 0 of a span other than the first
    "al_x0_wrap": "D260",                # at x = 0, y >= 2, the wrap pixel (X - 1, y - 2) not 0
    "al_col_mult4": "B256",              # at a column that is a multiple of 4, not a span's first
    "al_col_mod1": "B256",
    "al_col_mod2": "B256",
    "al_col_mod3": "B256",
    "al_ends_last_column": "D256",
    "al_band_first_row": "B516",         # in the first / second row of a band other than the first
    "al_band_second_row": "B516",
    # tile rows
    "row_two_of_each": "B260",           # at least two records of each kind
    "row_only_const": "W512",
    "row_only_above": "B260",
    "row_only_left": "D516",
    "row_left_no_const": "Q516",
    # byte arithmetic
    "grad_wrap_byte0": "Y256",           # start byte + addend byte >= 256 (a carry that leaked would change the byte above it)
    "grad_wrap_byte1": "Y256",
    "const_edge_bytes": "Y256",          # constants with 0x00, 0x7F, 0x80 and 0xFF in every byte position
    # records in a tile row
    "rec_63": "W512", "rec_64": "W512", "rec_65": "W512", "rec_128": "W512", "rec_129": "W512", "rec_256": "W512",
    "rec_cap": "T256",                   # the window's capacity (226 in one band of 200 rows) and one more
    "rec_cap_plus_1": "T256",
    "rec_64_first_of_window": "W512", "rec_64_later_in_window": "W512",
    "rec_65_first_of_window": "W512", "rec_65_later_in_window": "W512",
    # windows
    "win_rows_1": "W512", "win_rows_2": "W512", "win_rows_16": "W512", "win_rows_17": "W512", "win_rows_18": "W512",
    "win_rows_61": "W512", "win_rows_62": "W512",
    "direct_before_quiet": "T256", "direct_after_quiet": "T256",
    "win_offset_odd": "W512", "win_offset_even": "W512",
    "win_holds_129_256": "W512", "win_holds_257_384": "W512", "win_holds_385_510": "W512",
    "win_exactly_full": "W512",
    "win_overfilled_by_one": "W512",
    "last_band_short": "D260",
    # kRowRepeats
    "rep_band_second_row": "D260",
    "rep_band_last_row": "D516",
    "rep_window_first_row": "Q516",
    "rep_stretch_62": "Q516",
    # the same windows cut by the band instead of by the capacity
    "win_rows_61/bands": "Q516/61", "win_rows_18/bands": "Q516/61", "win_rows_17/bands": "Q516/17",
}
# the row kernel sees the row-major table: the above-left conditions and the byte arithmetic, at its own widths
ROW_PROVIDERS = {
    "al_span_start": "D257", "al_x0_wrap": "D261", "al_col_mult4": "B259", "al_col_mod1": "B259", "al_col_mod2": "B259",
    "al_col_mod3": "B261", "al_ends_last_column": "D259", "al_band_first_row": "B2053", "al_band_second_row": "B2053",
    "grad_wrap_byte0": "B2053", "grad_wrap_byte1": "B257",
}


def _provided(condition, where):
    name, _, rows = where.partition("/")
    c = kp.census_of(name, 4, int(rows) if rows else None)
    return condition.partition("/")[0] in kp.conditions(c), sorted(kp.conditions(c))


@pytest.mark.parametrize("condition", sorted(TILE_PROVIDERS))
def test_a_picture_provides_the_condition_to_the_tile_kernel(condition):
    where = TILE_PROVIDERS[condition]
    assert where.partition("/")[0] in kp.ALIGNED
    ok, has = _provided(condition, where)
    assert ok, f"{where} does not provide {condition}; it provides {has}"


@pytest.mark.parametrize("condition", sorted(ROW_PROVIDERS))
def test_a_picture_provides_the_condition_to_the_row_kernel(condition):
    where = ROW_PROVIDERS[condition]
    assert where in kp.ODD
    ok, has = _provided(condition, where)
    assert ok, f"{where} does not provide {condition}; it provides {has}"


def test_the_wide_picture_has_an_above_left_run_across_the_row_kernels_second_trip():
    """2053 columns: a lane's second trip of the column loop begins at x = 2048; above-left runs cover 2047 and 2048 (the table cuts
    them there: a row-major record never crosses a multiple of 256 columns), in rows of every band (bands of 2)."""
    c = kp.census_of("B2053")
    across = (c.kind_rows[:, 2047] == kp.K_LEFT) & (c.kind_rows[:, 2048] == kp.K_LEFT)
    assert across[1:].all()
    assert set(np.unique(c.kind_rows[:, 2048:])) == {kp.K_CONST, kp.K_ABOVE, kp.K_LEFT}


def test_the_capacity_is_the_launchs():
    """hb.tile_window is sp.h's tile_window, which launch_iframe_tiles passes to the kernel: the figures the ledgers were laid out for."""
    assert hb.tile_window(128)[0] == 442 and hb.tile_window(200)[0] == 226 and hb.tile_window(24)[0] == 510
    assert hb.tile_window(4096)[0] == 128                       # never less: a row with more is scattered from memory
    for rows in (1, 24, 62, 128, 200, 1080, 4096):
        cap, words = hb.tile_window(rows)
        assert cap % 2 == 0 and 128 <= cap <= 510 and words % 4 == 0
        assert words >= 256 + (rows + 1) + 2 * rows + cap + 2 + 64   # head row, index, left pairs, window and its pad, the overrun


def test_the_window_plan_restated():
    assert hb.plan_windows([0, 10, 10, 10], 128) == [(0, 3, False)]
    assert hb.plan_windows([0, 129, 130], 128) == [(0, 1, True), (1, 1, False)]
    assert hb.plan_windows([0, 100, 128, 129], 128) == [(0, 2, False), (2, 1, False)]
    assert hb.plan_windows(list(range(0, 141)), 510) == [(0, 62, False), (62, 62, False), (124, 16, False)]


# ---- discrimination -------------------------------------------------------------------------------------------------------------
# fault: a picture that notices it
ROW_NOTICES = {"above_left_as_above": "D259", "left0_zero": "D261", "seed_word0_zero": "B2053", "seed_last_zero": "B259", "byte_carry": "B257"}
TILE_NOTICES = {"above_left_as_above": "D256", "left0_zero": "D260", "byte_carry": "Y256", "const_plus1_dropped": "Y256",
                "const_count_off_by_one": "B260", "repeat_ignored": "Q516", "past_64_dropped": "W512"}


def test_every_fault_has_a_picture():
    assert set(ROW_NOTICES) == set(hb.ROW_FAULTS) and set(TILE_NOTICES) == set(hb.TILE_FAULTS)


@pytest.mark.parametrize("fault", hb.ROW_FAULTS)
def test_the_row_model_with_a_fault_gets_a_pixel_wrong(fault):
    name = ROW_NOTICES[fault]
    pic = kp.picture(name)
    h, w = pic.shape
    d = kp.host_tables(pic, kp.band_rows_of(name), 4, 0, kp.chunk(name))
    assert np.array_equal(hb.expand_iframe(d, w, h), pic.reshape(-1))
    assert not np.array_equal(hb.expand_iframe(d, w, h, fault), pic.reshape(-1)), f"{name} does not notice {fault}"


@pytest.mark.parametrize("fault", hb.TILE_FAULTS)
def test_the_tile_model_with_a_fault_gets_a_pixel_wrong(fault):
    name = TILE_NOTICES[fault]
    pic = kp.picture(name)
    h, w = pic.shape
    t = kp.host_tables(pic, kp.band_rows_of(name), 4, kp.SPAN, kp.chunk(name))
    assert np.array_equal(hb.expand_iframe_tiles(t, w, h), pic.reshape(-1))
    assert not np.array_equal(hb.expand_iframe_tiles(t, w, h, fault), pic.reshape(-1)), f"{name} does not notice {fault}"


def test_the_carry_fault_is_noticed_by_gradients_alone():
    """In the tile model a carrying add breaks every constant (0xFFFFFF + colour + 1); the gradient rows must notice it on their own."""
    pic = kp.picture("Y256")
    h, w = pic.shape
    t = kp.host_tables(pic, 4, 4, kp.SPAN, kp.chunk("Y256"))
    bad = hb.expand_iframe_tiles(t, w, h, "byte_carry").reshape(h, w) != pic
    c = kp.census_of("Y256")
    assert (bad & (c.kind_tiles == kp.K_ABOVE)).any()


def test_a_mismatch_is_described():
    c = kp.census_of("B260")
    got = kp.picture("B260").copy()
    assert kp.describe_mismatch(got, c.pic, c, True) == ""
    got[7, 131] ^= 1
    text = kp.describe_mismatch(got, c.pic, c, True)
    assert "row 7 (row 2 of band 1 in the census's bands), column 131 (column 131 of span 0, lane 32, pixel 3 of the lane), inside constant run" in text, text
