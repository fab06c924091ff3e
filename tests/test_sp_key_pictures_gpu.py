"""The two ScreenPressor key-frame kernels, sp_iframe_tile_kernel and sp_iframe_rows_search_kernel, on the directed key pictures of
tests/sp_key_pictures.py, on an MI355X: above-left runs at every lane position, at span and band borders and through column 0,
gradient bytes that wrap, rows of 63 .. 256 records, windows of 1 .. 62 rows, filled exactly and overfilled by one, the `direct`
scatter, rows that repeat (tests/test_sp_key_pictures_cpu.py asserts that the pictures hold all of that, and that a kernel with one of
those things wrong would show it).

Truth: the painted picture; drive_pair holds the oracle beside it.  Everything is bit-exact.  A failure names the first wrong pixel:
row, band, column, span, lane and the kind of the run that covers it (sp_key_pictures.describe_mismatch)."""
import numpy as np
import pytest

import sp_key_pictures as kp
from jsplayer_amd import DecoderState, ScreenPressor
from jsplayer_amd import streamgen as sg
from test_screenpressor_gpu import dev_buf, drive_pair, to_np

pytestmark = pytest.mark.gpu

POISON = 0x5A5A5A5A
TILE, ROWS = "sp_iframe_tile_kernel", "sp_iframe_rows_search_kernel"


def bands_for(name):
    out = ["auto", 0, 1, 2, 3, 5]
    return out + [b for b in kp.bands_of(name) if b not in out]


def codec(w, h, band_rows):
    gpu = ScreenPressor(w, h, 24)
    gpu.Preinit(36)
    gpu.set_option("sp_band_rows", str(band_rows))
    return gpu


def exact(got, name, what, tiles):
    c = kp.census_of(name)
    text = kp.describe_mismatch(to_np(got), c.pic, c, tiles)
    assert not text, f"{name} {what}: {text}"


def one_call(name, band_rows, misalign):
    pic = kp.picture(name)
    h, w = pic.shape
    gpu = codec(w, h, band_rows)
    dst = dev_buf(w * h, POISON, misalign)
    assert dst.data_ptr() % 16 == (4 if misalign else 0)
    assert gpu.DecompressI(kp.chunk(name), dst) == DecoderState.zero_state
    gpu.sync()
    exact(dst, name, f"DecompressI, sp_band_rows {band_rows}{', buffer 4 bytes off' if misalign else ''}", not misalign and w % 4 == 0)
    gpu.StopAndClean()
    drive_pair(w, h, 24, [kp.chunk(name)], [True], [pic.reshape(-1)], band_rows=band_rows, misalign=misalign)


@pytest.mark.parametrize("name", kp.ALIGNED)
def test_tile_kernel_one_call_at_a_time(name):
    for band_rows in bands_for(name):
        one_call(name, band_rows, False)


def batches():
    by_size = {}
    for name in kp.PICTURES:
        by_size.setdefault(kp.picture(name).shape, []).append(name)
    return by_size


def staged(names, band_rows, misalign, kernel, other):
    """The pictures of one size as ONE batch of key frames: one launch, of `kernel`; decoded twice (a staged batch is replayable)."""
    h, w = kp.picture(names[0]).shape
    gpu = codec(w, h, band_rows)
    dsts = [dev_buf(w * h, POISON, misalign) for _ in names]
    extra = dev_buf(w * h, POISON, misalign)                         # never listed: must stay as it is
    assert all(d.data_ptr() % 16 == (4 if misalign else 0) for d in dsts)
    st = gpu.stage_batch([kp.chunk(n) for n in names], dsts)
    assert st.info()["kernel_launches"] == 1
    assert kernel in st.kernels() and other not in st.kernels(), st.kernels()
    for again in range(2):
        for d in dsts:
            d.fill_(POISON)
        st.decode()
        gpu.sync()
        status, adopted, _ = st.results()
        assert status == [0] * len(names) and adopted == [1] * len(names)
        for n, d in zip(names, dsts):
            exact(d, n, f"frame {names.index(n)} of the batch {names}, sp_band_rows {band_rows}, decode {again}", kernel == TILE)
    assert bool((extra == POISON).all()), "a buffer that was not listed was written"
    st.close()
    gpu.StopAndClean()


@pytest.mark.parametrize("size", [s for s in batches() if s[1] % 4 == 0], ids=lambda s: f"{s[1]}x{s[0]}")
def test_tile_kernel_one_batch(size):
    names = batches()[size]
    assert len(names) > 1 or names[0] in ("T256", "Q516")           # (the two tall pictures have their sizes to themselves)
    for band_rows in ["auto"] + sorted({b for n in names for b in kp.bands_of(n)}):
        staged(names, band_rows, False, TILE, ROWS)
        staged(names[::-1], band_rows, False, TILE, ROWS)            # every frame beside another neighbour


@pytest.mark.parametrize("size", [s for s in batches() if s[1] % 4], ids=lambda s: f"{s[1]}x{s[0]}")
def test_row_kernel_odd_widths(size):
    names = batches()[size]
    for name in names:
        for band_rows in bands_for(name):
            one_call(name, band_rows, False)
    for band_rows in ["auto"] + sorted({kp.band_rows_of(n) for n in names}):
        staged(names, band_rows, False, ROWS, TILE)


@pytest.mark.parametrize("size", [s for s in batches() if s[1] % 4 == 0], ids=lambda s: f"{s[1]}x{s[0]}")
def test_row_kernel_aligned_widths_in_buffers_4_bytes_off(size):
    names = batches()[size]
    for name in names:
        for band_rows in bands_for(name):
            one_call(name, band_rows, True)
    for band_rows in ["auto"] + sorted({kp.band_rows_of(n) for n in names}):
        staged(names, band_rows, True, ROWS, TILE)


def repainted(pic):
    """`pic` with the block at rows 0..11, columns 16..31 repainted: every pixel a colour the picture does not hold there."""
    out = pic.copy()
    out[0:12, 16:32] = (out[0:12, 16:32] ^ 0x00010101) & 0xFFFFFF
    return out


@pytest.mark.parametrize("name,misalign", [("B260", False), ("B259", False), ("B260", True)], ids=["tile", "rows_odd_width", "rows_buffer_4_bytes_off"])
def test_key_picture_then_an_inter_frame(name, misalign):
    """The inter frame is coded against the picture the host stage's shadow holds and laid over the one the kernel left: they agree."""
    pic = kp.picture(name)
    h, w = pic.shape
    enc = sg.SpEncoder(w, h, 24, 4)
    second = repainted(pic)
    chunks = [enc.encode_i(np.ascontiguousarray(pic)), enc.encode_p(second)]
    enc.close()
    for band_rows in ("auto", kp.band_rows_of(name)):
        drive_pair(w, h, 24, chunks, [True, False], [pic.reshape(-1), second.reshape(-1)], band_rows=band_rows, misalign=misalign)


@pytest.mark.parametrize("names,misalign", [(("D260", "B260"), False), (("D259", "B259"), False)], ids=["tile_layout", "row_major_layout"])
def test_seek_index_shows_the_key_pictures(names, misalign):
    """The seek index decodes its key frames with a band height of its own: frames 0 and 2 are directed pictures, 1 and 3 inter frames."""
    pics = [kp.picture(n) for n in names]
    h, w = pics[0].shape
    enc = sg.SpEncoder(w, h, 24, 4)
    chunks, keys, frames = [], [], []
    for pic in pics:
        chunks += [enc.encode_i(np.ascontiguousarray(pic)), enc.encode_p(repainted(pic))]
        keys += [True, False]
        frames += [pic.reshape(-1), repainted(pic).reshape(-1)]
    enc.close()
    gpu = ScreenPressor(w, h, 24)
    gpu.Preinit(5)
    idx = gpu.BuildScrubIndex(chunks, keys, key_row=5)
    assert idx.frames == 4
    dst = dev_buf(w * h, POISON)
    for t in (2, 0, 3, 1, 2):
        dst.fill_(POISON)
        r = idx.Show(t, dst)
        assert r.data_pnt is dst
        if keys[t]:
            exact(dst, names[t // 2], f"Show({t})", w % 4 == 0)
        assert np.array_equal(to_np(dst).view(np.uint32), frames[t]), f"Show({t})"
    idx.close()
    gpu.StopAndClean()
