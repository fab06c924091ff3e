"""The numpy reference of jsp_index_tensor (tests/index_tensor_ref.py) against answers worked out by hand, codec.normalisation, and
Manager.tensor_from_index over a recording fake index — no GPU."""
import copy

import numpy as np
import pytest

import index_present_ref as ipr
import index_tensor_ref as itr
import view_ref as vr
from jsplayer_amd import player
from jsplayer_amd.avi import CODEC_MSVC16, CODEC_SCREENPRESSOR, VideoInfo
from jsplayer_amd.codec import normalisation

# a 2 x 2 picture, bottom-up, 0x00RRGGBB: the window at k = 1 is the picture with its rows flipped
#            bottom row                top row
PIC = np.array([0x00002A07, 0x00FFDB00, 0x0001DA10, 0x00030209], dtype=np.uint32).view(np.int32)
R = np.array([[0x01, 0x03], [0x00, 0xFF]])      # top window row first
G = np.array([[0xDA, 0x02], [0x2A, 0xDB]])      # 218, 2 / 42, 219
B = np.array([[0x10, 0x09], [0x07, 0x00]])


def tensor(dtype, layout=itr.NCHW, scale=None, bias=None, filter=ipr.NEAREST):
    return itr.tensor([PIC], 2, 2, 2, 2, 1.0, 0.0, 0.0, vr.CANVAS, filter, 0xFF000000, dtype, layout, scale, bias)


def test_u8_nchw_is_the_bytes_of_the_window():
    got = tensor(itr.U8)
    assert got.dtype == np.uint8 and got.shape == (1, 3, 2, 2)
    assert np.array_equal(got[0], np.stack([R, G, B]))
    win = ipr.window(PIC, 2, 2, 2, 2, 1.0, 0.0, 0.0, vr.CANVAS, ipr.NEAREST)
    for ch in range(3):
        assert np.array_equal(got[0, ch], (win >> (8 * ch)) & 0xFF)
    for f in ipr.FILTERS:                                       # a plain crop: the three filters agree
        assert np.array_equal(tensor(itr.U8, filter=f), got)


def test_the_two_layouts_are_permutations_of_each_other():
    pics = [PIC, PIC[::-1].copy()]
    for dtype in itr.DTYPES:
        args = ([1.0 / 255] * 3, [0.25, 0.5, -1.0])
        a = itr.tensor(pics, 2, 2, 3, 2, 0.7, 0.2, -0.1, vr.CANVAS, ipr.BILINEAR, 0xFF102030, dtype, itr.NCHW, *args)
        b = itr.tensor(pics, 2, 2, 3, 2, 0.7, 0.2, -0.1, vr.CANVAS, ipr.BILINEAR, 0xFF102030, dtype, itr.NHWC, *args)
        assert a.shape == (2, 3, 2, 3) and b.shape == (2, 2, 3, 3) and a.dtype == b.dtype == itr.RAW[dtype]
        assert np.array_equal(a.transpose(0, 2, 3, 1), b) and b.flags["C_CONTIGUOUS"]
        assert not np.array_equal(a[0], a[1])


def test_f32_by_hand():
    got = tensor(itr.F32, scale=[0.5, 2.0, 1.0], bias=[1.0, -4.0, 0.25]).view(np.float32)
    assert np.array_equal(got[0, 0], R * 0.5 + 1.0) and np.array_equal(got[0, 1], G * 2.0 - 4.0) and np.array_equal(got[0, 2], B + 0.25)
    # one rounding to double, one to float: 255 * float32(1 / 255) is not 1 but the float next below it
    s = np.float32(1.0 / 255)
    got = tensor(itr.F32, scale=[s] * 3, bias=[0.0] * 3)
    assert got[0, 0, 1, 1] == 0x3F800000 and got[0, 0, 0, 0] == np.float32(s).view(np.uint32)      # (float32(1 / 255) is just above 1 / 255)
    assert got[0, 1, 1, 1] == np.float32(219.0 * float(s)).view(np.uint32)


def test_ties_round_to_even_overflow_goes_to_infinity_and_zero_stays_positive():
    # bfloat16 has 8 significant bits: at 256 .. 511 the spacing is 2 and every odd v + 256 is a tie
    got = tensor(itr.BF16, scale=[1.0] * 3, bias=[256.0] * 3)
    assert got.dtype == np.uint16
    assert got[0, 0, 0, 0] == 0x4380                            # 257 -> 256 (even) and not 258
    assert got[0, 0, 0, 1] == 0x4382                            # 259 -> 260 (even) and not 258
    assert got[0, 0, 1, 0] == 0x4380 and got[0, 0, 1, 1] == 0x4400      # 256; 511 -> 512
    assert got[0, 1, 0, 1] == 0x4381                            # 258 is exact
    # binary16 has 11: at 2048 .. 4095 the spacing is 2
    got = tensor(itr.F16, scale=[1.0] * 3, bias=[2048.0] * 3)
    assert [int(got[0, 0, y, x]) for y in (0, 1) for x in (0, 1)] == [0x6800, 0x6802, 0x6800, 0x6880]   # 2049, 2051, 2048, 2303 -> 2304
    # 219 * 300 = 65700 lies above 65520, the first value that rounds to infinity; 218 * 300 = 65400 rounds to 65408
    got = tensor(itr.F16, scale=[300.0] * 3, bias=[0.0] * 3)
    assert got[0, 1, 0, 0] == 0x7BFC and got[0, 1, 1, 1] == 0x7C00 and got[0, 0, 1, 1] == 0x7C00 and got[0, 0, 1, 0] == 0
    # 0 * 1 + -0.0 is +0.0 under round-to-nearest
    for dtype in (itr.F32, itr.F16, itr.BF16):
        assert tensor(dtype, scale=[1.0] * 3, bias=[-0.0] * 3)[0, 0, 1, 0] == 0
    assert tensor(itr.F32, scale=[-1.0] * 3, bias=[0.0] * 3)[0, 0, 1, 0] == 0                # -0.0 + 0.0 likewise
    assert tensor(itr.F32, scale=[-1.0] * 3, bias=[-0.0] * 3)[0, 0, 1, 0] == 0x80000000      # ... and -0.0 only where both are
    assert tensor(itr.BF16, scale=[-1.0] * 3, bias=[-0.0] * 3)[0, 0, 1, 0] == 0x8000


def test_bf16_bits_and_as_values():
    f = np.array([1.0, 1.00390625, 1.01171875, -2.5, np.inf, 3.0e38], dtype=np.float32)     # 1 + 2^-8: a tie, down; 1 + 3 * 2^-8: a tie, up
    assert [int(v) for v in itr.bf16_bits(f)] == [0x3F80, 0x3F80, 0x3F82, 0xC020, 0x7F80, 0x7F62]
    assert np.array_equal(itr.as_values(itr.bf16_bits(f[:4]), itr.BF16), np.array([1.0, 1.0, 1.015625, -2.5], dtype=np.float32))
    assert itr.table(itr.U8).tolist() == [list(range(256))] * 3


def test_normalisation():
    mean, std = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
    scale, bias = normalisation(mean, std)
    for ch in range(3):
        assert scale[ch] == float(np.float32(1.0 / (255.0 * std[ch]))) and bias[ch] == float(np.float32(-mean[ch] / std[ch]))
        assert np.float32(scale[ch]) == scale[ch] and np.float32(bias[ch]) == bias[ch]         # already float32 values
    assert normalisation((0, 0, 0), (1, 1, 1)) == ((float(np.float32(1 / 255)),) * 3, (-0.0,) * 3)
    with pytest.raises(ValueError):
        normalisation((0.5,), (0.5,))


# ---- Manager.tensor_from_index over a recording fake index --------------------------------------------------------------------------
class FakeDecoder:
    SEEKS = True

    def __init__(self):
        self.calls, self.prev = [], None

    def Preinit(self, lines):
        pass

    def PreviousFrame(self):
        return self.prev

    def IsKeyFrame(self, f):
        return f[0] == 1


class FakeIndex:
    """Tensor logs its arguments and answers with an array that names the frames."""

    def __init__(self, count):
        self.frames = count
        self.significance = [True] * count
        self.tensors = []

    def Tensor(self, frames, win_w, win_h, k, dx, dy, **kw):
        self.tensors.append((list(frames), win_w, win_h, k, dx, dy, kw))
        return np.array(frames)


class FakeIndexWithoutTensor:
    def __init__(self, count):
        self.frames = count
        self.significance = [True] * count


def manager(codec=CODEC_MSVC16, bpp=16, x=640, y=480):
    vi = VideoInfo(X=x, Y=y, bpp=bpp, fps=15.0, nframes=40, codec=codec, palette=None, riff_size=0)
    dec = FakeDecoder()
    return player.Manager(vi, dec, lambda n: np.full(n, -1, dtype=np.int32)), dec


def state(mgr, dec):
    return (copy.deepcopy(mgr.holds), mgr.frame_of_interest, mgr.next_frame_to_decode, list(mgr.log), dict(mgr.judged), list(dec.calls),
            [b.copy() for b in mgr.buffers])


def test_tensor_from_index_fits_renumbers_and_passes_its_arguments_on():
    from jsplayer_amd.codec import DISPLAY_CANVAS, DISPLAY_CANVAS_RGB15
    mgr, dec = manager()
    idx = FakeIndex(16)
    mgr.attach_index(idx, 8)                                    # clip frames 8 .. 23
    before = state(mgr, dec)
    got = mgr.tensor_from_index([23, 8, 15, 8], 224, 224, dtype="float16", layout="nhwc", scale=(1, 2, 3), bias=(4, 5, 6), filter=1,
                                background=0xFF123456, out="caller's")
    assert list(got) == [15, 0, 7, 0]
    (frames, ww, wh, k, dx, dy, kw), = idx.tensors              # ONE Tensor call
    assert frames == [15, 0, 7, 0] and (ww, wh) == (224, 224)
    assert (k, dx, dy) == vr.view_matrix(640, 480, 224, 224, 0.0, 0.5, 0.5)                   # Fit, as contact_sheet
    assert kw == dict(dtype="float16", layout="nhwc", scale=(1, 2, 3), bias=(4, 5, 6), filter=1, background=0xFF123456, out="caller's",
                      mode=DISPLAY_CANVAS)
    after = state(mgr, dec)                                     # a pure read
    assert before[:6] == after[:6] and all(np.array_equal(a, b) for a, b in zip(before[6], after[6]))
    # nothing but the fit and the mode is decided here: the index's defaults stay the index's
    mgr.tensor_from_index([9], 384, 216)
    assert idx.tensors[1][6] == dict(mode=DISPLAY_CANVAS) and idx.tensors[1][3:6] == vr.view_matrix(640, 480, 384, 216, 0.0, 0.5, 0.5)
    # 16-bpp ScreenPressor frames hold 5-bit components: the RGB15 conversion, as for Present
    mgr, dec = manager(CODEC_SCREENPRESSOR, 16)
    idx = FakeIndex(4)
    mgr.attach_index(idx, 0)
    mgr.tensor_from_index(range(4), 32, 24)
    assert idx.tensors[0][0] == [0, 1, 2, 3] and idx.tensors[0][6] == dict(mode=DISPLAY_CANVAS_RGB15)


def test_tensor_from_index_refuses_without_an_index_outside_it_and_without_tensor():
    mgr, dec = manager()
    with pytest.raises(ValueError, match="no seek index"):
        mgr.tensor_from_index([0], 8, 8)
    idx = FakeIndex(16)
    mgr.attach_index(idx, 8)
    for bad in ([7], [24], [8, 23, 24], [-1]):
        with pytest.raises(ValueError, match="not in an attached seek index"):
            mgr.tensor_from_index(bad, 8, 8)
    assert idx.tensors == []
    mgr.attach_index(FakeIndexWithoutTensor(16), 8)
    with pytest.raises(ValueError, match="no tensors"):
        mgr.tensor_from_index([8], 8, 8)
