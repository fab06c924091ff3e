"""Host-side mirror of jsplayer's IVideoCodec plugin surface over the C ABI.

Same class names, method names, argument meaning and results as the reference
(IVideoCodec.hx:16-29; MSVideo1.hx:8,262; ScreenPressor.hx:19), so code written against the
Haxe interface reads the same here:

    dec = MSVideo1_16bit(320, 240)
    dec.Preinit(36)
    state = dec.DecompressI(frame_bytes, buf)          # DecoderState
    res = dec.DecompressP(frame_bytes, other_buf)      # PFrameResult(data_pnt, significant_changes)
    res.data_pnt is dec.PreviousFrame()                # identity, as Manager.hx:516 relies on

Frame buffers are caller-owned int32 arrays of at least width*height elements, 0x00RRGGBB,
bottom-up (Manager.hx:114-118): a CUDA/HIP `torch.int32` tensor (the frame stays in HBM) or a
C-contiguous `numpy.int32` array (host-pointer compatibility mode).
"""
from __future__ import annotations

import ctypes as C
import enum
import weakref
from dataclasses import dataclass
from typing import Any, Optional, Sequence

import numpy as np

from . import _native as N
from .player import INSIGNIFICANT_LINES


class DecoderState(enum.IntEnum):
    """IVideoCodec.hx:5-9"""
    zero_state = 0
    in_progress = 1
    error_occured = 2


@dataclass
class PFrameResult:
    """IVideoCodec.hx:11-14"""
    data_pnt: Any
    significant_changes: bool


@dataclass
class ChangeResult:
    """FindChange: the frame found (range index), whether it is significant (False: the range's last frame, nothing changed),
    the previous frame afterwards and the significance of each frame of the range (None where it was not judged)."""
    index: int
    changed: bool
    data_pnt: Any
    significance: list


class CodecError(RuntimeError):
    pass


def _src_arg(src):
    """bytes / bytearray / memoryview / numpy uint8 -> (object to keep alive, pointer, length)"""
    if src is None:
        return None, None, 0
    if isinstance(src, (bytes, bytearray)):
        keep = bytes(src) if isinstance(src, bytearray) else src
        return keep, C.cast(C.c_char_p(keep), C.c_void_p), len(keep)
    arr = np.ascontiguousarray(np.frombuffer(src, dtype=np.uint8) if not isinstance(src, np.ndarray) else src,
                               dtype=np.uint8)
    return arr, C.c_void_p(arr.ctypes.data), arr.size


def _range_args(srcs: Sequence, is_key: Optional[Sequence[bool]]):
    """A range of frames -> (ctypes pointer array, ctypes length array, is_key bytes or None, objects to keep alive until the
    native call returns)"""
    n = len(srcs)
    keeps, ptrs, lens = [], (C.c_void_p * n)(), (C.c_size_t * n)()
    for i, s in enumerate(srcs):
        keep, p, ln = _src_arg(s)
        keeps.append(keep)
        ptrs[i] = p.value if p is not None else None
        lens[i] = ln
    keys = bytes(bytearray(1 if k else 0 for k in is_key)) if is_key is not None else None
    return ptrs, lens, keys, keeps


def _frame_ptr(buf, npixels: int) -> int:
    """Address of a caller-owned frame buffer (torch device tensor or numpy host array)."""
    if isinstance(buf, np.ndarray):
        if buf.dtype != np.int32 or not buf.flags["C_CONTIGUOUS"] or buf.size < npixels:
            raise CodecError("host frame buffer must be C-contiguous int32 with >= width*height elements")
        return buf.ctypes.data
    # torch tensor (duck-typed so importing this module does not import torch)
    if hasattr(buf, "data_ptr"):
        import torch
        if buf.dtype != torch.int32 or not buf.is_contiguous() or buf.numel() < npixels:
            raise CodecError("frame tensor must be contiguous int32 with >= width*height elements")
        return buf.data_ptr()
    raise CodecError(f"unsupported frame buffer type {type(buf)!r}")


def _device_frame_ptr(buf, npixels: int, what: str) -> int:
    """Address of a frame buffer that a kernel reads or writes directly: a device tensor, nothing else.  The display calls launch on
    whatever pointer they are given, so a host array is refused here, before the native library is touched."""
    if isinstance(buf, np.ndarray) or not getattr(buf, "is_cuda", False):
        raise CodecError(f"{what}: frame buffers must be device tensors (got {type(buf).__name__}"
                         f"{' on the host' if hasattr(buf, 'data_ptr') else ''})")
    return _frame_ptr(buf, npixels)


class _NativeCodec:
    """Common part of the three codec classes: owns one jsp_codec handle."""

    _kind = 0

    def __init__(self, width: int, height: int, bpp: int = 0, palette: Optional[bytes] = None,
                 device: int = 0):
        self.X, self.Y = int(width), int(height)
        self._device = int(device)
        self._lib = N.lib()
        pal = bytes(palette) if palette is not None else None
        self._h = self._lib.jsp_codec_create(self._kind, self.X, self.Y, int(bpp), pal,
                                             len(pal) if pal else 0, int(device))
        if not self._h:
            raise CodecError(N.last_error())
        # address -> caller object, to hand identical objects back.  Weak: the codec keeps alive only what the
        # reference keeps alive — the current previous frame (`_prev`) — plus the frames of live staged batches
        # (held by the StagedBatch); a caller that allocates a fresh buffer per frame does not accumulate them here.
        self._bufs = weakref.WeakValueDictionary()
        self._prev = None
        self._inflight = {}   # ticket -> (src bytes, dst) of frames between *_async and wait()

    # -- IVideoCodec ------------------------------------------------------------------------
    def Preinit(self, insignificant_lines: int) -> None:
        if self._lib.jsp_preinit(self._h, int(insignificant_lines)) != 0:
            raise CodecError(N.last_error())

    def PreviousFrame(self):
        return self._prev

    def _track_prev(self):
        addr = self._lib.jsp_previous_frame(self._h)
        self._prev = self._bufs.get(addr) if addr else None

    def IsKeyFrame(self, data) -> bool:
        keep, p, n = _src_arg(data)
        return bool(self._lib.jsp_is_key_frame(self._h, p, n))

    def State(self) -> DecoderState:
        return DecoderState(self._lib.jsp_state(self._h))

    def ContinueI(self) -> DecoderState:
        return DecoderState(self._lib.jsp_continue_i(self._h))

    def DecompressI(self, src, dst) -> DecoderState:
        keep, p, n = _src_arg(src)
        addr = _frame_ptr(dst, self.X * self.Y)
        self._bufs[addr] = dst
        rc = self._lib.jsp_decompress_i(self._h, p, n, C.c_void_p(addr))
        self._track_prev()
        return DecoderState(rc)

    def DecompressP(self, src, dst) -> PFrameResult:
        keep, p, n = _src_arg(src)
        addr = _frame_ptr(dst, self.X * self.Y)
        self._bufs[addr] = dst
        out_ptr = C.c_void_p()
        signif = C.c_int(0)
        rc = self._lib.jsp_decompress_p(self._h, p, n, C.c_void_p(addr), C.byref(out_ptr), C.byref(signif))
        self._track_prev()
        if rc != 0:
            # the reference raises out of DecompressP here (e.g. TypeError on a null prevFrame)
            raise CodecError(N.last_error())
        data = self._prev if out_ptr.value else None   # *data_pnt is the previous frame after the call
        return PFrameResult(data, bool(signif.value))

    # -- asynchronous form of DecompressI / DecompressP (jsp_decompress_*_async ... jsp_wait) ------------------
    def DecompressI_async(self, src, dst) -> int:
        """Host stage now, uploads and kernels queued; returns a ticket for wait().  `src` and `dst` are kept alive here
        until then; device frame buffers only."""
        return self._submit(self._lib.jsp_decompress_i_async, src, dst, True)

    def DecompressP_async(self, src, dst) -> int:
        return self._submit(self._lib.jsp_decompress_p_async, src, dst, False)

    def _submit(self, fn, src, dst, key: bool) -> int:
        keep, p, n = _src_arg(src)
        addr = _frame_ptr(dst, self.X * self.Y)
        self._bufs[addr] = dst
        ticket = C.c_uint64(0)
        if fn(self._h, p, n, C.c_void_p(addr), C.byref(ticket)) != 0:
            raise CodecError(N.last_error())
        self._inflight[ticket.value] = (keep, dst, key)
        self._track_prev()
        return ticket.value

    def wait(self, ticket: int):
        """What the synchronous call would have returned for the frame submitted under `ticket` (tickets are waited for
        in submission order): a DecoderState for DecompressI_async, a PFrameResult for DecompressP_async (CodecError
        where DecompressP raises)."""
        if ticket not in self._inflight:
            raise CodecError(f"no frame in flight under ticket {ticket}")
        if ticket != next(iter(self._inflight)):
            # (checked here as well: jsp_wait refuses it without consuming anything, and the frame's bytes and buffer must stay
            # alive for as long as the native job holds them)
            raise CodecError("tickets are waited for in submission order")
        out_ptr, signif = C.c_void_p(), C.c_int(0)
        rc = self._lib.jsp_wait(self._h, ticket, C.byref(out_ptr), C.byref(signif))
        _, _, key = self._inflight.pop(ticket)   # jsp_wait consumes the oldest ticket whatever its result
        self._track_prev()
        if key:
            return DecoderState(rc)
        if rc != 0:
            raise CodecError(N.last_error())
        return PFrameResult(self._bufs.get(out_ptr.value) if out_ptr.value else None, bool(signif.value))

    # -- seek (jsp_seek): the seek branch of Manager.GetDecompressedFrame (Manager.hx:216-259) ------------------------
    SEEKS = True   # Seek() composes a range in one call (ScreenPressor: no, it decodes frame by frame)

    def Seek(self, srcs: Sequence, dst, is_key: Optional[Sequence[bool]] = None) -> PFrameResult:
        """The frames `srcs` (from where the stream stands — typically the nearest key frame — up to and including the
        target) as DecompressI / DecompressP would decode them in order, each destination starting out as the picture
        before it, composed into `dst` alone (a device buffer; one launch).  `data_pnt` is `dst` when a frame of the range
        would have adopted its destination, else the unchanged previous frame; `significant_changes` is the last frame's.
        CodecError where the reference raises (the previous frame is then None) and on ScreenPressor."""
        n = len(srcs)
        if n == 0:
            raise CodecError("seek: empty range")
        ptrs, lens, keys, keeps = _range_args(srcs, is_key)
        addr = _frame_ptr(dst, self.X * self.Y)
        self._bufs[addr] = dst
        out_ptr, signif = C.c_void_p(), C.c_int(0)
        rc = self._lib.jsp_seek(self._h, n, ptrs, lens, keys, C.c_void_p(addr), C.byref(out_ptr), C.byref(signif))
        self._track_prev()
        if rc != 0:
            raise CodecError(N.last_error())
        return PFrameResult(self._prev if out_ptr.value else None, bool(signif.value))

    # -- skip stills (jsp_find_change): Manager.SkipStills over DataLoader.FindPossibleChange (Manager.hx:289-317) ----------
    FINDS_CHANGES = True   # FindChange() judges a range in one call (ScreenPressor: no, it decodes frame by frame)

    def FindChange(self, srcs: Sequence, dst, is_key: Optional[Sequence[bool]] = None, first: int = 0,
                   key_before=None, key_row: int = INSIGNIFICANT_LINES) -> ChangeResult:
        """The frames `srcs` (from where the stream stands) as DecompressI / DecompressP would decode them in order, up to the
        first frame at or after `first` that changes the picture significantly — or the last frame when none does —, that
        frame's picture composed into `dst` alone (a device buffer).  Key frames are judged by the Manager's rule
        (frames_differ_significantly: `key_before` = the bytes of the key frame before the range, if it is one; the pixel
        compare from row `key_row` on).  CodecError where the reference raises (the previous frame is then None), on a bad
        `first` and on ScreenPressor."""
        n = len(srcs)
        if n == 0:
            raise CodecError("find_change: empty range")
        ptrs, lens, keys, keeps = _range_args(srcs, is_key)
        addr = _frame_ptr(dst, self.X * self.Y)
        self._bufs[addr] = dst
        kb_keep, kb_ptr, kb_len = _src_arg(key_before) if key_before is not None else (None, None, 0)
        out_ptr, found, changed, sig = C.c_void_p(), C.c_int(-1), C.c_int(0), (C.c_int * n)()
        rc = self._lib.jsp_find_change(self._h, n, ptrs, lens, keys, int(first), kb_ptr, kb_len, int(key_row), C.c_void_p(addr),
                                       C.byref(found), C.byref(changed), sig, C.byref(out_ptr))
        self._track_prev()
        if rc != 0:
            raise CodecError(N.last_error())
        return ChangeResult(found.value, bool(changed.value), self._prev if out_ptr.value else None,
                            [None if v < 0 else bool(v) for v in sig])

    # -- seek index (jsp_index_*): a range resident in HBM, any frame of it shown by one launch ---------------------------------
    INDEXES = True   # BuildIndex() keeps a range resident (ScreenPressor: no, it decodes frame by frame)

    def BuildIndex(self, srcs: Sequence, is_key: Optional[Sequence[bool]] = None, key_row: int = INSIGNIFICANT_LINES) -> "SeekIndex":
        """The frames `srcs` (from where the stream stands, as for Seek) staged once and kept in HBM: SeekIndex.Show(t) then
        writes what Seek(srcs[:t + 1]) on the codec as it stands now would write, in one launch.  Every frame is judged as
        FindChange judges it (`significance`).  The codec is left as it is; CodecError where the reference raises (the error names
        the frame) and on ScreenPressor."""
        n = len(srcs)
        if n == 0:
            raise CodecError("index: empty range")
        ptrs, lens, keys, keeps = _range_args(srcs, is_key)
        h = self._lib.jsp_index_build(self._h, n, ptrs, lens, keys, int(key_row))
        if not h:
            raise CodecError(N.last_error())
        return SeekIndex(self, h, self._prev)

    def NeedsIndex(self) -> bool:
        return bool(self._lib.jsp_needs_index(self._h))

    def StopAndClean(self) -> None:
        if getattr(self, "_h", None):
            self._lib.jsp_codec_destroy(self._h)   # waits for whatever is still in flight
            self._h = None
        self._inflight = {}                        # ... only then are the frames' bytes and buffers let go
        self._bufs = weakref.WeakValueDictionary()
        self._prev = None

    # -- batched / resident-input extension ----------------------------------------------------
    def set_stream(self, hip_stream: Optional[int]) -> None:
        self._lib.jsp_set_stream(self._h, C.c_void_p(hip_stream) if hip_stream else None)

    def set_option(self, key: str, value: str) -> None:
        if self._lib.jsp_set_option(self._h, key.encode(), value.encode()) != 0:
            raise CodecError(f"option {key}={value} not accepted")

    def sync(self) -> None:
        if self._lib.jsp_sync(self._h) != 0:
            raise CodecError(N.last_error())

    def KeyFrameDiffers(self) -> Optional[bool]:
        """With option "key_frame_compare" = "<first row>": whether the last key frame (DecompressI, or the last one collected with
        wait) differs from the frame before it from that row on — the pixel loop of Manager.frames_differ_significantly
        (Manager.hx:413-419), worked out with the decode; None when there was nothing to compare with (jsp_key_frame_differs)."""
        v = int(self._lib.jsp_key_frame_differs(self._h))
        return None if v < 0 else bool(v)

    def prefetch(self, host) -> None:
        """jsp_prefetch: the next frames' bytes lie in `host` (a numpy uint8 array / memoryview over a stretch of the file, ideally
        in pinned memory: PinnedBytes.array slices) — the codec may take the whole range to the device in one copy; asynchronous
        frames whose `src` is a slice of it then queue no upload of their own.  `None` gives every range up.  The range must stay
        alive and unchanged while the codec keeps it (the 4 most recent ranges): the object is held here."""
        if host is None:
            self._lib.jsp_prefetch(self._h, None, 0)
            self._ranges = []
            return
        keep, p, n = _src_arg(host)
        if self._lib.jsp_prefetch(self._h, p, n) != 0:
            raise CodecError(N.last_error())
        self._ranges = (getattr(self, "_ranges", []) + [keep])[-4:]

    def counter(self, name: str) -> int:
        """How often this instance took one of its slow paths ("async_reruns", "lookback_fallbacks"): jsp_counter."""
        v = int(self._lib.jsp_counter(self._h, name.encode()))
        if v < 0:
            raise CodecError(f"no counter named {name}")
        return v

    def stage_batch(self, srcs: Sequence, dsts: Sequence, is_key: Optional[Sequence[bool]] = None,
                    reuse: Optional["StagedBatch"] = None) -> "StagedBatch":
        """jsp_stage_batch; with `reuse` (a batch of this codec whose decodes have finished) jsp_restage_batch: the batch
        object's buffers are taken over, `reuse` itself is returned, now holding this batch."""
        n = len(srcs)
        if len(dsts) != n:
            raise CodecError("srcs and dsts differ in length")
        keeps, ptrs, lens = [], (C.c_void_p * n)(), (C.c_size_t * n)()
        dptrs = (C.c_void_p * n)()
        for i, (s, d) in enumerate(zip(srcs, dsts)):
            keep, p, ln = _src_arg(s)
            keeps.append(keep)
            ptrs[i] = p.value if p is not None else None
            lens[i] = ln
            addr = _frame_ptr(d, self.X * self.Y)
            self._bufs[addr] = d
            dptrs[i] = addr
        keys = bytes(bytearray(1 if k else 0 for k in is_key)) if is_key is not None else None
        if reuse is not None and reuse._h:
            h = self._lib.jsp_restage_batch(self._h, reuse._h, n, ptrs, lens, keys, dptrs)
            if not h:
                raise CodecError(N.last_error())
            self._track_prev()
            reuse._h, reuse.n, reuse._dsts = h, n, list(dsts)
            return reuse
        h = self._lib.jsp_stage_batch(self._h, n, ptrs, lens, keys, dptrs)
        if not h:
            raise CodecError(N.last_error())
        self._track_prev()
        return StagedBatch(self, h, n, list(dsts))

    def DecompressI_batch(self, srcs: Sequence, dsts: Sequence) -> DecoderState:
        st = self.stage_batch(srcs, dsts)
        try:
            st.decode()
            self.sync()
            status, _, _ = st.results()
            bad = [s for s in status if s != 0]
            return DecoderState(bad[0] if bad else 0)
        finally:
            st.close()

    def __del__(self):
        try:
            self.StopAndClean()
        except Exception:
            pass


class StagedBatch:
    """A batch whose descriptor tables are resident in HBM (jsp_stage_batch)."""

    def __init__(self, codec: _NativeCodec, handle: int, n: int, dsts=()):
        self._codec, self._h, self.n = codec, handle, n
        self._dsts = dsts   # the kernels write here for as long as the batch can be decoded

    def decode(self) -> None:
        """Queue the reconstruction kernels (asynchronous on the codec's stream)."""
        if self._codec._lib.jsp_staged_decode(self._codec._h, self._h) != 0:
            raise CodecError(N.last_error())

    def info(self) -> dict:
        out = N.StagedInfo()
        self._codec._lib.jsp_staged_get_info(self._h, C.byref(out))
        return out.as_dict()

    def kernels(self) -> str:
        """Names of the kernels decode() launches, " + " separated (jsp_staged_kernels)."""
        return self._codec._lib.jsp_staged_kernels(self._h).decode()

    def results(self):
        st, ad, sg = (C.c_int * self.n)(), (C.c_int * self.n)(), (C.c_int * self.n)()
        self._codec._lib.jsp_staged_results(self._h, st, ad, sg)
        return list(st), list(ad), list(sg)

    def close(self) -> None:
        if self._h:
            self._codec._lib.jsp_staged_destroy(self._h)
            self._h = None
        self._dsts = ()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _IndexThumbs:
    """ThumbSize / Thumbs of a seek index, MSVideo1 or ScreenPressor: the two C calls have one contract, so the sheet arithmetic is
    here once.  A subclass names its pair of C functions in `_THUMB_CALLS` and has `_open(who)` (the codec, or CodecError)."""

    _THUMB_CALLS = ("", "")   # (thumb_size, thumbs): exports of the library, without the "jsp_" in front

    def ThumbSize(self, scale: int) -> tuple:
        """(width, height) of a thumbnail at `scale` (4, 8 or 16): whole scale x scale squares of the picture (of its whole 4x4
        blocks for MSVideo1, which is the same number at these scales)."""
        size_call, _ = self._THUMB_CALLS
        self._open(size_call)
        tw, th = C.c_int(0), C.c_int(0)
        if getattr(self._lib, "jsp_" + size_call)(self._h, int(scale), C.byref(tw), C.byref(th)) != 0:
            raise CodecError(N.last_error())
        return tw.value, th.value

    def Thumbs(self, frames, scale: int = 8, cols: int = 1, out=None):
        """The pictures of `frames` (any frame numbers of the index: unordered, repeats allowed, 1..4096 of them), each reduced
        scale x scale pixels to one (box mean, rounded half up), `cols` to a sheet row: ONE launch, the codec is not touched.
        Returns the sheet, an int32 device tensor of shape (ceil(n / cols) * TH, cols * TW) — `out` (contiguous, at least that
        many elements; cells of the last row past n keep what they held) or a new zero-filled one.  Rows are bottom-up as in a
        frame."""
        size_call, thumbs_call = self._THUMB_CALLS
        codec = self._open(thumbs_call)
        frames = [int(t) for t in frames]
        n, scale, cols = len(frames), int(scale), int(cols)
        tw, th = C.c_int(0), C.c_int(0)
        getattr(self._lib, "jsp_" + size_call)(self._h, scale, C.byref(tw), C.byref(th))   # (refused: 0 x 0, and the thumbs call says why)
        rows, width = -(-n // max(cols, 1)) * th.value, max(cols, 1) * tw.value
        if out is None:
            import torch
            out = torch.zeros(max(rows * width, 1), dtype=torch.int32, device=f"cuda:{codec._device}")
        arr = (C.c_int * max(n, 1))(*frames)
        rc = getattr(self._lib, "jsp_" + thumbs_call)(codec._h, self._h, n, arr, scale, cols, C.c_void_p(_frame_ptr(out, 0)), int(np.prod(out.shape)))
        if rc != 0:
            raise CodecError(N.last_error())
        return out.reshape(-1)[:rows * width].reshape(rows, width)


class _IndexPresent:
    """Present of a seek index, MSVideo1 or ScreenPressor: the two C calls have one contract (jsp_index_present), so the sheet
    arithmetic is here once.  A subclass names its C function in `_PRESENT_CALL` and has `_open(who)` and `_present_mode()`."""

    _PRESENT_CALL = ""   # export of the library, without the "jsp_" in front

    def _present_mode(self) -> int:
        return 0   # DISPLAY_CANVAS

    def Present(self, frames, win_w: int, win_h: int, k: float, dx: float, dy: float, mode: Optional[int] = None, filter: int = 1,
                background: int = 0xFF000000, cols: int = 1, out=None):
        """The win_w x win_h windows of `frames` (any frame numbers of the index: unordered, repeats allowed, 1..4096 of them)
        under the display matrix (k, dx, dy) of view_matrix, `cols` to a sheet row: cell i is exactly what display_present
        (filter PRESENT_NEAREST / PRESENT_BILINEAR, the default) or display_present_area (PRESENT_AREA) writes for the picture of
        frames[i] — ONE launch, no full-size picture, no frame buffer written, the codec not touched.  `mode` defaults to the
        conversion that gives canvas pixels.  Returns the sheet, an int32 device tensor of shape (ceil(n / cols) * win_h,
        cols * win_w), top row first — `out` (contiguous, at least that many elements, row pitch cols * win_w; cells of the last
        row past n keep what they held) or a new zero-filled one."""
        codec = self._open(self._PRESENT_CALL)
        frames = [int(t) for t in frames]
        n, cols, win_w, win_h = len(frames), int(cols), int(win_w), int(win_h)
        rows, width = -(-n // max(cols, 1)) * max(win_h, 0), max(cols, 1) * max(win_w, 0)
        if out is None:
            import torch
            out = torch.zeros(max(rows * width, 1), dtype=torch.int32, device=f"cuda:{codec._device}")
        arr = (C.c_int * max(n, 1))(*frames)
        rc = getattr(self._lib, "jsp_" + self._PRESENT_CALL)(
            codec._h, self._h, n, arr, C.c_void_p(_frame_ptr(out, 0)), int(np.prod(out.shape)), win_w, win_h, width, cols,
            float(k), float(dx), float(dy), self._present_mode() if mode is None else int(mode), int(filter), int(background) & 0xFFFFFFFF)
        if rc != 0:
            raise CodecError(N.last_error())
        return out.reshape(-1)[:rows * width].reshape(rows, width)


TENSOR_F32, TENSOR_F16, TENSOR_BF16, TENSOR_U8 = 0, 1, 2, 3   # JSP_TENSOR_*: the element type of Tensor
TENSOR_NCHW, TENSOR_NHWC = 0, 1                               # ... and its layout


def normalisation(mean, std):
    """(scale, bias) for Tensor from a model's per-channel mean and std over pixel values in 0..1: element = (v / 255 - mean) / std
    = v * scale + bias with scale = 1 / (255 * std) and bias = -mean / std, computed in Python floats and each rounded to float32."""
    mean, std = [float(m) for m in mean], [float(s) for s in std]
    if len(mean) != 3 or len(std) != 3:
        raise ValueError("normalisation: mean and std have one value per channel (R, G, B)")
    return (tuple(float(np.float32(1.0 / (255.0 * s))) for s in std),
            tuple(float(np.float32(-m / s)) for m, s in zip(mean, std)))


def _tensor_dtype(dtype):
    """(JSP_TENSOR_* code, torch dtype) of a torch dtype, its name ("float16", "f16", ...) or a JSP_TENSOR_* code."""
    import torch
    kinds = ((TENSOR_F32, torch.float32, ("float32", "f32")), (TENSOR_F16, torch.float16, ("float16", "f16")),
             (TENSOR_BF16, torch.bfloat16, ("bfloat16", "bf16")), (TENSOR_U8, torch.uint8, ("uint8", "u8")))
    for code, tdtype, names in kinds:
        if dtype is tdtype or (isinstance(dtype, str) and dtype.lower() in names) or (isinstance(dtype, int) and dtype == code):
            return code, tdtype
    raise CodecError(f"index_tensor: unknown dtype {dtype!r}")


class _IndexTensor:
    """Tensor of a seek index, MSVideo1 or ScreenPressor: the two C calls have one contract (jsp_index_tensor).  A subclass names its
    C function in `_TENSOR_CALL` and has `_open(who)` and `_present_mode()` (_IndexPresent's)."""

    _TENSOR_CALL = ""   # export of the library, without the "jsp_" in front

    def Tensor(self, frames, win_w: int, win_h: int, k: float, dx: float, dy: float, *, mode: Optional[int] = None, filter: int = 2,
               background: int = 0xFF000000, dtype=None, layout: str = "nchw", scale=(1 / 255,) * 3, bias=(0,) * 3, out=None):
        """The win_w x win_h windows of `frames` that Present gives (same frames, matrix, mode, filter — default PRESENT_AREA — and
        background) as a model's input batch: a device tensor of `dtype` (torch.float32, the default, float16, bfloat16 or uint8)
        and shape (n, 3, win_h, win_w) (`layout` "nchw") or (n, win_h, win_w, 3) ("nhwc"), channels R, G, B, top row first.  An
        element is the byte v of its channel for uint8, else float32(v * scale[ch] + bias[ch]) computed in double, rounded once
        more (to nearest-even) for the 16-bit types; `normalisation(mean, std)` gives (scale, bias).  ONE launch, no sheet in
        between, the codec not touched.  Returns `out` (a contiguous device tensor of that dtype with at least n * 3 * win_h *
        win_w elements, reshaped) or a new tensor."""
        import torch
        codec = self._open(self._TENSOR_CALL)
        frames = [int(t) for t in frames]
        n, win_w, win_h = len(frames), int(win_w), int(win_h)
        code, tdtype = _tensor_dtype(torch.float32 if dtype is None else dtype)
        lay = {"nchw": TENSOR_NCHW, "nhwc": TENSOR_NHWC}.get(layout.lower() if isinstance(layout, str) else layout, layout)
        if lay not in (TENSOR_NCHW, TENSOR_NHWC):
            raise CodecError(f"{self._TENSOR_CALL}: unknown layout {layout!r}")
        count = n * 3 * max(win_h, 0) * max(win_w, 0)
        if out is None:
            out = torch.empty(max(count, 1), dtype=tdtype, device=f"cuda:{codec._device}")
        elif not hasattr(out, "data_ptr") or out.dtype != tdtype or not out.is_contiguous():
            raise CodecError(f"{self._TENSOR_CALL}: out must be a contiguous tensor of dtype {tdtype}")
        arr = (C.c_int * max(n, 1))(*frames)
        sc = (C.c_float * 3)(*[float(v) for v in scale]) if scale is not None else None
        bi = (C.c_float * 3)(*[float(v) for v in bias]) if bias is not None else None
        rc = getattr(self._lib, "jsp_" + self._TENSOR_CALL)(
            codec._h, self._h, n, arr, C.c_void_p(out.data_ptr()), out.numel() * out.element_size(), win_w, win_h,
            float(k), float(dx), float(dy), self._present_mode() if mode is None else int(mode), int(filter), int(background) & 0xFFFFFFFF,
            code, lay, sc, bi)
        if rc != 0:
            raise CodecError(N.last_error())
        shape = (n, 3, win_h, win_w) if lay == TENSOR_NCHW else (n, win_h, win_w, 3)
        return out.reshape(-1)[:count].reshape(shape)


ACTIVITY_MAX_RUN = 4096   # frames one jsp_index_activity / jsp_sp_index_activity call takes (jsp_index_distance / jsp_sp_index_distance too)
REF_PICTURE = -2          # JSP_REF_PICTURE: the ref_frame that goes with a reference picture
DELTA_ASK_TWICE = 64 << 20   # SeekIndex.DeltaFrames: above this many bytes of n frames at their bound, the lengths are asked for first


class _IndexActivity:
    """ActivitySize / Activity of a seek index, MSVideo1 or ScreenPressor: the two C calls have one contract (jsp_index_activity).  A
    subclass names its pair of C functions in `_ACTIVITY_CALLS` and has `_open(who)` and `frames`."""

    _ACTIVITY_CALLS = ("", "")   # (activity_size, activity): exports of the library, without the "jsp_" in front

    def ActivitySize(self) -> tuple:
        """(cols, rows) of the activity grid: ceil(X / 16), ceil(Y / 16) cells of 16 x 16 pixels, the last column / row clipped."""
        size_call, _ = self._ACTIVITY_CALLS
        self._open(size_call)
        cols, rows = C.c_int(0), C.c_int(0)
        if getattr(self._lib, "jsp_" + size_call)(self._h, C.byref(cols), C.byref(rows)) != 0:
            raise CodecError(N.last_error())
        return cols.value, rows.value

    def Activity(self, first: int = 0, n: Optional[int] = None, out=None):
        """How many pixels of each 16 x 16 cell each of the frames first .. first + n - 1 (n None: to the end of the index) changed:
        element [k, r, q] counts the pixels of cell (r, q) that differ between the pictures of frames first + k and first + k - 1
        (the picture before frame 0: the one before the index, else zeros) — 0 .. 256.  Grid rows are in the frame's own bottom-up
        order, as a thumbnail's.  ONE launch per 4096 frames, no picture written, the codec not touched.  Returns an int16 device
        tensor of shape (n, rows, cols) — no value exceeds 256, so the bits are the C call's uint16_t — `out` when it is given (that
        shape and dtype, contiguous) or a new one."""
        import torch
        size_call, call = self._ACTIVITY_CALLS
        codec = self._open(call)
        first = int(first)
        n = self.frames - first if n is None else int(n)
        cols, rows = self.ActivitySize()
        shape = (max(n, 0), rows, cols)
        if out is None:
            out = torch.empty(shape, dtype=torch.int16, device=f"cuda:{codec._device}")
        elif not hasattr(out, "data_ptr") or out.dtype != torch.int16 or tuple(out.shape) != shape or not out.is_contiguous():
            raise CodecError(f"{call}: out must be a contiguous int16 tensor of shape {shape}")
        fn = getattr(self._lib, "jsp_" + call)
        cell = rows * cols
        k = 0
        while True:   # (a run the C call refuses — empty, outside the index — goes to it once, for its message)
            m = min(n - k, ACTIVITY_MAX_RUN)
            if fn(codec._h, self._h, first + k, m, C.c_void_p(out.data_ptr() + 2 * k * cell), (out.numel() - k * cell)) != 0:
                raise CodecError(N.last_error())
            k += m
            if k >= n:
                break
        if hasattr(self, "_info"):
            self._info()   # (a ScreenPressor index that never played gets Play's per-frame table at the first call)
        return out

    _DISTANCE_CALL = ""   # jsp_index_distance / jsp_sp_index_distance, without the "jsp_" in front: one contract, on Activity's grid

    def Distance(self, ref, first: int = 0, n: Optional[int] = None, out=None):
        """How many pixels of each 16 x 16 cell of each of the frames first .. first + n - 1 (n None: to the end of the index) differ
        from ONE reference picture: element [k, r, q] counts the pixels of cell (r, q) that differ between the picture of frame
        first + k and R — 0 .. 256, on Activity's grid.  `ref` is an int, -1 .. frames - 1 (R is that frame's picture, -1 the picture
        before frame 0; nothing is written or shown for it), or a device frame buffer — a contiguous int32 device tensor of at least
        X * Y elements, anything else raises CodecError before the native call —, which is only read
        (MSVideo1: its X % 4 / Y % 4 remainder pixels are not compared).  ONE launch per 4096 frames, no picture written, the codec
        not touched.  Returns an int16 device tensor of shape (n, rows, cols), `out` when it is given (that shape and dtype,
        contiguous) or a new one."""
        import torch
        call = self._DISTANCE_CALL
        codec = self._open(call)
        first = int(first)
        n = self.frames - first if n is None else int(n)
        if hasattr(ref, "data_ptr") or isinstance(ref, np.ndarray):   # (the kernel reads X * Y words of it: checked before the call)
            ref_frame, ref_ptr = REF_PICTURE, C.c_void_p(_device_frame_ptr(ref, codec.X * codec.Y, call))
        elif isinstance(ref, bool) or not hasattr(ref, "__index__"):
            raise CodecError(f"{call}: ref must be a frame number or a device frame buffer")
        else:
            ref_frame, ref_ptr = int(ref), None
        cols, rows = self.ActivitySize()
        shape = (max(n, 0), rows, cols)
        if out is None:
            out = torch.empty(shape, dtype=torch.int16, device=f"cuda:{codec._device}")
        elif not hasattr(out, "data_ptr") or out.dtype != torch.int16 or tuple(out.shape) != shape or not out.is_contiguous():
            raise CodecError(f"{call}: out must be a contiguous int16 tensor of shape {shape}")
        fn = getattr(self._lib, "jsp_" + call)
        cell = rows * cols
        k = 0
        while True:   # (a run the C call refuses — empty, outside the index — goes to it once, for its message)
            m = min(n - k, ACTIVITY_MAX_RUN)
            if fn(codec._h, self._h, ref_frame, ref_ptr, first + k, m, C.c_void_p(out.data_ptr() + 2 * k * cell), (out.numel() - k * cell)) != 0:
                raise CodecError(N.last_error())
            k += m
            if k >= n:
                break
        if hasattr(self, "_info"):
            self._info()
        return out


class SeekIndex(_IndexThumbs, _IndexPresent, _IndexTensor, _IndexActivity):
    """A range resident in HBM (jsp_index_build, via BuildIndex): Show(t) is one launch, Play(first, dsts, stride) one launch for
    a run of frames, each into a buffer of its own (jsp_index_play), Present(frames, ...) one launch for the windows of any
    frames (jsp_index_present), Tensor(frames, ...) one launch for the same windows as a model's input batch (jsp_index_tensor),
    Activity(first, n) one launch for the changed pixels per frame and 16x16 cell of a run (jsp_index_activity; _IndexActivity),
    Distance(ref, first, n) one launch for the pixels per frame and cell that differ from ONE reference picture (jsp_index_distance),
    KeyFrame(t) two launches for a key frame that decodes to frame t's picture, made of the codes the range holds (jsp_index_key_frame),
    DeltaFrames(pairs) inter frames that each span a gap (a, b] of the range, made of the same codes and skips (jsp_index_delta_frames);
    with tight=True without the blocks whose pixels the gap did not change (jsp_index_tight_frames).  CropFrames / PanFrames the same
    for a block rectangle that stands or moves, PathFrames for pairs in either direction — steps back and holds: a reversed clip.
    `significance` = FindChange's verdict
    for every frame, `frames`, `device_bytes`.  close() (or the context manager) frees it; safe after the codec is gone."""

    ADOPTS = True   # Show(adopt=True) leaves the decoder at frame t: a Manager moves its decode position with it
    _THUMB_CALLS = ("index_thumb_size", "index_thumbs")
    _PRESENT_CALL = "index_present"
    _TENSOR_CALL = "index_tensor"
    _ACTIVITY_CALLS = ("index_activity_size", "index_activity")
    _DISTANCE_CALL = "index_distance"

    def __init__(self, codec: _NativeCodec, handle: int, prev_at_build):
        self._codec, self._h = codec, handle
        self._prev_at_build = prev_at_build   # what data_pnt is for a frame before the first one that adopts its buffer
        lib = codec._lib
        n, dev, host = C.c_int(0), C.c_uint64(0), C.c_uint64(0)
        lib.jsp_index_info(handle, C.byref(n), C.byref(dev), C.byref(host))
        self.frames, self.device_bytes, self.host_bytes = n.value, dev.value, host.value
        sig = (C.c_int * self.frames)()
        lib.jsp_index_significance(handle, sig)
        self.significance = [bool(v) for v in sig]
        self._lib = lib

    def Show(self, t: int, dst, adopt: bool = True) -> PFrameResult:
        """Frame t's picture into `dst` (a device buffer, not the codec's previous frame), as Seek(srcs[:t + 1]) would write it
        on the codec as it stood at the build.  adopt: the codec ends as that Seek leaves it (DecompressP(t + 1) follows on);
        else it is not touched."""
        codec = self._open("index_show")
        addr = _frame_ptr(dst, codec.X * codec.Y)
        codec._bufs[addr] = dst
        out_ptr, signif = C.c_void_p(), C.c_int(0)
        rc = self._lib.jsp_index_show(codec._h, self._h, int(t), C.c_void_p(addr), 1 if adopt else 0, C.byref(out_ptr), C.byref(signif))
        if rc != 0:
            raise CodecError(N.last_error())
        if adopt:
            codec._track_prev()
        if not out_ptr.value:
            data = None
        elif out_ptr.value == addr:
            data = dst
        else:
            data = self._prev_at_build
        return PFrameResult(data, bool(signif.value))

    def Play(self, first: int, dsts, stride: int = 1, adopt: Optional[int] = None) -> list:
        """Frames first, first + stride, ... of the index, one per buffer of `dsts` (device buffers, all different, none the
        codec's previous frame): dsts[k] ends exactly as Show(first + k * stride, dsts[k], adopt=False) leaves it — ONE launch
        whatever len(dsts) and stride (jsp_index_play): frame `first` is composed once, the pixels are carried forward in
        registers and only the last writer of each gap is decoded.  Returns Show's PFrameResult per buffer.  adopt: an index into
        `dsts`; the codec ends as Show(that frame, that buffer, adopt=True) leaves it (None: it is not touched).  Reverse
        playback: the same call with adopt=0, the buffers shown in reverse."""
        codec = self._open("index_play")
        dsts = list(dsts)
        n = len(dsts)
        addrs = [_frame_ptr(d, codec.X * codec.Y) for d in dsts]
        ptrs = (C.c_void_p * max(n, 1))(*addrs)
        outs = (C.c_void_p * max(n, 1))()
        signif = (C.c_int * max(n, 1))()
        adopt_k = -1 if adopt is None else int(adopt)
        if adopt is not None and not 0 <= adopt_k < n:
            raise CodecError("index_play: adopt is outside dsts")
        if 0 <= adopt_k < n:
            codec._bufs[addrs[adopt_k]] = dsts[adopt_k]
        if self._lib.jsp_index_play(codec._h, self._h, int(first), n, int(stride), ptrs, adopt_k, outs, signif) != 0:
            raise CodecError(N.last_error())
        if adopt_k >= 0:
            codec._track_prev()
        dev, host = C.c_uint64(0), C.c_uint64(0)   # (the first Play adds the destination list, a longer run a longer one)
        self._lib.jsp_index_info(self._h, None, C.byref(dev), C.byref(host))
        self.device_bytes, self.host_bytes = dev.value, host.value
        results = []
        for k, d in enumerate(dsts):
            data = None if not outs[k] else d if outs[k] == addrs[k] else self._prev_at_build
            results.append(PFrameResult(data, bool(signif[k])))
        return results

    def KeyFrameBound(self) -> int:
        """The most bytes KeyFrame returns: 18 per 4x4 block of a 16-bit picture, 10 per block of an 8-bit one."""
        self._open("index_key_frame_bound")
        n = C.c_size_t(0)
        if self._lib.jsp_index_key_frame_bound(self._h, C.byref(n)) != 0:
            raise CodecError(N.last_error())
        return n.value

    def KeyFrame(self, t: int) -> bytes:
        """A key frame that decodes to the picture of frame t: for every block the code of its last writer <= t, in block order —
        bytes the range already contained, nothing decoded or re-quantised (jsp_index_key_frame: two launches, the codec not
        touched).  IsKeyFrame of it is true; the range's frames t + 1 ... decoded on top give the pictures the range gives.
        CodecError, naming the block, when a block has no writer <= t in the index or its last writer's code is cut off."""
        codec = self._open("index_key_frame")
        buf = (C.c_uint8 * max(self.KeyFrameBound(), 1))()
        n = C.c_size_t(0)
        if self._lib.jsp_index_key_frame(codec._h, self._h, int(t), buf, len(buf), C.byref(n)) != 0:
            raise CodecError(N.last_error())
        dev, host = C.c_uint64(0), C.c_uint64(0)   # (the first call adds the scratch the frame is assembled in)
        self._lib.jsp_index_info(self._h, None, C.byref(dev), C.byref(host))
        self.device_bytes, self.host_bytes = dev.value, host.value
        return bytes(memoryview(buf)[:n.value])

    def DeltaBound(self) -> int:
        """The most bytes one frame of DeltaFrames has: 18 per 4x4 block of a 16-bit picture, 10 per block of an 8-bit one."""
        self._open("index_delta_bound")
        n = C.c_size_t(0)
        if self._lib.jsp_index_delta_bound(self._h, C.byref(n)) != 0:
            raise CodecError(N.last_error())
        return n.value

    def DeltaFrames(self, pairs, tight: bool = False) -> list:
        """One inter frame per pair (a, b), -1 <= a < b < frames: decoded on top of the picture of frame a (-1: the picture before the
        range) it gives the picture of frame b — for every block the code of its last writer in (a, b], else a skip; bytes the range
        already contained, nothing decoded or re-quantised (jsp_index_delta_frames: two launches per slice of pairs, the codec not
        touched).  IsKeyFrame of a frame is true exactly when its gap writes every block.  CodecError, naming the pair, the block and
        the writer frame, when a written block's last code is cut off; nothing is returned then.
        tight: a block the gap codes but whose 16 pixels are the same before and after it is dropped as well (jsp_index_tight_frames:
        the sizes launch decodes both ends of the gap and compares them) — frames never longer than without it, the same pictures;
        "written" above then reads "kept", and a dropped block's cut code refuses nothing."""
        codec = self._open("index_tight" if tight else "index_delta")
        call = self._lib.jsp_index_tight_frames if tight else self._lib.jsp_index_delta_frames
        pairs = [(int(a), int(b)) for a, b in pairs]
        n = len(pairs)
        frm = (C.c_int * max(n, 1))(*[a for a, _ in pairs])
        to = (C.c_int * max(n, 1))(*[b for _, b in pairs])
        lens = (C.c_size_t * max(n, 1))()
        total = C.c_size_t(0)
        cap = max(n, 1) * self.DeltaBound()
        return self._clip_tail(n, cap, lens, total, lambda out, room: call(codec._h, self._h, n, frm, to, out, room, lens, C.byref(total)))

    KEY = -2            # JSP_CROP_KEY: a pair's `a` that makes it a key pair of CropFrames
    _CROP_TIGHT = 1     # JSP_CROP_TIGHT

    def CropBound(self, bw: int, bh: int) -> int:
        """The most bytes one frame of CropFrames has for a rectangle of bw x bh blocks: 18 per block at 16 bits, 10 at 8."""
        self._open("index_crop_bound")
        n = C.c_size_t(0)
        if self._lib.jsp_index_crop_bound(self._h, int(bw), int(bh), C.byref(n)) != 0:
            raise CodecError(N.last_error())
        return n.value

    def CropFrames(self, rect, pairs, tight: bool = False):
        """The frames of the block rectangle rect = (bx, by, bw, bh) — 4x4 blocks in table order, block row 0 the BOTTOM of the picture
        as displayed — one per pair: (list of bytes, list of bool).  A pair (SeekIndex.KEY, t) is the key frame of the rectangle at
        frame t; a pair (a, b), -1 <= a < b < frames, the inter frame over the gap as DeltaFrames makes it (tight: as
        DeltaFrames(tight=True); key pairs are not touched), both of the virtual index whose block j is block j of the rectangle
        (jsp_index_crop_frames: two launches per slice of pairs, the codec not touched).  A decoder of 4 bw x 4 bh pixels fed a key
        pair's frame and then chained gap pairs' frames shows that part of the source's pictures.  The flag of a frame says that it
        codes every block of the rectangle: IsKeyFrame of it.  CodecError, naming the pair, the block (in the rectangle and in the
        picture), the kind and for a cut code the writer frame; nothing is returned then."""
        return self._rect_frames("index_crop", self._lib.jsp_index_crop_frames, rect, pairs, tight)

    def PathFrames(self, rect, pairs, tight: bool = False):
        """CropFrames with pairs in EITHER direction: (list of bytes, list of bool), one frame per pair.  Besides CropFrames' pairs —
        (SeekIndex.KEY, t) and a step forward (a, b), a < b — a pair may step BACK, (a, b) with 0 <= b < a < frames: the inter frame
        from the picture of frame a to the picture of the EARLIER frame b, for every block that a frame of (b, a] coded the code of
        its last writer <= b, a skip elsewhere; or HOLD, (a, a): only skip words.  tight drops the blocks whose pixels are equal in
        both pictures (jsp_index_path_frames: two launches per slice of pairs, the codec not touched).  rect=None is the whole block
        grid.  A decoder of 4 bw x 4 bh pixels fed a key pair's frame and then the frames of pairs chained by their ends, in any
        order of frames, shows that part of the source's pictures along the path: a reversed clip, a boomerang, a freeze frame.
        CodecError as CropFrames'; a step back to a block that no frame up to b coded refuses ("no writer")."""
        if rect is None:
            rect = (0, 0, self._codec.X // 4, self._codec.Y // 4)
        return self._rect_frames("index_path", self._lib.jsp_index_path_frames, rect, pairs, tight)

    def _rect_frames(self, who: str, call, rect, pairs, tight: bool):
        """CropFrames and PathFrames: one marshalling of a rectangle, pairs and the tight flag around `call`."""
        codec = self._open(who)
        bx, by, bw, bh = (int(v) for v in rect)
        pairs = [(int(a), int(b)) for a, b in pairs]
        n = len(pairs)
        frm = (C.c_int * max(n, 1))(*[a for a, _ in pairs])
        to = (C.c_int * max(n, 1))(*[b for _, b in pairs])
        lens = (C.c_size_t * max(n, 1))()
        keys = (C.c_int * max(n, 1))()
        total = C.c_size_t(0)
        flags = self._CROP_TIGHT if tight else 0
        # (a rectangle the block grid does not hold gives no bound to size a buffer by: the call then refuses in its own order)
        bound = C.c_size_t(0)
        self._lib.jsp_index_crop_bound(self._h, bw, bh, C.byref(bound))
        cap = n * bound.value if 1 <= n <= 4096 else 0
        out = self._clip_tail(n, cap, lens, total, lambda out, room: call(codec._h, self._h, bx, by, bw, bh, n, frm, to, flags, out, room, lens,
                                                                          keys, C.byref(total)))
        return out, [bool(keys[j]) for j in range(n)]

    def PanFrames(self, size, pairs, tight: bool = False):
        """CropFrames for a rectangle of size = (bw, bh) blocks that MOVES: (list of bytes, list of bool), one frame per pair.  A pair
        is (a, b, (abx, aby), (bbx, bby)) — the rectangle stands at (abx, aby) in the picture of frame a and at (bbx, bby) in that of
        frame b, origins in table order as CropFrames' — or (SeekIndex.KEY, t, None, (bx, by)), the key frame of the rectangle there.
        With equal origins a pair is CropFrames' gap pair; with different ones (a <= b: the picture may stand still) the frame codes
        every block, or with tight only those where the block that stood at that position of the rectangle before differs from the
        one that stands there now (jsp_index_pan_frames).  A decoder of 4 bw x 4 bh pixels fed a key pair's frame and then chained
        pairs' frames shows the rectangle along its path.  CodecError with the C text; nothing is returned then."""
        codec = self._open("index_pan")
        bw, bh = (int(v) for v in size)
        pairs = [(int(a), int(b), None if fa is None else (int(fa[0]), int(fa[1])), (int(tb[0]), int(tb[1]))) for a, b, fa, tb in pairs]
        n = len(pairs)
        m = max(n, 1)
        frm = (C.c_int * m)(*[p[0] for p in pairs])
        to = (C.c_int * m)(*[p[1] for p in pairs])
        to_xy = (C.c_int * (2 * m))(*[v for p in pairs for v in p[3]])
        if all(p[2] is None for p in pairs):
            from_xy = None
        else:   # (a key pair's origin at `from` is not read)
            from_xy = (C.c_int * (2 * m))(*[v for p in pairs for v in (p[2] if p[2] is not None else p[3])])
        lens = (C.c_size_t * m)()
        keys = (C.c_int * m)()
        total = C.c_size_t(0)
        flags = self._CROP_TIGHT if tight else 0
        call = self._lib.jsp_index_pan_frames
        bound = C.c_size_t(0)
        self._lib.jsp_index_crop_bound(self._h, bw, bh, C.byref(bound))
        cap = n * bound.value if 1 <= n <= 4096 else 0
        out = self._clip_tail(n, cap, lens, total, lambda out, room: call(codec._h, self._h, bw, bh, n, frm, to, from_xy, to_xy, flags, out, room,
                                                                          lens, keys, C.byref(total)))
        return out, [bool(keys[j]) for j in range(n)]

    def _clip_tail(self, n: int, cap: int, lens, total, call) -> list:
        """What DeltaFrames, CropFrames, PathFrames and PanFrames do once their arguments are marshalled: call(out, room) is the C call
        with everything but the buffer bound, filling lens[] and total; cap is the room the caller worked out (it decides which refusal a
        bad n meets).  The n frames as a list of bytes."""
        if cap > DELTA_ASK_TWICE:   # many large frames: the lengths first (cap 0 is the refusal that still sets them), then the bytes
            if call(None, 0) == 0 or total.value == 0:
                raise CodecError(N.last_error())
            cap = total.value
        buf = (C.c_uint8 * max(cap, 1))()
        if call(buf, len(buf)) != 0:
            raise CodecError(N.last_error())
        dev, host = C.c_uint64(0), C.c_uint64(0)   # (the first call adds the scratch the frames are assembled in)
        self._lib.jsp_index_info(self._h, None, C.byref(dev), C.byref(host))
        self.device_bytes, self.host_bytes = dev.value, host.value
        view, out, at = memoryview(buf), [], 0
        for j in range(n):
            out.append(bytes(view[at:at + lens[j]]))
            at += lens[j]
        return out

    def _open(self, who: str) -> _NativeCodec:
        if not self._h:
            raise CodecError(f"{who}: the index is closed")
        if not self._codec._h:
            raise CodecError(f"{who}: the codec is closed")
        return self._codec

    def close(self) -> None:
        if self._h:
            self._lib.jsp_index_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class MSVideo1_16bit(_NativeCodec):
    """MSVideo1.hx:8-260 — `new MSVideo1_16bit(width, height)`"""
    _kind = N.JSP_CODEC_MSVIDEO1_16

    def __init__(self, width: int, height: int, device: int = 0):
        super().__init__(width, height, 16, None, device)


class MSVideo1_8bit(_NativeCodec):
    """MSVideo1.hx:262-429 — `new MSVideo1_8bit(width, height, palette)`; `palette` = the strf
    bytes after the BITMAPINFOHEADER (RGBQUADs), AVIParser.hx:79-85."""
    _kind = N.JSP_CODEC_MSVIDEO1_8

    def __init__(self, width: int, height: int, palette: bytes, device: int = 0):
        super().__init__(width, height, 8, palette, device)


class ScreenPressor(_NativeCodec):
    """ScreenPressor.hx:19-490 — `new ScreenPressor(width, height, bits_per_pixel)`"""
    _kind = N.JSP_CODEC_SCREENPRESSOR

    SEEKS = False   # jsp_seek refuses it: sequential entropy stage, motion in inter frames
    FINDS_CHANGES = False   # jsp_find_change refuses it likewise
    INDEXES = False   # jsp_index_build refuses it likewise

    def __init__(self, width: int, height: int, bits_per_pixel: int, device: int = 0):
        super().__init__(width, height, bits_per_pixel, None, device)
        self.bpp = int(bits_per_pixel)

    def BuildScrubIndex(self, srcs: Sequence, is_key: Optional[Sequence[bool]] = None, key_row: int = INSIGNIFICANT_LINES) -> "SpScrubIndex":
        """The host entropy stage over the frames `srcs` ONCE (srcs[0] a coded key frame), its records kept in HBM
        (jsp_sp_index_build): SpScrubIndex.Show(t) then writes frame t's picture in one launch, with no host decode work.  The
        codec is only lent — its stream position, previous frame and entropy state stay as they are — and the index keeps no
        reference to `srcs`.  CodecError for a range that does not start at a coded key frame or holds a frame that does not
        decode (the error names it)."""
        n = len(srcs)
        if n == 0:
            raise CodecError("sp_index: empty range")
        ptrs, lens, keys, keeps = _range_args(srcs, is_key)
        h = self._lib.jsp_sp_index_build(self._h, n, ptrs, lens, keys, int(key_row))
        del keeps
        if not h:
            raise CodecError(N.last_error())
        return SpScrubIndex(self, h)


class SpScrubIndex(_IndexThumbs, _IndexPresent, _IndexTensor, _IndexActivity):
    """A ScreenPressor range resident in HBM (jsp_sp_index_build, via ScreenPressor.BuildScrubIndex): Show(t) is one launch,
    Play(first, dsts, stride) one launch for a run of frames played forward from any frame (jsp_sp_index_play),
    Thumbs(frames) one launch for any number of downscaled frames (jsp_sp_index_thumbs; _IndexThumbs has the two methods),
    Present(frames, ...) one launch for their windows of any size (jsp_sp_index_present; _IndexPresent),
    Tensor(frames, ...) one launch for the same windows as a model's input batch (jsp_sp_index_tensor; _IndexTensor),
    Activity(first, n) one launch for the changed pixels per frame and 16x16 block of a run (jsp_sp_index_activity; _IndexActivity),
    Distance(ref, first, n) one launch for the pixels per frame and block that differ from ONE reference picture (jsp_sp_index_distance).
    `significance` = the verdict the sequential run records for every frame, `frames`, `device_bytes`, `host_bytes`.  close() (or
    the context manager) frees it; safe after the codec is gone."""

    ADOPTS = False   # Show never moves the decoder: a Manager serves the frame and leaves its decode position where it is
    _THUMB_CALLS = ("sp_index_thumb_size", "sp_index_thumbs")
    _PRESENT_CALL = "sp_index_present"
    _TENSOR_CALL = "sp_index_tensor"
    _ACTIVITY_CALLS = ("sp_index_activity_size", "sp_index_activity")
    _DISTANCE_CALL = "sp_index_distance"

    def _present_mode(self) -> int:   # 16-bpp frames hold 5-bit components (Manager.hx:121), as Manager.present chooses it
        return 1 if getattr(self._codec, "bpp", 0) == 16 else 0   # DISPLAY_CANVAS_RGB15 / DISPLAY_CANVAS

    def __init__(self, codec: _NativeCodec, handle: int):
        self._codec, self._h = codec, handle
        lib = self._lib = codec._lib
        self._info()
        sig = (C.c_int * self.frames)()
        lib.jsp_sp_index_significance(handle, sig)
        self.significance = [bool(v) for v in sig]

    def _info(self) -> None:
        n, dev, host = C.c_int(0), C.c_uint64(0), C.c_uint64(0)
        self._lib.jsp_sp_index_info(self._h, C.byref(n), C.byref(dev), C.byref(host))
        self.frames, self.device_bytes, self.host_bytes = n.value, dev.value, host.value

    def Show(self, t: int, dst, adopt: bool = False) -> PFrameResult:
        """Frame t's picture into `dst` (a device buffer, not the codec's previous frame): what a fresh codec leaves as its
        previous frame after decoding srcs[:t + 1] in order.  Every pixel is written.  PFrameResult(dst, the frame's verdict).
        The codec is not touched (`adopt` must stay False: the entropy state after frame t is not in the index)."""
        if adopt:
            raise CodecError("sp_index_show: a ScreenPressor index cannot adopt")
        if not self._h:
            raise CodecError("sp_index_show: the index is closed")
        codec = self._codec
        if not codec._h:
            raise CodecError("sp_index_show: the codec is closed")
        addr = _frame_ptr(dst, codec.X * codec.Y)
        signif = C.c_int(0)
        if self._lib.jsp_sp_index_show(codec._h, self._h, int(t), C.c_void_p(addr), C.byref(signif)) != 0:
            raise CodecError(N.last_error())
        return PFrameResult(dst, bool(signif.value))

    def Play(self, first: int, dsts, stride: int = 1) -> list:
        """Frames first, first + stride, ... of the index, one per buffer of `dsts` (device buffers, all different, none the
        codec's previous frame): dsts[k] receives exactly what Show(first + k * stride) writes — ONE launch whatever len(dsts) and
        stride (jsp_sp_index_play): frame `first` is composed once and the pixels are carried forward in registers.  Returns a
        PFrameResult(dsts[k], the frame's verdict) per buffer.  The codec is not touched (it forgets the buffers' last columns, as
        after Show).  Reverse playback: the same call, the buffers shown in reverse."""
        codec = self._open("sp_index_play")
        dsts = list(dsts)
        n = len(dsts)
        ptrs = (C.c_void_p * max(n, 1))(*[_frame_ptr(d, codec.X * codec.Y) for d in dsts])
        signif = (C.c_int * max(n, 1))()
        if self._lib.jsp_sp_index_play(codec._h, self._h, int(first), n, int(stride), ptrs, signif) != 0:
            raise CodecError(N.last_error())
        self._info()   # (the first Play adds the per-frame table, a longer run a longer destination list)
        return [PFrameResult(d, bool(signif[k])) for k, d in enumerate(dsts)]

    def _open(self, who: str) -> _NativeCodec:
        if not self._h:
            raise CodecError(f"{who}: the index is closed")
        if not self._codec._h:
            raise CodecError(f"{who}: the codec is closed")
        return self._codec

    def close(self) -> None:
        if self._h:
            self._lib.jsp_sp_index_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _DeviceView:
    """npixels int32 at a device address, for torch.as_tensor (the CUDA array interface; ROCm builds of torch honour it)."""

    def __init__(self, ptr: int, npixels: int):
        self.__cuda_array_interface__ = {"shape": (npixels,), "typestr": "<i4", "data": (ptr, False), "version": 2}


class FramePool:
    """The frame buffers a caller decodes into (Manager.hx:114-118, hx/FrameBuffer.hx): jsp_pool_create.  `frames` are torch int32
    tensors over the pool's buffers (valid until close()).  A pool of 32 frames or more is one allocation that the library PLACES —
    it measures what candidate allocations take from the decode kernels' store shape and keeps a fast one (include/jsplayer_amd.h);
    `store_rate` (GB/s, 0 for small pools) and `attempts` say what it found."""

    def __init__(self, width: int, height: int, count: int, device: int = 0):
        import torch
        self._lib = N.lib()
        self._h = self._lib.jsp_pool_create(device, width, height, count)
        if not self._h:
            raise CodecError(N.last_error())
        tried = C.c_int(0)
        self.store_rate = float(self._lib.jsp_pool_store_rate(self._h, C.byref(tried)))
        self.attempts = tried.value
        ms, held, limit = C.c_double(0), C.c_uint64(0), C.c_uint64(0)
        self._lib.jsp_pool_probe_info(self._h, C.byref(ms), C.byref(held), C.byref(limit))
        self.probe_ms, self.held_bytes, self.hold_limit = ms.value, held.value, limit.value   # what placing the pool cost
        rates = (C.c_double * 64)()
        n = self._lib.jsp_pool_probe_rates(self._h, rates, 64)
        self.tried_rates = [float(rates[i]) for i in range(max(0, min(n, 64)))]             # GB/s of every candidate measured, in order
        n = width * height
        self.frames = [torch.as_tensor(_DeviceView(int(self._lib.jsp_pool_buffer(self._h, i)), n), device=f"cuda:{device}") for i in range(count)]

    def close(self) -> None:
        if self._h:
            self.frames = []
            self._lib.jsp_pool_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class HostBuffer:
    """Pinned host memory for compressed frames (jsp_host_alloc): uploads from it need no staging copy.  `.array` is a
    numpy uint8 view; frames handed to the *_async calls as slices of it are uploaded from where they are."""

    def __init__(self, nbytes: int):
        self._lib = N.lib()
        self._p = self._lib.jsp_host_alloc(max(int(nbytes), 1))
        if not self._p:
            raise CodecError("jsp_host_alloc failed")
        self.array = np.ctypeslib.as_array((C.c_uint8 * max(int(nbytes), 1)).from_address(self._p))

    def close(self) -> None:
        if self._p:
            self.array = None
            self._lib.jsp_host_free(self._p)
            self._p = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Msv1Encoder:
    """An MSVideo1 16-bit encoder for pictures of width x height in device memory (jsp_msv1_encoder_create; the rule:
    include/jsplayer_amd.h, "Encode").  No codec is involved; the pictures are only read."""

    def __init__(self, width: int, height: int, device: int = 0):
        self._lib = N.lib()
        self.width, self.height, self.device = int(width), int(height), int(device)
        self._h = self._lib.jsp_msv1_encoder_create(self.device, self.width, self.height)
        if not self._h:
            raise CodecError(N.last_error())

    def Bound(self) -> int:
        """The most bytes one frame has: 18 per 4x4 block."""
        if not self._h:
            raise CodecError("msv1_encode: the encoder is closed")
        n = C.c_size_t(0)
        if self._lib.jsp_msv1_encode_bound(self._h, C.byref(n)) != 0:
            raise CodecError(N.last_error())
        return n.value

    def _picture_ptr(self, buf, pitch: int):
        """The base of a picture: a device int32 tensor that starts at row 0 (pitch < 0: at the LAST row of a top-row-first window, the
        rows before it in memory being the caller's word), or a device address as an int."""
        if buf is None:
            return None
        if isinstance(buf, int):
            return buf
        need = (self.height - 1) * pitch + self.width if pitch > 0 else self.width
        return _device_frame_ptr(buf, max(need, 1), "msv1_encode")

    def EncodeFrames(self, pictures, previous=None, pitch: Optional[int] = None, stream: int = 0) -> list:
        """One frame per picture: a key frame where previous is None or previous[j] is None, else the inter frame that takes the
        decode of previous[j] to the decode of pictures[j] (blocks whose quantised pixels are equal are skipped).  `pitch`: ints
        from a row to the next, default the width; negative for a top-row-first window handed over by its last row.  Two launches
        per slice of pictures; returns synchronised.  Exact on every picture an MSVideo1 16-bit decoder produced."""
        if not self._h:
            raise CodecError("msv1_encode: the encoder is closed")
        pitch = self.width if pitch is None else int(pitch)
        pictures = list(pictures)
        n = len(pictures)
        if previous is not None and len(previous) != n:
            raise CodecError("msv1_encode: previous must have an entry per picture")
        pics = (C.c_void_p * max(n, 1))(*[self._picture_ptr(p, pitch) for p in pictures])
        prevs = (C.c_void_p * max(n, 1))(*[self._picture_ptr(p, pitch) for p in previous]) if previous is not None else None
        lens = (C.c_size_t * max(n, 1))()
        total = C.c_size_t(0)
        call = lambda out, room: self._lib.jsp_msv1_encode_frames(self._h, n, pics, prevs, pitch, out, room, lens, C.byref(total),
                                                                  C.c_void_p(stream) if stream else None)
        cap = max(n, 1) * self.Bound()
        if cap > DELTA_ASK_TWICE:   # many large frames: the lengths first (cap 0 is the refusal that still sets them), then the bytes
            if call(None, 0) == 0 or total.value == 0:
                raise CodecError(N.last_error())
            cap = total.value
        buf = (C.c_uint8 * max(cap, 1))()
        if call(buf, len(buf)) != 0:
            raise CodecError(N.last_error())
        view, out, at = memoryview(buf), [], 0
        for j in range(n):
            out.append(bytes(view[at:at + lens[j]]))
            at += lens[j]
        return out

    def close(self) -> None:
        if self._h:
            self._lib.jsp_msv1_encoder_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---- the two Manager passes that follow the codec (Manager.hx:325-390, 413-419), on the GPU --------
DISPLAY_CANVAS, DISPLAY_CANVAS_RGB15, DISPLAY_SETPIXELS, DISPLAY_SETPIXELS_RGB15 = 0, 1, 2, 3


def display_convert(frame, out, width: int, height: int, mode: int = DISPLAY_CANVAS, flip_rows: bool = False,
                    stream: int = 0) -> None:
    """Manager.fill_bitmap_data on device tensors (int32, width*height; width and height 1 .. 65535).  `out` may be `frame` itself
    when flip_rows is false."""
    src, dst = _device_frame_ptr(frame, width * height, "display_convert"), _device_frame_ptr(out, width * height, "display_convert")
    lib = N.lib()
    rc = lib.jsp_display_convert(C.c_void_p(src), C.c_void_p(dst),
                                 width, height, mode, 1 if flip_rows else 0, C.c_void_p(stream) if stream else None)
    if rc != 0:
        raise CodecError(N.last_error())


# ---- a frame in a window: Main's view geometry and the browser's resampling (Main.hx:288-319, 948), one launch ----
PRESENT_NEAREST, PRESENT_BILINEAR = 0, 1
PRESENT_AREA = 2          # the area average: display_present_area's rule (display_present itself refuses it); Manager.present routes it
# what one workgroup of the present kernel covers (csrc/present_kernels.hip: kPresentSpanX, kPresentBandRows); results do not depend on it
PRESENT_SPAN_X, PRESENT_BAND_ROWS = 256, 8
# the same of the area kernel (csrc/present_area_kernels.hip: kAreaLanes — a lane owns one pixel —, kAreaBandRows)
PRESENT_AREA_SPAN_X, PRESENT_AREA_BAND_ROWS = 64, 1


def view_matrix(frame_w: int, frame_h: int, win_w: int, win_h: int, zoom: float = 0.0, hor_view_pos: float = 0.5,
                ver_view_pos: float = 0.5):
    """Main.on_stage_resize's display matrix (Main.hx:301-315) -> (k, dx, dy): zoom 0 is "Fit", a positive zoom is the factor with
    the window centred by the two view positions.  Host arithmetic; needs no GPU."""
    k, dx, dy = C.c_double(0), C.c_double(0), C.c_double(0)
    rc = N.lib().jsp_view_matrix(int(frame_w), int(frame_h), int(win_w), int(win_h), float(zoom), float(hor_view_pos),
                                 float(ver_view_pos), C.byref(k), C.byref(dx), C.byref(dy))
    if rc != 0:
        raise CodecError(N.last_error())
    return k.value, dx.value, dy.value


def display_present(frame, frame_w: int, frame_h: int, out, win_w: int, win_h: int, k: float, dx: float, dy: float,
                    mode: int = DISPLAY_CANVAS, filter: int = PRESENT_BILINEAR, background: int = 0xFF000000,
                    out_pitch: Optional[int] = None, stream: int = 0) -> None:
    """The win_w x win_h window onto `frame` (a device frame buffer, bottom-up) under the display matrix (k, dx, dy), as canvas
    pixels, top row first, into the device tensor `out` (row pitch `out_pitch` ints, default win_w): conversion by `mode`, row
    flip, crop and resampling in one launch on `stream`, asynchronous."""
    pitch = int(win_w) if out_pitch is None else int(out_pitch)
    need = max((int(win_h) - 1) * pitch + int(win_w), 1)
    src = _device_frame_ptr(frame, max(int(frame_w) * int(frame_h), 1), "display_present")
    dst = _device_frame_ptr(out, need, "display_present")
    lib = N.lib()
    rc = lib.jsp_display_present(C.c_void_p(src), int(frame_w), int(frame_h),
                                 C.c_void_p(dst), int(win_w), int(win_h), C.c_size_t(max(pitch, 0)),
                                 float(k), float(dx), float(dy), int(mode), int(filter), C.c_uint32(int(background) & 0xFFFFFFFF),
                                 C.c_void_p(stream) if stream else None)
    if rc != 0:
        raise CodecError(N.last_error())


def display_present_area(frame, frame_w: int, frame_h: int, out, win_w: int, win_h: int, k: float, dx: float, dy: float,
                         mode: int = DISPLAY_CANVAS, background: int = 0xFF000000, out_pitch: Optional[int] = None,
                         stream: int = 0) -> None:
    """display_present's window with every covered pixel the area average of the converted source pixels under it (the rule of
    jsp_display_present_area): what Fit of a large picture into a small window needs.  Same arguments, no filter; one launch on
    `stream`, asynchronous."""
    pitch = int(win_w) if out_pitch is None else int(out_pitch)
    need = max((int(win_h) - 1) * pitch + int(win_w), 1)
    src = _device_frame_ptr(frame, max(int(frame_w) * int(frame_h), 1), "display_present_area")
    dst = _device_frame_ptr(out, need, "display_present_area")
    lib = N.lib()
    rc = lib.jsp_display_present_area(C.c_void_p(src), int(frame_w), int(frame_h),
                                      C.c_void_p(dst), int(win_w), int(win_h), C.c_size_t(max(pitch, 0)),
                                      float(k), float(dx), float(dy), int(mode), C.c_uint32(int(background) & 0xFFFFFFFF),
                                      C.c_void_p(stream) if stream else None)
    if rc != 0:
        raise CodecError(N.last_error())


def frames_differ(a, b, first_pixel: int, npixels: int, stream: int = 0) -> bool:
    """The pixel compare of Manager.frames_differ_significantly on device tensors: any a[i] != b[i] for first_pixel <= i < npixels."""
    first_pixel, npixels = int(first_pixel), int(npixels)
    if first_pixel < 0 or npixels < 0:
        raise CodecError(f"frames_differ: first_pixel and npixels must not be negative (got {first_pixel}, {npixels})")
    pa, pb = _device_frame_ptr(a, npixels, "frames_differ"), _device_frame_ptr(b, npixels, "frames_differ")
    lib = N.lib()
    out = C.c_int(0)
    rc = lib.jsp_frames_differ(C.c_void_p(pa), C.c_void_p(pb), first_pixel, npixels,
                               C.byref(out), C.c_void_p(stream) if stream else None)
    if rc != 0:
        raise CodecError(N.last_error())
    return bool(out.value)
