"""Manager.worker-equivalent decode loop: the direct caller of the plugin surface,
kept to what touches the codec — construction from VideoInfo (Manager.hx:103-142), the frame-buffer
pool that never hands out the buffer holding the previous frame (:424-443,470-477), the
DecompressI / DecompressP protocol with its identity test (:499-524) and
`frames_differ_significantly` for key frames (:392-421), and the seek branch of
`GetDecompressedFrame` (:216-259; `Manager.seek`, `nearest_key_frame` = DataLoader.hx:125-132): a held
frame is shown as it is, a seek outside the stretch being decoded trashes every buffer and starts again
at the nearest key frame, and the frames up to the target go to the decoder's `Seek` (MSVideo1 on the
GPU: one call, one launch) or, for decoders without one (ScreenPressor, the oracle's classes), through
`worker` frame by frame as the reference does.  `Manager.skip_stills` is SkipStills (:289-317) over
DataLoader.FindPossibleChange (DataLoader.hx:239-252) plus the SeekTo that Main.play_timer does with its
answer: significance already known is used as it is, and the frames nobody has judged go to the
decoder's `FindChange` (MSVideo1 on the GPU: one call) or through `worker` frame by frame.  With a seek index
attached (`Manager.attach_index`: a range kept resident by the decoder's `BuildIndex`), a seek inside it is one
`Show` launch and its frames' significance is known without decoding (an index that cannot leave the decoder at the frame
shown — ScreenPressor's, `ADOPTS` false — serves the frame and leaves the decode position where it is); `next_frame` / `prev_frame` / `next_key` /
`prev_key` are the navigation of Manager.hx:184-208 over `seek`; `play_from_index` plays a run of frames out of such a non-adopting
index, one `Play` launch per batch of free buffers; `preview` / `filmstrip` are the seek bar's small pictures, one
`Thumbs` launch of the attached index of either codec (SeekIndex or SpScrubIndex); `activity` / `change_totals` / `change_box` /
`next_change` say where and when the picture changes, from the index's `Activity` map (changed pixels per frame and 16x16 cell);
`distance` / `distance_totals` / `find_picture` / `repeats_of` / `distinct_frames` say how far each frame is from ONE picture, from
the index's `Distance` map (pixels per frame and cell that differ from a reference frame or device picture);
`cut` / `write_cut` give the clip from any frame on as frames and flags / as an AVI file, its first frame the index's `KeyFrame`;
`thin` / `write_thin` the clip made of any ascending list of frames, the gaps spanned by the index's `DeltaFrames`.  `crop_rect` / `crop` / `write_crop`
the same list of frames for a part of the picture, from the index's `CropFrames`; `follow` / `pan` / `write_pan` for a part that follows what
changes, from `activity` and the index's `PanFrames`; `transcode` / `write_transcode` the pictures of any frames of an index of either codec as a 16-bit MSVideo1
clip, made by the encoder (`Msv1Encoder`), `proxy` / `write_proxy` the same of their windows.  `View` is the zoom / scroll / fit state of Main
(Main.hx:288-319, 1186-1278) and `Manager.present` draws the window it shows of a frame buffer, one launch.  Timers, bitmaps and audio
of the reference's Manager are not rebuilt.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Callable, Dict, List, Optional, Sequence

import numpy as np

from .avi import CODEC_MSVC16, CODEC_MSVC8, CODEC_SCREENPRESSOR, VideoInfo

INSIGNIFICANT_LINES = 36  # Manager.hx:61
NUM_BUFFERS = 8           # Main.hx:148 (the pool holds NUM_BUFFERS + 1 frames, Manager.hx:114-118)
PRESENT_AREA = 2          # codec.PRESENT_AREA (JSP_PRESENT_AREA): the default filter of Manager.proxy


@dataclass
class DecodedFrame:
    index: int
    key: bool
    buffer_index: int            # pool slot holding the picture shown for this frame
    significant_changes: Optional[bool]
    state: int = 0               # DecoderState of a key frame


def make_decoder(vi: VideoInfo, classes) -> object:
    """`classes` = (MSVideo1_16bit, MSVideo1_8bit, ScreenPressor) — the HIP codecs or the oracle's."""
    m16, m8, sp = classes
    if vi.codec == CODEC_SCREENPRESSOR:
        return sp(vi.X, vi.Y, vi.bpp)
    if vi.codec == CODEC_MSVC16:
        return m16(vi.X, vi.Y)
    if vi.codec == CODEC_MSVC8:
        return m8(vi.X, vi.Y, vi.palette or b"")
    raise ValueError(vi.codec)


def nearest_key_frame(key_flags, n: int, count: Optional[int] = None) -> int:
    """DataLoader.GetNearestKeyframe (DataLoader.hx:125-132): `n` clamped to the last frame, then walked back to the
    nearest frame flagged key (frame 0 when none is).  `key_flags`: a sequence of flags (None or a missing entry = not
    key), or a callable index -> bool together with `count` frames."""
    if callable(key_flags):
        total = int(count or 0)
        flag = key_flags
    else:
        total = len(key_flags) if count is None else int(count)
        flag = lambda i: i < len(key_flags) and bool(key_flags[i])
    if total <= 0:
        return 0
    n = min(max(int(n), 0), total - 1)
    while n > 0 and not flag(n):
        n -= 1
    return n


def _differ(a, b, start: int) -> bool:
    if isinstance(a, np.ndarray):
        return bool(np.any(a[start:] != b[start:]))
    from .codec import frames_differ   # device tensors: HIP reduction, the frames stay in HBM
    return frames_differ(a, b, start, a.numel())


def _takes_tight(method) -> bool:
    """Whether an index object's DeltaFrames has the keyword `tight` (or takes any keyword)."""
    import inspect
    try:
        params = inspect.signature(method).parameters.values()
    except (TypeError, ValueError):
        return False
    return any(p.name == "tight" or p.kind is p.VAR_KEYWORD for p in params)


class View:
    """What Main keeps about the part of the picture a window shows: `zoom_index` into ZOOM_FACTORS ("Fit", "100%", "200%",
    Main.hx:170-171) and the two view positions in 0..1.  The slider drawing (calc_slider_handles) is not rebuilt."""

    ZOOM_FACTORS = (0, 1, 2)

    def __init__(self):
        self.zoom_index = 0
        self.hor_view_pos = 0.5
        self.ver_view_pos = 0.5

    @staticmethod
    def _fit(a: float, mn: float, mx: float) -> float:   # Main.hx:282-286
        if a < mn:
            return mn
        if a > mx:
            return mx
        return a

    def zoom_in(self) -> None:                            # on_zoomin, Main.hx:1257-1263
        if self.zoom_index < len(self.ZOOM_FACTORS) - 1:
            self.zoom_index += 1

    def zoom_out(self) -> None:                           # on_zoomout, :1264-1271
        if self.zoom_index > 0:
            self.zoom_index -= 1

    def zoom_fit(self) -> None:                           # on_zoomfit, :1272-1278
        self.zoom_index = 0

    def scroll(self, hor: bool, pos: float) -> None:      # Main.hx:1234-1239; pos in 0..1
        if hor:
            self.hor_view_pos = pos
        else:
            self.ver_view_pos = pos

    def key(self, code: int) -> None:
        """on_key_down (Main.hx:1186-1193): the arrow keys move the view by a tenth, clamped to 0..1; nothing happens in Fit."""
        if self.zoom_index == 0:
            return
        if code == 37:
            self.scroll(True, self._fit(self.hor_view_pos - 0.1, 0, 1))     # left
        elif code == 38:
            self.scroll(False, self._fit(self.ver_view_pos - 0.1, 0, 1))    # up
        elif code == 39:
            self.scroll(True, self._fit(self.hor_view_pos + 0.1, 0, 1))     # right
        elif code == 40:
            self.scroll(False, self._fit(self.ver_view_pos + 0.1, 0, 1))    # down

    def matrix(self, frame_w: int, frame_h: int, win_w: int, win_h: int):
        """(k, dx, dy) of the display matrix for the current state (Main.hx:301-315, jsp_view_matrix)."""
        from .codec import view_matrix
        return view_matrix(frame_w, frame_h, win_w, win_h, self.ZOOM_FACTORS[self.zoom_index], self.hor_view_pos, self.ver_view_pos)


class Manager:
    """Feeds compressed frames to an IVideoCodec in order, with the reference's buffer discipline."""

    def __init__(self, vi: VideoInfo, decoder, alloc: Callable[[int], object], num_buffers: int = NUM_BUFFERS):
        self.vi, self.decoder = vi, decoder
        self.buffers = [alloc(vi.X * vi.Y) for _ in range(num_buffers + 1)]
        self.holds: List[Optional[range]] = [None] * len(self.buffers)  # frames each slot currently shows
        self.decoder.Preinit(INSIGNIFICANT_LINES)
        # HIP codecs compare a key frame with the frame before it while they decode it (option "key_frame_compare"): no pass of the
        # Manager's own over the two frames (Manager.hx:413-419)
        self._fused_compare = hasattr(self.decoder, "KeyFrameDiffers")
        if self._fused_compare:
            self.decoder.set_option("key_frame_compare", str(INSIGNIFICANT_LINES))
        self.next_frame_to_decode = 0
        self.frame_of_interest = 0
        self.log: List[DecodedFrame] = []
        self.judged: Dict[int, bool] = {}   # significance of frames a FindChange call judged (skip_stills)
        self.index = None                   # attach_index: a seek index over clip frames index_first .. index_first + index.frames - 1
        self.index_first = 0
        self.view = View()                  # zoom and view positions of the window present() draws (Main.hx:288-319)

    def present(self, buf, out, win_w: int, win_h: int, filter: Optional[int] = None, background: int = 0xFF000000, stream: int = 0) -> None:
        """The window `self.view` shows of one of this Manager's frame buffers (`buf`: the buffer, or its slot number), as canvas
        pixels, top row first, into the device tensor `out` (win_w * win_h ints): one launch (jsp_display_present, or
        jsp_display_present_area for filter = PRESENT_AREA), the frame stays in HBM.  The conversion is chosen as Manager.hx:121 chooses convert_fromRGB15: 16-bpp ScreenPressor frames hold 5-bit
        components.  `filter` defaults to bilinear (bitmap.smoothing = true, Main.hx:948).  HIP frame buffers only."""
        from .codec import DISPLAY_CANVAS, DISPLAY_CANVAS_RGB15, PRESENT_AREA, PRESENT_BILINEAR, display_present, display_present_area
        if isinstance(buf, (int, np.integer)):
            buf = self.buffers[int(buf)]
        elif self._slot_of(buf) < 0:
            raise ValueError("present: not one of this Manager's frame buffers")
        from_rgb15 = self.vi.bpp == 16 and self.vi.codec == CODEC_SCREENPRESSOR
        k, dx, dy = self.view.matrix(self.vi.X, self.vi.Y, win_w, win_h)
        if filter == PRESENT_AREA:
            display_present_area(buf, self.vi.X, self.vi.Y, out, win_w, win_h, k, dx, dy,
                                 mode=DISPLAY_CANVAS_RGB15 if from_rgb15 else DISPLAY_CANVAS, background=background, stream=stream)
            return
        display_present(buf, self.vi.X, self.vi.Y, out, win_w, win_h, k, dx, dy,
                        mode=DISPLAY_CANVAS_RGB15 if from_rgb15 else DISPLAY_CANVAS,
                        filter=PRESENT_BILINEAR if filter is None else filter, background=background, stream=stream)

    def attach_index(self, index, first: int = 0) -> None:
        """Serve seeks to clip frames first .. first + index.frames - 1 from `index` (the decoder's BuildIndex over those frames,
        built where the decoder's state was that of frame first - 1 — typically from a key frame): one Show launch each, and the
        index's significance verdicts count as known.  None detaches.  An index whose `ADOPTS` is false (ScreenPressor's
        BuildScrubIndex) shows pictures without moving the decoder: a frame inside it is served before the decode position is
        touched, and decoding continues later from where the decoder really stands."""
        self.index, self.index_first = index, int(first)
        self._activity = None   # (the map belongs to the index it was computed from)
        self._distance = None   # (the distance maps too: per reference frame of the index)

    _activity = None
    _distance = None

    # -- where and when the picture changes: the attached index's activity map (jsp_index_activity / jsp_sp_index_activity) ----------
    def activity(self):
        """The activity map of the whole attached index: [frame of the index, grid row, grid column] -> pixels of that 16 x 16 cell
        the frame changed, grid rows in the frame's own bottom-up order (the index's `Activity`: one launch per 4096 frames, no
        picture written, the decoder not touched).  Computed once per attach_index and kept where the index puts it (on the device);
        attach_index drops it.  No index attached, or an index object without `Activity`: ValueError."""
        if self.index is None:
            raise ValueError("no seek index attached")
        if not hasattr(self.index, "Activity"):
            raise ValueError("the attached seek index has no activity map")
        if self._activity is None:
            self._activity = self.index.Activity()
        return self._activity

    @staticmethod
    def _frame_sums(cells) -> np.ndarray:
        """Per frame, the sum of the cells of a [frames, rows, cols] part of the map, on the host (int64)."""
        if isinstance(cells, np.ndarray):
            return cells.astype(np.int64).sum(axis=(1, 2))
        import torch
        return cells.to(torch.int64).sum(dim=(1, 2)).cpu().numpy()

    def change_totals(self) -> List[int]:
        """Changed pixels per frame of the attached index (entry k: clip frame index_first + k): the seek bar's activity strip."""
        return [int(v) for v in self._frame_sums(self.activity())]

    def change_box(self, i: int):
        """(x, y, w, h) of what clip frame `i` changed, in display coordinates (top row first; the map is in stored bottom-up
        order, so display row = H - 1 - stored row), clipped to the picture: the union of the frame's non-zero 16 x 16 cells — CELL
        granularity, a superset of the changed pixels.  None for a frame that changes nothing.  `i` outside the index: ValueError."""
        if not self._in_index(i):
            raise ValueError(f"frame {i} is not in an attached seek index")
        cells = self.activity()[i - self.index_first]
        cells = cells if isinstance(cells, np.ndarray) else cells.cpu().numpy()
        rs, qs = np.nonzero(cells)
        if rs.size == 0:
            return None
        W, H = self.vi.X, self.vi.Y
        x0, x1 = int(qs.min()) * 16, min((int(qs.max()) + 1) * 16, W)
        y0, y1 = int(rs.min()) * 16, min((int(rs.max()) + 1) * 16, H)   # stored rows y0 .. y1 - 1
        return x0, H - y1, x1 - x0, y1 - y0

    def next_change(self, frames: Sequence[bytes], rect=None, min_pixels: int = 1, key_flags: Optional[Sequence[bool]] = None):
        """Show the first frame after `frame_of_interest`, inside the attached index, that changes at least `min_pixels` pixels of
        `rect` = (x, y, w, h) in display coordinates (top row first; None: the whole picture) — "skip idle" for the part of the
        picture in view.  Whole 16 x 16 cells are summed: every cell `rect` intersects counts in full, so a SUPERSET of `rect` is
        judged.  The frame is shown through seek(), exactly as skip_stills shows a known change, and its DecodedFrame returned;
        None, and nothing shown, when no such frame is left in the index (or `rect` lies outside the picture)."""
        act = self.activity()
        W, H = self.vi.X, self.vi.Y
        if rect is None:
            rect = (0, 0, W, H)
        x, y, w, h = (int(v) for v in rect)
        x0, x1 = max(x, 0), min(x + w, W)
        s0, s1 = max(H - (y + h), 0), min(H - y, H)          # stored rows s0 .. s1 - 1
        k0 = max(self.frame_of_interest + 1 - self.index_first, 0)
        if x0 >= x1 or s0 >= s1 or k0 >= self.index.frames:
            return None
        sums = self._frame_sums(act[k0:, s0 // 16:(s1 + 15) // 16, x0 // 16:(x1 + 15) // 16])
        hits = np.nonzero(sums >= int(min_pixels))[0]
        if hits.size == 0:
            return None
        return self.seek(frames, self.index_first + k0 + int(hits[0]), key_flags)

    # -- how far each frame is from ONE picture: the attached index's distance map (jsp_index_distance / jsp_sp_index_distance) ---------
    def _need_distance(self) -> None:
        if self.index is None:
            raise ValueError("no seek index attached")
        if not hasattr(self.index, "Distance"):
            raise ValueError("the attached seek index has no distance map")

    def _ref_of(self, ref):
        """`ref` as the index's Distance takes it: a clip frame number index_first - 1 .. index_first + frames - 1 becomes a frame of
        the index (-1: the picture before it); a device tensor / frame buffer passes through."""
        self._need_distance()
        if hasattr(ref, "data_ptr"):
            return ref
        t = int(ref) - self.index_first
        if not -1 <= t < self.index.frames:
            raise ValueError(f"frame {int(ref)} is neither in the attached seek index nor the frame before it")
        return t

    def distance(self, ref):
        """The distance map of the whole attached index against ONE reference picture: [frame of the index, grid row, grid column]
        -> pixels of that 16 x 16 cell that differ from the reference, on Activity's grid (the index's `Distance`: one launch per
        4096 frames, no picture written, the decoder not touched).  `ref` is a clip frame number, index_first - 1 (the picture before
        the index) .. the index's last frame, or a device tensor / frame buffer.  The map of a frame number is computed once and
        kept where the index puts it; attach_index drops them all (a tensor's map is computed at every call: its pixels may have
        changed).  No index attached, an index object without `Distance`, a frame outside the range: ValueError."""
        r = self._ref_of(ref)
        if not isinstance(r, int):
            return self.index.Distance(r)
        if self._distance is None:
            self._distance = {}
        if r not in self._distance:
            self._distance[r] = self.index.Distance(r)
        return self._distance[r]

    def _rect_cells(self, rect):
        """(row slice, column slice) of the cells the display rectangle `rect` intersects (next_change's rule: top row first, every
        cell it touches counts in full); None when nothing of it lies inside the picture.  rect None: the whole grid."""
        W, H = self.vi.X, self.vi.Y
        if rect is None:
            return slice(None), slice(None)
        x, y, w, h = (int(v) for v in rect)
        x0, x1 = max(x, 0), min(x + w, W)
        s0, s1 = max(H - (y + h), 0), min(H - y, H)          # stored rows s0 .. s1 - 1
        if x0 >= x1 or s0 >= s1:
            return None
        return slice(s0 // 16, (s1 + 15) // 16), slice(x0 // 16, (x1 + 15) // 16)

    def distance_totals(self, ref, rect=None) -> List[int]:
        """Pixels per frame of the attached index (entry k: clip frame index_first + k) that differ from the reference `ref`
        (see distance).  rect = (x, y, w, h) in display coordinates: summed over the 16 x 16 cells it intersects, each in full, as
        next_change does (a rectangle outside the picture: all zeros)."""
        cells = self.distance(ref)
        at = self._rect_cells(rect)
        if at is None:
            return [0] * self.index.frames
        return [int(v) for v in self._frame_sums(cells[:, at[0], at[1]])]

    def find_picture(self, ref, max_pixels: int = 0, rect=None) -> List[int]:
        """The clip frames of the attached index, ascending, that differ from the reference `ref` (see distance) by at most
        `max_pixels` pixels — of `rect` when one is given (distance_totals): where else the recording shows this picture, which
        frame looks like this screenshot.  A frame of the index as `ref` is in the list itself."""
        totals = self.distance_totals(ref, rect)
        return [self.index_first + k for k, v in enumerate(totals) if v <= int(max_pixels)]

    def repeats_of(self, i: int) -> List[int]:
        """The other frames of the attached index that show exactly the picture of clip frame `i`: find_picture(i) without i."""
        return [k for k in self.find_picture(int(i)) if k != int(i)]

    def distinct_frames(self, min_pixels: int, first: Optional[int] = None, count: Optional[int] = None) -> List[int]:
        """A `keep` list for thin / crop / sequence: the frames of clip frames first .. first + count - 1 (None: from the index's
        first frame / to its last) that are worth keeping.  The first frame is kept; then the next frame that differs from the LAST
        KEPT frame by at least `min_pixels` pixels, and so on — one `Distance` call per kept frame, over the frames still ahead of
        it; the last frame of the range is always kept.  Strictly ascending.  These calls cover a part of the index each and go to
        the index directly: they neither use nor fill the maps `distance` keeps.  ValueError: no index attached, an index object
        without `Distance`, an empty range or one outside the index."""
        self._need_distance()
        first = self.index_first if first is None else int(first)
        end = self.index_first + self.index.frames if count is None else first + int(count)   # one past the range
        if not (self._in_index(first) and first < end <= self.index_first + self.index.frames):
            raise ValueError(f"distinct_frames: frames {first} .. {end - 1} are not a range of the attached seek index")
        keep = [first]
        while keep[-1] < end - 1:
            at = keep[-1]
            ahead = self.index.Distance(at - self.index_first, at + 1 - self.index_first, end - 1 - at)
            hits = np.nonzero(self._frame_sums(ahead) >= int(min_pixels))[0]
            keep.append(at + 1 + int(hits[0]) if hits.size else end - 1)
        return keep

    # -- a clip that starts at any frame: the attached index's KeyFrame (jsp_index_key_frame) ------------------------------------------
    def cut(self, frames: Sequence[bytes], first: int, last: Optional[int] = None, key_flags: Optional[Sequence[bool]] = None):
        """Clip frames first .. last (None: to the end), as a clip of its own: (list of frame bytes, key flags).  A clip has to start
        on a key frame.  Where frame `first` is one — by `key_flags`, else frame 0 or the decoder's IsKeyFrame — it is taken as it
        is and no index is needed.  Else the attached index must contain `first`, and the first frame of the result is
        index.KeyFrame(first - index_first): a key frame that decodes to the picture of frame `first`, made of the codes the index
        holds (a frame the index cannot cut raises its CodecError).  The frames after it are the caller's own objects and keep
        their flags; the first flag is True.  Nothing is decoded and neither decoder nor buffers change.  ValueError: `first`
        outside the clip or last < first; at an inter frame, no index attached, `first` outside it, or an index object without
        `KeyFrame` (ScreenPressor's)."""
        first = int(first)
        last = len(frames) - 1 if last is None else int(last)
        if not 0 <= first < len(frames):
            raise ValueError(f"cut: frame {first} is not in the clip")
        if last < first:
            raise ValueError(f"cut: last ({last}) is before first ({first})")
        last = min(last, len(frames) - 1)
        tail = list(frames[first + 1:last + 1])
        flags = [True] + [bool(key_flags[i]) if key_flags is not None else bool(self.decoder.IsKeyFrame(frames[i]))
                          for i in range(first + 1, last + 1)]
        if self._key_at(frames, first, key_flags):
            return [frames[first]] + tail, flags
        if self.index is None:
            raise ValueError(f"cut: frame {first} is not a key frame and no seek index is attached")
        if not self._in_index(first):
            raise ValueError(f"cut: frame {first} is not a key frame and not in the attached seek index")
        if not hasattr(self.index, "KeyFrame"):
            raise ValueError("cut: the attached seek index cannot make a key frame")
        return [self.index.KeyFrame(first - self.index_first)] + tail, flags

    def write_cut(self, frames: Sequence[bytes], first: int, last: Optional[int] = None, key_flags: Optional[Sequence[bool]] = None,
                  fps: float = 15.0) -> bytes:
        """`cut` as an AVI file (avi.write_avi) with this Manager's stream: width, height, bit depth and palette of its VideoInfo,
        fourcc CRAM for MSVideo1 and SCPR for ScreenPressor."""
        from .avi import write_avi
        out, flags = self.cut(frames, first, last, key_flags)
        fourcc = b"SCPR" if self.vi.codec == CODEC_SCREENPRESSOR else b"CRAM"
        return write_avi(self.vi.X, self.vi.Y, out, fourcc=fourcc, bpp=self.vi.bpp, fps=fps, palette=self.vi.palette, key_flags=flags)

    # -- a clip thinned to the frames worth keeping: the attached index's DeltaFrames (jsp_index_delta_frames) -----------------------------
    def thin(self, frames: Sequence[bytes], keep: Sequence[int], key_flags: Optional[Sequence[bool]] = None, tight: bool = False):
        """The clip's frames `keep` (strictly ascending frame numbers) as a clip of its own: (list of frame bytes, key flags) — a
        time-lapse (every s-th frame), a recording without its idle frames (`change_totals`), any list.  Entry 0 follows `cut`: the
        frame itself where it is a key frame, else index.KeyFrame.  A later entry that is a key frame of the clip is copied; one
        that follows its predecessor directly (keep[k] == keep[k - 1] + 1) is the caller's own object; every other one is
        index.DeltaFrames' inter frame from the picture of keep[k - 1] to the picture of keep[k], all of them from ONE call.
        Flags: True for entry 0 and the copied key frames, else the decoder's IsKeyFrame of the bytes.  Nothing is decoded and
        neither decoder nor buffers change; a gap the index cannot span raises its CodecError.  ValueError: `keep` empty, not
        strictly ascending or outside the clip; where the index is needed, none attached, a frame outside it, or an index object
        without `KeyFrame` / `DeltaFrames` (ScreenPressor's).  tight: the one DeltaFrames call is made with tight=True (blocks whose
        pixels a gap did not change are dropped from its frames); everything else is the same.  ValueError as well when the index's
        DeltaFrames takes no `tight`."""
        keep = [int(k) for k in keep]
        if not keep:
            raise ValueError("thin: keep is empty")
        for k in keep:
            if not 0 <= k < len(frames):
                raise ValueError(f"thin: frame {k} is not in the clip")
        for prev, k in zip(keep, keep[1:]):
            if k <= prev:
                raise ValueError(f"thin: keep is not strictly ascending ({k} after {prev})")
        is_key = [self._key_at(frames, k, key_flags) for k in keep]
        gaps = [j for j in range(1, len(keep)) if not is_key[j] and keep[j] != keep[j - 1] + 1]
        need_key = not is_key[0]
        if need_key or gaps:
            if self.index is None:
                raise ValueError("thin: no seek index is attached")
            wanted = ([keep[0]] if need_key else []) + [keep[j] for j in gaps]
            for k in wanted:
                if not self._in_index(k):
                    raise ValueError(f"thin: frame {k} is not in the attached seek index")
            for j in gaps:   # (the gap may start on the frame before the index: its picture is the one before the range)
                if keep[j - 1] < self.index_first - 1:
                    raise ValueError(f"thin: frame {keep[j - 1]} is not in the attached seek index")
            if need_key and not hasattr(self.index, "KeyFrame"):
                raise ValueError("thin: the attached seek index cannot make a key frame")
            if gaps and not hasattr(self.index, "DeltaFrames"):
                raise ValueError("thin: the attached seek index cannot span a gap")
            if gaps and tight and not _takes_tight(self.index.DeltaFrames):
                raise ValueError("thin: the attached seek index cannot span a gap tightly")
        out = [frames[k] for k in keep]
        if need_key:
            out[0] = self.index.KeyFrame(keep[0] - self.index_first)
        if gaps:
            pairs = [(keep[j - 1] - self.index_first, keep[j] - self.index_first) for j in gaps]
            made = self.index.DeltaFrames(pairs, tight=True) if tight else self.index.DeltaFrames(pairs)
            for j, data in zip(gaps, made):
                out[j] = data
        flags = [True] + [True if is_key[j] else bool(self.decoder.IsKeyFrame(out[j])) for j in range(1, len(keep))]
        return out, flags

    def write_thin(self, frames: Sequence[bytes], keep: Sequence[int], key_flags: Optional[Sequence[bool]] = None, fps: float = 15.0,
                   tight: bool = False) -> bytes:
        """`thin` as an AVI file (avi.write_avi) with this Manager's stream, as `write_cut` writes `cut`."""
        from .avi import write_avi
        out, flags = self.thin(frames, keep, key_flags, tight=tight)
        fourcc = b"SCPR" if self.vi.codec == CODEC_SCREENPRESSOR else b"CRAM"
        return write_avi(self.vi.X, self.vi.Y, out, fourcc=fourcc, bpp=self.vi.bpp, fps=fps, palette=self.vi.palette, key_flags=flags)

    # -- a clip of pictures that exist only as pixels: the MSVideo1 encoder (jsp_msv1_encode_frames) ----------------------------------------
    def _transcode_frames(self, who: str, keep: Sequence[int]) -> List[int]:
        """`keep` as frame numbers of the attached index, checked: what transcode and proxy refuse alike."""
        keep = [int(k) for k in keep]
        if not keep:
            raise ValueError(f"{who}: keep is empty")
        if self.index is None:
            raise ValueError(f"{who}: no seek index is attached")
        if self.vi.codec == CODEC_SCREENPRESSOR and self.vi.bpp == 16:
            raise ValueError(f"{who}: a 16-bpp ScreenPressor index holds 5-bit components, not 0x00RRGGBB words")
        for k in keep:
            if not self._in_index(k):
                raise ValueError(f"{who}: frame {k} is not in the attached seek index")
        return [k - self.index_first for k in keep]

    def transcode(self, keep: Sequence[int]):
        """The pictures of clip frames `keep` (any order, repeats allowed) of the attached index — MSVideo1's or ScreenPressor's
        alike — as a 16-bit MSVideo1 clip of its own: (list of frame bytes, key flags).  The pictures are shown into device buffers
        of this call's own, as many as the Manager's pool has, a run at a time (index.Show, the decoder not touched), and each is
        encoded against the one before it (Msv1Encoder: two launches per slice of a run); the first is a key frame and the only one
        flagged.  Exact for an MSVideo1 16-bit index; for any other the pinned rule of the encoder (include/jsplayer_amd.h,
        "Encode").  Neither decoder nor the Manager's buffers change.  ValueError: `keep` empty, no index attached, a frame outside
        it, a 16-bpp ScreenPressor index (its frame words are not 0x00RRGGBB)."""
        import torch
        from .codec import Msv1Encoder
        frames = self._transcode_frames("transcode", keep)
        device = getattr(self.index._codec, "_device", 0)
        run = max(len(self.buffers), 1)
        bufs = [torch.zeros(self.vi.X * self.vi.Y, dtype=torch.int32, device=f"cuda:{device}") for _ in range(run + 1)]
        out: List[bytes] = []
        last = None
        with Msv1Encoder(self.vi.X, self.vi.Y, device) as enc:
            for k0 in range(0, len(frames), run):
                batch = frames[k0:k0 + run]
                free = [b for b in bufs if b is not last]
                pics = []
                for t, dst in zip(batch, free):
                    self.index.Show(t, dst, adopt=False)   # (the pixels are in dst whatever the call says of data_pnt)
                    pics.append(dst)
                out += enc.EncodeFrames(pics, [last] + pics[:-1])
                last = pics[-1]
        return out, [True] + [False] * (len(out) - 1)

    def write_transcode(self, keep: Sequence[int], fps: float = 15.0) -> bytes:
        """`transcode` as an AVI file (avi.write_avi): fourcc CRAM, 16 bpp, this Manager's width and height."""
        from .avi import write_avi
        out, flags = self.transcode(keep)
        return write_avi(self.vi.X, self.vi.Y, out, fourcc=b"CRAM", bpp=16, fps=fps, key_flags=flags)

    def proxy(self, keep: Sequence[int], win_w: int, win_h: int, filter: int = PRESENT_AREA):
        """Clip frames `keep` of the attached index, each Fit into a window of win_w x win_h (multiples of 4) as `contact_sheet` fits
        them, as a 16-bit MSVideo1 clip of that size: (list of frame bytes, key flags) — a 640x360 proxy of a 1080p recording.  The
        windows come from index.Present on a sheet (mode JSP_DISPLAY_SETPIXELS), a run of as many cells as
        the Manager's pool has buffers at a time; each cell goes to the encoder by the sheet's pitch, negated from its last row, so
        that the decoded frame buffer is bottom-up as every frame buffer is and the proxy plays upright.  No full-size picture is
        written.  ValueError as `transcode`, and for a window size that is not a positive multiple of 4."""
        import torch
        from .codec import DISPLAY_SETPIXELS, Msv1Encoder, view_matrix
        win_w, win_h = int(win_w), int(win_h)
        if win_w < 4 or win_h < 4 or win_w % 4 or win_h % 4:
            raise ValueError(f"proxy: the window size must be a positive multiple of 4 (got {win_w} x {win_h})")
        frames = self._transcode_frames("proxy", keep)
        if not hasattr(self.index, "Present"):
            raise ValueError("proxy: the attached seek index cannot present")
        device = getattr(self.index._codec, "_device", 0)
        cols = max(len(self.buffers), 1)
        pitch = cols * win_w
        sheets = [torch.zeros(win_h * pitch, dtype=torch.int32, device=f"cuda:{device}") for _ in range(2)]
        k, dx, dy = view_matrix(self.vi.X, self.vi.Y, win_w, win_h, 0.0)
        cell = lambda sheet, i: sheet.data_ptr() + 4 * ((win_h - 1) * pitch + i * win_w)   # the last row of cell i
        out: List[bytes] = []
        last = None
        with Msv1Encoder(win_w, win_h, device) as enc:
            for n, k0 in enumerate(range(0, len(frames), cols)):
                batch = frames[k0:k0 + cols]
                sheet = sheets[n & 1]
                self.index.Present(batch, win_w, win_h, k, dx, dy, mode=DISPLAY_SETPIXELS,
                                   filter=int(filter), cols=cols, out=sheet)
                pics = [cell(sheet, i) for i in range(len(batch))]
                out += enc.EncodeFrames(pics, [last] + pics[:-1], pitch=-pitch)
                last = pics[-1]
        return out, [True] + [False] * (len(out) - 1)

    def write_proxy(self, keep: Sequence[int], win_w: int, win_h: int, filter: int = PRESENT_AREA, fps: float = 15.0) -> bytes:
        """`proxy` as an AVI file (avi.write_avi): fourcc CRAM, 16 bpp, win_w x win_h."""
        from .avi import write_avi
        out, flags = self.proxy(keep, win_w, win_h, filter)
        return write_avi(int(win_w), int(win_h), out, fourcc=b"CRAM", bpp=16, fps=fps, key_flags=flags)

    # -- a clip of a part of the picture: the attached index's CropFrames (jsp_index_crop_frames) ------------------------------------------
    def crop_rect(self, rect):
        """The block rectangle for the display rectangle `rect` = (x, y, w, h), top row first, as `change_box` returns it: the
        smallest rectangle of 4x4 blocks that contains it, clipped to the block grid — ((bx, by, bw, bh), (x, y, w, h)): the block
        rectangle as CropFrames takes it (table order: block row 0 is the BOTTOM of the picture as displayed, so stored row =
        H - 1 - display row) and the display rectangle that really results.  ValueError when nothing is left."""
        x, y, w, h = (int(v) for v in rect)
        W, H = self.vi.X, self.vi.Y
        nbx, nby = W // 4, H // 4
        x0, x1 = max(x, 0), min(x + w, 4 * nbx)
        s0, s1 = max(H - (y + h), 0), min(H - y, 4 * nby)          # stored rows s0 .. s1 - 1
        if x0 >= x1 or s0 >= s1:
            raise ValueError(f"crop: nothing of the rectangle {(x, y, w, h)} lies in the picture's blocks")
        bx, by = x0 // 4, s0 // 4
        bw, bh = (x1 + 3) // 4 - bx, (s1 + 3) // 4 - by
        return (bx, by, bw, bh), (4 * bx, H - 4 * (by + bh), 4 * bw, 4 * bh)

    CROP_CALL = 4096   # pairs in one CropFrames call (jsp_index_crop_frames takes no more)

    def crop(self, frames: Sequence[bytes], rect, keep: Sequence[int], tight: bool = False):
        """The part `rect` (a display rectangle, see crop_rect) of the clip's frames `keep` (strictly ascending frame numbers, all in
        the attached index) as a clip of its own: (list of frame bytes, key flags, the display rectangle that results).  Entry 0 is
        the rectangle's key frame at keep[0], entry k the inter frame from the picture of keep[k - 1] to that of keep[k], all from
        the index's CropFrames in calls of at most 4096 pairs.  flags[0] is True; a later flag says that the frame codes every
        block of the rectangle.  tight: blocks whose pixels a gap did not change are dropped.  Nothing is decoded and neither
        decoder nor buffers change; what the index cannot cut raises its CodecError.  ValueError: `keep` empty, not strictly
        ascending or outside the clip; no index attached, a frame outside it, an index object without `CropFrames`
        (ScreenPressor's); nothing left of `rect`."""
        keep = [int(k) for k in keep]
        if not keep:
            raise ValueError("crop: keep is empty")
        for k in keep:
            if not 0 <= k < len(frames):
                raise ValueError(f"crop: frame {k} is not in the clip")
        for prev, k in zip(keep, keep[1:]):
            if k <= prev:
                raise ValueError(f"crop: keep is not strictly ascending ({k} after {prev})")
        if self.index is None:
            raise ValueError("crop: no seek index is attached")
        for k in keep:
            if not self._in_index(k):
                raise ValueError(f"crop: frame {k} is not in the attached seek index")
        if not hasattr(self.index, "CropFrames"):
            raise ValueError("crop: the attached seek index cannot crop")
        blocks, shown = self.crop_rect(rect)
        key = getattr(self.index, "KEY", -2)
        at = [k - self.index_first for k in keep]
        pairs = [(key, at[0])] + list(zip(at, at[1:]))
        out, flags = [], []
        for j0 in range(0, len(pairs), self.CROP_CALL):
            part = pairs[j0:j0 + self.CROP_CALL]
            made, keys = self.index.CropFrames(blocks, part, tight=True) if tight else self.index.CropFrames(blocks, part)
            out += list(made)
            flags += [bool(v) for v in keys]
        flags[0] = True
        return out, flags, shown

    def write_crop(self, frames: Sequence[bytes], rect, keep: Sequence[int], fps: float = 15.0, tight: bool = False) -> bytes:
        """`crop` as an AVI file (avi.write_avi) of the rectangle's size, 4 bw x 4 bh, fourcc CRAM, with this Manager's bit depth and
        palette."""
        from .avi import write_avi
        out, flags, (_, _, w, h) = self.crop(frames, rect, keep, tight=tight)
        return write_avi(w, h, out, fourcc=b"CRAM", bpp=self.vi.bpp, fps=fps, palette=self.vi.palette, key_flags=flags)

    # -- a clip that follows the action: the activity map joined to the attached index's PanFrames (jsp_index_pan_frames) ------------------
    def pan_size(self, size):
        """(bw, bh): `size` = (w, h) display pixels rounded up to 4x4 blocks and clipped to the block grid.  ValueError when nothing is left."""
        w, h = (int(v) for v in size)
        nbx, nby = self.vi.X // 4, self.vi.Y // 4
        bw, bh = min((w + 3) // 4, nbx), min((h + 3) // 4, nby)
        if bw < 1 or bh < 1:
            raise ValueError(f"pan: nothing of a rectangle of {(w, h)} pixels lies in the picture's blocks")
        return bw, bh

    @staticmethod
    def _follow_axis(p: int, n: int, b0: int, b1: int, room: int) -> int:
        """Where a span [p, p + n) goes so that [b0, b1) lies inside it: the least move, or centred on a wider box; then within [0, room]."""
        if b1 - b0 > n:
            p = b0 + (b1 - b0 - n) // 2
        elif b0 < p:
            p = b0
        elif b1 > p + n:
            p = b1 - n
        return max(0, min(p, room))

    def follow(self, size, keep: Sequence[int], start=None):
        """A path [(frame, bx, by), ...], one entry per frame of `keep` (strictly ascending, all in the attached index), for a rectangle
        of `size` display pixels (pan_size) that follows what the frames change: plain host arithmetic on activity().  Origins are in
        blocks in table order (block row 0 the BOTTOM of the picture as displayed), as PanFrames takes them.  For entry k the box is
        the union of the non-zero 16 x 16 cells of the index frames (keep[k - 1], keep[k]], in blocks, clipped to the grid.  An empty
        box, or one inside the rectangle, leaves the rectangle where it is; otherwise on each axis it moves the least number of
        blocks that brings the box inside, or centres on a box wider than itself, and is clamped to the grid.  It starts at `start`
        = (bx, by), clamped; without one centred on the first non-empty box, or on the picture when there is none.  ValueError as
        `crop`'s for `keep`, and for an index without an activity map."""
        keep = [int(k) for k in keep]
        if not keep:
            raise ValueError("pan: keep is empty")
        for prev, k in zip(keep, keep[1:]):
            if k <= prev:
                raise ValueError(f"pan: keep is not strictly ascending ({k} after {prev})")
        for k in keep:
            if not self._in_index(k):
                raise ValueError(f"pan: frame {k} is not in the attached seek index")
        bw, bh = self.pan_size(size)
        nbx, nby = self.vi.X // 4, self.vi.Y // 4
        cells = self.activity()
        cells = cells if isinstance(cells, np.ndarray) else cells.cpu().numpy()
        busy = cells != 0
        rows, cols = busy.any(axis=2), busy.any(axis=1)           # [frame, grid row], [frame, grid column]
        boxes = [None]
        for prev, k in zip(keep, keep[1:]):
            a, b = prev - self.index_first + 1, k - self.index_first + 1
            rs, qs = np.nonzero(rows[a:b].any(axis=0))[0], np.nonzero(cols[a:b].any(axis=0))[0]
            if rs.size == 0:
                boxes.append(None)
            else:   # (x0, x1, y0, y1) in blocks: a cell is 4 x 4 of them
                boxes.append((int(qs[0]) * 4, min((int(qs[-1]) + 1) * 4, nbx), int(rs[0]) * 4, min((int(rs[-1]) + 1) * 4, nby)))
        if start is not None:
            x, y = max(0, min(int(start[0]), nbx - bw)), max(0, min(int(start[1]), nby - bh))
        else:
            x0, x1, y0, y1 = next((b for b in boxes if b is not None), (0, nbx, 0, nby))
            x = max(0, min(x0 + (x1 - x0 - bw) // 2, nbx - bw))
            y = max(0, min(y0 + (y1 - y0 - bh) // 2, nby - bh))
        path = []
        for k, box in zip(keep, boxes):
            if box is not None:
                x = self._follow_axis(x, bw, box[0], box[1], nbx - bw)
                y = self._follow_axis(y, bh, box[2], box[3], nby - bh)
            path.append((k, x, y))
        return path

    PAN_CALL = 4096   # pairs in one PanFrames call (jsp_index_pan_frames takes no more)

    def pan(self, frames: Sequence[bytes], size, path, tight: bool = True):
        """The clip of a rectangle of `size` display pixels (pan_size) along `path` = [(frame, bx, by), ...] as `follow` returns it:
        (list of frame bytes, key flags, the display rectangles (x, y, w, h) top row first, one per entry).  Entry 0 is the
        rectangle's key frame at its first position; entry k the frame from the rectangle at path[k - 1] in the picture of that
        frame to the rectangle at path[k] in the picture of this one — all from the index's PanFrames, in calls of at most 4096
        pairs.  tight (the default): a frame codes only the blocks that differ from the block that stood at the same place of the
        rectangle before; else a frame behind a move codes every block.  flags[0] is True; a later flag says that the frame codes
        every block.  Nothing is decoded and neither decoder nor buffers change; what the index cannot cut raises its CodecError.
        ValueError: `crop`'s, a path that is not strictly ascending, an origin outside the grid, an index object without `PanFrames`."""
        path = [(int(k), int(x), int(y)) for k, x, y in path]
        if not path:
            raise ValueError("pan: the path is empty")
        for k, _, _ in path:
            if not 0 <= k < len(frames):
                raise ValueError(f"pan: frame {k} is not in the clip")
        for (prev, _, _), (k, _, _) in zip(path, path[1:]):
            if k <= prev:
                raise ValueError(f"pan: the path is not strictly ascending ({k} after {prev})")
        if self.index is None:
            raise ValueError("pan: no seek index is attached")
        for k, _, _ in path:
            if not self._in_index(k):
                raise ValueError(f"pan: frame {k} is not in the attached seek index")
        if not hasattr(self.index, "PanFrames"):
            raise ValueError("pan: the attached seek index cannot pan")
        bw, bh = self.pan_size(size)
        nbx, nby, H = self.vi.X // 4, self.vi.Y // 4, self.vi.Y
        for k, x, y in path:
            if not (0 <= x <= nbx - bw and 0 <= y <= nby - bh):
                raise ValueError(f"pan: the rectangle of frame {k} at block ({x}, {y}) is outside the block grid")
        key = getattr(self.index, "KEY", -2)
        at = [(k - self.index_first, (x, y)) for k, x, y in path]
        pairs = [(key, at[0][0], None, at[0][1])] + [(a, b, A, B) for (a, A), (b, B) in zip(at, at[1:])]
        out, flags = [], []
        for j0 in range(0, len(pairs), self.PAN_CALL):
            made, keys = self.index.PanFrames((bw, bh), pairs[j0:j0 + self.PAN_CALL], tight=bool(tight))
            out += list(made)
            flags += [bool(v) for v in keys]
        flags[0] = True
        return out, flags, [(4 * x, H - 4 * (y + bh), 4 * bw, 4 * bh) for _, x, y in path]

    def write_pan(self, frames: Sequence[bytes], size, path, fps: float = 15.0, tight: bool = True) -> bytes:
        """`pan` as an AVI file (avi.write_avi) of the rectangle's size, 4 bw x 4 bh, fourcc CRAM, with this Manager's bit depth and
        palette, as `write_crop` writes `crop`."""
        from .avi import write_avi
        out, flags, shown = self.pan(frames, size, path, tight=tight)
        return write_avi(shown[0][2], shown[0][3], out, fourcc=b"CRAM", bpp=self.vi.bpp, fps=fps, palette=self.vi.palette, key_flags=flags)

    # -- a clip along any path through the index: the attached index's PathFrames (jsp_index_path_frames) ----------------------------------
    PATH_CALL = 4096   # pairs in one PathFrames call (jsp_index_path_frames takes no more)

    def sequence(self, frames: Sequence[bytes], order: Sequence[int], rect=None, tight: bool = False):
        """The clip's frames in ANY order as a clip of its own: (list of frame bytes, key flags, the display rectangle that results).
        `order` is a list of frame numbers of the attached index — repeats allowed, any direction, at most 4096.  Entry 0 is the
        key frame of the rectangle at order[0]; entry k the inter frame from the picture of order[k - 1] to that of order[k] — a
        step forward, a step back or, for a repeat, a frame of skip words — all from ONE PathFrames call.  rect: a display
        rectangle (see crop_rect), None for the whole block grid.  tight: blocks whose pixels are equal in both pictures are
        dropped.  flags[0] is True; a later flag says that the frame codes every block of the rectangle.  Nothing is decoded and
        neither decoder nor buffers change; what the index cannot make raises its CodecError.  ValueError: `order` empty, too
        long or outside the clip; no index attached, a frame outside it, an index object without `PathFrames` (ScreenPressor's);
        nothing left of `rect`."""
        order = [int(k) for k in order]
        if not order:
            raise ValueError("sequence: order is empty")
        if len(order) > self.PATH_CALL:
            raise ValueError(f"sequence: order has more than {self.PATH_CALL} frames")
        for k in order:
            if not 0 <= k < len(frames):
                raise ValueError(f"sequence: frame {k} is not in the clip")
        if self.index is None:
            raise ValueError("sequence: no seek index is attached")
        for k in order:
            if not self._in_index(k):
                raise ValueError(f"sequence: frame {k} is not in the attached seek index")
        if not hasattr(self.index, "PathFrames"):
            raise ValueError("sequence: the attached seek index cannot step back")
        W, H = self.vi.X, self.vi.Y
        blocks, shown = self.crop_rect((0, 0, W, H) if rect is None else rect)
        key = getattr(self.index, "KEY", -2)
        at = [k - self.index_first for k in order]
        pairs = [(key, at[0])] + list(zip(at, at[1:]))
        made, keys = self.index.PathFrames(blocks, pairs, tight=True) if tight else self.index.PathFrames(blocks, pairs)
        flags = [bool(v) for v in keys]
        flags[0] = True
        return list(made), flags, shown

    @staticmethod
    def _ascending(who: str, keep: Sequence[int]):
        keep = [int(k) for k in keep]
        if not keep:
            raise ValueError(f"{who}: keep is empty")
        for prev, k in zip(keep, keep[1:]):
            if k <= prev:
                raise ValueError(f"{who}: keep is not strictly ascending ({k} after {prev})")
        return keep

    def reverse(self, frames: Sequence[bytes], keep: Sequence[int], rect=None, tight: bool = False):
        """`sequence` of the strictly ascending list `keep` played from its end: keep[-1], ..., keep[0]."""
        return self.sequence(frames, self._ascending("reverse", keep)[::-1], rect=rect, tight=tight)

    def boomerang(self, frames: Sequence[bytes], keep: Sequence[int], rect=None, tight: bool = False):
        """`sequence` of the strictly ascending list `keep` there and back: keep[0], ..., keep[-1], ..., keep[0].  The last step
        returns to keep[0], so the last picture is the first and the file loops."""
        keep = self._ascending("boomerang", keep)
        return self.sequence(frames, keep + keep[-2::-1], rect=rect, tight=tight)

    def write_sequence(self, frames: Sequence[bytes], order: Sequence[int], rect=None, fps: float = 15.0, tight: bool = False) -> bytes:
        """`sequence` as an AVI file (avi.write_avi) of the rectangle's size, 4 bw x 4 bh, fourcc CRAM, with this Manager's bit depth
        and palette, as `write_crop` writes `crop`."""
        from .avi import write_avi
        out, flags, (_, _, w, h) = self.sequence(frames, order, rect=rect, tight=tight)
        return write_avi(w, h, out, fourcc=b"CRAM", bpp=self.vi.bpp, fps=fps, palette=self.vi.palette, key_flags=flags)

    def write_reverse(self, frames: Sequence[bytes], keep: Sequence[int], rect=None, fps: float = 15.0, tight: bool = False) -> bytes:
        """`reverse` as an AVI file, as `write_sequence` writes `sequence`."""
        return self.write_sequence(frames, self._ascending("reverse", keep)[::-1], rect=rect, fps=fps, tight=tight)

    def write_boomerang(self, frames: Sequence[bytes], keep: Sequence[int], rect=None, fps: float = 15.0, tight: bool = False) -> bytes:
        """`boomerang` as an AVI file, as `write_sequence` writes `sequence`."""
        keep = self._ascending("boomerang", keep)
        return self.write_sequence(frames, keep + keep[-2::-1], rect=rect, fps=fps, tight=tight)

    def _index_adopts(self) -> bool:
        return bool(getattr(self.index, "ADOPTS", True))

    def _in_index(self, i: int) -> bool:
        return self.index is not None and self.index_first <= i < self.index_first + self.index.frames

    def preview(self, i: int, scale: int = 8):
        """The thumbnail of clip frame `i` from the attached index (the picture that follows the pointer along the seek bar,
        Main.on_mouse_move): one `Thumbs` launch, a pure read — no buffer, hold, log entry or decoder state changes.  The index is
        MSVideo1's SeekIndex or ScreenPressor's SpScrubIndex alike.  No index attached, `i` outside it, or an index object without
        `Thumbs`: ValueError (a hover preview is not worth a decode)."""
        if not self._in_index(i):
            raise ValueError(f"frame {i} is not in an attached seek index")
        if not hasattr(self.index, "Thumbs"):
            raise ValueError("the attached seek index has no thumbnails")
        return self.index.Thumbs([i - self.index_first], scale=scale, cols=1)

    def filmstrip(self, n: int, scale: int = 8, cols: Optional[int] = None):
        """`n` frames spread evenly over the attached index — clip frame index_first + (k * index.frames) // n for k < n — as one
        sheet of thumbnails, `cols` to a row (None: one row): (clip frame numbers, sheet).  One `Thumbs` launch, a pure read as
        `preview`, from the index of either codec.  No index attached, or an index object without `Thumbs`: ValueError."""
        if self.index is None:
            raise ValueError("no seek index attached")
        if not hasattr(self.index, "Thumbs"):
            raise ValueError("the attached seek index has no thumbnails")
        n = int(n)
        if n < 1:
            raise ValueError("a filmstrip needs at least one frame")
        picks = [(k * self.index.frames) // n for k in range(n)]
        sheet = self.index.Thumbs(picks, scale=scale, cols=n if cols is None else int(cols))
        return [self.index_first + t for t in picks], sheet

    def _index_present_mode(self) -> int:
        from .codec import DISPLAY_CANVAS, DISPLAY_CANVAS_RGB15
        return DISPLAY_CANVAS_RGB15 if self.vi.bpp == 16 and self.vi.codec == CODEC_SCREENPRESSOR else DISPLAY_CANVAS

    def present_from_index(self, i: int, out, win_w: int, win_h: int, filter: Optional[int] = None, background: int = 0xFF000000):
        """The window `self.view` shows of clip frame `i` of the attached index, as canvas pixels, top row first, into the device
        tensor `out` (win_w * win_h ints): what `present` gives for a buffer holding that frame, straight from the index — one
        `Present` launch, a pure read as `preview`: no buffer, hold, log entry or decoder state changes.  `filter` as for
        `present` (None: bilinear; PRESENT_AREA is taken too).  No index attached, `i` outside it, or an index object without
        `Present`: ValueError."""
        from .codec import PRESENT_BILINEAR
        if not self._in_index(i):
            raise ValueError(f"frame {i} is not in an attached seek index")
        if not hasattr(self.index, "Present"):
            raise ValueError("the attached seek index cannot present")
        k, dx, dy = self.view.matrix(self.vi.X, self.vi.Y, win_w, win_h)
        return self.index.Present([i - self.index_first], win_w, win_h, k, dx, dy, mode=self._index_present_mode(),
                                  filter=PRESENT_BILINEAR if filter is None else filter, background=background, cols=1, out=out)

    def contact_sheet(self, n: int, win_w: int, win_h: int, cols: Optional[int] = None, filter: Optional[int] = None):
        """The `n` frames `filmstrip` picks — clip frame index_first + (k * index.frames) // n for k < n — each Fit into a cell of
        win_w x win_h canvas pixels, `cols` to a row (None: one row): (clip frame numbers, sheet).  One `Present` launch, a pure
        read.  `filter` None: PRESENT_AREA, what a shrunk picture needs.  No index attached, or an index object without `Present`:
        ValueError."""
        from .codec import PRESENT_AREA, view_matrix
        if self.index is None:
            raise ValueError("no seek index attached")
        if not hasattr(self.index, "Present"):
            raise ValueError("the attached seek index cannot present")
        n = int(n)
        if n < 1:
            raise ValueError("a contact sheet needs at least one frame")
        picks = [(k * self.index.frames) // n for k in range(n)]
        k, dx, dy = view_matrix(self.vi.X, self.vi.Y, win_w, win_h, 0.0)
        sheet = self.index.Present(picks, win_w, win_h, k, dx, dy, mode=self._index_present_mode(),
                                   filter=PRESENT_AREA if filter is None else filter, cols=n if cols is None else int(cols))
        return [self.index_first + t for t in picks], sheet

    def tensor_from_index(self, frames, win_w: int, win_h: int, **kw):
        """The clip frames `frames` of the attached index, each Fit into win_w x win_h as `contact_sheet` fits them, as a model's
        input batch: the index's `Tensor` (dtype, layout, scale, bias, filter — default PRESENT_AREA —, background and out go
        through `kw`).  One `Tensor` launch, a pure read.  No index attached, a frame outside it, or an index object without
        `Tensor`: ValueError."""
        from .codec import view_matrix
        if self.index is None:
            raise ValueError("no seek index attached")
        if not hasattr(self.index, "Tensor"):
            raise ValueError("the attached seek index has no tensors")
        frames = [int(i) for i in frames]
        for i in frames:
            if not self._in_index(i):
                raise ValueError(f"frame {i} is not in an attached seek index")
        k, dx, dy = view_matrix(self.vi.X, self.vi.Y, win_w, win_h, 0.0)
        kw.setdefault("mode", self._index_present_mode())
        return self.index.Tensor([i - self.index_first for i in frames], win_w, win_h, k, dx, dy, **kw)

    def _slot_of(self, buf) -> int:
        for i, b in enumerate(self.buffers):
            if b is buf:
                return i
        return -1

    def _get_free_buffer(self, prev_idx: int) -> int:  # Manager.hx:424-443
        oldest, oldest_first = -1, 1 << 30
        for i, h in enumerate(self.holds):
            if i == prev_idx:
                continue
            if h is None:
                return i
            if h.stop - 1 < self.frame_of_interest and h.start < oldest_first:
                oldest, oldest_first = i, h.start
        if oldest >= 0:
            self.holds[oldest] = None
        return oldest

    def worker(self, frame: bytes, index: int, prev_key_bytes: Optional[bytes], key: Optional[bool] = None) -> DecodedFrame:
        """One decode tick for compressed frame `index` (Manager.hx:454-539).  `key` = the flag the loader
        attached to the frame (an AVI index's, DataLoader.hx:373-401); None = scan the bytes."""
        dec = self.decoder
        if key is None:
            key = index == 0 or dec.IsKeyFrame(frame)      # DataLoaderAVISeq.hx:45
        prev = dec.PreviousFrame()
        prev_idx = self._slot_of(prev) if prev is not None else -1
        self.frame_of_interest = index                       # sequential playback keeps up with decode
        free = self._get_free_buffer(prev_idx)
        assert free >= 0
        new = self.buffers[free]
        if key:
            state = int(dec.DecompressI(frame, new))
            sig: Optional[bool] = None
            if state == 0:
                self.holds[free] = range(index, index + 1)
                # frames_differ_significantly, Manager.hx:392-421
                if index == 0:
                    sig = True
                elif prev_key_bytes is not None:
                    sig = prev_key_bytes != frame
                elif prev is None:
                    sig = True
                elif self._fused_compare:
                    sig = dec.KeyFrameDiffers()
                    sig = True if sig is None else sig
                else:
                    sig = _differ(new, prev, INSIGNIFICANT_LINES * self.vi.X)
            out = DecodedFrame(index, True, free, sig, state)
        else:
            res = dec.DecompressP(frame, new)
            shown = free
            if res.data_pnt is not None:
                if res.data_pnt is prev:                     # "no changes": the old slot keeps showing
                    h = self.holds[prev_idx]
                    self.holds[prev_idx] = range(h.start, index + 1) if h else range(index, index + 1)
                    shown = prev_idx
                else:
                    self.holds[free] = range(index, index + 1)
            out = DecodedFrame(index, False, shown, res.significant_changes)
        self.log.append(out)
        self.next_frame_to_decode = index + 1
        self._last_was_key = key
        return out

    def play(self, frames: Sequence[bytes], on_frame: Optional[Callable[[DecodedFrame, object], None]] = None,
             key_flags: Optional[Sequence[bool]] = None):
        prev_key = None
        for i, f in enumerate(frames):
            was_key = bool(key_flags[i]) if key_flags is not None else (i == 0 or self.decoder.IsKeyFrame(f))
            d = self.worker(f, i, prev_key if was_key and i > 0 and self._last_was_key else None, was_key)
            self._last_was_key = was_key
            prev_key = f if was_key else prev_key
            if on_frame:
                on_frame(d, self.buffers[d.buffer_index])
        return self.log

    _last_was_key = False

    def _key_at(self, frames: Sequence[bytes], i: int, key_flags) -> bool:
        if key_flags is not None:
            return i < len(key_flags) and bool(key_flags[i])
        return i == 0 or bool(self.decoder.IsKeyFrame(frames[i]))

    def seek(self, frames: Sequence[bytes], index: int, key_flags: Optional[Sequence[bool]] = None) -> DecodedFrame:
        """Show frame `index` of `frames` — the seek branch of GetDecompressedFrame (Manager.hx:216-259).  A frame some
        buffer holds is shown without decoding.  Otherwise decoding starts at the nearest key frame (every hold trashed)
        unless the stretch being decoded already leads to `index`, and the frames up to it go to the decoder's Seek (one
        call) or, without one, through worker() one by one.  worker / play continue from index + 1 afterwards."""
        if not 0 <= index < len(frames):
            raise IndexError(f"frame {index} outside the clip ({len(frames)} frames)")
        self.frame_of_interest = index
        for nb, h in enumerate(self.holds):
            if h is not None and h.start <= index < h.stop:
                return DecodedFrame(index, self._key_at(frames, index, key_flags), nb, None)
        if self._in_index(index) and not self._index_adopts():
            # one launch into a free buffer, never the decoder's previous frame; the decoder, the decode position and the other
            # holds stay as they are: a later seek outside the index, or play, goes on from where the decoder really stands
            prev = self.decoder.PreviousFrame()
            prev_idx = self._slot_of(prev) if prev is not None else -1
            free = self._get_free_buffer(prev_idx)
            if free < 0:   # (a walk backwards: every hold lies after the frame of interest — the one farthest from it goes)
                free = max((nb for nb in range(len(self.holds)) if nb != prev_idx), key=lambda nb: abs(self.holds[nb].start - index))
            res = self.index.Show(index - self.index_first, self.buffers[free])
            self.holds[free] = range(index, index + 1)
            out = DecodedFrame(index, self._key_at(frames, index, key_flags), free, res.significant_changes)
            self.log.append(out)
            return out
        key_idx = nearest_key_frame(lambda i: self._key_at(frames, i, key_flags), index, len(frames))
        if self.next_frame_to_decode < key_idx or self.next_frame_to_decode > index:
            self.next_frame_to_decode = key_idx
            self.holds = [None] * len(self.buffers)
        start = self.next_frame_to_decode
        keys = [self._key_at(frames, i, key_flags) for i in range(start, index + 1)]
        dec = self.decoder
        use_index = self._in_index(index)
        if use_index or (getattr(dec, "SEEKS", False) and hasattr(dec, "Seek")):
            prev = dec.PreviousFrame()
            prev_idx = self._slot_of(prev) if prev is not None else -1
            free = self._get_free_buffer(prev_idx)
            assert free >= 0
            if use_index:   # one launch; the decoder ends as the Seek from the index's first frame would leave it
                res = self.index.Show(index - self.index_first, self.buffers[free], adopt=True)
            else:
                res = dec.Seek(frames[start:index + 1], self.buffers[free], keys)
            shown = free
            if res.data_pnt is not None:
                held = self._slot_of(res.data_pnt)
                if res.data_pnt is not self.buffers[free] and held >= 0:      # nothing in the range changed the picture
                    h = self.holds[held]
                    self.holds[held] = range(h.start, index + 1) if h else range(index, index + 1)
                    shown = held
                else:
                    self.holds[free] = range(index, index + 1)
            out = DecodedFrame(index, keys[-1], shown, None if keys[-1] else res.significant_changes)
            self.log.append(out)
        else:
            for i in range(start, index + 1):
                out = self.worker(frames[i], i, None, keys[i - start])
        self._last_was_key = keys[-1]
        self.next_frame_to_decode = index + 1
        return out

    def play_from_index(self, start: int, count: Optional[int] = None, stride: int = 1,
                        on_frame: Optional[Callable[[DecodedFrame, object], None]] = None,
                        key_flags: Optional[Sequence[bool]] = None) -> List[DecodedFrame]:
        """Clip frames start, start + stride, ... (`count` of them; None: to the end of the index) served from an attached index
        that does not adopt (ScreenPressor's SpScrubIndex) — play on from a shown frame, fast-forward, filling the free buffers
        around the frame of interest.  The frames go out in batches of the buffers that are not the decoder's previous frame, ONE
        `Play` launch per batch; holds, `frame_of_interest` and `log` (a DecodedFrame with the index's verdict) follow each frame,
        and `on_frame(frame, buffer)` is called per frame in order, before the next batch overwrites its buffer.  The decoder, its
        previous buffer and `next_frame_to_decode` are untouched.  `key_flags` (the clip's, as for seek(); optional) only fills
        DecodedFrame.key.  Past the end of the index play goes on with `seek()` to the
        next clip frame: one decode when that frame is a coded key frame (which renews every bit of decoder state), else the
        decodes from the nearest key frame.  ValueError: no index attached, a frame outside it, an index that adopts (MSVideo1's
        SeekIndex needs none of this: its Show leaves the decoder at the frame), an index object without `Play`."""
        if self.index is None:
            raise ValueError("no seek index attached")
        if self._index_adopts():
            raise ValueError("the attached seek index adopts: seek() moves the decoder with it")
        if not hasattr(self.index, "Play"):
            raise ValueError("the attached seek index cannot play")
        start, stride = int(start), int(stride)
        if stride < 1:
            raise ValueError("stride must be at least 1")
        end = self.index_first + self.index.frames
        if count is None:
            count = (end - start + stride - 1) // stride if self._in_index(start) else 0
        count = int(count)
        if count < 1 or not self._in_index(start) or not self._in_index(start + (count - 1) * stride):
            raise ValueError(f"frames {start} .. {start + (max(count, 1) - 1) * stride} are not all in the attached seek index")
        prev = self.decoder.PreviousFrame()
        prev_idx = self._slot_of(prev) if prev is not None else -1
        slots = [nb for nb in range(len(self.buffers)) if nb != prev_idx]
        out: List[DecodedFrame] = []
        for k0 in range(0, count, len(slots)):
            batch = slots[:min(len(slots), count - k0)]
            first = start + k0 * stride
            results = self.index.Play(first - self.index_first, [self.buffers[nb] for nb in batch], stride)
            for nb in batch:
                self.holds[nb] = None
            for j, (nb, res) in enumerate(zip(batch, results)):
                i = first + j * stride
                self.holds[nb] = range(i, i + 1)
                self.frame_of_interest = i
                d = DecodedFrame(i, key_flags is not None and i < len(key_flags) and bool(key_flags[i]), nb, res.significant_changes)
                self.log.append(d)
                out.append(d)
                if on_frame:
                    on_frame(d, self.buffers[nb])
        return out

    def run_from_index(self, start: int, count: Optional[int] = None, stride: int = 1, reverse: bool = False,
                       on_frame: Optional[Callable[[DecodedFrame, object], None]] = None,
                       key_flags: Optional[Sequence[bool]] = None) -> List[DecodedFrame]:
        """Clip frames start, start + stride, ... — or, with `reverse`, start, start - stride, ... — (`count` of them; None: to the
        end, or the start, of the index) served from an attached index that adopts and has `Play` (MSVideo1's SeekIndex): reverse
        play and the step-back button held down, fast-forward, filling the free buffers around the frame of interest.  The frames
        go out in batches of the buffers that are not the decoder's previous frame, ONE `Play` launch per batch (for reverse the
        batch's lowest frame is its first and the buffer list is reversed).  `on_frame(frame, buffer)` is called per frame in shown
        order, before the next batch overwrites its buffer; holds follow each frame's data_pnt as in seek() (a frame that wrote
        nothing extends the hold of the buffer that shows it), `log` gets a DecodedFrame per frame.  The last frame shown is
        adopted, in the final batch only: afterwards the decoder stands at it, `next_frame_to_decode` is that frame + 1,
        `frame_of_interest` that frame, and worker / play go on from there.  `key_flags` as for seek().  ValueError: no index
        attached, a frame outside it, an index that does not adopt (play_from_index serves it), an index object without `Play`."""
        if self.index is None:
            raise ValueError("no seek index attached")
        if not self._index_adopts():
            raise ValueError("the attached seek index does not adopt: play_from_index serves it")
        if not hasattr(self.index, "Play"):
            raise ValueError("the attached seek index cannot play")
        start, stride = int(start), int(stride)
        if stride < 1:
            raise ValueError("stride must be at least 1")
        step = -stride if reverse else stride
        if count is None:
            room = start - self.index_first if reverse else self.index_first + self.index.frames - 1 - start
            count = room // stride + 1 if self._in_index(start) else 0
        count = int(count)
        if count < 1 or not self._in_index(start) or not self._in_index(start + (count - 1) * step):
            raise ValueError(f"frames {start} .. {start + (max(count, 1) - 1) * step} are not all in the attached seek index")
        prev = self.decoder.PreviousFrame()
        prev_idx = self._slot_of(prev) if prev is not None else -1
        slots = [nb for nb in range(len(self.buffers)) if nb != prev_idx]
        out: List[DecodedFrame] = []
        for k0 in range(0, count, len(slots)):
            batch = slots[:min(len(slots), count - k0)]
            m = len(batch)
            shown_first = start + k0 * step                     # the batch's frames in shown order: shown_first + j * step
            final = k0 + m >= count
            bufs = [self.buffers[nb] for nb in batch]
            if reverse:   # an ascending run from the batch's lowest frame, the last one shown: buffer j holds run frame m - 1 - j
                results = self.index.Play(shown_first + (m - 1) * step - self.index_first, bufs[::-1], stride, adopt=0 if final else None)[::-1]
            else:
                results = self.index.Play(shown_first - self.index_first, bufs, stride, adopt=m - 1 if final else None)
            for nb in batch:
                self.holds[nb] = None
            for j, (nb, res) in enumerate(zip(batch, results)):
                i = shown_first + j * step
                shown = nb
                if res.data_pnt is not None:
                    held = self._slot_of(res.data_pnt)
                    if res.data_pnt is not self.buffers[nb] and held >= 0:      # nothing up to frame i changed the picture
                        h = self.holds[held]
                        self.holds[held] = range(min(h.start, i), max(h.stop, i + 1)) if h else range(i, i + 1)
                        shown = held
                    else:
                        self.holds[nb] = range(i, i + 1)
                self.frame_of_interest = i
                key = key_flags is not None and i < len(key_flags) and bool(key_flags[i])
                d = DecodedFrame(i, key, shown, None if key else res.significant_changes)
                self.log.append(d)
                out.append(d)
                if on_frame:
                    on_frame(d, self.buffers[shown])
        self.next_frame_to_decode = out[-1].index + 1
        self._last_was_key = out[-1].key
        return out

    def _known_significance(self) -> Dict[int, bool]:
        """frames[i].significant_changes of the reference's loader: what decoding frame i recorded (missing = not known)."""
        known = {}
        if self.index is not None:
            known.update((self.index_first + i, bool(v)) for i, v in enumerate(self.index.significance))
        known.update(self.judged)
        for d in self.log:
            if d.significant_changes is not None:
                known[d.index] = bool(d.significant_changes)
        return known

    def skip_stills(self, frames: Sequence[bytes], key_flags: Optional[Sequence[bool]] = None) -> DecodedFrame:
        """Skip to the next frame that changes the picture significantly — SkipStills(first_call = true) (Manager.hx:289-317)
        over FindPossibleChange (DataLoader.hx:239-252), then the SeekTo that Main.play_timer does with the answer.  The
        candidates start after the frame shown; significance already known (frames decoded before, frames a FindChange call
        judged) is used as it is, and a known change is shown through seek().  From the first frame nobody has judged on, a
        decoder with FindChange gets ONE call from the decode position to the end of the clip; without one, worker() decodes
        frame by frame up to a significant frame.  When nothing changes up to the end, the last frame is shown.  worker /
        play continue from the frame shown + 1 afterwards."""
        n = len(frames)
        if n == 0:
            raise IndexError("skip_stills: empty clip")
        pos = self.frame_of_interest + 1
        known = self._known_significance()
        while pos < n:
            sig = known.get(pos)
            if sig is None:
                break
            if sig:
                return self.seek(frames, pos, key_flags)
            pos += 1
        if pos >= n:
            return self.seek(frames, n - 1, key_flags)
        # frame `pos` has not been judged: decode from where decoding stands (or, as seek() does, from the nearest key frame)
        self.frame_of_interest = pos
        key_idx = nearest_key_frame(lambda i: self._key_at(frames, i, key_flags), pos, n)
        chained = True    # decoding goes on from the frame decoded last
        if self.next_frame_to_decode < key_idx or self.next_frame_to_decode > pos:
            self.next_frame_to_decode = key_idx
            self.holds = [None] * len(self.buffers)
            chained = False
        start = self.next_frame_to_decode
        keys = [self._key_at(frames, i, key_flags) for i in range(start, n)]
        key_before = frames[start - 1] if chained and start > 0 and self._last_was_key else None
        dec = self.decoder
        if getattr(dec, "FINDS_CHANGES", False) and hasattr(dec, "FindChange"):
            prev = dec.PreviousFrame()
            prev_idx = self._slot_of(prev) if prev is not None else -1
            free = self._get_free_buffer(prev_idx)
            assert free >= 0
            res = dec.FindChange(frames[start:], self.buffers[free], keys, first=pos - start, key_before=key_before,
                                 key_row=INSIGNIFICANT_LINES)
            f = start + res.index
            for j, sg in enumerate(res.significance):
                if sg is not None:
                    self.judged[start + j] = sg
            shown = free
            if res.data_pnt is not None:
                if res.data_pnt is prev and prev_idx >= 0:      # nothing up to f changed the picture
                    h = self.holds[prev_idx]
                    self.holds[prev_idx] = range(h.start, f + 1) if h else range(f, f + 1)
                    shown = prev_idx
                else:
                    self.holds[free] = range(f, f + 1)
            out = DecodedFrame(f, keys[f - start], shown, res.significance[f - start])
            self.log.append(out)
            self._last_was_key = keys[f - start]
        else:
            prev_key = key_before
            for i in range(start, n):
                key = keys[i - start]
                out = self.worker(frames[i], i, prev_key if key else None, key)
                prev_key = frames[i] if key else None
                if i >= pos and out.significant_changes:
                    break
            f = out.index
        self.frame_of_interest = f
        self.next_frame_to_decode = f + 1
        return out

    # -- navigation, Manager.hx:184-208 (last_frame_drawn = the frame shown) over seek() -------------------------------------
    def next_frame(self, frames: Sequence[bytes], key_flags: Optional[Sequence[bool]] = None) -> DecodedFrame:
        """NextFrameTime: the frame after the one shown (the last frame stays)."""
        return self.seek(frames, min(self.frame_of_interest + 1, len(frames) - 1), key_flags)

    def prev_frame(self, frames: Sequence[bytes], key_flags: Optional[Sequence[bool]] = None) -> DecodedFrame:
        """PrevFrameTime: the frame before the one shown (frame 0 stays)."""
        return self.seek(frames, max(self.frame_of_interest - 1, 0), key_flags)

    def next_key(self, frames: Sequence[bytes], key_flags: Optional[Sequence[bool]] = None) -> DecodedFrame:
        """NextKeyTime over DataLoader.GetNextKeyFrame (DataLoader.hx:134-142): the first key frame after the one shown, else the
        last frame."""
        n = len(frames)
        i = min(self.frame_of_interest + 1, n - 1)
        while i < n - 1 and not self._key_at(frames, i, key_flags):
            i += 1
        return self.seek(frames, i, key_flags)

    def prev_key(self, frames: Sequence[bytes], key_flags: Optional[Sequence[bool]] = None) -> DecodedFrame:
        """PrevKeyTime: the nearest key frame before the one shown (frame 0 at the start)."""
        i = nearest_key_frame(lambda k: self._key_at(frames, k, key_flags), self.frame_of_interest - 1, len(frames))
        return self.seek(frames, i, key_flags)

    def play_pipelined(self, frames: Sequence[bytes], depth: int = 4,
                       on_frame: Optional[Callable[[DecodedFrame, object], None]] = None,
                       key_flags: Optional[Sequence[bool]] = None, prefetch_bytes: int = 0):
        """play() through the asynchronous calls (DecompressI_async / DecompressP_async / wait): up to `depth` frames are in
        flight, the host stage of frame n+1 runs while the uploads and kernels of frame n do.  The log is the one play()
        writes.  HIP codecs only; the pool must hold `depth` more buffers than play() needs (Manager(..., num_buffers =
        NUM_BUFFERS + depth)): a frame in flight keeps its destination AND the buffer it was decoded against."""
        from collections import deque
        from .codec import CodecError
        dec = self.decoder
        dec.set_option("async_depth", str(depth))
        # prefetch_bytes > 0 (MSVideo1): the frames are laid out in ONE pinned arena, as the file holds them (a chunk header in front of
        # each), and the arena goes to the device in ranges of about that size — the range after the current one ahead of the frames
        # being submitted (decoder.prefetch / jsp_prefetch); the frames then queue no upload of their own.  examples/jsp_play --prefetch.
        arena, spans, ahead = None, [], deque()
        if prefetch_bytes > 0 and hasattr(dec, "prefetch") and len(frames):
            from .codec import HostBuffer
            import numpy as np
            arena = HostBuffer(sum(len(f) + 8 + (len(f) & 1) for f in frames) + 16)
            pos = 0
            for f in frames:
                pos += 8
                arena.array[pos:pos + len(f)] = np.frombuffer(bytes(f), dtype=np.uint8)
                spans.append((pos, pos + len(f)))
                pos += len(f) + (len(f) & 1)
            frames = [arena.array[a:b] for a, b in spans]

        def fetch(i0):
            lo, j, hi = spans[i0][0] - 8, i0, spans[i0][1]
            while j < len(spans) and (j == i0 or spans[j][1] - lo <= prefetch_bytes):
                hi = spans[j][1]
                j += 1
            dec.prefetch(arena.array[lo:hi])
            ahead.append((i0, j))
        flying: deque = deque()      # (ticket, index, key, slot, prev_slot, prev buffer, compare bytes?, frame bytes)

        def collect():
            ticket, index, key, slot, prev_slot, prev, cmp_bytes, blob, prev_blob = flying.popleft()
            got = dec.wait(ticket)
            if key:
                state, sig = int(got), None
                if state == 0:
                    if index == 0:
                        sig = True
                    elif cmp_bytes:
                        sig = not (len(prev_blob) == len(blob) and bytes(prev_blob) == bytes(blob))
                    elif prev is None:
                        sig = True
                    elif self._fused_compare:
                        sig = dec.KeyFrameDiffers()      # (of the key frame just collected)
                        sig = True if sig is None else sig
                    else:
                        sig = _differ(self.buffers[slot], prev, INSIGNIFICANT_LINES * self.vi.X)
                out = DecodedFrame(index, True, slot, sig, state)
            else:
                shown = slot
                if got.data_pnt is not None and got.data_pnt is prev and prev_slot >= 0:
                    shown = prev_slot
                out = DecodedFrame(index, False, shown, got.significant_changes)
            self.log.append(out)
            if on_frame:
                on_frame(out, self.buffers[out.buffer_index])

        prev_key, last_was_key = None, False
        for i, f in enumerate(frames):
            if len(flying) == depth:
                collect()
            if arena is not None:
                while ahead and not (ahead[0][0] <= i < ahead[0][1]):
                    ahead.popleft()
                if not ahead:
                    fetch(i)
                if len(ahead) < 2 and ahead[-1][1] < len(spans):
                    fetch(ahead[-1][1])
            key = bool(key_flags[i]) if key_flags is not None else (i == 0 or dec.IsKeyFrame(f))
            prev = dec.PreviousFrame()                      # as of the last SUBMITTED frame
            prev_slot = self._slot_of(prev) if prev is not None else -1
            busy = {prev_slot} | {fl[3] for fl in flying} | {fl[4] for fl in flying}
            # what may still be looked at: everything from the oldest frame in flight on
            horizon = flying[0][1] - 1 if flying else i
            slot, oldest, oldest_first = -1, -1, 1 << 30
            for k, h in enumerate(self.holds):
                if k in busy:
                    continue
                if h is None:
                    slot = k
                    break
                if h.stop - 1 < horizon and h.start < oldest_first:
                    oldest, oldest_first = k, h.start
            if slot < 0:
                slot = oldest
                if slot >= 0:
                    self.holds[slot] = None
            if slot < 0:
                raise CodecError("no free frame buffer: the pool needs NUM_BUFFERS + depth + 1 buffers")
            dst = self.buffers[slot]
            ticket = dec.DecompressI_async(f, dst) if key else dec.DecompressP_async(f, dst)
            now = dec.PreviousFrame()                        # adoption is decided by the host stage: known at submission
            if now is dst:
                self.holds[slot] = range(i, i + 1)
            elif now is not None and now is prev and prev_slot >= 0:
                h = self.holds[prev_slot]
                self.holds[prev_slot] = range(h.start, i + 1) if h else range(i, i + 1)
            flying.append((ticket, i, key, slot, prev_slot, prev, key and last_was_key and i > 0, f, prev_key))
            last_was_key = key
            prev_key = f if key else prev_key
            self.next_frame_to_decode = i + 1
        while flying:
            collect()
        if arena is not None:
            dec.prefetch(None)                              # (the arena goes away: the codec must not find frames in it any more)
            arena.close()
        return self.log
