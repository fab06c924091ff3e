// Host arithmetic of jsp_index_pan_frames (msv1_seek.cpp) that needs neither HIP nor the codec: the check of a rectangle's origin
// against the block grid, the kind of a pair and its check; the parts of the scratch: msv1_index_clip_layout.h.  On top of
// msv1_index_crop_layout.h.  Plain C++, so that a program of its own can run it under a sanitizer.
#pragma once
#include "msv1_index_crop_layout.h"

namespace jsp {

// Whether a rectangle of bw x bh blocks with origin (x, y) lies in a grid of nbx x nby blocks.
inline bool pan_origin_ok(int nbx, int nby, int bw, int bh, int x, int y) { return crop_rect_ok(nbx, nby, x, y, bw, bh); }

// The kinds of pair (THE RULE: msv1_index_pan_kernels.hip).  a, b: the origins (x, y) at `from` and at `to`; a is not read for a key pair.
enum PanKind { PAN_KEY = 0, PAN_STILL = 1, PAN_MOVED = 2 };
inline PanKind pan_kind(int from, int key, const int* a, const int* b) {
    if (from == key) return PAN_KEY;
    return a[0] == b[0] && a[1] == b[1] ? PAN_STILL : PAN_MOVED;
}

// What is wrong with a pair, in the order it is looked for: its frames by its kind, the origin at `to`, for gap pairs the origin at `from`.
enum PanBad { PAN_OK = 0, PAN_BAD_FRAMES = 1, PAN_BAD_TO_ORIGIN = 2, PAN_BAD_FROM_ORIGIN = 3 };
inline PanBad pan_pair_check(int nframes, int nbx, int nby, int bw, int bh, int from, int to, int key, const int* a, const int* b) {
    const PanKind kind = pan_kind(from, key, a, b);
    const bool frames = kind == PAN_KEY ? to >= 0 && to < nframes
                                        : from >= -1 && to >= 0 && to < nframes && (kind == PAN_MOVED ? from <= to : from < to);
    if (!frames) return PAN_BAD_FRAMES;
    if (!pan_origin_ok(nbx, nby, bw, bh, b[0], b[1])) return PAN_BAD_TO_ORIGIN;
    if (kind != PAN_KEY && !pan_origin_ok(nbx, nby, bw, bh, a[0], a[1])) return PAN_BAD_FROM_ORIGIN;
    return PAN_OK;
}

}  // namespace jsp
