// Host arithmetic of jsp_index_path_frames (msv1_seek.cpp) that needs neither HIP nor the codec: the kind of a pair and its check
// against the index.  The rectangle is crop's (msv1_index_crop_layout.h).  Plain C++, so that a program of its own
// can run it under a sanitizer.
#pragma once
#include "msv1_index_crop_layout.h"

namespace jsp {

// The kinds of pair (THE RULE: msv1_index_path_kernels.hip), for a pair that path_pair_ok accepts.
enum PathKind { PATH_KEY = 0, PATH_FORWARD = 1, PATH_HOLD = 2, PATH_BACK = 3 };
inline PathKind path_kind(int from, int to, int key) {
    if (from == key) return PATH_KEY;
    return from < to ? PATH_FORWARD : from == to ? PATH_HOLD : PATH_BACK;
}

// Whether (from, to) is a pair of an index of nframes frames: a key pair (from == key = -2, 0 <= to < nframes), a step forward
// (-1 <= from < to < nframes), a hold (0 <= from == to < nframes) or a step back (0 <= to < from < nframes).  That is: `to` is a
// frame of the index, and `from` is one, or -1 (before the range), or the key word.
inline bool path_pair_ok(int nframes, int from, int to, int key) {
    if (to < 0 || to >= nframes) return false;
    return from == key || (from >= -1 && from < nframes);
}

}  // namespace jsp
