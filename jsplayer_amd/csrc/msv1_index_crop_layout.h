// Host arithmetic of jsp_index_crop_frames (msv1_seek.cpp) that needs neither HIP nor the codec: the check of a block rectangle
// against the block grid and src(j); the parts of the scratch: msv1_index_clip_layout.h.  Plain C++, so that a program of its own
// can run it under a sanitizer.
#pragma once
#include <cstddef>
#include <cstdint>

namespace jsp {

// Whether (bx, by, bw, bh) is a rectangle of a grid of nbx x nby blocks: bw, bh >= 1, 0 <= bx, bx + bw <= nbx, 0 <= by,
// by + bh <= nby (no sum is formed that could overflow).  A grid without a block has no rectangle.
inline bool crop_rect_ok(int nbx, int nby, int bx, int by, int bw, int bh) {
    return nbx >= 1 && nby >= 1 && bw >= 1 && bh >= 1 && bx >= 0 && by >= 0 && bw <= nbx && bh <= nby && bx <= nbx - bw && by <= nby - bh;
}

// Source block of block j of the rectangle, 0 <= j < bw * bh (THE RULE: msv1_index_crop_kernels.hip).
inline int64_t crop_src_block(int nbx, int bx, int by, int bw, int64_t j) {
    return ((int64_t)by + j / bw) * nbx + bx + j % bw;
}

}  // namespace jsp
