// Host arithmetic of jsp_index_crop_frames (msv1_seek.cpp) that needs neither HIP nor the codec: the check of a block rectangle
// against the block grid, src(j), and the parts of the scratch for a slice of pairs.  Plain C++, so that a program of its own can
// run it under a sanitizer.
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

// The parts of the scratch for slices of S pairs of a rectangle of nb blocks (nwg workgroups, `bound` bytes a frame), each
// 16-byte aligned; the host's pinned side has the parts before records_at at the same offsets.
struct CropLayout {
    size_t pairs_at, bases_at, status_at, totals_at, counts_at, first_at, records_at, out_at, bytes;
};
inline CropLayout crop_layout(size_t S, size_t nb, size_t nwg, size_t bound) {
    const auto up16 = [](size_t n) { return (n + 15) & ~(size_t)15; };
    CropLayout l{};
    l.pairs_at = 0;
    l.bases_at = l.pairs_at + up16(2 * sizeof(int32_t) * S);
    l.status_at = l.bases_at + up16(sizeof(uint64_t) * S);
    l.totals_at = l.status_at + up16(sizeof(uint32_t) * S);
    l.counts_at = l.totals_at + up16(sizeof(uint32_t) * S * nwg);
    l.first_at = l.counts_at + up16(sizeof(uint32_t) * S * nwg);
    l.records_at = l.first_at + up16(sizeof(uint32_t) * S * nwg);
    l.out_at = l.records_at + up16(2 * sizeof(uint32_t) * S * nb);
    l.bytes = l.out_at + S * bound;
    return l;
}

}  // namespace jsp
