// Activity map of an MSVideo1 seek index for gfx950 (MI355X): for a run of frames, how many pixels of every 16x16 cell each frame
// changed (jsp_index_activity) — ONE launch, no picture written anywhere.  Host side in msv1_seek.cpp.
//
// THE PICTURE P(t) is jsp_index_present's (index_block, msv1_block_io.h: the last frame <= t that coded the block, else the picture
// before the index, else zeros); P(-1) is the picture before the index, else zeros.  out[(k * rows + r) * cols + q] = the pixels of
// cell (r, q) whose word differs between P(first + k) and P(first + k - 1).  The X % 4 / Y % 4 remainder pixels are the same in every
// P(t) and are never read.
//
// Geometry: a lane per 4x4 block, 256 to a workgroup.  The 16 blocks of one cell are 16 consecutive lanes (lane & 3 the block column,
// the next two bits the block row inside the cell, as msv1_index_thumbs_kernel arranges S = 16), cells in raster order of the grid: a
// wave is four neighbouring cells of a grid row.  Unlike the thumbnails every cell of ceil(X / 16) x ceil(Y / 16) is enumerated: a lane
// of an edge cell whose block lies outside the picture owns nothing, contributes 0 and still reaches every shuffle.  blockIdx.y is a
// SEGMENT of the run (frames [y * seg, (y + 1) * seg) of it).
//
// The walk: the lane composes its block of P(t0 - 1) for its segment's first frame t0 (index_block; `before` or zeros for t0 = 0) and
// keeps the 16 pixels in registers.  It then reads the block's bitmap words over the segment, masked to the segment's frames.  The
// words of a cell's 16 lanes are ORed with __shfl_xor, so the 16 lanes visit the same frames — those that code any block of the cell —
// in the same order; a frame no block of the cell is coded in costs nothing.  At a visited frame a lane whose own bit is set decodes
// that frame's code (index_decode), counts the pixels that differ from its 16 and keeps the new 16; the counts are added over the 16
// lanes with __shfl_xor (no LDS, no barrier; a group is aligned to 16 lanes and loops as one) and the group's first lane stores the
// sum when it is not 0.  The host zeroes `out` in front of the launch: every cell has one owner, nothing is accumulated in memory.
#include "msv1_block_io.h"

namespace jsp {
namespace {

constexpr int WG = 256;

typedef __attribute__((address_space(1))) uint16_t gu16;

template <int BITS>
__global__ __launch_bounds__(WG) void msv1_index_activity_kernel(const Msv1IndexSrc s, int first, int n, int seg, uint16_t* __restrict__ out,
                                                                 int cols, int rows) {
    __shared__ uint32_t s_pal[BITS == 8 ? 256 : 1];
    load_palette<BITS>(s_pal, s.palette);
    const long gid = (long)blockIdx.x * WG + threadIdx.x;
    const long q = gid >> 4;                                        // cell of the grid, raster order
    // The tail of the last workgroup: q is the same for the 16 lanes of a group, so whole groups leave — up to 15 of the workgroup's
    // 16, one to three of a wave's four while the rest of the wave goes on.  The shuffles below stay inside a group (xor 1..8).
    // (After load_palette: every lane of the workgroup loads its palette entry and reaches the barrier behind it.)
    if (q >= (long)cols * rows) return;
    const int sub = (int)(gid & 15);
    const int r = (int)(q / cols);
    const int qx = (int)(q - (long)r * cols);
    const int by = r * 4 + (sub >> 2);
    const int bx = qx * 4 + (sub & 3);
    const bool live = by < s.nby && bx < s.nbx;                     // the lane has a block inside the picture
    const int blk = live ? by * s.nbx + bx : 0;
    const int k0 = (int)blockIdx.y * seg;
    const int k1 = min(n, k0 + seg);
    const int t0 = first + k0, t1 = first + k1 - 1;                 // the segment's frames, both ends included

    uint32_t px[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) px[i] = 0u;
    if (live) {
        if (t0 > 0) index_block<BITS>(s, t0 - 1, blk, bx, by, s.before_vec != 0, s_pal, px);
        else if (s.before != nullptr) {                             // P(-1): the picture before the index (else the zeros above)
            const uint32_t* p = s.before + (size_t)by * 4u * (size_t)s.X + (size_t)bx * 4u;
            if (s.before_vec) load_block<true>(p, s.X, px);
            else load_block<false>(p, s.X, px);
        }
    }

    for (int w = t0 >> 5; w <= (t1 >> 5); ++w) {
        const int lo = max(t0, 32 * w), hi = min(t1, 32 * w + 31);
        const uint32_t range = (0xFFFFFFFFu << (lo & 31)) & (0xFFFFFFFFu >> (31 - (hi & 31)));
        const uint32_t mine = live ? *(cgu32*)(s.bitmap + (size_t)w * (size_t)s.nblocks + blk) & range : 0u;
        uint32_t any = mine;                                        // the frames of this word that code a block of the cell
#pragma unroll
        for (int d = 1; d < 16; d <<= 1) any |= (uint32_t)__shfl_xor((int)any, d);
        while (any != 0u) {
            const int bit = __builtin_ctz(any);
            any &= any - 1u;
            uint32_t cnt = 0;
            if ((mine >> bit) & 1u) {
                uint32_t nx[16];
                index_decode<BITS>(s, 32 * w + bit, blk, s_pal, nx);
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    cnt += nx[i] != px[i] ? 1u : 0u;
                    px[i] = nx[i];
                }
            }
#pragma unroll
            for (int d = 1; d < 16; d <<= 1) cnt += (uint32_t)__shfl_xor((int)cnt, d);
            if (sub == 0 && cnt != 0u) *(gu16*)(out + ((size_t)(32 * w + bit - first) * (size_t)rows + (size_t)r) * (size_t)cols + (size_t)qx) = (uint16_t)cnt;
        }
    }
}

}  // namespace

void msv1_launch_index_activity(const Msv1IndexSrc& src, int first, int n, int segs, uint16_t* out, int cols, int rows, hipStream_t stream) {
    if (n <= 0 || cols <= 0 || rows <= 0) return;
    const int nseg = std::min(std::max(segs, 1), n);
    const int seg = (n + nseg - 1) / nseg;                          // frames per segment
    const long lanes = (long)cols * rows * 16;
    const dim3 grid((unsigned)((lanes + WG - 1) / WG), (unsigned)((n + seg - 1) / seg));
    if (src.bits == 16) hipLaunchKernelGGL(msv1_index_activity_kernel<16>, grid, dim3(WG), 0, stream, src, first, n, seg, out, cols, rows);
    else hipLaunchKernelGGL(msv1_index_activity_kernel<8>, grid, dim3(WG), 0, stream, src, first, n, seg, out, cols, rows);
}

}  // namespace jsp
