// Distance map of an MSVideo1 seek index for gfx950 (MI355X): for a run of frames, how many pixels of every 16x16 cell differ from a
// FIXED reference picture R (jsp_index_distance) — ONE launch, no picture written anywhere.  Host side in msv1_seek.cpp.
//
// THE PICTURE P(t), P(-1) and the grid are msv1_index_activity_kernel's (msv1_index_activity_kernels.hip).  R is P(ref_frame), ref_frame
// -1 .. nframes - 1, composed here block by block (index_block; `before` or zeros for -1), or a device picture `ref` of X * Y words in
// frame-buffer layout, which is only read.  out[(k * rows + r) * cols + q] = the pixels of cell (r, q), inside whole 4x4 blocks, whose
// word differs between P(first + k) and R.  The X % 4 / Y % 4 remainder pixels are never read, of `ref` neither.
//
// Geometry: the activity kernel's, unchanged — a lane per 4x4 block, the 16 lanes of a cell consecutive, every cell of the grid
// enumerated, dead lanes of edge cells contribute 0 and still reach every shuffle, blockIdx.y a SEGMENT of the run.
//
// The walk: the lane keeps the 16 words of R's block in registers, and the count of its block; it has no "current picture".  It composes
// its block of P(t0) for the segment's first frame t0 (index_block) and counts.  It then reads the block's bitmap words over the frames
// t0 + 1 .. t1 of the segment, ORed over the cell's 16 lanes as Activity does, so that the 16 lanes visit the same frames.  At a visited
// frame a lane whose own bit is set decodes that frame's code and recounts against R.  The 16 counts are added with __shfl_xor (no LDS, no
// barrier) and the sum is stored for the visited frame — and for every frame between two visited frames, where the cell's value simply
// repeats: the launch writes EVERY element of the map, the host zeroes nothing.  The repeats of a cell go out 16 frames to a store, a lane
// of the group each.
#include "msv1_block_io.h"

namespace jsp {
namespace {

constexpr int WG = 256;

typedef __attribute__((address_space(1))) uint16_t gu16;

__device__ __forceinline__ uint32_t differing(const uint32_t (&a)[16], const uint32_t (&b)[16]) {
    uint32_t cnt = 0;
#pragma unroll
    for (int i = 0; i < 16; ++i) cnt += a[i] != b[i] ? 1u : 0u;
    return cnt;
}

// The sum of `cnt` over the 16 lanes of a cell (a group is aligned to 16 lanes and calls this as one).
__device__ __forceinline__ uint32_t cell_sum(uint32_t cnt) {
#pragma unroll
    for (int d = 1; d < 16; d <<= 1) cnt += (uint32_t)__shfl_xor((int)cnt, d);
    return cnt;
}

template <int BITS>
__global__ __launch_bounds__(WG) void msv1_index_distance_kernel(const Msv1IndexSrc s, int ref_frame, const uint32_t* __restrict__ ref, int ref_vec,
                                                                 int first, int n, int seg, uint16_t* __restrict__ out, int cols, int rows) {
    __shared__ uint32_t s_pal[BITS == 8 ? 256 : 1];
    load_palette<BITS>(s_pal, s.palette);
    const long gid = (long)blockIdx.x * WG + threadIdx.x;
    const long q = gid >> 4;                                        // cell of the grid, raster order
    // The tail of the last workgroup: whole groups of 16 leave, as in msv1_index_activity_kernel (behind the palette barrier).
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

    uint32_t rx[16];                                                // R's block
#pragma unroll
    for (int i = 0; i < 16; ++i) rx[i] = 0u;
    uint32_t cnt = 0;                                               // the pixels of the lane's block that differ from R (a dead lane: 0)
    if (live) {
        if (ref != nullptr) {
            const uint32_t* p = ref + (size_t)by * 4u * (size_t)s.X + (size_t)bx * 4u;
            if (ref_vec) load_block<true>(p, s.X, rx);
            else load_block<false>(p, s.X, rx);
        } else if (ref_frame >= 0) {
            index_block<BITS>(s, ref_frame, blk, bx, by, s.before_vec != 0, s_pal, rx);
        } else if (s.before != nullptr) {                           // P(-1): the picture before the index (else the zeros above)
            const uint32_t* p = s.before + (size_t)by * 4u * (size_t)s.X + (size_t)bx * 4u;
            if (s.before_vec) load_block<true>(p, s.X, rx);
            else load_block<false>(p, s.X, rx);
        }
        uint32_t px[16];
        index_block<BITS>(s, t0, blk, bx, by, s.before_vec != 0, s_pal, px);
        cnt = differing(px, rx);
    }
    uint32_t sum = cell_sum(cnt);
    gu16* const cell = (gu16*)(out + (size_t)r * (size_t)cols + (size_t)qx);   // the cell's element of frame `first`
    const size_t pitch = (size_t)rows * (size_t)cols;                         // elements from a frame to the next
    if (sub == 0) cell[(size_t)k0 * pitch] = (uint16_t)sum;
    int done = t0;                                                  // the frames up to here have their element

    for (int w = (t0 + 1) >> 5; t0 < t1 && w <= (t1 >> 5); ++w) {
        const int lo = max(t0 + 1, 32 * w), hi = min(t1, 32 * w + 31);
        const uint32_t range = (0xFFFFFFFFu << (lo & 31)) & (0xFFFFFFFFu >> (31 - (hi & 31)));
        const uint32_t mine = live ? *(cgu32*)(s.bitmap + (size_t)w * (size_t)s.nblocks + blk) & range : 0u;
        uint32_t any = mine;                                        // the frames of this word that code a block of the cell
#pragma unroll
        for (int d = 1; d < 16; d <<= 1) any |= (uint32_t)__shfl_xor((int)any, d);
        while (any != 0u) {
            const int f = 32 * w + __builtin_ctz(any);
            any &= any - 1u;
            for (int t = done + 1 + sub; t < f; t += 16) cell[(size_t)(t - first) * pitch] = (uint16_t)sum;   // the value repeats
            if ((mine >> (f & 31)) & 1u) {
                uint32_t nx[16];
                index_decode<BITS>(s, f, blk, s_pal, nx);
                cnt = differing(nx, rx);
            }
            sum = cell_sum(cnt);
            if (sub == 0) cell[(size_t)(f - first) * pitch] = (uint16_t)sum;
            done = f;
        }
    }
    for (int t = done + 1 + sub; t <= t1; t += 16) cell[(size_t)(t - first) * pitch] = (uint16_t)sum;
}

}  // namespace

void msv1_launch_index_distance(const Msv1IndexSrc& src, int ref_frame, const int32_t* ref_picture, int first, int n, int segs, uint16_t* out,
                                int cols, int rows, hipStream_t stream) {
    if (n <= 0 || cols <= 0 || rows <= 0) return;
    const int nseg = std::min(std::max(segs, 1), n);
    const int seg = (n + nseg - 1) / nseg;                          // frames per segment
    const long lanes = (long)cols * rows * 16;
    const dim3 grid((unsigned)((lanes + WG - 1) / WG), (unsigned)((n + seg - 1) / seg));
    const auto* ref = reinterpret_cast<const uint32_t*>(ref_picture);
    const int ref_vec = ref != nullptr && (src.X & 3) == 0 && (reinterpret_cast<uintptr_t>(ref) & 15) == 0;
    if (src.bits == 16)
        hipLaunchKernelGGL(msv1_index_distance_kernel<16>, grid, dim3(WG), 0, stream, src, ref_frame, ref, ref_vec, first, n, seg, out, cols, rows);
    else
        hipLaunchKernelGGL(msv1_index_distance_kernel<8>, grid, dim3(WG), 0, stream, src, ref_frame, ref, ref_vec, first, n, seg, out, cols, rows);
}

}  // namespace jsp
