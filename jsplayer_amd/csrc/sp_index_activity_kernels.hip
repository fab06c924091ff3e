// Activity map of a ScreenPressor seek index for gfx950 (MI355X): for a run of frames, how many pixels of every 16x16 block each frame
// changed (jsp_sp_index_activity) — ONE launch, no picture written anywhere.  Host side in sp_index.cpp; sp_index_kernels.hip has the
// index's layout.
//
// THE PICTURE P(t) is jsp_sp_index_present's (what jsp_sp_index_show(t) writes); P(-1) is zeros.  out[(k * nby + by) * nbx + bx] = the
// pixels of block (bx, by), clipped to the picture, whose word differs between P(first + k) and P(first + k - 1): the grid of cells is
// the codec's own grid of blocks.
//
// Geometry: sp_index_play_kernel's — a wave per 16x16 block, lane = (row, 4-pixel chunk), four neighbouring blocks to a workgroup.  The
// wave composes P(first - 1) of its block (index_compose; zeros for first = 0) and walks FORWARD over the frames first .. last with its
// four pixels in registers.  Per 32 frames it reads one bitmap word of its block and one word of the key-frame mask (the block number is
// wave-uniform: scalar loads) and visits only the events, in frame order:
//   a set bitmap bit   the frame's record and PBlock (scalar loads); a lane counts its pixels inside the rectangle and inside the
//                      picture whose literal differs from the register, then takes the literal.  The rectangle is the bounding box of
//                      a change and literalised motion rewrites unchanged pixels: a pixel under the rectangle need not have changed.
//   a key frame        (a key frame sets no bitmap bit) a lane counts its pixels inside the picture that differ from the key picture,
//                      and reloads them from it.
// The wave's count is four ballots and population counts — wave-uniform, no LDS, no barrier — and its first lane stores it, with a
// vector store through a global pointer, when it is not 0.  The host zeroes `out` in front of the launch.
#include <hip/hip_runtime.h>

#include "sp_index_activity.h"
#include "sp_index_compose.h"

namespace jsp::sp {
namespace {

using namespace index_walk;

constexpr int ACT_WG = 256;   // four waves = four neighbouring blocks

typedef __attribute__((address_space(1))) uint16_t act_gu16;

template <bool VEC>
__global__ __launch_bounds__(ACT_WG) void sp_index_activity_kernel(uint16_t* __restrict__ out, const uint32_t* __restrict__ keys,
                                                                   const IndexPlayFrame* __restrict__ frames,
                                                                   const uint32_t* __restrict__ keymask, const uint4* __restrict__ blocks,
                                                                   const uint32_t* __restrict__ payload, const uint32_t* __restrict__ bitmap,
                                                                   long pic_stride, int first, int last, int X, int Y, int nbx, int nblocks) {
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int lane = threadIdx.x & 63;
    const int bx = (int)blockIdx.x * 4 + wave, by = (int)blockIdx.y;
    if (bx >= nbx) return;   // (wave-uniform)
    const int b = by * nbx + bx;
    const int ly = lane >> 2, cx0 = (lane & 3) * 4;
    const int y = by * 16 + ly, x0 = bx * 16 + cx0;
    const bool mine = y < Y && x0 < X;
    const size_t i0 = (size_t)y * (size_t)X + (size_t)x0;
    uint32_t inpic = 0;   // bit j: pixel j of the chunk is inside the picture
    if (mine) {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (VEC || x0 + j < X) inpic |= 1u << j;
    }

    uint32_t px[4] = {0u, 0u, 0u, 0u};   // P(first - 1); pixels outside the picture stay 0 and are never counted
    if (first > 0) {
        const IndexPlayFrame r0 = frames[first - 1];
        index_compose<VEC>(px, keys + (size_t)r0.key_slot * (size_t)pic_stride, blocks, payload, bitmap, first - 1, r0.k, (long)r0.slot_base, X,
                           nblocks, b, ly, cx0, x0, i0, mine);
    }

    for (int w = first >> 5; w <= (last >> 5); ++w) {
        const int lo = first > 32 * w ? first : 32 * w, hi = last < 32 * w + 31 ? last : 32 * w + 31;
        const uint32_t range = (0xFFFFFFFFu << (lo & 31)) & (0xFFFFFFFFu >> (31 - (hi & 31)));
        const uint32_t m = bitmap[(size_t)w * (size_t)nblocks + b] & range;
        const uint32_t km = keymask[w] & range;
        uint32_t ev = m | km;
        while (ev != 0u) {
            const int bit = __builtin_ctz(ev);
            const uint32_t one = 1u << bit;
            ev &= ev - 1u;
            const int f = 32 * w + bit;
            uint32_t diff = 0;   // bit j: pixel j of the chunk changes at frame f
            if (m & one) {
                const IndexPlayFrame rf = frames[f];
                const Rect r = unpack(blocks[((size_t)((long)f + (long)rf.slot_base)) * (size_t)nblocks + b]);
                if (inpic != 0u && (uint32_t)ly >= r.y1 && (uint32_t)ly < r.y2) {
                    const uint32_t* lit = payload + (size_t)r.payload16 * 4 + (size_t)(((uint32_t)ly - r.y1) * (r.x2 - r.x1));
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const uint32_t rx = (uint32_t)(cx0 + j);
                        if (((inpic >> j) & 1u) && rx >= r.x1 && rx < r.x2) {
                            const uint32_t v = lit[rx - r.x1];
                            if (v != px[j]) diff |= 1u << j;
                            px[j] = v;
                        }
                    }
                }
            } else {
                const uint32_t* key = keys + (size_t)frames[f].key_slot * (size_t)pic_stride;
                if (mine) {
                    uint32_t kx[4] = {px[0], px[1], px[2], px[3]};
                    if (VEC) {
                        const uint4 q = *reinterpret_cast<const uint4*>(key + i0);
                        kx[0] = q.x; kx[1] = q.y; kx[2] = q.z; kx[3] = q.w;
                    } else {
#pragma unroll
                        for (int j = 0; j < 4; ++j)
                            if (x0 + j < X) kx[j] = key[i0 + j];
                    }
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        if (kx[j] != px[j]) diff |= 1u << j;
                        px[j] = kx[j];
                    }
                }
            }
            uint32_t cnt = 0;   // (the loop and both branches above are wave-uniform: every lane of the wave takes part in the ballots)
#pragma unroll
            for (int j = 0; j < 4; ++j) cnt += (uint32_t)__popcll(__ballot((diff >> j) & 1u));
            if (lane == 0 && cnt != 0u) *(act_gu16*)(out + (size_t)(f - first) * (size_t)nblocks + (size_t)b) = (uint16_t)cnt;
        }
    }
}

}  // namespace

void launch_index_activity(const Geometry& g, uint16_t* out, int first, int n, const int32_t* d_keys, size_t pic_stride,
                           const IndexPlayFrame* d_frames, const uint32_t* d_keymask, const PBlock* d_blocks, const uint32_t* d_payload,
                           const uint32_t* d_bitmap, hipStream_t stream) {
    if (n <= 0 || g.nbx <= 0 || g.nby <= 0) return;
    const bool vec = (g.X & 3) == 0 && (reinterpret_cast<uintptr_t>(d_keys) & 15) == 0 && (pic_stride & 3) == 0;
    const dim3 grid((g.nbx + 3) / 4, g.nby);
    const int nblocks = g.nbx * g.nby, last = first + n - 1;
#define JSP_SP_ACTIVITY(VEC)                                                                                                              \
    hipLaunchKernelGGL(sp_index_activity_kernel<VEC>, grid, dim3(ACT_WG), 0, stream, out, reinterpret_cast<const uint32_t*>(d_keys), d_frames, \
                       d_keymask, reinterpret_cast<const uint4*>(d_blocks), d_payload, d_bitmap, (long)pic_stride, first, last, g.X, g.Y,   \
                       g.nbx, nblocks)
    if (vec) JSP_SP_ACTIVITY(true);
    else JSP_SP_ACTIVITY(false);
#undef JSP_SP_ACTIVITY
}

}  // namespace jsp::sp
