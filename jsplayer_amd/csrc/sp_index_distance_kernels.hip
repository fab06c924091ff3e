// Distance map of a ScreenPressor seek index for gfx950 (MI355X): for a run of frames, how many pixels of every 16x16 block differ from
// a FIXED reference picture R (jsp_sp_index_distance) — ONE launch, no picture written anywhere.  Host side in sp_index.cpp;
// sp_index_kernels.hip has the index's layout.
//
// THE PICTURE P(t), P(-1) = zeros and the grid are sp_index_activity_kernel's (sp_index_activity_kernels.hip).  R is P(ref_frame),
// ref_frame -1 .. nframes - 1, composed here (index_compose), or a device picture `ref` of X * Y words in frame-buffer layout, which is
// only read.  out[(k * nby + by) * nbx + bx] = the pixels of block (bx, by), clipped to the picture, whose word differs between
// P(first + k) and R.
//
// Geometry: the activity kernel's — a wave per 16x16 block, lane = (row, 4-pixel chunk), four neighbouring blocks to a workgroup.  A lane
// keeps its four words of R and ONE MISMATCH BIT per pixel; it has no pixel registers of its own.  It composes P(first) of its chunk
// once (index_compose) and sets the bits.  It then walks FORWARD over the events of the frames first + 1 .. last, in frame order:
//   a set bitmap bit   the lane recomputes the bits of its pixels inside the record's rectangle and inside the picture, from the literals
//                      (a pixel outside the rectangle keeps its word, so its bit);
//   a key frame        (a key frame sets no bitmap bit) the lane recomputes all of its pixels inside the picture, from the key picture.
// The wave's count is four ballots and population counts — wave-uniform, no LDS, no barrier.  It is stored for EVERY frame of the run,
// repeated where the block has no event: the launch writes every element of the map, the host zeroes nothing.  The repeats of a block go
// out 64 frames to a store, a lane of the wave each.
#include <hip/hip_runtime.h>

#include "sp_index_activity.h"
#include "sp_index_compose.h"

namespace jsp::sp {
namespace {

using namespace index_walk;

constexpr int DIST_WG = 256;   // four waves = four neighbouring blocks

typedef __attribute__((address_space(1))) uint16_t dist_gu16;

// The wave's count of set mismatch bits: every lane of the wave takes part.
__device__ __forceinline__ uint32_t wave_count(uint32_t bad) {
    uint32_t cnt = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) cnt += (uint32_t)__popcll(__ballot((bad >> j) & 1u));
    return cnt;
}

template <bool VEC>
__global__ __launch_bounds__(DIST_WG) void sp_index_distance_kernel(uint16_t* __restrict__ out, int ref_frame, const uint32_t* __restrict__ ref,
                                                                    int ref_vec, const uint32_t* __restrict__ keys,
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

    uint32_t rx[4] = {0u, 0u, 0u, 0u};   // R; pixels outside the picture stay 0 and are never counted
    if (ref != nullptr) {
        if (mine) {
            if (ref_vec) {               // (X % 4 == 0: the chunk is whole)
                const uint4 q = *reinterpret_cast<const uint4*>(ref + i0);
                rx[0] = q.x; rx[1] = q.y; rx[2] = q.z; rx[3] = q.w;
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if ((inpic >> j) & 1u) rx[j] = ref[i0 + j];
            }
        }
    } else if (ref_frame >= 0) {
        const IndexPlayFrame rr = frames[ref_frame];
        index_compose<VEC>(rx, keys + (size_t)rr.key_slot * (size_t)pic_stride, blocks, payload, bitmap, ref_frame, rr.k, (long)rr.slot_base, X,
                           nblocks, b, ly, cx0, x0, i0, mine);
    }

    uint32_t bad = 0;   // bit j: pixel j of the chunk differs from R in the frame the walk stands at
    {
        uint32_t px[4];
        const IndexPlayFrame r0 = frames[first];
        index_compose<VEC>(px, keys + (size_t)r0.key_slot * (size_t)pic_stride, blocks, payload, bitmap, first, r0.k, (long)r0.slot_base, X, nblocks,
                           b, ly, cx0, x0, i0, mine);
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (((inpic >> j) & 1u) && px[j] != rx[j]) bad |= 1u << j;
    }
    uint32_t cnt = wave_count(bad);
    dist_gu16* const cell = (dist_gu16*)(out + (size_t)b);   // the block's element of frame `first`
    if (lane == 0) cell[0] = (uint16_t)cnt;
    int done = first;                                        // the frames up to here have their element

    for (int w = (first + 1) >> 5; first < last && w <= (last >> 5); ++w) {
        const int lo = first + 1 > 32 * w ? first + 1 : 32 * w, hi = last < 32 * w + 31 ? last : 32 * w + 31;
        const uint32_t range = (0xFFFFFFFFu << (lo & 31)) & (0xFFFFFFFFu >> (31 - (hi & 31)));
        const uint32_t m = bitmap[(size_t)w * (size_t)nblocks + b] & range;
        const uint32_t km = keymask[w] & range;
        uint32_t ev = m | km;
        while (ev != 0u) {
            const int bit = __builtin_ctz(ev);
            const uint32_t one = 1u << bit;
            ev &= ev - 1u;
            const int f = 32 * w + bit;
            for (int t = done + 1 + lane; t < f; t += 64) cell[(size_t)(t - first) * (size_t)nblocks] = (uint16_t)cnt;   // the value repeats
            if (m & one) {
                const IndexPlayFrame rf = frames[f];
                const Rect r = unpack(blocks[((size_t)((long)f + (long)rf.slot_base)) * (size_t)nblocks + b]);
                if (inpic != 0u && (uint32_t)ly >= r.y1 && (uint32_t)ly < r.y2) {
                    const uint32_t* lit = payload + (size_t)r.payload16 * 4 + (size_t)(((uint32_t)ly - r.y1) * (r.x2 - r.x1));
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const uint32_t rxj = (uint32_t)(cx0 + j);
                        if (((inpic >> j) & 1u) && rxj >= r.x1 && rxj < r.x2)
                            bad = (bad & ~(1u << j)) | ((lit[rxj - r.x1] != rx[j] ? 1u : 0u) << j);
                    }
                }
            } else {
                const uint32_t* key = keys + (size_t)frames[f].key_slot * (size_t)pic_stride;
                if (mine) {
                    if (VEC) {
                        const uint4 q = *reinterpret_cast<const uint4*>(key + i0);
                        bad = (q.x != rx[0] ? 1u : 0u) | (q.y != rx[1] ? 2u : 0u) | (q.z != rx[2] ? 4u : 0u) | (q.w != rx[3] ? 8u : 0u);
                    } else {
                        bad = 0u;
#pragma unroll
                        for (int j = 0; j < 4; ++j)
                            if (x0 + j < X && key[i0 + j] != rx[j]) bad |= 1u << j;
                    }
                }
            }
            cnt = wave_count(bad);   // (the loop and both branches above are wave-uniform: every lane of the wave takes part in the ballots)
            if (lane == 0) cell[(size_t)(f - first) * (size_t)nblocks] = (uint16_t)cnt;
            done = f;
        }
    }
    for (int t = done + 1 + lane; t <= last; t += 64) cell[(size_t)(t - first) * (size_t)nblocks] = (uint16_t)cnt;
}

}  // namespace

void launch_index_distance(const Geometry& g, uint16_t* out, int ref_frame, const int32_t* ref_picture, int first, int n, const int32_t* d_keys,
                           size_t pic_stride, const IndexPlayFrame* d_frames, const uint32_t* d_keymask, const PBlock* d_blocks,
                           const uint32_t* d_payload, const uint32_t* d_bitmap, hipStream_t stream) {
    if (n <= 0 || g.nbx <= 0 || g.nby <= 0) return;
    const bool vec = (g.X & 3) == 0 && (reinterpret_cast<uintptr_t>(d_keys) & 15) == 0 && (pic_stride & 3) == 0;
    const auto* ref = reinterpret_cast<const uint32_t*>(ref_picture);
    const int ref_vec = ref != nullptr && (g.X & 3) == 0 && (reinterpret_cast<uintptr_t>(ref) & 15) == 0;
    const dim3 grid((g.nbx + 3) / 4, g.nby);
    const int nblocks = g.nbx * g.nby, last = first + n - 1;
#define JSP_SP_DISTANCE(VEC)                                                                                                                  \
    hipLaunchKernelGGL(sp_index_distance_kernel<VEC>, grid, dim3(DIST_WG), 0, stream, out, ref_frame, ref, ref_vec,                             \
                       reinterpret_cast<const uint32_t*>(d_keys), d_frames, d_keymask, reinterpret_cast<const uint4*>(d_blocks), d_payload,    \
                       d_bitmap, (long)pic_stride, first, last, g.X, g.Y, g.nbx, nblocks)
    if (vec) JSP_SP_DISTANCE(true);
    else JSP_SP_DISTANCE(false);
#undef JSP_SP_DISTANCE
}

}  // namespace jsp::sp
