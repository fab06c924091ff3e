// The walk of the ScreenPressor seek index that composes frame t of one 16x16 block (sp_index_kernels.hip has the index's layout):
// shared by the show, thumbnail and play kernels there and by sp_index_present_kernel (sp_index_present_kernels.hip).
#pragma once
#include <hip/hip_runtime.h>

#include "sp.h"

namespace jsp::sp {
namespace index_walk {

constexpr int SHOW_AHEAD = 4;  // records fetched per step of the walk

struct Rect {   // a PBlock as the walk needs it
    uint32_t x1, y1, x2, y2, payload16;   // payload16: first literal, in 16-byte units of the index's payload
};
__device__ __forceinline__ Rect unpack(const uint4 raw) {
    return Rect{(raw.x >> 8) & 0xFFu, (raw.x >> 16) & 0xFFu, raw.x >> 24, raw.y & 0xFFu, raw.w};
}

// The walk, shared by the show and the thumbnail kernel: the lane's 4 pixels of frame t of block b — row ly, columns cx0 .. cx0 + 3 of
// the block, pixel i0 of the picture — into px[].  Pixels outside the picture (`mine` false, or past column X - 1) come out as 0.
// EVERY lane of the wave must call it (the walk ends on a ballot), with wave-uniform b, t, k and slot_base.
template <bool VEC>
__device__ __forceinline__ void index_compose(uint32_t (&px)[4], const uint32_t* __restrict__ key, const uint4* __restrict__ blocks,
                                              const uint32_t* __restrict__ payload, const uint32_t* __restrict__ bitmap, int t, int k,
                                              long slot_base, int X, int nblocks, int b, int ly, int cx0, int x0, size_t i0, bool mine) {
    px[0] = px[1] = px[2] = px[3] = 0u;
    uint32_t need = 0;                                // bit j: pixel j of the chunk is inside the picture and not covered yet
    if (mine) {
        if (VEC) {                                    // (X % 4 == 0: the chunk is whole)
            const uint4 q = *reinterpret_cast<const uint4*>(key + i0);
            px[0] = q.x; px[1] = q.y; px[2] = q.z; px[3] = q.w;
            need = 0xFu;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (x0 + j < X) { px[j] = key[i0 + j]; need |= 1u << j; }
        }
    }
    if (t <= k) return;
    const int wlo = (k + 1) >> 5;
    int w = t >> 5;
    uint32_t m = bitmap[(size_t)w * (size_t)nblocks + b] & (0xFFFFFFFFu >> (31 - (t & 31)));
    bool open = true;
    while (open) {
        if (w == wlo) m &= 0xFFFFFFFFu << ((k + 1) & 31);   // frames up to k belong to the pictures before the key frame
        while (m != 0u && open) {
            // the most recent SHOW_AHEAD writers of this word: their records are fetched together, applied newest first
            int f[SHOW_AHEAD];
            uint4 raw[SHOW_AHEAD];
            int n = 0;
#pragma unroll
            for (int a = 0; a < SHOW_AHEAD; ++a) {
                f[a] = -1;
                if (m != 0u) {
                    const int bit = 31 - __builtin_clz(m);
                    m &= ~(1u << bit);
                    f[a] = 32 * w + bit;
                    raw[a] = blocks[((size_t)((long)f[a] + slot_base)) * (size_t)nblocks + b];
                    ++n;
                }
            }
#pragma unroll
            for (int a = 0; a < SHOW_AHEAD; ++a) {
                if (a < n && open) {
                    const Rect r = unpack(raw[a]);
                    if (need != 0u && (uint32_t)ly >= r.y1 && (uint32_t)ly < r.y2) {
                        const uint32_t* lit = payload + (size_t)r.payload16 * 4 + (size_t)(((uint32_t)ly - r.y1) * (r.x2 - r.x1));
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            const uint32_t rx = (uint32_t)(cx0 + j);
                            if (((need >> j) & 1u) && rx >= r.x1 && rx < r.x2) {
                                px[j] = lit[rx - r.x1];
                                need &= ~(1u << j);
                            }
                        }
                    }
                    open = __ballot(need != 0u) != 0ull;   // every pixel of the block has its last writer: done
                }
            }
        }
        if (w == wlo) break;
        --w;
        m = bitmap[(size_t)w * (size_t)nblocks + b];
    }
}

}  // namespace index_walk
}  // namespace jsp::sp
