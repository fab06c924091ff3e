// What the stream-producing calls of an MSVideo1 seek index share — the key frame (msv1_index_keyframe_kernels.hip, which states
// when a code is WHOLE), the inter frame over a gap (msv1_index_delta_kernels.hip, which states WRITTEN and KEPT) and the frames of
// a block rectangle that stands (msv1_index_crop_kernels.hip) or moves (msv1_index_pan_kernels.hip): where a writer's code lies and how
// long it is, whether a gap writes or keeps a block, a block of a picture of the index, the workgroup's exclusive scan of byte
// counts, the sum of the workgroup totals before one's own, and the way an LDS image of a workgroup's output leaves in 16-byte
// pieces.  Workgroups of INDEX_CODES_WG lanes.
#pragma once
#include "msv1_block_io.h"

namespace jsp {
namespace {

constexpr int INDEX_CODES_WG = 256;

typedef const __attribute__((address_space(1))) uint16_t cgu16;
typedef __attribute__((address_space(1))) uint16_t gu16;

// The writer frame's chunk, and within it the offset of the code of block `blk` and the end of the frame's data.
__device__ __forceinline__ Msv1IndexChunk index_code_at(const Msv1IndexSrc& s, int f, int blk, int bits, uint32_t& o, uint32_t& e) {
    const Msv1IndexChunk ch = s.chunks[s.frame_chunk[f]];
    const int lf = f - (int)ch.first;
    o = *(cgu32*)(ch.desc + (size_t)lf * s.pitch + blk);
    const uint32_t end = ch.frames[lf].stream_end;
    e = bits == 16 ? (end & ~1u) : end;
    return ch;
}

// The length L of the code at offset o when it is WHOLE below the end e, else 0 (the code is cut off).
template <int BITS>
__device__ __forceinline__ uint32_t index_whole_length(const Msv1IndexChunk& ch, uint32_t o, uint32_t e) {
    // (o + 4 cannot wrap: o and e are offsets into one allocation; o <= e - 2 is established first)
    if (!(e >= 2u && o <= e - 2u)) return 0u;
    const uint32_t b = (uint32_t)*(cgu16*)(ch.stream + o) >> 8;
    uint32_t L = 2u;
    bool settled = true;
    if (BITS == 16) {
        if (b < 0x80u) {
            settled = e >= 4u && o <= e - 4u;
            if (settled) L = (*(cgu16*)(ch.stream + o + 2u) & 0x8000u) ? 18u : 6u;
        }
    } else {
        L = b < 0x80u ? 4u : (b >= 0x90u ? 10u : 2u);
    }
    return settled && e >= L && o <= e - L ? L : 0u;
}

// Whether block `blk` is written in (a, b], and then by which frame.
__device__ __forceinline__ bool delta_written(const Msv1IndexSrc& s, int blk, int a, int b, int& f) {
    int w;
    const uint32_t m = index_last_writer(s, blk, b, w);
    if (m == 0u) return false;
    f = index_word_frame(w, m);
    return f > a;
}

// THE TIGHT RULE's (msv1_index_delta_kernels.hip) test of block `blk`, written in (a, b] by frame f: false (dropped) when P(a) is
// defined and equals P(b).
template <int BITS>
__device__ __forceinline__ bool tight_kept(const Msv1IndexSrc& s, int blk, int a, int f, const uint32_t* s_pal) {
    uint32_t pa[16], pb[16];
    int w;
    const uint32_t m = a >= 0 ? index_last_writer(s, blk, a, w) : 0u;
    if (m != 0u) {
        index_decode<BITS>(s, index_word_frame(w, m), blk, s_pal, pa);
    } else if (s.before != nullptr) {
        const uint32_t* p = s.before + (size_t)(blk / s.nbx) * 4u * (size_t)s.X + (size_t)(blk % s.nbx) * 4u;
        if (s.before_vec) load_block<true>(p, s.X, pa);
        else load_block<false>(p, s.X, pa);
    } else {
        return true;
    }
    index_decode<BITS>(s, f, blk, s_pal, pb);
    uint32_t diff = 0u;
#pragma unroll
    for (int k = 0; k < 16; ++k) diff |= pa[k] ^ pb[k];
    return diff != 0u;
}

// P(t)[blk] of THE TIGHT RULE, or "not DEFINED", for a block whose last writer <= t is known: the 16 words frame f makes of block
// `blk`, else (f = -1: no writer) the block of the picture before the range; false, and px untouched, when neither exists.
template <int BITS>
__device__ __forceinline__ bool picture_block_of(const Msv1IndexSrc& s, int blk, int f, const uint32_t* s_pal, uint32_t (&px)[16]) {
    if (f >= 0) {
        index_decode<BITS>(s, f, blk, s_pal, px);
        return true;
    }
    if (s.before == nullptr) return false;
    const uint32_t* p = s.before + (size_t)(blk / s.nbx) * 4u * (size_t)s.X + (size_t)(blk % s.nbx) * 4u;
    if (s.before_vec) load_block<true>(p, s.X, px);
    else load_block<false>(p, s.X, px);
    return true;
}

// The same for a frame t >= -1: the last writer <= t is looked up first (t = -1: only the picture before the range can define it).
// What tight_kept asks of both ends of a gap for one block, for callers that compare two different blocks
// (msv1_index_pan_kernels.hip).
template <int BITS>
__device__ __forceinline__ bool picture_block(const Msv1IndexSrc& s, int blk, int t, const uint32_t* s_pal, uint32_t (&px)[16]) {
    int w;
    const uint32_t m = t >= 0 ? index_last_writer(s, blk, t, w) : 0u;
    return picture_block_of<BITS>(s, blk, m != 0u ? index_word_frame(w, m) : -1, s_pal, px);
}

// Exclusive scan of `mine` over the workgroup's lanes: inclusive over the wave's lanes by shuffles, the waves' sums through LDS
// (s_wave: INDEX_CODES_WG / 64 words).  Returns the sum of the lanes before this one; total = the workgroup's sum.
__device__ __forceinline__ uint32_t index_wg_scan(uint32_t mine, uint32_t* s_wave, uint32_t& total) {
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
    uint32_t incl = mine;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t up = (uint32_t)__shfl_up((int)incl, d);
        if (lane >= d) incl += up;
    }
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    uint32_t off = incl - mine;
    total = 0u;
#pragma unroll
    for (int v = 0; v < INDEX_CODES_WG / 64; ++v) {
        if (v < wave) off += s_wave[v];
        total += s_wave[v];
    }
    return off;
}

// The sum of totals[0 .. g): the bytes of the workgroups before workgroup g (s_wave as above).
__device__ __forceinline__ size_t index_wg_bytes_before(const uint32_t* totals, int g, uint32_t* s_wave) {
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
    uint32_t sum = 0u;
    for (int k = (int)threadIdx.x; k < g; k += INDEX_CODES_WG) sum += *(cgu32*)(totals + k);
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) sum += (uint32_t)__shfl_xor((int)sum, d);
    if (lane == 0) s_wave[wave] = sum;
    __syncthreads();
    size_t base = 0;
#pragma unroll
    for (int v = 0; v < INDEX_CODES_WG / 64; ++v) base += s_wave[v];
    return base;
}

// The image — bytes [lo, hi) of s_img, lo < 16 — to dst + [lo, hi), dst 16-byte aligned: whole 16-byte pieces as one store, the
// first and the last piece, where the image covers only a part, 16 bits at a time (lo and hi are even, nothing more).
__device__ __forceinline__ void index_image_store(uint8_t* dst, const uint16_t* s_img, uint32_t lo, uint32_t hi) {
    for (uint32_t c = threadIdx.x; 16u * c < hi; c += INDEX_CODES_WG) {
        const uint32_t p0 = 16u * c;
        if (p0 >= lo && p0 + 16u <= hi) {
            *(gu32x4*)(dst + p0) = *reinterpret_cast<const u32x4*>(&s_img[p0 >> 1]);
        } else {
            for (uint32_t p = max(p0, lo); p < min(p0 + 16u, hi); p += 2u) *(gu16*)(dst + p) = s_img[p >> 1];
        }
    }
}

}  // namespace
}  // namespace jsp
