// What the MSVideo1 block kernels (msv1_kernels.hip, msv1_seek_kernels.hip) share around decode_block (msv1_decode.h): a block's row
// loads and stores, the look-before-OR of a significance word, the pixels no block covers, the palette prologue, the decode of a
// code in global memory, the seek index's block rule (index_block) with its last-writer walk, and the host's BITS x VEC dispatch.
#pragma once
#include <type_traits>

#include "msv1_decode.h"
#include "msv1_seek.h"

namespace jsp {
namespace {

// (dst/prev reach some kernels inside a struct read from memory: without the explicit global address space the accesses would be
// FLAT instructions)
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) u32x4 gu32x4;
typedef const __attribute__((address_space(1))) u32x4 cgu32x4;
typedef __attribute__((address_space(1))) uint32_t gu32;
typedef const __attribute__((address_space(1))) uint32_t cgu32;

// Frame rows are written once and never read back by the launch: nontemporal stores keep them from evicting the stream / descriptor
// lines out of L2 (measured: 168 -> 91 us per 64-frame batch together with msv1_blocks_kernel's LDS staging, tools/msv1_lab.hip).
__device__ __forceinline__ void store_row(uint32_t* p, uint32_t a, uint32_t b, uint32_t c, uint32_t d) {
    __builtin_nontemporal_store(u32x4{a, b, c, d}, (gu32x4*)p);
}
__device__ __forceinline__ uint4 load_row(const uint32_t* p) {
    const u32x4 v = *(cgu32x4*)p;
    return make_uint4(v.x, v.y, v.z, v.w);
}

// The 4x4 block at `p` of a picture X pixels wide: four 16-byte rows (VEC: X % 4 == 0 and a 16-byte aligned picture), else 16 dwords.
template <bool VEC>
__device__ __forceinline__ void load_block(const uint32_t* __restrict__ p, int X, uint32_t (&px)[16]) {
#pragma unroll
    for (int y = 0; y < 4; ++y) {
        if (VEC) {
            const u32x4 r = *(cgu32x4*)(p + (size_t)y * X);
            px[y * 4] = r.x; px[y * 4 + 1] = r.y; px[y * 4 + 2] = r.z; px[y * 4 + 3] = r.w;
        } else {
#pragma unroll
            for (int x = 0; x < 4; ++x) px[y * 4 + x] = *(cgu32*)(p + (size_t)y * X + x);
        }
    }
}
template <bool VEC>
__device__ __forceinline__ void store_block(uint32_t* __restrict__ p, int X, const uint32_t (&px)[16]) {
#pragma unroll
    for (int y = 0; y < 4; ++y) {
        if (VEC) {
            __builtin_nontemporal_store(u32x4{px[y * 4], px[y * 4 + 1], px[y * 4 + 2], px[y * 4 + 3]}, (gu32x4*)(p + (size_t)y * X));
        } else {
#pragma unroll
            for (int x = 0; x < 4; ++x) *(gu32*)(p + (size_t)y * X + x) = px[y * 4 + x];
        }
    }
}

// OR 1 into a significance word that thousands of waves share.  They would serialise on the address (measured: 24 us per inter frame,
// almost all of it there), so look before setting — a relaxed agent-scope load is enough, a stale 0 only costs one more atomic.
// Wave form: every lane of the wave calls it, the first lane with `diff` acts for all.  Lane form: the lane acts for itself.
__device__ __forceinline__ void raise_flag(uint32_t* word, bool diff) {
    if (__ballot(diff) != 0ull && (threadIdx.x & 63) == __ffsll((long long)__ballot(diff)) - 1 &&
        __hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0u)
        atomicOr(word, 1u);
}
__device__ __forceinline__ void raise_flag_lane(uint32_t* word, bool diff) {
    if (diff && __hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0u) atomicOr(word, 1u);
}

// Work-items past the last block take one pixel each that no block covers (the X % 4 / Y % 4 remainders): pixel index of the r-th
// such pixel — the right strip [0, cy) x [cx, X) first, then the rows [cy, Y).
__device__ __forceinline__ size_t uncovered_pixel(long r, int X, int cx, int cy) {
    const long rw = (long)(X - cx) * cy;
    return r < rw ? (size_t)(r / (X - cx)) * (size_t)X + (size_t)cx + (size_t)(r % (X - cx)) : (size_t)cy * (size_t)X + (size_t)(r - rw);
}

// 8-bit: the palette into LDS, an entry per work-item — called by 256 of them (s_pal has one entry for 16-bit, which never reads it).
// BARRIER = false: the kernel has a workgroup barrier of its own before the first decode.
template <int BITS, bool BARRIER = true>
__device__ __forceinline__ void load_palette(uint32_t* s_pal, const int32_t* __restrict__ palette) {
    if (BITS == 8) s_pal[threadIdx.x] = (uint32_t)palette[threadIdx.x];
    if (BITS == 8 && BARRIER) __syncthreads();
}

// The 16 pixels of the code at `o` of a frame in global memory whose data ends at `stream_end` (MSVideo1.hx:135-181 / 319-364; bytes
// past the end read as missing, which the reference turns into 0).  The rule for a code that the end cuts off — half a code word
// paints solid from its first byte, a code wholly past the end paints 0 — is also written out in msv1_blocks_temporal_kernel's
// workers, which have the bytes in LDS: every way tried of stating it once for both moved instructions in one kernel or the other.
template <int BITS>
__device__ __forceinline__ void decode_at(const uint8_t* __restrict__ stream, uint32_t o, uint32_t stream_end, const uint32_t* s_pal,
                                          uint32_t (&px)[16]) {
    // 16-bit: `end` counts whole words and a code word cut in two (only its first byte exists) is painted solid from that byte
    const uint32_t end = BITS == 16 ? (stream_end & ~1u) : stream_end;
    const uint32_t avail = end > o ? end - o : 0u;
    const bool half = BITS == 16 ? ((stream_end & 1u) && o == end) : avail == 1u;
    if (half) {
        const uint32_t a = stream[BITS == 16 ? stream_end - 1u : o];
        const uint32_t v = BITS == 16 ? rgb555(a) : s_pal[a];
#pragma unroll
        for (int k = 0; k < 16; ++k) px[k] = v;
        return;
    }
    if (avail == 0u) {
#pragma unroll
        for (int k = 0; k < 16; ++k) px[k] = 0u;
        return;
    }
    // o is even (codes are whole words from a 16-byte aligned frame start): six aligned dwords from o & ~3 hold the 20 bytes
    // decode_block may read; every dword lies inside the batch's stream buffer (64 bytes of slack past its last frame)
    const uint32_t a0 = o & ~3u;
    uint32_t w[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const uint32_t at = a0 + 4u * (uint32_t)k;
        const uint32_t v = at < end ? *(cgu32*)(stream + at) : 0u;
        const uint32_t have = end - at;   // bytes of this dword that are data (when at < end)
        w[k] = at >= end ? 0u : (have >= 4u ? v : v & ((1u << (8u * have)) - 1u));
    }
    const uint32_t sh = (o & 2u) * 8u;
    uint32_t cw[5];
#pragma unroll
    for (int k = 0; k < 5; ++k) cw[k] = __builtin_amdgcn_alignbit(w[k + 1], w[k], sh);
    decode_block<BITS>(reinterpret_cast<const uint8_t*>(cw), avail, s_pal, px);
}

// ---- the seek index (Msv1IndexSrc, msv1_seek.h): what its kernels — show, play, thumbnails, present, tensor — share ----------------
// The 16 pixels frame f of the index makes of block `blk`, which it codes: its chunk (frame_chunk[], chunks[]) gives the table
// entry and the stream.
template <int BITS>
__device__ __forceinline__ void index_decode(const Msv1IndexSrc& s, int f, int blk, const uint32_t* s_pal, uint32_t (&px)[16]) {
    const Msv1IndexChunk ch = s.chunks[s.frame_chunk[f]];
    const int lf = f - (int)ch.first;
    const uint32_t o = *(cgu32*)(ch.desc + (size_t)lf * s.pitch + blk);
    decode_at<BITS>(ch.stream, o, ch.frames[lf].stream_end, s_pal, px);
}

constexpr int INDEX_SCAN = 4;   // bitmap words a lane has in flight per step of its walk down (msv1_seek_kernels.hip's SCAN is this)

// The frame that the non-zero masked bitmap word `m`, word `w` of its block, names: its highest set bit.
__device__ __forceinline__ int index_word_frame(int w, uint32_t m) { return 32 * w + 31 - __builtin_clz(m); }

// The bitmap word of block `blk` that holds the last frame <= t coding it, masked to the frames <= t (index_word_frame(w, m) is that
// frame; w is set), or 0 when nothing up to t coded the block.  Word t / 32 first, then the words below it, INDEX_SCAN in flight
// per step.
__device__ __forceinline__ uint32_t index_last_writer(const Msv1IndexSrc& s, int blk, int t, int& w) {
    w = t >> 5;
    uint32_t m = *(cgu32*)(s.bitmap + (size_t)w * (size_t)s.nblocks + blk) & (0xFFFFFFFFu >> (31 - (t & 31)));
    while (m == 0u && w > 0) {
        uint32_t e[INDEX_SCAN];
#pragma unroll
        for (int k = 0; k < INDEX_SCAN; ++k) e[k] = w - 1 - k >= 0 ? *(cgu32*)(s.bitmap + (size_t)(w - 1 - k) * (size_t)s.nblocks + blk) : 0u;
        int step = INDEX_SCAN;
#pragma unroll
        for (int k = INDEX_SCAN - 1; k >= 0; --k)
            if (e[k] != 0u) { m = e[k]; step = k + 1; }
        w -= step;
    }
    return m;
}

// THE BLOCK RULE of a seek index.  Block `blk` (block column bx, block row by) of the picture of index frame t is what the last
// frame <= t that coded it makes of it, decoded from its code; else the block of the picture before the index; else nothing: px[]
// is zeros then, and the result false (the block is not defined — Show and Play leave the destination alone, the kernels that
// have no destination picture use the zeros).  before_vec: the block of `before` is read 16 bytes a row (a constant where the caller
// has one: the branch folds away).
template <int BITS>
__device__ __forceinline__ bool index_block(const Msv1IndexSrc& s, int t, int blk, int bx, int by, bool before_vec, const uint32_t* s_pal,
                                            uint32_t (&px)[16]) {
    int w;
    const uint32_t m = index_last_writer(s, blk, t, w);
    if (m != 0u) {
        index_decode<BITS>(s, index_word_frame(w, m), blk, s_pal, px);
        return true;
    }
    if (s.before != nullptr) {
        const uint32_t* p = s.before + (size_t)by * 4u * (size_t)s.X + (size_t)bx * 4u;
        if (before_vec) load_block<true>(p, s.X, px);
        else load_block<false>(p, s.X, px);
        return true;
    }
#pragma unroll
    for (int i = 0; i < 16; ++i) px[i] = 0u;
    return false;
}

// Host: f(std::integral_constant<int, BITS>{}, std::bool_constant<VEC>{}) for the kernel instantiation that `bits` (16, else 8) and
// `vec` (rows move 16 bytes at a time) select.
template <class F>
inline void dispatch_bits_vec(int bits, bool vec, F&& f) {
    if (bits == 16) {
        if (vec) f(std::integral_constant<int, 16>{}, std::true_type{});
        else f(std::integral_constant<int, 16>{}, std::false_type{});
    } else {
        if (vec) f(std::integral_constant<int, 8>{}, std::true_type{});
        else f(std::integral_constant<int, 8>{}, std::false_type{});
    }
}

}  // namespace
}  // namespace jsp
