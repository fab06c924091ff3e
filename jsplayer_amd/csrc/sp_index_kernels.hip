// ScreenPressor seek index: frame t of a resident range in ONE launch (jsp_sp_index_show), and the thumbnails of any n frames of it in
// ONE launch (jsp_sp_index_thumbs), and a run of frames played forward from any frame of it in ONE launch (jsp_sp_index_play, at the end
// of the file); host side in sp_index.cpp.
//
// Every inter frame of the index is literalised (HostDecoder::literalise_motion): no block reads the picture before it anywhere but at
// its own position.  Pixel p of frame t is therefore the literal of the LAST frame in (k, t] whose changed rectangle covers p, else
// pixel p of the key picture k.  The index keeps, in HBM: the key pictures, one 16-byte PBlock per inter frame and 16x16 block, the
// literal pixels, and a changed-block bitmap (bitmap[w * nblocks + b], bit j: frame 32 w + j changes block b).
//
// One WAVE per 16x16 block, lane = (row, 4-pixel chunk); a workgroup is four neighbouring blocks, so its four waves together store
// 256 contiguous bytes per row.  The lane loads its 4 pixels of the key picture first (most blocks of a desktop clip need nothing
// else), then the wave walks the block's bitmap words DOWN from t / 32 to the word of frame k + 1, most recent frame first.  The
// block number is wave-uniform, so bitmap words and PBlocks come through the scalar path; the records of up to four set bits are
// fetched together before the first is applied.  A lane keeps a 4-bit mask of the pixels no rectangle has covered yet and takes
// literals only for those; the wave stops when a ballot says nothing is left uncovered.  No LDS, no barrier.
#include <hip/hip_runtime.h>

#include "sp_index_compose.h"   // Rect, unpack, index_compose: shared with sp_index_present_kernels.hip

namespace jsp::sp {
namespace {

using namespace index_walk;

constexpr int SHOW_WG = 256;   // four waves = four neighbouring blocks

template <bool VEC>
__global__ __launch_bounds__(SHOW_WG) void sp_index_show_kernel(uint32_t* __restrict__ dst, const uint32_t* __restrict__ key,
                                                                const uint4* __restrict__ blocks, const uint32_t* __restrict__ payload,
                                                                const uint32_t* __restrict__ bitmap, int t, int k, long slot_base,
                                                                int X, int Y, int nbx, int nblocks) {
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int lane = threadIdx.x & 63;
    const int bx = (int)blockIdx.x * 4 + wave, by = (int)blockIdx.y;
    if (bx >= nbx) return;
    const int b = by * nbx + bx;
    const int ly = lane >> 2, cx0 = (lane & 3) * 4;   // row and first column inside the block
    const int y = by * 16 + ly, x0 = bx * 16 + cx0;
    const bool mine = y < Y && x0 < X;
    const size_t i0 = (size_t)y * (size_t)X + (size_t)x0;
    uint32_t px[4];
    index_compose<VEC>(px, key, blocks, payload, bitmap, t, k, slot_base, X, nblocks, b, ly, cx0, x0, i0, mine);
    if (!mine) return;
    if (VEC) *reinterpret_cast<uint4*>(dst + i0) = make_uint4(px[0], px[1], px[2], px[3]);
    else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (x0 + j < X) dst[i0 + j] = px[j];
    }
}

// Thumbnails (jsp_sp_index_thumbs): the pictures of n frames of the index, each reduced S x S pixels to one (box mean per byte, rounded
// half up), into one sheet — ONE launch, no full-size picture anywhere.  blockIdx.z is the thumbnail, recs[blockIdx.z] its frame; a
// wave composes one 16x16 block of it exactly as the show kernel does (index_compose) and then holds the block in registers, four
// pixels per lane.  A lane adds its four pixels — R and B together under 0x00FF00FF, G apart: at S = 16 a field ends at
// 256 * 255 + 128 < 2^16, so the fields never carry into each other — which is one S = 4 cell's row; lanes are (row << 2 | chunk), so
// __shfl_xor by 4 and 8 adds the cell's four rows (16 cells a block), by 1 and 16 on top makes 8 x 8 cells (4), by 2 and 32 the one
// 16 x 16 cell.  The first lane of each group stores one word.  S divides 16: a cell never straddles two blocks.  Lanes outside the
// picture contribute zeros and a cell is stored only when it lies inside tw x th, so a cell that is not whole is never written.  No
// LDS allocated, no barrier; every lane of a wave reaches the shuffles (a wave past the last block column leaves as a whole).
template <int S, bool VEC>
__global__ __launch_bounds__(SHOW_WG) void sp_index_thumbs_kernel(uint32_t* __restrict__ out, const uint32_t* __restrict__ keys,
                                                                  const IndexThumbRec* __restrict__ recs, const uint4* __restrict__ blocks,
                                                                  const uint32_t* __restrict__ payload, const uint32_t* __restrict__ bitmap,
                                                                  long pic_stride, int X, int Y, int nbx, int nblocks, int tw, int th,
                                                                  int cols) {
    static_assert(S == 4 || S == 8 || S == 16, "scale");
    constexpr int SH = S == 4 ? 4 : (S == 8 ? 6 : 8);   // log2(S * S)
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int lane = threadIdx.x & 63;
    const int bx = (int)blockIdx.x * 4 + wave, by = (int)blockIdx.y;
    if (bx >= nbx) return;   // (wave-uniform)
    const IndexThumbRec rec = recs[blockIdx.z];
    const int b = by * nbx + bx;
    const int ly = lane >> 2, cx0 = (lane & 3) * 4;
    const int y = by * 16 + ly, x0 = bx * 16 + cx0;
    const bool mine = y < Y && x0 < X;
    const size_t i0 = (size_t)y * (size_t)X + (size_t)x0;
    uint32_t px[4];
    index_compose<VEC>(px, keys + (size_t)rec.key_slot * (size_t)pic_stride, blocks, payload, bitmap, rec.t, rec.k, (long)rec.slot_base, X,
                       nblocks, b, ly, cx0, x0, i0, mine);
    uint32_t rb = 0, g = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        rb += px[j] & 0x00FF00FFu;
        g += (px[j] >> 8) & 0xFFu;
    }
#pragma unroll
    for (int step : {4, 8, 1, 16, 2, 32}) {
        if ((step == 1 || step == 16) && S < 8) continue;
        if ((step == 2 || step == 32) && S < 16) continue;
        rb += (uint32_t)__shfl_xor((int)rb, step);
        g += (uint32_t)__shfl_xor((int)g, step);
    }
    constexpr int GROUP = S == 4 ? 12 : (S == 8 ? 29 : 63);   // the lane bits a cell is summed over: its first lane has none set
    const int tx = x0 / S, ty = y / S;
    if ((lane & GROUP) != 0 || tx >= tw || ty >= th) return;
    rb += (uint32_t)(S * S / 2) * 0x00010001u;
    g += (uint32_t)(S * S / 2);
    const uint32_t word = (((rb >> (16 + SH)) & 0xFFu) << 16) | (((g >> SH) & 0xFFu) << 8) | (((rb & 0xFFFFu) >> SH) & 0xFFu);
    const size_t pitch = (size_t)cols * (size_t)tw;
    const size_t cell = (size_t)(blockIdx.z / (unsigned)cols) * (size_t)th * pitch + (size_t)(blockIdx.z % (unsigned)cols) * (size_t)tw;
    out[cell + (size_t)ty * pitch + (size_t)tx] = word;
}

// Playback (jsp_sp_index_play): frames first, first + stride, ..., last of the index into dsts[0 .. n) — ONE launch.  Same geometry as the
// show kernel: a wave per 16x16 block, lane = (row, 4-pixel chunk), four neighbouring blocks to a workgroup.  The wave composes frame
// `first` (index_compose), stores it, and then walks FORWARD with its four pixels in registers.  Per 32 frames it reads one bitmap word of
// its block and one word of the key-frame mask (both wave-uniform: scalar loads) and visits only the frames that write the block, are key
// frames, or are stored:
//   a set bitmap bit   the frame's record and PBlock (scalar loads), and the lanes inside the rectangle take its literals;
//   a key frame        every lane reloads its pixels from that key picture (a key frame sets no bitmap bit);
//   a stored frame     (f - first) % stride == 0: the pixels go to dsts[(f - first) / stride].
// A wave's loads queue behind its own stores, so the record and literals of the NEXT writer of the word are asked for before the current
// frame's store goes out (`Ahead`): they depend on nothing the walk computes.  No LDS, no barrier; everything is written by vector stores.
struct Ahead {   // the literals of a frame that writes the block, fetched before they are needed
    int f;              // the frame (-1: none)
    uint32_t lit[4];
    uint32_t mask;      // bit j: pixel j of the lane's chunk is inside the frame's rectangle
};

// (The destinations are pointers read from memory: with no known address space, plain stores through them would be FLAT instructions,
// which count on lgkmcnt as well as vmcnt and would tie every wait for a scalar load to the latency of the frame stores.  Say "global".)
typedef uint32_t play_u32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) uint32_t play_gu32;
typedef __attribute__((address_space(1))) play_u32x4 play_gu32x4;

template <bool VEC>
__device__ __forceinline__ void play_store(uint32_t* dst, const uint32_t (&px)[4], size_t i0, int x0, int X, bool mine) {
    if (!mine) return;
    if (VEC) *(play_gu32x4*)(dst + i0) = play_u32x4{px[0], px[1], px[2], px[3]};
    else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (x0 + j < X) *(play_gu32*)(dst + i0 + j) = px[j];
    }
}

template <bool VEC>
__global__ __launch_bounds__(SHOW_WG) void sp_index_play_kernel(uint32_t* const* __restrict__ dsts, const uint32_t* __restrict__ keys,
                                                                const IndexPlayFrame* __restrict__ frames,
                                                                const uint32_t* __restrict__ keymask, const uint4* __restrict__ blocks,
                                                                const uint32_t* __restrict__ payload, const uint32_t* __restrict__ bitmap,
                                                                long pic_stride, int first, int last, int stride, int X, int Y, int nbx,
                                                                int nblocks) {
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

    const IndexPlayFrame r0 = frames[first];
    uint32_t px[4];
    index_compose<VEC>(px, keys + (size_t)r0.key_slot * (size_t)pic_stride, blocks, payload, bitmap, first, r0.k, (long)r0.slot_base, X, nblocks,
                       b, ly, cx0, x0, i0, mine);
    play_store<VEC>(dsts[0], px, i0, x0, X, mine);
    int out_k = 1, next_out = first + stride;   // the next destination, and the frame that goes there

    Ahead ah;
    ah.f = -1;
    ah.mask = 0u;
    ah.lit[0] = ah.lit[1] = ah.lit[2] = ah.lit[3] = 0u;
    auto fetch = [&](int f) {
        const IndexPlayFrame rf = frames[f];
        const Rect r = unpack(blocks[((size_t)((long)f + (long)rf.slot_base)) * (size_t)nblocks + b]);
        ah.f = f;
        ah.mask = 0u;
        if (inpic != 0u && (uint32_t)ly >= r.y1 && (uint32_t)ly < r.y2) {
            const uint32_t* lit = payload + (size_t)r.payload16 * 4 + (size_t)(((uint32_t)ly - r.y1) * (r.x2 - r.x1));
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const uint32_t rx = (uint32_t)(cx0 + j);
                if (((inpic >> j) & 1u) && rx >= r.x1 && rx < r.x2) {
                    ah.lit[j] = lit[rx - r.x1];
                    ah.mask |= 1u << j;
                }
            }
        }
    };

    for (int w = first >> 5; w <= (last >> 5); ++w) {
        const int lo = first + 1 > 32 * w ? first + 1 : 32 * w, hi = last < 32 * w + 31 ? last : 32 * w + 31;
        if (lo > hi) continue;   // (frame `first` is the last of its word)
        const uint32_t range = (0xFFFFFFFFu << (lo & 31)) & (0xFFFFFFFFu >> (31 - (hi & 31)));
        const uint32_t m = bitmap[(size_t)w * (size_t)nblocks + b] & range;
        const uint32_t km = keymask[w] & range;
        uint32_t om = 0;                 // the frames of this word that are stored
        for (int f = next_out; f <= hi; f += stride) om |= 1u << (f & 31);
        if (m != 0u) fetch(32 * w + __builtin_ctz(m));   // the word's first writer, ahead of everything else in the word
        uint32_t ev = m | km | om;
        while (ev != 0u) {
            const int bit = __builtin_ctz(ev);
            const uint32_t one = 1u << bit;
            ev &= ev - 1u;
            const int f = 32 * w + bit;
            if (m & one) {
                if (ah.f != f) fetch(f);
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if ((ah.mask >> j) & 1u) px[j] = ah.lit[j];
                const uint32_t later = m & ~(one | (one - 1u));
                if (later != 0u) fetch(32 * w + __builtin_ctz(later));   // before this frame's store: loads queue behind stores
            } else if (km & one) {
                const uint32_t* key = keys + (size_t)frames[f].key_slot * (size_t)pic_stride;
                if (mine) {
                    if (VEC) {
                        const uint4 q = *reinterpret_cast<const uint4*>(key + i0);
                        px[0] = q.x; px[1] = q.y; px[2] = q.z; px[3] = q.w;
                    } else {
#pragma unroll
                        for (int j = 0; j < 4; ++j)
                            if (x0 + j < X) px[j] = key[i0 + j];
                    }
                }
            }
            if (om & one) {
                play_store<VEC>(dsts[out_k], px, i0, x0, X, mine);
                ++out_k;
                next_out += stride;
            }
        }
    }
}

}  // namespace

void launch_index_play(const Geometry& g, int32_t* const* d_dsts, bool dsts_aligned16, int first, int n, int stride, const int32_t* d_keys,
                       size_t pic_stride, const IndexPlayFrame* d_frames, const uint32_t* d_keymask, const PBlock* d_blocks,
                       const uint32_t* d_payload, const uint32_t* d_bitmap, hipStream_t stream) {
    const bool vec = (g.X & 3) == 0 && dsts_aligned16 && (reinterpret_cast<uintptr_t>(d_keys) & 15) == 0 && (pic_stride & 3) == 0;
    const dim3 grid((g.nbx + 3) / 4, g.nby);
    const int nblocks = g.nbx * g.nby, last = first + (n - 1) * stride;
#define JSP_SP_PLAY(VEC)                                                                                                                  \
    hipLaunchKernelGGL(sp_index_play_kernel<VEC>, grid, dim3(SHOW_WG), 0, stream, reinterpret_cast<uint32_t* const*>(d_dsts),             \
                       reinterpret_cast<const uint32_t*>(d_keys), d_frames, d_keymask, reinterpret_cast<const uint4*>(d_blocks), d_payload, \
                       d_bitmap, (long)pic_stride, first, last, stride, g.X, g.Y, g.nbx, nblocks)
    if (vec) JSP_SP_PLAY(true);
    else JSP_SP_PLAY(false);
#undef JSP_SP_PLAY
}

void launch_index_show(const Geometry& g, int32_t* dst, const int32_t* key, const PBlock* d_blocks, const uint32_t* d_payload,
                       const uint32_t* d_bitmap, int t, int k, long slot_base, hipStream_t stream) {
    const bool vec = (g.X & 3) == 0 && (reinterpret_cast<uintptr_t>(dst) & 15) == 0 && (reinterpret_cast<uintptr_t>(key) & 15) == 0;
    const dim3 grid((g.nbx + 3) / 4, g.nby);
    const int nblocks = g.nbx * g.nby;
    if (vec)
        hipLaunchKernelGGL(sp_index_show_kernel<true>, grid, dim3(SHOW_WG), 0, stream, reinterpret_cast<uint32_t*>(dst),
                           reinterpret_cast<const uint32_t*>(key), reinterpret_cast<const uint4*>(d_blocks), d_payload, d_bitmap, t, k,
                           slot_base, g.X, g.Y, g.nbx, nblocks);
    else
        hipLaunchKernelGGL(sp_index_show_kernel<false>, grid, dim3(SHOW_WG), 0, stream, reinterpret_cast<uint32_t*>(dst),
                           reinterpret_cast<const uint32_t*>(key), reinterpret_cast<const uint4*>(d_blocks), d_payload, d_bitmap, t, k,
                           slot_base, g.X, g.Y, g.nbx, nblocks);
}

void launch_index_thumbs(const Geometry& g, int32_t* out, const int32_t* d_keys, size_t pic_stride, const IndexThumbRec* d_recs, int n,
                         const PBlock* d_blocks, const uint32_t* d_payload, const uint32_t* d_bitmap, int scale, int cols,
                         hipStream_t stream) {
    const bool vec = (g.X & 3) == 0 && (reinterpret_cast<uintptr_t>(d_keys) & 15) == 0 && (pic_stride & 3) == 0;
    const dim3 grid((g.nbx + 3) / 4, g.nby, n);
    const int nblocks = g.nbx * g.nby;
#define JSP_SP_THUMBS(S, VEC)                                                                                                            \
    hipLaunchKernelGGL((sp_index_thumbs_kernel<S, VEC>), grid, dim3(SHOW_WG), 0, stream, reinterpret_cast<uint32_t*>(out),                 \
                       reinterpret_cast<const uint32_t*>(d_keys), d_recs, reinterpret_cast<const uint4*>(d_blocks), d_payload, d_bitmap, \
                       (long)pic_stride, g.X, g.Y, g.nbx, nblocks, g.X / S, g.Y / S, cols)
    if (vec) { if (scale == 4) JSP_SP_THUMBS(4, true); else if (scale == 8) JSP_SP_THUMBS(8, true); else if (scale == 16) JSP_SP_THUMBS(16, true); }
    else { if (scale == 4) JSP_SP_THUMBS(4, false); else if (scale == 8) JSP_SP_THUMBS(8, false); else if (scale == 16) JSP_SP_THUMBS(16, false); }
#undef JSP_SP_THUMBS
}

}  // namespace jsp::sp
