// An MSVideo1 16-bit ENCODER for gfx950 (MI355X): the stream bytes of key and inter frames from pictures in device memory
// (jsp_msv1_encode_frames) — TWO launches per slice of pictures, grid.y = the picture, no workgroup ever waits for another, no atomics
// on global memory.  Host side in msv1_encode.cpp.  The clip calls of a seek index (msv1_index_clip_device.h) gather codes a stream
// already holds; this makes codes from pixels, for everything that exists only as pixels.
//
// THE RULE (the decoder it inverts: MSVideo1.hx:119-181).  A picture is width x height 32-bit words, row y at base + y * pitch ints,
// pitch signed.  nbx = width >> 2, nby = height >> 2; blocks in table order, block row 0 is rows 0..3; pixel k = 4 y + x of a block is
// flag bit k; the width % 4 / height % 4 remainder pixels are never read.
//   q(p) = ((p >> 3) & 0x1F) | ((p >> 6) & 0x3E0) | ((p >> 9) & 0x7C00): the inverse of fromRGB15 on 0x00RRGGBB.  No other bit of a
//   word is read.  v[k] = q(p[k]).
//   Quadrant i of 0..3 holds pixels {0,1,4,5}, {2,3,6,7}, {8,9,12,13}, {10,11,14,15}; its last pixel is 5, 7, 13, 15; its colour pair
//   is stream colours 2i (taken where the code word's bit is SET) and 2i + 1 (where it is CLEAR).
//   The code of a block, decided on v alone:
//     1. all 16 equal c: the two bytes of 0x8000 | c when (c & 0x7C00) != 0x0400; otherwise (the word's high byte would be 0x84..0x87,
//        a skip) the six bytes 00 00, c, c — a two-colour code of one colour;
//     2. exactly two distinct values: B = v[15], A the other; the word has bit k set where v[k] == A (bit 15 is clear by
//        construction), then A, B: six bytes, A with bit 15 clear;
//     3. otherwise 18 bytes: the word, then F0 | 0x8000, S0, F1, S1, F2, S2, F3, S3.  Per quadrant —
//        at most two distinct values: S = the value of the quadrant's last pixel, F the other (F = S when there is one), bits set
//          where v[k] != S;
//        three or four distinct values (the only lossy step): Y = R + 2 G + B of the 5-bit fields, T the sum of the four Y, a pixel is
//          high when 4 Y > T; the last pixel's group is the pixels on its side of that test; S = per channel floor((sum + n / 2) / n)
//          over that group (n / 2 in integers), F the same over the other group (F = S when it is empty); bits set for the other group.
//   Key(P) = the codes of blocks 0 .. nblocks-1; no skip word, no end marker.  Inter(Q, P): block i is CODED when v of P differs from
//   v of Q in at least one of its 16 pixels (quantised values are compared, not words); the frame is Delta's rule
//   (msv1_index_delta_kernels.hip) with "written" read as "coded": the run-head test, the count, never crossing a multiple of 1023,
//   ceil(nblocks / 1023) skip words when nothing changed.
//
// The shape is the clip calls': a lane owns ENC_LANE_BLOCKS consecutive blocks, a workgroup ENC_WG_BLOCKS.
//   Sizes, msv1_encode_sizes_kernel.  Per block: its 16 words (VEC: four 16-byte rows; else 16 scalar words) and, for an inter frame,
//     the 16 of the picture before; the verdict coded / not; the classification without divergence — B = v[15], A = the first value that
//     differs from B, then "all in {A, B}" — and so L in {2, 6, 18}; the code itself, which goes into the block's slot.  The run-head
//     test: block j - 1 is the lane's own previous block, else the neighbour lane's last block through LDS, else (the workgroup's
//     first block) a look of its own.  An exclusive scan of the contributions (L, 2 for a run head, 0) gives every block its offset;
//     per picture and workgroup go out the total and the first coded block.
//   Gather, msv1_encode_gather_kernel.  Workgroup g of a picture starts at bases[picture] + totals[picture][0 .. g).  The codes go
//     from their slots into an LDS image, the run heads' counts come from the workgroup's coded mask and first_coded of the next two
//     workgroups (1022 blocks ahead never reach further); the image leaves in 16-byte pieces.
//   The codes are KEPT by the sizes launch (20 bytes a block at most), not rebuilt from the pixels: the gather then reads 4 + L bytes
//   a block in place of 64 (128 for an inter frame) and does not classify a second time.
// Lanes with j >= nb touch nothing.
#include "msv1_encode.h"
#include "msv1_index_codes.h"

namespace jsp {
namespace {

constexpr int WG = INDEX_CODES_WG;
constexpr int ENC_LANE_BLOCKS = 4;
constexpr int ENC_WG_BLOCKS = MSV1_KEYFRAME_WG_BLOCKS;   // (msv1_seek.h: the host sizes totals[] and first_coded[] by it)
static_assert(ENC_WG_BLOCKS == WG * ENC_LANE_BLOCKS, "a lane owns ENC_LANE_BLOCKS consecutive blocks");
static_assert(2 * ENC_WG_BLOCKS >= MSV1_DELTA_RUN, "a count's look-ahead ends within the next two workgroups");
static_assert(MSV1_ENCODE_SLOT_WORDS == 5, "a slot holds the word and eight colours");

__device__ __forceinline__ uint32_t quantise(uint32_t p) { return ((p >> 3) & 0x1Fu) | ((p >> 6) & 0x3E0u) | ((p >> 9) & 0x7C00u); }

// v[] of the 4x4 block at `p` of a picture whose rows lie `pitch` ints apart.
template <bool VEC>
__device__ __forceinline__ void load_values(const int32_t* p, ptrdiff_t pitch, uint32_t (&v)[16]) {
#pragma unroll
    for (int y = 0; y < 4; ++y) {
        const int32_t* row = p + (ptrdiff_t)y * pitch;
        if (VEC) {
            const u32x4 r = *(cgu32x4*)row;
            v[y * 4] = quantise(r.x); v[y * 4 + 1] = quantise(r.y); v[y * 4 + 2] = quantise(r.z); v[y * 4 + 3] = quantise(r.w);
        } else {
#pragma unroll
            for (int x = 0; x < 4; ++x) v[y * 4 + x] = quantise(*(cgu32*)(row + x));
        }
    }
}

// Whether the block at offset `at` of picture `pic` is CODED against `prev` (null: a key frame codes every block); v[] = the picture's.
template <bool VEC>
__device__ __forceinline__ bool block_coded(const int32_t* pic, const int32_t* prev, ptrdiff_t at, ptrdiff_t pitch, uint32_t (&v)[16]) {
    load_values<VEC>(pic + at, pitch, v);
    if (prev == nullptr) return true;
    uint32_t u[16], diff = 0u;
    load_values<VEC>(prev + at, pitch, u);
#pragma unroll
    for (int k = 0; k < 16; ++k) diff |= u[k] ^ v[k];
    return diff != 0u;
}

// floor(x / n) for n in 1..4 and x < 512 (171 / 512 = 1/3 + 1/1536: exact below 512).
__device__ __forceinline__ uint32_t div_small(uint32_t x, uint32_t n) { return n == 3u ? (x * 171u) >> 9 : x >> (n >> 1); }

// One quadrant of an 18-byte code — pixels K0, K1, K2 and its last pixel K3: F, S and the bits of the word it sets.
template <int K0, int K1, int K2, int K3>
__device__ __forceinline__ uint32_t encode_quadrant(const uint32_t (&v)[16], uint32_t& F, uint32_t& S) {
    const uint32_t a = v[K0], b = v[K1], c = v[K2], d = v[K3];
    S = d;
    F = c != d ? c : d;
    F = b != d ? b : F;
    F = a != d ? a : F;
    if ((a == d || a == F) && (b == d || b == F) && (c == d || c == F))
        return ((uint32_t)(a != d) << K0) | ((uint32_t)(b != d) << K1) | ((uint32_t)(c != d) << K2);
    const uint32_t px[4] = {a, b, c, d};
    uint32_t y[4], T = 0u;
#pragma unroll
    for (int n = 0; n < 4; ++n) {
        y[n] = (px[n] & 0x1Fu) + 2u * ((px[n] >> 5) & 0x1Fu) + ((px[n] >> 10) & 0x1Fu);
        T += y[n];
    }
    const bool side = 4u * y[3] > T;
    uint32_t sum[2][3] = {{0u, 0u, 0u}, {0u, 0u, 0u}}, n_mine = 0u, other = 0u;   // sum[0]: the last pixel's group
#pragma unroll
    for (int n = 0; n < 4; ++n) {
        const bool mine = (4u * y[n] > T) == side;
        n_mine += mine ? 1u : 0u;
        other |= mine ? 0u : 1u << n;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const uint32_t f = (px[n] >> (5 * ch)) & 0x1Fu;
            sum[0][ch] += mine ? f : 0u;
            sum[1][ch] += mine ? 0u : f;
        }
    }
    const uint32_t n_other = 4u - n_mine;
    S = 0u;
    F = 0u;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        S |= div_small(sum[0][ch] + (n_mine >> 1), n_mine) << (5 * ch);
        F |= div_small(sum[1][ch] + (n_other >> 1), n_other == 0u ? 1u : n_other) << (5 * ch);
    }
    if (n_other == 0u) F = S;
    return ((other & 1u) << K0) | (((other >> 1) & 1u) << K1) | (((other >> 2) & 1u) << K2) | (((other >> 3) & 1u) << K3);
}

// The code of the block with values v[]: its length L, and its bytes in slot[0 .. L / 4] (little-endian words: the code word | colour
// 0 << 16, then two colours a word).
__device__ __forceinline__ uint32_t encode_block(const uint32_t (&v)[16], uint32_t (&slot)[MSV1_ENCODE_SLOT_WORDS]) {
    const uint32_t B = v[15];
    uint32_t A = B;
#pragma unroll
    for (int k = 14; k >= 0; --k) A = v[k] != B ? v[k] : A;              // the FIRST value that differs from B
    bool two = true;
    uint32_t word = 0u;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        two = two && (v[k] == A || v[k] == B);
        word |= (uint32_t)(v[k] != B) << k;
    }
    if (A == B && (B & 0x7C00u) != 0x0400u) {
        slot[0] = 0x8000u | B;
        return 2u;
    }
    if (two) {                                                           // (A == B: the two-colour code of one colour, word 0)
        slot[0] = word | (A << 16);
        slot[1] = B;
        return 6u;
    }
    uint32_t c[8];
    word = encode_quadrant<0, 1, 4, 5>(v, c[0], c[1]);
    word |= encode_quadrant<2, 3, 6, 7>(v, c[2], c[3]);
    word |= encode_quadrant<8, 9, 12, 13>(v, c[4], c[5]);
    word |= encode_quadrant<10, 11, 14, 15>(v, c[6], c[7]);
    slot[0] = word | ((c[0] | 0x8000u) << 16);
    slot[1] = c[1] | (c[2] << 16);
    slot[2] = c[3] | (c[4] << 16);
    slot[3] = c[5] | (c[6] << 16);
    slot[4] = c[7];
    return 18u;
}

template <bool VEC>
__global__ __launch_bounds__(WG) void msv1_encode_sizes_kernel(const Msv1EncodeArgs a) {
    __shared__ uint32_t s_wave[WG / 64];
    __shared__ uint32_t s_first[WG / 64];
    __shared__ uint8_t s_last[WG];                       // per lane: its last block is coded
    const int pic = (int)blockIdx.y, nwg = (int)gridDim.x, nb = a.nb;
    const int32_t* picture = a.pictures[pic];
    const int32_t* previous = a.previous[pic];
    const int j0 = (int)blockIdx.x * ENC_WG_BLOCKS + (int)threadIdx.x * ENC_LANE_BLOCKS;
    int by = j0 / a.nbx, bx = j0 - by * a.nbx;           // the ONE division per lane
    uint32_t* slots = a.slots + ((size_t)pic * (size_t)nb + (size_t)j0) * MSV1_ENCODE_SLOT_WORDS;
    uint32_t len[ENC_LANE_BLOCKS], first = MSV1_DELTA_NONE;
    bool coded[ENC_LANE_BLOCKS];
#pragma unroll
    for (int i = 0; i < ENC_LANE_BLOCKS; ++i) {
        const int j = j0 + i;
        len[i] = 0u;
        coded[i] = false;
        if (j >= nb) continue;
        uint32_t v[16];
        coded[i] = block_coded<VEC>(picture, previous, (ptrdiff_t)(4 * by) * a.pitch + 4 * bx, a.pitch, v);
        if (coded[i]) {
            first = min(first, (uint32_t)j);
            uint32_t slot[MSV1_ENCODE_SLOT_WORDS];
            len[i] = encode_block(v, slot);
            uint32_t* s = slots + i * MSV1_ENCODE_SLOT_WORDS;
            *(gu32*)s = slot[0];
            if (len[i] >= 6u) *(gu32*)(s + 1) = slot[1];
            if (len[i] == 18u) {
                *(gu32*)(s + 2) = slot[2];
                *(gu32*)(s + 3) = slot[3];
                *(gu32*)(s + 4) = slot[4];
            }
        }
        if (++bx == a.nbx) {
            bx = 0;
            ++by;
        }
    }

    // the block before the lane's first one: the neighbour lane's last block; the workgroup's first lane looks for itself
    s_last[threadIdx.x] = coded[ENC_LANE_BLOCKS - 1] ? 1 : 0;
    bool before = true;                                  // (block 0 is a run head: as if a coded block stood before it)
    if (threadIdx.x == 0 && previous != nullptr && j0 > 0 && j0 < nb) {   // (a key frame has no run heads: nothing to look for)
        const int pby = (j0 - 1) / a.nbx, pbx = j0 - 1 - pby * a.nbx;
        uint32_t v[16];
        before = block_coded<VEC>(picture, previous, (ptrdiff_t)(4 * pby) * a.pitch + 4 * pbx, a.pitch, v);
    }
    __syncthreads();
    if (threadIdx.x > 0) before = s_last[threadIdx.x - 1] != 0;
#pragma unroll
    for (int i = 0; i < ENC_LANE_BLOCKS; ++i) {
        const int j = j0 + i;
        if (j < nb && !coded[i] && (before || j % MSV1_DELTA_RUN == 0)) len[i] = MSV1_DELTA_SKIP;
        before = coded[i];
    }

    // exclusive scan of the contributions over the workgroup; its first coded block
    uint32_t mine = 0u;
#pragma unroll
    for (int i = 0; i < ENC_LANE_BLOCKS; ++i) mine += len[i] == MSV1_DELTA_SKIP ? 2u : len[i];
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
#pragma unroll
    for (int k = 1; k < 64; k <<= 1) first = min(first, (uint32_t)__shfl_xor((int)first, k));
    if (lane == 0) s_first[wave] = first;
    uint32_t total;
    uint32_t off = index_wg_scan(mine, s_wave, total);   // (its barrier also publishes s_first)
    uint32_t* records = a.records + (size_t)pic * (size_t)nb;
#pragma unroll
    for (int i = 0; i < ENC_LANE_BLOCKS; ++i) {
        const int j = j0 + i;
        if (j < nb) *(gu32*)(records + j) = (off << 8) | len[i];
        off += len[i] == MSV1_DELTA_SKIP ? 2u : len[i];
    }
    if (threadIdx.x == 0) {
        uint32_t f0 = s_first[0];
#pragma unroll
        for (int w = 1; w < WG / 64; ++w) f0 = min(f0, s_first[w]);
        *(gu32*)(a.totals + (size_t)pic * nwg + blockIdx.x) = total;
        *(gu32*)(a.first_coded + (size_t)pic * nwg + blockIdx.x) = f0;
    }
}

// After a sizes launch over the same pictures, with bases[] = the running sums of the pictures' lengths: the frames into a.out.
__global__ __launch_bounds__(WG) void msv1_encode_gather_kernel(const Msv1EncodeArgs a) {
    constexpr int IMAGE = ENC_WG_BLOCKS * 18;                                    // bytes of a workgroup's output at its bound
    __shared__ __attribute__((aligned(16))) uint16_t s_img[(IMAGE + 16) / 2];   // (+ 16: the image starts base % 16 bytes in)
    __shared__ uint32_t s_wave[WG / 64];
    __shared__ uint32_t s_mask[ENC_WG_BLOCKS / 32];                              // bit k of word w: block 32 w + k of the workgroup is coded
    const int pic = (int)blockIdx.y, nwg = (int)gridDim.x, g = (int)blockIdx.x, nb = a.nb;
    const uint32_t* totals = a.totals + (size_t)pic * nwg;
    const uint32_t* records = a.records + (size_t)pic * (size_t)nb;
    if (threadIdx.x < ENC_WG_BLOCKS / 32) s_mask[threadIdx.x] = 0u;
    const size_t base = (size_t)a.bases[pic] + index_wg_bytes_before(totals, g, s_wave);   // (its barrier also publishes the zeroed mask)
    const uint32_t total = *(cgu32*)(totals + g);
    const uint32_t lo = (uint32_t)(base & 15), hi = lo + total;                  // the image is s_img bytes [lo, hi)

    const int j0 = g * ENC_WG_BLOCKS + (int)threadIdx.x * ENC_LANE_BLOCKS;
    const uint32_t* slots = a.slots + ((size_t)pic * (size_t)nb + (size_t)j0) * MSV1_ENCODE_SLOT_WORDS;
    uint32_t ol[ENC_LANE_BLOCKS], bits4 = 0u;
#pragma unroll
    for (int i = 0; i < ENC_LANE_BLOCKS; ++i) {
        const int j = j0 + i;
        ol[i] = j < nb ? *(cgu32*)(records + j) : 0u;
        const uint32_t L = ol[i] & 0xFFu, at = lo + (ol[i] >> 8);
        if (L >= 2u && at + L <= hi) {                                          // (else nothing or a run head; the second test always holds)
            bits4 |= 1u << i;
            const uint32_t* s = slots + i * MSV1_ENCODE_SLOT_WORDS;
            uint32_t w[MSV1_ENCODE_SLOT_WORDS];
#pragma unroll
            for (int k = 0; k < MSV1_ENCODE_SLOT_WORDS; ++k) w[k] = 4u * (uint32_t)k < L ? *(cgu32*)(s + k) : 0u;
#pragma unroll
            for (int k = 0; k < 9; ++k)
                if (2u * (uint32_t)k < L) s_img[(at >> 1) + k] = (uint16_t)(w[k >> 1] >> (16 * (k & 1)));
        }
    }
    if (bits4 != 0u) atomicOr(&s_mask[threadIdx.x >> 3], bits4 << (ENC_LANE_BLOCKS * (threadIdx.x & 7)));
    __syncthreads();

    // the run heads: count = up to the next coded block, the next multiple of 1023, nb
#pragma unroll
    for (int i = 0; i < ENC_LANE_BLOCKS; ++i) {
        if ((ol[i] & 0xFFu) != MSV1_DELTA_SKIP) continue;
        const int j = j0 + i;
        const uint32_t at = lo + (ol[i] >> 8);
        if (at + 2u > hi) continue;                                             // (never holds)
        const int q = (int)threadIdx.x * ENC_LANE_BLOCKS + i + 1;               // the first block behind the head, within the workgroup
        uint32_t next = MSV1_DELTA_NONE;
        for (int w = q >> 5; w < ENC_WG_BLOCKS / 32 && next == MSV1_DELTA_NONE; ++w) {
            uint32_t m = s_mask[w];
            if (w == (q >> 5)) m &= 0xFFFFFFFFu << (q & 31);
            if (m != 0u) next = (uint32_t)(g * ENC_WG_BLOCKS + 32 * w + __builtin_ctz(m));
        }
        for (int k = g + 1; k <= g + 2 && k < nwg && next == MSV1_DELTA_NONE; ++k) next = *(cgu32*)(a.first_coded + (size_t)pic * nwg + k);
        const uint32_t limit = min((uint32_t)(j / MSV1_DELTA_RUN + 1) * (uint32_t)MSV1_DELTA_RUN, (uint32_t)nb);
        const uint32_t count = min(next, limit) - (uint32_t)j;
        s_img[at >> 1] = (uint16_t)((count & 0xFFu) | ((0x84u + (count >> 8)) << 8));
    }
    __syncthreads();

    index_image_store(a.out + (base - lo), s_img, lo, hi);                       // (a.out is 16-byte aligned, so is this)
}

}  // namespace

void msv1_launch_encode_sizes(const Msv1EncodeArgs& a, int npictures, bool vec, hipStream_t stream) {
    if (a.nb <= 0 || npictures <= 0) return;
    const dim3 grid((unsigned)msv1_keyframe_workgroups(a.nb), (unsigned)npictures);
    if (vec) hipLaunchKernelGGL(msv1_encode_sizes_kernel<true>, grid, dim3(WG), 0, stream, a);
    else hipLaunchKernelGGL(msv1_encode_sizes_kernel<false>, grid, dim3(WG), 0, stream, a);
}

void msv1_launch_encode_gather(const Msv1EncodeArgs& a, int npictures, hipStream_t stream) {
    if (a.nb <= 0 || npictures <= 0) return;
    const dim3 grid((unsigned)msv1_keyframe_workgroups(a.nb), (unsigned)npictures);
    hipLaunchKernelGGL(msv1_encode_gather_kernel, grid, dim3(WG), 0, stream, a);
}

}  // namespace jsp
