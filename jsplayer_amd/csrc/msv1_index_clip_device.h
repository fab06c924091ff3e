// The skeleton of the clip calls of an MSVideo1 seek index — the inter frame over a gap (msv1_index_delta_kernels.hip), the frames of
// a block rectangle that stands (msv1_index_crop_kernels.hip), moves (msv1_index_pan_kernels.hip) or is walked along any path
// (msv1_index_path_kernels.hip) — stated ONCE: src(j), the body of a sizes kernel, the body of a gather kernel and the launch of
// either.  Those files state their rules and keep their kernels; a kernel there is its rule plus a call of a body here.  The
// key frame (msv1_index_keyframe_kernels.hip) has one frame, no pairs and no run heads, and stays on its own.
//
// The shape, grid.y = the pair, no workgroup ever waits for another.  A frame has nb blocks in j-numbering; block j is source block
// src(j).  A lane owns CLIP_LANE_BLOCKS consecutive blocks j, a workgroup CLIP_WG_BLOCKS.
//   Sizes.  Per block: the rule's verdict — coded or not, and from which writer frame — then L or the status; the run-head test —
//     block j - 1 is the lane's own previous block, else the neighbour lane's last block through LDS, else (the workgroup's first
//     block) a look of its own by the same rule.  An exclusive scan of the contributions (L, 2 for a run head, 0; in the upper half of
//     the scanned word the number of codes) gives every block its offset within the workgroup's output; per pair and workgroup go
//     out the total, the first coded block and, for a rule that asks for it, the number of coded blocks.
//   Gather.  Workgroup g of pair p starts at bases[p] + totals[p][0 .. g).  Codes travel through an LDS image and leave in 16-byte
//     pieces.  The count of a run head: the next coded block from an LDS bitmask of the workgroup's records, beyond the workgroup from
//     first_written of the next two workgroups (1022 blocks ahead never reach further), clipped by the multiple of 1023 and by nb.
// Lanes with j >= nb touch nothing, and no lane forms a source block for such a j.
#pragma once
#include <type_traits>

#include "msv1_index_codes.h"

namespace jsp {
namespace {

constexpr int CLIP_LANE_BLOCKS = 4;
constexpr int CLIP_WG_BLOCKS = MSV1_KEYFRAME_WG_BLOCKS;   // (msv1_seek.h: the host sizes totals[], first_written[] and counts[] by it)
static_assert(CLIP_WG_BLOCKS == INDEX_CODES_WG * CLIP_LANE_BLOCKS, "a lane owns CLIP_LANE_BLOCKS consecutive blocks");
static_assert(2 * CLIP_WG_BLOCKS >= MSV1_DELTA_RUN, "a count's look-ahead ends within the next two workgroups");
static_assert(CLIP_WG_BLOCKS * 18 < (1 << 16) && CLIP_WG_BLOCKS < (1 << 15), "bytes and codes of a workgroup share one scanned word");

// src(j) of the whole block grid: src(j) = j, nb = nblocks.
struct ClipGridSrc {
    int nb;
    int blk = 0;   // src(j) of the block the lane stands at
    __device__ __forceinline__ int at(int j) const { return j; }
    __device__ __forceinline__ void start(int j) { blk = j; }
    __device__ __forceinline__ void step() { ++blk; }
};

// src(j) of the rectangle (bx, by, bw, nb / bw) of a grid nbx blocks wide, j < nb: (by + j / bw) * nbx + bx + j % bw.  The host has
// checked the rectangle against the block grid, so every src(j) lies in [0, nblocks).
struct ClipRectSrc {
    int nbx, bx, by, bw, nb;
    int col = 0, blk = 0;   // the column of block j in the rectangle, and src(j)
    __device__ __forceinline__ int at(int j) const {
        const int row = j / bw;
        return (by + row) * nbx + bx + (j - row * bw);
    }
    // the lane's first block: the ONE division per lane
    __device__ __forceinline__ void start(int j) {
        const int row = j / bw;
        col = j - row * bw;
        blk = (by + row) * nbx + bx + col;
    }
    // src(j) from src(j - 1): the next column, or the first one of the next row
    __device__ __forceinline__ void step() {
        ++blk;
        if (++col == bw) {
            col = 0;
            blk += nbx - bw;
        }
    }
};

// src(j) of the rectangle of a launch (crop, path).
__device__ __forceinline__ ClipRectSrc clip_rect_src(const Msv1IndexSrc& s, const Msv1CropRect& r) {
    return ClipRectSrc{s.nbx, r.bx, r.by, r.bw, r.nb};
}

// The body of a sizes kernel for the workgroup's pair, blockIdx.y.  Rule:
//   bool key                                          the pair is a key pair: no run heads, and a block without a code refuses;
//   static constexpr bool counts                      whether d.counts gets the workgroup's number of codes;
//   bool coded(s, blk, s_pal, f) const                whether source block blk gets a code; f: the writer frame whose code it is — left
//                                                     at -1 for "coded, no writer", which refuses (MSV1_KEYFRAME_NO_WRITER).
// TIGHT: the rule decodes pictures, so the palette (8 bits) is brought into LDS first.  The status of a pair is min over
// (j << 1 | kind): the FIRST block of the frame that refuses.
template <int BITS, bool TIGHT, class Src, class Rule>
__device__ __forceinline__ void clip_sizes_body(const Msv1IndexSrc& s, Src src, const Rule& rule, const Msv1ClipScratch& d) {
    constexpr int WG = INDEX_CODES_WG;
    __shared__ uint32_t s_pal[TIGHT && BITS == 8 ? 256 : 1];
    if (TIGHT) load_palette<BITS>(s_pal, s.palette);
    __shared__ uint32_t s_wave[WG / 64];
    __shared__ uint32_t s_first[WG / 64];
    __shared__ uint8_t s_last[WG];                       // per lane: its last block is coded
    const int pair = (int)blockIdx.y, nwg = (int)gridDim.x, nb = src.nb;
    const int j0 = (int)blockIdx.x * CLIP_WG_BLOCKS + (int)threadIdx.x * CLIP_LANE_BLOCKS;
    if (j0 < nb) src.start(j0);
    uint32_t frame[CLIP_LANE_BLOCKS], len[CLIP_LANE_BLOCKS];
    bool coded[CLIP_LANE_BLOCKS];
    uint32_t worst = 0xFFFFFFFFu, first = MSV1_DELTA_NONE;
#pragma unroll
    for (int i = 0; i < CLIP_LANE_BLOCKS; ++i) {
        const int j = j0 + i;
        frame[i] = 0u;
        len[i] = 0u;
        coded[i] = false;
        if (j >= nb) continue;
        if (i > 0) src.step();
        int f = -1;
        const bool wanted = rule.coded(s, src.blk, s_pal, f);
        if (wanted && f >= 0) {
            coded[i] = true;
            first = min(first, (uint32_t)j);
            uint32_t o, e;
            const Msv1IndexChunk ch = index_code_at(s, f, src.blk, BITS, o, e);
            frame[i] = (uint32_t)f;
            len[i] = index_whole_length<BITS>(ch, o, e);
            if (len[i] == 0u) worst = min(worst, ((uint32_t)j << 1) | MSV1_KEYFRAME_CUT);
        } else if (wanted || rule.key) {                 // (no code to take: the pair refuses, nothing of it is gathered)
            worst = min(worst, ((uint32_t)j << 1) | MSV1_KEYFRAME_NO_WRITER);
        }
    }
    if (worst != 0xFFFFFFFFu) atomicMin(d.status + pair, worst);

    // the block before the lane's first one: the neighbour lane's last block; the workgroup's first lane judges src(j0 - 1) by the rule
    s_last[threadIdx.x] = coded[CLIP_LANE_BLOCKS - 1] ? 1 : 0;
    bool before = true;                                  // (block 0 is a run head: as if a coded block stood before it)
    if (threadIdx.x == 0 && !rule.key && j0 > 0 && j0 < nb) {   // (a key pair has no run heads: nothing to look for)
        int f = -1;
        before = rule.coded(s, src.at(j0 - 1), s_pal, f) && f >= 0;
    }
    __syncthreads();
    if (threadIdx.x > 0) before = s_last[threadIdx.x - 1] != 0;
#pragma unroll
    for (int i = 0; i < CLIP_LANE_BLOCKS; ++i) {
        const int j = j0 + i;
        if (j < nb && !rule.key && !coded[i] && (before || j % MSV1_DELTA_RUN == 0)) len[i] = MSV1_DELTA_SKIP;
        before = coded[i];
    }

    // exclusive scan of the contributions over the workgroup (low half: bytes, high half: codes); its first coded block
    uint32_t mine = 0u;
#pragma unroll
    for (int i = 0; i < CLIP_LANE_BLOCKS; ++i)
        mine += len[i] == MSV1_DELTA_SKIP ? 2u : len[i] != 0u && Rule::counts ? (1u << 16) | len[i] : len[i];
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
#pragma unroll
    for (int k = 1; k < 64; k <<= 1) first = min(first, (uint32_t)__shfl_xor((int)first, k));
    if (lane == 0) s_first[wave] = first;
    uint32_t total;
    uint32_t off = index_wg_scan(mine, s_wave, total) & 0xFFFFu;   // (its barrier also publishes s_first)
    uint32_t* records = d.records + 2 * (size_t)pair * (size_t)nb;
#pragma unroll
    for (int i = 0; i < CLIP_LANE_BLOCKS; ++i) {
        const int j = j0 + i;
        if (j < nb) {
            *(gu32*)(records + 2 * (size_t)j) = frame[i];
            *(gu32*)(records + 2 * (size_t)j + 1) = (off << 8) | len[i];
        }
        off += len[i] == MSV1_DELTA_SKIP ? 2u : len[i];
    }
    if (threadIdx.x == 0) {
        uint32_t f0 = s_first[0];
#pragma unroll
        for (int v = 1; v < WG / 64; ++v) f0 = min(f0, s_first[v]);
        *(gu32*)(d.totals + (size_t)pair * nwg + blockIdx.x) = total & 0xFFFFu;
        if (Rule::counts) *(gu32*)(d.counts + (size_t)pair * nwg + blockIdx.x) = total >> 16;
        *(gu32*)(d.first_written + (size_t)pair * nwg + blockIdx.x) = f0;
    }
}

// The body of a gather kernel for the workgroup's pair, after a sizes launch over the same pairs with no status raised and with
// bases[] = the running sums of the pairs' lengths: the frames into d.out.
template <int BITS, class Src>
__device__ __forceinline__ void clip_gather_body(const Msv1IndexSrc& s, Src src, const Msv1ClipScratch& d) {
    constexpr int WG = INDEX_CODES_WG;
    constexpr int IMAGE = CLIP_WG_BLOCKS * (BITS == 16 ? 18 : 10);              // bytes of a workgroup's output at its bound
    __shared__ __attribute__((aligned(16))) uint16_t s_img[(IMAGE + 16) / 2];   // (+ 16: the image starts base % 16 bytes in)
    __shared__ uint32_t s_wave[WG / 64];
    __shared__ uint32_t s_mask[CLIP_WG_BLOCKS / 32];                             // bit k of word w: block 32 w + k of the workgroup is coded
    const int pair = (int)blockIdx.y, nwg = (int)gridDim.x, g = (int)blockIdx.x, nb = src.nb;
    const uint32_t* totals = d.totals + (size_t)pair * nwg;
    const uint32_t* records = d.records + 2 * (size_t)pair * (size_t)nb;
    if (threadIdx.x < CLIP_WG_BLOCKS / 32) s_mask[threadIdx.x] = 0u;
    const size_t base = (size_t)d.bases[pair] + index_wg_bytes_before(totals, g, s_wave);   // (its barrier also publishes the zeroed mask)
    const uint32_t total = *(cgu32*)(totals + g);
    const uint32_t lo = (uint32_t)(base & 15), hi = lo + total;                  // the image is s_img bytes [lo, hi)

    const int j0 = g * CLIP_WG_BLOCKS + (int)threadIdx.x * CLIP_LANE_BLOCKS;
    if (j0 < nb) src.start(j0);
    uint32_t ol[CLIP_LANE_BLOCKS], bits4 = 0u;
#pragma unroll
    for (int i = 0; i < CLIP_LANE_BLOCKS; ++i) {
        const int j = j0 + i;
        ol[i] = 0u;
        if (j >= nb) continue;
        if (i > 0) src.step();
        const uint32_t f = *(cgu32*)(records + 2 * (size_t)j);
        ol[i] = *(cgu32*)(records + 2 * (size_t)j + 1);
        const uint32_t L = ol[i] & 0xFFu, at = lo + (ol[i] >> 8);
        if (L >= 2u && at + L <= hi) {                                          // (else nothing or a run head; the second test always holds)
            bits4 |= 1u << i;
            uint32_t o, e;
            const Msv1IndexChunk ch = index_code_at(s, (int)f, src.blk, BITS, o, e);
            for (uint32_t k = 0; k < L; k += 2u) s_img[(at + k) >> 1] = *(cgu16*)(ch.stream + o + k);
        }
    }
    if (bits4 != 0u) atomicOr(&s_mask[threadIdx.x >> 3], bits4 << (CLIP_LANE_BLOCKS * (threadIdx.x & 7)));
    __syncthreads();

    // the run heads: count = up to the next coded block, the next multiple of 1023, nb — all in j-numbering
#pragma unroll
    for (int i = 0; i < CLIP_LANE_BLOCKS; ++i) {
        if ((ol[i] & 0xFFu) != MSV1_DELTA_SKIP) continue;
        const int j = j0 + i;
        const uint32_t at = lo + (ol[i] >> 8);
        if (at + 2u > hi) continue;                                             // (never holds)
        const int q = (int)threadIdx.x * CLIP_LANE_BLOCKS + i + 1;              // the first block behind the head, within the workgroup
        uint32_t next = MSV1_DELTA_NONE;
        for (int w = q >> 5; w < CLIP_WG_BLOCKS / 32 && next == MSV1_DELTA_NONE; ++w) {
            uint32_t m = s_mask[w];
            if (w == (q >> 5)) m &= 0xFFFFFFFFu << (q & 31);
            if (m != 0u) next = (uint32_t)(g * CLIP_WG_BLOCKS + 32 * w + __builtin_ctz(m));
        }
        for (int k = g + 1; k <= g + 2 && k < nwg && next == MSV1_DELTA_NONE; ++k) next = *(cgu32*)(d.first_written + (size_t)pair * nwg + k);
        const uint32_t limit = min((uint32_t)(j / MSV1_DELTA_RUN + 1) * (uint32_t)MSV1_DELTA_RUN, (uint32_t)nb);
        const uint32_t count = min(next, limit) - (uint32_t)j;
        s_img[at >> 1] = (uint16_t)((count & 0xFFu) | ((0x84u + (count >> 8)) << 8));
    }
    __syncthreads();

    index_image_store(d.out + (base - lo), s_img, lo, hi);                       // (d.out is 16-byte aligned, so is this)
}

// The launch of a sizes or gather kernel over frames of nb blocks (host code): nothing for a frame without a block, else
// launch(grid, dim3(INDEX_CODES_WG), bits, tight) with the bit depth and the tight flag as integral constants for the kernel's
// template arguments (a gather kernel has one form for both: it passes tight = false).
template <class Launch>
void clip_launch(int nb, int npairs, int bits, bool tight, Launch&& launch) {
    if (nb <= 0 || npairs <= 0) return;
    const dim3 grid((unsigned)msv1_keyframe_workgroups(nb), (unsigned)npairs), wg(INDEX_CODES_WG);
    using B16 = std::integral_constant<int, 16>;
    using B8 = std::integral_constant<int, 8>;
    if (tight) {
        if (bits == 16) launch(grid, wg, B16{}, std::true_type{});
        else launch(grid, wg, B8{}, std::true_type{});
    } else if (bits == 16) {
        launch(grid, wg, B16{}, std::false_type{});
    } else {
        launch(grid, wg, B8{}, std::false_type{});
    }
}

}  // namespace
}  // namespace jsp
