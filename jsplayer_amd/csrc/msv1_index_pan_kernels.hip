// The frames of a BLOCK RECTANGLE THAT MOVES over an MSVideo1 seek index for gfx950 (MI355X): the stream bytes of a clip that pans
// across the picture (jsp_index_pan_frames) — TWO launches for any number of pairs, no pixel decoded to memory, nothing re-quantised.
// An MSVideo1 code carries no position, so a moved rectangle stays a gather of codes the index holds: the block at position j of
// the new rectangle is either the same 16 words as the block that stood at position j of the old one (skip it) or it needs the code
// its last writer gave it (copy it).  Host side in msv1_seek.cpp.
//
// THE RULE (PAN).  WHOLE (msv1_index_keyframe_kernels.hip), WRITTEN, RUN HEAD, the skip word, the 1023 rule, KEPT, P(t)[i] and
// DEFINED (msv1_index_delta_kernels.hip) and src(j) (msv1_index_crop_kernels.hip) are exactly those definitions.  A call has ONE
// rectangle size (bw, bh) in 4x4 blocks, nb = bw * bh, and n pairs.  Pair k has from, to, an origin A = (from_xy[2k], from_xy[2k+1])
// of the rectangle at frame `from` and an origin B = (to_xy[2k], to_xy[2k+1]) at frame `to`, both (bx, by) in TABLE order as in crop;
// srcA(j) and srcB(j) are crop's src(j) of the rectangles (A, bw, bh) and (B, bw, bh).  A pair is one of three kinds.
//   KEY pair, from == JSP_CROP_KEY: crop's key pair of rectangle B at `to`.  A is not read.
//   STILL gap pair, A == B and -1 <= from < to < nframes: crop's gap pair of that rectangle (Delta, or with JSP_CROP_TIGHT Tight).
//   MOVED pair, A != B and -1 <= from <= to, 0 <= to < nframes.  from == to is allowed here and only here: a pan across a picture
//     that stands still.
//       Without JSP_CROP_TIGHT every block is coded: the bytes and the refusals are those of the KEY pair (B, to), keys[k] = 1.
//       With JSP_CROP_TIGHT block j is DROPPED when P(from)[srcA(j)] and P(to)[srcB(j)] are both DEFINED and equal in all 16 words;
//       otherwise it is KEPT.  "Written in the gap" plays no part: a block no frame of the gap touches is kept when the two
//       pictures differ there, a block every frame rewrote is dropped when they agree.  A kept block contributes the whole code of
//       the last writer <= to of srcB(j); a kept block with no such writer refuses ("no writer"), one whose code is cut refuses
//       ("cut"); a dropped block never refuses.  Run heads, counts and the multiples of 1023 are Tight's, in j-numbering.
// The status of a pair is crop's: min over (j << 1 | kind), the FIRST refusing block of the rectangle.
// PROMISED: a fresh decoder of 4 bw x 4 bh pixels fed a KEY pair's frame as a key frame, then the frames of pairs chained by
// to[k-1] == from[k] and to_xy[k-1] == from_xy[k], holds after each the pixels of rectangle B of the source picture of to[k].  A call
// whose pairs are all KEY or STILL with one origin throughout returns byte for byte what jsp_index_crop_frames returns for that
// rectangle.  len(moved tight) <= len(KEY pair (B, to)) whenever both exist.  NOT promised: the exclusions of KeyFrame.
//
// The shape is the crop kernels', grid.y = the pair, no workgroup ever waits for another: a lane owns PAN_LANE_BLOCKS consecutive
// blocks OF THE RECTANGLE, a workgroup PAN_WG_BLOCKS; the scan runs inside the workgroup with a total per workgroup, the gather sums
// the totals before its own.  What differs:
//   * the origins are per pair, read from the scratch beside the pair word (Msv1PanScratch::origins).  The one division per lane
//     and the wrap step stay; srcA(j) = srcB(j) + shift with ONE shift per pair, (A.y - B.y) * nbx + A.x - B.x;
//   * ONE test, pan_coded, with a branch on the pair word that is uniform over the workgroup (the pair is blockIdx.y).  KEY and STILL
//     pairs leave through crop's test first — an unwritten block, and every block of a key pair, decodes nothing — and a still tight
//     pair then compares what tight_kept compares.  A MOVED pair of a tight call skips that test and compares picture_block
//     (msv1_index_codes.h) of srcA(j) at `from` with that of srcB(j) at `to`, 16 words.  A moved pair of a call without the tight flag
//     arrives as the key pair (B, to): the host writes it so;
//   * the block before a workgroup's first block, j0 - 1, is judged by the same rule with both sources by the workgroup's first lane;
//   * the gather takes codes from srcB(j) only: it is crop's gather with the origin read per pair.
// Lanes with j >= nb touch nothing and form no source block.  The host has checked B, and for gap pairs A, against the block grid, so
// every srcB(j) and, where it is formed (gap pairs only), every srcA(j), j < nb, lies in [0, nblocks).
#include "msv1_index_codes.h"

namespace jsp {
namespace {

constexpr int WG = INDEX_CODES_WG;
constexpr int PAN_LANE_BLOCKS = 4;
constexpr int PAN_WG_BLOCKS = MSV1_KEYFRAME_WG_BLOCKS;   // (msv1_seek.h: the host sizes totals[], first_written[] and counts[] by it)
static_assert(PAN_WG_BLOCKS == WG * PAN_LANE_BLOCKS, "a lane owns PAN_LANE_BLOCKS consecutive blocks");
static_assert(2 * PAN_WG_BLOCKS >= MSV1_DELTA_RUN, "a count's look-ahead ends within the next two workgroups");
static_assert(PAN_WG_BLOCKS * 18 < (1 << 16) && PAN_WG_BLOCKS < (1 << 15), "bytes and codes of a workgroup share one scanned word");

// A pair as a workgroup sees it: rectangle B, and what to add to srcB(j) for srcA(j) (0 for a key pair: A is not read).
struct PanPair {
    int a, b;            // from, to
    bool key, moved;     // moved: A != B (a gap pair)
    int bx, by, bw, nb;  // rectangle B
    int shift;
};
__device__ __forceinline__ PanPair pan_pair(const Msv1IndexSrc& s, const Msv1PanScratch& d, int bw, int bh, int pair) {
    PanPair p;
    p.a = d.c.pairs[2 * pair];
    p.b = d.c.pairs[2 * pair + 1];
    p.key = p.a == MSV1_CROP_KEY;
    p.bx = d.origins[4 * pair + 2];
    p.by = d.origins[4 * pair + 3];
    p.bw = bw;
    p.nb = bw * bh;
    p.shift = 0;
    if (!p.key) p.shift = (d.origins[4 * pair + 1] - p.by) * s.nbx + d.origins[4 * pair] - p.bx;
    p.moved = p.shift != 0;   // (both rectangles lie in the grid: the shift is 0 only for A == B)
    return p;
}

// srcB(j) for j < nb.
__device__ __forceinline__ int pan_src(const Msv1IndexSrc& s, const PanPair& p, int j) {
    const int row = j / p.bw;
    return (p.by + row) * s.nbx + p.bx + (j - row * p.bw);
}

// srcB(j) from srcB(j - 1), j < nb: the next column, or the first one of the next row.
__device__ __forceinline__ void pan_step(const Msv1IndexSrc& s, const PanPair& p, int& col, int& blk) {
    ++blk;
    if (++col == p.bw) {
        col = 0;
        blk += s.nbx - p.bw;
    }
}

// Whether block `blk` = srcB(j) gets a code.  f: its last writer <= b, -1 without one.
//   KEY and STILL pairs, crop's test (delta_written, then tight_kept's compare): a key pair — some frame <= b codes it; a gap pair —
//     written (TIGHT: kept) in (a, b].  An unwritten block leaves before anything is decoded.
//   MOVED pairs of a tight call: KEPT — "written" plays no part, and P(b)[srcB(j)] may be the picture before the range.
// One compare serves both: P(a) of block blk + shift (shift = 0: the block itself) against P(b) of blk.
template <int BITS, bool TIGHT>
__device__ __forceinline__ bool pan_coded(const Msv1IndexSrc& s, int blk, const PanPair& p, const uint32_t* s_pal, int& f) {
    int w;
    const uint32_t m = index_last_writer(s, blk, p.b, w);
    f = m != 0u ? index_word_frame(w, m) : -1;
    if (!(TIGHT && p.moved)) {
        if (f < 0 || (!p.key && f <= p.a)) return false;
        if (!TIGHT || p.key) return true;
    }
    uint32_t pa[16], pb[16];
    if (!picture_block_of<BITS>(s, blk, f, s_pal, pb)) return true;   // (this order: two registers fewer than the other one)
    if (!picture_block<BITS>(s, blk + p.shift, p.a, s_pal, pa)) return true;
    uint32_t diff = 0u;
#pragma unroll
    for (int k = 0; k < 16; ++k) diff |= pa[k] ^ pb[k];
    return diff != 0u;
}

// TIGHT = true applies THE TIGHT RULE to the still gap pairs and the two-block compare to the moved ones: `written` below then reads
// "kept".  With TIGHT = false no pair is moved.  No occupancy attribute: asked for eight waves the compiler spills 32 to 48 SGPRs to
// get there; left alone the tight form takes 64 VGPRs and nothing is spilled (DESIGN.md has the report's figures).
template <int BITS, bool TIGHT>
__global__ __launch_bounds__(WG) void msv1_index_pan_sizes_kernel(const Msv1IndexSrc s, const int bw, const int bh, Msv1PanScratch d) {
    __shared__ uint32_t s_pal[TIGHT && BITS == 8 ? 256 : 1];
    if (TIGHT) load_palette<BITS>(s_pal, s.palette);
    __shared__ uint32_t s_wave[WG / 64];
    __shared__ uint32_t s_first[WG / 64];
    __shared__ uint8_t s_last[WG];                       // per lane: its last block is written
    const int pair = (int)blockIdx.y, nwg = (int)gridDim.x;
    const PanPair p = pan_pair(s, d, bw, bh, pair);
    const int j0 = (int)blockIdx.x * PAN_WG_BLOCKS + (int)threadIdx.x * PAN_LANE_BLOCKS;
    int col = 0, blk = 0;                                // the column of block j in the rectangle, and srcB(j)
    if (j0 < p.nb) {
        const int row = j0 / p.bw;
        col = j0 - row * p.bw;
        blk = (p.by + row) * s.nbx + p.bx + col;
    }
    uint32_t frame[PAN_LANE_BLOCKS], len[PAN_LANE_BLOCKS];
    bool written[PAN_LANE_BLOCKS];
    uint32_t worst = 0xFFFFFFFFu, first = MSV1_DELTA_NONE;
#pragma unroll
    for (int i = 0; i < PAN_LANE_BLOCKS; ++i) {
        const int j = j0 + i;
        frame[i] = 0u;
        len[i] = 0u;
        written[i] = false;
        if (j >= p.nb) continue;
        if (i > 0) pan_step(s, p, col, blk);
        int f = -1;
        const bool coded = pan_coded<BITS, TIGHT>(s, blk, p, s_pal, f);
        if (coded && f >= 0) {
            written[i] = true;
            first = min(first, (uint32_t)j);
            uint32_t o, e;
            const Msv1IndexChunk ch = index_code_at(s, f, blk, BITS, o, e);
            frame[i] = (uint32_t)f;
            len[i] = index_whole_length<BITS>(ch, o, e);
            if (len[i] == 0u) worst = min(worst, ((uint32_t)j << 1) | MSV1_KEYFRAME_CUT);
        } else if (p.key || coded) {                     // a key pair's block without a writer, or a moved pair's kept one
            worst = min(worst, ((uint32_t)j << 1) | MSV1_KEYFRAME_NO_WRITER);
        }
    }
    if (worst != 0xFFFFFFFFu) atomicMin(d.c.status + pair, worst);

    // the block before the lane's first one: the neighbour lane's last block; the workgroup's first lane judges srcB(j0 - 1) (a
    // moved pair: with srcA(j0 - 1)) by the same rule
    s_last[threadIdx.x] = written[PAN_LANE_BLOCKS - 1] ? 1 : 0;
    bool before = true;                                  // (block 0 is a run head: as if a written block stood before it)
    if (threadIdx.x == 0 && !p.key && j0 > 0 && j0 < p.nb) {   // (a key pair has no run heads: nothing to walk for)
        int f = -1;
        const int prev = pan_src(s, p, j0 - 1);
        before = pan_coded<BITS, TIGHT>(s, prev, p, s_pal, f) && f >= 0;
    }
    __syncthreads();
    if (threadIdx.x > 0) before = s_last[threadIdx.x - 1] != 0;
#pragma unroll
    for (int i = 0; i < PAN_LANE_BLOCKS; ++i) {
        const int j = j0 + i;
        if (j < p.nb && !p.key && !written[i] && (before || j % MSV1_DELTA_RUN == 0)) len[i] = MSV1_DELTA_SKIP;
        before = written[i];
    }

    // exclusive scan of the contributions over the workgroup (low half: bytes, high half: codes); its first written block
    uint32_t mine = 0u;
#pragma unroll
    for (int i = 0; i < PAN_LANE_BLOCKS; ++i) mine += len[i] == MSV1_DELTA_SKIP ? 2u : len[i] != 0u ? (1u << 16) | len[i] : 0u;
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
#pragma unroll
    for (int k = 1; k < 64; k <<= 1) first = min(first, (uint32_t)__shfl_xor((int)first, k));
    if (lane == 0) s_first[wave] = first;
    uint32_t total;
    uint32_t off = index_wg_scan(mine, s_wave, total) & 0xFFFFu;   // (its barrier also publishes s_first)
    uint32_t* records = d.c.records + 2 * (size_t)pair * (size_t)p.nb;
#pragma unroll
    for (int i = 0; i < PAN_LANE_BLOCKS; ++i) {
        const int j = j0 + i;
        if (j < p.nb) {
            *(gu32*)(records + 2 * (size_t)j) = frame[i];
            *(gu32*)(records + 2 * (size_t)j + 1) = (off << 8) | len[i];
        }
        off += len[i] == MSV1_DELTA_SKIP ? 2u : len[i];
    }
    if (threadIdx.x == 0) {
        uint32_t f0 = s_first[0];
#pragma unroll
        for (int v = 1; v < WG / 64; ++v) f0 = min(f0, s_first[v]);
        *(gu32*)(d.c.totals + (size_t)pair * nwg + blockIdx.x) = total & 0xFFFFu;
        *(gu32*)(d.c.counts + (size_t)pair * nwg + blockIdx.x) = total >> 16;
        *(gu32*)(d.c.first_written + (size_t)pair * nwg + blockIdx.x) = f0;
    }
}

// Crop's gather with rectangle B of the pair: the LDS image, the mask and the look-ahead are the same — a COPY of
// msv1_index_crop_gather_kernel (crop's path is pinned and not routed through here): a fix to one belongs in the other too.
template <int BITS>
__global__ __launch_bounds__(WG) void msv1_index_pan_gather_kernel(const Msv1IndexSrc s, const int bw, const int bh, Msv1PanScratch d) {
    constexpr int IMAGE = PAN_WG_BLOCKS * (BITS == 16 ? 18 : 10);                // bytes of a workgroup's output at its bound
    __shared__ __attribute__((aligned(16))) uint16_t s_img[(IMAGE + 16) / 2];   // (+ 16: the image starts base % 16 bytes in)
    __shared__ uint32_t s_wave[WG / 64];
    __shared__ uint32_t s_mask[PAN_WG_BLOCKS / 32];                              // bit k of word w: block 32 w + k of the workgroup is written
    const int pair = (int)blockIdx.y, nwg = (int)gridDim.x, g = (int)blockIdx.x;
    const int nb = bw * bh, bx = d.origins[4 * pair + 2], by = d.origins[4 * pair + 3];
    const uint32_t* totals = d.c.totals + (size_t)pair * nwg;
    const uint32_t* records = d.c.records + 2 * (size_t)pair * (size_t)nb;
    if (threadIdx.x < PAN_WG_BLOCKS / 32) s_mask[threadIdx.x] = 0u;
    const size_t base = (size_t)d.c.bases[pair] + index_wg_bytes_before(totals, g, s_wave);   // (its barrier also publishes the zeroed mask)
    const uint32_t total = *(cgu32*)(totals + g);
    const uint32_t lo = (uint32_t)(base & 15), hi = lo + total;                  // the image is s_img bytes [lo, hi)

    const int j0 = g * PAN_WG_BLOCKS + (int)threadIdx.x * PAN_LANE_BLOCKS;
    int col = 0, blk = 0;
    if (j0 < nb) {
        const int row = j0 / bw;
        col = j0 - row * bw;
        blk = (by + row) * s.nbx + bx + col;
    }
    uint32_t ol[PAN_LANE_BLOCKS], bits4 = 0u;
#pragma unroll
    for (int i = 0; i < PAN_LANE_BLOCKS; ++i) {
        const int j = j0 + i;
        ol[i] = 0u;
        if (j >= nb) continue;
        if (i > 0) {
            ++blk;
            if (++col == bw) {
                col = 0;
                blk += s.nbx - bw;
            }
        }
        const uint32_t f = *(cgu32*)(records + 2 * (size_t)j);
        ol[i] = *(cgu32*)(records + 2 * (size_t)j + 1);
        const uint32_t L = ol[i] & 0xFFu, at = lo + (ol[i] >> 8);
        if (L >= 2u && at + L <= hi) {                                          // (else nothing or a run head; the second test always holds)
            bits4 |= 1u << i;
            uint32_t o, e;
            const Msv1IndexChunk ch = index_code_at(s, (int)f, blk, BITS, o, e);
            for (uint32_t k = 0; k < L; k += 2u) s_img[(at + k) >> 1] = *(cgu16*)(ch.stream + o + k);
        }
    }
    if (bits4 != 0u) atomicOr(&s_mask[threadIdx.x >> 3], bits4 << (PAN_LANE_BLOCKS * (threadIdx.x & 7)));
    __syncthreads();

    // the run heads: count = up to the next written block, the next multiple of 1023, nb — all in the rectangle's numbering
#pragma unroll
    for (int i = 0; i < PAN_LANE_BLOCKS; ++i) {
        if ((ol[i] & 0xFFu) != MSV1_DELTA_SKIP) continue;
        const int j = j0 + i;
        const uint32_t at = lo + (ol[i] >> 8);
        if (at + 2u > hi) continue;                                             // (never holds)
        const int q = (int)threadIdx.x * PAN_LANE_BLOCKS + i + 1;               // the first block behind the head, within the workgroup
        uint32_t next = MSV1_DELTA_NONE;
        for (int w = q >> 5; w < PAN_WG_BLOCKS / 32 && next == MSV1_DELTA_NONE; ++w) {
            uint32_t m = s_mask[w];
            if (w == (q >> 5)) m &= 0xFFFFFFFFu << (q & 31);
            if (m != 0u) next = (uint32_t)(g * PAN_WG_BLOCKS + 32 * w + __builtin_ctz(m));
        }
        for (int k = g + 1; k <= g + 2 && k < nwg && next == MSV1_DELTA_NONE; ++k) next = *(cgu32*)(d.c.first_written + (size_t)pair * nwg + k);
        const uint32_t limit = min((uint32_t)(j / MSV1_DELTA_RUN + 1) * (uint32_t)MSV1_DELTA_RUN, (uint32_t)nb);
        const uint32_t count = min(next, limit) - (uint32_t)j;
        s_img[at >> 1] = (uint16_t)((count & 0xFFu) | ((0x84u + (count >> 8)) << 8));
    }
    __syncthreads();

    index_image_store(d.c.out + (base - lo), s_img, lo, hi);                     // (d.c.out is 16-byte aligned, so is this)
}

}  // namespace

void msv1_launch_index_pan_sizes(const Msv1IndexSrc& src, int bw, int bh, int npairs, const Msv1PanScratch& d, bool tight, hipStream_t stream) {
    if (bw <= 0 || bh <= 0 || npairs <= 0) return;
    const dim3 grid((unsigned)msv1_keyframe_workgroups(bw * bh), (unsigned)npairs);
    if (tight) {
        if (src.bits == 16) hipLaunchKernelGGL((msv1_index_pan_sizes_kernel<16, true>), grid, dim3(WG), 0, stream, src, bw, bh, d);
        else hipLaunchKernelGGL((msv1_index_pan_sizes_kernel<8, true>), grid, dim3(WG), 0, stream, src, bw, bh, d);
    } else if (src.bits == 16) {
        hipLaunchKernelGGL((msv1_index_pan_sizes_kernel<16, false>), grid, dim3(WG), 0, stream, src, bw, bh, d);
    } else {
        hipLaunchKernelGGL((msv1_index_pan_sizes_kernel<8, false>), grid, dim3(WG), 0, stream, src, bw, bh, d);
    }
}

void msv1_launch_index_pan_gather(const Msv1IndexSrc& src, int bw, int bh, int npairs, const Msv1PanScratch& d, hipStream_t stream) {
    if (bw <= 0 || bh <= 0 || npairs <= 0) return;
    const dim3 grid((unsigned)msv1_keyframe_workgroups(bw * bh), (unsigned)npairs);
    if (src.bits == 16) hipLaunchKernelGGL(msv1_index_pan_gather_kernel<16>, grid, dim3(WG), 0, stream, src, bw, bh, d);
    else hipLaunchKernelGGL(msv1_index_pan_gather_kernel<8>, grid, dim3(WG), 0, stream, src, bw, bh, d);
}

}  // namespace jsp
