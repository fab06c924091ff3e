// The frames of a BLOCK RECTANGLE of an MSVideo1 seek index for gfx950 (MI355X): the stream bytes of a clip that shows only a part of
// the picture (jsp_index_crop_frames) — TWO launches for any number of pairs, no pixel decoded, nothing re-quantised.  An MSVideo1
// code carries no position (colours and a mask; at 8 bits indices into a palette that the cropped clip keeps), so the clip of a
// block-aligned rectangle is a gather of codes the index already holds.  Host side in msv1_seek.cpp.
//
// THE RULE.  A rectangle is (bx, by, bw, bh) in 4x4 blocks, in TABLE order: block row 0 is stored rows 0 .. 3 of the frame buffer,
// the bottom of the picture as displayed.  bw, bh >= 1, 0 <= bx, bx + bw <= nbx, 0 <= by, by + bh <= nby.  nb = bw * bh, and for
// j < nb block j of the rectangle is source block src(j) = (by + j / bw) * nbx + bx + j % bw.  The cropped clip is 4 bw x 4 bh
// pixels, with the source's bit depth and palette.
// WHOLE (msv1_index_keyframe_kernels.hip), WRITTEN, RUN HEAD, the skip word, the 1023 rule and KEPT (msv1_index_delta_kernels.hip)
// are exactly those definitions, applied to the VIRTUAL index whose block j is source block src(j) — everything in j-numbering:
//   * a run head is j = 0, or block j - 1 OF THE RECTANGLE written (tight: kept), or j % 1023 = 0.  At a row start block j - 1 is
//     the last block of the rectangle's row before, a source block far away, never src(j) - 1;
//   * counts stop at the next multiple of 1023 in j, and at nb.
// A pair is one of two kinds.
//   GAP pair (from, to], -1 <= from < to < nframes: Delta(from, to), or with the tight flag Tight(from, to), of the virtual index.  A
//     cut code of a written (tight: kept) block refuses; a block without a writer is skipped.
//   KEY pair, from == JSP_CROP_KEY (-2), 0 <= to < nframes: the key frame of the rectangle at `to` — the whole code of the last
//     writer <= to of every src(j), no skip words.  A block of the rectangle with no writer <= to refuses (kind "no writer"), a cut
//     code refuses (kind "cut").  The tight flag does not touch key pairs.
// Blocks outside the rectangle never matter: a rectangle can be cut where the key frame of the whole picture refuses.  The status of
// a pair is min over (j << 1 | kind), the key frame's: the FIRST block of the rectangle that refuses.  With the rectangle equal to
// the whole block grid src(j) = j, and the bytes are those of the whole-picture calls.
//
// The shape is the delta kernels', grid.y = the pair, no workgroup ever waits for another: a lane owns CR_LANE_BLOCKS consecutive
// blocks OF THE RECTANGLE, a workgroup CR_WG_BLOCKS.  What differs:
//   * src(j): ONE division per lane (j0 / bw); the column then steps with a wrap into the next row;
//   * the block before a lane's first one is the neighbour lane's last block through LDS, as there; the workgroup's first lane
//     walks for block j0 - 1 of the rectangle, src(j0 - 1);
//   * the pair word says key: an unwritten block then raises the status instead of becoming a run;
//   * the sizes kernel also leaves, per pair and workgroup, the number of blocks that got a code (one plain store: it rides in
//     the upper half of the word the byte counts are scanned in).  The host sums them: a frame that codes all nb blocks is a key frame.
// Records, totals and first_written are in j-numbering.  Lanes with j >= nb touch nothing, and no lane forms a source block for
// such a j: the host has checked the rectangle against the block grid, so every src(j), j < nb, lies in [0, nblocks).
#include "msv1_index_codes.h"

namespace jsp {
namespace {

constexpr int WG = INDEX_CODES_WG;
constexpr int CR_LANE_BLOCKS = 4;
constexpr int CR_WG_BLOCKS = MSV1_KEYFRAME_WG_BLOCKS;   // (msv1_seek.h: the host sizes totals[], first_written[] and counts[] by it)
static_assert(CR_WG_BLOCKS == WG * CR_LANE_BLOCKS, "a lane owns CR_LANE_BLOCKS consecutive blocks");
static_assert(2 * CR_WG_BLOCKS >= MSV1_DELTA_RUN, "a count's look-ahead ends within the next two workgroups");
static_assert(CR_WG_BLOCKS * 18 < (1 << 16) && CR_WG_BLOCKS < (1 << 15), "bytes and codes of a workgroup share one scanned word");

// src(j) for j < nb.
__device__ __forceinline__ int crop_src(const Msv1IndexSrc& s, const Msv1CropRect& r, int j) {
    const int row = j / r.bw;
    return (r.by + row) * s.nbx + r.bx + (j - row * r.bw);
}

// src(j) from src(j - 1), j < nb: the next column, or the first one of the next row.
__device__ __forceinline__ void crop_step(const Msv1IndexSrc& s, const Msv1CropRect& r, int& col, int& blk) {
    ++blk;
    if (++col == r.bw) {
        col = 0;
        blk += s.nbx - r.bw;
    }
}

// Whether source block `blk` counts for the pair: a key pair — some frame <= b codes it; a gap pair — written (TIGHT: kept) in (a, b].
// f: its last writer <= b.
template <int BITS, bool TIGHT>
__device__ __forceinline__ bool crop_coded(const Msv1IndexSrc& s, int blk, bool key, int a, int b, const uint32_t* s_pal, int& f) {
    if (!delta_written(s, blk, key ? -1 : a, b, f)) return false;
    return !TIGHT || key || tight_kept<BITS>(s, blk, a, f, s_pal);
}

// TIGHT = true applies THE TIGHT RULE to the gap pairs: `written` below then reads "kept".
template <int BITS, bool TIGHT>
__global__ __launch_bounds__(WG) void msv1_index_crop_sizes_kernel(const Msv1IndexSrc s, const Msv1CropRect r, Msv1CropScratch d) {
    __shared__ uint32_t s_pal[TIGHT && BITS == 8 ? 256 : 1];
    if (TIGHT) load_palette<BITS>(s_pal, s.palette);
    __shared__ uint32_t s_wave[WG / 64];
    __shared__ uint32_t s_first[WG / 64];
    __shared__ uint8_t s_last[WG];                       // per lane: its last block is written
    const int pair = (int)blockIdx.y, nwg = (int)gridDim.x;
    const int a = d.pairs[2 * pair], b = d.pairs[2 * pair + 1];
    const bool key = a == MSV1_CROP_KEY;
    const int j0 = (int)blockIdx.x * CR_WG_BLOCKS + (int)threadIdx.x * CR_LANE_BLOCKS;
    int col = 0, blk = 0;                                // the column of block j in the rectangle, and src(j)
    if (j0 < r.nb) {
        const int row = j0 / r.bw;
        col = j0 - row * r.bw;
        blk = (r.by + row) * s.nbx + r.bx + col;
    }
    uint32_t frame[CR_LANE_BLOCKS], len[CR_LANE_BLOCKS];
    bool written[CR_LANE_BLOCKS];
    uint32_t worst = 0xFFFFFFFFu, first = MSV1_DELTA_NONE;
#pragma unroll
    for (int i = 0; i < CR_LANE_BLOCKS; ++i) {
        const int j = j0 + i;
        frame[i] = 0u;
        len[i] = 0u;
        written[i] = false;
        if (j >= r.nb) continue;
        if (i > 0) crop_step(s, r, col, blk);
        int f;
        if (crop_coded<BITS, TIGHT>(s, blk, key, a, b, s_pal, f)) {
            written[i] = true;
            first = min(first, (uint32_t)j);
            uint32_t o, e;
            const Msv1IndexChunk ch = index_code_at(s, f, blk, BITS, o, e);
            frame[i] = (uint32_t)f;
            len[i] = index_whole_length<BITS>(ch, o, e);
            if (len[i] == 0u) worst = min(worst, ((uint32_t)j << 1) | MSV1_KEYFRAME_CUT);
        } else if (key) {
            worst = min(worst, ((uint32_t)j << 1) | MSV1_KEYFRAME_NO_WRITER);
        }
    }
    if (worst != 0xFFFFFFFFu) atomicMin(d.status + pair, worst);

    // the block before the lane's first one: the neighbour lane's last block; the workgroup's first lane walks for src(j0 - 1)
    s_last[threadIdx.x] = written[CR_LANE_BLOCKS - 1] ? 1 : 0;
    bool before = true;                                  // (block 0 is a run head: as if a written block stood before it)
    if (threadIdx.x == 0 && !key && j0 > 0 && j0 < r.nb) {   // (a key pair has no run heads: nothing to walk for)
        int f;
        before = crop_coded<BITS, TIGHT>(s, crop_src(s, r, j0 - 1), key, a, b, s_pal, f);
    }
    __syncthreads();
    if (threadIdx.x > 0) before = s_last[threadIdx.x - 1] != 0;
#pragma unroll
    for (int i = 0; i < CR_LANE_BLOCKS; ++i) {
        const int j = j0 + i;
        if (j < r.nb && !key && !written[i] && (before || j % MSV1_DELTA_RUN == 0)) len[i] = MSV1_DELTA_SKIP;
        before = written[i];
    }

    // exclusive scan of the contributions over the workgroup (low half: bytes, high half: codes); its first written block
    uint32_t mine = 0u;
#pragma unroll
    for (int i = 0; i < CR_LANE_BLOCKS; ++i) mine += len[i] == MSV1_DELTA_SKIP ? 2u : len[i] != 0u ? (1u << 16) | len[i] : 0u;
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
#pragma unroll
    for (int k = 1; k < 64; k <<= 1) first = min(first, (uint32_t)__shfl_xor((int)first, k));
    if (lane == 0) s_first[wave] = first;
    uint32_t total;
    uint32_t off = index_wg_scan(mine, s_wave, total) & 0xFFFFu;   // (its barrier also publishes s_first)
    uint32_t* records = d.records + 2 * (size_t)pair * (size_t)r.nb;
#pragma unroll
    for (int i = 0; i < CR_LANE_BLOCKS; ++i) {
        const int j = j0 + i;
        if (j < r.nb) {
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
        *(gu32*)(d.counts + (size_t)pair * nwg + blockIdx.x) = total >> 16;
        *(gu32*)(d.first_written + (size_t)pair * nwg + blockIdx.x) = f0;
    }
}

// (msv1_index_pan_gather_kernel, msv1_index_pan_kernels.hip, is a copy of this kernel with the origin read per pair: a fix to one
// belongs in the other too.)
template <int BITS>
__global__ __launch_bounds__(WG) void msv1_index_crop_gather_kernel(const Msv1IndexSrc s, const Msv1CropRect r, Msv1CropScratch d) {
    constexpr int IMAGE = CR_WG_BLOCKS * (BITS == 16 ? 18 : 10);                 // bytes of a workgroup's output at its bound
    __shared__ __attribute__((aligned(16))) uint16_t s_img[(IMAGE + 16) / 2];   // (+ 16: the image starts base % 16 bytes in)
    __shared__ uint32_t s_wave[WG / 64];
    __shared__ uint32_t s_mask[CR_WG_BLOCKS / 32];                               // bit k of word w: block 32 w + k of the workgroup is written
    const int pair = (int)blockIdx.y, nwg = (int)gridDim.x, g = (int)blockIdx.x;
    const uint32_t* totals = d.totals + (size_t)pair * nwg;
    const uint32_t* records = d.records + 2 * (size_t)pair * (size_t)r.nb;
    if (threadIdx.x < CR_WG_BLOCKS / 32) s_mask[threadIdx.x] = 0u;
    const size_t base = (size_t)d.bases[pair] + index_wg_bytes_before(totals, g, s_wave);   // (its barrier also publishes the zeroed mask)
    const uint32_t total = *(cgu32*)(totals + g);
    const uint32_t lo = (uint32_t)(base & 15), hi = lo + total;                  // the image is s_img bytes [lo, hi)

    const int j0 = g * CR_WG_BLOCKS + (int)threadIdx.x * CR_LANE_BLOCKS;
    int col = 0, blk = 0;
    if (j0 < r.nb) {
        const int row = j0 / r.bw;
        col = j0 - row * r.bw;
        blk = (r.by + row) * s.nbx + r.bx + col;
    }
    uint32_t ol[CR_LANE_BLOCKS], bits4 = 0u;
#pragma unroll
    for (int i = 0; i < CR_LANE_BLOCKS; ++i) {
        const int j = j0 + i;
        ol[i] = 0u;
        if (j >= r.nb) continue;
        if (i > 0) crop_step(s, r, col, blk);
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
    if (bits4 != 0u) atomicOr(&s_mask[threadIdx.x >> 3], bits4 << (CR_LANE_BLOCKS * (threadIdx.x & 7)));
    __syncthreads();

    // the run heads: count = up to the next written block, the next multiple of 1023, nb — all in the rectangle's numbering
#pragma unroll
    for (int i = 0; i < CR_LANE_BLOCKS; ++i) {
        if ((ol[i] & 0xFFu) != MSV1_DELTA_SKIP) continue;
        const int j = j0 + i;
        const uint32_t at = lo + (ol[i] >> 8);
        if (at + 2u > hi) continue;                                             // (never holds)
        const int q = (int)threadIdx.x * CR_LANE_BLOCKS + i + 1;                // the first block behind the head, within the workgroup
        uint32_t next = MSV1_DELTA_NONE;
        for (int w = q >> 5; w < CR_WG_BLOCKS / 32 && next == MSV1_DELTA_NONE; ++w) {
            uint32_t m = s_mask[w];
            if (w == (q >> 5)) m &= 0xFFFFFFFFu << (q & 31);
            if (m != 0u) next = (uint32_t)(g * CR_WG_BLOCKS + 32 * w + __builtin_ctz(m));
        }
        for (int k = g + 1; k <= g + 2 && k < nwg && next == MSV1_DELTA_NONE; ++k) next = *(cgu32*)(d.first_written + (size_t)pair * nwg + k);
        const uint32_t limit = min((uint32_t)(j / MSV1_DELTA_RUN + 1) * (uint32_t)MSV1_DELTA_RUN, (uint32_t)r.nb);
        const uint32_t count = min(next, limit) - (uint32_t)j;
        s_img[at >> 1] = (uint16_t)((count & 0xFFu) | ((0x84u + (count >> 8)) << 8));
    }
    __syncthreads();

    index_image_store(d.out + (base - lo), s_img, lo, hi);                       // (d.out is 16-byte aligned, so is this)
}

}  // namespace

void msv1_launch_index_crop_sizes(const Msv1IndexSrc& src, const Msv1CropRect& r, int npairs, const Msv1CropScratch& d, bool tight,
                                  hipStream_t stream) {
    if (r.nb <= 0 || npairs <= 0) return;
    const dim3 grid((unsigned)msv1_keyframe_workgroups(r.nb), (unsigned)npairs);
    if (tight) {
        if (src.bits == 16) hipLaunchKernelGGL((msv1_index_crop_sizes_kernel<16, true>), grid, dim3(WG), 0, stream, src, r, d);
        else hipLaunchKernelGGL((msv1_index_crop_sizes_kernel<8, true>), grid, dim3(WG), 0, stream, src, r, d);
    } else if (src.bits == 16) {
        hipLaunchKernelGGL((msv1_index_crop_sizes_kernel<16, false>), grid, dim3(WG), 0, stream, src, r, d);
    } else {
        hipLaunchKernelGGL((msv1_index_crop_sizes_kernel<8, false>), grid, dim3(WG), 0, stream, src, r, d);
    }
}

void msv1_launch_index_crop_gather(const Msv1IndexSrc& src, const Msv1CropRect& r, int npairs, const Msv1CropScratch& d, hipStream_t stream) {
    if (r.nb <= 0 || npairs <= 0) return;
    const dim3 grid((unsigned)msv1_keyframe_workgroups(r.nb), (unsigned)npairs);
    if (src.bits == 16) hipLaunchKernelGGL(msv1_index_crop_gather_kernel<16>, grid, dim3(WG), 0, stream, src, r, d);
    else hipLaunchKernelGGL(msv1_index_crop_gather_kernel<8>, grid, dim3(WG), 0, stream, src, r, d);
}

}  // namespace jsp
