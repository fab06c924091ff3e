// The frames of a block rectangle of an MSVideo1 seek index ALONG ANY PATH through it, for gfx950 (MI355X): the stream bytes of a clip
// that steps forward, backward or stands (jsp_index_path_frames) — a reversed clip, a boomerang, a freeze frame — TWO launches for any
// number of pairs, no pixel decoded to memory, nothing re-quantised.  An MSVideo1 code carries no position and no reference to the
// previous picture, so the inter frame that takes the picture of frame a BACK to the picture of frame b < a is a gather of codes the
// index holds, as the step forward is: a block some frame of (b, a] coded gets the code of its last writer <= b, every other block
// a skip.  Host side in msv1_seek.cpp; the gather launch is crop's own (msv1_index_crop_kernels.hip).
//
// THE RULE (PATH).  WHOLE (msv1_index_keyframe_kernels.hip), RUN HEAD, the skip word, the 1023 rule, P(t)[blk] and DEFINED
// (msv1_index_delta_kernels.hip), the rectangle (bx, by, bw, bh), nb and src(j) (msv1_index_crop_kernels.hip) are exactly those
// definitions, everything in the rectangle's j-numbering.  With the rectangle equal to the whole block grid src(j) = j.
// A pair (from = a, to = b) is one of four kinds.
//   KEY      a == JSP_CROP_KEY (-2), 0 <= b < nframes: crop's key pair — the whole code of the last writer <= b of every src(j), no
//            skip words; a block with no such writer refuses ("no writer"), a cut code refuses ("cut").  The tight flag does not
//            touch it.
//   FORWARD  -1 <= a < b < nframes: crop's gap pair.
//   HOLD     0 <= a == b < nframes: nothing is touched; the frame is ceil(nb / 1023) skip words.
//   BACK     0 <= b < a < nframes.
// ONE statement covers the three kinds that are not KEY.  Let lo = min(a, b), hi = max(a, b).
//   * Block j is TOUCHED when some frame f, lo < f <= hi, codes src(j): the last writer <= hi of src(j) is > lo.
//   * Without the tight flag a touched block is KEPT.  With it a touched block is DROPPED when P(a)[src(j)] and P(b)[src(j)] are both
//     DEFINED and equal in all 16 words, otherwise KEPT.
//   * A kept block contributes the whole code of the last writer <= b of src(j).  A kept block with no such writer refuses ("no
//     writer"): only a BACK pair can meet one, and it refuses even where the picture before the range defines P(b) — those pixels
//     come from no code the index holds.  A kept block whose code is cut off refuses ("cut").
//   * Dropped and untouched blocks are skipped under Delta's run-head and count rules in j — a run head is j = 0, or block j - 1 of
//     the rectangle kept, or j % 1023 = 0; counts stop at the next multiple of 1023 and at nb — and never refuse.
// For a FORWARD pair this is Delta, or with the flag Tight, of crop's virtual index, word for word.
// The status of a pair is crop's: min over (j << 1 | kind), the FIRST refusing block of the rectangle.
// PROMISED: a fresh decoder of 4 bw x 4 bh pixels fed a KEY pair's frame as a key frame, then the frames of pairs chained by
// to[k-1] == from[k] in any mix of kinds, holds after each the rectangle of the source picture of to[k].  keys[k] is 1 exactly when
// the frame codes all nb blocks.  A tight frame is never longer than the loose one.  Back(a, b) and Delta(b, a) have the same touched
// set, hence the same skip words when neither is tight.  A call of only KEY and FORWARD pairs returns byte for byte what
// jsp_index_crop_frames returns.  NOT promised: the exclusions of KeyFrame, and a step back to before the range (to = -1).
//
// The shape is the crop sizes kernel's, grid.y = the pair, no workgroup ever waits for another: a lane owns PA_LANE_BLOCKS
// consecutive blocks OF THE RECTANGLE, a workgroup PA_WG_BLOCKS; the block before a lane's first one is the neighbour lane's last
// block through LDS, the workgroup's first lane judges src(j0 - 1) by the same rule; bytes and code counts are scanned in one word.
// What differs is the decision per block, path_kept: the pair's kind is read from (a, b), uniform over the workgroup (the pair is
// blockIdx.y); a BACK pair walks the writer bitmap twice, for the last writer <= hi and, only for a touched block, the last writer
// <= b; a tight pair decodes both ends through picture_block_of with the writers it already has.  The records it leaves (writer
// frame, offset << 8 | length, MSV1_DELTA_SKIP for a run head), the totals, the counts and first_written are what
// msv1_index_crop_gather_kernel reads: there is no gather kernel here.  Lanes with j >= nb touch nothing, and no lane forms a source
// block for such a j: the host has checked the rectangle against the block grid, so every src(j), j < nb, lies in [0, nblocks), and
// every pair against the index, so no walk starts above frame nframes - 1 or below frame 0.
#include "msv1_index_codes.h"

namespace jsp {
namespace {

constexpr int WG = INDEX_CODES_WG;
constexpr int PA_LANE_BLOCKS = 4;
constexpr int PA_WG_BLOCKS = MSV1_KEYFRAME_WG_BLOCKS;   // (msv1_seek.h: the host sizes totals[], first_written[] and counts[] by it)
static_assert(PA_WG_BLOCKS == WG * PA_LANE_BLOCKS, "a lane owns PA_LANE_BLOCKS consecutive blocks");
static_assert(2 * PA_WG_BLOCKS >= MSV1_DELTA_RUN, "a count's look-ahead ends within the next two workgroups");
static_assert(PA_WG_BLOCKS * 18 < (1 << 16) && PA_WG_BLOCKS < (1 << 15), "bytes and codes of a workgroup share one scanned word");

// The last writer <= t of source block `blk`, -1 when there is none (t = -1: none).
__device__ __forceinline__ int path_last_writer(const Msv1IndexSrc& s, int blk, int t) {
    if (t < 0) return -1;
    int w;
    const uint32_t m = index_last_writer(s, blk, t, w);
    return m != 0u ? index_word_frame(w, m) : -1;
}

// Whether source block `blk` is KEPT by the pair (a, b).  f: its last writer <= b, -1 when a kept block has none (it refuses).
template <int BITS, bool TIGHT>
__device__ __forceinline__ bool path_kept(const Msv1IndexSrc& s, int blk, int a, int b, const uint32_t* s_pal, int& f) {
    f = -1;
    if (a == MSV1_CROP_KEY) {                            // every block of a key pair is kept
        f = path_last_writer(s, blk, b);
        return true;
    }
    const int lo = min(a, b), hi = max(a, b);
    if (lo == hi) return false;                          // HOLD
    const int fh = path_last_writer(s, blk, hi);         // (hi > lo >= -1)
    if (fh <= lo) return false;                          // not touched
    const bool back = a > b;
    const int fl = back || TIGHT ? path_last_writer(s, blk, lo) : -1;
    f = back ? fl : fh;
    if (TIGHT) {
        uint32_t pa[16], pb[16];
        if (picture_block_of<BITS>(s, blk, back ? fh : fl, s_pal, pa) && picture_block_of<BITS>(s, blk, f, s_pal, pb)) {
            uint32_t diff = 0u;
#pragma unroll
            for (int k = 0; k < 16; ++k) diff |= pa[k] ^ pb[k];
            if (diff == 0u) return false;                // dropped
        }
    }
    return true;
}

// TIGHT = true applies the tight flag to the pairs that are not KEY.
template <int BITS, bool TIGHT>
__global__ __launch_bounds__(WG) void msv1_index_path_sizes_kernel(const Msv1IndexSrc s, const Msv1CropRect r, Msv1CropScratch d) {
    __shared__ uint32_t s_pal[TIGHT && BITS == 8 ? 256 : 1];
    if (TIGHT) load_palette<BITS>(s_pal, s.palette);
    __shared__ uint32_t s_wave[WG / 64];
    __shared__ uint32_t s_first[WG / 64];
    __shared__ uint8_t s_last[WG];                       // per lane: its last block is kept
    const int pair = (int)blockIdx.y, nwg = (int)gridDim.x;
    const int a = d.pairs[2 * pair], b = d.pairs[2 * pair + 1];
    const bool key = a == MSV1_CROP_KEY;
    const int j0 = (int)blockIdx.x * PA_WG_BLOCKS + (int)threadIdx.x * PA_LANE_BLOCKS;
    int col = 0, blk = 0;                                // the column of block j in the rectangle, and src(j)
    if (j0 < r.nb) {
        const int row = j0 / r.bw;
        col = j0 - row * r.bw;
        blk = (r.by + row) * s.nbx + r.bx + col;
    }
    uint32_t frame[PA_LANE_BLOCKS], len[PA_LANE_BLOCKS];
    bool kept[PA_LANE_BLOCKS];
    uint32_t worst = 0xFFFFFFFFu, first = MSV1_DELTA_NONE;
#pragma unroll
    for (int i = 0; i < PA_LANE_BLOCKS; ++i) {
        const int j = j0 + i;
        frame[i] = 0u;
        len[i] = 0u;
        kept[i] = false;
        if (j >= r.nb) continue;
        if (i > 0) {                                     // src(j) from src(j - 1): the next column, or the first one of the next row
            ++blk;
            if (++col == r.bw) {
                col = 0;
                blk += s.nbx - r.bw;
            }
        }
        int f;
        if (!path_kept<BITS, TIGHT>(s, blk, a, b, s_pal, f)) continue;
        if (f < 0) {                                     // (no code to take: the pair refuses, nothing of it is gathered)
            worst = min(worst, ((uint32_t)j << 1) | MSV1_KEYFRAME_NO_WRITER);
            continue;
        }
        kept[i] = true;
        first = min(first, (uint32_t)j);
        uint32_t o, e;
        const Msv1IndexChunk ch = index_code_at(s, f, blk, BITS, o, e);
        frame[i] = (uint32_t)f;
        len[i] = index_whole_length<BITS>(ch, o, e);
        if (len[i] == 0u) worst = min(worst, ((uint32_t)j << 1) | MSV1_KEYFRAME_CUT);
    }
    if (worst != 0xFFFFFFFFu) atomicMin(d.status + pair, worst);

    // the block before the lane's first one: the neighbour lane's last block; the workgroup's first lane judges src(j0 - 1)
    s_last[threadIdx.x] = kept[PA_LANE_BLOCKS - 1] ? 1 : 0;
    bool before = true;                                  // (block 0 is a run head: as if a kept block stood before it)
    if (threadIdx.x == 0 && !key && j0 > 0 && j0 < r.nb) {   // (a key pair has no run heads: nothing to walk for)
        const int row = (j0 - 1) / r.bw;
        int f;
        before = path_kept<BITS, TIGHT>(s, (r.by + row) * s.nbx + r.bx + (j0 - 1 - row * r.bw), a, b, s_pal, f) && f >= 0;
    }
    __syncthreads();
    if (threadIdx.x > 0) before = s_last[threadIdx.x - 1] != 0;
#pragma unroll
    for (int i = 0; i < PA_LANE_BLOCKS; ++i) {
        const int j = j0 + i;
        if (j < r.nb && !key && !kept[i] && (before || j % MSV1_DELTA_RUN == 0)) len[i] = MSV1_DELTA_SKIP;
        before = kept[i];
    }

    // exclusive scan of the contributions over the workgroup (low half: bytes, high half: codes); its first kept block
    uint32_t mine = 0u;
#pragma unroll
    for (int i = 0; i < PA_LANE_BLOCKS; ++i) mine += len[i] == MSV1_DELTA_SKIP ? 2u : len[i] != 0u ? (1u << 16) | len[i] : 0u;
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
#pragma unroll
    for (int k = 1; k < 64; k <<= 1) first = min(first, (uint32_t)__shfl_xor((int)first, k));
    if (lane == 0) s_first[wave] = first;
    uint32_t total;
    uint32_t off = index_wg_scan(mine, s_wave, total) & 0xFFFFu;   // (its barrier also publishes s_first)
    uint32_t* records = d.records + 2 * (size_t)pair * (size_t)r.nb;
#pragma unroll
    for (int i = 0; i < PA_LANE_BLOCKS; ++i) {
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

}  // namespace

void msv1_launch_index_path_sizes(const Msv1IndexSrc& src, const Msv1CropRect& r, int npairs, const Msv1CropScratch& d, bool tight,
                                  hipStream_t stream) {
    if (r.nb <= 0 || npairs <= 0) return;
    const dim3 grid((unsigned)msv1_keyframe_workgroups(r.nb), (unsigned)npairs);
    if (tight) {
        if (src.bits == 16) hipLaunchKernelGGL((msv1_index_path_sizes_kernel<16, true>), grid, dim3(WG), 0, stream, src, r, d);
        else hipLaunchKernelGGL((msv1_index_path_sizes_kernel<8, true>), grid, dim3(WG), 0, stream, src, r, d);
    } else if (src.bits == 16) {
        hipLaunchKernelGGL((msv1_index_path_sizes_kernel<16, false>), grid, dim3(WG), 0, stream, src, r, d);
    } else {
        hipLaunchKernelGGL((msv1_index_path_sizes_kernel<8, false>), grid, dim3(WG), 0, stream, src, r, d);
    }
}

}  // namespace jsp
