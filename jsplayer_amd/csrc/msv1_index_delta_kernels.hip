// An inter frame that spans a gap of an MSVideo1 seek index for gfx950 (MI355X): the stream bytes that, decoded as an inter frame on
// top of the picture of index frame a, give the picture of index frame b (jsp_index_delta_frames) — TWO launches for any number of
// pairs (a, b], no pixel decoded, nothing re-quantised.  Host side in msv1_seek.cpp.
//
// THE RULE.  WHOLE is the key frame's definition (msv1_index_keyframe_kernels.hip).  Block i is WRITTEN in (a, b] when some frame f
// with a < f <= b codes it: index_last_writer(s, i, b, w) is non-zero and names a frame > a.  a = -1 means "from before the range".
// Delta(a, b), -1 <= a < b < nframes = for blocks i = 0 .. nblocks-1 in table order:
//   * i is written: the L bytes of the whole code of its last writer <= b;
//   * i is not written and is a RUN HEAD — i = 0, or block i - 1 is written, or i % 1023 = 0: one skip word, bytes (count & 0xFF,
//     0x84 + (count >> 8)), count = the consecutive unwritten blocks from i on, stopping before the next written block, before the
//     next multiple of 1023 above i, and at nblocks: 1 <= count <= 1023;
//   * otherwise: nothing.
// A skip word never crosses a block number that is a multiple of 1023 (MSVideo1.hx:131-133, :315-317: the count has 10 bits), so a
// block's contribution follows from the block and its one neighbour, and the look-ahead for a count is at most 1022 blocks.  The
// frame always covers all nblocks blocks.  A written block whose last writer's code is not whole makes the pair uncuttable: the
// pair's status word names the FIRST such block, and the host writes nothing.  A block without a writer is skipped, never refused.
//
// The shape is the key frame's, with grid.y = the pair: no workgroup ever waits for another.  A lane owns DL_LANE_BLOCKS
// consecutive blocks, a workgroup DL_WG_BLOCKS.
//
// Launch 1, msv1_index_delta_sizes_kernel.  Per block: written or not, L or the status, the run-head test — block i - 1 is the
// lane's own previous block, else the neighbour lane's last block through LDS, else (the workgroup's first block) a walk of its
// own.  An exclusive scan of the contributions (L, 2 for a run head, 0) gives every block its offset within the workgroup's
// output; per pair and workgroup go out the total and the first written block.
//
// Launch 2, msv1_index_delta_gather_kernel.  Workgroup g of pair p starts at bases[p] + totals[p][0 .. g).  Codes travel through an
// LDS image and leave in 16-byte pieces, as in the key frame's gather.  The count of a run head: the next written block from an LDS
// bitmask of the workgroup's records, beyond the workgroup from first_written of the next two workgroups (1022 blocks ahead never
// reach further), clipped by the multiple of 1023 and by nblocks.
//
// THE TIGHT RULE (jsp_index_tight_frames; the sizes kernel's TIGHT form, the gather kernel as it is).  P(t)[i] is index_block's: the
// 16 frame-buffer words that the last frame <= t coding block i makes of it (a code that the frame's end cuts off decoded by
// decode_at's rule), else the block of the picture before the index; P(a)[i] is DEFINED when one of the two exists (a = -1: only the
// picture before the index can define it).  Block i is KEPT in (a, b] when it is written in (a, b] and P(a)[i] is not defined or
// differs from P(b)[i] in at least one of the 16 words; every other block is DROPPED.  Tight(a, b) is Delta(a, b) with "written"
// replaced by "kept" everywhere — codes, run heads (is block i - 1 kept?), counts — and only a KEPT block whose last writer's code is
// not whole refuses: no byte of a dropped block is used.  Words are compared as a frame buffer holds them: two palette indices of
// one colour are equal, and so are different code bytes that decode alike.  The sizes kernel takes a lane's blocks one after the
// other, 2 x 16 pixel registers at a time; records, totals and first_written then say "kept" where they said "written".
#include "msv1_index_codes.h"

namespace jsp {
namespace {

constexpr int WG = INDEX_CODES_WG;
constexpr int DL_LANE_BLOCKS = 4;
constexpr int DL_WG_BLOCKS = MSV1_KEYFRAME_WG_BLOCKS;   // (msv1_seek.h: the host sizes totals[] and first_written[] by it)
static_assert(DL_WG_BLOCKS == WG * DL_LANE_BLOCKS, "a lane owns DL_LANE_BLOCKS consecutive blocks");
static_assert(2 * DL_WG_BLOCKS >= MSV1_DELTA_RUN, "a count's look-ahead ends within the next two workgroups");

// TIGHT = false is jsp_index_delta_frames' kernel; TIGHT = true applies THE TIGHT RULE: `written` below then reads "kept".
template <int BITS, bool TIGHT>
__global__ __launch_bounds__(WG) void msv1_index_delta_sizes_kernel(const Msv1IndexSrc s, Msv1DeltaScratch d) {
    __shared__ uint32_t s_pal[TIGHT && BITS == 8 ? 256 : 1];
    if (TIGHT) load_palette<BITS>(s_pal, s.palette);
    __shared__ uint32_t s_wave[WG / 64];
    __shared__ uint32_t s_first[WG / 64];
    __shared__ uint8_t s_last[WG];                       // per lane: its last block is written
    const int pair = (int)blockIdx.y, nwg = (int)gridDim.x;
    const int a = d.pairs[2 * pair], b = d.pairs[2 * pair + 1];
    const int blk0 = (int)blockIdx.x * DL_WG_BLOCKS + (int)threadIdx.x * DL_LANE_BLOCKS;
    uint32_t frame[DL_LANE_BLOCKS], len[DL_LANE_BLOCKS];
    bool written[DL_LANE_BLOCKS];
    uint32_t worst = 0xFFFFFFFFu, first = MSV1_DELTA_NONE;
#pragma unroll
    for (int i = 0; i < DL_LANE_BLOCKS; ++i) {
        const int blk = blk0 + i;
        frame[i] = 0u;
        len[i] = 0u;
        written[i] = false;
        if (blk >= s.nblocks) continue;
        int f;
        if (!delta_written(s, blk, a, b, f)) continue;
        if (TIGHT && !tight_kept<BITS>(s, blk, a, f, s_pal)) continue;
        written[i] = true;
        first = min(first, (uint32_t)blk);
        uint32_t o, e;
        const Msv1IndexChunk ch = index_code_at(s, f, blk, BITS, o, e);
        frame[i] = (uint32_t)f;
        len[i] = index_whole_length<BITS>(ch, o, e);
        if (len[i] == 0u) worst = min(worst, (uint32_t)blk);
    }
    if (worst != 0xFFFFFFFFu) atomicMin(d.status + pair, worst);

    // the block before the lane's first one: the neighbour lane's last block; the workgroup's first lane walks for it
    s_last[threadIdx.x] = written[DL_LANE_BLOCKS - 1] ? 1 : 0;
    bool before = true;                                  // (block 0 is a run head: as if a written block stood before it)
    if (threadIdx.x == 0 && blk0 > 0 && blk0 < s.nblocks) {
        int f;
        before = delta_written(s, blk0 - 1, a, b, f) && (!TIGHT || tight_kept<BITS>(s, blk0 - 1, a, f, s_pal));
    }
    __syncthreads();
    if (threadIdx.x > 0) before = s_last[threadIdx.x - 1] != 0;
#pragma unroll
    for (int i = 0; i < DL_LANE_BLOCKS; ++i) {
        const int blk = blk0 + i;
        if (blk < s.nblocks && !written[i] && (before || blk % MSV1_DELTA_RUN == 0)) len[i] = MSV1_DELTA_SKIP;
        before = written[i];
    }

    // exclusive scan of the contributions over the workgroup; the workgroup's first written block
    uint32_t mine = 0u;
#pragma unroll
    for (int i = 0; i < DL_LANE_BLOCKS; ++i) mine += len[i] == MSV1_DELTA_SKIP ? 2u : len[i];
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
#pragma unroll
    for (int k = 1; k < 64; k <<= 1) first = min(first, (uint32_t)__shfl_xor((int)first, k));
    if (lane == 0) s_first[wave] = first;
    uint32_t total;
    uint32_t off = index_wg_scan(mine, s_wave, total);   // (its barrier also publishes s_first)
    uint32_t* records = d.records + 2 * (size_t)pair * (size_t)s.nblocks;
#pragma unroll
    for (int i = 0; i < DL_LANE_BLOCKS; ++i) {
        const int blk = blk0 + i;
        if (blk < s.nblocks) {
            *(gu32*)(records + 2 * (size_t)blk) = frame[i];
            *(gu32*)(records + 2 * (size_t)blk + 1) = (off << 8) | len[i];
        }
        off += len[i] == MSV1_DELTA_SKIP ? 2u : len[i];
    }
    if (threadIdx.x == 0) {
        uint32_t f0 = s_first[0];
#pragma unroll
        for (int v = 1; v < WG / 64; ++v) f0 = min(f0, s_first[v]);
        *(gu32*)(d.totals + (size_t)pair * nwg + blockIdx.x) = total;
        *(gu32*)(d.first_written + (size_t)pair * nwg + blockIdx.x) = f0;
    }
}

template <int BITS>
__global__ __launch_bounds__(WG) void msv1_index_delta_gather_kernel(const Msv1IndexSrc s, Msv1DeltaScratch d) {
    constexpr int IMAGE = DL_WG_BLOCKS * (BITS == 16 ? 18 : 10);                 // bytes of a workgroup's output at its bound
    __shared__ __attribute__((aligned(16))) uint16_t s_img[(IMAGE + 16) / 2];   // (+ 16: the image starts base % 16 bytes in)
    __shared__ uint32_t s_wave[WG / 64];
    __shared__ uint32_t s_mask[DL_WG_BLOCKS / 32];                               // bit k of word j: block 32 j + k of the workgroup is written
    const int pair = (int)blockIdx.y, nwg = (int)gridDim.x, g = (int)blockIdx.x;
    const uint32_t* totals = d.totals + (size_t)pair * nwg;
    const uint32_t* records = d.records + 2 * (size_t)pair * (size_t)s.nblocks;
    if (threadIdx.x < DL_WG_BLOCKS / 32) s_mask[threadIdx.x] = 0u;
    const size_t base = (size_t)d.bases[pair] + index_wg_bytes_before(totals, g, s_wave);   // (its barrier also publishes the zeroed mask)
    const uint32_t total = *(cgu32*)(totals + g);
    const uint32_t lo = (uint32_t)(base & 15), hi = lo + total;                  // the image is s_img bytes [lo, hi)

    const int blk0 = g * DL_WG_BLOCKS + (int)threadIdx.x * DL_LANE_BLOCKS;
    uint32_t ol[DL_LANE_BLOCKS], bits4 = 0u;
#pragma unroll
    for (int i = 0; i < DL_LANE_BLOCKS; ++i) {
        const int blk = blk0 + i;
        ol[i] = 0u;
        if (blk >= s.nblocks) continue;
        const uint32_t f = *(cgu32*)(records + 2 * (size_t)blk);
        ol[i] = *(cgu32*)(records + 2 * (size_t)blk + 1);
        const uint32_t L = ol[i] & 0xFFu, at = lo + (ol[i] >> 8);
        if (L < 2u || at + L > hi) continue;                                    // (nothing or a run head; the second test never holds)
        bits4 |= 1u << i;
        uint32_t o, e;
        const Msv1IndexChunk ch = index_code_at(s, (int)f, blk, BITS, o, e);
        for (uint32_t k = 0; k < L; k += 2u) s_img[(at + k) >> 1] = *(cgu16*)(ch.stream + o + k);
    }
    if (bits4 != 0u) atomicOr(&s_mask[threadIdx.x >> 3], bits4 << (DL_LANE_BLOCKS * (threadIdx.x & 7)));
    __syncthreads();

    // the run heads: count = up to the next written block, the next multiple of 1023, nblocks
#pragma unroll
    for (int i = 0; i < DL_LANE_BLOCKS; ++i) {
        if ((ol[i] & 0xFFu) != MSV1_DELTA_SKIP) continue;
        const int blk = blk0 + i;
        const uint32_t at = lo + (ol[i] >> 8);
        if (at + 2u > hi) continue;                                             // (never holds)
        const int j = (int)threadIdx.x * DL_LANE_BLOCKS + i + 1;                // the first block behind the head, within the workgroup
        uint32_t next = MSV1_DELTA_NONE;
        for (int w = j >> 5; w < DL_WG_BLOCKS / 32 && next == MSV1_DELTA_NONE; ++w) {
            uint32_t m = s_mask[w];
            if (w == (j >> 5)) m &= 0xFFFFFFFFu << (j & 31);
            if (m != 0u) next = (uint32_t)(g * DL_WG_BLOCKS + 32 * w + __builtin_ctz(m));
        }
        for (int k = g + 1; k <= g + 2 && k < nwg && next == MSV1_DELTA_NONE; ++k) next = *(cgu32*)(d.first_written + (size_t)pair * nwg + k);
        const uint32_t limit = min((uint32_t)(blk / MSV1_DELTA_RUN + 1) * (uint32_t)MSV1_DELTA_RUN, (uint32_t)s.nblocks);
        const uint32_t count = min(next, limit) - (uint32_t)blk;
        s_img[at >> 1] = (uint16_t)((count & 0xFFu) | ((0x84u + (count >> 8)) << 8));
    }
    __syncthreads();

    index_image_store(d.out + (base - lo), s_img, lo, hi);                       // (d.out is 16-byte aligned, so is this)
}

}  // namespace

void msv1_launch_index_delta_sizes(const Msv1IndexSrc& src, int npairs, const Msv1DeltaScratch& d, bool tight, hipStream_t stream) {
    if (src.nblocks <= 0 || npairs <= 0) return;
    const dim3 grid((unsigned)msv1_keyframe_workgroups(src.nblocks), (unsigned)npairs);
    if (tight) {
        if (src.bits == 16) hipLaunchKernelGGL((msv1_index_delta_sizes_kernel<16, true>), grid, dim3(WG), 0, stream, src, d);
        else hipLaunchKernelGGL((msv1_index_delta_sizes_kernel<8, true>), grid, dim3(WG), 0, stream, src, d);
    } else if (src.bits == 16) {
        hipLaunchKernelGGL((msv1_index_delta_sizes_kernel<16, false>), grid, dim3(WG), 0, stream, src, d);
    } else {
        hipLaunchKernelGGL((msv1_index_delta_sizes_kernel<8, false>), grid, dim3(WG), 0, stream, src, d);
    }
}

void msv1_launch_index_delta_gather(const Msv1IndexSrc& src, int npairs, const Msv1DeltaScratch& d, hipStream_t stream) {
    if (src.nblocks <= 0 || npairs <= 0) return;
    const dim3 grid((unsigned)msv1_keyframe_workgroups(src.nblocks), (unsigned)npairs);
    if (src.bits == 16) hipLaunchKernelGGL(msv1_index_delta_gather_kernel<16>, grid, dim3(WG), 0, stream, src, d);
    else hipLaunchKernelGGL(msv1_index_delta_gather_kernel<8>, grid, dim3(WG), 0, stream, src, d);
}

}  // namespace jsp
