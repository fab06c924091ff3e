// A key frame for any frame of an MSVideo1 seek index for gfx950 (MI355X): the stream bytes that, decoded as a key frame, give the
// picture of index frame t (jsp_index_key_frame) — TWO launches, no pixel decoded, nothing re-quantised.  Host side in msv1_seek.cpp.
//
// THE RULE.  Let e be the end of the writer's frame data (16-bit: rounded down to a whole word, as decode_at does).  The code at
// offset o is WHOLE when (1) its two-byte code word lies below e, (2) the bytes that settle its length lie below e — for a 16-bit code
// with b < 0x80 that is the colour word at o + 2 — and (3) o + L <= e.  L follows MSVideo1.hx:135-181 (16-bit: 1-colour 2, 2-colour
// 6, 8-colour 18 bytes) and :319-364 (8-bit: 2, 4, 10).  KeyFrame(t) = for blocks 0 .. nblocks-1 in table order (which is stream
// order), the L bytes of the whole code of the block's last writer <= t.  No skip codes, no end marker, nothing after the last block.
// A block with no writer <= t in the index, or whose last writer's code is not whole, makes t uncuttable: the status word names the
// FIRST such block, and the host writes nothing.
//
// TWO launches, and why not one: the output position of a block is a prefix sum over data.  A single pass would have a workgroup
// wait for the totals of the workgroups before it (a scan with look-back), that is spin on other workgroups' progress.  Here no
// workgroup ever waits for another: launch 1 leaves per-workgroup totals, launch 2 sums the ones before its own.
//
// Launch 1, msv1_index_keyframe_sizes_kernel.  A lane owns KF_LANE_BLOCKS consecutive blocks, a workgroup KF_WG_BLOCKS.  Per block:
// the last writer (index_last_writer / index_word_frame, msv1_block_io.h), its table entry, the code's head bytes, and so L — or a
// status, which goes into the status word by atomicMin over (block, kind).  An exclusive scan of L inside the workgroup (shuffles
// within a wave, LDS across the waves) gives every block its offset within the workgroup's output; the record of a block is its
// writer frame and (offset << 8 | L), L = 0 for a block with a status.  totals[g] = the bytes of workgroup g.
//
// Launch 2, msv1_index_keyframe_gather_kernel.  Workgroup g sums totals[0 .. g): its base.  Every lane copies its blocks' code bytes,
// 16 bits at a time (offsets and lengths are always even), into an LDS image of the workgroup's output, which starts base % 16 bytes
// into the LDS array: LDS and global positions then agree modulo 16.  The image leaves in 16-byte pieces, whole pieces as one 16-byte
// store; the first and the last piece, where the image covers only a part, 16 bits at a time (base is even, nothing more).  The last
// workgroup writes the frame's length next to the status word.
#include "msv1_index_codes.h"

namespace jsp {
namespace {

constexpr int WG = INDEX_CODES_WG;
constexpr int KF_LANE_BLOCKS = 4;
constexpr int KF_WG_BLOCKS = MSV1_KEYFRAME_WG_BLOCKS;   // (msv1_seek.h: the host sizes totals[] by it)
static_assert(KF_WG_BLOCKS == WG * KF_LANE_BLOCKS, "a lane owns KF_LANE_BLOCKS consecutive blocks");

template <int BITS>
__global__ __launch_bounds__(WG) void msv1_index_keyframe_sizes_kernel(const Msv1IndexSrc s, int t, Msv1KeyFrameScratch k) {
    __shared__ uint32_t s_wave[WG / 64];
    const int blk0 = (int)blockIdx.x * KF_WG_BLOCKS + (int)threadIdx.x * KF_LANE_BLOCKS;
    uint32_t frame[KF_LANE_BLOCKS], len[KF_LANE_BLOCKS];
    uint32_t worst = 0xFFFFFFFFu;   // the lane's first block with a status: (block << 1 | kind)
#pragma unroll
    for (int i = 0; i < KF_LANE_BLOCKS; ++i) {
        const int blk = blk0 + i;
        frame[i] = 0u;
        len[i] = 0u;
        if (blk >= s.nblocks) continue;
        int w;
        const uint32_t m = index_last_writer(s, blk, t, w);
        uint32_t kind = MSV1_KEYFRAME_NO_WRITER;
        if (m != 0u) {
            const int f = index_word_frame(w, m);
            uint32_t o, e;
            const Msv1IndexChunk ch = index_code_at(s, f, blk, BITS, o, e);
            frame[i] = (uint32_t)f;
            len[i] = index_whole_length<BITS>(ch, o, e);
            kind = len[i] != 0u ? 0xFFFFFFFFu : MSV1_KEYFRAME_CUT;
        }
        if (kind != 0xFFFFFFFFu) worst = min(worst, ((uint32_t)blk << 1) | kind);
    }
    if (worst != 0xFFFFFFFFu) atomicMin(k.status, worst);

    // exclusive scan of the lengths over the workgroup
    uint32_t mine = 0u;
#pragma unroll
    for (int i = 0; i < KF_LANE_BLOCKS; ++i) mine += len[i];
    uint32_t total;
    uint32_t off = index_wg_scan(mine, s_wave, total);
#pragma unroll
    for (int i = 0; i < KF_LANE_BLOCKS; ++i) {
        const int blk = blk0 + i;
        if (blk < s.nblocks) {
            *(gu32*)(k.records + 2 * (size_t)blk) = frame[i];
            *(gu32*)(k.records + 2 * (size_t)blk + 1) = (off << 8) | len[i];
        }
        off += len[i];
    }
    if (threadIdx.x == 0) *(gu32*)(k.totals + blockIdx.x) = total;
}

template <int BITS>
__global__ __launch_bounds__(WG) void msv1_index_keyframe_gather_kernel(const Msv1IndexSrc s, Msv1KeyFrameScratch k) {
    constexpr int IMAGE = KF_WG_BLOCKS * (BITS == 16 ? 18 : 10);                 // bytes of a workgroup's output at its bound
    __shared__ __attribute__((aligned(16))) uint16_t s_img[(IMAGE + 16) / 2];   // (+ 16: the image starts base % 16 bytes in)
    __shared__ uint32_t s_wave[WG / 64];
    const size_t base = index_wg_bytes_before(k.totals, (int)blockIdx.x, s_wave);   // the bytes of the workgroups before this one
    const uint32_t total = *(cgu32*)(k.totals + blockIdx.x);
    const uint32_t lo = (uint32_t)(base & 15), hi = lo + total;                  // the image is s_img bytes [lo, hi)

    const int blk0 = (int)blockIdx.x * KF_WG_BLOCKS + (int)threadIdx.x * KF_LANE_BLOCKS;
#pragma unroll
    for (int i = 0; i < KF_LANE_BLOCKS; ++i) {
        const int blk = blk0 + i;
        if (blk >= s.nblocks) continue;
        const uint32_t f = *(cgu32*)(k.records + 2 * (size_t)blk), ol = *(cgu32*)(k.records + 2 * (size_t)blk + 1);
        const uint32_t L = ol & 0xFFu, at = lo + (ol >> 8);
        if (L == 0u || at + L > hi) continue;                                   // (a block with a status; the second test never holds)
        uint32_t o, e;
        const Msv1IndexChunk ch = index_code_at(s, (int)f, blk, BITS, o, e);
        for (uint32_t b = 0; b < L; b += 2u) s_img[(at + b) >> 1] = *(cgu16*)(ch.stream + o + b);
    }
    __syncthreads();

    index_image_store(k.out + (base - lo), s_img, lo, hi);                       // (16-byte aligned; piece c is bytes [16 c, 16 c + 16))
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) *(gu32*)(k.status + 1) = (uint32_t)base + total;
}

}  // namespace

void msv1_launch_index_keyframe(const Msv1IndexSrc& src, int t, const Msv1KeyFrameScratch& k, hipStream_t stream) {
    if (src.nblocks <= 0) return;
    const dim3 grid((unsigned)msv1_keyframe_workgroups(src.nblocks));
    if (src.bits == 16) {
        hipLaunchKernelGGL(msv1_index_keyframe_sizes_kernel<16>, grid, dim3(WG), 0, stream, src, t, k);
        hipLaunchKernelGGL(msv1_index_keyframe_gather_kernel<16>, grid, dim3(WG), 0, stream, src, k);
    } else {
        hipLaunchKernelGGL(msv1_index_keyframe_sizes_kernel<8>, grid, dim3(WG), 0, stream, src, t, k);
        hipLaunchKernelGGL(msv1_index_keyframe_gather_kernel<8>, grid, dim3(WG), 0, stream, src, k);
    }
}

}  // namespace jsp
