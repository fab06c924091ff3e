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
// The shape, the two kernels' bodies and their launch are the clip skeleton's (msv1_index_clip_device.h), shared with the crop, pan and
// path calls: here src(j) = j over the whole grid, no pair is a key pair, and nobody asks for the workgroups' code counts.  The status
// word is the skeleton's, block << 1 | MSV1_KEYFRAME_CUT.
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
#include "msv1_index_clip_device.h"

namespace jsp {
namespace {

// The rule of a pair (a, b]: written, and with TIGHT kept.  f: the last writer <= b.
template <int BITS, bool TIGHT>
struct DeltaRule {
    static constexpr bool key = false, counts = false;
    int a, b;
    __device__ __forceinline__ bool coded(const Msv1IndexSrc& s, int blk, const uint32_t* s_pal, int& f) const {
        return delta_written(s, blk, a, b, f) && (!TIGHT || tight_kept<BITS>(s, blk, a, f, s_pal));
    }
};

// TIGHT = false is jsp_index_delta_frames' kernel; TIGHT = true applies THE TIGHT RULE: "written" then reads "kept".
template <int BITS, bool TIGHT>
__global__ __launch_bounds__(INDEX_CODES_WG) void msv1_index_delta_sizes_kernel(const Msv1IndexSrc s, Msv1ClipScratch d) {
    const DeltaRule<BITS, TIGHT> rule{d.pairs[2 * blockIdx.y], d.pairs[2 * blockIdx.y + 1]};
    clip_sizes_body<BITS, TIGHT>(s, ClipGridSrc{s.nblocks}, rule, d);
}

template <int BITS>
__global__ __launch_bounds__(INDEX_CODES_WG) void msv1_index_delta_gather_kernel(const Msv1IndexSrc s, Msv1ClipScratch d) {
    clip_gather_body<BITS>(s, ClipGridSrc{s.nblocks}, d);
}

}  // namespace

void msv1_launch_index_delta_sizes(const Msv1IndexSrc& src, int npairs, const Msv1ClipScratch& d, bool tight, hipStream_t stream) {
    clip_launch(src.nblocks, npairs, src.bits, tight, [&](dim3 grid, dim3 wg, auto bits, auto tight_) {
        hipLaunchKernelGGL((msv1_index_delta_sizes_kernel<decltype(bits)::value, decltype(tight_)::value>), grid, wg, 0, stream, src, d);
    });
}

void msv1_launch_index_delta_gather(const Msv1IndexSrc& src, int npairs, const Msv1ClipScratch& d, hipStream_t stream) {
    clip_launch(src.nblocks, npairs, src.bits, false, [&](dim3 grid, dim3 wg, auto bits, auto) {
        hipLaunchKernelGGL(msv1_index_delta_gather_kernel<decltype(bits)::value>, grid, wg, 0, stream, src, d);
    });
}

}  // namespace jsp
