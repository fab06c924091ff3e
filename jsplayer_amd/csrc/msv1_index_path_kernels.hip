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
// The shape and the kernel's body are the clip skeleton's (msv1_index_clip_device.h), shared with the delta, crop and pan calls; src(j)
// is crop's.  What this call supplies is the decision per block, PathRule::coded: the pair's kind is read from (a, b), uniform over the
// workgroup (the pair is blockIdx.y); a BACK pair walks the writer bitmap twice, for the last writer <= hi and, only for a touched
// block, the last writer <= b; a tight pair decodes both ends through picture_block_of with the writers it already has.  The records
// it leaves, the totals, the counts and first_written are what msv1_index_crop_gather_kernel reads: there is no gather kernel here.
// The host has checked every pair against the index, so no walk starts above frame nframes - 1 or below frame 0.
#include "msv1_index_clip_device.h"

namespace jsp {
namespace {

// The last writer <= t of source block `blk`, -1 when there is none (t = -1: none).
__device__ __forceinline__ int path_last_writer(const Msv1IndexSrc& s, int blk, int t) {
    if (t < 0) return -1;
    int w;
    const uint32_t m = index_last_writer(s, blk, t, w);
    return m != 0u ? index_word_frame(w, m) : -1;
}

// Whether source block `blk` is KEPT by the pair (a, b).  f: its last writer <= b, -1 when a kept block has none (it refuses).
template <int BITS, bool TIGHT>
struct PathRule {
    static constexpr bool counts = true;
    int a, b;
    bool key;
    __device__ __forceinline__ bool coded(const Msv1IndexSrc& s, int blk, const uint32_t* s_pal, int& f) const {
        f = -1;
        if (key) {                                           // every block of a key pair is kept
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
};

// TIGHT = true applies the tight flag to the pairs that are not KEY.
template <int BITS, bool TIGHT>
__global__ __launch_bounds__(INDEX_CODES_WG) void msv1_index_path_sizes_kernel(const Msv1IndexSrc s, const Msv1CropRect r, Msv1ClipScratch d) {
    const int a = d.pairs[2 * blockIdx.y], b = d.pairs[2 * blockIdx.y + 1];
    clip_sizes_body<BITS, TIGHT>(s, clip_rect_src(s, r), PathRule<BITS, TIGHT>{a, b, a == MSV1_CROP_KEY}, d);
}

}  // namespace

void msv1_launch_index_path_sizes(const Msv1IndexSrc& src, const Msv1CropRect& r, int npairs, const Msv1ClipScratch& d, bool tight,
                                  hipStream_t stream) {
    clip_launch(r.nb, npairs, src.bits, tight, [&](dim3 grid, dim3 wg, auto bits, auto tight_) {
        hipLaunchKernelGGL((msv1_index_path_sizes_kernel<decltype(bits)::value, decltype(tight_)::value>), grid, wg, 0, stream, src, r, d);
    });
}

}  // namespace jsp
