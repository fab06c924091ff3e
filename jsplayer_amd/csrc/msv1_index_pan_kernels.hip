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
// The shape, the two kernels' bodies and their launch are the clip skeleton's (msv1_index_clip_device.h), shared with the delta, crop and
// path calls.  What this call supplies:
//   * the origins are per pair, read from the scratch beside the pair word (Msv1ClipScratch::origins): src(j) is the skeleton's
//     ClipRectSrc of rectangle B.  srcA(j) = srcB(j) + shift with ONE shift per pair, (A.y - B.y) * nbx + A.x - B.x;
//   * ONE test, PanRule::coded, with a branch on the pair word that is uniform over the workgroup (the pair is blockIdx.y).  KEY and STILL
//     pairs leave through crop's test first — an unwritten block, and every block of a key pair, decodes nothing — and a still tight
//     pair then compares what tight_kept compares.  A MOVED pair of a tight call skips that test and compares picture_block
//     (msv1_index_codes.h) of srcA(j) at `from` with that of srcB(j) at `to`, 16 words.  A moved pair of a call without the tight flag
//     arrives as the key pair (B, to): the host writes it so;
//   * the block before a workgroup's first block, j0 - 1, is judged by the same rule with both sources by the workgroup's first lane;
//   * the gather takes codes from srcB(j) only.
// The host has checked B, and for gap pairs A, against the block grid, so every srcB(j) and, where it is formed (gap pairs only), every
// srcA(j), j < nb, lies in [0, nblocks).
#include "msv1_index_clip_device.h"

namespace jsp {
namespace {

// Rectangle B of the workgroup's pair.
__device__ __forceinline__ ClipRectSrc pan_src(const Msv1IndexSrc& s, const Msv1ClipScratch& d, int bw, int bh) {
    return ClipRectSrc{s.nbx, d.origins[4 * blockIdx.y + 2], d.origins[4 * blockIdx.y + 3], bw, bw * bh};
}

// A pair as a workgroup sees it, and whether block `blk` = srcB(j) gets a code.  f: its last writer <= b, -1 without one.
//   KEY and STILL pairs, crop's test (delta_written, then tight_kept's compare): a key pair — some frame <= b codes it; a gap pair —
//     written (TIGHT: kept) in (a, b].  An unwritten block leaves before anything is decoded.
//   MOVED pairs of a tight call: KEPT — "written" plays no part, and P(b)[srcB(j)] may be the picture before the range.
// One compare serves both: P(a) of block blk + shift (shift = 0: the block itself) against P(b) of blk.
template <int BITS, bool TIGHT>
struct PanRule {
    static constexpr bool counts = true;
    int a, b;            // from, to
    bool key, moved;     // moved: A != B (a gap pair)
    int shift;           // what to add to srcB(j) for srcA(j) (0 for a key pair: A is not read)
    __device__ __forceinline__ PanRule(const Msv1IndexSrc& s, const Msv1ClipScratch& d, const ClipRectSrc& B) {
        const int pair = (int)blockIdx.y;
        a = d.pairs[2 * pair];
        b = d.pairs[2 * pair + 1];
        key = a == MSV1_CROP_KEY;
        shift = 0;
        if (!key) shift = (d.origins[4 * pair + 1] - B.by) * s.nbx + d.origins[4 * pair] - B.bx;
        moved = shift != 0;   // (both rectangles lie in the grid: the shift is 0 only for A == B)
    }
    __device__ __forceinline__ bool coded(const Msv1IndexSrc& s, int blk, const uint32_t* s_pal, int& f) const {
        int w;
        const uint32_t m = index_last_writer(s, blk, b, w);
        f = m != 0u ? index_word_frame(w, m) : -1;
        if (!(TIGHT && moved)) {
            if (f < 0 || (!key && f <= a)) return false;
            if (!TIGHT || key) return true;
        }
        uint32_t pa[16], pb[16];
        if (!picture_block_of<BITS>(s, blk, f, s_pal, pb)) return true;   // (this order: two registers fewer than the other one)
        if (!picture_block<BITS>(s, blk + shift, a, s_pal, pa)) return true;
        uint32_t diff = 0u;
#pragma unroll
        for (int k = 0; k < 16; ++k) diff |= pa[k] ^ pb[k];
        return diff != 0u;
    }
};

// TIGHT = true applies THE TIGHT RULE to the still gap pairs and the two-block compare to the moved ones: "written" then reads "kept".
// With TIGHT = false no pair is moved.  No occupancy attribute: asked for eight waves the compiler spills 32 to 48 SGPRs to get there;
// left alone the tight form takes 64 VGPRs and nothing is spilled (DESIGN.md has the report's figures).
template <int BITS, bool TIGHT>
__global__ __launch_bounds__(INDEX_CODES_WG) void msv1_index_pan_sizes_kernel(const Msv1IndexSrc s, const int bw, const int bh, Msv1ClipScratch d) {
    const ClipRectSrc B = pan_src(s, d, bw, bh);
    clip_sizes_body<BITS, TIGHT>(s, B, PanRule<BITS, TIGHT>(s, d, B), d);
}

template <int BITS>
__global__ __launch_bounds__(INDEX_CODES_WG) void msv1_index_pan_gather_kernel(const Msv1IndexSrc s, const int bw, const int bh, Msv1ClipScratch d) {
    clip_gather_body<BITS>(s, pan_src(s, d, bw, bh), d);
}

}  // namespace

void msv1_launch_index_pan_sizes(const Msv1IndexSrc& src, int bw, int bh, int npairs, const Msv1ClipScratch& d, bool tight, hipStream_t stream) {
    clip_launch(bw > 0 && bh > 0 ? bw * bh : 0, npairs, src.bits, tight, [&](dim3 grid, dim3 wg, auto bits, auto tight_) {
        hipLaunchKernelGGL((msv1_index_pan_sizes_kernel<decltype(bits)::value, decltype(tight_)::value>), grid, wg, 0, stream, src, bw, bh, d);
    });
}

void msv1_launch_index_pan_gather(const Msv1IndexSrc& src, int bw, int bh, int npairs, const Msv1ClipScratch& d, hipStream_t stream) {
    clip_launch(bw > 0 && bh > 0 ? bw * bh : 0, npairs, src.bits, false, [&](dim3 grid, dim3 wg, auto bits, auto) {
        hipLaunchKernelGGL(msv1_index_pan_gather_kernel<decltype(bits)::value>, grid, wg, 0, stream, src, bw, bh, d);
    });
}

}  // namespace jsp
