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
// The shape, the two kernels' bodies and their launch are the clip skeleton's (msv1_index_clip_device.h), shared with the delta, pan and
// path calls.  What this call supplies:
//   * src(j) of the rectangle of the launch (ClipRectSrc there: ONE division per lane, then the column steps with a wrap into the next
//     row); the workgroup's first lane looks at block j0 - 1 of the rectangle, src(j0 - 1);
//   * the pair word says key: an unwritten block then raises the status instead of becoming a run;
//   * the sizes kernel also leaves, per pair and workgroup, the number of blocks that got a code.  The host sums them: a frame that
//     codes all nb blocks is a key frame.
// Records, totals and first_written are in j-numbering.
#include "msv1_index_clip_device.h"

namespace jsp {
namespace {

// Whether source block `blk` counts for the pair: a key pair — some frame <= b codes it; a gap pair — written (TIGHT: kept) in (a, b].
// f: its last writer <= b.
template <int BITS, bool TIGHT>
struct CropRule {
    static constexpr bool counts = true;
    int a, b;
    bool key;
    __device__ __forceinline__ bool coded(const Msv1IndexSrc& s, int blk, const uint32_t* s_pal, int& f) const {
        if (!delta_written(s, blk, key ? -1 : a, b, f)) return false;
        return !TIGHT || key || tight_kept<BITS>(s, blk, a, f, s_pal);
    }
};

// TIGHT = true applies THE TIGHT RULE to the gap pairs: "written" then reads "kept".
template <int BITS, bool TIGHT>
__global__ __launch_bounds__(INDEX_CODES_WG) void msv1_index_crop_sizes_kernel(const Msv1IndexSrc s, const Msv1CropRect r, Msv1ClipScratch d) {
    const int a = d.pairs[2 * blockIdx.y], b = d.pairs[2 * blockIdx.y + 1];
    clip_sizes_body<BITS, TIGHT>(s, clip_rect_src(s, r), CropRule<BITS, TIGHT>{a, b, a == MSV1_CROP_KEY}, d);
}

template <int BITS>
__global__ __launch_bounds__(INDEX_CODES_WG) void msv1_index_crop_gather_kernel(const Msv1IndexSrc s, const Msv1CropRect r, Msv1ClipScratch d) {
    clip_gather_body<BITS>(s, clip_rect_src(s, r), d);
}

}  // namespace

void msv1_launch_index_crop_sizes(const Msv1IndexSrc& src, const Msv1CropRect& r, int npairs, const Msv1ClipScratch& d, bool tight,
                                  hipStream_t stream) {
    clip_launch(r.nb, npairs, src.bits, tight, [&](dim3 grid, dim3 wg, auto bits, auto tight_) {
        hipLaunchKernelGGL((msv1_index_crop_sizes_kernel<decltype(bits)::value, decltype(tight_)::value>), grid, wg, 0, stream, src, r, d);
    });
}

void msv1_launch_index_crop_gather(const Msv1IndexSrc& src, const Msv1CropRect& r, int npairs, const Msv1ClipScratch& d, hipStream_t stream) {
    clip_launch(r.nb, npairs, src.bits, false, [&](dim3 grid, dim3 wg, auto bits, auto) {
        hipLaunchKernelGGL(msv1_index_crop_gather_kernel<decltype(bits)::value>, grid, wg, 0, stream, src, r, d);
    });
}

}  // namespace jsp
