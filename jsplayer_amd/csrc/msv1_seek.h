// The MSVideo1 range calls jsp_seek, jsp_find_change and jsp_index_* (msv1_seek.cpp, msv1_seek_kernels.hip): what they need from a
// staged batch and the codec, and their kernel launchers.
#pragma once
#include <vector>

#include "common.h"
#include "index_present.h"
#include "msv1.h"

struct jsp_staged;
struct jsp_codec;

namespace jsp {

// What a staged batch holds for the seek kernel: its stream buffer, block tables and frame records in HBM.
struct Msv1SeekView {
    Msv1Geometry geo{};
    const uint8_t* d_stream = nullptr;
    const uint32_t* d_desc = nullptr;       // frame f's table at f * desc_pitch
    size_t desc_pitch = 0;
    const Msv1FrameArgs* d_frames = nullptr;
    const Msv1FrameArgs* h_frames = nullptr;
    const int32_t* d_palette = nullptr;
    uint32_t* d_signif = nullptr;           // one word per frame (device) ...
    uint32_t* h_signif = nullptr;           // ... and its pinned host copy
    int nframes = 0;
};
// False when `st` is not a batch of the MSVideo1 staging (msv1_codec.cpp).
bool msv1_seek_view(jsp_staged* st, Msv1SeekView& out);
// ONE launch writes `dst` as frames [0, v.nframes) of the batch leave it when each frame's destination starts out holding the picture
// before it: every block from the last frame that coded it, else from `base` (the picture before the batch; null: left as it is);
// the pixels no block covers from `base` as well.  cmp_row_lo != ~0u: the stage-2 compare of the last frame (its coded blocks against
// the picture before it, rows >= cmp_row_lo) ORs v.d_signif[v.nframes - 1].
void msv1_launch_seek(const Msv1SeekView& v, int32_t* dst, const int32_t* base, uint32_t cmp_row_lo, hipStream_t stream);

// ONE launch of msv1_change_scan_kernel: for every frame f of the batch with d_rows[f] != ~0u, whether a block f codes differs, on
// pixel rows >= d_rows[f], from that block's previous state — what the last earlier frame of the batch that coded it made of it, else
// `before` (the picture before the batch) — ORs v.d_signif[f] (zeroed by the caller).  d_walk: the batch's frames that code a block,
// ascending, nwalk of them; frames after the last judged one need not be listed.  *d_first_hit (~0u from the caller) ends at most at
// the earliest frame found to differ, and the scan may stop there (jsp_find_change); null d_first_hit: every frame with a row is
// judged (jsp_index_build).
void msv1_launch_change_scan(const Msv1SeekView& v, const uint32_t* d_walk, int nwalk, const uint32_t* d_rows, uint32_t* d_first_hit,
                             const int32_t* before, hipStream_t stream);
// What MSVideo1 staging advances on the host (Msv1Codec::stage): a copy taken before a batch is staged puts the codec back where
// it stood, so that a prefix of the batch can be staged again and the state end at the prefix's last frame.  False: not MSVideo1.
struct Msv1HostState {
    int32_t* prev_dev = nullptr;
    std::vector<uint8_t> block_changes, last_full_frame;
    bool block_changes_stale = false;
    const void* last_full_dev = nullptr;
    size_t last_full_dev_bytes = 0;
};
bool msv1_save_state(jsp_codec* c, Msv1HostState& out);
void msv1_restore_state(jsp_codec* c, const Msv1HostState& s);

// ---- jsp_index_* -------------------------------------------------------------------------------------------------------------
// The per-row flags (block_changes) the codec's next host parse would start from — rebuilt from the last fully parsed frame when the
// codec keeps them stale — without changing the codec.  False: not MSVideo1.
bool msv1_block_changes_now(jsp_codec* c, std::vector<uint8_t>& out);
// The batch's stream buffer, block tables and frame records change hands (the batch keeps none of them; its next staging allocates
// afresh).  False: not a batch of the MSVideo1 staging.
bool msv1_take_batch(jsp_staged* st, DeviceBuffer& stream, DeviceBuffer& desc, DeviceBuffer& frames);
// What the index kernels read of one staged chunk of an index.
struct Msv1IndexChunk {
    const uint8_t* stream;
    const uint32_t* desc;            // the chunk's frame f at f * pitch (pitch = nblocks)
    const Msv1FrameArgs* frames;
    uint32_t first;                  // index frame of the chunk's frame 0
    uint32_t pad;
};
// ONE launch of msv1_coded_bitmap_kernel over the chunk `v` = index frames [a, a + v.nframes): bitmap (word-major, nblocks words per
// 32 frames, zeroed before the first chunk), d_rows (nby words per 32 frames, zeroed) and d_stop (one word per frame, all ones before).
void msv1_launch_coded_bitmap(const Msv1SeekView& v, int a, uint32_t* d_bitmap, uint32_t* d_rows, uint32_t* d_stop, hipStream_t stream);
// What every kernel of a seek index reads, and nothing a kernel writes: filled once, at the end of jsp_index_build (index_src,
// msv1_seek.cpp — the one place with the clamps that keep a picture of fewer than 4 pixels a side harmless), and passed to the
// kernels by value.
struct Msv1IndexSrc {
    const Msv1IndexChunk* chunks;
    const uint32_t* frame_chunk;     // the chunk of every frame
    const int32_t* palette;          // 8-bit: 256 entries
    const uint32_t* bitmap;          // word-major: bit k of word w * nblocks + blk says that frame 32 w + k codes block blk
    const uint32_t* before;          // the picture before the index, or null
    size_t pitch;                    // table entries per frame: nblocks, 1 at least
    int nblocks, nbx, nby;           // none below 0 (nbx is only divided by for a block below nblocks, so where it is 1 at least)
    int X, Y, bits;
    int before_vec;                  // blocks of `before` may be read 16 bytes a row
};
// ONE launch of msv1_index_show_kernel: frame t of the index into dst.
void msv1_launch_index_show(const Msv1IndexSrc& src, int t, int32_t* dst, hipStream_t stream);
// ONE launch of msv1_index_play_kernel: index frames first + k * stride, k < n, each into d_dsts[k] (a device array; a null entry is
// walked but not written) exactly as msv1_launch_index_show writes it.  The run is split into `segs` (clamped to 1..n) contiguous
// segments of destinations along grid.y, each composing its own first frame; the pictures do not depend on the split.
// dsts_aligned16: every non-null destination is 16-byte aligned (else the scalar instantiation).
void msv1_launch_index_play(const Msv1IndexSrc& src, int first, int n, int stride, int segs, int32_t* const* d_dsts, bool dsts_aligned16,
                            hipStream_t stream);
// Segments for a run of n frames when the caller leaves it to the library (option "msv1_index_play_segments" = "auto").
int msv1_index_play_auto_segments(const Msv1IndexSrc& src, int n);
// ONE launch of msv1_index_thumbs_kernel: the pictures of index frames d_frames[0..n) (a device array), each reduced scale x scale
// pixels to one (scale 4, 8 or 16; box mean, rounded half up), into the sheet `out`: thumbnails of (4 nbx / scale) x (4 nby / scale)
// pixels, `cols` to a sheet row, row pitch cols thumbnail widths.  A block nothing up to its frame coded comes from `before`, else is 0.
void msv1_launch_index_thumbs(const Msv1IndexSrc& src, const int32_t* d_frames, int n, int scale, int cols, int32_t* out, hipStream_t stream);
// ONE launch of msv1_index_present_kernel (msv1_index_present_kernels.hip): the windows `a` describes of the pictures of index frames
// d_frames[0..n) (a device array) — the pictures msv1_launch_index_show writes into a destination that held zeros, remainder pixels
// included — converted by `mode` and resampled by `filter` (0, 1 or JSP_PRESENT_AREA) into the cells of the sheet a.out.
void msv1_launch_index_present(const Msv1IndexSrc& src, const int32_t* d_frames, int n, const IndexPresentArgs& a, int mode, int filter,
                               hipStream_t stream);
// The same windows as elements of the dense tensor `t` describes (msv1_index_tensor_kernel): ONE launch; `a` has one column of cells.
void msv1_launch_index_tensor(const Msv1IndexSrc& src, const int32_t* d_frames, int n, const IndexPresentArgs& a, const IndexTensorArgs& t,
                              int mode, int filter, hipStream_t stream);
// ONE launch of msv1_index_activity_kernel (msv1_index_activity_kernels.hip): out[(k * rows + r) * cols + q], k < n, = the pixels of
// the 16x16 cell (r, q) of the cols x rows grid (ceil(X / 16) x ceil(Y / 16)) that differ between the pictures of index frames
// first + k and first + k - 1 (the picture before frame 0: `before`, else zeros).  Only non-zero counts are stored: the caller zeroes
// `out` first.  The run is split into `segs` (clamped to 1..n) contiguous segments along grid.y, each composing the picture before its
// own first frame; the counts do not depend on the split.
void msv1_launch_index_activity(const Msv1IndexSrc& src, int first, int n, int segs, uint16_t* out, int cols, int rows, hipStream_t stream);
// ONE launch of msv1_index_distance_kernel (msv1_index_distance_kernels.hip): out[(k * rows + r) * cols + q], k < n, = the pixels of
// the 16x16 cell (r, q), inside whole 4x4 blocks, that differ between the picture of index frame first + k and the reference R — the
// picture of index frame ref_frame (-1: `before`, else zeros) when ref_picture is null, else the device picture ref_picture of X * Y
// words (4-byte aligned, only read; ref_frame is not looked at).  EVERY element is stored: the caller zeroes nothing.  Segments as for
// msv1_launch_index_activity; the counts do not depend on the split.
void msv1_launch_index_distance(const Msv1IndexSrc& src, int ref_frame, const int32_t* ref_picture, int first, int n, int segs, uint16_t* out,
                                int cols, int rows, hipStream_t stream);
// The device scratch of jsp_index_key_frame (the index owns it; every part 16-byte aligned).
struct Msv1KeyFrameScratch {
    uint32_t* status;                // [0]: all ones, else the first block that cannot be cut (block << 1 | kind); [1]: the frame's length
    uint32_t* totals;                // per workgroup of MSV1_KEYFRAME_WG_BLOCKS blocks: the bytes of its codes
    uint32_t* records;               // per block: writer frame, (offset within its workgroup's bytes << 8 | code length, 0 with a status)
    uint8_t* out;                    // the key frame, room for its bound (18 / 10 bytes a block)
};
constexpr int MSV1_KEYFRAME_WG_BLOCKS = 1024;      // consecutive blocks a workgroup of the two kernels owns
constexpr uint32_t MSV1_KEYFRAME_NO_WRITER = 0u;   // kinds of status: no frame <= t of the index codes the block ...
constexpr uint32_t MSV1_KEYFRAME_CUT = 1u;         // ... the end of its last writer's data cuts the code off
inline int msv1_keyframe_workgroups(int nblocks) { return (nblocks + MSV1_KEYFRAME_WG_BLOCKS - 1) / MSV1_KEYFRAME_WG_BLOCKS; }
// TWO launches (msv1_index_keyframe_kernels.hip, which states the rule): msv1_index_keyframe_sizes_kernel, then
// msv1_index_keyframe_gather_kernel — the codes of the last writers <= t of all blocks, in block order, into k.out, the length into
// k.status[1]; k.status[0] (all ones from the caller) names the first block without a writer or with a code cut off, and k.out is
// then not a key frame.  Nothing for an index without a block.
void msv1_launch_index_keyframe(const Msv1IndexSrc& src, int t, const Msv1KeyFrameScratch& k, hipStream_t stream);

// The device scratch of the clip calls — jsp_index_delta_frames / _tight_frames / _crop_frames / _path_frames / _pan_frames — for one
// slice of pairs (the index owns it; every part 16-byte aligned: clip_layout, msv1_index_clip_layout.h).  A frame has nb blocks in
// j-numbering — the whole grid, or a rectangle — and nwg = msv1_keyframe_workgroups(nb) workgroups of MSV1_KEYFRAME_WG_BLOCKS blocks.
// The bodies of the kernels that write and read it stand once, in msv1_index_clip_device.h.
struct Msv1ClipScratch {
    const int32_t* origins;          // pan only, else null.  Per pair: x, y of the rectangle at `from` (a key pair: not read), x, y at `to`
    const int32_t* pairs;            // per pair: from (-1: before the range; MSV1_CROP_KEY: a key pair), to.  Pan: a moved pair of a
                                     // call without the tight flag stands there as the key pair (to)
    const uint64_t* bases;           // per pair: where its frame starts in `out` (even; read by the gather only)
    uint32_t* status;                // per pair: all ones, else the first block of the frame that refuses (j << 1 | kind,
                                     // MSV1_KEYFRAME_NO_WRITER or MSV1_KEYFRAME_CUT)
    uint32_t* totals;                // per pair and workgroup (pair * nwg + g): the bytes of its codes and skip words
    uint32_t* first_written;         // per pair and workgroup: its first coded block j, MSV1_DELTA_NONE when it has none
    uint32_t* counts;                // per pair and workgroup: the blocks that got a code.  Delta and tight: null, nobody asks
    uint32_t* records;               // per pair and block ((pair * nb + j) * 2): writer frame, (offset within its workgroup's bytes
                                     // << 8 | L); L = code length, MSV1_DELTA_SKIP for a run head, 0 for nothing (or a status)
    uint8_t* out;                    // the slice's frames back to back, room for npairs * the bound
};
constexpr uint32_t MSV1_DELTA_NONE = 0xFFFFFFFFu;
constexpr uint32_t MSV1_DELTA_SKIP = 1u;           // (odd: no code has this length)
constexpr int MSV1_DELTA_RUN = 1023;               // a skip word's count is 10 bits: no skip word crosses a multiple of this
constexpr int MSV1_CROP_KEY = -2;                  // a pair's `from` that says "key pair" (JSP_CROP_KEY)
// A block rectangle of the picture, in table order (block row 0 = stored rows 0 .. 3), checked against the block grid by the host
// (crop_rect_ok, msv1_index_crop_layout.h): bw, bh >= 1, bx + bw <= nbx, by + bh <= nby; nb = bw * bh.  Block j < nb of the
// rectangle is source block (by + j / bw) * nbx + bx + j % bw.
struct Msv1CropRect {
    int bx, by, bw, bh, nb;
};
// ONE launch each, grid.y = the pair; the .hip file of a call states its rule.  Sizes: status (all ones from the caller), totals,
// first_written, records and (not delta) counts of npairs pairs.  Gather, after a sizes launch over the same pairs with no status
// raised and with bases[] = the running sums of the pairs' lengths: the frames into d.out.  Nothing for a frame without a block.
// Delta (msv1_index_delta_kernels.hip): the whole grid, gap pairs only.  tight (jsp_index_tight_frames): the sizes launch decodes both
// ends of the gap of every written block and keeps the block only where a pixel changed.
void msv1_launch_index_delta_sizes(const Msv1IndexSrc& src, int npairs, const Msv1ClipScratch& d, bool tight, hipStream_t stream);
void msv1_launch_index_delta_gather(const Msv1IndexSrc& src, int npairs, const Msv1ClipScratch& d, hipStream_t stream);
// Crop (msv1_index_crop_kernels.hip): the rectangle r, key and gap pairs.  tight: THE TIGHT RULE for the gap pairs.
void msv1_launch_index_crop_sizes(const Msv1IndexSrc& src, const Msv1CropRect& r, int npairs, const Msv1ClipScratch& d, bool tight,
                                  hipStream_t stream);
void msv1_launch_index_crop_gather(const Msv1IndexSrc& src, const Msv1CropRect& r, int npairs, const Msv1ClipScratch& d, hipStream_t stream);
// Path (msv1_index_path_kernels.hip): crop's with pairs in either direction — d.pairs may hold from > to (a step back) and from == to
// (a hold), checked by the host (path_pair_ok, msv1_index_path_layout.h).  msv1_launch_index_crop_gather gathers.
void msv1_launch_index_path_sizes(const Msv1IndexSrc& src, const Msv1CropRect& r, int npairs, const Msv1ClipScratch& d, bool tight,
                                  hipStream_t stream);
// Pan (msv1_index_pan_kernels.hip): a rectangle of bw x bh blocks whose origins stand per pair in d.origins, checked against the block
// grid by the host (pan_pair_check, msv1_index_pan_layout.h).  tight: THE TIGHT RULE for still gap pairs, the two-block compare for
// moved ones.
void msv1_launch_index_pan_sizes(const Msv1IndexSrc& src, int bw, int bh, int npairs, const Msv1ClipScratch& d, bool tight, hipStream_t stream);
void msv1_launch_index_pan_gather(const Msv1IndexSrc& src, int bw, int bh, int npairs, const Msv1ClipScratch& d, hipStream_t stream);

}  // namespace jsp
