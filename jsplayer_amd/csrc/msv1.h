// MSVideo1 (CRAM) path: host parse -> per-block descriptor table -> HIP block reconstruction.
// Reference behaviour: MSVideo1.hx (see include/jsplayer_amd.h for the per-call citations).
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include <hip/hip_runtime.h>

namespace jsp {

// Descriptor = one uint32 per 4x4 block, raster order over the (bottom-up) buffer:
// byte offset of the block's code word inside the batch's stream buffer, or one of:
constexpr uint32_t MSV1_DESC_SKIP = 0xFFFFFFFFu;       // copy the block from the previous frame
constexpr uint32_t MSV1_DESC_UNTOUCHED = 0xFFFFFFFEu;  // leave dst as it is (end marker / abort)

// Per-frame launch record, read by every workgroup of that frame (grid.y = frame).
struct Msv1FrameArgs {
    int32_t* dst;
    const int32_t* prev;   // may be null when no block is a skip and no compare is requested
    uint32_t* signif;      // device word OR-ed with 1 when a compared pixel differs
    uint32_t stream_end;   // absolute offset one past this frame's last stream byte
    uint32_t desc_base;    // index of this frame's first descriptor
    uint32_t cmp_row_lo;   // first pixel row taking part in the stage-2 compare; ~0u = none
    uint32_t pad;          // flags: MSV1_FRAME_USES_PREV
};

constexpr uint32_t MSV1_FRAME_USES_PREV = 1u;  // some block copies from / compares with the previous frame
constexpr uint32_t MSV1_FRAME_NOOP = 2u;       // early-out frame: no block is written

struct Msv1Geometry {
    int bits;  // 16 or 8
    int X, Y;
    int nbx, nby;
    int nblocks;
};

struct Msv1Parse {
    bool early_out = false;   // 16-bit only: empty / all-skip short stream -> prevFrame untouched
    bool changes = false;     // at least one coded block (dst gets adopted)
    bool s1 = false;          // stage-1 significance (coded block in a significant block row)
    bool aborted = false;     // skip block with no previous frame: the reference raises
    uint64_t n_coded = 0, n_skipped = 0, n_untouched = 0;
    uint64_t consumed = 0;    // stream bytes walked over
};

// Host parse (sequential: code lengths are data dependent, MSVideo1.hx:128-181,311-364).
// Writes geo.nblocks descriptors.  `base` is added to every offset (position of this frame's
// bytes in the batch stream buffer).  `block_changes` is the codec's persistent per-row state.
void msv1_parse(const Msv1Geometry& geo, const uint8_t* src, size_t n, bool have_prev,
                size_t size_of_just_skips, int insignificant_blocks, uint32_t base,
                uint32_t* desc, std::vector<uint8_t>& block_changes, Msv1Parse& out);

bool msv1_just_skip_blocks(const Msv1Geometry& geo, const uint8_t* src, size_t n);
int msv1_is_key_frame(const Msv1Geometry& geo, const uint8_t* src, size_t n);

// ---- on-GPU parse (msv1_parse_kernels.hip) ----------------------------------------------------
struct Msv1ParseFrame {   // one per frame of a batch
    uint32_t beg, end;        // byte range of the frame in the batch stream buffer (beg 16-byte aligned)
    uint32_t desc_base;       // index of the frame's first descriptor
    uint32_t first_tile, ntiles;
    uint32_t host_parsed;     // 1: descriptors come from the host parser, the GPU parse skips the frame
    uint32_t pad0, pad1;
};
constexpr uint32_t MSV1_INFO_END_MARKER = 1u;  // an 8-bit end-of-data marker sits on the code chain
constexpr uint32_t MSV1_INFO_S1 = 2u;          // a coded block lies in a significant block row
struct Msv1FrameInfo {    // counters the parse kernels return per frame
    uint32_t n_coded;         // coded (non-skip) blocks
    uint32_t n_skip_codes;
    uint32_t total_blocks;    // blocks covered by the whole stream (saturating); < nblocks = stream too short
    uint32_t flags;
    uint32_t consumed;        // bytes up to the end of the code covering the last block
    uint32_t pad[3];
};
uint32_t msv1_parse_tile_bytes();    // 16 KiB: staged batches (frames start on tile boundaries of the stream buffer)
uint32_t msv1_small_tile_bytes();    // 8 KiB: `small_tiles` launches (one frame per launch: the scout, decode and group launchers below)
void msv1_launch_parse(const Msv1Geometry& geo, const uint8_t* d_stream, const Msv1ParseFrame* d_frames, int nframes,
                       const uint32_t* d_tile_frame, int ntiles, int max_tiles_per_frame, uint32_t* d_tile_tab,
                       uint32_t* d_tile_entry, uint32_t* d_tile_block0, uint32_t* d_desc, Msv1FrameInfo* d_info,
                       int insignificant_blocks, hipStream_t stream);

// Fused parse + reconstruction (msv1_fused_kernel): everything one 16 KiB tile of a frame's stream needs, in one
// 64-byte record the workgroup reads with a single scalar load.
constexpr uint32_t MSV1_TILE_SKIP = 1u;   // the frame takes the descriptor path (host-parsed)
struct alignas(16) Msv1TileRec {
    uint32_t byte0;        // first byte of the tile in the batch stream buffer
    uint32_t frame_end;    // end of the frame's whole code units (even)
    uint32_t data_end;     // end of the bytes a code may read: frame_end (16-bit) or the frame's true end (8-bit)
    uint32_t k;            // index of the tile within its frame
    uint32_t first_tile;   // index of the frame's first tile within the batch
    uint32_t ntiles;       // tiles of the frame
    uint32_t cmp_row_lo;   // first pixel row of the stage-2 compare; ~0u = none
    uint32_t flags;        // MSV1_TILE_SKIP
    int32_t* dst;
    const int32_t* prev;
    uint32_t* signif;
    uint64_t pad;
};
static_assert(sizeof(Msv1TileRec) == 64, "one record = 64 bytes");
// msv1_fused_kernel is launched in four forms, each with a launcher of its own below: the batch form writing pixels or block tables, the
// scout + decode pair and the one-launch form of the asynchronous per-frame path.  In all of them the tiles publish where the code chain stands
// in `agg`: 9 words per tile, zeroed once; `epoch` (> 0) must differ from launch to launch on the same `agg`.
constexpr size_t MSV1_AGG_PUBLISHED = 9;
// A staged batch's `agg` has room behind the published words of all its tiles for 8 counters per tile, and its fault word (two words) for 64 bytes
// more: only a lab build's phase clocks use either (tools/lab/hooks_clocks/msv1_fused_hooks.h).
constexpr size_t MSV1_AGG_LAB_CLOCKS = 8;
constexpr size_t MSV1_SYNC_BYTES = 2 * sizeof(uint32_t) + 64;

// ---- the batch forms: tiles [tile0, tile0 + ntiles) of a staged batch in one launch, one record per tile ----
// *fault becomes non-zero if a tile gave up waiting for the tiles before it (the caller reports the batch as failed).
struct Msv1FusedBatch {
    const uint8_t* stream = nullptr;     // the batch's stream buffer
    const Msv1TileRec* recs = nullptr;   // device records, in launch order
    const int32_t* palette = nullptr;
    unsigned long long* agg = nullptr;   // published tile words
    uint32_t epoch = 0;
    uint32_t tile0 = 0;
    int ntiles = 0;
    uint32_t* fault = nullptr;
    uint32_t agg_tiles = 0;              // tiles `agg` was sized for.  Only a lab build reads it: its phase clocks keep their counters behind that
                                         // many tiles' published words
};
// Pixels straight from the stream bytes, no descriptor table (kernel mode 0): 16 KiB tiles, frames laid out on 16 KiB boundaries.
void msv1_launch_fused_pixels(const Msv1Geometry& geo, const Msv1FusedBatch& batch, hipStream_t stream);
// Nothing is rebuilt (kernel mode 4): every tile writes its blocks' entries of the frame's descriptor table (the record's `dst` points at it) —
// the on-GPU descriptor parse in ONE launch, for the batches whose frames depend on each other.  8 KiB tiles: the records say where each begins.
void msv1_launch_fused_tables(const Msv1Geometry& geo, const Msv1FusedBatch& batch, hipStream_t stream);

// ---- the asynchronous per-frame path: what a frame's launches report ----
constexpr uint32_t MSV1_ASYNC_SHORT = 1u;     // the stream does not cover every block: the host parser has to settle it
constexpr uint32_t MSV1_ASYNC_S1 = 2u;        // a coded block lies in a significant block row (MSVideo1.hx:187-194)
constexpr uint32_t MSV1_ASYNC_END = 4u;       // an 8-bit end-of-data marker sits on the code chain
constexpr uint32_t MSV1_ASYNC_SKIPCODE = 8u;  // a skip code sits on the code chain
constexpr uint32_t MSV1_ASYNC_STUCK = 16u;    // one-launch form: the frame's tiles did not all report in time (the GPU is shared with something that
                                              // keeps them from being resident together): the host path settles the frame
struct Msv1AsyncInfo {
    uint32_t flags;
    uint32_t signif;   // stage-2 significance word (OR-ed with 1 when a compared pixel differs)
    uint32_t fault;    // look-back gave up
    uint32_t arrived;  // one-launch form: workgroups whose findings are in `flags` / that have written their last pixel; both run
    uint32_t finished; //         on from launch to launch (see `want`)
    uint32_t verdict;  // one-launch form: 0 undecided, MSV1_VERDICT_GO / _VETO — set ONCE per launch (compare-and-swap), obeyed by every tile
    uint32_t pad[2];
};
constexpr uint32_t MSV1_VERDICT_GO = 1u, MSV1_VERDICT_VETO = 2u;
constexpr uint32_t MSV1_LAB_DEAF = 0x80000000u;   // in `bad_mask` (tests): one-launch tiles never see all reports in — the verdict is the time-out's
// One-frame launches of a small frame (an inter frame, an 8-bit frame: a few hundred KB) use 8 KiB tiles — `small_tiles` —: twice the
// workgroups, half the serial work in each; the kernel's time is a chain of dependent steps per tile, and such a launch has the
// GPU to itself.  (1080p inter frames with 70 % skipped blocks: 28.8 -> 37.9 Gpixels/s on one stream, 8-bit key frames 42.4 -> 52.8;
// frames of a megabyte gain nothing on one stream and lose a fifth on sixteen: they keep 16 KiB tiles — with their uploads gone, jsp_prefetch,
// they lose an eighth on one stream as well: profiles/r04_msv1_small_tiles_e2e.txt.)
constexpr size_t MSV1_SMALL_TILE_FRAME_BYTES = 640 * 1024;

// What a frame's launches have in common with those of the frames around it:
struct Msv1AsyncShared {
    const int32_t* palette = nullptr;
    int insignificant_blocks = 0;
    uint32_t* poison = nullptr;          // one word per codec instance: set by a vetoed decode, it vetoes every later one until the host clears it
    bool small_tiles = false;
};

// ---- scout + decode (kernel modes 1, 2): one frame in two launches, one record per tile ----
// The scout pass reports what the descriptor path's parse would have told the host (info->flags), then the decode pass, which does nothing when
// info->flags & bad_mask; the frame's significance word is info->signif, its fault word info->fault.
struct Msv1FusedPass {
    const uint8_t* stream = nullptr;
    const Msv1TileRec* recs = nullptr;
    unsigned long long* agg = nullptr;
    uint32_t epoch = 0;                  // (a new one for each of the two passes)
    int ntiles = 0;
    Msv1AsyncInfo* info = nullptr;       // the report, in device memory
    uint32_t bad_mask = 0;
    Msv1AsyncShared shared;
};
void msv1_launch_fused_scout(const Msv1Geometry& geo, const Msv1FusedPass& pass, hipStream_t stream);
void msv1_launch_fused_decode(const Msv1Geometry& geo, const Msv1FusedPass& pass, hipStream_t stream);

// ---- one launch per group of frames (kernel mode 3; each frame at most MSV1_MERGED_MAX_TILES tiles) ----
// Scout and decode in ONE launch — every tile parses and reports, waits until all of its frame's reports are in (`want` = the value of
// info->arrived / finished once this launch is through), and only then writes, or does not.  All tiles of a frame share `rec` (k = the tile's
// index, rec.ntiles = the frame's tiles); the last workgroup copies flags / signif / fault to `host_info` (pinned host memory) and clears them in
// `info`.  `stream` may be pinned HOST memory (any alignment, nothing read past the frame's last byte): each tile reads its bytes once, over the
// bus, and leaves a copy in `keep` (HBM, the frame's size rounded up to 16 bytes; null: none is kept).
constexpr int MSV1_MERGED_MAX_TILES = 128;
// SEVERAL frames in one launch: the frames submitted right behind the first one (up to 3) ride along — workgroups
// [0, f[0].first_wg) are the first frame's tiles, [f[i].first_wg, f[i].first_wg + f[i].rec.ntiles) those of rider i.  All frames load, parse
// and reach their verdicts side by side (none of that touches a pixel); a rider's tiles then wait until every tile of the frame in front
// has finished (that frame's `finished` has reached its `want`) before they write — a frame may copy from the pixels of the one before it
// and be compared with them — and leave their frame unwritten when the one in front was vetoed.  One launch and one kernel-to-kernel gap
// per group, and every frame's parse hidden behind the painting of the frames before it: what bounds ONE player stream is the chain of
// its frames' kernels.  count = 0: one frame, as ever.
struct Msv1Rider {
    const uint8_t* stream = nullptr;
    unsigned long long* agg = nullptr;
    Msv1AsyncInfo* info = nullptr;
    Msv1AsyncInfo* host_info = nullptr;
    uint8_t* keep = nullptr;
    Msv1TileRec rec{};
    uint32_t epoch = 0, bad_mask = 0, want = 0, first_wg = 0;
};
constexpr int MSV1_MAX_RIDERS = 3;
struct Msv1Riders {
    uint32_t count = 0, pad = 0;
    Msv1Rider f[MSV1_MAX_RIDERS];
};
// A frame of such a launch as its caller describes it: the first one like those behind it (`first_wg` is the launcher's to fill in).
using Msv1GroupFrame = Msv1Rider;
// frames[0 .. nframes), 1 <= nframes <= 1 + MSV1_MAX_RIDERS, in the order they were submitted.
void msv1_launch_fused_group(const Msv1Geometry& geo, const Msv1GroupFrame* frames, int nframes, const Msv1AsyncShared& shared, hipStream_t stream);

// Kernel launchers (msv1_kernels.hip).  All asynchronous on `stream`.
void msv1_launch_blocks(const Msv1Geometry& geo, const uint8_t* d_stream, const uint32_t* d_desc,
                        const Msv1FrameArgs* d_frames, int nframes, const int32_t* d_palette,
                        bool vec_ok, hipStream_t stream);
// Inter-frame group in one launch: workgroup = spatial tile, frames walked in registers (needs X%4==0,
// 16-byte aligned buffers, and frames that write all of their blocks or none).
void msv1_launch_blocks_temporal(const Msv1Geometry& geo, const uint8_t* d_stream, const uint32_t* d_desc,
                                 const Msv1FrameArgs* d_frames, int nframes, const int32_t* d_palette,
                                 hipStream_t stream);
// Stage-2 compare over the pixels no block covers (X&3 / Y&3 remainders), MSVideo1.hx:197-203.
void msv1_launch_edge_compare(const Msv1Geometry& geo, const Msv1FrameArgs* d_frames, int nframes,
                              hipStream_t stream);

}  // namespace jsp
