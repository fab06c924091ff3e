/*
 * jsplayer_amd — MI355X-native block-video decode path behind jsplayer's IVideoCodec.
 *
 * C ABI (plain pointers and sizes, no C++/torch types).  Every entry point cites the
 * reference interface it replaces; paths are relative to /root/reference/src.
 *
 * Frame buffers follow the reference's contract (MSVideo1.hx:211-214, ScreenPressor.hx:189,
 * Manager.hx:114-118,379): one int32 per pixel, value 0x00RRGGBB, stride = width ints,
 * BOTTOM-UP rows, length >= width*height ints, allocated and owned by the CALLER.  The codec
 * borrows `dst` and keeps it as its "previous frame" until a later frame replaces it; the caller
 * never passes the current previous frame as `dst` (Manager.hx:424-443,477).
 *
 * `dst` may be either
 *   - a DEVICE pointer (HBM; e.g. from jsp_pool_create): the frame stays on the GPU, or
 *   - a HOST pointer: the codec decodes into an internal HBM frame and copies the result back
 *     (compatibility mode for an unmodified Manager; PCIe-bound).
 * The two kinds must not be mixed on one codec instance.
 *
 * Ordering: a codec's own HIP stream is a blocking stream, i.e. ordered after work the caller queued on the legacy
 * default stream; work the caller has pending on other non-blocking streams that touches `dst` or the previous
 * frame must have finished before the call (or give the codec that stream with jsp_set_stream).
 *
 * Threading (reference: single-threaded, not re-entrant): one thread per codec instance at a
 * time; distinct instances may be used concurrently from distinct threads.
 * No exceptions cross this boundary; failures are reported by status + jsp_last_error().
 */
#ifndef JSPLAYER_AMD_H
#define JSPLAYER_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct jsp_codec jsp_codec;
typedef struct jsp_pool jsp_pool;
typedef struct jsp_staged jsp_staged;

/* Codec kinds = the three classes Manager.video_info_cb constructs (Manager.hx:105-110). */
enum {
    JSP_CODEC_MSVIDEO1_16 = 1,   /* new MSVideo1_16bit(w,h)            MSVideo1.hx:20-31   */
    JSP_CODEC_MSVIDEO1_8 = 2,    /* new MSVideo1_8bit(w,h,palette)     MSVideo1.hx:267-274 */
    JSP_CODEC_SCREENPRESSOR = 3  /* new ScreenPressor(w,h,bpp)         ScreenPressor.hx:53-64 */
};

/* enum DecoderState (IVideoCodec.hx:5-9) */
enum { JSP_ZERO_STATE = 0, JSP_IN_PROGRESS = 1, JSP_ERROR_OCCURED = 2 };

/* ---- IVideoCodec (IVideoCodec.hx:16-29) ------------------------------------------------- */

/* Constructors (Manager.hx:105-110).  `palette` = the strf bytes after the 40-byte
 * BITMAPINFOHEADER (AVIParser.hx:79-85), used by JSP_CODEC_MSVIDEO1_8 only; `bpp` is used by
 * JSP_CODEC_SCREENPRESSOR only.  `device_id` = HIP device ordinal.  NULL on failure. */
jsp_codec* jsp_codec_create(int kind, int width, int height, int bpp,
                            const uint8_t* palette, int palette_bytes, int device_id);

/* StopAndClean() (IVideoCodec.hx:28; MSVideo1.hx:33-35; ScreenPressor.hx:81-84) + release. */
void jsp_codec_destroy(jsp_codec* c);

/* Preinit(insignificant_lines) (IVideoCodec.hx:18; MSVideo1.hx:37-41,281-291;
 * ScreenPressor.hx:86-89).  Called once by Manager with 36 (Manager.hx:61,128). */
int jsp_preinit(jsp_codec* c, int insignificant_lines);

/* PreviousFrame() (IVideoCodec.hx:20): the caller-owned buffer last adopted, or NULL.
 * Compared BY IDENTITY by the caller (Manager.hx:470-475). */
int32_t* jsp_previous_frame(jsp_codec* c);

/* IsKeyFrame(data) (IVideoCodec.hx:21; MSVideo1.hx:226-259,395-427; ScreenPressor.hx:96-101).
 * Pure host-side scan; returns 0/1. */
int jsp_is_key_frame(jsp_codec* c, const uint8_t* src, size_t n);

/* State() / ContinueI() (IVideoCodec.hx:22,25).  The reference never reports in_progress
 * (resumable I-decode is disabled, ScreenPressor.hx:210-215,277-285); both return zero_state. */
int jsp_state(jsp_codec* c);
int jsp_continue_i(jsp_codec* c);

/* DecompressI(src,dst):DecoderState (IVideoCodec.hx:24; MSVideo1.hx:62-67;
 * ScreenPressor.hx:117-295).  Returns JSP_ZERO_STATE or JSP_ERROR_OCCURED. */
int jsp_decompress_i(jsp_codec* c, const uint8_t* src, size_t n, int32_t* dst);

/* DecompressP(src,dst):PFrameResult (IVideoCodec.hx:26; MSVideo1.hx:106-209,293-393;
 * ScreenPressor.hx:302-484).  *data_pnt = the old previous frame ("no change", dst not adopted)
 * or dst; *significant_changes = 0/1.  Returns JSP_ZERO_STATE, or JSP_ERROR_OCCURED where the
 * reference would raise (e.g. an MSVideo1 skip code before any frame was decoded). */
int jsp_decompress_p(jsp_codec* c, const uint8_t* src, size_t n, int32_t* dst,
                     int32_t** data_pnt, int* significant_changes);

/* NeedsIndex() (IVideoCodec.hx:27; MSVideo1.hx:221-224 -> 1; ScreenPressor.hx:486-489 -> 0). */
int jsp_needs_index(jsp_codec* c);

/* Thread-local description of the last failure on this thread ("" if none). */
const char* jsp_last_error(void);

/* ---- frame pool in HBM (Manager.hx:114-118: num_buffers+1 frame buffers) ---------------- */

/* A pool of 32 frames or more (what batch decoding writes into: tile j of every frame at about the same time, or every frame of a clip one after
 * the other from the same workgroups) is PLACED.  What the decode kernels' stores get from a pool depends on where its frames lie in physical memory,
 * relative to each other (no query reveals it), so the pool measures candidates with the kernels' store shape (a few milliseconds each)
 * against what a plain fill takes from the same device, and keeps the best:
 *   - first the MAPPED forms: one address range backed by physical allocations of the pool's own making (hipMemCreate / hipMemMap), in three
 *     arrangements — an allocation per frame; sixteen frames per allocation, dealt over them; sixteen per allocation, in order.  The first that comes
 *     within 3 % of the fill is kept; when none does, up to six more candidates of the first arrangement are made of other memory (for at most
 *     JSP_POOL_PROBE_MS milliseconds, default 250) and the best of all is kept.  The buffers are device pointers, but not hipMalloc allocations;
 *   - the bounds: at most JSP_POOL_PROBE_MAX candidates are measured (default 16), and what the probe holds while it chooses (the best so far and
 *     the rejects, so that the next candidate is made of other memory) stays within a quarter of the device memory that was free when it began, or
 *     JSP_POOL_PROBE_HOLD_GB (GB) if that is lower, never less than the pool itself (jsp_pool_probe_info);
 *   - the hipMalloc forms are tried only when no mapped form can be made (JSP_POOL_PROBE_MAPPED=0: as if none could), or after the mapped ones when
 *     JSP_POOL_PROBE_THOROUGH=1 and none of those came within 3 % of the fill: the older form that won the last probe of the process on this device
 *     (JSP_POOL_PROBE_FORM=0|1|2 names one: two frames per allocation, one allocation, one per frame); then chunks of 16 frames — a quarter of a run
 *     four times as long, the frames dealt round-robin over them, up to four choices of chunks —; then the older forms in turn, their frames taken
 *     in a strided order.
 * In the dealt, chunked and strided forms consecutive buffers of the pool are not neighbours in memory (unless the whole pool fits one physical allocation).  JSP_POOL_PROBE=0 in the environment: one
 * allocation per frame, first come — what smaller pools (a player's num_buffers + 1) always get.  JSP_POOL_PROBE_LOG: a line per candidate on stderr. */
jsp_pool* jsp_pool_create(int device_id, int width, int height, int nbuf);
int32_t* jsp_pool_buffer(jsp_pool* p, int i); /* device pointer, width*height ints, zeroed */
/* GB/s the chosen candidate took from the probe (0: a pool that is not probed); *attempts = candidates measured. */
double jsp_pool_store_rate(jsp_pool* p, int* attempts);
/* What placing the pool cost: wall time of the probe, the most device memory it held at one time (rejected candidates are kept until it
 * has chosen) and what it was allowed to hold (the bounds: jsp_pool_create above).  All 0 for a pool that is not probed.  Returns 0, -1 for a null pool. */
int jsp_pool_probe_info(jsp_pool* p, double* probe_ms, uint64_t* held_peak_bytes, uint64_t* hold_limit_bytes);
/* What every candidate the probe measured took (GB/s, in the order tried: the mapped candidates, then — when they are tried at all — the older
 * form hinted at, the chunked candidates, the older forms in turn): up to `cap` of them into `rates`; returns how many were measured (0 for a pool that is not probed, -1 for a null pool). */
int jsp_pool_probe_rates(jsp_pool* p, double* rates, int cap);
int jsp_pool_count(jsp_pool* p);
void jsp_pool_destroy(jsp_pool* p);
/* Copy one frame between a device frame buffer and host memory (parity checks, display). */
int jsp_download(const int32_t* device_frame, int32_t* host, size_t npixels);
int jsp_upload(int32_t* device_frame, const int32_t* host, size_t npixels);

/* ---- batched / resident-input entry points (extension; same semantics as the calls above) -- */

/* Run the codec's HIP work on `hip_stream` (a hipStream_t, e.g. torch's current stream) instead
 * of the codec's own stream.  NULL restores the codec's own stream. */
int jsp_set_stream(jsp_codec* c, void* hip_stream);
/* Codec options.  Returns 0 when accepted, -1 for an unknown key/value.
 *   "msv1_parse" = "gpu" (default) | "host" : MSVideo1 only.  "gpu" builds the per-block descriptor
 *       table with the on-GPU parse kernels (raw frame bytes are all the device needs; a replay of a
 *       staged batch re-runs the parse); frames the parse flags as special fall back to the host
 *       parser one by one, so results are identical either way.
 *   "msv1_parse_ahead" = "on" (default) | "off" : MSVideo1 only, replays of a staged batch of inter frames (jsp_staged_decode called again on the
 *       same batch).  Such a replay is a table-writing parse launch and the reconstruction launches that read the tables; "on" queues the NEXT
 *       replay's parse on a second stream of the codec, into a second set of tables, beside this replay's reconstruction (jsp_sync waits for both
 *       streams).  Costs a second table set (4 bytes per block and frame).  Results do not depend on it.
 *   ("sp_group_chunk" and "msv1_parse_pieces", launch plans of round 4 that measured slower and were removed in round 5, are still accepted and do
 *   nothing — results never depended on them; their environment twins JSP_SP_GROUP_CHUNK / JSP_MSV1_PARSE_PIECES are no longer read.)
 *   "sp_band_rows" = "auto" (default) | "0" | "<n>" : ScreenPressor only.  Key frames are rebuilt by one
 *       workgroup per band of n rows (0 = the whole frame is one band; auto = sized so a batch fills
 *       the GPU); the host stage hands each band the row above it.  Results do not depend on it.
 *   "sp_host_threads" = "auto" (default: up to 8) | "1".."64" : ScreenPressor only, jsp_stage_batch.  A coded key frame renews
 *       every bit of decoder state, so the frames from one coded key frame up to the next depend on nothing before them:
 *       the host entropy stage takes up to this many such groups of a batch side by side, a decoder and a host thread each
 *       (one-frame calls have nothing to split).  Results do not depend on it.
 *   "sp_inter_fusion" = "on" (default) | "off" : ScreenPressor only.  In a staged batch, consecutive inter
 *       frames are rebuilt by ONE launch (pixels carried in registers from frame to frame; the host stage
 *       hands motion rectangles over as literal pixels; a frame that moves more than a quarter of its
 *       pixels keeps its motion blocks and a launch of its own).  "off": one launch per frame.
 *   "sp_forget_buffers" = "1" : ScreenPressor only; nothing may be in flight.  CONTRACT behind it: an inter frame may read ONE pixel per row of
 *       its destination before writing it (ScreenPressor.hx:436-449: "left of column 0" is the last pixel of the row above, which this
 *       frame has not reached), so the codec remembers the last column of every picture it decoded into a buffer and asks the device for the
 *       column of a buffer it has never written — a synchronous copy, ordered after work on blocking streams only: the caller's own writes
 *       to that buffer must be complete.  A caller that writes into frame buffers itself BETWEEN decodes (jsp_upload, a clear, another codec
 *       sharing the pool, a buffer freed and allocated again at the same address) says so with this option and every buffer is asked for
 *       again; without such writes nothing needs to be said.  Buffers of a frame that failed are forgotten by the codec itself.
 *   "msv1_async_pairs" = "on" (default) | "off" : MSVideo1 with "msv1_parse" = "gpu", asynchronous calls, frames of up to 128 parse tiles.
 *       on: such a frame is not launched at once but HELD until half of "async_depth" frames (at most 4) have been submitted, and they go
 *       out in ONE launch: all of them load, parse and reach their verdicts side by side, each paints when the frame in front is through
 *       (it may copy from its pixels and be compared with them) and is left unpainted — for the host's re-run — when the frame in front
 *       was.  Whatever is held goes out at once when one of the held frames is waited for, or when anything else needs the stream
 *       (jsp_sync, a synchronous call, jsp_prefetch, jsp_set_stream).  One player stream is bound by the chain of its frames' kernels:
 *       64 -> 94 Gpixels/s at 1080p with 8 frames in flight.  jsp_counter(c, "paired_frames") counts the frames that shared a launch.
 *       Results do not depend on it. */
/*   "msv1_async" = "auto" (default) | "one_launch_dma" | "one_launch" | "two_launches" : MSVideo1 with "msv1_parse" = "gpu",
 *       asynchronous calls only; frames of up to 128 parse tiles (2 MiB).  auto: one_launch_dma while at most 3 codec instances
 *       of the process use this path, one_launch beyond (many streams: the copy queues are the bottleneck).  one_launch_dma: the copy engine brings the frame's bytes up on a
 *       stream of its own (next to the previous frame's kernel), ONE launch parses, waits until every tile of the frame
 *       has reported what the host parser would have found, and rebuilds the frame — or leaves `dst` untouched for the
 *       synchronous re-run.  one_launch: the same launch reads the bytes from the caller's pinned memory itself (no copy
 *       queued at all; the bus transfer then sits inside the kernel).  two_launches: a scout launch, then the decode
 *       launch it may veto (what larger frames always get).  Results do not depend on it. */
/*   "key_frame_compare" = "off" (default) | "<first row>" : any codec; nothing may be in flight.  With a first row set (Manager uses
 *       INSIGNIFICANT_LINES = 36), every key frame is also compared with the previous frame as the call found it — the pixel loop of
 *       frames_differ_significantly (Manager.hx:413-419: any dst[i] != prev[i], i >= row * width) — without a pass of the caller's
 *       own: ScreenPressor's host stage holds both pictures and answers itself (synchronous calls), otherwise the compare is queued on
 *       the codec's stream right behind the frame's kernels (no extra wait; the frame is still in the Infinity Cache).  The answer:
 *       jsp_key_frame_differs() after a synchronous DecompressI; *significant_changes of jsp_wait for an asynchronous one (a key
 *       frame that decoded and has no previous frame to be compared with counts as a change: Manager.hx:399-411; for a frame that FAILED
 *       *significant_changes stays what the decode reported and jsp_key_frame_differs() says -1).  Staged batches are not compared. */
/*   "msv1_seek_chunk_frames" = "auto" (default) | "1".."n" : MSVideo1 only, jsp_seek and jsp_find_change.  Frames staged and composed per chunk of a
 *       seek's range; auto: as many as keep the chunk's stream bytes and block tables under 1 GiB.  Results do not depend on it. */
/*   "msv1_index_play_segments" = "auto" (default) | "1".."64" : MSVideo1 only, jsp_index_play.  The run's destinations are split into this many
 *       contiguous segments along the launch grid (never more than frames in the run), each composing its own first frame; auto:
 *       enough segments for about 8 waves per SIMD.  Results do not depend on it. */
/*   "msv1_index_activity_segments" = "auto" (default) | "1".."64" : MSVideo1 only, jsp_index_activity.  The run's frames are split into this
 *       many contiguous segments along the launch grid (never more than frames in the run), each composing the picture before its own
 *       first frame; auto: as "msv1_index_play_segments".  Results do not depend on it. */
/*   "msv1_index_delta_slice" = "auto" (default) | "1".."4096" : MSVideo1 only, jsp_index_delta_frames.  The call's pairs run in slices of
 *       this many, which bounds the scratch the index owns (auto: as many pairs as 64 MiB of scratch hold, one at least).  Results do
 *       not depend on it. */
/*   "async_depth" = "1".."16" (default "4") : any codec.  Frames that may be in flight between jsp_decompress_*_async and
 *       jsp_wait. */
int jsp_set_option(jsp_codec* c, const char* key, const char* value);
/* Block until everything queued by this codec has finished (frames in flight on the asynchronous path stay to be
 * collected with jsp_wait). */
int jsp_sync(jsp_codec* c);
/* The last key frame decoded through jsp_decompress_i, or collected with jsp_wait, against the frame before it (option
 * "key_frame_compare"): 1 differs, 0 does not, -1 nothing to compare with (no previous frame, the frame failed, option off). */
int jsp_key_frame_differs(jsp_codec* c);
/* Diagnostics (no reference counterpart): how often this codec instance took one of its slow paths since it was created.
 *   "async_reruns"       frames of the asynchronous per-frame calls that were re-run through the synchronous path (the GPU
 *                        alone could not settle the stream — short streams, end markers, skip codes without a previous
 *                        frame — or the frame's tiles did not report in time);
 *   "lookback_fallbacks" staged MSVideo1 batches re-run through the descriptor kernels after a tile gave up waiting for
 *                        the tiles before it;
 *   "host_parsed_frames" (MSVideo1) frames staged with the on-GPU parse on ("msv1_parse" = "gpu") whose block table came
 *                        from the host parser all the same: the stream ends before every block is covered, an 8-bit end
 *                        marker or a skip code without a previous frame lies on the chain, or a 16-bit frame is short
 *                        enough for the all-skips early-out.  Every other frame is settled by the parse kernels alone;
 *   "sp_groups_held", "sp_spare_decoders"  (ScreenPressor) groups of pictures the asynchronous path keeps a record of, and
 *                        host decoders on its shelf: both stay bounded however long a stream runs without jsp_sync.
 *   "msv1_block_changes" (MSVideo1, for tests) not a count: the persistent per-row flags (MSVideo1.hx:122,305) of block
 *                        rows 0..61, row r in bit r — what the next DecompressP's significance starts from.
 * Unknown names and null arguments answer -1.  Results never depend on either path having been taken. */
long long jsp_counter(jsp_codec* c, const char* name);

/* ---- asynchronous per-frame calls: the `_async` variant SURVEY.md 8(b) allows for the one-call-per-tick surface
 * (Manager.hx:507,511) --------------------------------------------------------------------------------------------
 * jsp_decompress_i_async / jsp_decompress_p_async run the frame's HOST stage, queue its uploads and kernels and return
 * at once with a ticket; jsp_wait(ticket) blocks until that frame is complete and hands back exactly what the
 * synchronous call would have returned (DecoderState, *data_pnt, *significant_changes).  So the host stage of frame
 * n+1 (entropy decode, parse pre-scan, copy into pinned memory) overlaps the uploads and kernels of frame n.
 *   - device frame buffers only; tickets must be waited for in submission order, and a frame is complete when its ticket has been
 *     waited for.  The GPU work of DIFFERENT groups of pictures (ScreenPressor with worker threads: a coded key frame opens a
 *     group) is queued in the order their host stages finish, not in submission order — so the buffer a frame in flight is decoded
 *     AGAINST (the previous frame at its submission) must not be handed out as `dst` of a later frame until the frame reading it
 *     has been waited for, just like its own `dst` (examples/jsp_play and jsplayer_amd/player.py keep both out of circulation);
 *   - at most "async_depth" frames (jsp_set_option, default 4, 1..16) may be in flight: a further submission fails;
 *   - `src` must stay valid and unchanged, and `dst` untouched, until the frame's ticket has been waited for; if `src`
 *     lies in memory from jsp_host_alloc (pinned), it is uploaded from where it is, without a staging copy;
 *   - jsp_previous_frame() answers for the last SUBMITTED frame (adoption is decided by the host stage);
 *   - a frame the GPU cannot settle alone (MSVideo1: truncated stream, 8-bit end marker, skip code with nothing to
 *     copy from) is transparently re-run through the synchronous path inside jsp_wait, together with the frames
 *     submitted after it. */
int jsp_decompress_i_async(jsp_codec* c, const uint8_t* src, size_t n, int32_t* dst, uint64_t* ticket);
int jsp_decompress_p_async(jsp_codec* c, const uint8_t* src, size_t n, int32_t* dst, uint64_t* ticket);
int jsp_wait(jsp_codec* c, uint64_t ticket, int32_t** data_pnt, int* significant_changes);
/* Pinned host memory for compressed frames (what an AVI reader fills): uploads from it need no staging copy. */
void* jsp_host_alloc(size_t bytes);
void jsp_host_free(void* p);
/* The next frames' bytes lie in [host, host + bytes) (a stretch of the file the reader holds, chunk headers and all): the codec may
 * take the whole range to the device in ONE copy on a stream of its own, and asynchronous frames submitted afterwards whose `src`
 * lies inside it then queue no upload of their own (MSVideo1 with "msv1_parse" = "gpu"; everything else
 * accepts the call and does nothing).  No counterpart in the reference: its Manager hands the decoder slices of the one ArrayBuffer
 * the loader filled (DataLoader.hx), and this is that buffer crossing the bus in pieces sized for the bus instead of frame by frame
 * (a megabyte per copy goes at 24 - 39 GB/s here, 64 MB at 57).  Returns at once.  The codec keeps the 4 most recent ranges; a
 * range must stay unchanged in host memory while it is kept (frames are pre-scanned on the host from `src` itself); host == NULL,
 * bytes == 0 gives every range up (do so before the memory is reused for other bytes).  Results never depend on it.
 * jsp_counter(c, "prefetched_frames") counts the frames that found their bytes on the device. */
int jsp_prefetch(jsp_codec* c, const void* host, size_t bytes);

/* Equivalent to calling DecompressI on frames 0..n-1 in order (Manager.hx:507 in a loop); device
 * `dsts` only.  Key-frame-only MSVideo1 batches decode in ONE launch (grid.y = frame). */
int jsp_decompress_i_batch(jsp_codec* c, int nframes, const uint8_t* const* srcs,
                           const size_t* lens, int32_t* const* dsts);

/* Two-step form of the batch above, for measuring with inputs resident in HBM:
 *   jsp_stage_batch   host stage (parse / entropy -> descriptor tables) + H2D, untimed by callers;
 *   jsp_staged_decode queues the reconstruction kernels for the whole batch (asynchronous:
 *                     follow with jsp_sync or events on the stream given to jsp_set_stream);
 * `is_key[i]` selects DecompressI (non-zero) or DecompressP (zero) semantics for frame i
 * (NULL = all key frames).  Staging advances the codec's host-side state (entropy models,
 * previous-frame chain) exactly as the per-frame calls would; a staged batch may be decoded
 * any number of times into the same `dsts`. */
jsp_staged* jsp_stage_batch(jsp_codec* c, int nframes, const uint8_t* const* srcs,
                            const size_t* lens, const uint8_t* is_key, int32_t* const* dsts);
/* The same into an existing batch object, whose pinned and device buffers are taken over (a caller that stages batch after
 * batch: no allocation per batch).  Every decode of `reuse` must have finished (jsp_sync).  Returns the batch to use from
 * now on — `reuse` itself, or a new object when `reuse` was of a kind that cannot hold this batch (then it has been
 * destroyed) —, NULL on error (`reuse` stays valid). */
jsp_staged* jsp_restage_batch(jsp_codec* c, jsp_staged* reuse, int nframes, const uint8_t* const* srcs,
                              const size_t* lens, const uint8_t* is_key, int32_t* const* dsts);
int jsp_staged_decode(jsp_codec* c, jsp_staged* s);
void jsp_staged_destroy(jsp_staged* s);

/* Accounting for a staged batch (bench.py roofline): */
typedef struct jsp_staged_info {
    uint64_t frames;
    uint64_t pixels;           /* width*height*frames */
    uint64_t stream_bytes;     /* compressed bytes consumed (S in SURVEY.md 8d) */
    uint64_t descriptor_bytes; /* bytes of host-built tables resident in HBM */
    uint64_t units_coded;      /* MSVideo1: coded 4x4 blocks; ScreenPressor: data pixels */
    uint64_t units_copied;     /* MSVideo1: skipped blocks; ScreenPressor: pixels fetched from prev */
    uint64_t runs;             /* ScreenPressor run descriptors (R) */
    uint64_t algorithmic_bytes;/* SURVEY.md 8(d) formula for this batch */
    uint64_t kernel_launches;  /* launches jsp_staged_decode issues */
    double host_stage_ms;      /* wall time of the host parse / entropy stage */
    double h2d_ms;             /* wall time of the uploads */
    double device_parse_ms;    /* wall time of the on-GPU parse at staging (0 with the host parser) */
    uint64_t moved_bytes;      /* bytes the launch plan has to move through HBM at the least: every table and stream
                                  byte read once, every destination pixel written once, the previous frame read once
                                  per launch that carries pixels in registers from frame to frame.  Below
                                  algorithmic_bytes for those launches (the SURVEY.md formula charges a previous-frame
                                  read per frame), above it where host-built tables add bytes the formula leaves out. */
} jsp_staged_info;
int jsp_staged_get_info(const jsp_staged* s, jsp_staged_info* out);

/* Names of the kernels jsp_staged_decode launches for this batch, in launch order, each name once, separated by
 * " + " (what a rocprofv3 kernel trace of the decode shows).  Valid until the batch is destroyed. */
const char* jsp_staged_kernels(const jsp_staged* s);

/* Per-frame results of a staged batch: status[i] (DecoderState), adopted[i] (1 if dsts[i] became
 * the previous frame), significant[i] (valid after jsp_staged_decode + jsp_sync). */
int jsp_staged_results(jsp_staged* s, int* status, int* adopted, int* significant);

/* ---- seek: the seek branch of Manager.GetDecompressedFrame (Manager.hx:216-259) ---------------------------------------------
 * Seek: frames[0..nframes-1] are the frames from where the caller's stream stands (typically the nearest key frame,
 * DataLoader.hx:125-132) up to and including the target.  is_key as in jsp_stage_batch (NULL = all key frames).
 *   EQUIVALENCE  The call does what DecompressI / DecompressP do for each frame in order (is_key), WHEN EACH FRAME'S DESTINATION
 *       STARTS OUT HOLDING THE PICTURE BEFORE IT; nothing but `dst` is written.  For well-formed streams this is plain sequential
 *       decoding whatever the pool held.  It differs only where the reference leaves a block or pixel unwritten — blocks after an
 *       8-bit end marker or a truncated stream, the X % 4 / Y % 4 remainder pixels —: those show the previous picture, not stale pool
 *       content.  Pixels that no block covers are copied from the previous frame when there is one.  MSVideo1 has no motion, so
 *       block b of the target is block b as coded by the last frame of the range that coded it: the range is staged as one batch
 *       (either "msv1_parse") and ONE kernel launch writes `dst`.
 *   RESULTS  JSP_ZERO_STATE.  *data_pnt = dst if any frame of the range would have adopted its destination (jsp_previous_frame()
 *       is then dst); otherwise the unchanged previous frame (possibly NULL), and dst is not touched.  *significant_changes = what
 *       DecompressP of the LAST frame would report (stage 1, MSVideo1.hx:187-194 / 372-379, then the pixel compare against the
 *       picture before it from row insignificant_lines on, :195-205 / 380-390; 0 when the last frame is a key frame).  Host-side
 *       codec state — the persistent per-row block_changes included — ends as the sequential calls would leave it: the next
 *       DecompressP behaves exactly as after a sequential decode.
 *   ERRORS  Where the reference raises (a skip code with no previous picture): JSP_ERROR_OCCURED, jsp_last_error() names the
 *       frame's index in the range, jsp_previous_frame() becomes NULL, `dst` is unspecified.
 *   PRECONDITIONS  `dst` is a device buffer (a host pointer is an error); no asynchronous frame may be in flight; `dst` is not the
 *       current previous frame.  A violation is an error with nothing changed.
 *   The key-frame compare (option "key_frame_compare") does not run on a seek: jsp_key_frame_differs() answers -1 afterwards.
 *   ScreenPressor: JSP_ERROR_OCCURED ("seek: MSVideo1 only"), no state changed — its entropy stage is sequential and its inter
 *       frames carry motion; a caller decodes frame by frame there (jsplayer_amd/player.py Manager.seek).
 *   Ranges whose stream bytes and tables exceed a staging budget (1 GiB) are composed chunk by chunk (option
 *   "msv1_seek_chunk_frames"): after one chunk `dst` IS the picture before the next, so the result does not depend on the split. */
int jsp_seek(jsp_codec* c, int nframes, const uint8_t* const* srcs, const size_t* lens, const uint8_t* is_key,
             int32_t* dst, int32_t** data_pnt, int* significant_changes);

/* ---- skip stills: Manager.SkipStills (Manager.hx:289-317) over DataLoader.FindPossibleChange (DataLoader.hx:239-252) -------------
 * Find change: frames[0..nframes-1] run from where the caller's stream stands, as for jsp_seek (is_key likewise).  Frames before
 * `first` are decoded but not judged (the stretch from the decode position to the frame after the one shown); the candidates are
 * frames first..nframes-1.
 *   SIGNIFICANCE of candidate k = what the sequential Manager would record for it.  Inter frame: what DecompressP reports (stage 1;
 *       stage 2 from insignificant_lines on; stage 1 alone without a previous picture or, 16-bit, without Preinit; never for an
 *       8-bit frame that has a previous picture, since the 8-bit Preinit sets no line).  Key frame (frames_differ_significantly,
 *       Manager.hx:392-421): when the frame before is a key frame (k - 1 in the range; `key_before`, key_before_len bytes, for
 *       k == 0, NULL = not a key frame) its bytes differ; else when there is no picture before it 1; else the pixels from row
 *       `key_row` on differ between its picture and the picture before it (the Manager passes INSIGNIFICANT_LINES).  The Manager's
 *       rule for frame 0 of the clip stays with the caller.
 *   RESULTS  JSP_ZERO_STATE.  *found = the first significant candidate and *changed = 1; when there is none, *found = nframes - 1
 *       and *changed = 0 (FindPossibleChange lands on the last frame).  `dst` holds frame *found's picture, and *data_pnt is what
 *       jsp_seek defines for the range 0..*found.  significance[k] (NULL: not wanted; else nframes ints) = 0 / 1 for
 *       first <= k <= *found, -1 elsewhere.  Host-side codec state — previous frame, persistent per-row block_changes — ends as
 *       the sequential calls on frames 0..*found leave it; frames after *found leave no trace.
 *   EQUIVALENCE, ERRORS, PRECONDITIONS  as jsp_seek, for the frames up to *found (a frame the reference raises on is an error when
 *       no earlier candidate is significant; the error names its index in the range).  first outside 0..nframes-1, a null
 *       found / changed or a negative key_row: an error with nothing changed.  jsp_key_frame_differs() answers -1 afterwards.
 *   ScreenPressor: JSP_ERROR_OCCURED ("find_change: MSVideo1 only"), no state changed (jsplayer_amd/player.py Manager.skip_stills
 *       decodes frame by frame there).
 *   Per chunk of the range (option "msv1_seek_chunk_frames", the 1 GiB budget of jsp_seek): the chunk is staged, ONE launch
 *   compares every block a judged frame codes with what the block's previous writer left (msv1_change_scan_kernel, no picture
 *   written), then ONE launch composes `dst` up to the hit (a prefix of the chunk is staged again first, so that the host state
 *   ends at the hit) or the whole chunk; the chunks after a hit are not staged. */
int jsp_find_change(jsp_codec* c, int nframes, const uint8_t* const* srcs, const size_t* lens, const uint8_t* is_key, int first,
                    const uint8_t* key_before, size_t key_before_len, int key_row, int32_t* dst, int* found, int* changed,
                    int* significance, int32_t** data_pnt);

/* ---- seek index: scrubbing, previous frame, seek-bar clicks (Main.on_prevframe / Manager.PrevFrameTime, Manager.hx:184-208;
 * Main.on_click, Main.hx:1197-1215) over a range kept resident in HBM ------------------------------------------------------------
 * Build: frames[0..nframes-1] run from where the caller's stream stands, as for jsp_seek (is_key likewise).  The range is staged
 *   once (the codec's staging, either "msv1_parse", chunks under jsp_seek's 1 GiB budget / option "msv1_seek_chunk_frames") and its
 *   stream bytes, block tables and frame records stay in HBM, with a bitmap of which frame codes which block.  The codec's previous
 *   picture, if any, is COPIED into the index (the caller may reuse that buffer afterwards).  Every frame is judged as
 *   jsp_find_change judges its candidates (frame 0 with key_before = NULL; the Manager's rule for frame 0 of the clip stays with
 *   the caller).
 *   RESULTS  The index (jsp_index_destroy frees it), or NULL and jsp_last_error().  The codec's host state is left exactly as it
 *       was and no caller buffer is written.
 *   ERRORS  A frame the reference raises on (a skip code with no previous picture): NULL, the error names the frame's index in the
 *       range, nothing changed.  ScreenPressor: NULL ("index: MSVideo1 only"), nothing changed.  Otherwise the refusals of
 *       jsp_seek: an asynchronous frame in flight, a codec in host-pointer mode, a negative key_row.
 * Show: EQUIVALENCE  jsp_index_show(t) writes into `dst` exactly what jsp_seek(frames[0..t]) writes, called on the codec as it stood
 *       at the build: pixels, *data_pnt (dst when a frame 0..t adopts its destination, else the previous frame of the build's time)
 *       and *significant_changes.  ONE kernel launch, no staging, no upload: every block is decoded from the last frame <= t that
 *       coded it (bitmap words walked down from t / 32), else copied from the index's picture before the range (none: dst keeps
 *       it, as with jsp_seek).
 *   adopt = 0: the codec is not touched (thumbnails, a preview while scrubbing).  adopt = 1: the codec ends as that jsp_seek leaves
 *       it — previous frame, per-row block_changes (recorded per frame at the build: MSVideo1.hx:122,305 reset a row only when a
 *       frame reaches it), what the on-GPU parse needs — so a following DecompressP(t + 1) behaves as after sequential decoding.
 *       The codec keeps no pointer into the index.  jsp_key_frame_differs() answers -1 afterwards.
 *   PRECONDITIONS  `dst` is a device buffer and not the codec's current previous frame; no asynchronous frame in flight.
 *   ERRORS  t outside 0..nframes-1, an index built by another codec, ScreenPressor, a violated precondition: JSP_ERROR_OCCURED,
 *       nothing changed.
 * Significance: out[0..nframes-1] = 1 / 0, what jsp_find_change judges for each frame (inter frames: what DecompressP reports;
 *   key frames: frames_differ_significantly from key_row on) — loader.GetFrameChanges (Manager.hx:229) for every frame of the range.
 * Info: frames, and the bytes the index holds in HBM and in host memory (staging memory is released at the end of the build).
 * Destroy: frees the index's device (and pinned) memory only; safe before or after jsp_codec_destroy of its codec. */
typedef struct jsp_index jsp_index;
jsp_index* jsp_index_build(jsp_codec* c, int nframes, const uint8_t* const* srcs, const size_t* lens, const uint8_t* is_key, int key_row);
int jsp_index_show(jsp_codec* c, jsp_index* idx, int t, int32_t* dst, int adopt, int32_t** data_pnt, int* significant_changes);
int jsp_index_significance(const jsp_index* idx, int* out);
int jsp_index_info(const jsp_index* idx, int* nframes, uint64_t* device_bytes, uint64_t* host_bytes);
void jsp_index_destroy(jsp_index* idx);

/* ---- thumbnails of an index: the preview that follows the pointer along the seek bar (Main.on_mouse_move / the seek bar,
 * Main.hx:1147-1215), a filmstrip or contact sheet of a key interval, the landing candidates of "skip idle" ----------------------
 * Thumb size: for scale s = 4, 8 or 16, *width = (4 * (W / 4)) / s and *height = (4 * (H / 4)) / s: whole s x s squares of the
 *   picture's whole 4x4 blocks.  The W % 4 / H % 4 remainder pixels and, for s > 4, a trailing odd block column / row are left out.
 * Thumbs: EQUIVALENCE  thumbnail k is the picture of frame frames[k], reduced: pixel (x, y), per channel c of the 0x00RRGGBB words,
 *       = (sum of c over the s x s source pixels at (x s .. x s + s - 1, y s .. y s + s - 1) + s s / 2) >> log2(s s); top byte 0.
 *       The PICTURE of frame t is what jsp_index_show(t) writes into a destination that held zeros: every block from the last frame
 *       <= t that coded it, else from the index's copy of the picture before the range, else 0 (so a frame before the first one that
 *       adopts its destination, where Show writes nothing, shows the picture before the range).  Rows keep the frame's bottom-up
 *       order (thumbnail row 0 is frame rows 0 .. s - 1): jsp_display_convert with flip_rows applies to a thumbnail, or to a whole
 *       sheet, as it does to a frame.
 *   SHEET  `out` is one image of cols * width by ceil(n / cols) * height pixels, pitch cols * width; thumbnail k has its pixel
 *       (0, 0) at (k / cols) * height * pitch + (k % cols) * width.  cols = 1: a plain [n][height][width] array; cols = n: a
 *       horizontal strip.  The cells of the last sheet row past n are not written.  frames[] is any list of frames of the index:
 *       unordered, repeats allowed.
 *   ONE kernel launch whatever n (msv1_index_thumbs_kernel): per block and thumbnail a bitmap walk, a table entry and one code
 *       decoded and summed; no full-size picture is written anywhere.  Runs on the codec's stream and returns synchronised.  The
 *       codec's state, its previous frame and every frame buffer are untouched.  The frame list travels through pinned memory and a
 *       device array the index owns (grown on demand, counted in jsp_index_info).
 *   PRECONDITIONS  `out` is a device buffer of at least out_pixels ints; no asynchronous frame in flight.
 *   ERRORS  A null argument, n outside 1..4096, a frame number outside the index, a scale other than 4 / 8 / 16, a zero-sized
 *       thumbnail, cols < 1, out_pixels smaller than the sheet, an index built by another codec, ScreenPressor, a violated
 *       precondition: JSP_ERROR_OCCURED, jsp_last_error(), nothing written. */
int jsp_index_thumb_size(const jsp_index* idx, int scale, int* width, int* height);
int jsp_index_thumbs(jsp_codec* c, jsp_index* idx, int n, const int* frames, int scale, int cols, int32_t* out, size_t out_pixels);

/* ---- windows of an index: frames of a seek index straight into a window — the hover preview at the size the UI wants (a 320 x 180
 * preview of a 1080p clip is k = 1/6, none of the thumbnails' three scales), a scrub at 200 % with the view scrolled, a contact sheet
 * whose cells are what the page needs — without a full-size frame in between -------------------------------------------------------------
 * Present: THE PICTURE of frame t is the one jsp_index_thumbs reduces: what jsp_index_show(t) writes into a destination that held
 *       zeros — every block from the last frame <= t that coded it, else from the index's copy of the picture before the range, else 0;
 *       the X % 4 / Y % 4 remainder pixels no block covers from that picture, or 0.  Unlike Thumbs the WHOLE X x Y picture takes part,
 *       remainders included.
 *   EQUIVALENCE  cell i of the sheet holds exactly the win_w x win_h ints that
 *         jsp_display_present(P, X, Y, cell, win_w, win_h, out_pitch, k, dx, dy, mode, filter, background)        (filter 0 or 1)
 *         jsp_display_present_area(P, X, Y, cell, win_w, win_h, out_pitch, k, dx, dy, mode, background)           (filter JSP_PRESENT_AREA)
 *       write for P = the picture of frames[i]: THE RULE of jsp_display_present / jsp_display_present_area below — geometry, which
 *       pixels are picture, taps, weights, rounding and `background` — is not restated here.  All three filter values are taken.
 *       jsp_view_matrix supplies k, dx, dy as it does for those calls.
 *   SHEET  cell i has its pixel (0, 0) at (i / cols) * win_h * out_pitch + (i % cols) * win_w; out_pitch >= cols * win_w.  The sheet
 *       occupies (ceil(n / cols) * win_h - 1) * out_pitch + cols * win_w ints and out_ints must be at least that.  Only cell pixels
 *       are written: pitch padding, the cells of the last sheet row past n and memory behind the sheet are not.  frames[] is any list
 *       of frames of the index: unordered, repeats allowed.  n = 1, cols = 1 is the plain window.  `out` needs no alignment (cell rows
 *       that all start on 16-byte boundaries get 16-byte stores).
 *   ONE kernel launch whatever n (msv1_index_present_kernel): a workgroup composes the source pixels one rectangle of a cell reaches
 *       into a 64 x 64 tile of on-chip memory and resamples from there, tile by tile where the rectangle reaches further; no full-size
 *       picture is written anywhere and no frame buffer is touched.  Runs on the codec's stream and returns synchronised.  THE CODEC
 *       IS ONLY LENT, as for Thumbs: its state, previous frame and per-row flags stay as they were.  The frame list travels through
 *       pinned memory into the device array of jsp_index_thumbs (grown on demand, counted in jsp_index_info); the index grows by
 *       nothing the size of a picture.
 *   BOUNDS  n 1..4096; win_w, win_h 1..16384; 1/64 <= k <= 64; mode one of the four JSP_DISPLAY_*; filter 0, 1 or 2; cols >= 1.
 *   PRECONDITIONS  `out` is a device buffer of at least out_ints ints; no asynchronous frame in flight.
 *   ERRORS  A null argument, a ScreenPressor codec ("index: MSVideo1 only"), an index built by another codec, n, a size, k, mode,
 *       filter or cols outside its bounds, a non-finite k, dx or dy, a frame number outside the index, out_pitch < cols * win_w,
 *       out_ints below the sheet, a host-pointer `out`, an asynchronous frame in flight: JSP_ERROR_OCCURED, jsp_last_error()
 *       ("index_present:" ...), before anything is queued: nothing changed, nothing written. */
int jsp_index_present(jsp_codec* c, jsp_index* idx, int n, const int* frames,
                      int32_t* out, size_t out_ints, int win_w, int win_h, size_t out_pitch, int cols,
                      double k, double dx, double dy, int mode, int filter, uint32_t background);

/* ---- frames of an index as a model-ready tensor batch: what OCR, UI understanding or an embedding model takes of a screen recording —
 * N x 3 x H x W or N x H x W x 3, float32 / float16 / bfloat16 / uint8, resized to the model's input and normalised per channel —
 * straight from the index, without a sheet of packed pixels and the passes over it that unpack, cast, scale and permute ---------------
 * Tensor: EQUIVALENCE  let P(i, x, y) be the word jsp_index_present writes at pixel (x, y) of cell i for the same frames, win_w, win_h,
 *       k, dx, dy, mode, filter and background: THE RULE of jsp_display_present / jsp_display_present_area is inherited, not restated,
 *       and all three filters are taken.  Channel ch (0 = R, 1 = G, 2 = B) has the byte v = (P >> 8 ch) & 0xFF; the top byte is not
 *       emitted.  A `background` pixel goes through the same mapping as any other.
 *   MODE  JSP_DISPLAY_CANVAS or JSP_DISPLAY_CANVAS_RGB15, the two conversions whose bytes 0, 1, 2 are R, G, B.
 *   ELEMENT  JSP_TENSOR_U8: v; scale and bias may be NULL and are ignored.  The float types: scale and bias are three floats each,
 *       required and finite, and f = (float)((double)v * (double)scale[ch] + (double)bias[ch]) — the product has at most 32
 *       significant bits and is exact in double (so an fma changes nothing), the sum rounds once to double, the result once to float.
 *       F32 is f; F16 is f rounded to nearest-even as binary16 (overflow to infinity); BF16 is f rounded to nearest-even as bfloat16.
 *   LAYOUT  dense, top window row first, no pitch, no cols, no sheet.  JSP_TENSOR_NCHW: element (i, ch, y, x) at
 *       ((i 3 + ch) win_h + y) win_w + x.  JSP_TENSOR_NHWC: at ((i win_h + y) win_w + x) 3 + ch.  The tensor occupies
 *       n 3 win_h win_w elements; nothing else is written.  `out` must be aligned to its element and needs no more than that (where
 *       win_w is a multiple of 4 and `out` lies on a boundary of four elements, four elements go out in one store).
 *   ONE kernel launch whatever n (msv1_index_tensor_kernel): the kernel of jsp_index_present with another last step; no full-size
 *       picture and no sheet is written and no frame buffer is touched.  Runs on the codec's stream and returns synchronised.  THE
 *       CODEC IS ONLY LENT, as for Present.  The frame list travels as Present's does, into the same device array of the index.
 *   BOUNDS  n, win_w, win_h, k, filter and frames[] as jsp_index_present; out_bytes at least n 3 win_h win_w esize (in 64 bits).
 *   ERRORS, each before anything is queued, with nothing changed and nothing written (jsp_last_error() starts with "index_tensor:", but
 *       for a ScreenPressor codec's "index: MSVideo1 only"): a null c, idx, frames or out; null scale or bias with a float dtype; a
 *       non-finite scale or bias; an unknown dtype or layout; a mode other than the two above; n, a window size, k or filter outside
 *       its bounds, a non-finite k, dx or dy; a frame number outside the index; out_bytes below the tensor; `out` not aligned to its
 *       element; a host-pointer `out`; an index built by another codec; a ScreenPressor codec; an asynchronous frame in flight. */
enum { JSP_TENSOR_F32 = 0, JSP_TENSOR_F16 = 1, JSP_TENSOR_BF16 = 2, JSP_TENSOR_U8 = 3 };
enum { JSP_TENSOR_NCHW = 0, JSP_TENSOR_NHWC = 1 };
int jsp_index_tensor(jsp_codec* c, jsp_index* idx, int n, const int* frames,
                     void* out, size_t out_bytes, int win_w, int win_h,
                     double k, double dx, double dy, int mode, int filter, uint32_t background,
                     int dtype, int layout, const float* scale, const float* bias);

/* ---- playback from an MSVideo1 index: reverse play and the step-back button held down, xs fast-forward, filling the free frame
 * buffers around the frame of interest — a run of frames of the index, each into a buffer of its own ----------------------------------
 * Play: EQUIVALENCE  for k = 0 .. n-1 let t_k = first + k * stride.  dsts[k] ends exactly as jsp_index_show(c, idx, t_k, dsts[k], 0, ..)
 *       leaves a buffer that held the same content before; data_pnts[k] (n entries; may be NULL) is that call's *data_pnt and
 *       significant_changes[k] (may be NULL) its verdict.  That includes everything Show leaves unwritten: a frame before the index's
 *       first adopting frame writes nothing to its buffer (its data_pnt is the previous frame of the build's time); a block that no
 *       frame <= t_k has coded is left untouched in dsts[k] when the index holds no picture before the range; the W % 4 / H % 4
 *       remainder pixels are copied only when there is a picture before the range.
 *   ADOPT  adopt_k = -1: the codec is not touched.  0 <= adopt_k < n: the codec ends exactly as jsp_index_show(t_adopt_k,
 *       dsts[adopt_k], adopt = 1) leaves it — previous frame, per-row block_changes, what the on-GPU parse needs — so a following
 *       DecompressP(t + 1) behaves as after sequential decoding.  Reverse play adopts k = 0 of an ascending run and shows the buffers
 *       in reverse.  jsp_key_frame_differs() answers -1 after an adopting call.
 *   ONE kernel launch whatever n and stride (msv1_index_play_kernel): per block frame `first` is composed as Show composes it, once;
 *       the 16 pixels then stay in registers, and for each further frame only the LAST writer of the gap (t_{k-1}, t_k] is decoded (a
 *       coded block overwrites the whole block), found in the bitmap with a lower bound.  Option "msv1_index_play_segments" splits the
 *       run along the grid.  Runs on the codec's stream and returns synchronised.  The destination pointers travel through pinned
 *       memory into a device array the index owns (both grown on demand, counted in jsp_index_info; an index never asked to play
 *       holds neither); a destination that Show would not write goes to the device as a null entry.
 *   ERRORS, each before anything is queued, with nothing changed and nothing written (jsp_last_error() starts with "index_play:", but
 *       for a ScreenPressor codec's "index: MSVideo1 only"): a null c, idx or dsts or a null entry of dsts, a ScreenPressor codec, an
 *       index built by another codec, n outside 1..4096, stride < 1, first < 0 or first + (n - 1) * stride (computed in 64 bits)
 *       outside the index, adopt_k outside -1..n-1, an asynchronous frame in flight, a codec in host-pointer mode or a host-pointer
 *       buffer, a buffer that is the codec's current previous frame, the same pointer twice in dsts. */
int jsp_index_play(jsp_codec* c, jsp_index* idx, int first, int n, int stride, int32_t* const* dsts, int adopt_k, int32_t** data_pnts,
                   int* significant_changes);

/* ---- ScreenPressor seek index: previous frame, seek-bar clicks and skip idle over a range whose host-stage records stay resident in
 * HBM (the calls above refuse ScreenPressor: its entropy stage is sequential host work, and the Manager's fallback decodes again from
 * the nearest key frame for every step back) -------------------------------------------------------------------------------------
 * Build: the host entropy stage runs over frames[0..nframes-1] ONCE (is_key as in jsp_stage_batch), in waves of at most 64 frames,
 *   groups of pictures side by side on host threads, with host decoders of the build's own.  Every inter frame's motion rectangles are
 *   rewritten as literal ones, so no block of an inter frame reads the picture before it anywhere but at its own position.  Kept in
 *   HBM: per key frame (coded or flat) its PICTURE, materialised by the key-frame kernels; per inter frame one 16-byte record per
 *   16x16 block and the literal pixels of its changed rectangles; a bitmap of which frame changes which block.  Everything goes up
 *   from pinned memory that the build owns and releases; the index keeps no pointer to `srcs`.
 *   RANGE  frames[0] must be a CODED key frame (it renews every bit of decoder state: the index depends on nothing before it).  Key
 *       frames (coded or flat), unchanged frames and inter frames of any mix may follow.
 *   RESULTS  The index (jsp_sp_index_destroy frees it), or NULL and jsp_last_error().
 *   ERRORS, each with nothing changed and nothing written: an MSVideo1 codec ("sp_index: ScreenPressor only"); a range that does not
 *       start at a coded key frame; a frame that does not end in JSP_ZERO_STATE or clears the previous frame (a truncated or invalid
 *       stream: the error names the frame's index in the range); nframes < 1, a null argument, a negative key_row; an asynchronous
 *       frame in flight; literal pixels beyond what the records' 32-bit offsets (in 16-byte units) reach.
 * Show: EQUIVALENCE  jsp_sp_index_show(t) writes into `dst` exactly the picture that a FRESH ScreenPressor codec of the same geometry
 *       and Preinit leaves as its previous frame after DecompressI / DecompressP of frames[0..t] in order, WHEN EACH FRAME'S
 *       DESTINATION STARTS OUT HOLDING THE PICTURE BEFORE IT (the rule of jsp_seek; it settles the one read an inter frame makes of
 *       its destination, "left of column 0": the build answers it with the last column of the picture before the frame).  Every pixel
 *       of `dst` is written, whatever it held.  *significant_changes (may be NULL) = what that sequential run records for frame t:
 *       an inter frame's DecompressP verdict; a key frame's frames_differ_significantly (Manager.hx:392-421) as jsp_find_change words
 *       it — the frame before is a key frame: their bytes differ; else the pixels from row `key_row` on differ from the picture
 *       before (judged once, at the build, on the GPU); frame 0: 1.
 *   ONE kernel launch (sp_index_show_kernel): no entropy decoding, no staging, no upload, no host pass over pictures.  Per 16x16 block
 *       the bitmap words are walked down from t / 32 to the frame after t's key picture; every pixel takes the literal of the last
 *       frame whose changed rectangle covers it, else the key picture's.  Runs on the codec's stream and returns synchronised.
 *   THE CODEC IS ONLY LENT  Build and Show use the codec's device, stream, Preinit value and key-frame options ("sp_band_rows",
 *       "sp_host_threads") and nothing else: its stream position, previous frame, entropy state and worker groups are exactly as
 *       before, and a sequential decode can go on across any number of builds and shows.  There is no `adopt`: the entropy state
 *       after frame t exists only at the end of a host decode.  One thing Show does to the codec: it has written a caller buffer
 *       behind the codec's back, so the codec forgets what it remembers of that buffer's last column (what option
 *       "sp_forget_buffers" does, for `dst` alone).
 *   ERRORS, each with nothing changed and nothing written: a null argument, an MSVideo1 codec, an index built by another codec, t
 *       outside 0..nframes-1, an asynchronous frame in flight, `dst` = the codec's current previous frame, a host-pointer `dst`.
 * Significance: out[0..nframes-1] = 1 / 0, the verdict Show reports for each frame.
 * Info: frames, and the bytes the index holds in HBM and in host memory (the build's staging memory is released when it returns).
 * Destroy: frees the index's device (and pinned) memory only; safe before or after jsp_codec_destroy of its codec. */
typedef struct jsp_sp_index jsp_sp_index;
jsp_sp_index* jsp_sp_index_build(jsp_codec* c, int nframes, const uint8_t* const* srcs, const size_t* lens, const uint8_t* is_key, int key_row);
int jsp_sp_index_show(jsp_codec* c, jsp_sp_index* idx, int t, int32_t* dst, int* significant_changes);
int jsp_sp_index_significance(const jsp_sp_index* idx, int* out);
int jsp_sp_index_info(const jsp_sp_index* idx, int* nframes, uint64_t* device_bytes, uint64_t* host_bytes);
void jsp_sp_index_destroy(jsp_sp_index* idx);

/* ---- thumbnails of a ScreenPressor index: jsp_index_thumb_size / jsp_index_thumbs for a jsp_sp_index, the same contract wherever it
 * can be, so that a caller treats both kinds of index alike --------------------------------------------------------------------------
 * Thumb size: for scale s = 4, 8 or 16, *width = X / s and *height = Y / s: whole s x s squares of the picture.  For these three
 *   scales that equals the MSVideo1 formula (4 * (W / 4)) / s, so one rule (tests/thumbs_ref.thumb_size) serves both.  The X % s /
 *   Y % s remainder pixels are left out.  A refused call writes neither, as jsp_index_thumb_size.
 * Thumbs: EQUIVALENCE  thumbnail k is the picture that jsp_sp_index_show(frames[k]) writes, reduced: pixel (x, y), per byte channel of
 *       the words, = (sum over the s x s source pixels at (x s .. x s + s - 1, y s .. y s + s - 1) + s s / 2) >> log2(s s); top byte
 *       0.  Rows keep the frame's bottom-up order.  There is no "picture before the range": a ScreenPressor index starts at a coded
 *       key frame and every pixel of every frame is defined.
 *   16 BPP  frames carry one 5-bit component per byte (Manager.hx:362-370), so the per-byte mean is the per-component mean and stays
 *       at most 31 per byte: jsp_display_convert with JSP_DISPLAY_CANVAS_RGB15 applies to a thumbnail, or to a whole sheet, as it
 *       does to a frame.  (A FLAT 16-bpp key frame is the reference's exception, in frames and so in thumbnails: it fills the picture
 *       with components already shifted left by 3, ScreenPressor.hx:134-139.  A mean never exceeds what it is the mean of.)
 *   SHEET  as jsp_index_thumbs: `out` is one image of cols * width by ceil(n / cols) * height pixels, pitch cols * width; thumbnail k
 *       has its pixel (0, 0) at (k / cols) * height * pitch + (k % cols) * width.  The cells of the last sheet row past n are not
 *       written.  frames[] is any list of frames of the index: unordered, repeats allowed.
 *   ONE kernel launch whatever n (sp_index_thumbs_kernel): per 16x16 block and thumbnail the walk of sp_index_show_kernel, the block
 *       kept in the wave's registers and summed across lanes; no full-size picture is written anywhere.  Runs on the codec's stream
 *       and returns synchronised.  THE CODEC IS ONLY LENT, as for Show; and since no frame buffer is written, the codec forgets
 *       nothing either.  One 24-byte record per thumbnail travels through pinned memory into a device array the index owns (both
 *       grown on demand, counted in jsp_sp_index_info; an index never asked for thumbnails holds neither).
 *   PRECONDITIONS  `out` is a device buffer of at least out_pixels ints; no asynchronous frame in flight.
 *   ERRORS  A null argument, an MSVideo1 codec ("sp_index: ScreenPressor only"), an index built by another codec, n outside 1..4096,
 *       a frame number outside the index, a scale other than 4 / 8 / 16, a picture too small for one thumbnail pixel at this scale,
 *       cols < 1, out_pixels smaller than the sheet, a violated precondition: JSP_ERROR_OCCURED, jsp_last_error() ("sp_index_thumbs:"
 *       / "sp_index_thumb_size:" ...), nothing written. */
int jsp_sp_index_thumb_size(const jsp_sp_index* idx, int scale, int* width, int* height);
int jsp_sp_index_thumbs(jsp_codec* c, jsp_sp_index* idx, int n, const int* frames, int scale, int cols, int32_t* out, size_t out_pixels);

/* ---- windows of a ScreenPressor index: jsp_index_present for a jsp_sp_index, the same contract wherever it can be ---------------------
 * Present: THE PICTURE of frame t is what jsp_sp_index_show(t) writes, all X x Y pixels of it.
 *   EQUIVALENCE, SHEET, BOUNDS, PRECONDITIONS  as jsp_index_present: cell i holds exactly the ints jsp_display_present (filter 0 / 1)
 *       or jsp_display_present_area (filter JSP_PRESENT_AREA) writes for the picture of frames[i] — THE RULE of those two calls.  For
 *       16 bpp the conversion that gives canvas pixels is JSP_DISPLAY_CANVAS_RGB15, as for a frame.
 *   ONE kernel launch whatever n (sp_index_present_kernel): per 16x16 block of a rectangle's source tile the walk of
 *       sp_index_show_kernel, into on-chip memory; no full-size picture is written anywhere.  Runs on the codec's stream and returns
 *       synchronised.  THE CODEC IS ONLY LENT, as for Show; and since no frame buffer is written, the codec forgets nothing: its
 *       state, previous frame, entropy state and remembered columns stay as they were.  The per-cell records are those of
 *       jsp_sp_index_thumbs and travel the same way, into the same device array (grown on demand, counted in jsp_sp_index_info).
 *   ERRORS  as jsp_index_present, with an MSVideo1 codec for the wrong kind ("sp_index: ScreenPressor only"); jsp_last_error()
 *       starts with "sp_index_present:" otherwise.  Nothing queued, nothing changed, nothing written. */
int jsp_sp_index_present(jsp_codec* c, jsp_sp_index* idx, int n, const int* frames,
                         int32_t* out, size_t out_ints, int win_w, int win_h, size_t out_pitch, int cols,
                         double k, double dx, double dy, int mode, int filter, uint32_t background);

/* ---- frames of a ScreenPressor index as a tensor batch: jsp_index_tensor for a jsp_sp_index, the same contract ------------------------
 * Tensor: EQUIVALENCE, MODE, ELEMENT, LAYOUT, BOUNDS  as jsp_index_tensor, with P(i, x, y) the word jsp_sp_index_present writes.  For
 *       16 bpp the mode is JSP_DISPLAY_CANVAS_RGB15, as for a frame.
 *   ONE kernel launch whatever n (sp_index_tensor_kernel): the kernel of jsp_sp_index_present with another last step.  Runs on the
 *       codec's stream and returns synchronised.  THE CODEC IS ONLY LENT, as for Present: its state, previous frame, entropy state and
 *       remembered columns stay as they were.  The per-cell records travel as Present's do, into the same device array.
 *   ERRORS  as jsp_index_tensor, with an MSVideo1 codec for the wrong kind ("sp_index: ScreenPressor only"); jsp_last_error() starts
 *       with "sp_index_tensor:" otherwise.  Nothing queued, nothing changed, nothing written. */
int jsp_sp_index_tensor(jsp_codec* c, jsp_sp_index* idx, int n, const int* frames,
                        void* out, size_t out_bytes, int win_w, int win_h,
                        double k, double dx, double dy, int mode, int filter, uint32_t background,
                        int dtype, int layout, const float* scale, const float* bias);

/* ---- playback from a ScreenPressor index: play on from a shown frame, reverse play, fast-forward by `stride`, filling the free frame
 * buffers around the frame of interest in one go — a run of frames of the index, each into a buffer of its own ---------------------------
 * Play: EQUIVALENCE  for k = 0 .. n-1, dsts[k] receives exactly the picture that jsp_sp_index_show(first + k * stride) writes, and
 *       significant_changes[k] (n ints, may be NULL) the verdict Show reports for that frame.  Every pixel of every buffer is written,
 *       whatever it held.  The frames between the strided ones are walked, not written.  The caller orders `dsts` as it likes: reverse
 *       playback is the same call with the buffers shown in reverse.
 *   ONE kernel launch whatever n and stride (sp_index_play_kernel): per 16x16 block frame `first` is composed by the walk of
 *       sp_index_show_kernel, once; the pixels then stay in registers and the frames are walked forward — one bitmap word per 32 frames, a
 *       record and its literals for a frame that changes the block, a reload from the key picture at a key frame (coded or flat) inside
 *       the run, nothing for a frame that leaves the block alone — and stored at every stride-th frame.  Runs on the codec's stream and
 *       returns synchronised.  Per frame of the index a 16-byte record and a key-frame bit go to a device array the index owns at the
 *       first Play; the destination list of a call travels through pinned memory into a device array (both grown on demand).  All of it
 *       is counted in jsp_sp_index_info; an index never asked to play holds none of it.
 *   THE CODEC IS ONLY LENT, as for Show: device, stream, Preinit and options are used, nothing else is touched, and a sequential decode
 *       goes on across any number of Plays.  One thing Play does to the codec: it forgets what it remembers of the last column of EVERY
 *       buffer in `dsts`.  There is no `adopt`; a player that plays from the index to the end of a key interval hands over to the
 *       ordinary decoder at the next coded key frame, which renews every bit of decoder state.
 *   ERRORS, each before anything is queued, with nothing changed and nothing written (jsp_last_error() starts with "sp_index_play:",
 *       but for the MSVideo1 codec's "sp_index: ScreenPressor only"): a null argument or a null entry of `dsts`, an MSVideo1 codec, an
 *       index built by another codec, n outside 1..4096, stride < 1, first < 0 or first + (n - 1) * stride (computed in 64 bits) outside
 *       the index, an asynchronous frame in flight, a host-pointer buffer, a buffer that is the codec's current previous frame, the same
 *       pointer twice in `dsts`. */
int jsp_sp_index_play(jsp_codec* c, jsp_sp_index* idx, int first, int n, int stride, int32_t* const* dsts, int* significant_changes);

/* ---- activity map of an index, either codec: where and when a screen recording changes — an activity strip along the seek bar, "skip
 * idle" judged on the part of the picture in view, the rectangle a frame changed to scroll the view to, the frames worth giving to a
 * model — as changed pixels per frame and 16x16 cell, without a picture written or compared anywhere ---------------------------------------
 * Activity: THE PICTURE P(t) of frame t, 0 <= t < nframes, is the one jsp_index_present / jsp_sp_index_present define: not restated.
 *       P(-1), MSVideo1: the index's copy of the picture before the range, else all zeros.  P(-1), ScreenPressor: all zeros (its index
 *       starts at a coded key frame and holds nothing before it).  An MSVideo1 block that no frame <= t has coded and that has no picture
 *       before the range is zeros in P(t), as for Thumbs and Present: a first writer that writes zeros changes nothing.
 *   GRID  *cols = ceil(X / 16), *rows = ceil(Y / 16) (jsp_index_activity_size / jsp_sp_index_activity_size).  Cell (r, q) covers stored
 *       rows 16 r .. 16 r + 15 and columns 16 q .. 16 q + 15, clipped to the picture.  Rows are in the frame buffer's own order: grid row
 *       0 is frame rows 0 .. 15, as Thumbs keeps it.  A cell is the ScreenPressor block and 4 x 4 MSVideo1 blocks.
 *   EQUIVALENCE  out[(k * rows + r) * cols + q] = the number of pixels of cell (r, q) whose whole 32-bit word differs between
 *       P(first + k) and P(first + k - 1), for k = 0 .. n-1: 0 .. 256.  The X % 4 / Y % 4 remainder pixels of an MSVideo1 picture are
 *       the same in every P(t) and so never count.  Exactly n * rows * cols elements are written, every one of them; nothing else is.
 *       Coarser grids, totals and boxes are sums the caller takes: the call has one cell size, so every cell has one owner.
 *   ONE kernel launch whatever n (msv1_index_activity_kernel / sp_index_activity_kernel), behind a memset of `out` on the same stream:
 *       the walk of jsp_index_play / jsp_sp_index_play with a compare-and-count where Play has a store; a set bit of the index's bitmap
 *       is not a change (MSVideo1 codes a block again with the pixels it had; a ScreenPressor rectangle is the bounding box of a change
 *       and its literalised motion rewrites pixels that stay), so the pixels are compared.  Option "msv1_index_activity_segments"
 *       splits an MSVideo1 run along the grid, as "msv1_index_play_segments" does; the result does not depend on it.  Runs on the
 *       codec's stream and returns synchronised.  THE CODEC IS ONLY LENT, as for Thumbs / Present: its state, previous frame, per-row
 *       flags and every frame buffer stay untouched.  No full-size picture is written anywhere; the index grows by nothing the size of a
 *       picture (a ScreenPressor index that never played gets Play's 16-byte record and key-frame bit per frame).
 *   BOUNDS  n 1..4096; first >= 0; first + n <= nframes (computed in 64 bits); out_elems >= n * rows * cols; `out` is a device pointer
 *       aligned to 2 bytes.
 *   ERRORS, each before anything is queued, with nothing changed and nothing written (jsp_last_error() starts with "index_activity:",
 *       but for the wrong codec kind's "index: MSVideo1 only" / "sp_index: ScreenPressor only"): a null argument, n or first outside
 *       their bounds, out_elems too small, a misaligned or host-pointer `out`, an index built by another codec, the wrong codec kind, an
 *       asynchronous frame in flight. */
int jsp_index_activity_size(const jsp_index* idx, int* cols, int* rows);
int jsp_index_activity(jsp_codec* c, jsp_index* idx, int first, int n, uint16_t* out, size_t out_elems);
int jsp_sp_index_activity_size(const jsp_sp_index* idx, int* cols, int* rows);
int jsp_sp_index_activity(jsp_codec* c, jsp_sp_index* idx, int first, int n, uint16_t* out, size_t out_elems);

/* ---- distance map of an index, either codec: how far each frame is from ONE picture — where else the recording shows this picture (a
 * dialog that comes back, a loop, A -> B -> A), which frame looks like this screenshot, which frames differ enough from the last kept one
 * to be worth keeping, where a loop can close without a jump — as differing pixels per frame and 16x16 cell.  The activity map cannot
 * say it: the sum of changes along a path is the path's length, not the distance between its ends ---------------------------------------
 * Distance: THE PICTURE P(t), P(-1) and THE GRID are the activity map's, above (jsp_index_activity_size / jsp_sp_index_activity_size
 *       give cols and rows): not restated.
 *   THE REFERENCE R, two forms:
 *       ref_picture == NULL: R = P(ref_frame), ref_frame -1 .. nframes-1.  The kernel composes R's blocks itself; no picture is written
 *           and no Show is needed first.
 *       ref_picture != NULL: ref_frame must be JSP_REF_PICTURE.  R is a device buffer of X * Y words in frame-buffer layout.  It is
 *           only read; it may be any frame buffer, the codec's previous frame included.  It must be aligned to 4 bytes: rows are read
 *           16 bytes at a time where the pointer is 16-byte aligned and X % 4 == 0, word by word otherwise.
 *   EQUIVALENCE  out[(k * rows + r) * cols + q] = the number of pixels of cell (r, q) whose whole 32-bit word differs between
 *       P(first + k) and R, for k = 0 .. n-1: 0 .. 256.  ScreenPressor: every pixel of the cell inside the picture is compared.
 *       MSVideo1: the pixels inside whole 4 x 4 blocks are compared; THE X % 4 / Y % 4 REMAINDER PIXELS ARE NEVER READ AND NEVER
 *       COUNTED.  They are the same in every P(t), so with a frame as reference they would contribute 0 anyway; with a device picture as
 *       reference they are the caller's to compare.  Exactly n * rows * cols elements are written, every one of them, by the launch
 *       itself: nothing else is written and no memset goes in front (most elements are non-zero, unlike Activity's).
 *   ONE kernel launch whatever n (msv1_index_distance_kernel / sp_index_distance_kernel): the walk of Play and Activity with a third
 *       last step, a count against R; where a cell has no event its value is stored again.  Option "msv1_index_activity_segments" splits
 *       an MSVideo1 run along the grid here too — it is ONE knob for both walks, Activity's and Distance's — and the result does not
 *       depend on it.  Runs on the codec's stream and returns synchronised.  THE CODEC IS ONLY LENT, as for Activity; no full-size
 *       picture is written anywhere, and the index grows as for Activity.
 *   BOUNDS  Activity's: n 1..4096; first >= 0; first + n <= nframes (computed in 64 bits); out_elems >= n * rows * cols; `out` is a
 *       device pointer aligned to 2 bytes.
 *   ERRORS, each before anything is queued, with nothing changed and nothing written (jsp_last_error() starts with "index_distance:",
 *       but for the wrong codec kind's "index: MSVideo1 only" / "sp_index: ScreenPressor only"): Activity's — a null c, idx or out, n or
 *       first outside their bounds, out_elems too small, a misaligned or host-pointer `out`, an index built by another codec, the wrong
 *       codec kind, an asynchronous frame in flight — and three more: a ref_frame outside -1 .. nframes-1; ref_frame and ref_picture that
 *       disagree (a picture without JSP_REF_PICTURE, JSP_REF_PICTURE without a picture); a ref_picture that is a host pointer or not
 *       aligned to 4 bytes. */
#define JSP_REF_PICTURE (-2)
int jsp_index_distance(jsp_codec* c, jsp_index* idx, int ref_frame, const int32_t* ref_picture, int first, int n, uint16_t* out, size_t out_elems);
int jsp_sp_index_distance(jsp_codec* c, jsp_sp_index* idx, int ref_frame, const int32_t* ref_picture, int first, int n, uint16_t* out,
                          size_t out_elems);

/* ---- a key frame for any frame of an MSVideo1 index: cut a clip at frame t.  A clip has to start on a key frame, and t is almost never
 * one.  The picture of frame t is, block by block, what the last frame <= t that coded the block made of it, and that frame's code for
 * the block lies in the index's resident stream bytes: the key frame is those codes, concatenated in block order.  No pixel is
 * decoded, nothing is re-quantised, and every byte of the result is a byte of a code the range already contained -------------------------
 * KeyFrame: let e be the end of the writer's frame data (16-bit: rounded down to a whole word).  The code at offset o is WHOLE when
 *       (1) its two-byte code word lies below e, (2) the bytes that settle its length lie below e — for a 16-bit code whose second byte
 *       is below 0x80 that is the colour word at o + 2 — and (3) o + L <= e, L being 2 / 6 / 18 bytes (16-bit: 1-, 2-, 8-colour code)
 *       or 2 / 4 / 10 bytes (8-bit).  KeyFrame(t) = for blocks 0 .. nblocks-1 in table order, which is stream order, the L bytes of the
 *       whole code of the block's last writer <= t.  No skip codes, no end marker, nothing after the last block.
 *   PROMISED for the bytes written: jsp_is_key_frame says yes; decoded as a key frame they give the picture of frame t on every pixel a
 *       block covers (the X % 4 / Y % 4 remainder pixels are in no MSVideo1 frame and stay the caller's); the range's frames t + 1 ...
 *       decoded on top give the pictures the range gives.  NOT promised: that significance verdicts, per-row flags or data_pnt of the
 *       cut clip equal the original's — the new key frame codes every block.
 *   REFUSED, as an error with nothing written: a block that no frame <= t of the index codes (it shows the picture before the range, or
 *       nothing: its pixels came from no code the index holds) — the text names the first such block; a block whose last writer's code
 *       is not whole (the end of a damaged frame cuts it off; what the reference paints there need not be expressible) — the text names
 *       the block and the frame.  One rule for both depths; nothing is re-encoded.
 *   `out` is HOST memory: these are file bytes.  *len is set to the frame's length whenever the frame can be cut, also when `cap` is
 *       smaller — that is then an error with nothing written: size `out` by jsp_index_key_frame_bound (nblocks * 18 for 16-bit,
 *       nblocks * 10 for 8-bit) or ask twice (`out` may be null when cap is 0).  *len is 0 after every other error.
 *   TWO kernel launches (msv1_index_keyframe_sizes_kernel: per block the writer and the code's length, a scan inside each workgroup of
 *       1024 blocks, a total per workgroup; msv1_index_keyframe_gather_kernel: the totals before its own summed, the codes copied) — no
 *       workgroup waits for another.  The bytes are assembled in device scratch of the index (8 bytes per block, 4 per workgroup, the
 *       frame at its bound; allocated by the first call, counted by jsp_index_info) and reach `out` in one copy only after the status
 *       says that the frame can be cut.  Runs on the codec's stream and returns synchronised.  THE CODEC IS ONLY LENT: its state and
 *       every frame buffer stay untouched.
 *   ERRORS, each before anything is queued (jsp_last_error() starts with "index_key_frame:", but for the wrong codec kind's "index:
 *       MSVideo1 only"): a null argument, the wrong codec kind, an index built by another codec, t outside the index, a picture without
 *       a 4x4 block, an asynchronous frame in flight. */
int jsp_index_key_frame_bound(const jsp_index* idx, size_t* bytes);
int jsp_index_key_frame(jsp_codec* c, jsp_index* idx, int t, uint8_t* out, size_t cap, size_t* len);

/* ---- inter frames that span a gap of an MSVideo1 index: thin a clip.  A x8 time-lapse, "the same recording without its idle frames",
 * "frames 100, 164, 228, ..." each need frames that exist in no file.  An inter frame that takes the picture of frame a to the picture
 * of frame b is, block by block, the code of the block's last writer in (a, b] or a skip: again no pixel is decoded, nothing is
 * re-quantised, and every code byte is one the range contained ------------------------------------------------------------------------
 * Delta: WHOLE is KeyFrame's definition above.  Block i is WRITTEN in (a, b] when some frame f with a < f <= b codes it; a = -1 means
 *       "from before the range".  Delta(a, b), -1 <= a < b < nframes = for blocks i = 0 .. nblocks-1 in table order:
 *         - i is written: the L bytes of the whole code of its last writer <= b;
 *         - i is not written and is a RUN HEAD (i = 0, or block i - 1 is written, or i % 1023 = 0): one skip word, bytes (count & 0xFF,
 *           0x84 + (count >> 8)), count = the consecutive unwritten blocks from i on, stopping before the next written block, before
 *           the next multiple of 1023 above i, and at nblocks: 1 <= count <= 1023;
 *         - otherwise: nothing.
 *       A skip word never crosses a block number that is a multiple of 1023 (the format's 10-bit count).  The frame always covers all
 *       nblocks blocks.  A gap that writes nothing gives ceil(nblocks / 1023) skip words (shorter than the 16-bit decoder's early-out
 *       threshold, which it takes); a gap that writes every block gives no skip word and is, from a = -1, byte for byte KeyFrame(b).
 *   PROMISED: decoded as an inter frame on top of the picture of frame a (a = -1: the picture before the range, where one is defined)
 *       the bytes give the picture of frame b on every pixel a block covers; jsp_is_key_frame is true exactly when every block is
 *       written; len(Delta(a, b)) <= len(KeyFrame(b)) whenever both exist.  NOT promised: significance verdicts, per-row flags and
 *       data_pnt of the thinned clip — the exclusions of KeyFrame.
 *   REFUSED, as an error with nothing written: a written block whose last writer's code is not whole; the text names the pair, the
 *       block and the writer frame — of the FIRST refusing (pair, block) in that order.  A block without a writer is skipped, never
 *       refused.
 *   n pairs (from[j], to[j]], n in 1 .. 4096, independent of each other; frame j = Delta(from[j], to[j]); the frames lie back to back in
 *       `out`, HOST memory.  lens[j] and *total are set whenever every pair can be cut, also when `cap` is smaller than *total — that
 *       is then an error with nothing written (`out` may be null when cap is 0); they are zeros after every other error.  Size `out` by
 *       n * jsp_index_delta_bound (per frame nblocks * 18 for 16-bit, nblocks * 10 for 8-bit) or ask twice.
 *   TWO kernel launches for a slice of pairs, grid.y = the pair, in the shape of KeyFrame's (msv1_index_delta_sizes_kernel,
 *       msv1_index_delta_gather_kernel) — no workgroup waits for another.  A call runs in slices of pairs so that the scratch the index
 *       owns stays bounded (per pair 8 bytes per block, 8 per workgroup, the frame at its bound; allocated by the first call, counted
 *       by jsp_index_info): a sizes launch per slice first, so that statuses and lengths of ALL pairs are known before the first byte
 *       reaches `out`, then sizes and gather per slice (a single slice: the gather alone).  Option "msv1_index_delta_slice" sets the
 *       pairs per slice; the bytes do not depend on it.  Runs on the codec's stream and returns synchronised.  THE CODEC IS ONLY LENT.
 *   ERRORS, each before anything is queued (jsp_last_error() starts with "index_delta:", but for the wrong codec kind's "index:
 *       MSVideo1 only"), in this order: a null argument, the wrong codec kind, an index built by another codec, n outside 1 .. 4096, the
 *       first bad pair (from < -1, to <= from, to >= nframes), a picture without a 4x4 block, an asynchronous frame in flight. */
int jsp_index_delta_bound(const jsp_index* idx, size_t* bytes);
int jsp_index_delta_frames(jsp_codec* c, jsp_index* idx, int n, const int* from, const int* to, uint8_t* out, size_t cap, size_t* lens,
                           size_t* total);

/* ---- the same inter frames, tight: a block that the gap codes but whose pixels it does not change is dropped.  A gap that spans a key
 * frame of the clip writes every block, a picture that returns to an earlier state (a blinking cursor, A -> B -> A) is coded again in
 * full, an encoder may recode a block with what it already shows: Delta carries all of those, Tight carries none --------------------
 * Tight: WHOLE, WRITTEN, RUN HEAD, the skip word and the 1023 rule are Delta's.  P(t)[i] is the 16 frame-buffer words that the last
 *       frame <= t coding block i makes of it (a code that a frame's end cuts off is decoded as the decoder decodes it), else the block
 *       of the picture before the range; P(a)[i] is DEFINED when one of the two exists (for a = -1 only the picture before the range
 *       can define it).  Block i is KEPT in (a, b] when it is written in (a, b] and either P(a)[i] is not defined or P(b)[i] differs
 *       from P(a)[i] in at least one of the 16 words; every other block — unwritten, or written but unchanged — is DROPPED.  Pixels are
 *       compared as the 32-bit words a frame buffer holds: two 8-bit palette indices of one colour are equal, and so are different
 *       code bytes that decode alike.  Tight(a, b) is Delta's rule with "written" replaced by "kept" everywhere: in the codes, in the
 *       run-head test (is block i - 1 kept?) and in the counts.
 *   PROMISED: decoded as an inter frame on top of the picture of frame a the bytes give the picture of frame b on every pixel a block
 *       covers; jsp_is_key_frame is true exactly when every block is kept; len(Tight(a, b)) <= len(Delta(a, b)) whenever both exist
 *       (a dropped block removes L >= 2 bytes and adds at most one skip word); Tight(a, b) == Delta(a, b) when nothing is dropped, in
 *       particular for a = -1 on a range with no picture before it; a gap across which no pixel of any block changed gives exactly
 *       ceil(nblocks / 1023) skip words.  NOT promised: the exclusions of KeyFrame and Delta.
 *   REFUSED, as an error with nothing written: a KEPT block whose last writer's code is not whole; the text is Delta's with the prefix
 *       "index_tight:" and names the FIRST refusing (pair, block) in that order.  A dropped block never refuses, even when its
 *       writer's code is cut off: its pixels were defined and equal, and none of its bytes are used.
 *   Everything else is jsp_index_delta_frames', word for word: n pairs in 1 .. 4096, `out` in HOST memory, lens[] and *total set when
 *       only `cap` is short, zeros and nothing written after every other error, jsp_index_delta_bound, the index's scratch (shared
 *       with Delta's), option "msv1_index_delta_slice" (the bytes do not depend on it), synchronised on return, THE CODEC ONLY LENT.
 *       Two launches per slice as well: the sizes launch is msv1_index_delta_sizes_kernel's TIGHT form, which decodes both ends of the
 *       gap of every written block and compares them; the gather launch is Delta's.
 *   ERRORS: Delta's, in Delta's order, jsp_last_error() starting with "index_tight:". */
int jsp_index_tight_frames(jsp_codec* c, jsp_index* idx, int n, const int* from, const int* to, uint8_t* out, size_t cap, size_t* lens,
                           size_t* total);

/* CROP A CLIP: the frames of a block rectangle of an MSVideo1 index — the spatial counterpart of the key-frame cut and of Delta /
 * Tight, by the same means.  An MSVideo1 code carries no position (colours and a mask; 8 bits: indices into the palette, which the
 * cropped clip keeps), so the clip of a block-aligned rectangle is a gather of codes the index holds: no pixel decoded, nothing
 * re-quantised.
 *   THE RECTANGLE is (bx, by, bw, bh) in 4x4 blocks in TABLE order: block row 0 is stored rows 0 .. 3 of a frame buffer, the bottom of
 *       the picture as displayed.  bw, bh >= 1, 0 <= bx, bx + bw <= nbx, 0 <= by, by + bh <= nby.  nb = bw * bh; block j < nb of the
 *       rectangle is source block src(j) = (by + j / bw) * nbx + bx + j % bw.  The cropped clip is 4 bw x 4 bh pixels, with the
 *       source's bit depth and palette.
 *   THE RULE (stated in msv1_index_crop_kernels.hip): WHOLE, WRITTEN, RUN HEAD, the skip word, the 1023 rule and KEPT of
 *       jsp_index_key_frame / _delta_frames / _tight_frames, applied to the virtual index whose block j is source block src(j),
 *       everything in j-numbering: a run head is j = 0, block j - 1 OF THE RECTANGLE written (kept), or j % 1023 = 0; counts stop at
 *       the next multiple of 1023 in j and at nb.  A pair is
 *         a GAP pair (from, to], -1 <= from < to < nframes: Delta, or with JSP_CROP_TIGHT in `flags` Tight, of the virtual index.  A cut
 *           code of a written (tight: kept) block refuses; a block without a writer is skipped;
 *         a KEY pair, from == JSP_CROP_KEY, 0 <= to < nframes: the whole code of the last writer <= to of every src(j), no skip words.
 *           A block of the rectangle with no writer <= to refuses ("no writer"), a cut code refuses ("cut").  JSP_CROP_TIGHT does not
 *           touch key pairs.
 *       Blocks outside the rectangle never matter: a rectangle can be cut where jsp_index_key_frame of the whole picture refuses.
 *   PROMISED: a fresh decoder of 4 bw x 4 bh pixels fed a key pair's frame as a key frame, then gap pairs' frames chained
 *       to[k - 1] == from[k] as inter frames, holds after each the stored rows 4 by .. 4 by + 4 bh - 1, columns 4 bx .. 4 bx + 4 bw - 1
 *       of the source picture of frame to[k].  With the rectangle equal to the whole block grid the bytes are those of
 *       jsp_index_delta_frames / _tight_frames, and a key pair's those of jsp_index_key_frame(to).  Every frame is at most
 *       jsp_index_crop_bound's bytes (nb * 18; 8 bits: nb * 10).  keys[j] (may be null) = frame j codes every block of the rectangle:
 *       jsp_is_key_frame of it.  NOT promised: the exclusions of KeyFrame.
 *   REFUSED, as an error with nothing written: the text starts with "index_crop:" and names the FIRST refusing (pair, block) in that
 *       order — the pair, the block in the rectangle's numbering and in the picture's, the kind, and for "cut" the writer frame.
 *   Everything else is jsp_index_delta_frames', word for word: n pairs in 1 .. 4096, `out` in HOST memory, frames back to back, lens[],
 *       keys[] and *total set when only `cap` is short, zeros and nothing written after every other error, a scratch of the index's
 *       own that jsp_index_info counts, option "msv1_index_delta_slice" (the bytes do not depend on it), synchronised on return, THE
 *       CODEC ONLY LENT.  Two launches per slice: msv1_index_crop_sizes_kernel, msv1_index_crop_gather_kernel.
 *   ERRORS before anything is queued, in this order: a null argument; not an MSVideo1 codec ("index: MSVideo1 only"); an index of
 *       another codec; a rectangle outside the block grid (also: a picture without a block); n outside 1 .. 4096; unknown flag bits;
 *       the first bad pair; an asynchronous frame in flight. */
#define JSP_CROP_KEY   (-2)
#define JSP_CROP_TIGHT 1
int jsp_index_crop_bound(const jsp_index* idx, int bw, int bh, size_t* bytes);
int jsp_index_crop_frames(jsp_codec* c, jsp_index* idx, int bx, int by, int bw, int bh, int n, const int* from, const int* to, int flags,
                          uint8_t* out, size_t cap, size_t* lens, int* keys, size_t* total);

/* PAN A CROP: the frames of a block rectangle THAT MOVES — a 640x360 clip that follows the action across a 1080p recording, the
 * rectangle jsp_index_activity names ("the rectangle a frame changed to scroll the view to") joined to jsp_index_crop_frames.  Codes
 * carry no position, so a moved rectangle stays a gather: the block at position j of the new rectangle is either the same 16 words
 * as the block that stood at position j of the old one (skipped) or gets the code of its last writer (copied).
 *   A CALL has one rectangle size (bw, bh) in 4x4 blocks, nb = bw * bh, and n pairs.  Pair k: from[k], to[k], the origin
 *       A = (from_xy[2k], from_xy[2k+1]) of the rectangle at frame `from` and B = (to_xy[2k], to_xy[2k+1]) at frame `to`, both (bx, by)
 *       in table order as in crop.  srcA(j), srcB(j): crop's src(j) for the two origins.
 *   THE RULE (PAN, stated in msv1_index_pan_kernels.hip).  A pair is
 *         a KEY pair, from == JSP_CROP_KEY: crop's key pair of rectangle B at `to`; from_xy is not read;
 *         a STILL gap pair, A == B and -1 <= from < to < nframes: crop's gap pair (Delta, or Tight with JSP_CROP_TIGHT);
 *         a MOVED pair, A != B and -1 <= from <= to, 0 <= to < nframes (from == to only here: a pan across a picture that stands
 *           still).  Without JSP_CROP_TIGHT: the bytes and refusals of the KEY pair (B, to), keys[k] = 1.  With it: block j is DROPPED
 *           when P(from)[srcA(j)] and P(to)[srcB(j)] are both defined and equal in all 16 words, else KEPT — "written in the gap"
 *           plays no part.  A kept block gives the whole code of the last writer <= to of srcB(j); without one it refuses ("no
 *           writer"), with a cut code it refuses ("cut"); a dropped block never refuses.  Run heads and counts are Tight's, in j.
 *   PROMISED: a fresh decoder of 4 bw x 4 bh pixels fed a KEY pair's frame as a key frame, then the frames of pairs chained by
 *       to[k-1] == from[k] and to_xy[k-1] == from_xy[k], holds after each the pixels of rectangle B of the source picture of to[k].  A
 *       call whose pairs are all KEY or STILL with one origin throughout returns byte for byte what jsp_index_crop_frames returns
 *       for that rectangle (lens, keys, total and the refusal texts too, apart from the prefix).  A moved tight frame is never longer
 *       than the KEY pair (B, to).  NOT promised: the exclusions of KeyFrame.
 *   REFUSED as in crop, the text starting with "index_pan:"; a moved pair reads "(from -> to, moved)", and the picture's block number
 *       is srcB(j).
 *   Everything else is jsp_index_crop_frames', word for word: jsp_index_crop_bound(idx, bw, bh) sizes `out` (HOST memory, frames back
 *       to back), lens[], keys[] (may be null) and *total set when only `cap` is short, zeros and nothing written after every other
 *       error, slices under "msv1_index_delta_slice" with a sizes launch for all slices first, a scratch of the index's own that
 *       jsp_index_info counts, synchronised on return, THE CODEC ONLY LENT.  Two launches per slice: msv1_index_pan_sizes_kernel,
 *       msv1_index_pan_gather_kernel.
 *   ERRORS before anything is queued, in this order: a null argument (keys may be null; from_xy may be null only when every pair is a
 *       KEY pair); not an MSVideo1 codec ("index: MSVideo1 only"); an index of another codec; bw or bh outside 1 .. nbx / 1 .. nby
 *       (also: a picture without a block); n outside 1 .. 4096; unknown flag bits; the first bad pair — its frames by its kind, then B
 *       outside the grid, then for gap pairs A outside the grid (the text names the pair and which); an asynchronous frame in flight. */
int jsp_index_pan_frames(jsp_codec* c, jsp_index* idx, int bw, int bh, int n, const int* from, const int* to, const int* from_xy,
                         const int* to_xy, int flags, uint8_t* out, size_t cap, size_t* lens, int* keys, size_t* total);

/* REVERSE A CLIP: the frames of a block rectangle ALONG ANY PATH through an MSVideo1 index — a reversed clip, a boomerang (there and
 * back, loopable), a freeze frame: the temporal counterpart of crop and pan.  A code carries no position and no reference to the
 * previous picture, so the inter frame that takes the picture of frame a BACK to the picture of frame b < a is a gather of codes the
 * index holds, as the step forward is: no pixel decoded, nothing re-quantised.
 *   THE RECTANGLE, src(j) and the j-numbering are crop's; the whole block grid as the rectangle gives the whole picture.
 *   THE RULE (PATH, stated in msv1_index_path_kernels.hip).  A pair (from = a, to = b) is
 *         a KEY pair, a == JSP_CROP_KEY, 0 <= b < nframes: crop's key pair;
 *         a FORWARD pair, -1 <= a < b < nframes: crop's gap pair (Delta, or Tight with JSP_CROP_TIGHT);
 *         a HOLD pair, 0 <= a == b < nframes: nothing is touched, the frame is ceil(nb / 1023) skip words;
 *         a BACK pair, 0 <= b < a < nframes.
 *       For the three kinds that are not KEY, with lo = min(a, b) and hi = max(a, b): block j is TOUCHED when some frame f,
 *       lo < f <= hi, codes src(j).  Without JSP_CROP_TIGHT a touched block is KEPT; with it a touched block is DROPPED when
 *       P(a)[src(j)] and P(b)[src(j)] are both defined and equal in all 16 words, else KEPT.  A kept block gives the whole code of the
 *       last writer <= b of src(j); without one it refuses ("no writer": only a BACK pair can, and it does even where the picture
 *       before the range defines P(b) — those pixels come from no code the index holds), with a cut code it refuses ("cut").  Dropped
 *       and untouched blocks are skipped under Delta's run-head and count rules in j and never refuse.
 *   PROMISED: a fresh decoder of 4 bw x 4 bh pixels fed a KEY pair's frame as a key frame, then the frames of pairs chained by
 *       to[k-1] == from[k] in any mix of kinds, holds after each the rectangle of the source picture of to[k].  keys[k] = the frame codes
 *       all nb blocks: jsp_is_key_frame of it.  A tight frame is never longer than the loose one.  Back(a, b) and Delta(b, a) have
 *       the same touched set, hence the same skip words when neither is tight.  A call of only KEY and FORWARD pairs returns byte
 *       for byte what jsp_index_crop_frames returns (lens, keys, total and the refusal texts too, apart from the prefix).  NOT
 *       promised: the exclusions of KeyFrame, and a step back to before the range (to = -1).
 *   REFUSED as in crop, the text starting with "index_path:" and naming the FIRST refusing (pair, block) in that order; a BACK pair
 *       reads "(from -> to, back)".
 *   Everything else is jsp_index_crop_frames', word for word: jsp_index_crop_bound(idx, bw, bh) sizes `out` (HOST memory, frames back
 *       to back), lens[], keys[] (may be null) and *total set when only `cap` is short, zeros and nothing written after every other
 *       error, slices under "msv1_index_delta_slice" with a sizes launch for all slices first, the scratch of the crop call (one of
 *       the index's own that jsp_index_info counts), synchronised on return, THE CODEC ONLY LENT.  Two launches per slice:
 *       msv1_index_path_sizes_kernel, msv1_index_crop_gather_kernel.
 *   ERRORS before anything is queued, in this order: a null argument (keys may be null); not an MSVideo1 codec ("index: MSVideo1
 *       only"); an index of another codec; a rectangle outside the block grid (also: a picture without a block); n outside 1 .. 4096;
 *       unknown flag bits; the first bad pair — from < JSP_CROP_KEY, from == -1 with to < 0, `to` outside 0 .. nframes - 1, or
 *       from >= nframes (the text names the pair and says what a pair may be); an asynchronous frame in flight. */
int jsp_index_path_frames(jsp_codec* c, jsp_index* idx, int bx, int by, int bw, int bh, int n, const int* from, const int* to, int flags,
                          uint8_t* out, size_t cap, size_t* lens, int* keys, size_t* total);

/* ---- ENCODE PICTURES AS MSVIDEO1: frames from any picture in device memory.  Every clip call above gathers codes that an MSVideo1
 * index already holds — exact and fast, and no help for what exists only as pixels: the pictures of a ScreenPressor index (its stream
 * is entropy coded), a window of jsp_index_present, a block that no frame of an index codes (KeyFrame refuses it), any picture the
 * caller holds.  This is the encoder for those, 16-bit MSVideo1 only: a pure function of pictures in HBM ---------------------------------
 * Encode (the decoder it inverts: MSVideo1.hx:119-181):
 *   GEOMETRY  A picture is width x height 32-bit words; row y starts at base + y * pitch ints; pitch is signed and |pitch| >= width.  A
 *       frame buffer as the codecs leave it has pitch = width; a top-row-first window is given as a pointer to its LAST row with a
 *       negative pitch; a cell of a sheet by the sheet's pitch.  nbx = width >> 2, nby = height >> 2, blocks in table order (block row 0
 *       is rows 0..3); pixel k = 4 y + x of a block is flag bit k.  The width % 4 / height % 4 remainder pixels are never read.
 *   QUANTISATION  q(p) = ((p >> 3) & 0x1F) | ((p >> 6) & 0x3E0) | ((p >> 9) & 0x7C00), the inverse of fromRGB15 on the layout
 *       0x00RRGGBB that MSVideo1 and 24-bpp ScreenPressor frame buffers share.  No other bit of a word is read: the top byte may hold
 *       anything, for example the 0xFF of JSP_DISPLAY_SETPIXELS.  v[k] = q(p[k]).
 *   QUADRANTS  Quadrant i of 0..3 holds pixels {0,1,4,5}, {2,3,6,7}, {8,9,12,13}, {10,11,14,15}; its last pixel is 5, 7, 13, 15; its
 *       colour pair is stream colours 2i (taken where the code word's bit is SET) and 2i + 1 (where it is CLEAR).
 *   THE CODE OF A BLOCK, decided on v alone:
 *       1. all 16 values equal c: the two bytes of 0x8000 | c when (c & 0x7C00) != 0x0400; otherwise the word's high byte would be
 *          0x84..0x87, a skip: then the six bytes 00 00, c, c — a two-colour code of one colour;
 *       2. exactly two distinct values: B = v[15], A the other; the word has bit k set where v[k] == A (bit 15 is clear by
 *          construction); then A, B.  Six bytes; A carries bit 15 clear;
 *       3. otherwise 18 bytes: the word, then F0 | 0x8000, S0, F1, S1, F2, S2, F3, S3 (bit 15 clear in all colours but the first).  Per
 *          quadrant — at most two distinct values: S is the value of the quadrant's last pixel, F the other (F = S when there is one),
 *          bits are set where v[k] != S; three or four distinct values (THE ONLY LOSSY STEP): Y = R + 2 G + B of the 5-bit fields, T the
 *          sum of the four Y, a pixel is high when 4 Y > T, the last pixel's group is the pixels on its side of that test; S is the
 *          per-channel floor((sum + n / 2) / n) over that group (n / 2 in integers), F the same over the other group (F = S when it
 *          is empty); bits are set for the other group.
 *   FRAMES  Key(P) = the codes of blocks 0 .. nblocks-1; no skip word, no end marker.  Inter(Q, P): block i is CODED when v of P differs
 *       from v of Q in at least one of its 16 pixels (quantised values are compared, not words); the frame is Delta's rule above with
 *       "written" read as "coded": the run-head test, the count, never crossing a multiple of 1023, ceil(nblocks / 1023) skip words
 *       when nothing changed.
 *   PROMISED, D(P) being the decode of Key(P): jsp_is_key_frame(Key(P)) says yes; D(P) == P on every covered pixel when every word of P
 *       is fromRGB15 of something and every quadrant has at most two colours — every picture an MSVideo1 16-bit decoder produced;
 *       D(D(P)) == D(P) always; Key(P0), Inter(P0, P1), Inter(P1, P2), ... decoded in sequence give exactly D(Pt) at every t (equal
 *       quantised blocks encode alike, so a skip loses nothing); len(Inter) <= len(Key); Inter(Q, P) == Key(P) when every block is
 *       coded; the bytes do not depend on pitch sign, alignment, slice size, or which pictures share a call.  NOT promised: that the
 *       bytes equal what any other encoder, or the original stream, holds.
 *   jsp_msv1_encoder_create: an encoder for pictures of width x height on a device; it owns its scratch (per picture of a slice 24 bytes
 *       per block, 8 per workgroup, the frame at its bound; allocated by the first call).  NULL and jsp_last_error() for a width or
 *       height below 4 or above 16384, or a device that is not there.  jsp_msv1_encode_bound: nblocks * 18, the most bytes of a frame.
 *   jsp_msv1_encode_frames: n pictures, n in 1 .. 4096; pictures[j] and previous[j] are DEVICE pointers (the two arrays themselves are
 *       host memory), all of one pitch; `previous` may be null, or hold null entries: a null entry means a key frame, else frame j =
 *       Inter(previous[j], pictures[j]).  The frames lie back to back in `out`, HOST memory.  lens[j] and *total are set also when
 *       `cap` is smaller than *total — that is then an error with nothing written, as Delta (`out` may be null when cap is 0); they
 *       are zeros after every other error.  The pictures are only read.
 *   TWO kernel launches for a slice of pictures, grid.y = the picture, in the shape of KeyFrame's (msv1_encode_sizes_kernel: a block's
 *       words 16 bytes a row when every base is 16-byte aligned and pitch % 4 == 0, else word by word; the classification, the code
 *       kept in scratch, the run-head test, a scan inside each workgroup of 1024 blocks; msv1_encode_gather_kernel: the totals before
 *       its own summed, the codes and skip words through an LDS image, out in 16-byte pieces) — no workgroup waits for another and
 *       nothing is atomic on global memory.  A call runs in slices of at most 16 pictures (fewer for large pictures) so that the
 *       scratch stays bounded: a sizes launch per slice first, then sizes and gather per slice (a single slice: the gather alone).
 *       Runs on `hip_stream` and returns synchronised.  No codec is involved and no frame buffer is written.
 *   ERRORS, each before anything is queued (jsp_last_error() starts with "msv1_encode:"): a null argument, |pitch| < width, n outside
 *       1 .. 4096, a null entry of pictures[]. */
typedef struct jsp_encoder jsp_encoder;
jsp_encoder* jsp_msv1_encoder_create(int device_id, int width, int height);
void jsp_msv1_encoder_destroy(jsp_encoder* e);
int jsp_msv1_encode_bound(const jsp_encoder* e, size_t* bytes);
int jsp_msv1_encode_frames(jsp_encoder* e, int n, const int32_t* const* pictures, const int32_t* const* previous, ptrdiff_t pitch,
                           uint8_t* out, size_t cap, size_t* lens, size_t* total, void* hip_stream);

/* ---- what sits right after the codec in the reference's Manager, on the GPU --------------- */

/* Manager.fill_bitmap_data (Manager.hx:325-390): RGB32 frame -> canvas pixels.  Modes: */
enum {
    JSP_DISPLAY_CANVAS = 0,        /* 0xFF000000 | B<<16 | G<<8 | R              (Manager.hx:379) */
    JSP_DISPLAY_CANVAS_RGB15 = 1,  /* 0xFF000000 | c << 3  (ScreenPressor 16 bpp)  (Manager.hx:370) */
    JSP_DISPLAY_SETPIXELS = 2,     /* 0xFF000000 | c                               (Manager.hx:351) */
    JSP_DISPLAY_SETPIXELS_RGB15 = 3 /* c << 11                                     (Manager.hx:340) */
};
/* `frame`, `out`: device pointers, width*height ints.  flip_rows != 0 also undoes the bottom-up row
 * order (the reference leaves that to its display matrix, Main.hx:318).  Asynchronous on `hip_stream`.
 *   ARGUMENTS: width and height 1 .. 65535 (height is the launch's grid y; 65535 is the limit HIP documents for it, taken from the
 *     documentation and not measured).  Neither pointer needs alignment: a width divisible by 4 with both pointers on 16-byte
 *     boundaries gets 16-byte loads and stores.  Only the width*height ints of `out` are written.  out == frame (conversion in
 *     place) is allowed without flip_rows; any other overlap of the two buffers is the caller's error.
 *   ERRORS (JSP_ERROR_OCCURED, jsp_last_error() starts with "display_convert:", nothing queued, nothing written): a null pointer, a
 *     width or height outside its bounds, an unknown mode. */
int jsp_display_convert(const int32_t* frame, int32_t* out, int width, int height, int mode, int flip_rows,
                        void* hip_stream);

/* ---- a frame in a window: zoom, scroll and fit (Main.on_stage_resize, Main.hx:288-319) ------ */

/* The reference never shows its bitmap one-to-one: it draws it through the display matrix
 *     screen (sx, sy) = (k x - dx, -k y + win_h + dy)                                   (Main.hx:318)
 * with bitmap.smoothing = true (Main.hx:948), and leaves the resampling to the browser.  The two calls below are that step:
 * jsp_view_matrix is Main's view geometry, jsp_display_present turns a frame buffer into the canvas pixels of a window of any size in
 * ONE kernel launch — the conversion of jsp_display_convert, the row flip, the crop and the resampling fused; no full-size converted
 * frame is written anywhere. */
enum {
    JSP_PRESENT_NEAREST = 0, JSP_PRESENT_BILINEAR = 1,        /* bitmap.smoothing false / true (Main.hx:948) */
    JSP_PRESENT_AREA = 2   /* the area average, for the layers above: jsp_display_present does NOT take it (it refuses every filter but
                            * 0 and 1) — jsp_display_present_area is the call */
};

/* Main.hx:301-315 in doubles; pure host arithmetic, no device needed.
 *   zoom == 0 ("Fit"): *k = min(win_w / frame_w, win_h / frame_h), *dx = *dy = 0.
 *   zoom > 0 (Main's table holds 1 and 2; any positive factor is taken): *k = zoom,
 *       *dx = fit(frame_w * k * hor_view_pos - win_w / 2, 0, frame_w * k - win_w)
 *       *dy = fit(frame_h * k * (1 - ver_view_pos) - win_h / 2, 0, frame_h * k - win_h)
 *     fit(a, mn, mx): if a < mn return mn; if a > mx return mx; return a   (Main.hx:282-286) — kept with its quirk: a zoomed picture
 *     narrower than the window makes mx negative, and a view position past the middle then gives a negative dx, which pushes the
 *     picture to the window's right edge.  win_w / 2 is a real division: an odd window gives a half-pixel offset.
 *   Returns 0, or JSP_ERROR_OCCURED (jsp_last_error() starts with "view_matrix:", nothing written) for a non-positive size, a null
 *   output, a negative or non-finite zoom or view position. */
int jsp_view_matrix(int frame_w, int frame_h, int win_w, int win_h, double zoom,
                    double hor_view_pos, double ver_view_pos, double* k, double* dx, double* dy);

/* Writes the win_w x win_h window, top row first, into `out` (row pitch `out_pitch` ints, out_pitch >= win_w).  `frame` is a frame
 * buffer as the codecs leave it (bottom-up rows, stride frame_w; bitmap row y = buffer row y).  ONE kernel launch on `hip_stream`,
 * asynchronous, as jsp_display_convert.
 *   THE RULE, in integers (the reference's resampler is the browser's; this one is pinned so that a test can ask for bit equality):
 *     F(v) = floor(v * 65536.0 + 0.5) in double precision;  step = F(1.0 / k), ax = F((0.5 + dx) / k), ay = F((win_h + dy - 0.5) / k).
 *     Output pixel (ox, oy): X = ax + ox * step, Y = ay - oy * step in 64-bit integers — the 16.16 bitmap coordinates of its centre.
 *     It shows the picture when 0 <= X < frame_w * 65536 and 0 <= Y < frame_h * 65536; otherwise it is `background`, as given.
 *     Every source pixel a tap reads is first converted by `mode` (the four JSP_DISPLAY_* conversions, bit for bit).
 *     JSP_PRESENT_NEAREST: the converted pixel at (X >> 16, Y >> 16).
 *     JSP_PRESENT_BILINEAR: U = X - 32768, V = Y - 32768; x0 = U >> 16, y0 = V >> 16 (arithmetic shifts); wx = (U & 0xFFFF) >> 8,
 *       wy = (V & 0xFFFF) >> 8; taps x0, x0 + 1, y0, y0 + 1, each clamped into the picture; each of the four bytes of the converted
 *       words on its own:  (p00 (256-wx)(256-wy) + p10 wx (256-wy) + p01 (256-wx) wy + p11 wx wy + 32768) >> 16.
 *     Hence at k = 1 with integral dx, dy both filters give the same plain crop.
 *   ARGUMENTS: `frame`, `out` device pointers; `out` holds (win_h - 1) * out_pitch + win_w ints, does not overlap `frame` and needs no
 *     alignment (rows that start on 16-byte boundaries get 16-byte stores).  Only the window's pixels are written: pitch padding and
 *     memory behind the window are not.  Sizes 1 .. 16384, 1/64 <= k <= 64.
 *   ERRORS (JSP_ERROR_OCCURED, jsp_last_error() starts with "display_present:", nothing queued, nothing written): a null pointer, a
 *     size or k outside its bounds, a non-finite k, dx or dy, out_pitch < win_w, an unknown mode or filter. */
int jsp_display_present(const int32_t* frame, int frame_w, int frame_h,
                        int32_t* out, int win_w, int win_h, size_t out_pitch,
                        double k, double dx, double dy, int mode, int filter,
                        uint32_t background, void* hip_stream);

/* The same window, area-averaged: what "Fit" of a large picture into a small window needs (k = 1/3 samples four source pixels out of
 * nine with the two filters above; a browser's compositor averages when it minifies).  Same contract as jsp_display_present in
 * everything except the filter, which it does not take: ONE kernel launch on `hip_stream`, asynchronous, no full-size intermediate.
 *   THE RULE, in integers:
 *     Geometry: F, step, ax, ay, X = ax + ox * step, Y = ay - oy * step exactly as above (the same +-2^62 hold).  An output pixel
 *       shows the picture under the SAME condition — its centre lies inside: 0 <= X < frame_w * 65536 and 0 <= Y < frame_h * 65536 —
 *       and is `background` otherwise: the three filters agree on which pixels are picture.
 *     Footprint, per axis, in 1/256 source pixels: s = step >> 8 (4 .. 16384).  Columns: c = X >> 8, lo = c - (s >> 1), hi = lo + s,
 *       clipped to the picture: lo' = max(lo, 0), hi' = min(hi, frame_w * 256) (a covered pixel has hi' > lo').  Source column x has
 *       the weight wx(x) = max(0, min(hi', (x + 1) * 256) - max(lo', x * 256)), and Wx = hi' - lo'.  Rows likewise from Y and frame_h
 *       (wy, Wy); bitmap row y = buffer row y.
 *     Average: every source pixel is first converted by `mode` (the four JSP_DISPLAY_* conversions, bit for bit); each of the four
 *       bytes of the converted words on its own:  S = sum_y wy(y) * sum_x wx(x) * p(x, y),  D = Wx * Wy,
 *       result = floor((S + (D >> 1)) / D).  (Wx, Wy <= 16384, D <= 2^28, S < 2^36: S needs more than 32 bits below k of about 1/16,
 *       and the quotient is exact.)
 *     Hence: at k = 1 with integral dx, dy the footprint is exactly one pixel — the plain crop of the other two filters; at k = 1/n
 *     with dx = dy = 0 it is the n x n box mean with halves rounded up, (sum + n*n/2) / (n*n), the rounding of the filmstrip calls;
 *     the alpha byte 0xFF of the canvas modes stays 0xFF.  The rule holds for every k in bounds; for k > 1 it is a box under one
 *     pixel wide — legal and pinned, not the recommended use.
 *   ARGUMENTS: `frame`, `out` device pointers; `out` holds (win_h - 1) * out_pitch + win_w ints, does not overlap `frame` and needs no
 *     alignment (rows that start on 16-byte boundaries get 16-byte stores).  Only the window's pixels are written: pitch padding and
 *     memory behind the window are not.  Sizes 1 .. 16384, 1/64 <= k <= 64.
 *   ERRORS (JSP_ERROR_OCCURED, jsp_last_error() starts with "display_present_area:", nothing queued, nothing written): a null
 *     pointer, a size or k outside its bounds, a non-finite k, dx or dy, out_pitch < win_w, an unknown mode. */
int jsp_display_present_area(const int32_t* frame, int frame_w, int frame_h,
                             int32_t* out, int win_w, int win_h, size_t out_pitch,
                             double k, double dx, double dy, int mode,
                             uint32_t background, void* hip_stream);

/* The pixel loop of frames_differ_significantly (Manager.hx:413-419): *differ = any a[i] != b[i] for
 * first_pixel <= i < npixels.  Device pointers; synchronous. */
int jsp_frames_differ(const int32_t* a, const int32_t* b, size_t first_pixel, size_t npixels, int* differ,
                      void* hip_stream);

/* ---- streams sharded one per GPU inside ONE process (the caller side of Manager.hx:97-142: a Manager and a decoder per
 * stream).  Streams are independent — a codec instance, its previous-frame chain and its entropy models each — so stream i simply
 * lives on devices[i mod ndev] (jsp_codec_create / jsp_pool_create take the device; every call activates its codec's device), one
 * host thread per stream, and no frame ever crosses xGMI.  The one collective is the sum of the per-device counters. */
int jsp_device_count(void);                                             /* HIP devices visible to the process (0: none) */
int jsp_assign_stream(int stream_index, const int* devices, int ndev);  /* devices[stream_index mod ndev]; -1 on bad arguments */
/* per_device = ndev pairs (frames, pixels), entry i belonging to devices[i]; total[0..1] = their sums.  When librccl can be loaded
 * the sums are ALSO computed on the GPUs — one RCCL communicator per distinct device, ncclAllReduce(ncclSum) of the two counters
 * over xGMI — and must agree with the host's (*via_rccl = 1; a mismatch is JSP_ERROR_OCCURED); without RCCL, or when it declines
 * (jsp_shard_last_error says why), *via_rccl = 0 and the host's sums stand.  Returns JSP_ZERO_STATE or JSP_ERROR_OCCURED. */
int jsp_reduce_counters(const int* devices, int ndev, const uint64_t* per_device, uint64_t* total, int* via_rccl);
const char* jsp_shard_last_error(void);

/* Library/build identification: "jsplayer_amd <version> gfx950". */
const char* jsp_version(void);

#ifdef __cplusplus
}
#endif
#endif /* JSPLAYER_AMD_H */
