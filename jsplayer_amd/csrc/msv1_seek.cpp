// The MSVideo1 range calls of include/jsplayer_amd.h — jsp_seek, jsp_find_change and jsp_index_* — and what they share: the chunks a
// range is staged in (the codec's own staging, host or on-GPU parse), the refusals, the significance rules and the change scan.
//
// Kept apart from jsp_api.cpp / msv1_codec.cpp: those are also built against the stub HIP runtime of the host-layer sanitizer
// build (tools/tsan_cpu.sh), which knows nothing of the seek kernels.
#include <algorithm>
#include <cstring>

#include "codec.h"
#include "msv1_index_clip_layout.h"
#include "msv1_index_crop_layout.h"
#include "msv1_index_pan_layout.h"
#include "msv1_index_path_layout.h"
#include "msv1_seek.h"

using namespace jsp;

struct jsp_index {
    uint64_t codec_serial = 0;       // jsp_codec::serial of the codec that built it
    int device = 0;
    Msv1Geometry geo{};
    int nframes = 0;
    struct Chunk {
        DeviceBuffer stream, desc, frames;
        int first = 0, count = 0;
    };
    std::vector<std::unique_ptr<Chunk>> chunks;
    DeviceBuffer d_chunks, d_frame_chunk, d_bitmap, d_palette, d_before;   // (d_before: nothing when there is no picture before the index)
    Msv1IndexSrc src{};                    // what the index kernels read of all that: filled when the build ends (index_src)
    std::vector<int> significance;         // per frame: jsp_find_change's verdict (1 / 0)
    std::vector<uint8_t> reported;         // per frame: what jsp_seek of frames 0..t reports as *significant_changes
    std::vector<uint8_t> block_changes;    // nframes rows of nby flags: the per-row state after frame t
    int first_adopted = 0;                 // the first frame that adopts its destination (nframes: none)
    int32_t* prev_caller = nullptr;        // the codec's previous frame at build time (what a show before first_adopted leaves)
    int32_t* prev_dev = nullptr;
    PinnedBuffer h_frame_list;             // jsp_index_thumbs / _present / _tensor: the call's frame list on its way to ...
    DeviceBuffer d_frame_list;             // ... the array the kernel reads (both grown on demand)
    PinnedBuffer h_play_dsts;              // jsp_index_play: the call's destinations on their way to ...
    DeviceBuffer d_play_dsts;              // ... the array the kernel reads (both grown on demand; nothing until the first call)
    DeviceBuffer d_key_frame;              // jsp_index_key_frame: status, workgroup totals, block records, the frame at its bound ...
    PinnedBuffer h_key_frame;              // ... and where the status, the length and a refused block's record arrive (both: first call)
    DeviceBuffer d_delta;                  // jsp_index_delta_frames: one slice of pairs — their list, statuses, totals, records, frames ...
    PinnedBuffer h_delta;                  // ... and the host's side of the list, the statuses and the totals (both: first call)
    DeviceBuffer d_crop;                   // jsp_index_crop_frames, jsp_index_path_frames: the same for a slice of pairs of a rectangle ...
    PinnedBuffer h_crop;                   // ... and the host's side of it (both: first call)
    DeviceBuffer d_pan;                    // jsp_index_pan_frames: the same with the pairs' origins in front (clip_layout) ...
    PinnedBuffer h_pan;                    // ... and the host's side of it (both: first call)
    uint64_t device_bytes() const {
        uint64_t n = d_chunks.cap + d_frame_chunk.cap + d_bitmap.cap + d_palette.cap + d_before.cap + d_frame_list.cap + d_play_dsts.cap +
                     d_key_frame.cap + d_delta.cap + d_crop.cap + d_pan.cap;
        for (const auto& c : chunks) n += c->stream.cap + c->desc.cap + c->frames.cap;
        return n;
    }
    uint64_t host_bytes() const {
        return sizeof(*this) + chunks.size() * sizeof(Chunk) + significance.size() * sizeof(int) + reported.size() + block_changes.size() +
               h_frame_list.cap + h_play_dsts.cap + h_key_frame.cap + h_delta.cap + h_crop.cap + h_pan.cap;
    }
};

namespace {

// Frames per chunk when the caller leaves it to the library: what the staged range holds in HBM (stream bytes in 16 KiB tiles,
// 4 bytes per block of table) and in pinned host memory stays under this budget.
constexpr uint64_t kChunkBudget = 1ull << 30;

int fail(const char* fmt, const char* what = "") {
    set_error(fmt, what);
    return JSP_ERROR_OCCURED;
}

bool same_bytes(const uint8_t* a, size_t na, const uint8_t* b, size_t nb) {
    return na == nb && (na == 0 || std::memcmp(a, b, na) == 0);
}

// The caller's range: frame k is srcs[k], lens[k] bytes, a key frame unless is_key[k] == 0 (no is_key: every frame is one).
// key_before: the bytes of the key frame before the range, if it is one (jsp_find_change; null: there is none).
struct Range {
    const uint8_t* const* srcs;
    const size_t* lens;
    const uint8_t* is_key;
    const uint8_t* key_before = nullptr;
    size_t key_before_len = 0;
    bool key(int k) const { return is_key ? is_key[k] != 0 : true; }
};

bool null_frame(int nframes, const uint8_t* const* srcs, const size_t* lens) {
    for (int i = 0; i < nframes; ++i)
        if (!srcs[i] && lens[i]) return true;
    return false;
}

// ---- refusals: one function each, so that every entry point keeps its order (and so its message for an input refused on several
// counts).  False: refused, the error "<who>: <what>" is set. ------------------------------------------------------------------
bool refuse(const char* who, const char* what) {
    set_error("%s: %s", who, what);
    return false;
}
bool is_msv1(const jsp_codec* c, const char* who) {
    return c->kind == JSP_CODEC_MSVIDEO1_16 || c->kind == JSP_CODEC_MSVIDEO1_8 || refuse(who, "MSVideo1 only");
}
bool nothing_in_flight(const jsp_codec* c, const char* who) {
    return c->next_ticket == c->oldest_ticket || refuse(who, "an asynchronous frame is in flight (jsp_wait for it first)");
}
bool dst_not_previous(const jsp_codec* c, const int32_t* dst, const char* who) {
    return dst != c->prev_caller || refuse(who, "dst is the current previous frame");
}
bool on_device(const void* p, const char* who, const char* what) {   // (after c->activate())
    hipPointerAttribute_t attr{};
    if (hipPointerGetAttributes(&attr, p) == hipSuccess && (attr.type == hipMemoryTypeDevice || attr.type == hipMemoryTypeManaged)) return true;
    (void)hipGetLastError();
    return refuse(who, what);
}
bool dst_on_device(const int32_t* dst, const char* who) { return on_device(dst, who, "dst must be a device frame buffer"); }
bool device_pointers(const jsp_codec* c, const char* who) { return c->ptr_mode != 2 || refuse(who, "codec is in host-pointer mode"); }

// A call that leaves the codec where a sequential decode into `dst` would: the worker's frames finished, device pointers from now
// on, and no key-frame compare to report (it does not run on these calls).
void take_over(jsp_codec* c) {
    c->worker_drain();
    c->ptr_mode = 1;
    c->last_key_differs = -1;
}

// ---- chunks ----------------------------------------------------------------------------------------------------------------
// The end of the chunk that starts at frame a: option "msv1_seek_chunk_frames" frames, else as many as kChunkBudget holds (one at least).
int chunk_end(const jsp_codec* c, const size_t* lens, int nframes, int a) {
    if (c->seek_chunk_frames > 0) return std::min(nframes, a + c->seek_chunk_frames);
    const uint64_t table_bytes = 4ull * (uint64_t)std::max((int64_t)c->X / 4 * (c->Y / 4), (int64_t)1);
    int b = a + 1;
    uint64_t bytes = lens[a] + table_bytes;
    while (b < nframes && bytes + lens[b] + 16384 + table_bytes <= kChunkBudget) bytes += lens[b++] + 16384 + table_bytes;
    return b;
}

// Frames [a, b) of the range staged into `into` (reused, or replaced by the staging object the codec returns), every frame's
// destination `dst`.  The codec's host state advances to frame b - 1.
jsp_staged* stage(jsp_codec* c, const Range& r, int a, int b, std::unique_ptr<jsp_staged>& into, int32_t* dst) {
    std::vector<jsp_frame_in> frames((size_t)(b - a));
    for (int i = a; i < b; ++i) frames[(size_t)(i - a)] = jsp_frame_in{r.srcs[i], r.lens[i], r.key(i), dst};
    jsp_staged* st = c->stage(frames, into.get());
    st->device = c->device;
    if (st != into.get()) into.reset(st);
    return st;
}

// The first frame of a staged chunk of nf frames that the reference raises on (-1: none): nothing at or past it is reached.
int first_error(const jsp_staged* st, int nf) {
    for (int i = 0; i < nf; ++i)
        if (st->status[(size_t)i] != JSP_ZERO_STATE) return i;
    return -1;
}

void range_error(const char* who, int k, const jsp_staged* st) {
    set_error("%s: frame %d of the range: %s", who, k, st->why.empty() ? "the reference raises on this stream" : st->why.c_str());
}

// jsp_seek / jsp_find_change: the reference raises out of frame k, and what the caller had as its previous frame is gone with the range.
int raised(jsp_codec* c, const char* who, int k, const jsp_staged* st) {
    c->prev_dev = nullptr;
    c->prev_caller = nullptr;
    range_error(who, k, st);
    return JSP_ERROR_OCCURED;
}

bool adopts(const jsp_staged* st) { return std::any_of(st->adopted.begin(), st->adopted.end(), [](int ad) { return ad != 0; }); }

// ---- significance ------------------------------------------------------------------------------------------------------------
// Frame k of the range (frame i of the staged chunk st / v): 1 / 0 where the host stage settles it, else -1 with `row` set to the
// pixel row the compare starts from.  Key frames by frames_differ_significantly (Manager.hx:392-421): after a key frame by their
// bytes, else significant with no picture before them, else the pixel compare from key_row.  Inter frames as DecompressP: stage 1
// on the host, stage 2 (st->significant == -1) from insign_lines on.
int settle(const Range& r, int k, int i, const jsp_staged* st, const Msv1SeekView& v, int key_row, uint32_t& row) {
    if (r.key(k)) {
        const bool key_prev = k > 0 ? r.key(k - 1) : r.key_before != nullptr;
        if (key_prev)
            return k > 0 ? !same_bytes(r.srcs[k - 1], r.lens[k - 1], r.srcs[k], r.lens[k]) : !same_bytes(r.key_before, r.key_before_len, r.srcs[k], r.lens[k]);
        if (!v.h_frames[i].prev) return 1;
        row = (uint32_t)key_row;
        return -1;
    }
    const int s = st->significant[(size_t)i];
    if (s >= 0) return s;
    row = v.h_frames[i].cmp_row_lo;
    return -1;
}

// A chunk's judgement lives in the caller's scratch, host `h` and device `d` alike laid out as [first-hit word, with stop_at_hit]
// [rows: one per frame of the chunk][walk list].  judge_rows: room for a chunk of nf frames, every row ~0u (not judged); the rows.
uint32_t* judge_rows(PinnedBuffer& h, int nf, bool stop_at_hit) {
    h.reserve(sizeof(uint32_t) * ((stop_at_hit ? 1 : 0) + 2 * (size_t)nf));
    uint32_t* rows = static_cast<uint32_t*>(h.p) + (stop_at_hit ? 1 : 0);
    std::fill(rows, rows + nf, 0xFFFFFFFFu);
    return rows;
}

// ONE launch of msv1_change_scan_kernel judges the chunk's frames that have a row, against `before` (the picture before the chunk),
// and v.d_signif comes back to v.h_signif — queued on the codec's stream, not waited for.  The walk list: the frames up to judged_last
// that code a block (early-outs and all-skip frames code none).  stop_at_hit: the scan stops at the first frame found to differ
// (jsp_find_change); else every frame with a row is judged (jsp_index_build).
void judge_chunk(jsp_codec* c, const jsp_staged* st, const Msv1SeekView& v, int judged_last, bool stop_at_hit, PinnedBuffer& h,
                 DeviceBuffer& d, const int32_t* before) {
    const int nf = v.nframes, head = stop_at_hit ? 1 : 0;
    uint32_t* h_first = static_cast<uint32_t*>(h.p);
    uint32_t* h_walk = h_first + head + nf;
    int nwalk = 0;
    for (int i = 0; i <= judged_last; ++i)
        if (st->adopted[(size_t)i]) h_walk[nwalk++] = (uint32_t)i;
    if (stop_at_hit) *h_first = 0xFFFFFFFFu;
    const size_t words = (size_t)head + (size_t)nf + (size_t)nwalk;
    d.reserve(sizeof(uint32_t) * words);
    uint32_t* d_first = static_cast<uint32_t*>(d.p);
    JSP_HIP(hipMemcpyAsync(d_first, h_first, sizeof(uint32_t) * words, hipMemcpyHostToDevice, c->stream));
    JSP_HIP(hipMemsetAsync(v.d_signif, 0, sizeof(uint32_t) * (size_t)nf, c->stream));
    msv1_launch_change_scan(v, d_first + head + nf, nwalk, d_first + head, stop_at_hit ? d_first : nullptr, before, c->stream);
    JSP_HIP(hipGetLastError());
    JSP_HIP(hipMemcpyAsync(v.h_signif, v.d_signif, sizeof(uint32_t) * (size_t)nf, hipMemcpyDeviceToHost, c->stream));
}

// What the index kernels read of a built index (Msv1IndexSrc, msv1_seek.h), with the clamps a picture without a block needs.
Msv1IndexSrc index_src(const jsp_index& idx) {
    const Msv1Geometry& geo = idx.geo;
    Msv1IndexSrc s{};
    s.chunks = idx.d_chunks.as<const Msv1IndexChunk>();
    s.frame_chunk = idx.d_frame_chunk.as<const uint32_t>();
    s.palette = idx.d_palette.as<const int32_t>();
    s.bitmap = idx.d_bitmap.as<const uint32_t>();
    s.before = idx.d_before.as<const uint32_t>();
    s.pitch = (size_t)std::max(geo.nblocks, 1);
    s.nblocks = std::max(geo.nblocks, 0);
    s.nbx = std::max(geo.nbx, 0);
    s.nby = std::max(geo.nby, 0);
    s.X = geo.X;
    s.Y = geo.Y;
    s.bits = geo.bits;
    s.before_vec = (geo.X & 3) == 0 && !(reinterpret_cast<uintptr_t>(s.before) & 15);
    return s;
}

}  // namespace

// ---- jsp_seek: the seek branch of Manager.GetDecompressedFrame (Manager.hx:216-259) — frames K..N staged as one batch and composed
// into the caller's buffer by ONE launch of msv1_seek_kernel, instead of N - K + 1 decodes each writing a whole frame. --------------
extern "C" int jsp_seek(jsp_codec* c, int nframes, const uint8_t* const* srcs, const size_t* lens, const uint8_t* is_key, int32_t* dst,
                        int32_t** data_pnt, int* significant_changes) {
    if (data_pnt) *data_pnt = c ? c->prev_caller : nullptr;
    if (significant_changes) *significant_changes = 0;
    if (!c || nframes <= 0 || !srcs || !lens || !dst) return fail("seek: null argument or empty range");
    if (null_frame(nframes, srcs, lens)) return fail("seek: null frame bytes");
    if (!is_msv1(c, "seek") || !nothing_in_flight(c, "seek") || !dst_not_previous(c, dst, "seek")) return JSP_ERROR_OCCURED;
    try {
        c->activate();
        if (!dst_on_device(dst, "seek") || !device_pointers(c, "seek")) return JSP_ERROR_OCCURED;
        take_over(c);

        const Range range{srcs, lens, is_key};
        int sig = 0, last_sig_word = -1;
        bool any_adopted = false;
        uint32_t* h_word = nullptr;
        for (int a = 0, b = 0; a < nframes; a = b) {
            b = chunk_end(c, lens, nframes, a);
            // (the chunk before may still be composing from the batch buffers that staging refills)
            if (a > 0) JSP_HIP(hipStreamSynchronize(c->stream));
            const int32_t* base = c->prev_dev;   // the picture before this chunk (null: there is none; dst: the chunks before wrote it)
            jsp_staged* st = stage(c, range, a, b, c->seek_scratch, dst);
            if (const int err = first_error(st, b - a); err >= 0) return raised(c, "seek", a + err, st);
            Msv1SeekView v;
            if (!msv1_seek_view(st, v)) throw std::runtime_error("seek: not an MSVideo1 batch");
            const bool chunk_adopted = adopts(st);
            const bool last = b == nframes;
            const int lf = b - a - 1;
            uint32_t cmp_row_lo = 0xFFFFFFFFu;
            if (last) {
                sig = st->significant[(size_t)lf];
                if (sig < 0) { cmp_row_lo = v.h_frames[lf].cmp_row_lo; sig = 0; last_sig_word = lf; h_word = v.h_signif + lf; }
            }
            if (chunk_adopted) {
                if (cmp_row_lo != 0xFFFFFFFFu) JSP_HIP(hipMemsetAsync(v.d_signif + lf, 0, sizeof(uint32_t), c->stream));
                msv1_launch_seek(v, dst, base == dst ? nullptr : base, cmp_row_lo, c->stream);
                JSP_HIP(hipGetLastError());
                if (cmp_row_lo != 0xFFFFFFFFu)
                    JSP_HIP(hipMemcpyAsync(h_word, v.d_signif + lf, sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
            }
            any_adopted |= chunk_adopted;
        }
        JSP_HIP(hipStreamSynchronize(c->stream));
        if (last_sig_word >= 0) sig = *h_word ? 1 : 0;
        if (any_adopted) c->prev_caller = dst;
        if (data_pnt) *data_pnt = c->prev_caller;
        if (significant_changes) *significant_changes = sig;
        return JSP_ZERO_STATE;
    } catch (const std::exception& e) {
        set_error("%s", e.what());
        return JSP_ERROR_OCCURED;
    }
}

// ---- jsp_find_change: Manager.SkipStills (Manager.hx:289-317) over DataLoader.FindPossibleChange (DataLoader.hx:239-252) — which
// frame after the one shown is the first to change the picture significantly, and that frame's picture, without decoding and writing
// every idle frame in between.  Per chunk: ONE launch of msv1_change_scan_kernel for the frames whose significance needs a pixel
// compare, then ONE launch of msv1_seek_kernel composing the picture up to the hit (or the whole chunk, which becomes the next
// chunk's picture before). ---------------------------------------------------------------------------------------------------
extern "C" int jsp_find_change(jsp_codec* c, int nframes, const uint8_t* const* srcs, const size_t* lens, const uint8_t* is_key, int first,
                               const uint8_t* key_before, size_t key_before_len, int key_row, int32_t* dst, int* found, int* changed,
                               int* significance, int32_t** data_pnt) {
    if (data_pnt) *data_pnt = c ? c->prev_caller : nullptr;
    if (found) *found = -1;
    if (changed) *changed = 0;
    if (significance)
        for (int i = 0; i < nframes; ++i) significance[i] = -1;
    if (!c || nframes <= 0 || !srcs || !lens || !dst || !found || !changed) return fail("find_change: null argument or empty range");
    if (null_frame(nframes, srcs, lens)) return fail("find_change: null frame bytes");
    if (first < 0 || first >= nframes) return fail("find_change: first is outside the range");
    if (key_row < 0) return fail("find_change: negative key_row");
    if (!is_msv1(c, "find_change") || !nothing_in_flight(c, "find_change") || !dst_not_previous(c, dst, "find_change")) return JSP_ERROR_OCCURED;
    try {
        c->activate();
        if (!dst_on_device(dst, "find_change") || !device_pointers(c, "find_change")) return JSP_ERROR_OCCURED;
        take_over(c);

        const Range range{srcs, lens, is_key, key_before, key_before_len};
        int hit = -1;               // the frame found (range index)
        bool any_adopted = false;
        for (int a = 0, b = 0; a < nframes && hit < 0; a = b) {
            b = chunk_end(c, lens, nframes, a);
            if (a > 0) JSP_HIP(hipStreamSynchronize(c->stream));   // (the chunk before may still be composing from the batch buffers)
            const int32_t* base = c->prev_dev;   // the picture before this chunk (null: there is none; dst: the chunks before wrote it)
            Msv1HostState saved;
            if (!msv1_save_state(c, saved)) throw std::runtime_error("find_change: not an MSVideo1 codec");
            jsp_staged* st = stage(c, range, a, b, c->seek_scratch, dst);
            const int nf = b - a;
            const int err = first_error(st, nf);
            Msv1SeekView v;
            if (!msv1_seek_view(st, v)) throw std::runtime_error("find_change: not an MSVideo1 batch");

            // from `first` on, up to the first frame the host already knows to be significant (nothing after it is judged)
            const int lo = std::max(first - a, 0), limit = err >= 0 ? err : nf;
            std::vector<int> sig((size_t)nf, -1);
            uint32_t* h_rows = judge_rows(c->find_host, nf, true);
            int judged_last = -1;
            for (int i = lo; i < limit; ++i) {
                const int s = sig[(size_t)i] = settle(range, a + i, i, st, v, key_row, h_rows[i]);
                if (s == 1) break;
                if (s < 0) judged_last = i;
            }
            if (judged_last >= 0) {
                judge_chunk(c, st, v, judged_last, true, c->find_host, c->find_dev, base ? base : dst);
                JSP_HIP(hipStreamSynchronize(c->stream));
            }
            int local = -1;
            for (int i = lo; i < limit && local < 0; ++i) {
                if (sig[(size_t)i] < 0) sig[(size_t)i] = v.h_signif[i] ? 1 : 0;
                if (significance) significance[a + i] = sig[(size_t)i];
                if (sig[(size_t)i] == 1) local = i;
            }
            if (local < 0 && err >= 0) return raised(c, "find_change", a + err, st);
            if (local >= 0) {
                hit = a + local;
                *changed = 1;
                if (local < nf - 1) {
                    // the staging ran on to the chunk's end: back to where the chunk began, and the prefix up to the hit again, so that
                    // prev_dev and block_changes end at the hit as the per-frame calls would leave them
                    msv1_restore_state(c, saved);
                    st = stage(c, range, a, hit + 1, c->seek_scratch, dst);
                    if (!msv1_seek_view(st, v)) throw std::runtime_error("find_change: not an MSVideo1 batch");
                }
            } else if (b == nframes) {
                hit = nframes - 1;   // nothing changes up to the end: FindPossibleChange lands on the last frame
            }
            const bool chunk_adopted = adopts(st);
            if (chunk_adopted) {
                msv1_launch_seek(v, dst, base == dst ? nullptr : base, 0xFFFFFFFFu, c->stream);
                JSP_HIP(hipGetLastError());
            }
            any_adopted |= chunk_adopted;
        }
        JSP_HIP(hipStreamSynchronize(c->stream));
        if (any_adopted) c->prev_caller = dst;
        if (data_pnt) *data_pnt = c->prev_caller;
        *found = hit;
        return JSP_ZERO_STATE;
    } catch (const std::exception& e) {
        set_error("%s", e.what());
        return JSP_ERROR_OCCURED;
    }
}

// ---- jsp_index_*: a resident MSVideo1 SEEK INDEX — a range's stream bytes, block tables and frame records kept in HBM after one
// staging, so that showing any frame of it is ONE launch of msv1_index_show_kernel with no host work: the scrubbing, previous-frame
// and seek-bar navigation of the reference player (Main.on_prevframe / Manager.PrevFrameTime, Manager.hx:184-208; Main.on_click,
// Main.hx:1197-1215) without restaging the range from its key frame on every step.
//
// Build, per chunk of the range:
//   * the chunk is staged and its device buffers change hands (msv1_take_batch) — the index keeps no staged batch, nothing that
//     refers to the codec's streams;
//   * ONE launch of msv1_change_scan_kernel<.., ALL> judges every frame whose significance needs a pixel compare, against a running
//     picture of the build's own (the picture before the chunk);
//   * ONE launch of msv1_coded_bitmap_kernel adds the chunk's frames to the global coded-block bitmap, the per-row coded words and the
//     first untouched block of each frame — from which the host derives, per frame, the per-row block_changes the sequential calls
//     leave behind (MSVideo1.hx:122,305: a row is reset when a frame reaches it);
//   * ONE launch of msv1_seek_kernel moves the running picture on to the chunk's end (when a chunk follows).
// The codec's host state is saved first and put back at the end: the build changes nothing but the index. ---------------------------
extern "C" jsp_index* jsp_index_build(jsp_codec* c, int nframes, const uint8_t* const* srcs, const size_t* lens, const uint8_t* is_key,
                                      int key_row) {
    if (!c || nframes <= 0 || !srcs || !lens) { fail("index: null argument or empty range"); return nullptr; }
    if (null_frame(nframes, srcs, lens)) { fail("index: null frame bytes"); return nullptr; }
    if (key_row < 0) { fail("index: negative key_row"); return nullptr; }
    if (!is_msv1(c, "index") || !nothing_in_flight(c, "index") || !device_pointers(c, "index")) return nullptr;
    Msv1HostState saved;
    bool restore = false;
    std::unique_ptr<jsp_staged> stg;   // the build's own staging object (its last chunk's leftovers go with it, before the build returns)
    try {
        c->activate();
        c->worker_drain();
        if (!msv1_save_state(c, saved)) throw std::runtime_error("index: not an MSVideo1 codec");
        restore = true;
        auto idx = std::make_unique<jsp_index>();
        idx->codec_serial = c->serial;
        idx->device = c->device;
        idx->nframes = nframes;
        idx->prev_caller = c->prev_caller;
        idx->prev_dev = c->prev_dev;
        idx->significance.assign((size_t)nframes, 0);
        idx->reported.assign((size_t)nframes, 0);
        idx->first_adopted = nframes;
        std::vector<uint8_t> noop((size_t)nframes, 0);
        std::vector<uint8_t> rows_now;   // block_changes at build time, as the next host parse would see them
        if (!msv1_block_changes_now(c, rows_now)) throw std::runtime_error("index: not an MSVideo1 codec");

        const size_t npix = (size_t)c->X * (size_t)c->Y;
        const size_t pic_bytes = sizeof(int32_t) * std::max<size_t>(npix, 1);
        // the running picture: the picture before the chunk being judged (and the staging's stand-in destination — nothing writes
        // it but this build)
        DeviceBuffer d_run;
        d_run.reserve(pic_bytes);
        int32_t* run = static_cast<int32_t*>(d_run.p);
        if (c->prev_dev) {
            idx->d_before.reserve(pic_bytes);
            JSP_HIP(hipMemcpyAsync(idx->d_before.p, c->prev_dev, sizeof(int32_t) * npix, hipMemcpyDeviceToDevice, c->stream));
            JSP_HIP(hipMemcpyAsync(run, c->prev_dev, sizeof(int32_t) * npix, hipMemcpyDeviceToDevice, c->stream));
        } else {
            JSP_HIP(hipMemsetAsync(run, 0, pic_bytes, c->stream));
        }
        const int nwords = (nframes + 31) / 32;
        const int nblocks_all = (c->X / 4) * (c->Y / 4), nby = c->Y / 4;
        idx->d_bitmap.reserve(sizeof(uint32_t) * std::max<size_t>((size_t)nwords * (size_t)nblocks_all, 1));
        JSP_HIP(hipMemsetAsync(idx->d_bitmap.p, 0, sizeof(uint32_t) * (size_t)nwords * (size_t)nblocks_all, c->stream));
        DeviceBuffer d_rows, d_stop, d_work;   // per-row coded words, first untouched block per frame; rows / walk list of a chunk
        d_rows.reserve(sizeof(uint32_t) * std::max<size_t>((size_t)nwords * (size_t)nby, 1));
        d_stop.reserve(sizeof(uint32_t) * (size_t)nframes);
        JSP_HIP(hipMemsetAsync(d_rows.p, 0, sizeof(uint32_t) * (size_t)nwords * (size_t)nby, c->stream));
        JSP_HIP(hipMemsetAsync(d_stop.p, 0xFF, sizeof(uint32_t) * (size_t)nframes, c->stream));
        PinnedBuffer h_work;

        const Range range{srcs, lens, is_key};
        for (int a = 0, b = 0; a < nframes; a = b) {
            b = chunk_end(c, lens, nframes, a);
            const int nf = b - a;
            jsp_staged* st = stage(c, range, a, b, stg, run);
            if (const int err = first_error(st, nf); err >= 0) {
                range_error("index", a + err, st);
                msv1_restore_state(c, saved);
                return nullptr;
            }
            Msv1SeekView v;
            if (!msv1_seek_view(st, v)) throw std::runtime_error("index: not an MSVideo1 batch");
            if (a == 0) {   // the codec's palette (8-bit): the index keeps a copy of its own
                idx->geo = v.geo;
                idx->d_palette.reserve(sizeof(int32_t) * 256);
                if (v.d_palette) JSP_HIP(hipMemcpyAsync(idx->d_palette.p, v.d_palette, sizeof(int32_t) * 256, hipMemcpyDeviceToDevice, c->stream));
                else JSP_HIP(hipMemsetAsync(idx->d_palette.p, 0, sizeof(int32_t) * 256, c->stream));
            }

            // every frame judged (frame 0 of the range: no key frame before it)
            uint32_t* h_rows = judge_rows(h_work, nf, false);
            int judged_last = -1;
            bool chunk_adopted = false;
            for (int i = 0; i < nf; ++i) {
                const int k = a + i;
                const int s = idx->significance[(size_t)k] = settle(range, k, i, st, v, key_row, h_rows[i]);
                if (s < 0) judged_last = i;
                noop[(size_t)k] = (v.h_frames[i].pad & MSV1_FRAME_NOOP) != 0;
                if (st->adopted[(size_t)i]) {
                    chunk_adopted = true;
                    idx->first_adopted = std::min(idx->first_adopted, k);
                }
            }
            if (judged_last >= 0) judge_chunk(c, st, v, judged_last, false, h_work, d_work, run);
            msv1_launch_coded_bitmap(v, a, static_cast<uint32_t*>(idx->d_bitmap.p), static_cast<uint32_t*>(d_rows.p),
                                     static_cast<uint32_t*>(d_stop.p), c->stream);
            JSP_HIP(hipGetLastError());
            if (b < nframes && chunk_adopted) {   // the running picture moves on to the chunk's end: the picture before the next one
                msv1_launch_seek(v, run, nullptr, 0xFFFFFFFFu, c->stream);
                JSP_HIP(hipGetLastError());
            }
            JSP_HIP(hipStreamSynchronize(c->stream));   // (the judged words are read now; the pinned work buffer is reused next chunk)
            for (int i = 0; i < nf; ++i) {
                const int k = a + i;
                if (idx->significance[(size_t)k] < 0) idx->significance[(size_t)k] = v.h_signif[i] ? 1 : 0;
                idx->reported[(size_t)k] = range.key(k) ? 0 : (uint8_t)idx->significance[(size_t)k];   // (DecompressI reports nothing)
            }
            auto ch = std::make_unique<jsp_index::Chunk>();
            ch->first = a;
            ch->count = nf;
            if (!msv1_take_batch(st, ch->stream, ch->desc, ch->frames)) throw std::runtime_error("index: not an MSVideo1 batch");
            idx->chunks.push_back(std::move(ch));
        }
        stg.reset();   // (pinned stream copy, host tables, parse buffers: not needed any more)
        h_work.release();
        d_work.release();

        // ---- per-row block_changes after every frame: a frame resets and sets the rows its walk reaches (all of them, up to the row
        // of its first untouched block; none for an early-out), the rows after that keep what was there ----------------------------
        std::vector<uint32_t> rows((size_t)nwords * (size_t)nby), stop((size_t)nframes);
        if (!rows.empty()) JSP_HIP(hipMemcpy(rows.data(), d_rows.p, sizeof(uint32_t) * rows.size(), hipMemcpyDeviceToHost));
        JSP_HIP(hipMemcpy(stop.data(), d_stop.p, sizeof(uint32_t) * stop.size(), hipMemcpyDeviceToHost));
        const Msv1Geometry& geo = idx->geo;
        idx->block_changes.resize((size_t)nframes * (size_t)nby);
        rows_now.resize((size_t)nby, 0);
        for (int t = 0; t < nframes; ++t) {
            if (!noop[(size_t)t] && geo.nblocks > 0) {
                const int reached = std::min((int)(std::min<uint32_t>(stop[(size_t)t], (uint32_t)geo.nblocks) / (uint32_t)geo.nbx), geo.nby - 1);
                for (int r = 0; r <= reached; ++r) rows_now[(size_t)r] = (uint8_t)((rows[(size_t)(t / 32) * nby + r] >> (t % 32)) & 1u);
            }
            std::copy(rows_now.begin(), rows_now.end(), idx->block_changes.begin() + (size_t)t * (size_t)nby);
        }

        // ---- what the index kernels read: per-chunk pointers, the chunk of every frame, and the record that names it all -------------
        std::vector<Msv1IndexChunk> table;
        std::vector<uint32_t> frame_chunk((size_t)nframes);
        for (size_t k = 0; k < idx->chunks.size(); ++k) {
            const auto& ch = *idx->chunks[k];
            table.push_back(Msv1IndexChunk{static_cast<const uint8_t*>(ch.stream.p), static_cast<const uint32_t*>(ch.desc.p),
                                           static_cast<const Msv1FrameArgs*>(ch.frames.p), (uint32_t)ch.first, 0});
            std::fill(frame_chunk.begin() + ch.first, frame_chunk.begin() + ch.first + ch.count, (uint32_t)k);
        }
        idx->d_chunks.reserve(sizeof(Msv1IndexChunk) * table.size());
        idx->d_frame_chunk.reserve(sizeof(uint32_t) * frame_chunk.size());
        JSP_HIP(hipMemcpy(idx->d_chunks.p, table.data(), sizeof(Msv1IndexChunk) * table.size(), hipMemcpyHostToDevice));
        JSP_HIP(hipMemcpy(idx->d_frame_chunk.p, frame_chunk.data(), sizeof(uint32_t) * frame_chunk.size(), hipMemcpyHostToDevice));
        idx->src = index_src(*idx);
        msv1_restore_state(c, saved);
        return idx.release();
    } catch (const std::exception& e) {
        if (restore) msv1_restore_state(c, saved);
        set_error("%s", e.what());
        return nullptr;
    }
}

// What adopting frame t of the index, shown in `dst`, does to the codec once the picture is written: it ends as jsp_seek of frames
// 0..t leaves it.
namespace {
void adopt_frame(jsp_codec* c, const jsp_index* idx, int t, int32_t* dst) {
    const bool adopted = t >= idx->first_adopted;
    take_over(c);   // (as on a seek)
    const int nby = std::max(idx->geo.nby, 0);
    Msv1HostState s;
    s.prev_dev = adopted ? dst : idx->prev_dev;
    s.block_changes.assign(idx->block_changes.begin() + (size_t)t * (size_t)nby, idx->block_changes.begin() + (size_t)(t + 1) * (size_t)nby);
    msv1_restore_state(c, s);   // (exact per-row flags: nothing stale, nothing that points into the index)
    c->prev_caller = adopted ? dst : idx->prev_caller;
}
}  // namespace

extern "C" int jsp_index_show(jsp_codec* c, jsp_index* idx, int t, int32_t* dst, int adopt, int32_t** data_pnt, int* significant_changes) {
    if (data_pnt) *data_pnt = c ? c->prev_caller : nullptr;
    if (significant_changes) *significant_changes = 0;
    if (!c || !idx || !dst) return fail("index_show: null argument");
    if (!is_msv1(c, "index")) return JSP_ERROR_OCCURED;
    if (idx->codec_serial != c->serial) return fail("index_show: the index was built by another codec");
    if (t < 0 || t >= idx->nframes) return fail("index_show: t is outside the index");
    if (!nothing_in_flight(c, "index_show") || !dst_not_previous(c, dst, "index_show")) return JSP_ERROR_OCCURED;
    try {
        c->activate();
        if (!dst_on_device(dst, "index_show") || !device_pointers(c, "index_show")) return JSP_ERROR_OCCURED;
        const bool adopted = t >= idx->first_adopted;   // jsp_seek of frames 0..t writes dst only then
        if (adopted) {
            msv1_launch_index_show(idx->src, t, dst, c->stream);
            JSP_HIP(hipGetLastError());
            JSP_HIP(hipStreamSynchronize(c->stream));
        }
        int32_t* shown = adopted ? dst : idx->prev_caller;
        if (adopt) adopt_frame(c, idx, t, dst);
        if (data_pnt) *data_pnt = shown;
        if (significant_changes) *significant_changes = idx->reported[(size_t)t];
        return JSP_ZERO_STATE;
    } catch (const std::exception& e) {
        set_error("%s", e.what());
        return JSP_ERROR_OCCURED;
    }
}

// ---- playback: a run of frames of the index, each into a buffer of its own — reverse play and the step-back button held down, xs
// fast-forward, filling the Manager's free buffers around the frame of interest — in ONE launch of msv1_index_play_kernel instead of a
// loop of Shows, each a launch and a synchronise that walks the bitmap and decodes every block of the picture again.
extern "C" int jsp_index_play(jsp_codec* c, jsp_index* idx, int first, int n, int stride, int32_t* const* dsts, int adopt_k,
                              int32_t** data_pnts, int* significant_changes) {
    if (!c || !idx || !dsts) return fail("index_play: null argument");
    if (!is_msv1(c, "index")) return JSP_ERROR_OCCURED;
    if (idx->codec_serial != c->serial) return fail("index_play: the index was built by another codec");
    if (n < 1 || n > 4096) return fail("index_play: n is outside 1..4096");
    if (stride < 1) return fail("index_play: stride must be at least 1");
    if (first < 0 || (int64_t)first + (int64_t)(n - 1) * (int64_t)stride >= (int64_t)idx->nframes) return fail("index_play: the run is outside the index");
    if (adopt_k < -1 || adopt_k >= n) return fail("index_play: adopt_k is outside -1..n-1");
    for (int k = 0; k < n; ++k)
        if (!dsts[k]) return fail("index_play: null argument (an entry of dsts)");
    if (!nothing_in_flight(c, "index_play")) return JSP_ERROR_OCCURED;
    bool aligned16 = true;
    {
        std::vector<const int32_t*> sorted(dsts, dsts + n);
        std::sort(sorted.begin(), sorted.end());
        if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end()) return fail("index_play: the same buffer twice in dsts");
        for (int k = 0; k < n; ++k) {
            if (!dst_not_previous(c, dsts[k], "index_play")) return JSP_ERROR_OCCURED;
            aligned16 = aligned16 && (reinterpret_cast<uintptr_t>(dsts[k]) & 15) == 0;
        }
    }
    try {
        c->activate();
        for (int k = 0; k < n; ++k)
            if (!dst_on_device(dsts[k], "index_play")) return JSP_ERROR_OCCURED;
        if (!device_pointers(c, "index_play")) return JSP_ERROR_OCCURED;
        if (n == 1) stride = 1;
        // a frame before the first adopting one writes nothing (jsp_seek of frames 0..t would not): a null entry for the kernel
        const int first_written = first >= idx->first_adopted ? 0 : (int)std::min<int64_t>(n, ((int64_t)idx->first_adopted - first + stride - 1) / stride);
        if (first_written < n) {
            idx->h_play_dsts.reserve(sizeof(int32_t*) * (size_t)n);
            idx->d_play_dsts.reserve(sizeof(int32_t*) * (size_t)n);
            int32_t** h = static_cast<int32_t**>(idx->h_play_dsts.p);
            std::fill(h, h + first_written, nullptr);
            std::copy(dsts + first_written, dsts + n, h + first_written);
            JSP_HIP(hipMemcpyAsync(idx->d_play_dsts.p, h, sizeof(int32_t*) * (size_t)n, hipMemcpyHostToDevice, c->stream));
            const int segs = c->index_play_segments > 0 ? c->index_play_segments : msv1_index_play_auto_segments(idx->src, n);
            msv1_launch_index_play(idx->src, first, n, stride, segs, idx->d_play_dsts.as<int32_t*>(), aligned16, c->stream);
            JSP_HIP(hipGetLastError());
            JSP_HIP(hipStreamSynchronize(c->stream));   // (the pinned destination list is free for the next call)
        }
        if (adopt_k >= 0) adopt_frame(c, idx, first + adopt_k * stride, dsts[adopt_k]);
        for (int k = 0; k < n; ++k) {
            const int t = first + k * stride;
            if (data_pnts) data_pnts[k] = t >= idx->first_adopted ? dsts[k] : idx->prev_caller;
            if (significant_changes) significant_changes[k] = idx->reported[(size_t)t];
        }
        return JSP_ZERO_STATE;
    } catch (const std::exception& e) {
        set_error("%s", e.what());
        return JSP_ERROR_OCCURED;
    }
}

// ---- the calls the codec is only lent to — jsp_index_thumbs, jsp_index_present, jsp_index_tensor: its stream carries the launch,
// nothing of its state is read or written, and no full-size picture exists anywhere. ---------------------------------------------------
namespace {
// The thumbnail of an index at `scale`: false (error set) for a scale other than 4 / 8 / 16 or a picture too small for one pixel.
bool thumb_size(const jsp_index* idx, int scale, const char* who, int& tw, int& th) {
    if (scale != 4 && scale != 8 && scale != 16) return refuse(who, "scale must be 4, 8 or 16");
    tw = std::max(idx->geo.nbx, 0) * 4 / scale;
    th = std::max(idx->geo.nby, 0) * 4 / scale;
    return (tw > 0 && th > 0) || refuse(who, "the picture is too small for a thumbnail at this scale");
}

// What those calls do before their launch, in the order of their refusals: the index is this codec's; `first`, the call's own checks
// that come before the frame numbers (n is one of them); every frame number lies inside the index; `then`, the call's other checks;
// nothing is in flight; c->activate(); `out` is device memory; the frame list goes to the device on the codec's stream.  The device
// list, or null: refused and the error set (`first` and `then` return false with theirs).
template <class First, class Then>
const int32_t* lent_frame_list(jsp_codec* c, jsp_index* idx, const char* who, int n, const int* frames, const void* out, First&& first, Then&& then) {
    if (idx->codec_serial != c->serial) return refuse(who, "the index was built by another codec"), nullptr;
    if (!first()) return nullptr;
    for (int k = 0; k < n; ++k)
        if (frames[k] < 0 || frames[k] >= idx->nframes) return refuse(who, "a frame number is outside the index"), nullptr;
    if (!then() || !nothing_in_flight(c, who)) return nullptr;
    c->activate();
    if (!on_device(out, who, "out must be a device buffer")) return nullptr;
    idx->h_frame_list.reserve(sizeof(int32_t) * (size_t)n);
    idx->d_frame_list.reserve(sizeof(int32_t) * (size_t)n);
    std::copy(frames, frames + n, idx->h_frame_list.as<int32_t>());
    JSP_HIP(hipMemcpyAsync(idx->d_frame_list.p, idx->h_frame_list.p, sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice, c->stream));
    return idx->d_frame_list.as<const int32_t>();
}

// ... and after it: the launch went in, and the pinned list is free for the next call.
int launched(jsp_codec* c) {
    JSP_HIP(hipGetLastError());
    JSP_HIP(hipStreamSynchronize(c->stream));
    return JSP_ZERO_STATE;
}
}  // namespace

extern "C" int jsp_index_thumb_size(const jsp_index* idx, int scale, int* width, int* height) {
    if (!idx || !width || !height) return fail("index_thumb_size: null argument");
    int tw = 0, th = 0;
    if (!thumb_size(idx, scale, "index_thumb_size", tw, th)) return JSP_ERROR_OCCURED;
    *width = tw;
    *height = th;
    return JSP_ZERO_STATE;
}

// Thumbnails: the preview that follows the pointer along the seek bar (Main.on_mouse_move, Main.hx:1147-1215), a filmstrip of a key
// interval — n frames of the index, each reduced scale x scale pixels to one, in ONE launch of msv1_index_thumbs_kernel.
extern "C" int jsp_index_thumbs(jsp_codec* c, jsp_index* idx, int n, const int* frames, int scale, int cols, int32_t* out, size_t out_pixels) {
    const char* who = "index_thumbs";
    if (!c || !idx || !frames || !out) return fail("index_thumbs: null argument");
    if (!is_msv1(c, who)) return JSP_ERROR_OCCURED;
    try {
        const int32_t* d_frames = lent_frame_list(
            c, idx, who, n, frames, out, [&] { return (n >= 1 && n <= 4096) || refuse(who, "n is outside 1..4096"); },
            [&] {
                int tw = 0, th = 0;
                if (!thumb_size(idx, scale, who, tw, th)) return false;
                if (cols < 1) return refuse(who, "cols must be at least 1");
                const uint64_t sheet = (uint64_t)cols * (uint64_t)tw * (uint64_t)((n + (int64_t)cols - 1) / cols) * (uint64_t)th;
                return (uint64_t)out_pixels >= sheet || refuse(who, "out_pixels is smaller than the sheet");
            });
        if (!d_frames) return JSP_ERROR_OCCURED;
        msv1_launch_index_thumbs(idx->src, d_frames, n, scale, cols, out, c->stream);
        return launched(c);
    } catch (const std::exception& e) {
        set_error("%s", e.what());
        return JSP_ERROR_OCCURED;
    }
}

// Windows: the hover preview at the size the UI wants, a scrub at 200 % with the view scrolled, a contact sheet — the windows
// jsp_display_present / jsp_display_present_area would show of n frames of the index, on one sheet, in ONE launch of
// msv1_index_present_kernel.  No frame buffer is written.
extern "C" int jsp_index_present(jsp_codec* c, jsp_index* idx, int n, const int* frames, int32_t* out, size_t out_ints, int win_w, int win_h,
                                 size_t out_pitch, int cols, double k, double dx, double dy, int mode, int filter, uint32_t background) {
    const char* who = "index_present";
    if (!c || !idx || !frames || !out) return fail("index_present: null argument");
    if (!is_msv1(c, "index")) return JSP_ERROR_OCCURED;
    try {
        const int32_t* d_frames = lent_frame_list(
            c, idx, who, n, frames, out,
            [&] {
                const char* why = index_present_refusal(n, out_ints, win_w, win_h, out_pitch, cols, k, dx, dy, mode, filter);
                return !why || refuse(who, why);
            },
            [&] { return (idx->geo.X >= 1 && idx->geo.Y >= 1) || refuse(who, "the index has no picture"); });
        if (!d_frames) return JSP_ERROR_OCCURED;
        const IndexPresentArgs a = index_present_args(out, n, idx->geo.X, idx->geo.Y, win_w, win_h, out_pitch, cols, k, dx, dy, filter, background, 4);
        msv1_launch_index_present(idx->src, d_frames, n, a, mode, filter, c->stream);
        return launched(c);
    } catch (const std::exception& e) {
        set_error("%s", e.what());
        return JSP_ERROR_OCCURED;
    }
}

// Tensors: the same windows as a model's input batch — N x 3 x H x W or N x H x W x 3, float32 / float16 / bfloat16 / uint8, scaled and
// biased per channel — in ONE launch of msv1_index_tensor_kernel: Present's kernel with another last step.  No sheet is written.
extern "C" int jsp_index_tensor(jsp_codec* c, jsp_index* idx, int n, const int* frames, void* out, size_t out_bytes, int win_w, int win_h, double k,
                                double dx, double dy, int mode, int filter, uint32_t background, int dtype, int layout, const float* scale,
                                const float* bias) {
    const char* who = "index_tensor";
    if (!c || !idx || !frames || !out) return fail("index_tensor: null argument");
    if (!is_msv1(c, "index")) return JSP_ERROR_OCCURED;
    try {
        const int32_t* d_frames = lent_frame_list(
            c, idx, who, n, frames, out,
            [&] {
                const char* why = index_tensor_refusal(n, out, out_bytes, win_w, win_h, k, dx, dy, mode, filter, dtype, layout, scale, bias);
                return !why || refuse(who, why);
            },
            [&] { return (idx->geo.X >= 1 && idx->geo.Y >= 1) || refuse(who, "the index has no picture"); });
        if (!d_frames) return JSP_ERROR_OCCURED;
        const IndexPresentArgs a = index_present_args(nullptr, n, idx->geo.X, idx->geo.Y, win_w, win_h, (size_t)win_w, 1, k, dx, dy, filter, background, 4);
        const IndexTensorArgs t = index_tensor_args(out, win_w, dtype, layout, scale, bias);
        msv1_launch_index_tensor(idx->src, d_frames, n, a, t, mode, filter, c->stream);
        return launched(c);
    } catch (const std::exception& e) {
        set_error("%s", e.what());
        return JSP_ERROR_OCCURED;
    }
}

// ---- activity: how many pixels of every 16x16 cell each frame of a run changed — the seek bar's activity strip, "skip idle" judged
// on the part of the picture in view, the rectangle to scroll to — in ONE launch of msv1_index_activity_kernel.  The first call that
// looks across frames instead of at one; the codec is only lent, as for Thumbs, and no picture is written.
extern "C" int jsp_index_activity_size(const jsp_index* idx, int* cols, int* rows) {
    if (!idx || !cols || !rows) return fail("index_activity: null argument");
    *cols = (std::max(idx->geo.X, 0) + 15) / 16;
    *rows = (std::max(idx->geo.Y, 0) + 15) / 16;
    return JSP_ZERO_STATE;
}

extern "C" int jsp_index_activity(jsp_codec* c, jsp_index* idx, int first, int n, uint16_t* out, size_t out_elems) {
    const char* who = "index_activity";
    if (!c || !idx || !out) return fail("index_activity: null argument");
    if (!is_msv1(c, "index")) return JSP_ERROR_OCCURED;
    if (idx->codec_serial != c->serial) return fail("index_activity: the index was built by another codec");
    if (n < 1 || n > 4096) return fail("index_activity: n is outside 1..4096");
    if (first < 0 || (int64_t)first + (int64_t)n > (int64_t)idx->nframes) return fail("index_activity: the run is outside the index");
    const int cols = (std::max(idx->geo.X, 0) + 15) / 16, rows = (std::max(idx->geo.Y, 0) + 15) / 16;
    const uint64_t elems = (uint64_t)n * (uint64_t)rows * (uint64_t)cols;
    if ((uint64_t)out_elems < elems) return fail("index_activity: out_elems is smaller than the map");
    if (reinterpret_cast<uintptr_t>(out) & 1) return fail("index_activity: out is not aligned to 2 bytes");
    if (!nothing_in_flight(c, who)) return JSP_ERROR_OCCURED;
    try {
        c->activate();
        if (!on_device(out, who, "out must be a device buffer")) return JSP_ERROR_OCCURED;
        if (elems == 0) return JSP_ZERO_STATE;   // (an index without a picture)
        JSP_HIP(hipMemsetAsync(out, 0, elems * sizeof(uint16_t), c->stream));   // (the kernel stores the non-zero counts only)
        const int segs = c->index_activity_segments > 0 ? c->index_activity_segments : msv1_index_play_auto_segments(idx->src, n);
        msv1_launch_index_activity(idx->src, first, n, segs, out, cols, rows, c->stream);
        return launched(c);
    } catch (const std::exception& e) {
        set_error("%s", e.what());
        return JSP_ERROR_OCCURED;
    }
}

// ---- distance: how many pixels of every 16x16 cell each frame of a run differs from ONE reference picture — a frame of the index or a
// device picture — in ONE launch of msv1_index_distance_kernel: Activity's walk with another last step.  The launch writes every
// element, so no memset goes in front; the codec is only lent and no picture is written.
extern "C" int jsp_index_distance(jsp_codec* c, jsp_index* idx, int ref_frame, const int32_t* ref_picture, int first, int n, uint16_t* out,
                                  size_t out_elems) {
    const char* who = "index_distance";
    if (!c || !idx || !out) return fail("index_distance: null argument");
    if (!is_msv1(c, "index")) return JSP_ERROR_OCCURED;
    if (idx->codec_serial != c->serial) return fail("index_distance: the index was built by another codec");
    if (n < 1 || n > 4096) return fail("index_distance: n is outside 1..4096");
    if (first < 0 || (int64_t)first + (int64_t)n > (int64_t)idx->nframes) return fail("index_distance: the run is outside the index");
    if ((ref_picture != nullptr) != (ref_frame == JSP_REF_PICTURE)) return fail("index_distance: ref_frame and ref_picture disagree (JSP_REF_PICTURE goes with a picture, a frame with none)");
    if (!ref_picture && (ref_frame < -1 || ref_frame >= idx->nframes)) return fail("index_distance: ref_frame is outside -1..nframes-1");
    if (reinterpret_cast<uintptr_t>(ref_picture) & 3) return fail("index_distance: ref_picture is not aligned to 4 bytes");
    const int cols = (std::max(idx->geo.X, 0) + 15) / 16, rows = (std::max(idx->geo.Y, 0) + 15) / 16;
    const uint64_t elems = (uint64_t)n * (uint64_t)rows * (uint64_t)cols;
    if ((uint64_t)out_elems < elems) return fail("index_distance: out_elems is smaller than the map");
    if (reinterpret_cast<uintptr_t>(out) & 1) return fail("index_distance: out is not aligned to 2 bytes");
    if (!nothing_in_flight(c, who)) return JSP_ERROR_OCCURED;
    try {
        c->activate();
        if (!on_device(out, who, "out must be a device buffer")) return JSP_ERROR_OCCURED;
        if (ref_picture && !on_device(ref_picture, who, "ref_picture must be a device frame buffer")) return JSP_ERROR_OCCURED;
        if (elems == 0) return JSP_ZERO_STATE;   // (an index without a picture)
        const int segs = c->index_activity_segments > 0 ? c->index_activity_segments : msv1_index_play_auto_segments(idx->src, n);
        msv1_launch_index_distance(idx->src, ref_frame, ref_picture, first, n, segs, out, cols, rows, c->stream);
        return launched(c);
    } catch (const std::exception& e) {
        set_error("%s", e.what());
        return JSP_ERROR_OCCURED;
    }
}

// ---- a key frame for any frame: the clip from frame t on has to start on a key frame, and t is almost never one.  The picture of
// frame t is, block by block, what the last frame <= t that coded the block made of it, and that frame's code lies in the resident
// stream bytes: the key frame is those codes in block order — file bytes the file already contained, no pixel decoded (the rule:
// msv1_index_keyframe_kernels.hip).  TWO launches; the first call that produces a stream, and into HOST memory.  The codec is only lent.
extern "C" int jsp_index_key_frame_bound(const jsp_index* idx, size_t* bytes) {
    if (!idx || !bytes) return fail("index_key_frame: null argument");
    *bytes = (size_t)std::max(idx->geo.nblocks, 0) * (idx->geo.bits == 16 ? 18u : 10u);
    return JSP_ZERO_STATE;
}

extern "C" int jsp_index_key_frame(jsp_codec* c, jsp_index* idx, int t, uint8_t* out, size_t cap, size_t* len) {
    const char* who = "index_key_frame";
    if (len) *len = 0;
    if (!c || !idx || !len || (!out && cap)) return fail("index_key_frame: null argument");
    if (!is_msv1(c, "index")) return JSP_ERROR_OCCURED;
    if (idx->codec_serial != c->serial) return fail("index_key_frame: the index was built by another codec");
    if (t < 0 || t >= idx->nframes) return fail("index_key_frame: t is outside the index");
    const Msv1IndexSrc& src = idx->src;
    if (src.nblocks < 1) return fail("index_key_frame: the picture has no 4x4 block");
    if (!nothing_in_flight(c, who)) return JSP_ERROR_OCCURED;
    try {
        c->activate();
        // the scratch: [status, length][a total per workgroup][two words per block][the frame at its bound], 16-byte aligned parts
        const auto up16 = [](size_t n) { return (n + 15) & ~(size_t)15; };
        const size_t totals_at = 16, records_at = totals_at + up16(sizeof(uint32_t) * (size_t)msv1_keyframe_workgroups(src.nblocks));
        const size_t out_at = records_at + up16(2 * sizeof(uint32_t) * (size_t)src.nblocks);
        const size_t bound = (size_t)src.nblocks * (src.bits == 16 ? 18u : 10u);
        idx->d_key_frame.reserve(out_at + bound);
        idx->h_key_frame.reserve(4 * sizeof(uint32_t));
        uint8_t* d = idx->d_key_frame.as<uint8_t>();
        const Msv1KeyFrameScratch k{reinterpret_cast<uint32_t*>(d), reinterpret_cast<uint32_t*>(d + totals_at),
                                    reinterpret_cast<uint32_t*>(d + records_at), d + out_at};
        uint32_t* h = idx->h_key_frame.as<uint32_t>();
        JSP_HIP(hipMemsetAsync(k.status, 0xFF, 2 * sizeof(uint32_t), c->stream));
        msv1_launch_index_keyframe(src, t, k, c->stream);
        JSP_HIP(hipGetLastError());
        JSP_HIP(hipMemcpyAsync(h, k.status, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
        JSP_HIP(hipStreamSynchronize(c->stream));
        if (h[0] != 0xFFFFFFFFu) {   // not cuttable: the first block that says so, and for a code cut off its writer
            const uint32_t blk = h[0] >> 1;
            if ((h[0] & 1u) == MSV1_KEYFRAME_NO_WRITER) {
                set_error("index_key_frame: block %u has no writer up to frame %d in the index (it shows the picture before the range)", blk, t);
            } else {
                JSP_HIP(hipMemcpyAsync(h + 2, k.records + 2 * (size_t)blk, sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
                JSP_HIP(hipStreamSynchronize(c->stream));
                set_error("index_key_frame: the code of block %u in frame %u, its last writer, is cut off by the end of the frame's data", blk, h[2]);
            }
            return JSP_ERROR_OCCURED;
        }
        const size_t total = h[1];
        if (total > bound) throw std::runtime_error("index_key_frame: the frame is longer than its bound");
        *len = total;
        if (cap < total) return fail("index_key_frame: cap is smaller than the frame (*len has its length)");
        JSP_HIP(hipMemcpyAsync(out, k.out, total, hipMemcpyDeviceToHost, c->stream));
        JSP_HIP(hipStreamSynchronize(c->stream));
        return JSP_ZERO_STATE;
    } catch (const std::exception& e) {
        set_error("%s", e.what());
        return JSP_ERROR_OCCURED;
    }
}

// ---- the clip calls: stream bytes of frames that exist in no file, gathered from codes the index holds by a block rule — frames that
// span a gap (delta, tight), frames of a block rectangle (crop), along any path (path), of a rectangle that moves (pan).  n pairs a call,
// in slices of pairs so that the scratch stays bounded: a sizes launch per slice first — statuses and lengths of ALL pairs are known
// before a byte reaches `out` — then a sizes and a gather launch per slice (one slice: its records are still there, the gather alone).
// Into HOST memory; the codec is only lent.  The entry points check their arguments and pairs; clip_frames does the rest, once.
namespace {
constexpr uint64_t kDeltaSliceBudget = 64ull << 20;   // option "msv1_index_delta_slice" = "auto": the pairs whose scratch this holds

// Where a clip call's results go (keys: null for a call that reports none).  zero(): what a refusal leaves, and every call starts from.
struct ClipOut {
    int n;
    uint8_t* out;
    size_t cap;
    size_t* lens;
    int* keys;
    size_t* total;
    void zero() const {
        const bool n_ok = n >= 1 && n <= 4096;
        if (total) *total = 0;
        if (lens && n_ok) std::fill(lens, lens + n, (size_t)0);
        if (keys && n_ok) std::fill(keys, keys + n, 0);
    }
};

// Which of the index's scratch pairs a clip call uses, and in which layout.
struct ClipBuffers {
    ClipForm form;
    DeviceBuffer& d;
    PinnedBuffer& h;
};

// The words for block j of a rectangle at (bx, by), bw blocks wide, in a refusal.
void rect_block_words(char (&block)[96], int nbx, int bx, int by, int bw, uint32_t j) {
    snprintf(block, sizeof(block), "block %u of the rectangle (block %lld of the picture)", j, (long long)crop_src_block(nbx, bx, by, bw, (int64_t)j));
}

// The checked call `who` over frames of nb blocks, with the scratch pair `buf` of the index.  The call
// supplies what is its own:
//   put(p, pair, origin)        the two pair words of pair p for the device, and (CLIP_PAN; else origin is null) its four origin words;
//   sizes(m, k), gather(m, k)   its two launches over the m pairs of a slice;
//   name(p, j, pair, block)     the words that name pair p and block j of its frame in a refusal; returns the pair's `to`.
template <class Put, class Sizes, class Gather, class Name>
int clip_frames(const char* who, jsp_codec* c, const Msv1IndexSrc& src, const ClipBuffers& buf, size_t nb, const ClipOut& o, Put&& put,
                Sizes&& sizes, Gather&& gather, Name&& name) {
    const size_t n = (size_t)o.n;
    const ClipForm form = buf.form;
    try {
        c->activate();
        const size_t nwg = (size_t)msv1_keyframe_workgroups((int)nb);
        const size_t bound = nb * (src.bits == 16 ? 18u : 10u);
        size_t S = (size_t)c->index_delta_slice;
        if (S == 0) S = std::clamp<uint64_t>(kDeltaSliceBudget / clip_layout(form, 1, nb, nwg, bound).bytes, 1, 4096);
        S = std::min(S, n);
        const ClipLayout l = clip_layout(form, S, nb, nwg, bound);
        buf.d.reserve(l.bytes);
        buf.h.reserve(l.host_bytes);
        uint8_t* d = buf.d.as<uint8_t>();
        uint8_t* h = buf.h.as<uint8_t>();
        const auto words = [&](size_t at) { return reinterpret_cast<uint32_t*>(d + at); };
        const Msv1ClipScratch k{form == CLIP_PAN ? reinterpret_cast<const int32_t*>(d + l.origins_at) : nullptr,
                                reinterpret_cast<const int32_t*>(d + l.pairs_at),
                                reinterpret_cast<const uint64_t*>(d + l.bases_at),
                                words(l.status_at),
                                words(l.totals_at),
                                words(l.first_at),
                                form == CLIP_GRID ? nullptr : words(l.counts_at),
                                words(l.records_at),
                                d + l.out_at};
        std::vector<size_t> length(n, 0);
        std::vector<uint8_t> all_coded(n, 0);
        // pairs [j0, j0 + m) and where their frames start go to the device, then the sizes launch (not when the records are there)
        const auto upload = [&](size_t j0, size_t m, bool launch) {
            int32_t* ho = reinterpret_cast<int32_t*>(h + l.origins_at);
            int32_t* hp = reinterpret_cast<int32_t*>(h + l.pairs_at);
            uint64_t* hb = reinterpret_cast<uint64_t*>(h + l.bases_at);
            uint64_t at = 0;
            for (size_t i = 0; i < m; ++i) {
                put(j0 + i, hp + 2 * i, k.origins ? ho + 4 * i : nullptr);
                hb[i] = at;
                at += length[j0 + i];
            }
            JSP_HIP(hipMemcpyAsync(d, h, l.status_at, hipMemcpyHostToDevice, c->stream));
            if (!launch) return;
            JSP_HIP(hipMemsetAsync(k.status, 0xFF, sizeof(uint32_t) * m, c->stream));
            sizes((int)m, k);
            JSP_HIP(hipGetLastError());
        };
        for (size_t j0 = 0; j0 < n; j0 += S) {
            const size_t m = std::min(S, n - j0);
            upload(j0, m, true);
            JSP_HIP(hipMemcpyAsync(h + l.status_at, d + l.status_at, l.first_at - l.status_at, hipMemcpyDeviceToHost, c->stream));
            JSP_HIP(hipStreamSynchronize(c->stream));
            const uint32_t* status = reinterpret_cast<const uint32_t*>(h + l.status_at);
            const uint32_t* totals = reinterpret_cast<const uint32_t*>(h + l.totals_at);
            const uint32_t* counts = reinterpret_cast<const uint32_t*>(h + l.counts_at);
            for (size_t i = 0; i < m; ++i) {
                const size_t p = j0 + i;
                if (status[i] != 0xFFFFFFFFu) {   // refused: the first pair, and its first block, that says so
                    const uint32_t j = status[i] >> 1;
                    char pair[64], block[96];
                    const int to = name(p, j, pair, block);
                    if ((status[i] & 1u) == MSV1_KEYFRAME_NO_WRITER) {
                        set_error("%s: pair %d %s: %s has no writer up to frame %d in the index", who, (int)p, pair, block, to);
                    } else {
                        uint32_t* writer = reinterpret_cast<uint32_t*>(h + l.host_bytes - 16);
                        JSP_HIP(hipMemcpyAsync(writer, k.records + 2 * (i * nb + j), sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
                        JSP_HIP(hipStreamSynchronize(c->stream));
                        set_error("%s: pair %d %s: the code of %s in frame %u, its last writer, is cut off by the end of the frame's data", who,
                                  (int)p, pair, block, *writer);
                    }
                    return JSP_ERROR_OCCURED;
                }
                size_t coded = 0;
                for (size_t g = 0; g < nwg; ++g) {
                    length[p] += totals[i * nwg + g];
                    if (k.counts) coded += counts[i * nwg + g];
                }
                all_coded[p] = coded == nb;
                if (length[p] > bound) throw std::runtime_error(std::string(who) + ": a frame is longer than its bound");
            }
        }
        size_t sum = 0;
        for (size_t j = 0; j < n; ++j) {
            sum += (o.lens[j] = length[j]);
            if (o.keys) o.keys[j] = all_coded[j];
        }
        *o.total = sum;
        if (o.cap < sum) return fail("%s: cap is smaller than the frames (*total has their length, lens[] each frame's)", who);
        size_t at = 0;
        for (size_t j0 = 0; j0 < n; j0 += S) {
            const size_t m = std::min(S, n - j0);
            upload(j0, m, S < n);
            gather((int)m, k);
            JSP_HIP(hipGetLastError());
            size_t bytes = 0;
            for (size_t i = 0; i < m; ++i) bytes += length[j0 + i];
            JSP_HIP(hipMemcpyAsync(o.out + at, k.out, bytes, hipMemcpyDeviceToHost, c->stream));
            JSP_HIP(hipStreamSynchronize(c->stream));
            at += bytes;
        }
        return JSP_ZERO_STATE;
    } catch (const std::exception& e) {
        o.zero();
        set_error("%s", e.what());
        return JSP_ERROR_OCCURED;
    }
}
}  // namespace

// ---- inter frames that span a gap: a clip thinned to every s-th frame, or without its idle frames.  The inter frame from the picture
// of frame a to the picture of frame b is, block by block, the code of the block's last writer in (a, b] or a skip (the rule:
// msv1_index_delta_kernels.hip).
extern "C" int jsp_index_delta_bound(const jsp_index* idx, size_t* bytes) {
    if (!idx || !bytes) return fail("index_delta: null argument");
    *bytes = (size_t)std::max(idx->geo.nblocks, 0) * (idx->geo.bits == 16 ? 18u : 10u);
    return JSP_ZERO_STATE;
}

namespace {
// jsp_index_delta_frames (who = "index_delta") and jsp_index_tight_frames ("index_tight", tight): the rule of the sizes launch apart.
int index_gap_frames(const char* who, bool tight, jsp_codec* c, jsp_index* idx, int n, const int* from, const int* to, uint8_t* out, size_t cap,
                     size_t* lens, size_t* total) {
    const ClipOut o{n, out, cap, lens, nullptr, total};
    o.zero();
    if (!c || !idx || !from || !to || !lens || !total || (!out && cap)) return fail("%s: null argument", who);
    if (!is_msv1(c, "index")) return JSP_ERROR_OCCURED;
    if (idx->codec_serial != c->serial) return fail("%s: the index was built by another codec", who);
    if (n < 1 || n > 4096) return fail("%s: n is outside 1..4096", who);
    for (int j = 0; j < n; ++j)
        if (from[j] < -1 || to[j] <= from[j] || to[j] >= idx->nframes) {
            set_error("%s: pair %d (%d, %d] is not a gap of the index (-1 <= from < to < %d frames)", who, j, from[j], to[j], idx->nframes);
            return JSP_ERROR_OCCURED;
        }
    const Msv1IndexSrc& src = idx->src;
    if (src.nblocks < 1) return fail("%s: the picture has no 4x4 block", who);
    if (!nothing_in_flight(c, who)) return JSP_ERROR_OCCURED;
    return clip_frames(
        who, c, src, ClipBuffers{CLIP_GRID, idx->d_delta, idx->h_delta}, (size_t)src.nblocks, o,
        [&](size_t p, int32_t* pair, int32_t*) {
            pair[0] = from[p];
            pair[1] = to[p];
        },
        [&](int m, const Msv1ClipScratch& k) { msv1_launch_index_delta_sizes(src, m, k, tight, c->stream); },
        [&](int m, const Msv1ClipScratch& k) { msv1_launch_index_delta_gather(src, m, k, c->stream); },
        [&](size_t p, uint32_t j, char(&pair)[64], char(&block)[96]) {
            snprintf(pair, sizeof(pair), "(%d, %d]", from[p], to[p]);
            snprintf(block, sizeof(block), "block %u", j);
            return to[p];
        });
}
}  // namespace

extern "C" int jsp_index_delta_frames(jsp_codec* c, jsp_index* idx, int n, const int* from, const int* to, uint8_t* out, size_t cap, size_t* lens,
                                      size_t* total) {
    return index_gap_frames("index_delta", false, c, idx, n, from, to, out, cap, lens, total);
}

// The same frames with the blocks dropped whose pixels the gap did not change (THE TIGHT RULE: msv1_index_delta_kernels.hip).
extern "C" int jsp_index_tight_frames(jsp_codec* c, jsp_index* idx, int n, const int* from, const int* to, uint8_t* out, size_t cap, size_t* lens,
                                      size_t* total) {
    return index_gap_frames("index_tight", true, c, idx, n, from, to, out, cap, lens, total);
}

// ---- a clip of a part of the picture: the frames of a block rectangle (bx, by, bw, bh) of the index — per pair a key frame of the
// rectangle (from == JSP_CROP_KEY) or the inter frame over a gap, Delta or with JSP_CROP_TIGHT Tight, of the virtual index whose
// block j is the rectangle's block j (the rule: msv1_index_crop_kernels.hip).  A code carries no position, so again only codes the
// index holds are gathered.  keys[j] says that frame j codes every block of the rectangle.
extern "C" int jsp_index_crop_bound(const jsp_index* idx, int bw, int bh, size_t* bytes) {
    if (bytes) *bytes = 0;
    if (!idx || !bytes) return fail("index_crop: null argument");
    if (!crop_rect_ok(idx->geo.nbx, idx->geo.nby, 0, 0, bw, bh)) return fail("index_crop: the rectangle is outside the block grid");
    *bytes = (size_t)bw * (size_t)bh * (idx->geo.bits == 16 ? 18u : 10u);
    return JSP_ZERO_STATE;
}

// jsp_index_crop_frames (who = "index_crop") and jsp_index_path_frames ("index_path", path): the check of a pair, the sizes launch and
// the words that name a pair in a refusal apart.  Both use the index's crop scratch.
namespace {
int index_rect_frames(const char* who, bool path, jsp_codec* c, jsp_index* idx, int bx, int by, int bw, int bh, int n, const int* from,
                      const int* to, int flags, uint8_t* out, size_t cap, size_t* lens, int* keys, size_t* total) {
    const ClipOut o{n, out, cap, lens, keys, total};
    o.zero();
    if (!c || !idx || !from || !to || !lens || !total || (!out && cap)) return fail("%s: null argument", who);
    if (!is_msv1(c, "index")) return JSP_ERROR_OCCURED;
    if (idx->codec_serial != c->serial) return fail("%s: the index was built by another codec", who);
    const Msv1IndexSrc& src = idx->src;
    if (src.nblocks < 1 || !crop_rect_ok(src.nbx, src.nby, bx, by, bw, bh)) {
        set_error("%s: the rectangle (%d, %d, %d x %d blocks) is outside the block grid (%d x %d blocks)", who, bx, by, bw, bh,
                  src.nblocks < 1 ? 0 : src.nbx, src.nblocks < 1 ? 0 : src.nby);
        return JSP_ERROR_OCCURED;
    }
    if (n < 1 || n > 4096) return fail("%s: n is outside 1..4096", who);
    if (flags & ~JSP_CROP_TIGHT) return fail("%s: unknown flag bits", who);
    for (int j = 0; j < n; ++j) {
        if (path) {
            if (path_pair_ok(idx->nframes, from[j], to[j], JSP_CROP_KEY)) continue;
            set_error("%s: pair %d (%d, %d) is no pair of the index: `to` is one of its %d frames, `from` is one too (a step forward, a "
                      "hold or a step back), or -1 (before the range), or %d (a key pair)",
                      who, j, from[j], to[j], idx->nframes, JSP_CROP_KEY);
            return JSP_ERROR_OCCURED;
        }
        const bool ok = from[j] == JSP_CROP_KEY ? to[j] >= 0 && to[j] < idx->nframes : from[j] >= -1 && to[j] > from[j] && to[j] < idx->nframes;
        if (!ok) {
            set_error("%s: pair %d (%d, %d) is neither a gap of the index (-1 <= from < to < %d frames) nor a key pair (from = %d, 0 <= to)",
                      who, j, from[j], to[j], idx->nframes, JSP_CROP_KEY);
            return JSP_ERROR_OCCURED;
        }
    }
    if (!nothing_in_flight(c, who)) return JSP_ERROR_OCCURED;
    const bool tight = (flags & JSP_CROP_TIGHT) != 0;
    const Msv1CropRect r{bx, by, bw, bh, bw * bh};
    return clip_frames(
        who, c, src, ClipBuffers{CLIP_RECT, idx->d_crop, idx->h_crop}, (size_t)r.nb, o,
        [&](size_t p, int32_t* pair, int32_t*) {
            pair[0] = from[p];
            pair[1] = to[p];
        },
        [&](int m, const Msv1ClipScratch& k) {
            if (path) msv1_launch_index_path_sizes(src, r, m, k, tight, c->stream);
            else msv1_launch_index_crop_sizes(src, r, m, k, tight, c->stream);
        },
        [&](int m, const Msv1ClipScratch& k) { msv1_launch_index_crop_gather(src, r, m, k, c->stream); },
        [&](size_t p, uint32_t j, char(&pair)[64], char(&block)[96]) {
            if (from[p] == JSP_CROP_KEY) snprintf(pair, sizeof(pair), "(key, %d)", to[p]);
            else if (from[p] > to[p]) snprintf(pair, sizeof(pair), "(%d -> %d, back)", from[p], to[p]);   // (path only)
            else snprintf(pair, sizeof(pair), "(%d, %d]", from[p], to[p]);
            rect_block_words(block, src.nbx, bx, by, bw, j);
            return to[p];
        });
}
}  // namespace

extern "C" int jsp_index_crop_frames(jsp_codec* c, jsp_index* idx, int bx, int by, int bw, int bh, int n, const int* from, const int* to,
                                     int flags, uint8_t* out, size_t cap, size_t* lens, int* keys, size_t* total) {
    return index_rect_frames("index_crop", false, c, idx, bx, by, bw, bh, n, from, to, flags, out, cap, lens, keys, total);
}

// ---- a clip along any path through the index: jsp_index_crop_frames with pairs in either direction — a step back (from > to), a hold
// (from == to), and crop's key and gap pairs unchanged (the rule: msv1_index_path_kernels.hip).  A step back gathers, for the blocks
// the frames of (to, from] coded, the code of the last writer <= to: again only codes the index holds.  Scratch and gather launch are
// jsp_index_crop_frames'.
extern "C" int jsp_index_path_frames(jsp_codec* c, jsp_index* idx, int bx, int by, int bw, int bh, int n, const int* from, const int* to,
                                     int flags, uint8_t* out, size_t cap, size_t* lens, int* keys, size_t* total) {
    return index_rect_frames("index_path", true, c, idx, bx, by, bw, bh, n, from, to, flags, out, cap, lens, keys, total);
}

// ---- a clip that pans across the picture: jsp_index_crop_frames with an origin per pair and end of a pair (the rule:
// msv1_index_pan_kernels.hip).  A moved pair of a call without JSP_CROP_TIGHT goes to the device as the key pair of its rectangle at
// `to`.
extern "C" int jsp_index_pan_frames(jsp_codec* c, jsp_index* idx, int bw, int bh, int n, const int* from, const int* to, const int* from_xy,
                                    const int* to_xy, int flags, uint8_t* out, size_t cap, size_t* lens, int* keys, size_t* total) {
    const char* who = "index_pan";
    const bool n_ok = n >= 1 && n <= 4096;
    const ClipOut o{n, out, cap, lens, keys, total};
    o.zero();
    if (!c || !idx || !from || !to || !to_xy || !lens || !total || (!out && cap)) return fail("%s: null argument", who);
    if (!from_xy && n_ok && std::any_of(from, from + n, [](int f) { return f != JSP_CROP_KEY; })) return fail("%s: null argument", who);
    if (!is_msv1(c, "index")) return JSP_ERROR_OCCURED;
    if (idx->codec_serial != c->serial) return fail("%s: the index was built by another codec", who);
    const Msv1IndexSrc& src = idx->src;
    if (src.nblocks < 1 || !crop_rect_ok(src.nbx, src.nby, 0, 0, bw, bh)) {
        set_error("%s: the rectangle's size (%d x %d blocks) is outside the block grid (%d x %d blocks)", who, bw, bh,
                  src.nblocks < 1 ? 0 : src.nbx, src.nblocks < 1 ? 0 : src.nby);
        return JSP_ERROR_OCCURED;
    }
    if (!n_ok) return fail("%s: n is outside 1..4096", who);
    if (flags & ~JSP_CROP_TIGHT) return fail("%s: unknown flag bits", who);
    for (int j = 0; j < n; ++j) {
        const int* a = from_xy ? from_xy + 2 * j : to_xy + 2 * j;   // (null: every pair is a key pair, and a key pair's A is not read)
        const int* b = to_xy + 2 * j;
        switch (pan_pair_check(idx->nframes, src.nbx, src.nby, bw, bh, from[j], to[j], JSP_CROP_KEY, a, b)) {
            case PAN_OK: continue;
            case PAN_BAD_FRAMES:
                set_error("%s: pair %d (%d, %d) is neither a gap of the index (-1 <= from < to < %d frames; from <= to where the rectangle "
                          "moves) nor a key pair (from = %d, 0 <= to)",
                          who, j, from[j], to[j], idx->nframes, JSP_CROP_KEY);
                break;
            case PAN_BAD_TO_ORIGIN:
                set_error("%s: pair %d (%d, %d): the rectangle at `to` (%d, %d, %d x %d blocks) is outside the block grid (%d x %d blocks)", who, j,
                          from[j], to[j], b[0], b[1], bw, bh, src.nbx, src.nby);
                break;
            case PAN_BAD_FROM_ORIGIN:
                set_error("%s: pair %d (%d, %d): the rectangle at `from` (%d, %d, %d x %d blocks) is outside the block grid (%d x %d blocks)", who,
                          j, from[j], to[j], a[0], a[1], bw, bh, src.nbx, src.nby);
                break;
        }
        return JSP_ERROR_OCCURED;
    }
    if (!nothing_in_flight(c, who)) return JSP_ERROR_OCCURED;
    const bool tight = (flags & JSP_CROP_TIGHT) != 0;
    const auto kind_of = [&](size_t p) { return pan_kind(from[p], JSP_CROP_KEY, from_xy ? from_xy + 2 * p : to_xy + 2 * p, to_xy + 2 * p); };
    return clip_frames(
        who, c, src, ClipBuffers{CLIP_PAN, idx->d_pan, idx->h_pan}, (size_t)bw * (size_t)bh, o,
        [&](size_t p, int32_t* pair, int32_t* origin) {
            const PanKind kind = kind_of(p);
            const int* b = to_xy + 2 * p;
            const int* a = kind == PAN_KEY ? b : from_xy + 2 * p;
            origin[0] = a[0];
            origin[1] = a[1];
            origin[2] = b[0];
            origin[3] = b[1];
            pair[0] = kind == PAN_MOVED && !tight ? JSP_CROP_KEY : from[p];
            pair[1] = to[p];
        },
        [&](int m, const Msv1ClipScratch& k) { msv1_launch_index_pan_sizes(src, bw, bh, m, k, tight, c->stream); },
        [&](int m, const Msv1ClipScratch& k) { msv1_launch_index_pan_gather(src, bw, bh, m, k, c->stream); },
        [&](size_t p, uint32_t j, char(&pair)[64], char(&block)[96]) {
            const PanKind kind = kind_of(p);
            if (kind == PAN_KEY) snprintf(pair, sizeof(pair), "(key, %d)", to[p]);
            else if (kind == PAN_STILL) snprintf(pair, sizeof(pair), "(%d, %d]", from[p], to[p]);
            else snprintf(pair, sizeof(pair), "(%d -> %d, moved)", from[p], to[p]);
            rect_block_words(block, src.nbx, to_xy[2 * p], to_xy[2 * p + 1], bw, j);
            return to[p];
        });
}

extern "C" int jsp_index_significance(const jsp_index* idx, int* out) {
    if (!idx || !out) return fail("index_significance: null argument");
    std::copy(idx->significance.begin(), idx->significance.end(), out);
    return JSP_ZERO_STATE;
}

extern "C" int jsp_index_info(const jsp_index* idx, int* nframes, uint64_t* device_bytes, uint64_t* host_bytes) {
    if (!idx) return fail("index_info: null index");
    if (nframes) *nframes = idx->nframes;
    if (device_bytes) *device_bytes = idx->device_bytes();
    if (host_bytes) *host_bytes = idx->host_bytes();
    return JSP_ZERO_STATE;
}

extern "C" void jsp_index_destroy(jsp_index* idx) {
    if (!idx) return;
    // device memory (and the pinned frame list of jsp_index_thumbs) only: no stream, event or staged batch of the codec is touched,
    // so the codec may be gone already
    (void)hipSetDevice(idx->device);
    delete idx;
}
