// jsp_index_* (include/jsplayer_amd.h): a resident MSVideo1 SEEK INDEX — a range's stream bytes, block tables and frame records kept in
// HBM after one staging, so that showing any frame of it is ONE launch of msv1_index_show_kernel with no host work: the scrubbing,
// previous-frame and seek-bar navigation of the reference player (Main.on_prevframe / Manager.PrevFrameTime, Manager.hx:184-208;
// Main.on_click, Main.hx:1197-1215) without restaging the range from its key frame on every step.
//
// Build, per chunk of the range (the codec's own staging, the 1 GiB budget and option "msv1_seek_chunk_frames" of jsp_seek):
//   * the chunk is staged and its device buffers change hands (msv1_take_batch) — the index keeps no staged batch, nothing that
//     refers to the codec's streams;
//   * ONE launch of msv1_change_scan_kernel<.., ALL> judges every frame whose significance needs a pixel compare, against a running
//     picture of the build's own (the picture before the chunk);
//   * ONE launch of msv1_coded_bitmap_kernel adds the chunk's frames to the global coded-block bitmap, the per-row coded words and the
//     first untouched block of each frame — from which the host derives, per frame, the per-row block_changes the sequential calls
//     leave behind (MSVideo1.hx:122,305: a row is reset when a frame reaches it);
//   * ONE launch of msv1_seek_kernel moves the running picture on to the chunk's end (when a chunk follows).
// The codec's host state is saved first and put back at the end: the build changes nothing but the index.
//
// Kept apart from jsp_api.cpp / msv1_codec.cpp for the same reason as msv1_seek.cpp: those are also built against the stub HIP
// runtime of tools/tsan_cpu.sh.
#include <algorithm>
#include <cstring>

#include "codec.h"
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
    DeviceBuffer d_chunks, d_frame_chunk, d_bitmap, d_palette, d_before;
    bool has_before = false;
    std::vector<int> significance;         // per frame: jsp_find_change's verdict (1 / 0)
    std::vector<uint8_t> reported;         // per frame: what jsp_seek of frames 0..t reports as *significant_changes
    std::vector<uint8_t> block_changes;    // nframes rows of nby flags: the per-row state after frame t
    int first_adopted = 0;                 // the first frame that adopts its destination (nframes: none)
    int32_t* prev_caller = nullptr;        // the codec's previous frame at build time (what a show before first_adopted leaves)
    int32_t* prev_dev = nullptr;
    uint64_t device_bytes() const {
        uint64_t n = d_chunks.cap + d_frame_chunk.cap + d_bitmap.cap + d_palette.cap + d_before.cap;
        for (const auto& c : chunks) n += c->stream.cap + c->desc.cap + c->frames.cap;
        return n;
    }
    uint64_t host_bytes() const {
        return sizeof(*this) + chunks.size() * sizeof(Chunk) + significance.size() * sizeof(int) + reported.size() + block_changes.size();
    }
};

namespace {

constexpr uint64_t kIndexChunkBudget = 1ull << 30;   // as jsp_seek's kSeekChunkBudget

int fail(const char* fmt, const char* what = "") {
    set_error(fmt, what);
    return JSP_ERROR_OCCURED;
}

bool same_bytes(const uint8_t* a, size_t na, const uint8_t* b, size_t nb) {
    return na == nb && (na == 0 || std::memcmp(a, b, na) == 0);
}

bool is_msv1(const jsp_codec* c) { return c->kind == JSP_CODEC_MSVIDEO1_16 || c->kind == JSP_CODEC_MSVIDEO1_8; }

bool device_pointer(const void* p) {
    hipPointerAttribute_t attr{};
    if (hipPointerGetAttributes(&attr, p) != hipSuccess || (attr.type != hipMemoryTypeDevice && attr.type != hipMemoryTypeManaged)) {
        (void)hipGetLastError();
        return false;
    }
    return true;
}

}  // namespace

extern "C" jsp_index* jsp_index_build(jsp_codec* c, int nframes, const uint8_t* const* srcs, const size_t* lens, const uint8_t* is_key,
                                      int key_row) {
    if (!c || nframes <= 0 || !srcs || !lens) { fail("index: null argument or empty range"); return nullptr; }
    for (int i = 0; i < nframes; ++i)
        if (!srcs[i] && lens[i]) { fail("index: null frame bytes"); return nullptr; }
    if (key_row < 0) { fail("index: negative key_row"); return nullptr; }
    if (!is_msv1(c)) { fail("index: MSVideo1 only"); return nullptr; }
    if (c->next_ticket != c->oldest_ticket) { fail("index: an asynchronous frame is in flight (jsp_wait for it first)"); return nullptr; }
    if (c->ptr_mode == 2) { fail("index: codec is in host-pointer mode"); return nullptr; }
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
            idx->has_before = true;
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

        auto key_at = [&](int k) { return is_key ? is_key[k] != 0 : true; };
        const uint64_t table_bytes = 4ull * (uint64_t)std::max((int64_t)c->X / 4 * (c->Y / 4), (int64_t)1);
        for (int a = 0, b = 0; a < nframes; a = b) {
            b = a + 1;
            if (c->seek_chunk_frames > 0) {
                b = std::min(nframes, a + c->seek_chunk_frames);
            } else {
                uint64_t bytes = lens[a] + table_bytes;
                while (b < nframes && bytes + lens[b] + 16384 + table_bytes <= kIndexChunkBudget) bytes += lens[b++] + 16384 + table_bytes;
            }
            const int nf = b - a;
            std::vector<jsp_frame_in> frames((size_t)nf);
            for (int i = a; i < b; ++i) frames[(size_t)(i - a)] = jsp_frame_in{srcs[i], lens[i], key_at(i), run};
            jsp_staged* st = c->stage(frames, stg.get());
            st->device = c->device;
            if (st != stg.get()) stg.reset(st);
            for (int i = 0; i < nf; ++i)
                if (st->status[(size_t)i] != JSP_ZERO_STATE) {
                    set_error("index: frame %d of the range: %s", i + a, st->why.empty() ? "the reference raises on this stream" : st->why.c_str());
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

            // ---- significance: what the host stage settles (1 / 0), or the pixel compare from h_rows[i] on (jsp_find_change's rules) ----
            h_work.reserve(sizeof(uint32_t) * 2 * (size_t)nf);
            uint32_t* h_rows = static_cast<uint32_t*>(h_work.p);
            uint32_t* h_walk = h_rows + nf;
            std::fill(h_rows, h_rows + nf, 0xFFFFFFFFu);
            int judged_last = -1;
            bool chunk_adopted = false;
            for (int i = 0; i < nf; ++i) {
                const int k = a + i;
                int s;
                if (key_at(k)) {   // frames_differ_significantly, Manager.hx:392-421 (frame 0 of the range: no key frame before it)
                    if (k > 0 && key_at(k - 1)) s = !same_bytes(srcs[k - 1], lens[k - 1], srcs[k], lens[k]);
                    else if (!v.h_frames[i].prev) s = 1;
                    else { s = -1; h_rows[i] = (uint32_t)key_row; }
                } else {           // DecompressP: stage 1 on the host, stage 2 (st->significant == -1) from insign_lines on
                    s = st->significant[(size_t)i] < 0 ? -1 : st->significant[(size_t)i];
                    if (s < 0) h_rows[i] = v.h_frames[i].cmp_row_lo;
                }
                idx->significance[(size_t)k] = s;
                if (s < 0) judged_last = i;
                noop[(size_t)k] = (v.h_frames[i].pad & MSV1_FRAME_NOOP) != 0;
                if (st->adopted[(size_t)i]) {
                    chunk_adopted = true;
                    idx->first_adopted = std::min(idx->first_adopted, k);
                }
            }
            if (judged_last >= 0) {
                int nwalk = 0;
                for (int i = 0; i <= judged_last; ++i)
                    if (st->adopted[(size_t)i]) h_walk[nwalk++] = (uint32_t)i;
                d_work.reserve(sizeof(uint32_t) * ((size_t)nf + (size_t)nwalk));
                uint32_t* d_hrows = static_cast<uint32_t*>(d_work.p);
                JSP_HIP(hipMemcpyAsync(d_hrows, h_rows, sizeof(uint32_t) * ((size_t)nf + (size_t)nwalk), hipMemcpyHostToDevice, c->stream));
                JSP_HIP(hipMemsetAsync(v.d_signif, 0, sizeof(uint32_t) * (size_t)nf, c->stream));
                msv1_launch_judge_all(v, d_hrows + nf, nwalk, d_hrows, run, c->stream);
                JSP_HIP(hipGetLastError());
                JSP_HIP(hipMemcpyAsync(v.h_signif, v.d_signif, sizeof(uint32_t) * (size_t)nf, hipMemcpyDeviceToHost, c->stream));
            }
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
                idx->reported[(size_t)k] = key_at(k) ? 0 : (uint8_t)idx->significance[(size_t)k];   // (DecompressI reports nothing)
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

        // ---- what the show kernel reads: per-chunk pointers, the chunk of every frame, the palette ---------------------------------
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
        msv1_restore_state(c, saved);
        return idx.release();
    } catch (const std::exception& e) {
        if (restore) msv1_restore_state(c, saved);
        set_error("%s", e.what());
        return nullptr;
    }
}

extern "C" int jsp_index_show(jsp_codec* c, jsp_index* idx, int t, int32_t* dst, int adopt, int32_t** data_pnt, int* significant_changes) {
    if (data_pnt) *data_pnt = c ? c->prev_caller : nullptr;
    if (significant_changes) *significant_changes = 0;
    if (!c || !idx || !dst) return fail("index_show: null argument");
    if (!is_msv1(c)) return fail("index: MSVideo1 only");
    if (idx->codec_serial != c->serial) return fail("index_show: the index was built by another codec");
    if (t < 0 || t >= idx->nframes) return fail("index_show: t is outside the index");
    if (c->next_ticket != c->oldest_ticket) return fail("index_show: an asynchronous frame is in flight (jsp_wait for it first)");
    if (dst == c->prev_caller) return fail("index_show: dst is the current previous frame");
    try {
        c->activate();
        if (!device_pointer(dst)) return fail("index_show: dst must be a device frame buffer");
        if (c->ptr_mode == 2) return fail("index_show: codec is in host-pointer mode");
        const bool adopted = t >= idx->first_adopted;   // jsp_seek of frames 0..t writes dst only then
        if (adopted) {
            msv1_launch_index_show(idx->geo, static_cast<const Msv1IndexChunk*>(idx->d_chunks.p), static_cast<const uint32_t*>(idx->d_frame_chunk.p),
                                   static_cast<const int32_t*>(idx->d_palette.p), static_cast<const uint32_t*>(idx->d_bitmap.p), t, dst,
                                   idx->has_before ? static_cast<const int32_t*>(idx->d_before.p) : nullptr, c->stream);
            JSP_HIP(hipGetLastError());
            JSP_HIP(hipStreamSynchronize(c->stream));
        }
        int32_t* shown = adopted ? dst : idx->prev_caller;
        if (adopt) {
            c->worker_drain();
            c->ptr_mode = 1;
            c->last_key_differs = -1;   // (the key-frame compare does not run on a show, as on a seek)
            const int nby = std::max(idx->geo.nby, 0);
            Msv1HostState s;
            s.prev_dev = adopted ? dst : idx->prev_dev;
            s.block_changes.assign(idx->block_changes.begin() + (size_t)t * (size_t)nby, idx->block_changes.begin() + (size_t)(t + 1) * (size_t)nby);
            msv1_restore_state(c, s);   // (exact per-row flags: nothing stale, nothing that points into the index)
            c->prev_caller = shown;
        }
        if (data_pnt) *data_pnt = shown;
        if (significant_changes) *significant_changes = idx->reported[(size_t)t];
        return JSP_ZERO_STATE;
    } catch (const std::exception& e) {
        set_error("%s", e.what());
        return JSP_ERROR_OCCURED;
    }
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
    // device memory only: no stream, event or staged batch of the codec is touched, so the codec may be gone already
    (void)hipSetDevice(idx->device);
    delete idx;
}
