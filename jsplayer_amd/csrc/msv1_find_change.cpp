// jsp_find_change (include/jsplayer_amd.h): Manager.SkipStills (Manager.hx:289-317) over DataLoader.FindPossibleChange
// (DataLoader.hx:239-252) for MSVideo1 — which frame after the one shown is the first to change the picture significantly, and
// that frame's picture, without decoding and writing every idle frame in between.  Per chunk of the range: the codec's own
// staging, ONE launch of msv1_change_scan_kernel for the frames whose significance needs a pixel compare, then ONE launch of
// msv1_seek_kernel composing the picture up to the hit (or the whole chunk, which becomes the next chunk's picture before).
//
// Kept apart from jsp_api.cpp / msv1_codec.cpp for the same reason as msv1_seek.cpp: those are also built against the stub HIP
// runtime of tools/tsan_cpu.sh.
#include <algorithm>
#include <cstring>

#include "codec.h"
#include "msv1_seek.h"

using namespace jsp;

namespace {

constexpr uint64_t kFindChunkBudget = 1ull << 30;   // as jsp_seek's kSeekChunkBudget

int fail(const char* fmt, const char* what = "") {
    set_error(fmt, what);
    return JSP_ERROR_OCCURED;
}

bool same_bytes(const uint8_t* a, size_t na, const uint8_t* b, size_t nb) {
    return na == nb && (na == 0 || std::memcmp(a, b, na) == 0);
}

}  // namespace

extern "C" int jsp_find_change(jsp_codec* c, int nframes, const uint8_t* const* srcs, const size_t* lens, const uint8_t* is_key, int first,
                               const uint8_t* key_before, size_t key_before_len, int key_row, int32_t* dst, int* found, int* changed,
                               int* significance, int32_t** data_pnt) {
    if (data_pnt) *data_pnt = c ? c->prev_caller : nullptr;
    if (found) *found = -1;
    if (changed) *changed = 0;
    if (significance)
        for (int i = 0; i < nframes; ++i) significance[i] = -1;
    if (!c || nframes <= 0 || !srcs || !lens || !dst || !found || !changed) return fail("find_change: null argument or empty range");
    for (int i = 0; i < nframes; ++i)
        if (!srcs[i] && lens[i]) return fail("find_change: null frame bytes");
    if (first < 0 || first >= nframes) return fail("find_change: first is outside the range");
    if (key_row < 0) return fail("find_change: negative key_row");
    if (c->kind != JSP_CODEC_MSVIDEO1_16 && c->kind != JSP_CODEC_MSVIDEO1_8) return fail("find_change: MSVideo1 only");
    if (c->next_ticket != c->oldest_ticket) return fail("find_change: an asynchronous frame is in flight (jsp_wait for it first)");
    if (dst == c->prev_caller) return fail("find_change: dst is the current previous frame");
    try {
        c->activate();
        hipPointerAttribute_t attr{};
        if (hipPointerGetAttributes(&attr, dst) != hipSuccess || (attr.type != hipMemoryTypeDevice && attr.type != hipMemoryTypeManaged)) {
            (void)hipGetLastError();
            return fail("find_change: dst must be a device frame buffer");
        }
        if (c->ptr_mode == 2) return fail("find_change: codec is in host-pointer mode");
        c->worker_drain();
        c->ptr_mode = 1;
        c->last_key_differs = -1;   // (the key-frame compare of the per-frame calls does not run here)

        auto key_at = [&](int k) { return is_key ? is_key[k] != 0 : true; };
        int hit = -1;               // the frame found (range index)
        bool any_adopted = false;
        const uint64_t table_bytes = 4ull * (uint64_t)std::max((int64_t)c->X / 4 * (c->Y / 4), (int64_t)1);
        for (int a = 0, b = 0; a < nframes && hit < 0; a = b) {
            b = a + 1;
            if (c->seek_chunk_frames > 0) {
                b = std::min(nframes, a + c->seek_chunk_frames);
            } else {
                uint64_t bytes = lens[a] + table_bytes;
                while (b < nframes && bytes + lens[b] + 16384 + table_bytes <= kFindChunkBudget) bytes += lens[b++] + 16384 + table_bytes;
            }
            if (a > 0) JSP_HIP(hipStreamSynchronize(c->stream));   // (the chunk before may still be composing from the batch buffers)
            const int32_t* base = c->prev_dev;   // the picture before this chunk (null: there is none; dst: the chunks before wrote it)
            Msv1HostState saved;
            if (!msv1_save_state(c, saved)) throw std::runtime_error("find_change: not an MSVideo1 codec");
            auto stage = [&](int upto) {         // frames [a, upto) of the range, staged into the codec's seek batch
                std::vector<jsp_frame_in> frames((size_t)(upto - a));
                for (int i = a; i < upto; ++i) frames[(size_t)(i - a)] = jsp_frame_in{srcs[i], lens[i], key_at(i), dst};
                jsp_staged* st = c->stage(frames, c->seek_scratch.get());
                st->device = c->device;
                if (st != c->seek_scratch.get()) c->seek_scratch.reset(st);
                return st;
            };
            jsp_staged* st = stage(b);
            const int nf = b - a;
            int err = -1;   // the first frame of the chunk the reference raises on: nothing at or past it is reached
            for (int i = 0; i < nf && err < 0; ++i)
                if (st->status[(size_t)i] != JSP_ZERO_STATE) err = i;
            Msv1SeekView v;
            if (!msv1_seek_view(st, v)) throw std::runtime_error("find_change: not an MSVideo1 batch");

            // ---- significance the host stage settles: 1 / 0, or -1 = the pixel compare from rows[i] on decides -----------------
            const int lo = std::max(first - a, 0), limit = err >= 0 ? err : nf;
            std::vector<int> sig((size_t)nf, -1);
            c->find_host.reserve(sizeof(uint32_t) * (1 + 2 * (size_t)nf));
            uint32_t* h_first = static_cast<uint32_t*>(c->find_host.p);
            uint32_t* h_rows = h_first + 1;
            uint32_t* h_walk = h_rows + nf;
            std::fill(h_rows, h_rows + nf, 0xFFFFFFFFu);
            int judged_last = -1;
            for (int i = lo; i < limit; ++i) {
                const int k = a + i;
                int s;
                if (key_at(k)) {   // frames_differ_significantly, Manager.hx:392-421
                    const bool key_prev = k > 0 ? key_at(k - 1) : key_before != nullptr;
                    if (key_prev) s = k > 0 ? !same_bytes(srcs[k - 1], lens[k - 1], srcs[k], lens[k]) : !same_bytes(key_before, key_before_len, srcs[k], lens[k]);
                    else if (!v.h_frames[i].prev) s = 1;
                    else { s = -1; h_rows[i] = (uint32_t)key_row; }
                } else {           // DecompressP: stage 1 on the host, stage 2 (st->significant == -1) from insign_lines on
                    s = st->significant[(size_t)i] < 0 ? -1 : st->significant[(size_t)i];
                    if (s < 0) h_rows[i] = v.h_frames[i].cmp_row_lo;
                }
                sig[(size_t)i] = s;
                if (s == 1) break;                 // nothing after a frame the host already knows to be significant is judged
                if (s < 0) judged_last = i;
            }
            if (judged_last >= 0) {
                int nwalk = 0;
                for (int i = 0; i <= judged_last; ++i)   // (frames that code no block — early-outs, all-skip frames — are left out)
                    if (st->adopted[(size_t)i]) h_walk[nwalk++] = (uint32_t)i;
                *h_first = 0xFFFFFFFFu;
                const size_t words = 1 + (size_t)nf + (size_t)nwalk;
                c->find_dev.reserve(sizeof(uint32_t) * words);
                uint32_t* d_first = static_cast<uint32_t*>(c->find_dev.p);
                JSP_HIP(hipMemcpyAsync(d_first, h_first, sizeof(uint32_t) * words, hipMemcpyHostToDevice, c->stream));
                JSP_HIP(hipMemsetAsync(v.d_signif, 0, sizeof(uint32_t) * nf, c->stream));
                msv1_launch_change_scan(v, d_first + 1 + nf, nwalk, d_first + 1, d_first, base ? base : dst, c->stream);
                JSP_HIP(hipGetLastError());
                JSP_HIP(hipMemcpyAsync(v.h_signif, v.d_signif, sizeof(uint32_t) * nf, hipMemcpyDeviceToHost, c->stream));
                JSP_HIP(hipStreamSynchronize(c->stream));
            }
            int local = -1;
            for (int i = lo; i < limit && local < 0; ++i) {
                if (sig[(size_t)i] < 0) sig[(size_t)i] = v.h_signif[i] ? 1 : 0;
                if (significance) significance[a + i] = sig[(size_t)i];
                if (sig[(size_t)i] == 1) local = i;
            }
            if (local < 0 && err >= 0) {
                // the reference raises out of this frame: what the caller had as its previous frame is gone with the range
                c->prev_dev = nullptr;
                c->prev_caller = nullptr;
                set_error("find_change: frame %d of the range: %s", err + a,
                          st->why.empty() ? "the reference raises on this stream" : st->why.c_str());
                return JSP_ERROR_OCCURED;
            }
            if (local >= 0) {
                hit = a + local;
                *changed = 1;
                if (local < nf - 1) {
                    // the staging ran on to the chunk's end: back to where the chunk began, and the prefix up to the hit again, so that
                    // prev_dev and block_changes end at the hit as the per-frame calls would leave them
                    msv1_restore_state(c, saved);
                    st = stage(hit + 1);
                    if (!msv1_seek_view(st, v)) throw std::runtime_error("find_change: not an MSVideo1 batch");
                }
            } else if (b == nframes) {
                hit = nframes - 1;   // nothing changes up to the end: FindPossibleChange lands on the last frame
            }
            bool chunk_adopted = false;
            for (int i = 0; i < v.nframes; ++i) chunk_adopted |= st->adopted[(size_t)i] != 0;
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
