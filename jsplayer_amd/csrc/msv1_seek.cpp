// jsp_seek (include/jsplayer_amd.h): the seek branch of Manager.GetDecompressedFrame (Manager.hx:216-259) for MSVideo1 — frames
// K..N staged as one batch (host or on-GPU parse, the codec's own staging) and composed into the caller's buffer by ONE launch of
// msv1_seek_kernel, instead of N - K + 1 decodes each writing a whole frame.
//
// Kept apart from jsp_api.cpp / msv1_codec.cpp: those are also built against the stub HIP runtime of the host-layer sanitizer
// build (tools/tsan_cpu.sh), which knows nothing of the seek kernel.
#include <algorithm>

#include "codec.h"
#include "msv1_seek.h"

using namespace jsp;

namespace {

// Frames per chunk when the caller leaves it to the library: what the staged range holds in HBM (stream bytes in 16 KiB tiles,
// 4 bytes per block of table) and in pinned host memory stays under this budget.
constexpr uint64_t kSeekChunkBudget = 1ull << 30;

int fail(const char* fmt, const char* what = "") {
    set_error(fmt, what);
    return JSP_ERROR_OCCURED;
}

}  // namespace

extern "C" int jsp_seek(jsp_codec* c, int nframes, const uint8_t* const* srcs, const size_t* lens, const uint8_t* is_key, int32_t* dst,
                        int32_t** data_pnt, int* significant_changes) {
    if (data_pnt) *data_pnt = c ? c->prev_caller : nullptr;
    if (significant_changes) *significant_changes = 0;
    if (!c || nframes <= 0 || !srcs || !lens || !dst) return fail("seek: null argument or empty range");
    for (int i = 0; i < nframes; ++i)
        if (!srcs[i] && lens[i]) return fail("seek: null frame bytes");
    if (c->kind != JSP_CODEC_MSVIDEO1_16 && c->kind != JSP_CODEC_MSVIDEO1_8) return fail("seek: MSVideo1 only");
    if (c->next_ticket != c->oldest_ticket) return fail("seek: an asynchronous frame is in flight (jsp_wait for it first)");
    if (dst == c->prev_caller) return fail("seek: dst is the current previous frame");
    try {
        c->activate();
        hipPointerAttribute_t attr{};
        if (hipPointerGetAttributes(&attr, dst) != hipSuccess || (attr.type != hipMemoryTypeDevice && attr.type != hipMemoryTypeManaged)) {
            (void)hipGetLastError();
            return fail("seek: dst must be a device frame buffer");
        }
        if (c->ptr_mode == 2) return fail("seek: codec is in host-pointer mode");
        c->worker_drain();
        c->ptr_mode = 1;
        c->last_key_differs = -1;   // (the key-frame compare does not run on a seek)

        int sig = 0, last_sig_word = -1;
        bool any_adopted = false;
        uint32_t* h_word = nullptr;
        const uint64_t table_bytes = 4ull * (uint64_t)std::max((int64_t)c->X / 4 * (c->Y / 4), (int64_t)1);
        for (int a = 0, b = 0; a < nframes; a = b) {
            b = a + 1;
            if (c->seek_chunk_frames > 0) {
                b = std::min(nframes, a + c->seek_chunk_frames);
            } else {
                uint64_t bytes = lens[a] + table_bytes;
                while (b < nframes && bytes + lens[b] + 16384 + table_bytes <= kSeekChunkBudget) bytes += lens[b++] + 16384 + table_bytes;
            }
            // (the chunk before may still be composing from the batch buffers that staging refills)
            if (a > 0) JSP_HIP(hipStreamSynchronize(c->stream));
            const int32_t* base = c->prev_dev;   // the picture before this chunk (null: there is none; dst: the chunks before wrote it)
            std::vector<jsp_frame_in> frames((size_t)(b - a));
            for (int i = a; i < b; ++i) frames[(size_t)(i - a)] = jsp_frame_in{srcs[i], lens[i], is_key ? is_key[i] != 0 : true, dst};
            jsp_staged* st = c->stage(frames, c->seek_scratch.get());
            st->device = c->device;
            if (st != c->seek_scratch.get()) c->seek_scratch.reset(st);
            for (int i = 0; i < b - a; ++i)
                if (st->status[(size_t)i] != JSP_ZERO_STATE) {
                    // the reference raises out of this frame: what the caller had as its previous frame is gone with the range
                    c->prev_dev = nullptr;
                    c->prev_caller = nullptr;
                    set_error("seek: frame %d of the range: %s", i + a, st->why.empty() ? "the reference raises on this stream" : st->why.c_str());
                    return JSP_ERROR_OCCURED;
                }
            Msv1SeekView v;
            if (!msv1_seek_view(st, v)) throw std::runtime_error("seek: not an MSVideo1 batch");
            bool chunk_adopted = false;
            for (int ad : st->adopted) chunk_adopted |= ad != 0;
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
