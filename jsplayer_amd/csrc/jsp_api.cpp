// extern "C" surface of libjsplayer_amd.so (declared in include/jsplayer_amd.h).
#include <cstdlib>

#include "codec.h"

namespace jsp {
std::string& last_error_slot() {
    thread_local std::string s;
    return s;
}
void set_error(const char* fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    std::vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    last_error_slot() = buf;
}
}  // namespace jsp

using namespace jsp;

// ---- jsp_codec common parts ---------------------------------------------------------------

jsp_codec::~jsp_codec() {
    if (next_ticket != oldest_ticket) {   // frames still in flight (never waited for): their kernels write the buffers freed below
        (void)hipSetDevice(device);
        (void)hipDeviceSynchronize();
    }
    for (auto& j : jobs) {
        j.st.reset();
        if (j.done) (void)hipEventDestroy(j.done);
    }
    scratch.reset();
    seek_scratch.reset();
    if (side_stream) { (void)hipStreamSynchronize(side_stream); (void)hipStreamDestroy(side_stream); }
    if (own_stream) (void)hipStreamDestroy(own_stream);
}

void jsp_codec::init_device(int device_id) {
    int count = 0;
    JSP_HIP(hipGetDeviceCount(&count));
    if (count <= 0) throw std::runtime_error("no HIP device visible: the HIP path is mandatory, there is no CPU fallback");
    if (device_id < 0 || device_id >= count) throw std::runtime_error("device_id out of range");
    device = device_id;
    JSP_HIP(hipSetDevice(device));
    // a BLOCKING stream: ordered after whatever the caller queued on the legacy default stream (e.g. the fill that
    // initialised a freshly allocated frame buffer) — a caller that fills and decodes back to back needs no sync of
    // its own.  Distinct codec instances still overlap each other.  (jsp_set_stream replaces it.)
    JSP_HIP(hipStreamCreateWithFlags(&own_stream, hipStreamDefault));
    stream = own_stream;
}

void jsp_codec::activate() { JSP_HIP(hipSetDevice(device)); }

void jsp_staged::finish_results() noexcept {
    if (!decoded) return;
    try {
        if (device >= 0) JSP_HIP(hipSetDevice(device));   // (a re-run launches kernels: on the batch's device, whatever the caller's thread had current)
        after_sync();
    } catch (const std::exception& e) {
        status.assign(status.size(), JSP_ERROR_OCCURED);
        adopted.assign(adopted.size(), 0);
        for (int& s : significant) if (s < 0) s = 0;
        why = e.what();
        set_error("%s", e.what());
        return;
    }
    const auto* words = static_cast<const uint32_t*>(h_signif.p);
    for (size_t i = 0; i < significant.size(); ++i)
        if (significant[i] < 0) significant[i] = words[i] ? 1 : 0;
}

namespace jsp {
void launch_frames_differ(const int32_t* a, const int32_t* b, size_t first_pixel, size_t npixels, uint32_t* d_flag, hipStream_t stream);
}
void jsp_codec::queue_key_compare(const int32_t* dst, const int32_t* prev, int slot) {
    uint32_t* d = static_cast<uint32_t*>(d_keyflag.p) + slot;
    jsp::launch_frames_differ(dst, prev, (size_t)key_compare_row * (size_t)X, (size_t)X * (size_t)Y, d, stream);
    JSP_HIP(hipMemcpyAsync(static_cast<uint32_t*>(h_keyflag.p) + slot, d, sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
}

namespace {

// 1 = device memory, 2 = host memory
int classify_pointer(const void* p) {
    hipPointerAttribute_t attr{};
    hipError_t e = hipPointerGetAttributes(&attr, p);
    if (e != hipSuccess) {
        (void)hipGetLastError();  // plain malloc'd memory: not known to HIP
        return 2;
    }
    return (attr.type == hipMemoryTypeDevice || attr.type == hipMemoryTypeManaged) ? 1 : 2;
}

template <class F>
int guarded(F&& f, int on_error = JSP_ERROR_OCCURED) {
    try {
        return f();
    } catch (const std::exception& e) {
        set_error("%s", e.what());
        return on_error;
    }
}

// Shared body of DecompressI / DecompressP.
int decompress_one(jsp_codec* c, const uint8_t* src, size_t n, int32_t* dst, bool key, int32_t** data_pnt,
                   int* significant) {
    if (!c || !dst || (!src && n)) {
        set_error("null argument");
        return JSP_ERROR_OCCURED;
    }
    c->activate();
    c->worker_drain();
    const int mode = classify_pointer(dst);
    if (c->ptr_mode == 0) c->ptr_mode = mode;
    if (c->ptr_mode != mode) {
        set_error("host and device frame buffers mixed on one codec instance");
        return JSP_ERROR_OCCURED;
    }
    const size_t npx = (size_t)c->X * c->Y;
    jsp_frame_in f{src, n, key, dst};
    if (mode == 2) {
        for (auto& b : c->compat) b.reserve(npx * sizeof(int32_t) + 16);
        int32_t* d0 = static_cast<int32_t*>(c->compat[0].p);
        int32_t* d1 = static_cast<int32_t*>(c->compat[1].p);
        f.dst = (c->prev_dev == d0) ? d1 : d0;
        f.caller_host_dst = dst;
        if (c->may_leave_pixels(f))
            JSP_HIP(hipMemcpyAsync(f.dst, dst, npx * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    }
    std::vector<jsp_frame_in> frames{f};
    const int32_t* prev_before = c->prev_dev;          // what a key frame is compared with (Manager.hx:470, 499-504)
    jsp_staged* st = c->stage(frames, c->scratch.get());
    st->device = c->device;
    if (st != c->scratch.get()) c->scratch.reset(st);
    st->decode(c->stream);
    int key_known = -1;
    bool key_queued = false;
    if (key && c->key_compare_row >= 0 && st->status[0] == JSP_ZERO_STATE && st->adopted[0] && prev_before) {
        key_known = st->key_differs.empty() ? -2 : st->key_differs[0];
        if (key_known == -2) { c->queue_key_compare(f.dst, prev_before, 0); key_queued = true; }
    }
    // the reference paints dst in place, adopted or not: hand back whatever was written
    if (mode == 2 && (st->info.units_coded || st->info.units_copied))
        JSP_HIP(hipMemcpyAsync(dst, f.dst, npx * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    JSP_HIP(hipStreamSynchronize(c->stream));
    st->finish_results();
    if (key) c->last_key_differs = key_queued ? c->read_key_compare(0) : key_known;
    if (!st->cleared.empty() && st->cleared[0]) c->prev_caller = nullptr;
    if (st->adopted[0]) c->prev_caller = dst;
    if (data_pnt) *data_pnt = c->prev_caller;
    if (significant) *significant = st->significant[0];
    if (st->status[0] != JSP_ZERO_STATE)
        set_error("%s", st->why.empty() ? "decode aborted: the reference raises on this stream" : st->why.c_str());
    return st->status[0];
}

}  // namespace

extern "C" {

const char* jsp_last_error(void) { return last_error_slot().c_str(); }
const char* jsp_version(void) { return "jsplayer_amd 0.1 gfx950"; }

jsp_codec* jsp_codec_create(int kind, int width, int height, int bpp, const uint8_t* palette,
                            int palette_bytes, int device_id) {
    try {
        if (width <= 0 || height <= 0) throw std::runtime_error("bad frame size");
        if ((uint64_t)width * height > (1ull << 28)) throw std::runtime_error("frame too large");
        std::unique_ptr<jsp_codec> c;
        switch (kind) {
            case JSP_CODEC_MSVIDEO1_16: c.reset(jsp_make_msv1(16, width, height, nullptr, 0)); break;
            case JSP_CODEC_MSVIDEO1_8: c.reset(jsp_make_msv1(8, width, height, palette, palette_bytes)); break;
            case JSP_CODEC_SCREENPRESSOR: c.reset(jsp_make_screenpressor(width, height, bpp)); break;
            default: throw std::runtime_error("unknown codec kind");
        }
        c->init_device(device_id);
        return c.release();
    } catch (const std::exception& e) {
        set_error("%s", e.what());
        return nullptr;
    }
}

void jsp_codec_destroy(jsp_codec* c) {
    if (!c) return;
    try {
        c->activate();
        c->worker_drain();
        (void)hipStreamSynchronize(c->stream);
        // frames still in flight (never waited for) on other streams of this codec: their kernels write buffers that the
        // derived class's members own — wait here, before any destructor runs
        if (c->next_ticket != c->oldest_ticket) (void)hipDeviceSynchronize();
    } catch (...) {
    }
    delete c;
}

int jsp_preinit(jsp_codec* c, int lines) {
    if (!c) { set_error("null codec"); return JSP_ERROR_OCCURED; }
    return guarded([&] { return c->preinit(lines); });
}

int32_t* jsp_previous_frame(jsp_codec* c) { return c ? c->prev_caller : nullptr; }

int jsp_is_key_frame(jsp_codec* c, const uint8_t* src, size_t n) {
    if (!c || (!src && n)) return 0;
    return guarded([&] { return c->is_key_frame(src, n); }, 0);
}

int jsp_state(jsp_codec*) { return JSP_ZERO_STATE; }
int jsp_continue_i(jsp_codec*) { return JSP_ZERO_STATE; }
int jsp_needs_index(jsp_codec* c) { return c ? c->needs_index() : 0; }

// (defined with the asynchronous path below) the synchronous call as submit + wait, when the codec says that serves it better
bool sync_call_takes_async_path(jsp_codec* c, const int32_t* dst);
int submit_and_wait(jsp_codec* c, const uint8_t* src, size_t n, int32_t* dst, bool key, int32_t** data_pnt, int* significant);

int jsp_decompress_i(jsp_codec* c, const uint8_t* src, size_t n, int32_t* dst) {
    return guarded([&] {
        if (sync_call_takes_async_path(c, dst)) return submit_and_wait(c, src, n, dst, true, nullptr, nullptr);
        return decompress_one(c, src, n, dst, true, nullptr, nullptr);
    });
}

int jsp_decompress_p(jsp_codec* c, const uint8_t* src, size_t n, int32_t* dst, int32_t** data_pnt,
                     int* significant_changes) {
    if (data_pnt) *data_pnt = c ? c->prev_caller : nullptr;
    if (significant_changes) *significant_changes = 0;
    return guarded([&] {
        if (sync_call_takes_async_path(c, dst)) return submit_and_wait(c, src, n, dst, false, data_pnt, significant_changes);
        return decompress_one(c, src, n, dst, false, data_pnt, significant_changes);
    });
}

// ---- frame copies (the frame pool: jsp_pool.cpp) ---------------------------------------------

int jsp_download(const int32_t* device_frame, int32_t* host, size_t npixels) {
    return guarded([&] {
        JSP_HIP(hipMemcpy(host, device_frame, npixels * sizeof(int32_t), hipMemcpyDeviceToHost));
        return 0;
    });
}
int jsp_upload(int32_t* device_frame, const int32_t* host, size_t npixels) {
    return guarded([&] {
        JSP_HIP(hipMemcpy(device_frame, host, npixels * sizeof(int32_t), hipMemcpyHostToDevice));
        return 0;
    });
}

// ---- batched / staged ---------------------------------------------------------------------

int jsp_set_stream(jsp_codec* c, void* hip_stream) {
    if (!c) return JSP_ERROR_OCCURED;
    return guarded([&] {
        c->activate();
        c->async_flush(nullptr);                         // (a frame held for its successor belongs on the stream it was staged for)
        c->stream = hip_stream ? static_cast<hipStream_t>(hip_stream) : c->own_stream;
        return 0;
    });
}

int jsp_prefetch(jsp_codec* c, const void* host, size_t bytes) {
    if (!c || (!host && bytes)) return JSP_ERROR_OCCURED;
    return guarded([&] {
        c->activate();
        return c->prefetch(host, bytes) == 0 ? JSP_ZERO_STATE : JSP_ERROR_OCCURED;
    });
}

int jsp_set_option(jsp_codec* c, const char* key, const char* value) {
    if (!c || !key || !value) return -1;
    if (std::strcmp(key, "key_frame_compare") == 0) {
        if (c->next_ticket != c->oldest_ticket) return -1;
        int row = -1;
        if (std::strcmp(value, "off") != 0) {
            char* end = nullptr;
            const long v = std::strtol(value, &end, 10);
            if (end == value || *end || v < 0 || v > (1 << 24)) return -1;
            row = (int)v;
        }
        return guarded([&] {
            c->activate();
            c->worker_drain();
            if (row >= 0) { c->d_keyflag.reserve(16 * sizeof(uint32_t)); c->h_keyflag.reserve(16 * sizeof(uint32_t)); }
            c->key_compare_row = row;
            c->last_key_differs = -1;
            return 0;
        }, -1);
    }
    if (std::strcmp(key, "async_depth") == 0) {
        char* end = nullptr;
        const long v = std::strtol(value, &end, 10);
        if (end == value || *end || v < 1 || v > 16 || c->next_ticket != c->oldest_ticket) return -1;
        c->async_depth = (int)v;
        return 0;
    }
    // retired launch-plan options (measured slower, removed in round 5): results never depended on them, so a caller that still sets them is not refused
    if (std::strcmp(key, "sp_group_chunk") == 0 || std::strcmp(key, "msv1_parse_pieces") == 0) return 0;
    return guarded([&] {
        c->activate();
        return c->set_option(key, value);
    }, -1);
}

int jsp_key_frame_differs(jsp_codec* c) { return c ? c->last_key_differs : -1; }

long long jsp_counter(jsp_codec* c, const char* name) {
    if (!c || !name) return -1;
    if (std::strcmp(name, "async_reruns") == 0) return c->async_reruns;
    return c->counter(name);
}

// ---- asynchronous per-frame path ---------------------------------------------------------------------------

namespace {

// The frame of job `from` could not be settled by the GPU alone: everything from it on is re-run, in order, through
// the synchronous path (the codec's state is put back to what it was before that frame).
void redo_from(jsp_codec* c, uint64_t from) {
    c->async_flush(nullptr);                             // (frames held for their successors go out as submitted: they find the veto word set and leave their frames alone)
    JSP_HIP(hipStreamSynchronize(c->stream));
    jsp_async_job& first = c->jobs[from % c->async_depth];
    c->async_reset(first.st.get());
    c->prev_caller = first.prev_caller_before;
    c->prev_dev = first.prev_dev_before;
    for (uint64_t t = from; t < c->next_ticket; ++t) {
        jsp_async_job& j = c->jobs[t % c->async_depth];
        int32_t* data = nullptr;
        int sig = 0;
        j.status = decompress_one(c, j.frame.src, j.frame.n, j.frame.dst, j.frame.key, &data, &sig);
        j.significant = sig;
        j.key_differs = c->last_key_differs;
        j.key_compare_queued = false;
        if (j.status != JSP_ZERO_STATE) j.why = last_error_slot();
        j.prev_caller_after = c->prev_caller;
        j.redone = true;
        ++c->async_reruns;
    }
}

// Makes the results of job `t` final: waits for its kernels, reads the verdict of the scout, and re-runs everything from
// it on when the GPU alone could not settle the frame.
void settle(jsp_codec* c, uint64_t t) {
    jsp_async_job& j = c->jobs[t % c->async_depth];
    if (j.redone || j.settled) return;
    if (j.by_worker) {
        c->worker_wait(j);                               // host stage done, uploads and kernels queued, the event recorded
        JSP_HIP(hipEventSynchronize(j.done));
        j.st->finish_results();
        j.status = j.st->status[0];
        j.significant = j.st->significant[0] < 0 ? 0 : j.st->significant[0];
        if (j.status != JSP_ZERO_STATE) j.why = j.st->why.empty() ? "decode aborted: the reference raises on this stream" : j.st->why;
        // what the frame really did to the previous frame (frames are settled in submission order)
        if (!j.st->cleared.empty() && j.st->cleared[0]) c->settled_prev = nullptr;
        if (j.st->adopted[0]) c->settled_prev = j.frame.dst;
        if (j.key_compare_queued) { j.key_differs = c->read_key_compare((int)(t % c->async_depth)); j.key_compare_queued = false; }
        j.prev_caller_after = c->settled_prev;
        if (t + 1 == c->next_ticket) c->prev_caller = c->settled_prev;   // (nothing submitted behind it: the prediction gives way)
        j.settled = true;
        return;
    }
    c->async_flush(&j);                                  // (held for a frame that has not come: launched alone)
    JSP_HIP(hipEventSynchronize(j.done));
    j.st->finish_results();
    if (!c->async_finish(j.st.get())) { redo_from(c, t); return; }
    if (j.key_compare_queued) { j.key_differs = c->read_key_compare((int)(t % c->async_depth)); j.key_compare_queued = false; }
    else if (j.key_differs == -3) j.key_differs = j.st->key_differs.empty() ? -1 : j.st->key_differs[0];
    j.status = j.st->status[0];
    j.significant = j.st->significant[0] < 0 ? 0 : j.st->significant[0];
    if (j.status != JSP_ZERO_STATE) j.why = j.st->why.empty() ? "decode aborted: the reference raises on this stream" : j.st->why;
    j.settled = true;
}


int submit_async(jsp_codec* c, const uint8_t* src, size_t n, int32_t* dst, bool key, uint64_t* ticket) {
    if (!c || !dst || !ticket || (!src && n)) throw std::runtime_error("null argument");
    c->activate();
    if (classify_pointer(dst) != 1) throw std::runtime_error("asynchronous calls take device frame buffers only");
    if (c->ptr_mode == 2) throw std::runtime_error("codec is in host-pointer mode");
    c->ptr_mode = 1;
    if ((int)(c->next_ticket - c->oldest_ticket) >= c->async_depth) throw std::runtime_error("too many frames in flight: jsp_wait for the oldest first");
    // (the ring only ever grows: a smaller `async_depth` changes the modulus, not the vector — the jobs beyond it keep their
    // event and their staged object, whose device buffers the codec may still refer to: Msv1Codec::last_full_dev)
    if ((int)c->jobs.size() < c->async_depth) c->jobs.resize(c->async_depth);
    jsp_async_job& j = c->jobs[c->next_ticket % c->async_depth];
    if (!j.done) JSP_HIP(hipEventCreateWithFlags(&j.done, hipEventDisableTiming));
    j.frame = jsp_frame_in{src, n, key, dst};
    if (c->async_by_workers()) {
        if (c->next_ticket == c->oldest_ticket) c->settled_prev = c->prev_caller;   // nothing in flight: predictions start from the facts
        j.prev_caller_before = c->prev_caller;
        j.prev_dev_before = c->prev_dev;
        j.redone = j.settled = false;
        j.by_worker = true;
        j.key_differs = -1;
        j.key_compare_queued = false;
        j.why.clear();
        c->worker_submit(j);
        j.prev_caller_after = c->prev_caller;
        j.ticket = c->next_ticket++;
        *ticket = j.ticket;
        return JSP_ZERO_STATE;
    }
    j.by_worker = false;
    if (c->async_settle_first(j.frame))
        for (uint64_t t = c->oldest_ticket; t < c->next_ticket; ++t)
            if (c->jobs[t % c->async_depth].st->verdict_pending) settle(c, t);   // the others were settled when they were staged
    j.prev_caller_before = c->prev_caller;
    j.prev_dev_before = c->prev_dev;
    j.redone = j.settled = false;
    j.why.clear();
    j.key_differs = -1;
    j.key_compare_queued = false;
    jsp_staged* st = c->stage_async(j.frame, j.st.get());
    st->device = c->device;
    if (st != j.st.get()) j.st.reset(st);
    const bool wants_compare = key && c->key_compare_row >= 0 && st->status[0] == JSP_ZERO_STATE && st->adopted[0] && j.prev_dev_before;
    if (wants_compare) j.key_differs = st->key_differs.empty() ? -2 : st->key_differs[0];   // (-3: the frame's own kernels compare; async_finish() knows)
    // (a compare pass of the codec's own must follow the frame's kernels at once: such a frame is not handed to async_launch, which may hold it)
    if (j.key_differs == -2 && wants_compare) c->async_flush(nullptr);
    if (!(wants_compare && j.key_differs == -2) && c->async_launch(j)) {
        // the codec launches the frame — now, or together with the next one — and records j.done behind it
    } else {
        st->decode(c->stream);
        // (a frame the GPU may still veto leaves `dst` untouched and is re-run through the synchronous path, which compares again)
        if (wants_compare && j.key_differs == -2) { c->queue_key_compare(dst, j.prev_dev_before, (int)(c->next_ticket % c->async_depth)); j.key_compare_queued = true; }
        JSP_HIP(hipEventRecord(j.done, c->stream));
    }
    if (!st->cleared.empty() && st->cleared[0]) c->prev_caller = nullptr;
    if (st->adopted[0]) c->prev_caller = dst;
    j.prev_caller_after = c->prev_caller;
    j.ticket = c->next_ticket++;
    *ticket = j.ticket;
    return JSP_ZERO_STATE;
}

}  // namespace

extern "C" int jsp_decompress_i_async(jsp_codec* c, const uint8_t* src, size_t n, int32_t* dst, uint64_t* ticket) {
    return guarded([&] { return submit_async(c, src, n, dst, true, ticket); });
}
extern "C" int jsp_decompress_p_async(jsp_codec* c, const uint8_t* src, size_t n, int32_t* dst, uint64_t* ticket) {
    return guarded([&] { return submit_async(c, src, n, dst, false, ticket); });
}
namespace {
int wait_ticket(jsp_codec* c, uint64_t ticket, int32_t** data_pnt, int* significant_changes) {
    if (!c) throw std::runtime_error("null codec");
    if (ticket != c->oldest_ticket || ticket >= c->next_ticket) throw std::runtime_error("tickets are waited for in submission order");
    c->activate();
    jsp_async_job& j = c->jobs[ticket % c->async_depth];
    // from here on the ticket is consumed whatever happens: a caller may let go of the frame's `src` / `dst` exactly when
    // jsp_wait was given the oldest ticket (anything that fails while settling the frame becomes the frame's error)
    try {
        settle(c, ticket);
    } catch (const std::exception& e) {
        j.status = JSP_ERROR_OCCURED;
        j.why = e.what();
        j.settled = true;
    }
    if (j.status != JSP_ZERO_STATE) set_error("%s", j.why.c_str());
    ++c->oldest_ticket;
    j.ticket = 0;
    if (data_pnt) *data_pnt = j.prev_caller_after;
    if (significant_changes) *significant_changes = j.significant;
    if (j.frame.key) {
        c->last_key_differs = c->key_compare_row >= 0 && j.status == JSP_ZERO_STATE ? j.key_differs : -1;
        // ONE mapping, here: jsp_key_frame_differs() says 1 / 0 / -1 (nothing to compare with, or the frame failed); *significant_changes of a
        // key frame THAT DECODED says "changed" for 1 and for -1 (Manager.hx:399-411: the first frame, no previous frame, counts as a
        // change).  A frame that failed reports what the decode reported (0): its status is the news, not a change.
        if (c->key_compare_row >= 0 && significant_changes && j.status == JSP_ZERO_STATE) *significant_changes = j.key_differs != 0 ? 1 : 0;
    }
    return j.status;
}
}  // namespace
// The reference's one synchronous call per frame (Manager.hx:507,511), served by the asynchronous path: device frame buffer,
// nothing in flight, and a codec whose one-frame launch settles the frame by itself (MSVideo1 with the on-GPU parse:
// 0.18 -> 0.07 ms per 1080p key frame against staging a batch of one).
bool sync_call_takes_async_path(jsp_codec* c, const int32_t* dst) {
    return c && dst && c->sync_through_async() && c->ptr_mode != 2 && c->next_ticket == c->oldest_ticket &&
           classify_pointer(dst) == 1;
}
int submit_and_wait(jsp_codec* c, const uint8_t* src, size_t n, int32_t* dst, bool key, int32_t** data_pnt, int* significant) {
    uint64_t ticket = 0;
    submit_async(c, src, n, dst, key, &ticket);
    return wait_ticket(c, ticket, data_pnt, significant);
}
extern "C" int jsp_wait(jsp_codec* c, uint64_t ticket, int32_t** data_pnt, int* significant_changes) {
    if (data_pnt) *data_pnt = nullptr;
    if (significant_changes) *significant_changes = 0;
    return guarded([&] { return wait_ticket(c, ticket, data_pnt, significant_changes); });
}
extern "C" void* jsp_host_alloc(size_t bytes) {
    void* p = nullptr;
    if (hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    return p;
}
extern "C" void jsp_host_free(void* p) { if (p) (void)hipHostFree(p); }

int jsp_sync(jsp_codec* c) {
    if (!c) { set_error("null codec"); return JSP_ERROR_OCCURED; }
    return guarded([&] {
        c->activate();
        c->worker_drain();
        JSP_HIP(hipStreamSynchronize(c->stream));
        if (c->side_stream) JSP_HIP(hipStreamSynchronize(c->side_stream));   // (what was queued beside the launches counts as the caller's work too)
        return 0;
    });
}

namespace {
jsp_staged* stage_batch_into(jsp_codec* c, jsp_staged* reuse, int nframes, const uint8_t* const* srcs, const size_t* lens,
                             const uint8_t* is_key, int32_t* const* dsts);
}
jsp_staged* jsp_stage_batch(jsp_codec* c, int nframes, const uint8_t* const* srcs, const size_t* lens,
                            const uint8_t* is_key, int32_t* const* dsts) {
    return stage_batch_into(c, nullptr, nframes, srcs, lens, is_key, dsts);
}
jsp_staged* jsp_restage_batch(jsp_codec* c, jsp_staged* reuse, int nframes, const uint8_t* const* srcs, const size_t* lens,
                              const uint8_t* is_key, int32_t* const* dsts) {
    return stage_batch_into(c, reuse, nframes, srcs, lens, is_key, dsts);
}
namespace {
jsp_staged* stage_batch_into(jsp_codec* c, jsp_staged* reuse, int nframes, const uint8_t* const* srcs, const size_t* lens,
                             const uint8_t* is_key, int32_t* const* dsts) {
    try {
        if (!c || nframes < 0 || (nframes && (!srcs || !lens || !dsts))) throw std::runtime_error("null argument");
        c->activate();
        std::vector<jsp_frame_in> frames(nframes);
        for (int i = 0; i < nframes; ++i) {
            if (!dsts[i]) throw std::runtime_error("null dst in batch");
            if (classify_pointer(dsts[i]) != 1) throw std::runtime_error("batch entry points take device frame buffers only");
            frames[i] = jsp_frame_in{srcs[i], lens[i], is_key ? is_key[i] != 0 : true, dsts[i]};
        }
        if (c->ptr_mode == 2) throw std::runtime_error("codec is in host-pointer mode");
        if (nframes) c->ptr_mode = 1;
        c->worker_drain();
        jsp_staged* st = c->stage(frames, reuse);
        st->device = c->device;
        if (reuse && st != reuse) delete reuse;       // (a batch object of another kind: replaced)
        for (int i = 0; i < nframes; ++i) {
            if (!st->cleared.empty() && st->cleared[i]) c->prev_caller = nullptr;
            if (st->adopted[i]) c->prev_caller = dsts[i];
        }
        return st;
    } catch (const std::exception& e) {
        set_error("%s", e.what());
        return nullptr;
    }
}
}  // namespace

int jsp_staged_decode(jsp_codec* c, jsp_staged* s) {
    return guarded([&] {
        if (!c || !s) throw std::runtime_error("null argument");
        c->activate();
        s->decode(c->stream);
        return 0;
    });
}

void jsp_staged_destroy(jsp_staged* s) { delete s; }

int jsp_staged_get_info(const jsp_staged* s, jsp_staged_info* out) {
    if (!s || !out) return JSP_ERROR_OCCURED;
    *out = s->info;
    return 0;
}

const char* jsp_staged_kernels(const jsp_staged* s) { return s ? s->kernels.c_str() : ""; }

int jsp_staged_results(jsp_staged* s, int* status, int* adopted, int* significant) {
    if (!s) return JSP_ERROR_OCCURED;
    return guarded([&] {
        s->finish_results();
        for (size_t i = 0; i < s->status.size(); ++i) {
            if (status) status[i] = s->status[i];
            if (adopted) adopted[i] = s->adopted[i];
            if (significant) significant[i] = s->significant[i] < 0 ? 0 : s->significant[i];
        }
        return 0;
    });
}

int jsp_decompress_i_batch(jsp_codec* c, int nframes, const uint8_t* const* srcs, const size_t* lens,
                           int32_t* const* dsts) {
    jsp_staged* st = jsp_stage_batch(c, nframes, srcs, lens, nullptr, dsts);
    if (!st) return JSP_ERROR_OCCURED;
    int rc = jsp_staged_decode(c, st);
    if (rc == 0) rc = jsp_sync(c);
    if (rc == 0) {
        st->finish_results();
        for (int s : st->status)
            if (s != JSP_ZERO_STATE) rc = s;
        if (rc != 0 && !st->why.empty()) set_error("%s", st->why.c_str());
    }
    jsp_staged_destroy(st);
    return rc;
}

}  // extern "C"
