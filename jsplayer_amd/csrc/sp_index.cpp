// The ScreenPressor seek index of include/jsplayer_amd.h — jsp_sp_index_* —: the host entropy stage runs over a range ONCE, its
// records stay resident in HBM, and any frame of the range is then one launch of sp_index_show_kernel, the thumbnails of any n frames
// of it one launch of sp_index_thumbs_kernel, a run of frames played forward from any frame of it one launch of sp_index_play_kernel
// (sp_index_kernels.hip).
//
// Kept apart from sp_codec.cpp / jsp_api.cpp: those are also built against the stub kernels of the host-layer sanitizer build
// (tools/tsan_cpu.sh), which knows nothing of the index kernel.  What the build needs of the codec comes through sp::IndexLender.
#include <algorithm>
#include <cstring>

#include "codec.h"
#include "sp.h"
#include "sp_index_activity.h"

using namespace jsp;
using namespace jsp::sp;

namespace jsp {
void launch_frames_differ(const int32_t* a, const int32_t* b, size_t first_pixel, size_t npixels, uint32_t* d_flag, hipStream_t stream);
}

struct jsp_sp_index {
    uint64_t codec_serial = 0;       // jsp_codec::serial of the codec that built it
    int device = 0;
    Geometry geo{};
    int nframes = 0;
    size_t pic_stride = 0;           // ints from one key picture to the next (a multiple of 4: every picture 16-byte aligned)
    DeviceBuffer d_keys, d_blocks, d_payload, d_bitmap;
    uint64_t table_bytes = 0, payload_bytes = 0, bitmap_bytes = 0, key_bytes = 0;
    std::vector<int32_t> key_of;     // per frame: the frame number of its key picture (a key frame: its own)
    std::vector<int32_t> key_slot;   // per frame: which picture of d_keys that is
    std::vector<int64_t> slot_base;  // per frame: its block table is d_blocks + (frame + slot_base) * nblocks (key frames: unused)
    std::vector<int> significance;   // per frame: the verdict of the sequential run (1 / 0)
    PinnedBuffer h_thumb_recs;       // jsp_sp_index_thumbs / jsp_sp_index_present: the call's per-cell records on their way to ...
    DeviceBuffer d_thumb_recs;       // ... the array the kernel reads (both grown on demand: nothing until the first call)
    DeviceBuffer d_play_frames;      // jsp_sp_index_play: an IndexPlayFrame per frame, then the key-frame mask (nothing until the first call)
    PinnedBuffer h_play_dsts;        // jsp_sp_index_play: the call's destinations on their way to ...
    DeviceBuffer d_play_dsts;        // ... the array the kernel reads (both grown on demand)
    uint64_t device_bytes() const {
        return d_keys.cap + d_blocks.cap + d_payload.cap + d_bitmap.cap + d_thumb_recs.cap + d_play_frames.cap + d_play_dsts.cap;
    }
    uint64_t host_bytes() const {
        return sizeof(*this) + key_of.size() * sizeof(int32_t) + key_slot.size() * sizeof(int32_t) + slot_base.size() * sizeof(int64_t) +
               significance.size() * sizeof(int) + h_thumb_recs.cap + h_play_dsts.cap;
    }
    size_t play_mask_offset() const { return (size_t)nframes * sizeof(IndexPlayFrame); }   // (a multiple of 16)
    const int32_t* key_picture(int t) const { return static_cast<const int32_t*>(d_keys.p) + (size_t)key_slot[(size_t)t] * pic_stride; }
    void show(int t, int32_t* dst, hipStream_t stream) const {
        launch_index_show(geo, dst, key_picture(t), static_cast<const PBlock*>(d_blocks.p), static_cast<const uint32_t*>(d_payload.p),
                          static_cast<const uint32_t*>(d_bitmap.p), t, key_of[(size_t)t], (long)slot_base[(size_t)t], stream);
    }
};

namespace {

int fail(const char* fmt, const char* what = "") {
    set_error(fmt, what);
    return JSP_ERROR_OCCURED;
}

bool on_device(const void* p) {   // (after c->activate())
    hipPointerAttribute_t attr{};
    if (hipPointerGetAttributes(&attr, p) == hipSuccess && (attr.type == hipMemoryTypeDevice || attr.type == hipMemoryTypeManaged)) return true;
    (void)hipGetLastError();
    return false;
}

// exactly `bytes` of device memory (DeviceBuffer::reserve keeps a quarter spare for growth: an index never grows)
void exact(DeviceBuffer& d, size_t bytes) {
    d.release();
    bytes = std::max<size_t>(bytes, 16);
    JSP_HIP(hipMalloc(&d.p, bytes));
    d.cap = bytes;
}

// Host memory to the device through pinned memory owned by the build, slice by slice.
struct Uploader {
    PinnedBuffer pin;
    hipStream_t stream;
    static constexpr size_t kSlice = 8u << 20;
    explicit Uploader(hipStream_t s) : stream(s) { pin.reserve(kSlice); }
    void operator()(void* d, const void* h, size_t bytes) {
        for (size_t at = 0; at < bytes; at += kSlice) {
            const size_t n = std::min(kSlice, bytes - at);
            std::memcpy(pin.p, static_cast<const uint8_t*>(h) + at, n);
            JSP_HIP(hipMemcpyAsync(static_cast<uint8_t*>(d) + at, pin.p, n, hipMemcpyHostToDevice, stream));
            JSP_HIP(hipStreamSynchronize(stream));   // (the slice is free for the next one)
        }
    }
};

// What the destination of frame i holds in its last column: the last column of the picture before it (the rule of jsp_seek — each
// frame's destination starts out holding the picture before it).  `after` notes the column every frame leaves; groups of pictures run
// on threads of their own, each writing its own frames' rows and reading the row of the frame before, which its own thread wrote (a
// group opens with a key frame, and key frames do not ask).
struct PictureColumns : DstColumns {
    const HostFrame* base = nullptr;
    int Y = 0;
    std::vector<int32_t> cols;   // nframes rows of Y
    const int32_t* before(const HostFrame& f) override {
        const size_t i = (size_t)(&f - base);
        return i > 0 ? cols.data() + (i - 1) * (size_t)Y : nullptr;
    }
    void after(const HostFrame& f, const HostDecoder& d, const FrameOut& out) override {
        const size_t i = (size_t)(&f - base);
        int32_t* mine = cols.data() + i * (size_t)Y;
        if (out.adopted) d.last_column(mine);
        else if (i > 0) std::copy(mine - Y, mine, mine);   // an unchanged frame: the picture before it stays
    }
};

// The key frames of one wave of the build, materialised by the codec's key-frame kernels into pictures the index owns.
struct KeyWave {
    std::vector<IRun> runs;
    std::vector<uint32_t> rows, seeds, tileidx, left;
    std::vector<IFrameArgs> iargs;
    std::vector<size_t> run_off, row_off, seed_off, tile_off, left_off;
    DeviceBuffer d_runs, d_rows, d_seeds, d_tileidx, d_left, d_iargs;
    void clear() {
        runs.clear(); rows.clear(); seeds.clear(); tileidx.clear(); left.clear(); iargs.clear();
        run_off.clear(); row_off.clear(); seed_off.clear(); tile_off.clear(); left_off.clear();
    }
    void add(const FrameOut& fo, int32_t* dst, bool tiles) {
        IFrameArgs a{};
        a.dst = dst;
        a.flat = fo.kind == FrameKind::Flat;
        a.colour = fo.flat_colour;
        a.nruns = (uint32_t)fo.runs.size();
        run_off.push_back(runs.size()); row_off.push_back(rows.size()); seed_off.push_back(seeds.size());
        tile_off.push_back(tileidx.size()); left_off.push_back(left.size());
        runs.insert(runs.end(), fo.runs.begin(), fo.runs.end());
        if (!tiles) rows.insert(rows.end(), fo.row_run.begin(), fo.row_run.end());
        seeds.insert(seeds.end(), fo.seeds.begin(), fo.seeds.end());
        tileidx.insert(tileidx.end(), fo.tile_idx.begin(), fo.tile_idx.end());
        left.insert(left.end(), fo.left.begin(), fo.left.end());
        iargs.push_back(a);
    }
    void launch(const Geometry& g, int band_rows, bool tiles, Uploader& up, hipStream_t stream) {
        if (iargs.empty()) return;
        d_runs.reserve(std::max<size_t>(runs.size(), 1) * sizeof(IRun));
        d_rows.reserve(std::max<size_t>(rows.size(), 1) * 4);
        d_seeds.reserve(std::max<size_t>(seeds.size(), 1) * 4);
        d_tileidx.reserve(std::max<size_t>(tileidx.size(), 1) * 4);
        d_left.reserve(std::max<size_t>(left.size(), 1) * 4);
        d_iargs.reserve(iargs.size() * sizeof(IFrameArgs));
        for (size_t k = 0; k < iargs.size(); ++k) {
            iargs[k].runs = static_cast<const IRun*>(d_runs.p) + run_off[k];
            iargs[k].row_run = static_cast<const uint32_t*>(d_rows.p) + row_off[k];
            iargs[k].seeds = static_cast<const uint32_t*>(d_seeds.p) + seed_off[k];
            iargs[k].tile_idx = static_cast<const uint32_t*>(d_tileidx.p) + tile_off[k];
            iargs[k].left = static_cast<const uint32_t*>(d_left.p) + left_off[k];
        }
        up(d_runs.p, runs.data(), runs.size() * sizeof(IRun));
        up(d_rows.p, rows.data(), rows.size() * 4);
        up(d_seeds.p, seeds.data(), seeds.size() * 4);
        up(d_tileidx.p, tileidx.data(), tileidx.size() * 4);
        up(d_left.p, left.data(), left.size() * 4);
        up(d_iargs.p, iargs.data(), iargs.size() * sizeof(IFrameArgs));
        if (tiles) launch_iframe_tiles(g, static_cast<const IFrameArgs*>(d_iargs.p), (int)iargs.size(), band_rows, stream);
        else launch_iframes(g, static_cast<const IFrameArgs*>(d_iargs.p), (int)iargs.size(), band_rows, stream);
        JSP_HIP(hipGetLastError());
        JSP_HIP(hipStreamSynchronize(stream));   // (the wave's tables are reused by the next wave)
    }
};

}  // namespace

extern "C" jsp_sp_index* jsp_sp_index_build(jsp_codec* c, int nframes, const uint8_t* const* srcs, const size_t* lens, const uint8_t* is_key,
                                            int key_row) {
    if (!c || !srcs || !lens) { set_error("sp_index: null argument"); return nullptr; }
    if (nframes < 1) { set_error("sp_index: empty range"); return nullptr; }
    if (key_row < 0) { set_error("sp_index: negative key_row"); return nullptr; }
    auto* lender = c->kind == JSP_CODEC_SCREENPRESSOR ? dynamic_cast<IndexLender*>(c) : nullptr;
    if (!lender) { set_error("sp_index: ScreenPressor only"); return nullptr; }
    for (int i = 0; i < nframes; ++i)
        if (!srcs[i] && lens[i]) { set_error("sp_index: null frame bytes"); return nullptr; }
    if (c->next_ticket != c->oldest_ticket) { set_error("sp_index: an asynchronous frame is in flight (jsp_wait for it first)"); return nullptr; }
    std::vector<HostFrame> hf((size_t)nframes);
    static const int32_t kSomewhere = 0;   // (a destination that is never written: it makes the host stage ask for its last column)
    for (int i = 0; i < nframes; ++i) hf[(size_t)i] = HostFrame{srcs[i], lens[i], is_key ? is_key[i] != 0 : true, &kSomewhere};
    if (!starts_group(hf[0])) { set_error("sp_index: the range must start at a coded key frame"); return nullptr; }
    try {
        c->activate();
        hipStream_t stream = c->stream;
        const Geometry g = lender->lend_geometry();
        auto idx = std::make_unique<jsp_sp_index>();
        idx->codec_serial = c->serial;
        idx->device = c->device;
        idx->geo = g;
        idx->geo.aligned16 = true;
        idx->nframes = nframes;
        idx->key_of.assign((size_t)nframes, 0);
        idx->key_slot.assign((size_t)nframes, 0);
        idx->slot_base.assign((size_t)nframes, 0);
        idx->significance.assign((size_t)nframes, 0);
        const size_t npix = (size_t)g.X * (size_t)g.Y, nblocks = (size_t)g.nbx * (size_t)g.nby;
        idx->pic_stride = (npix + 3) & ~size_t(3);

        // ---- layout of what stays: a picture per key frame, a table slot per other frame --------------------------------------
        int nkeys = 0;
        int64_t nslots = 0;
        for (int i = 0; i < nframes; ++i) {
            if (hf[(size_t)i].key) {
                idx->key_of[(size_t)i] = i;
                idx->key_slot[(size_t)i] = nkeys++;
            } else {
                idx->key_of[(size_t)i] = idx->key_of[(size_t)i - 1];
                idx->key_slot[(size_t)i] = idx->key_slot[(size_t)i - 1];
                idx->slot_base[(size_t)i] = nslots++ - i;
            }
        }
        const int nwords = (nframes + 31) / 32;
        idx->key_bytes = (uint64_t)nkeys * idx->pic_stride * sizeof(int32_t);
        idx->table_bytes = (uint64_t)nslots * nblocks * sizeof(PBlock);
        idx->bitmap_bytes = (uint64_t)nwords * nblocks * sizeof(uint32_t);
        exact(idx->d_keys, idx->key_bytes);
        exact(idx->d_blocks, idx->table_bytes);
        exact(idx->d_bitmap, idx->bitmap_bytes);
        std::vector<uint32_t> bitmap((size_t)nwords * nblocks, 0u);
        std::vector<uint32_t> payload;               // every literal of the range (the frames' sizes are known only once they are decoded)

        // ---- host decoders of the build's own, with the codec's Preinit and key-frame options -----------------------------------
        const bool tiles = iframe_tiles_ok(idx->geo);
        int band_rows = lender->lend_band_rows() >= 0 ? lender->lend_band_rows() : choose_band_rows(g, std::min(nkeys, 64));
        if (tiles && g.Y > iframe_tile_max_band_rows() && (band_rows <= 0 || band_rows > iframe_tile_max_band_rows())) band_rows = iframe_tile_max_band_rows();
        HostDecoder host(g.X, g.Y, g.bpp);
        host.adopt_settings(lender->lend_settings());
        host.set_iframe_layout(band_rows, tiles ? iframe_tile_span(idx->geo) : 0);
        host.set_key_compare_row(-1);
        std::vector<std::unique_ptr<HostDecoder>> spare;
        int threads = lender->lend_host_threads();
        if (threads <= 0) { threads = usable_cpus(); threads = threads < 1 ? 1 : (threads > 8 ? 8 : threads); }
        PictureColumns cols;
        cols.base = hf.data();
        cols.Y = g.Y;
        cols.cols.assign((size_t)nframes * (size_t)g.Y, 0);

        Uploader up(stream);
        KeyWave keys;
        std::vector<FrameOut> outs;
        std::vector<PBlock> table;
        for (int w0 = 0; w0 < nframes;) {   // waves as the codec's staging cuts them: up to `threads` groups of pictures, at most 64 frames
            int w1 = w0 + 1, groups = 1;
            while (w1 < nframes && w1 - w0 < 64) {
                if (starts_group(hf[(size_t)w1])) { if (groups == threads) break; ++groups; }
                ++w1;
            }
            if ((int)outs.size() < w1 - w0) outs.resize((size_t)(w1 - w0));
            decode_frames(host, spare, hf.data() + w0, w1 - w0, outs.data(), threads, false, &cols, true);
            keys.clear();
            for (int i = w0; i < w1; ++i) {
                FrameOut& fo = outs[(size_t)(i - w0)];
                if (fo.status != JSP_ZERO_STATE || fo.prev_cleared) {
                    set_error("sp_index: frame %d of the range: %s", i, fo.error ? fo.error : "the frame does not decode");
                    return nullptr;
                }
                if (hf[(size_t)i].key) {
                    if (fo.kind != FrameKind::Flat && fo.kind != FrameKind::Intra) {
                        set_error("sp_index: frame %d of the range: the key frame leaves no picture", i);
                        return nullptr;
                    }
                    keys.add(fo, static_cast<int32_t*>(idx->d_keys.p) + (size_t)idx->key_slot[(size_t)i] * idx->pic_stride, tiles);
                    continue;
                }
                idx->significance[(size_t)i] = fo.significant ? 1 : 0;
                if (fo.kind != FrameKind::Inter) continue;   // an unchanged frame: no bit of the bitmap is set, its slot is never read
                if (fo.blocks.size() != nblocks) throw std::runtime_error("sp_index: block table of unexpected size");
                const uint64_t base16 = payload.size() / 4;
                if (base16 + (fo.payload.size() + 3) / 4 > 0xFFFFFFFFull) {
                    set_error("sp_index: the range's literal pixels do not fit the records' 32-bit offsets (frame %d)", i);
                    return nullptr;
                }
                table.assign(fo.blocks.begin(), fo.blocks.end());
                uint32_t* word = bitmap.data() + (size_t)(i >> 5) * nblocks;
                for (size_t b = 0; b < nblocks; ++b) {
                    PBlock& pb = table[b];
                    if (!pb.flags) continue;
                    if ((pb.flags & PB_MOTION) || !(pb.flags & PB_DATA) || (pb.payload & 3u)) throw std::runtime_error("sp_index: a block that is not a literal rectangle");
                    pb.payload = (uint32_t)(base16 + pb.payload / 4);   // in 16-byte units of the index's payload
                    word[b] |= 1u << (i & 31);
                }
                up(static_cast<PBlock*>(idx->d_blocks.p) + (size_t)((int64_t)i + idx->slot_base[(size_t)i]) * nblocks, table.data(), nblocks * sizeof(PBlock));
                payload.insert(payload.end(), fo.payload.begin(), fo.payload.end());
                payload.resize((payload.size() + 3) & ~size_t(3), 0u);   // every frame's literals start on a 16-byte boundary (so does every rectangle)
            }
            keys.launch(idx->geo, band_rows, tiles, up, stream);
            w0 = w1;
        }
        idx->payload_bytes = payload.size() * sizeof(uint32_t);
        exact(idx->d_payload, idx->payload_bytes);
        up(idx->d_payload.p, payload.data(), idx->payload_bytes);
        up(idx->d_bitmap.p, bitmap.data(), idx->bitmap_bytes);

        // ---- key frames: frames_differ_significantly (Manager.hx:392-421), once -----------------------------------------------------
        std::vector<int> judged;   // key frames behind an inter frame: the picture before them against their own, from key_row on
        for (int i = 0; i < nframes; ++i) {
            if (!hf[(size_t)i].key) continue;
            if (i == 0) idx->significance[0] = 1;
            else if (hf[(size_t)i - 1].key)
                idx->significance[(size_t)i] = !(lens[i] == lens[i - 1] && (lens[i] == 0 || std::memcmp(srcs[i], srcs[i - 1], lens[i]) == 0));
            else judged.push_back(i);
        }
        if (!judged.empty()) {
            DeviceBuffer d_before, d_flags;
            d_before.reserve(idx->pic_stride * sizeof(int32_t));
            d_flags.reserve(judged.size() * sizeof(uint32_t));
            std::vector<uint32_t> flags(judged.size(), 0u);
            for (size_t j = 0; j < judged.size(); ++j) {
                const int i = judged[j];
                idx->show(i - 1, static_cast<int32_t*>(d_before.p), stream);
                JSP_HIP(hipGetLastError());
                launch_frames_differ(idx->key_picture(i), static_cast<const int32_t*>(d_before.p), (size_t)key_row * (size_t)g.X, npix,
                                     static_cast<uint32_t*>(d_flags.p) + j, stream);
                JSP_HIP(hipGetLastError());
            }
            JSP_HIP(hipMemcpyAsync(flags.data(), d_flags.p, flags.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
            JSP_HIP(hipStreamSynchronize(stream));
            for (size_t j = 0; j < judged.size(); ++j) idx->significance[(size_t)judged[j]] = flags[j] ? 1 : 0;
        }
        return idx.release();
    } catch (const std::exception& e) {
        set_error("%s", e.what());
        return nullptr;
    }
}

extern "C" int jsp_sp_index_show(jsp_codec* c, jsp_sp_index* idx, int t, int32_t* dst, int* significant_changes) {
    if (!c || !idx || !dst) return fail("sp_index_show: null argument");
    auto* lender = c->kind == JSP_CODEC_SCREENPRESSOR ? dynamic_cast<IndexLender*>(c) : nullptr;
    if (!lender) return fail("sp_index: ScreenPressor only");
    if (idx->codec_serial != c->serial) return fail("sp_index_show: the index was built by another codec");
    if (t < 0 || t >= idx->nframes) return fail("sp_index_show: t is outside the index");
    if (c->next_ticket != c->oldest_ticket) return fail("sp_index_show: an asynchronous frame is in flight (jsp_wait for it first)");
    if (dst == c->prev_caller || dst == c->prev_dev) return fail("sp_index_show: dst is the current previous frame");
    try {
        c->activate();
        if (!on_device(dst)) return fail("sp_index_show: dst must be a device frame buffer");
        idx->show(t, dst, c->stream);
        JSP_HIP(hipGetLastError());
        JSP_HIP(hipStreamSynchronize(c->stream));
        lender->forget_buffer(dst);   // (written behind the codec's back: its last column is asked for again)
        if (significant_changes) *significant_changes = idx->significance[(size_t)t];
        return JSP_ZERO_STATE;
    } catch (const std::exception& e) {
        set_error("%s", e.what());
        return JSP_ERROR_OCCURED;
    }
}

// ---- thumbnails: the preview that follows the pointer along the seek bar, a filmstrip or contact sheet of a screen recording — n
// frames of the index, each reduced scale x scale pixels to one, in ONE launch of sp_index_thumbs_kernel.  The full-size pictures never
// exist and no frame buffer is written, so the codec is lent its stream and nothing else (no forget_buffer either).
namespace {
// The thumbnail of an index at `scale`: false (error set) for a scale other than 4 / 8 / 16 or a picture too small for one pixel.
bool thumb_size(const jsp_sp_index* idx, int scale, const char* who, int& tw, int& th) {
    if (scale != 4 && scale != 8 && scale != 16) { set_error("%s: scale must be 4, 8 or 16", who); return false; }
    tw = idx->geo.X / scale;
    th = idx->geo.Y / scale;
    if (tw > 0 && th > 0) return true;
    set_error("%s: the picture is too small for a thumbnail at this scale", who);
    return false;
}
}  // namespace

extern "C" int jsp_sp_index_thumb_size(const jsp_sp_index* idx, int scale, int* width, int* height) {
    if (!idx || !width || !height) return fail("sp_index_thumb_size: null argument");
    int tw = 0, th = 0;
    if (!thumb_size(idx, scale, "sp_index_thumb_size", tw, th)) return JSP_ERROR_OCCURED;
    *width = tw;
    *height = th;
    return JSP_ZERO_STATE;
}

extern "C" int jsp_sp_index_thumbs(jsp_codec* c, jsp_sp_index* idx, int n, const int* frames, int scale, int cols, int32_t* out,
                                   size_t out_pixels) {
    if (!c || !idx || !frames || !out) return fail("sp_index_thumbs: null argument");
    if (c->kind != JSP_CODEC_SCREENPRESSOR || !dynamic_cast<IndexLender*>(c)) return fail("sp_index: ScreenPressor only");
    if (idx->codec_serial != c->serial) return fail("sp_index_thumbs: the index was built by another codec");
    if (n < 1 || n > 4096) return fail("sp_index_thumbs: n is outside 1..4096");
    for (int k = 0; k < n; ++k)
        if (frames[k] < 0 || frames[k] >= idx->nframes) return fail("sp_index_thumbs: a frame number is outside the index");
    int tw = 0, th = 0;
    if (!thumb_size(idx, scale, "sp_index_thumbs", tw, th)) return JSP_ERROR_OCCURED;
    if (cols < 1) return fail("sp_index_thumbs: cols must be at least 1");
    const uint64_t sheet = (uint64_t)cols * (uint64_t)tw * (uint64_t)((n + (int64_t)cols - 1) / cols) * (uint64_t)th;
    if ((uint64_t)out_pixels < sheet) return fail("sp_index_thumbs: out_pixels is smaller than the sheet");
    if (c->next_ticket != c->oldest_ticket) return fail("sp_index_thumbs: an asynchronous frame is in flight (jsp_wait for it first)");
    try {
        c->activate();
        if (!on_device(out)) return fail("sp_index_thumbs: out must be a device buffer");
        idx->h_thumb_recs.reserve(sizeof(IndexThumbRec) * (size_t)n);
        idx->d_thumb_recs.reserve(sizeof(IndexThumbRec) * (size_t)n);
        auto* recs = static_cast<IndexThumbRec*>(idx->h_thumb_recs.p);
        for (int k = 0; k < n; ++k) {
            const size_t t = (size_t)frames[k];
            recs[k] = IndexThumbRec{frames[k], idx->key_of[t], (uint32_t)idx->key_slot[t], 0u, idx->slot_base[t]};
        }
        JSP_HIP(hipMemcpyAsync(idx->d_thumb_recs.p, recs, sizeof(IndexThumbRec) * (size_t)n, hipMemcpyHostToDevice, c->stream));
        launch_index_thumbs(idx->geo, out, static_cast<const int32_t*>(idx->d_keys.p), idx->pic_stride,
                            static_cast<const IndexThumbRec*>(idx->d_thumb_recs.p), n, static_cast<const PBlock*>(idx->d_blocks.p),
                            static_cast<const uint32_t*>(idx->d_payload.p), static_cast<const uint32_t*>(idx->d_bitmap.p), scale, cols, c->stream);
        JSP_HIP(hipGetLastError());
        JSP_HIP(hipStreamSynchronize(c->stream));   // (the pinned records are free for the next call)
        return JSP_ZERO_STATE;
    } catch (const std::exception& e) {
        set_error("%s", e.what());
        return JSP_ERROR_OCCURED;
    }
}

// ---- windows: the windows jsp_display_present / jsp_display_present_area would show of n frames of the index, on one sheet, in ONE
// launch of sp_index_present_kernel.  As for the thumbnails the full-size pictures never exist and no frame buffer is written, so the
// codec is lent its stream and nothing else (no forget_buffer); the per-cell records are the thumbnails' and travel their way.
extern "C" int jsp_sp_index_present(jsp_codec* c, jsp_sp_index* idx, int n, const int* frames, int32_t* out, size_t out_ints, int win_w, int win_h,
                                    size_t out_pitch, int cols, double k, double dx, double dy, int mode, int filter, uint32_t background) {
    if (!c || !idx || !frames || !out) return fail("sp_index_present: null argument");
    if (c->kind != JSP_CODEC_SCREENPRESSOR || !dynamic_cast<IndexLender*>(c)) return fail("sp_index: ScreenPressor only");
    if (idx->codec_serial != c->serial) return fail("sp_index_present: the index was built by another codec");
    if (const char* why = index_present_refusal(n, out_ints, win_w, win_h, out_pitch, cols, k, dx, dy, mode, filter)) return fail("sp_index_present: %s", why);
    for (int i = 0; i < n; ++i)
        if (frames[i] < 0 || frames[i] >= idx->nframes) return fail("sp_index_present: a frame number is outside the index");
    if (c->next_ticket != c->oldest_ticket) return fail("sp_index_present: an asynchronous frame is in flight (jsp_wait for it first)");
    try {
        c->activate();
        if (!on_device(out)) return fail("sp_index_present: out must be a device buffer");
        idx->h_thumb_recs.reserve(sizeof(IndexThumbRec) * (size_t)n);
        idx->d_thumb_recs.reserve(sizeof(IndexThumbRec) * (size_t)n);
        auto* recs = static_cast<IndexThumbRec*>(idx->h_thumb_recs.p);
        for (int i = 0; i < n; ++i) {
            const size_t t = (size_t)frames[i];
            recs[i] = IndexThumbRec{frames[i], idx->key_of[t], (uint32_t)idx->key_slot[t], 0u, idx->slot_base[t]};
        }
        JSP_HIP(hipMemcpyAsync(idx->d_thumb_recs.p, recs, sizeof(IndexThumbRec) * (size_t)n, hipMemcpyHostToDevice, c->stream));
        const IndexPresentArgs a = index_present_args(out, n, idx->geo.X, idx->geo.Y, win_w, win_h, out_pitch, cols, k, dx, dy, filter, background, 16);
        launch_index_present(idx->geo, static_cast<const int32_t*>(idx->d_keys.p), idx->pic_stride, static_cast<const IndexThumbRec*>(idx->d_thumb_recs.p),
                             n, static_cast<const PBlock*>(idx->d_blocks.p), static_cast<const uint32_t*>(idx->d_payload.p),
                             static_cast<const uint32_t*>(idx->d_bitmap.p), a, mode, filter, c->stream);
        JSP_HIP(hipGetLastError());
        JSP_HIP(hipStreamSynchronize(c->stream));   // (the pinned records are free for the next call)
        return JSP_ZERO_STATE;
    } catch (const std::exception& e) {
        set_error("%s", e.what());
        return JSP_ERROR_OCCURED;
    }
}

// ---- tensors: the same windows as a model's input batch (jsp_index_tensor's contract), in ONE launch of sp_index_tensor_kernel: Present's
// kernel with another last step.  No sheet is written; the codec is lent its stream and nothing else, the records travel as for Present.
extern "C" int jsp_sp_index_tensor(jsp_codec* c, jsp_sp_index* idx, int n, const int* frames, void* out, size_t out_bytes, int win_w, int win_h,
                                   double k, double dx, double dy, int mode, int filter, uint32_t background, int dtype, int layout,
                                   const float* scale, const float* bias) {
    if (!c || !idx || !frames || !out) return fail("sp_index_tensor: null argument");
    if (c->kind != JSP_CODEC_SCREENPRESSOR || !dynamic_cast<IndexLender*>(c)) return fail("sp_index: ScreenPressor only");
    if (idx->codec_serial != c->serial) return fail("sp_index_tensor: the index was built by another codec");
    if (const char* why = index_tensor_refusal(n, out, out_bytes, win_w, win_h, k, dx, dy, mode, filter, dtype, layout, scale, bias))
        return fail("sp_index_tensor: %s", why);
    for (int i = 0; i < n; ++i)
        if (frames[i] < 0 || frames[i] >= idx->nframes) return fail("sp_index_tensor: a frame number is outside the index");
    if (c->next_ticket != c->oldest_ticket) return fail("sp_index_tensor: an asynchronous frame is in flight (jsp_wait for it first)");
    try {
        c->activate();
        if (!on_device(out)) return fail("sp_index_tensor: out must be a device buffer");
        idx->h_thumb_recs.reserve(sizeof(IndexThumbRec) * (size_t)n);
        idx->d_thumb_recs.reserve(sizeof(IndexThumbRec) * (size_t)n);
        auto* recs = static_cast<IndexThumbRec*>(idx->h_thumb_recs.p);
        for (int i = 0; i < n; ++i) {
            const size_t t = (size_t)frames[i];
            recs[i] = IndexThumbRec{frames[i], idx->key_of[t], (uint32_t)idx->key_slot[t], 0u, idx->slot_base[t]};
        }
        JSP_HIP(hipMemcpyAsync(idx->d_thumb_recs.p, recs, sizeof(IndexThumbRec) * (size_t)n, hipMemcpyHostToDevice, c->stream));
        const IndexPresentArgs a = index_present_args(nullptr, n, idx->geo.X, idx->geo.Y, win_w, win_h, (size_t)win_w, 1, k, dx, dy, filter, background, 16);
        const IndexTensorArgs ta = index_tensor_args(out, win_w, dtype, layout, scale, bias);
        launch_index_tensor(idx->geo, static_cast<const int32_t*>(idx->d_keys.p), idx->pic_stride, static_cast<const IndexThumbRec*>(idx->d_thumb_recs.p),
                            n, static_cast<const PBlock*>(idx->d_blocks.p), static_cast<const uint32_t*>(idx->d_payload.p),
                            static_cast<const uint32_t*>(idx->d_bitmap.p), a, ta, mode, filter, c->stream);
        JSP_HIP(hipGetLastError());
        JSP_HIP(hipStreamSynchronize(c->stream));   // (the pinned records are free for the next call)
        return JSP_ZERO_STATE;
    } catch (const std::exception& e) {
        set_error("%s", e.what());
        return JSP_ERROR_OCCURED;
    }
}

namespace {
// The per-frame table of the kernels that walk forward (Play, Activity) — an IndexPlayFrame per frame, then the key-frame mask — made by
// the first call that needs it, once.
void play_frames(jsp_sp_index* idx, hipStream_t stream) {
    if (idx->d_play_frames.p) return;
    const size_t nwords = ((size_t)idx->nframes + 31) / 32;
    const size_t bytes = idx->play_mask_offset() + nwords * sizeof(uint32_t);
    PinnedBuffer pin;
    pin.reserve(bytes);
    auto* recs = static_cast<IndexPlayFrame*>(pin.p);
    auto* mask = reinterpret_cast<uint32_t*>(static_cast<uint8_t*>(pin.p) + idx->play_mask_offset());
    std::fill(mask, mask + nwords, 0u);
    for (int f = 0; f < idx->nframes; ++f) {
        recs[f] = IndexPlayFrame{idx->key_of[(size_t)f], (uint32_t)idx->key_slot[(size_t)f], idx->slot_base[(size_t)f]};
        if (idx->key_of[(size_t)f] == f) mask[f >> 5] |= 1u << (f & 31);
    }
    DeviceBuffer d;
    exact(d, bytes);
    JSP_HIP(hipMemcpyAsync(d.p, pin.p, bytes, hipMemcpyHostToDevice, stream));
    JSP_HIP(hipStreamSynchronize(stream));   // (the pinned copy goes away here)
    std::swap(idx->d_play_frames.p, d.p);
    std::swap(idx->d_play_frames.cap, d.cap);
}
}  // namespace

// ---- playback: a run of frames of the index, carried forward in registers from the first one, in ONE launch of sp_index_play_kernel.
// Everything Show does to the codec, per destination: the buffers are written behind its back, so it forgets their last columns.
extern "C" int jsp_sp_index_play(jsp_codec* c, jsp_sp_index* idx, int first, int n, int stride, int32_t* const* dsts, int* significant_changes) {
    if (!c || !idx || !dsts) return fail("sp_index_play: null argument");
    auto* lender = c->kind == JSP_CODEC_SCREENPRESSOR ? dynamic_cast<IndexLender*>(c) : nullptr;
    if (!lender) return fail("sp_index: ScreenPressor only");
    if (idx->codec_serial != c->serial) return fail("sp_index_play: the index was built by another codec");
    if (n < 1 || n > 4096) return fail("sp_index_play: n is outside 1..4096");
    if (stride < 1) return fail("sp_index_play: stride must be at least 1");
    if (first < 0 || (int64_t)first + (int64_t)(n - 1) * (int64_t)stride >= (int64_t)idx->nframes) return fail("sp_index_play: the run is outside the index");
    for (int k = 0; k < n; ++k)
        if (!dsts[k]) return fail("sp_index_play: null argument (an entry of dsts)");
    if (c->next_ticket != c->oldest_ticket) return fail("sp_index_play: an asynchronous frame is in flight (jsp_wait for it first)");
    bool aligned16 = true;
    {
        std::vector<const int32_t*> sorted(dsts, dsts + n);
        std::sort(sorted.begin(), sorted.end());
        if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end()) return fail("sp_index_play: the same buffer twice in dsts");
        for (int k = 0; k < n; ++k) {
            if (dsts[k] == c->prev_caller || dsts[k] == c->prev_dev) return fail("sp_index_play: a buffer of dsts is the current previous frame");
            aligned16 = aligned16 && (reinterpret_cast<uintptr_t>(dsts[k]) & 15) == 0;
        }
    }
    try {
        c->activate();
        for (int k = 0; k < n; ++k)
            if (!on_device(dsts[k])) return fail("sp_index_play: every buffer of dsts must be a device frame buffer");
        hipStream_t stream = c->stream;
        play_frames(idx, stream);
        idx->h_play_dsts.reserve(sizeof(int32_t*) * (size_t)n);
        idx->d_play_dsts.reserve(sizeof(int32_t*) * (size_t)n);
        std::copy(dsts, dsts + n, static_cast<int32_t**>(idx->h_play_dsts.p));
        JSP_HIP(hipMemcpyAsync(idx->d_play_dsts.p, idx->h_play_dsts.p, sizeof(int32_t*) * (size_t)n, hipMemcpyHostToDevice, stream));
        launch_index_play(idx->geo, static_cast<int32_t* const*>(idx->d_play_dsts.p), aligned16, first, n, n == 1 ? 1 : stride,
                          static_cast<const int32_t*>(idx->d_keys.p), idx->pic_stride, static_cast<const IndexPlayFrame*>(idx->d_play_frames.p),
                          reinterpret_cast<const uint32_t*>(static_cast<const uint8_t*>(idx->d_play_frames.p) + idx->play_mask_offset()),
                          static_cast<const PBlock*>(idx->d_blocks.p), static_cast<const uint32_t*>(idx->d_payload.p),
                          static_cast<const uint32_t*>(idx->d_bitmap.p), stream);
        JSP_HIP(hipGetLastError());
        JSP_HIP(hipStreamSynchronize(stream));   // (the pinned destination list is free for the next call)
        for (int k = 0; k < n; ++k) {
            lender->forget_buffer(dsts[k]);       // (written behind the codec's back: their last columns are asked for again)
            if (significant_changes) significant_changes[k] = idx->significance[(size_t)first + (size_t)k * (size_t)stride];
        }
        return JSP_ZERO_STATE;
    } catch (const std::exception& e) {
        set_error("%s", e.what());
        return JSP_ERROR_OCCURED;
    }
}

// ---- activity: how many pixels of every 16x16 block each frame of a run changed (jsp_index_activity's contract), in ONE launch of
// sp_index_activity_kernel: Play's walk with a compare-and-count where Play has a store.  No picture is written, so the codec is lent
// its stream and nothing else (no forget_buffer); the per-frame table is Play's.
extern "C" int jsp_sp_index_activity_size(const jsp_sp_index* idx, int* cols, int* rows) {
    if (!idx || !cols || !rows) return fail("index_activity: null argument");
    *cols = idx->geo.nbx;
    *rows = idx->geo.nby;
    return JSP_ZERO_STATE;
}

extern "C" int jsp_sp_index_activity(jsp_codec* c, jsp_sp_index* idx, int first, int n, uint16_t* out, size_t out_elems) {
    if (!c || !idx || !out) return fail("index_activity: null argument");
    if (c->kind != JSP_CODEC_SCREENPRESSOR || !dynamic_cast<IndexLender*>(c)) return fail("sp_index: ScreenPressor only");
    if (idx->codec_serial != c->serial) return fail("index_activity: the index was built by another codec");
    if (n < 1 || n > 4096) return fail("index_activity: n is outside 1..4096");
    if (first < 0 || (int64_t)first + (int64_t)n > (int64_t)idx->nframes) return fail("index_activity: the run is outside the index");
    const uint64_t elems = (uint64_t)n * (uint64_t)idx->geo.nby * (uint64_t)idx->geo.nbx;
    if ((uint64_t)out_elems < elems) return fail("index_activity: out_elems is smaller than the map");
    if (reinterpret_cast<uintptr_t>(out) & 1) return fail("index_activity: out is not aligned to 2 bytes");
    if (c->next_ticket != c->oldest_ticket) return fail("index_activity: an asynchronous frame is in flight (jsp_wait for it first)");
    try {
        c->activate();
        if (!on_device(out)) return fail("index_activity: out must be a device buffer");
        hipStream_t stream = c->stream;
        play_frames(idx, stream);
        JSP_HIP(hipMemsetAsync(out, 0, elems * sizeof(uint16_t), stream));   // (the kernel stores the non-zero counts only)
        launch_index_activity(idx->geo, out, first, n, static_cast<const int32_t*>(idx->d_keys.p), idx->pic_stride,
                              static_cast<const IndexPlayFrame*>(idx->d_play_frames.p),
                              reinterpret_cast<const uint32_t*>(static_cast<const uint8_t*>(idx->d_play_frames.p) + idx->play_mask_offset()),
                              static_cast<const PBlock*>(idx->d_blocks.p), static_cast<const uint32_t*>(idx->d_payload.p),
                              static_cast<const uint32_t*>(idx->d_bitmap.p), stream);
        JSP_HIP(hipGetLastError());
        JSP_HIP(hipStreamSynchronize(stream));
        return JSP_ZERO_STATE;
    } catch (const std::exception& e) {
        set_error("%s", e.what());
        return JSP_ERROR_OCCURED;
    }
}

// ---- distance: how many pixels of every 16x16 block each frame of a run differs from ONE reference picture (jsp_index_distance's
// contract), in ONE launch of sp_index_distance_kernel: Activity's walk with another last step.  The launch writes every element, so no
// memset goes in front; the codec is lent its stream and nothing else, and the per-frame table is Play's.
extern "C" int jsp_sp_index_distance(jsp_codec* c, jsp_sp_index* idx, int ref_frame, const int32_t* ref_picture, int first, int n, uint16_t* out,
                                     size_t out_elems) {
    if (!c || !idx || !out) return fail("index_distance: null argument");
    if (c->kind != JSP_CODEC_SCREENPRESSOR || !dynamic_cast<IndexLender*>(c)) return fail("sp_index: ScreenPressor only");
    if (idx->codec_serial != c->serial) return fail("index_distance: the index was built by another codec");
    if (n < 1 || n > 4096) return fail("index_distance: n is outside 1..4096");
    if (first < 0 || (int64_t)first + (int64_t)n > (int64_t)idx->nframes) return fail("index_distance: the run is outside the index");
    if ((ref_picture != nullptr) != (ref_frame == JSP_REF_PICTURE)) return fail("index_distance: ref_frame and ref_picture disagree (JSP_REF_PICTURE goes with a picture, a frame with none)");
    if (!ref_picture && (ref_frame < -1 || ref_frame >= idx->nframes)) return fail("index_distance: ref_frame is outside -1..nframes-1");
    if (reinterpret_cast<uintptr_t>(ref_picture) & 3) return fail("index_distance: ref_picture is not aligned to 4 bytes");
    const uint64_t elems = (uint64_t)n * (uint64_t)idx->geo.nby * (uint64_t)idx->geo.nbx;
    if ((uint64_t)out_elems < elems) return fail("index_distance: out_elems is smaller than the map");
    if (reinterpret_cast<uintptr_t>(out) & 1) return fail("index_distance: out is not aligned to 2 bytes");
    if (c->next_ticket != c->oldest_ticket) return fail("index_distance: an asynchronous frame is in flight (jsp_wait for it first)");
    try {
        c->activate();
        if (!on_device(out)) return fail("index_distance: out must be a device buffer");
        if (ref_picture && !on_device(ref_picture)) return fail("index_distance: ref_picture must be a device frame buffer");
        hipStream_t stream = c->stream;
        play_frames(idx, stream);
        launch_index_distance(idx->geo, out, ref_frame, ref_picture, first, n, static_cast<const int32_t*>(idx->d_keys.p), idx->pic_stride,
                              static_cast<const IndexPlayFrame*>(idx->d_play_frames.p),
                              reinterpret_cast<const uint32_t*>(static_cast<const uint8_t*>(idx->d_play_frames.p) + idx->play_mask_offset()),
                              static_cast<const PBlock*>(idx->d_blocks.p), static_cast<const uint32_t*>(idx->d_payload.p),
                              static_cast<const uint32_t*>(idx->d_bitmap.p), stream);
        JSP_HIP(hipGetLastError());
        JSP_HIP(hipStreamSynchronize(stream));
        return JSP_ZERO_STATE;
    } catch (const std::exception& e) {
        set_error("%s", e.what());
        return JSP_ERROR_OCCURED;
    }
}

extern "C" int jsp_sp_index_significance(const jsp_sp_index* idx, int* out) {
    if (!idx || !out) return fail("sp_index_significance: null argument");
    std::copy(idx->significance.begin(), idx->significance.end(), out);
    return JSP_ZERO_STATE;
}

extern "C" int jsp_sp_index_info(const jsp_sp_index* idx, int* nframes, uint64_t* device_bytes, uint64_t* host_bytes) {
    if (!idx) return fail("sp_index_info: null index");
    if (nframes) *nframes = idx->nframes;
    if (device_bytes) *device_bytes = idx->device_bytes();
    if (host_bytes) *host_bytes = idx->host_bytes();
    return JSP_ZERO_STATE;
}

extern "C" void jsp_sp_index_destroy(jsp_sp_index* idx) {
    if (!idx) return;
    // device memory (and the pinned records of jsp_sp_index_thumbs) only: no stream, event or decoder of the codec is touched, so the
    // codec may be gone already
    (void)hipSetDevice(idx->device);
    delete idx;
}
