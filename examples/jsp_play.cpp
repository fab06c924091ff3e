// Manager.worker-equivalent decode loop in plain C++ over the C ABI: no Python, no torch —
// what a native host (or an hxcpp build of the player) would do with libjsplayer_amd.so.
//
//   jsp_play clip.avi            prints one line per frame:  index key|inter slot significant crc32
//   jsp_play clip.avi --present WxH[:zoom[:hpos:vpos]]
//                                the plain run, and every frame shown is also presented into a W x H device window (jsp_view_matrix +
//                                jsp_display_present, bilinear: zoom 0 = "Fit" (default), 1 = "100%", 2 = "200%"; view positions in 0..1,
//                                default 0.5 — Main.on_stage_resize, Main.hx:288-319); the lines end in the window's crc32
//   jsp_play clip.avi --present-area WxH[:zoom[:hpos:vpos]]
//                                the same with the window area-averaged (jsp_display_present_area): what Fit into a small window needs
//   jsp_play clip.avi --pipelined [--depth D]
//                                the same lines, decoded through jsp_decompress_*_async / jsp_wait with D frames in
//                                flight: the host stage of frame n+1 overlaps the uploads and kernels of frame n
//   jsp_play clip.avi --pipelined --quiet [--streams T] [--repeat R | --seconds S] [--depth D]
//                                end-to-end rate: T independent streams (threads, a codec instance each) play the clip R
//                                times (or over and over for S seconds, all streams for the same interval) from the file's
//                                bytes in pinned memory; prints one JSON line
//   ... --pipelined [--prefetch MB]  MSVideo1: the file's bytes go to the device in ranges of about MB megabytes (default 32), one range
//                                ahead of the one being decoded and every pass over the file anew (jsp_prefetch): the frames then queue
//                                no upload of their own.  --prefetch 0: a copy, or a read over the bus inside the kernel, per frame
//   jsp_play clip.avi --skip-stills   MSVideo1: frame 0, then skip to the next significant change until the end (Manager.SkipStills,
//                                one jsp_find_change per skip); prints "<index> <key|inter> <changed> <crc32>" per landing
//   jsp_play clip.avi --play-index FIRST[:COUNT[:STRIDE]]
//                                ScreenPressor: ONE seek index over the clip (jsp_sp_index_build), then frames FIRST, FIRST + STRIDE, ...
//                                (COUNT of them; default: to the end of the clip) out of it, ONE jsp_sp_index_play per batch of the
//                                pool's buffers; prints "<index> <key|inter> <significant> <crc32>" per frame, the plain run's values.
//   jsp_play clip.avi --index-run FIRST[:COUNT[:STRIDE]]
//                                MSVideo1: ONE seek index over the clip (jsp_index_build), then frames FIRST, FIRST + STRIDE, ... (COUNT
//                                of them; default: to the end of the clip) out of it, ONE jsp_index_play per batch of the pool's
//                                buffers; prints "<index> <key|inter> <significant> <crc32>" per frame, the plain run's values.
//   jsp_play clip.avi --step-back   ONE seek index over the clip (MSVideo1: jsp_index_build; ScreenPressor: jsp_sp_index_build and
//                                jsp_sp_index_show), then the last frame and every frame down
//                                to 0, one jsp_index_show each (Main.on_prevframe, Manager.hx:191-196); prints "<index> <key|inter>
//                                <changed> <crc32>" per frame — sorted, the plain run's frames, significance and CRCs
//   jsp_play clip.avi --activity [FIRST[:COUNT]]
//                                ONE seek index over the clip of either codec, built as for --step-back, then its activity map for frames
//                                FIRST .. FIRST + COUNT - 1 (default: the whole clip), ONE jsp_index_activity / jsp_sp_index_activity call
//                                per 4096 frames: prints "<frame> <changed pixels> <x,y,w,h of its non-zero 16x16 cells, display
//                                coordinates, or ->" per frame and "map <cols>x<rows>x<frames> <crc32 of the map's uint16 words>"
//   jsp_play clip.avi --distance REF[:FIRST[:COUNT]]
//                                the same index, then its distance map against the picture of frame REF (-1: the picture before frame
//                                0) for frames FIRST .. FIRST + COUNT - 1 (default: the whole clip), ONE jsp_index_distance /
//                                jsp_sp_index_distance call per 4096 frames: prints "<frame> <pixels that differ from REF's picture>" per
//                                frame, "zero <the frames at distance 0 ...>" and "map <cols>x<rows>x<frames> <crc32>".  Goes alone.
//   jsp_play clip.avi --cut FIRST[:COUNT] OUT.avi
//                                MSVideo1: the clip from frame FIRST on (COUNT frames; default: to the end) as an AVI file of its own.
//                                ONE seek index from the nearest key frame <= FIRST up to FIRST, ONE jsp_index_key_frame call (a key frame
//                                that decodes to frame FIRST's picture, made of the codes the clip holds; a FIRST that is a key frame
//                                is copied), the frames after it copied.  Then OUT.avi is played back through the ordinary decode loop:
//                                prints "<frame of the clip> <crc32 from OUT.avi> <crc32 from the clip>" per frame (the CRC-32 of the
//                                pixels that blocks cover) and exits with 1 on any difference
//   jsp_play clip.avi --thin FIRST[:COUNT[:STRIDE]] OUT.avi
//                                MSVideo1: frames FIRST, FIRST + STRIDE, ... of the clip (COUNT of them; default: as many as the clip
//                                holds; STRIDE default 8) as an AVI file of its own — a time-lapse.  ONE seek index from the nearest key
//                                frame <= FIRST up to the last frame kept; the first frame as for --cut; a later frame that is a key
//                                frame of the clip, or that follows the one before it directly, is copied; every other one is an inter
//                                frame that spans its gap, made of the codes the clip holds and skips, all of them from ONE
//                                jsp_index_delta_frames call.  Then OUT.avi is played back through the ordinary decode loop: prints
//                                "<frame of the clip> <crc32 from OUT.avi> <crc32 from the clip>" per frame kept and exits with 1 on any
//                                difference
//   jsp_play clip.avi --thin-tight FIRST[:COUNT[:STRIDE]] OUT.avi
//                                --thin with jsp_index_tight_frames in place of jsp_index_delta_frames: a block that a gap codes but
//                                whose pixels it does not change is dropped from the gap's frame.  The same playback, CRC check and
//                                exit status; OUT.avi is never longer than --thin's
//   jsp_play clip.avi --crop X:Y:W:H[:tight] FIRST[:COUNT[:STRIDE]] OUT.avi
//                                MSVideo1: the part X:Y:W:H of the picture (display coordinates, top row first) of the frames --thin
//                                would keep, as an AVI file of its own.  The rectangle is widened to whole 4x4 blocks and clipped to
//                                the block grid; prints "crop blocks <bx> <by> <bw> <bh> display <x> <y> <w> <h>", the rectangle used.
//                                ONE seek index from the nearest key frame <= FIRST; the first frame is a key pair, every other one the
//                                gap pair from the frame kept before it (":tight": JSP_CROP_TIGHT), jsp_index_crop_frames calls of at
//                                most 4096 pairs.  Then OUT.avi is played back through a decoder of its own size: prints "<frame of
//                                the clip> <crc32 from OUT.avi> <crc32 of that part of the clip's picture>" per frame kept and exits
//                                with 1 on any difference
//   jsp_play clip.avi --reverse FIRST[:COUNT[:STRIDE]][:tight] OUT.avi
//   jsp_play clip.avi --boomerang FIRST[:COUNT[:STRIDE]][:tight] OUT.avi
//                                MSVideo1: the frames --thin would keep, the whole picture, played BACKWARDS (--reverse: last kept
//                                frame first) or there and back (--boomerang: the last step returns to the first frame kept, so the
//                                file loops), as an AVI file of its own.  ONE seek index from the nearest key frame <= FIRST; the first
//                                frame is a key pair, every other one the pair from the frame before it in that order — a step back
//                                takes, for every block the frames in between coded, the code of its last writer up to the earlier
//                                frame (":tight": JSP_CROP_TIGHT) — all from ONE jsp_index_path_frames call (at most 4096 frames).
//                                Prints "reverse blocks ..." / "boomerang blocks ..." as --crop does, then OUT.avi is played back
//                                through a decoder of its own size: "<frame of the clip> <crc32 from OUT.avi> <crc32 of the clip's
//                                picture>" per frame written, and exits with 1 on any difference
//   jsp_play clip.avi --pan WxH[:loose] FIRST[:COUNT[:STRIDE]] OUT.avi
//                                MSVideo1: a rectangle of W x H pixels (rounded up to whole 4x4 blocks, clipped to the block grid)
//                                that FOLLOWS what the frames --thin would keep change, as an AVI file of its own.  ONE seek index from
//                                the nearest key frame <= FIRST and its activity map (jsp_index_activity); per frame kept the box of
//                                the non-zero cells since the frame kept before; the rectangle moves, on each axis, the least number of
//                                blocks that brings the box inside (centred on a box wider than itself; it starts centred on the first
//                                box, or on the picture).  The first frame is a key pair, every other one the pair from the rectangle at
//                                the frame kept before to the rectangle now, with JSP_CROP_TIGHT (":loose": without — a frame behind a
//                                move then codes every block); jsp_index_pan_frames calls of at most 4096 pairs.  Prints "pan blocks
//                                <bw> <bh>", then OUT.avi is played back through a decoder of its own size: "<frame of the clip> <bx>
//                                <by> <crc32 from OUT.avi> <crc32 of that rectangle of the clip's picture>" per frame kept, origins in
//                                blocks with block row 0 at the bottom; exits with 1 on any difference
//   jsp_play clip.avi --filmstrip N[:scale]
//                                ONE seek index over the clip (MSVideo1: jsp_index_build; ScreenPressor: jsp_sp_index_build), then ONE
//                                jsp_index_thumbs / jsp_sp_index_thumbs call for N frames spread evenly over it (frame (k * frames) / N for k < N), each reduced scale x scale pixels to one (4, 8 or 16; default
//                                8) — the seek bar's hover preview / a contact sheet (Main.on_mouse_move, Main.hx:1147-1215); prints
//                                "<frame> <crc32 of the thumbnail's words>" per thumbnail
//   jsp_play clip.avi --index-tensor WxH N[:filter[:dtype[:layout]]]
//                                ONE seek index over the clip of either codec, then ONE jsp_index_tensor / jsp_sp_index_tensor call: the N
//                                frames --index-present picks, each Fit into W x H, as a dense tensor (filter 0..2, default 2; dtype f32,
//                                f16, bf16 or u8, default f32; layout nchw or nhwc, default nchw; scale 1/255, bias 0); prints per frame
//                                its number and the CRC-32 of its slice of the tensor's bytes
//   jsp_play clip.avi --index-present WxH[:zoom[:hpos:vpos]] N[:filter]
//                                ONE seek index over the clip of either codec, then ONE jsp_index_present / jsp_sp_index_present call
//                                for N frames spread evenly over it (frame (k * frames) / N for k < N): the W x H window of --present
//                                (zoom 0 = Fit) of each, without a full-size frame, as one sheet of N cells; filter 0 nearest, 1
//                                bilinear (default), 2 area; prints "<frame> <crc32 of the cell's words>" per cell
//   jsp_play clip.avi --seek N   MSVideo1: frame N first, through ONE jsp_seek from the nearest key frame (DataLoader.hx:125-132;
//                                Manager.hx:216-259), then on frame by frame; the lines from N on carry the CRCs of a plain run
//   jsp_play a.avi,b.avi --pipelined --devices 0,1,... [--streams T] [--quiet ...]
//                                streams sharded one per GPU inside this process: stream s plays file s (mod their number) on
//                                device devices[s mod G], a host thread, a codec instance and a frame pool each; the per-device
//                                (frames, pixels) counters are summed through jsp_reduce_counters (RCCL all-reduce when it loads).
//                                Without --quiet every stream's per-frame lines are printed under a "# stream s device d file" header
//
// It restates, in this project's own words, only what touches the codec:
//   * the container facts that select and feed it (AVIParser.hx:42-88,142-171; ParserUtils.hx:24-27):
//     avih size / rate, strh fourcc, strf depth + palette, `00dc`/`00db` chunks of LIST movi padded to even size;
//   * the frame-buffer pool of NUM_BUFFERS + 1 device frames that never hands out the buffer holding the
//     previous frame (Manager.hx:114-118,424-443,470-477);
//   * the DecompressI / DecompressP protocol with its identity test (Manager.hx:499-524) and
//     frames_differ_significantly for key frames (Manager.hx:392-421): its pixel loop comes with the decode (option
//     "key_frame_compare", jsp_key_frame_differs / jsp_wait) — no pass of the player's own over the two frames.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <array>
#include <atomic>
#include <chrono>
#include <deque>
#include <string>
#include <thread>
#include <vector>

#include "jsplayer_amd.h"

namespace {
constexpr int kInsignificantLines = 36;   // Manager.hx:61
constexpr int kNumBuffers = 8;            // Main.hx:148

uint32_t le32(const uint8_t* p) { return p[0] | p[1] << 8 | p[2] << 16 | (uint32_t)p[3] << 24; }
uint32_t crc32(const uint8_t* p, size_t n) {
    static uint32_t table[256];
    if (!table[1])
        for (uint32_t i = 0; i < 256; ++i) {
            uint32_t c = i;
            for (int k = 0; k < 8; ++k) c = c & 1 ? 0xEDB88320u ^ (c >> 1) : c >> 1;
            table[i] = c;
        }
    uint32_t c = 0xFFFFFFFFu;
    for (size_t i = 0; i < n; ++i) c = table[(c ^ p[i]) & 0xFF] ^ (c >> 8);
    return c ^ 0xFFFFFFFFu;
}

struct Clip {
    int X = 0, Y = 0, bpp = 32, kind = JSP_CODEC_SCREENPRESSOR;
    uint32_t usec = 66667;                           // avih: microseconds per frame
    std::vector<uint8_t> palette;
    std::vector<std::pair<size_t, size_t>> frames;   // offset, padded size inside `bytes`
    std::vector<uint8_t> index_key;                  // idx1 key flags of the video chunks, in file order (empty: no index)
    struct Bytes {                                   // the file, in pinned host memory (jsp_host_alloc): uploads need no copy
        uint8_t* p = nullptr;
        size_t n = 0;
        const uint8_t* data() const { return p; }
        size_t size() const { return n; }
        ~Bytes() { jsp_host_free(p); }
        Bytes() = default;
        Bytes(const Bytes&) = delete;             // (owns pinned memory: a Clip is never copied)
        Bytes& operator=(const Bytes&) = delete;
    } bytes;
};

bool is_msvc(const uint8_t* f) {
    return !std::memcmp(f, "MSVC", 4) || !std::memcmp(f, "msvc", 4) || !std::memcmp(f, "CRAM", 4) || !std::memcmp(f, "\0\0\0\0", 4);
}

void walk(Clip& c, size_t lo, size_t hi, bool in_movi, uint8_t (&fourcc)[4], bool& video_stream, bool& have_video) {
    const uint8_t* d = c.bytes.data();
    for (size_t pos = lo; pos + 8 <= hi;) {
        const uint8_t* tag = d + pos;
        const size_t size = le32(d + pos + 4), body = pos + 8, padded = (size + 1) & ~size_t(1);
        if (!std::memcmp(tag, "LIST", 4)) {
            const bool movi = !std::memcmp(d + body, "movi", 4);
            walk(c, body + 4, std::min(body + size, hi), in_movi || movi, fourcc, video_stream, have_video);
        } else if (!std::memcmp(tag, "avih", 4)) {
            c.usec = le32(d + body);
            c.X = (int)le32(d + body + 32);
            c.Y = (int)le32(d + body + 36);
        } else if (!std::memcmp(tag, "strh", 4)) {
            video_stream = !std::memcmp(d + body, "vids", 4) && !have_video;
            if (video_stream) std::memcpy(fourcc, d + body + 4, 4);
        } else if (!std::memcmp(tag, "strf", 4) && video_stream) {
            c.bpp = d[body + 14] | d[body + 15] << 8;
            const uint8_t* f = std::memcmp(fourcc, "\0\0\0\0", 4) ? fourcc : d + body + 16;
            if (is_msvc(f)) c.kind = c.bpp == 8 ? JSP_CODEC_MSVIDEO1_8 : JSP_CODEC_MSVIDEO1_16;
            if (c.bpp == 8 && padded > 40) c.palette.assign(d + body + 40, d + body + padded);
            video_stream = false;
            have_video = true;
        } else if (in_movi && (!std::memcmp(tag, "00dc", 4) || !std::memcmp(tag, "00db", 4))) {
            c.frames.emplace_back(body, std::min(padded, c.bytes.size() - body));
        } else if (!std::memcmp(tag, "idx1", 4)) {   // AVIOLDINDEX: ckid, flags (0x10 = key frame), offset, size
            for (size_t e = body; e + 16 <= std::min(body + size, hi); e += 16)
                if (!std::memcmp(d + e, "00dc", 4) || !std::memcmp(d + e, "00db", 4)) c.index_key.push_back((le32(d + e + 4) & 0x10) ? 1 : 0);
        }
        pos = body + padded;
    }
}

bool load(const char* path, Clip& c) {
    FILE* f = std::fopen(path, "rb");
    if (!f) return false;
    std::fseek(f, 0, SEEK_END);
    const long n = std::ftell(f);
    std::fseek(f, 0, SEEK_SET);
    c.bytes.n = n > 0 ? (size_t)n : 0;
    c.bytes.p = static_cast<uint8_t*>(jsp_host_alloc(c.bytes.n + 64));
    const bool ok = c.bytes.p && n > 12 && std::fread(c.bytes.p, 1, (size_t)n, f) == (size_t)n;
    std::fclose(f);
    if (!ok || std::memcmp(c.bytes.data(), "RIFF", 4) || std::memcmp(c.bytes.data() + 8, "AVI ", 4)) return false;
    uint8_t fourcc[4] = {0, 0, 0, 0};
    bool video_stream = false, have_video = false;
    walk(c, 12, std::min(c.bytes.size(), (size_t)8 + le32(c.bytes.data() + 4)), false, fourcc, video_stream, have_video);
    if (c.index_key.size() != c.frames.size()) c.index_key.clear();   // an index that does not describe these chunks is ignored
    return c.X > 0 && c.Y > 0;
}
// Key flag of frame i as the loaders attach it: the index's when the file has one (DataLoader.hx:373-401), else
// (first frame) || IsKeyFrame(bytes) (DataLoaderAVISeq.hx:45).
bool frame_is_key(const Clip& c, jsp_codec* dec, size_t i) {
    if (!c.index_key.empty()) return c.index_key[i] != 0;
    return i == 0 || jsp_is_key_frame(dec, c.bytes.data() + c.frames[i].first, c.frames[i].second);
}

// ---- --cut ---------------------------------------------------------------------------------------------------------------------
void put16(std::vector<uint8_t>& v, uint32_t x) { v.push_back((uint8_t)x); v.push_back((uint8_t)(x >> 8)); }
void put32(std::vector<uint8_t>& v, uint32_t x) { put16(v, x); put16(v, x >> 16); }
void put_chunk(std::vector<uint8_t>& v, const char* tag, const uint8_t* p, size_t n) {
    v.insert(v.end(), tag, tag + 4);
    put32(v, (uint32_t)n);
    v.insert(v.end(), p, p + n);
    if (n & 1) v.push_back(0);
}
// A minimal AVI file with the video stream of `c` (its size, depth, palette and frame time; fourcc CRAM) and these frames:
// hdrl(avih, strl(strh, strf)), movi(00dc ...), idx1 with the key flags.
std::vector<uint8_t> avi_file(const Clip& c, const std::vector<std::pair<const uint8_t*, size_t>>& frames, const std::vector<uint8_t>& keys) {
    const uint32_t n = (uint32_t)frames.size();
    std::vector<uint8_t> avih, strh, strf, strl, hdrl, movi, idx1, body, file;
    for (uint32_t x : {c.usec, 0u, 0u, 0x10u, n, 0u, 1u, 0u, (uint32_t)c.X, (uint32_t)c.Y, 0u, 0u, 0u, 0u}) put32(avih, x);
    strh.insert(strh.end(), {'v', 'i', 'd', 's', 'C', 'R', 'A', 'M'});
    put32(strh, 0); put16(strh, 0); put16(strh, 0); put32(strh, 0);
    put32(strh, c.usec); put32(strh, 1000000);                       // scale / rate: frames per second = rate / scale
    for (uint32_t x : {0u, n, 0u, 0xFFFFFFFFu, 0u}) put32(strh, x);
    for (uint32_t x : {0u, 0u, (uint32_t)c.X, (uint32_t)c.Y}) put16(strh, x);
    const bool pal = c.bpp == 8;
    put32(strf, 40); put32(strf, (uint32_t)c.X); put32(strf, (uint32_t)c.Y); put16(strf, 1); put16(strf, (uint32_t)c.bpp);
    strf.insert(strf.end(), {'C', 'R', 'A', 'M'});
    for (uint32_t x : {0u, 0u, 0u, pal ? (uint32_t)c.palette.size() / 4 : 0u, 0u}) put32(strf, x);
    if (pal) strf.insert(strf.end(), c.palette.begin(), c.palette.end());
    strl.insert(strl.end(), {'s', 't', 'r', 'l'});
    put_chunk(strl, "strh", strh.data(), strh.size());
    put_chunk(strl, "strf", strf.data(), strf.size());
    hdrl.insert(hdrl.end(), {'h', 'd', 'r', 'l'});
    put_chunk(hdrl, "avih", avih.data(), avih.size());
    put_chunk(hdrl, "LIST", strl.data(), strl.size());
    movi.insert(movi.end(), {'m', 'o', 'v', 'i'});
    for (uint32_t i = 0; i < n; ++i) {
        idx1.insert(idx1.end(), {'0', '0', 'd', 'c'});
        put32(idx1, keys[i] ? 0x10u : 0u); put32(idx1, (uint32_t)movi.size()); put32(idx1, (uint32_t)frames[i].second);
        put_chunk(movi, "00dc", frames[i].first, frames[i].second);
    }
    body.insert(body.end(), {'A', 'V', 'I', ' '});
    put_chunk(body, "LIST", hdrl.data(), hdrl.size());
    put_chunk(body, "LIST", movi.data(), movi.size());
    put_chunk(body, "idx1", idx1.data(), idx1.size());
    file.insert(file.end(), {'R', 'I', 'F', 'F'});
    put32(file, (uint32_t)body.size());
    file.insert(file.end(), body.begin(), body.end());
    return file;
}

// The ordinary decode loop over frames 0 .. upto - 1 of `clip` on a codec and two frame buffers of its own (DecompressI for a key
// frame, DecompressP else, never into the previous frame): per frame the CRC-32 of the pixels of the picture shown that 4x4 blocks
// cover (the X % 4 / Y % 4 remainder pixels are in no MSVideo1 frame) — or, with rw > 0, of the pixels of stored rows ry .. ry + rh - 1,
// columns rx .. rx + rw - 1 (inside the covered part).  False: an error, printed.
// `at` (with rw > 0): frame i takes (rx, ry) from (*at)[i] where that entry exists.
bool covered_crcs(const Clip& clip, size_t upto, std::vector<uint32_t>& crcs, size_t rx = 0, size_t ry = 0, size_t rw = 0, size_t rh = 0,
                  const std::vector<std::pair<size_t, size_t>>* at = nullptr) {
    jsp_codec* dec = jsp_codec_create(clip.kind, clip.X, clip.Y, clip.bpp, clip.palette.empty() ? nullptr : clip.palette.data(), (int)clip.palette.size(), 0);
    jsp_pool* pool = dec ? jsp_pool_create(0, clip.X, clip.Y, 2) : nullptr;
    bool ok = dec && pool;
    if (!ok) std::fprintf(stderr, "jsp_codec_create / jsp_pool_create: %s\n", jsp_last_error());
    if (ok) jsp_preinit(dec, kInsignificantLines);
    const size_t npx = (size_t)clip.X * clip.Y, cw = rw ? rw : (size_t)(clip.X / 4) * 4, chh = rw ? rh : (size_t)(clip.Y / 4) * 4;
    std::vector<int32_t> host(npx), cov(cw * chh);
    crcs.clear();
    for (size_t i = 0; ok && i < upto; ++i) {
        const uint8_t* src = clip.bytes.data() + clip.frames[i].first;
        const size_t len = clip.frames[i].second;
        int32_t* dst = jsp_pool_buffer(pool, jsp_previous_frame(dec) == jsp_pool_buffer(pool, 0) ? 1 : 0);
        int32_t* shown = nullptr;
        int signif = 0;
        if (frame_is_key(clip, dec, i)) ok = jsp_decompress_i(dec, src, len, dst) == JSP_ZERO_STATE;
        else ok = jsp_decompress_p(dec, src, len, dst, &shown, &signif) == 0;
        if (!ok) { std::fprintf(stderr, "frame %zu: %s\n", i, jsp_last_error()); break; }
        shown = jsp_previous_frame(dec);
        if (shown && jsp_download(shown, host.data(), npx) != 0) { std::fprintf(stderr, "jsp_download: %s\n", jsp_last_error()); ok = false; break; }
        if (at && i < at->size()) rx = (*at)[i].first, ry = (*at)[i].second;
        for (size_t y = 0; shown && y < chh; ++y) std::memcpy(cov.data() + y * cw, host.data() + (ry + y) * (size_t)clip.X + rx, cw * 4);
        crcs.push_back(shown ? crc32(reinterpret_cast<const uint8_t*>(cov.data()), cov.size() * 4) : 0u);
    }
    if (pool) jsp_pool_destroy(pool);
    if (dec) jsp_codec_destroy(dec);
    return ok;
}
}  // namespace

// The same loop with up to `depth` frames in flight.  A slot is handed out when it is neither the previous frame of the
// last submitted frame, nor a destination in flight, nor showing a frame the oldest frame in flight may still be compared
// with.  Returns frames decoded, or -1.
// Throughput runs (--quiet): `warmup` untimed passes over the clip (the codec's buffers reach their size, the clocks ramp up), then every
// stream waits at `gate` and the timed passes begin together; *t0 / *t1 bracket this stream's timed passes.
struct Gate { std::atomic<int> waiting{0}; int parties = 1; };
using Clock = std::chrono::steady_clock;
// `seconds` > 0: the timed passes start the file over until that much time has passed since the gate opened and stop where they are (frames
// in flight are collected) — streams with files of different lengths then all run for the same interval.
// `sink`: the per-frame lines go there instead of stdout (several streams printing side by side).
// --prefetch MB (g_prefetch_bytes): the file's bytes go to the device in ranges of about that size, the range after the current one ahead of the frames being
// submitted (jsp_prefetch), every pass over the file anew; the frames' own uploads then fall away (MSVideo1; other codecs ignore it).
// what the streams' decoders counted (jsp_counter), summed when they are destroyed: frames re-run through the synchronous path, frames that shared a
// launch, frames that found their bytes in a prefetched range
std::atomic<long long> g_async_reruns{0}, g_paired_frames{0}, g_prefetched_frames{0};
size_t g_prefetch_bytes = 32u << 20;                     // (--prefetch 0: every frame finds its own way up)
long play_pipelined(const Clip& clip, int depth, int repeat, bool quiet, int warmup = 0, Gate* gate = nullptr, Clock::time_point* t0 = nullptr,
                    Clock::time_point* t1 = nullptr, int device = 0, double seconds = 0, std::string* sink = nullptr) {
    auto say = [&](const char* fmt, auto... a) {
        if (!sink) { std::printf(fmt, a...); return; }
        char line[256];
        std::snprintf(line, sizeof line, fmt, a...);
        *sink += line;
    };
    jsp_codec* dec = jsp_codec_create(clip.kind, clip.X, clip.Y, clip.bpp, clip.palette.empty() ? nullptr : clip.palette.data(),
                                      (int)clip.palette.size(), device);
    if (!dec) { std::fprintf(stderr, "jsp_codec_create: %s\n", jsp_last_error()); return -1; }
    jsp_preinit(dec, kInsignificantLines);
    if (clip.kind != JSP_CODEC_SCREENPRESSOR) {
        jsp_set_option(dec, "msv1_parse", "gpu");
        if (const char* form = std::getenv("JSP_PLAY_MSV1_ASYNC")) jsp_set_option(dec, "msv1_async", form);   // measurements: "two_launches"
    }
    char dbuf[16];
    std::snprintf(dbuf, sizeof dbuf, "%d", depth);
    jsp_set_option(dec, "async_depth", dbuf);
    std::snprintf(dbuf, sizeof dbuf, "%d", kInsignificantLines);
    if (!quiet) jsp_set_option(dec, "key_frame_compare", dbuf);   // key frames are compared with the frame before them as they are decoded
    jsp_pool* pool = jsp_pool_create(device, clip.X, clip.Y, kNumBuffers + 1 + depth);
    if (!pool) { std::fprintf(stderr, "jsp_pool_create: %s\n", jsp_last_error()); jsp_codec_destroy(dec); return -1; }
    const int nbuf = jsp_pool_count(pool);
    const size_t npx = (size_t)clip.X * clip.Y;
    std::vector<long> first(nbuf, -1), last(nbuf, -1);
    std::vector<int32_t> host(quiet ? 0 : npx);
    struct Flight { uint64_t ticket; size_t index; long gindex; bool key; int slot, prev_slot; int32_t* prev; bool cmp_bytes, first_ever; };
    std::deque<Flight> flying;
    long done = 0;
    bool failed = false;
    auto collect = [&] {
        const Flight f = flying.front();
        flying.pop_front();
        int32_t* shown_ptr = nullptr;
        int signif = -1, shown = f.slot;
        const int state = jsp_wait(dec, f.ticket, &shown_ptr, &signif);
        if (f.key) {
            if (state != JSP_ZERO_STATE) { if (!quiet) say("%zu key error %d %s\n", f.index, state, jsp_last_error()); return; }
            const int compared = signif;             // (option "key_frame_compare": the key frame against the frame before it)
            signif = -1;
            if (!quiet) {   // frames_differ_significantly, Manager.hx:392-421
                const uint8_t* src = clip.bytes.data() + clip.frames[f.index].first;
                const size_t len = clip.frames[f.index].second;
                if (f.first_ever) signif = 1;
                else if (f.cmp_bytes) {
                    const uint8_t* psrc = clip.bytes.data() + clip.frames[f.index - 1].first;
                    signif = !(clip.frames[f.index - 1].second == len && !std::memcmp(psrc, src, len));
                } else if (!f.prev) signif = 1;
                else signif = compared;
            }
        } else {
            if (state != JSP_ZERO_STATE) { if (!quiet) say("%zu inter raised %s\n", f.index, jsp_last_error()); return; }
            if (shown_ptr && shown_ptr == f.prev && f.prev_slot >= 0) shown = f.prev_slot;
            else if (!shown_ptr) shown = -1;
        }
        ++done;
        if (quiet) return;
        uint32_t crc = 0;
        if (shown >= 0 && jsp_download(jsp_pool_buffer(pool, shown), host.data(), npx) == 0)
            crc = crc32(reinterpret_cast<const uint8_t*>(host.data()), npx * 4);
        say("%zu %s %d %d %08x\n", f.index, f.key ? "key" : "inter", shown, signif, crc);
    };
    Clock::time_point deadline{};
    bool timed_out = false;
    if (seconds > 0) repeat = 1 << 30;
    struct Ahead { int pass; size_t begin, end; };          // frames [begin, end) of a pass whose bytes were handed to jsp_prefetch
    std::deque<Ahead> ahead;
    // A file that fits in ONE range and is played over and over: the next pass's range is the very bytes this pass is decoding from, and a frame
    // takes the NEWEST copy of its bytes (jsp_prefetch's rule) — so every pass would wait for an upload issued at its own start.  A player that reads
    // ahead has the next stretch of its file in ANOTHER buffer: passes alternate between two pinned copies of the file, the copy for pass p + 1 travels
    // while pass p is decoded from the other one.
    uint8_t* alt = nullptr;
    struct AltFree { uint8_t*& p; ~AltFree() { if (p) jsp_host_free(p); } } alt_free{alt};
    if (g_prefetch_bytes && clip.kind != JSP_CODEC_SCREENPRESSOR && !clip.frames.empty() && (repeat > 1 || seconds > 0 || warmup > 0)) {
        const size_t lo = clip.frames.front().first, hi = clip.frames.back().first + clip.frames.back().second;
        if (hi - lo <= g_prefetch_bytes) {
            alt = static_cast<uint8_t*>(jsp_host_alloc(clip.bytes.size() + 64));
            if (alt) std::memcpy(alt, clip.bytes.data(), clip.bytes.size());
        }
    }
    auto base = [&](int pass) -> const uint8_t* { return alt && (pass & 1) ? alt : clip.bytes.data(); };
    auto fetch = [&](int pass, size_t i0) {
        const size_t lo = clip.frames[i0].first;
        size_t j = i0, hi = lo;
        while (j < clip.frames.size() && (j == i0 || clip.frames[j].first + clip.frames[j].second - lo <= g_prefetch_bytes)) {
            hi = clip.frames[j].first + clip.frames[j].second;
            ++j;
        }
        if (jsp_prefetch(dec, base(pass) + lo, hi - lo) != 0) std::fprintf(stderr, "jsp_prefetch: %s\n", jsp_last_error());
        ahead.push_back({pass, i0, j});
    };
    for (int rep = -warmup; rep < repeat && !failed && !timed_out; ++rep) {
        if (rep == 0) {
            if (gate) { gate->waiting.fetch_add(1); while (gate->waiting.load() < gate->parties) std::this_thread::yield(); }
            const Clock::time_point now = Clock::now();
            if (t0) *t0 = now;
            deadline = now + std::chrono::duration_cast<Clock::duration>(std::chrono::duration<double>(seconds));
            done = 0;
        }
        bool last_was_key = false;
        for (size_t i = 0; i < clip.frames.size(); ++i) {
            if (seconds > 0 && rep >= 0 && Clock::now() >= deadline) { timed_out = true; break; }
            if ((int)flying.size() == depth) collect();
            if (g_prefetch_bytes && clip.kind != JSP_CODEC_SCREENPRESSOR) {
                while (!ahead.empty() && (ahead.front().pass != rep || i < ahead.front().begin || i >= ahead.front().end)) ahead.pop_front();
                if (ahead.empty()) fetch(rep, i);
                if (ahead.size() < 2) {                       // the range after this one travels while this one is decoded
                    const Ahead& b = ahead.back();
                    if (b.end < clip.frames.size()) fetch(b.pass, b.end);
                    else if (rep + 1 < repeat) fetch(b.pass + 1, 0);
                }
            }
            const uint8_t* src = base(rep) + clip.frames[i].first;
            const size_t len = clip.frames[i].second;
            const bool key = frame_is_key(clip, dec, i);
            int32_t* prev = jsp_previous_frame(dec);          // as of the last submitted frame
            int prev_slot = -1, slot = -1;
            for (int k = 0; k < nbuf; ++k) if (prev && jsp_pool_buffer(pool, k) == prev) prev_slot = k;
            const long gi = (long)((rep + warmup) * (long)clip.frames.size() + (long)i);
            const long horizon = flying.empty() ? gi : flying.front().gindex - 1;   // what may still be looked at
            {
                long oldest = 1L << 60;
                int victim = -1;
                for (int k = 0; k < nbuf && slot < 0; ++k) {
                    bool busy = k == prev_slot;
                    for (const Flight& f : flying) busy |= f.slot == k || f.prev_slot == k;
                    if (busy) continue;
                    if (first[k] < 0) slot = k;
                    else if (last[k] < horizon && first[k] < oldest) { oldest = first[k]; victim = k; }
                }
                if (slot < 0) { slot = victim; if (slot >= 0) first[slot] = last[slot] = -1; }
            }
            if (slot < 0) { std::fprintf(stderr, "no free frame buffer\n"); failed = true; break; }
            uint64_t ticket = 0;
            int32_t* dst = jsp_pool_buffer(pool, slot);
            const int rc = key ? jsp_decompress_i_async(dec, src, len, dst, &ticket) : jsp_decompress_p_async(dec, src, len, dst, &ticket);
            if (rc != 0) { std::fprintf(stderr, "submit: %s\n", jsp_last_error()); failed = true; break; }
            // which slot shows this frame is decided by the host stage: the previous frame after submission
            int32_t* now = jsp_previous_frame(dec);
            if (now == dst) first[slot] = last[slot] = gi;
            else if (now && now == prev && prev_slot >= 0) last[prev_slot] = gi;
            flying.push_back({ticket, i, gi, key, slot, prev_slot, prev, key && last_was_key && i > 0, rep == -warmup && i == 0});
            last_was_key = key;
        }
        while (!flying.empty()) collect();
    }
    if (t1) *t1 = Clock::now();
    for (auto [name, sum] : {std::pair<const char*, std::atomic<long long>*>{"async_reruns", &g_async_reruns}, {"paired_frames", &g_paired_frames},
                             {"prefetched_frames", &g_prefetched_frames}}) {
        const long long v = jsp_counter(dec, name);
        if (v > 0) sum->fetch_add(v);
    }
    jsp_pool_destroy(pool);
    jsp_codec_destroy(dec);
    return failed ? -1 : done;
}

// --batch B: the file through the batch calls (jsp_stage_batch / jsp_staged_decode), B frames at a time, every frame of a batch
// into a buffer of its own.  Prints what each frame shows as "<index> <key|inter> <adopted> <crc32>" (a frame that changes
// nothing shows the picture before it), or with --quiet plays the file `repeat` times and returns the frames decoded.
long play_batched(const Clip& clip, int batch, int repeat, bool quiet, int warmup = 0, double* seconds = nullptr) {
    jsp_codec* dec = jsp_codec_create(clip.kind, clip.X, clip.Y, clip.bpp, clip.palette.empty() ? nullptr : clip.palette.data(),
                                      (int)clip.palette.size(), 0);
    if (!dec) { std::fprintf(stderr, "jsp_codec_create: %s\n", jsp_last_error()); return -1; }
    jsp_preinit(dec, kInsignificantLines);
    if (clip.kind != JSP_CODEC_SCREENPRESSOR) jsp_set_option(dec, "msv1_parse", "gpu");
    jsp_pool* pool = jsp_pool_create(0, clip.X, clip.Y, batch + 1);     // + the picture carried over from the batch before
    if (!pool) { std::fprintf(stderr, "jsp_pool_create: %s\n", jsp_last_error()); jsp_codec_destroy(dec); return -1; }
    const size_t npx = (size_t)clip.X * clip.Y;
    std::vector<int32_t> host(quiet ? 0 : npx);
    std::vector<const uint8_t*> srcs(batch);
    std::vector<size_t> lens(batch);
    std::vector<uint8_t> keys(batch);
    std::vector<int32_t*> dsts(batch);
    std::vector<int> status(batch), adopted(batch), signif(batch);
    long done = 0;
    bool failed = false;
    jsp_staged* st = nullptr;
    auto t0 = std::chrono::steady_clock::now();
    for (int rep = -warmup; rep < repeat && !failed; ++rep) {
        if (rep == 0) { t0 = std::chrono::steady_clock::now(); done = 0; }   // (untimed passes first: buffers, clocks)
        int carry = batch;                                  // pool slot holding the last picture of the batch before (none yet: unused)
        bool have_picture = false;
        for (size_t f0 = 0; f0 < clip.frames.size() && !failed; f0 += batch) {
            const int n = (int)std::min<size_t>(batch, clip.frames.size() - f0);
            int slot = 0;
            for (int i = 0; i < n; ++i) {
                if (slot == carry) ++slot;                  // the picture the first inter frames are decoded against stays
                srcs[i] = clip.bytes.data() + clip.frames[f0 + i].first;
                lens[i] = clip.frames[f0 + i].second;
                keys[i] = frame_is_key(clip, dec, f0 + i) ? 1 : 0;
                dsts[i] = jsp_pool_buffer(pool, slot++);
            }
            jsp_staged* next = st ? jsp_restage_batch(dec, st, n, srcs.data(), lens.data(), keys.data(), dsts.data())
                                  : jsp_stage_batch(dec, n, srcs.data(), lens.data(), keys.data(), dsts.data());
            if (!next) { std::fprintf(stderr, "jsp_stage_batch: %s\n", jsp_last_error()); failed = true; break; }
            st = next;                                      // one batch object for the whole file: its buffers are taken over
            if (jsp_staged_decode(dec, st) != 0 || jsp_sync(dec) != 0) { std::fprintf(stderr, "decode: %s\n", jsp_last_error()); failed = true; }
            jsp_staged_results(st, status.data(), adopted.data(), signif.data());
            const int32_t* shown = have_picture ? jsp_pool_buffer(pool, carry) : nullptr;
            for (int i = 0; i < n && !failed; ++i) {
                if (adopted[i]) { shown = dsts[i]; have_picture = true; }
                ++done;
                if (quiet) continue;
                uint32_t crc = 0;
                if (shown && jsp_download(shown, host.data(), npx) == 0) crc = crc32(reinterpret_cast<const uint8_t*>(host.data()), npx * 4);
                std::printf("%zu %s %d %08x\n", f0 + i, keys[i] ? "key" : "inter", adopted[i], crc);
            }
            if (shown)
                for (int k = 0; k <= batch; ++k) if (jsp_pool_buffer(pool, k) == shown) carry = k;
        }
    }
    if (seconds) *seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (st) jsp_staged_destroy(st);
    jsp_pool_destroy(pool);
    jsp_codec_destroy(dec);
    return failed ? -1 : done;
}

int main(int argc, char** argv) {
    if (argc < 2) { std::fprintf(stderr, "usage: %s clip.avi [--pipelined [--depth D] [--quiet [--streams T] [--repeat R] [--warmup W]]] | --batch B [--quiet [--repeat R]] | --seek N | --skip-stills | --step-back | --filmstrip N[:scale] | --play-index FIRST[:COUNT[:STRIDE]] | --index-run FIRST[:COUNT[:STRIDE]] | --present WxH[:zoom[:hpos:vpos]] | --present-area WxH[:zoom[:hpos:vpos]] | --index-present WxH[:zoom[:hpos:vpos]] N[:filter] | --index-tensor WxH N[:filter[:dtype[:layout]]] | --transcode FIRST[:COUNT[:STRIDE]] OUT.avi | --proxy WxH FIRST[:COUNT[:STRIDE]] OUT.avi\n", argv[0]); return 2; }
    // (throughput runs: several files, separated by commas — stream s plays file s modulo their number, so that the streams of a
    // multi-stream run are independent inputs)
    std::deque<Clip> clips;                                   // (a deque: elements never move)
    {
        std::string list = argv[1];
        for (size_t at = 0; at <= list.size();) {
            const size_t comma = list.find(',', at);
            const std::string name = list.substr(at, comma == std::string::npos ? std::string::npos : comma - at);
            clips.emplace_back();
            if (!load(name.c_str(), clips.back())) { std::fprintf(stderr, "%s: not a RIFF/AVI file this player understands\n", name.c_str()); return 2; }
            if (comma == std::string::npos) break;
            at = comma + 1;
        }
    }
    const Clip& clip = clips[0];
    bool pipelined = false, quiet = false;
    int depth = 4, streams = 0, repeat = 1, warmup = 1, batch = 0, device = 0;
    double seconds = 0;
    long seek_to = -1;                                        // --seek N: frame N first, through jsp_seek
    bool skip_stills = false;                                 // --skip-stills: from frame 0, skip to each significant change (jsp_find_change)
    bool step_back = false;                                   // --step-back: a seek index over the clip, shown from the last frame down to 0
    long act_first = -1, act_count = -1;                      // --activity [FIRST[:COUNT]]: the activity map of a seek index over the clip
    bool dist = false;                                        // --distance REF[:FIRST[:COUNT]]: the distance map instead, against frame REF's picture
    long dist_ref = 0;
    long cut_first = -1, cut_count = -1;                      // --cut FIRST[:COUNT] OUT.avi: the clip from frame FIRST on as a file of its own
    std::string cut_path;
    bool thin_tight = false;   // --thin-tight: --thin with jsp_index_tight_frames
    long thin_first = -1, thin_count = -1, thin_stride = 8;   // --thin FIRST[:COUNT[:STRIDE]] OUT.avi: every STRIDE-th frame as a file of its own
    std::string thin_path;
    bool crop = false, crop_tight = false;   // --crop X:Y:W:H[:tight] FIRST[:COUNT[:STRIDE]] OUT.avi: --thin's frames, a part of the picture
    long crop_rect[4] = {0, 0, 0, 0};
    int path_mode = 0;                       // --reverse (1) / --boomerang (2) FIRST[:COUNT[:STRIDE]][:tight] OUT.avi: --thin's frames in another order (with crop, crop_tight)
    bool pan = false, pan_tight = true;      // --pan WxH[:loose] FIRST[:COUNT[:STRIDE]] OUT.avi: --thin's frames, a rectangle that follows the changes
    long pan_size[2] = {0, 0};
    int strip = 0, strip_scale = 8;                           // --filmstrip N[:scale]: N evenly spaced thumbnails of a seek index over the clip
    long play_first = -1, play_count = -1, play_stride = 1;   // --play-index FIRST[:COUNT[:STRIDE]]: frames played out of a ScreenPressor seek index
    long run_first = -1, run_count = -1, run_stride = 1;      // --index-run FIRST[:COUNT[:STRIDE]]: frames played out of an MSVideo1 seek index
    int present_w = 0, present_h = 0;                         // --present WxH[:zoom[:hpos:vpos]]: every frame shown also goes into a device window
    double present_zoom = 0, present_hpos = 0.5, present_vpos = 0.5;
    bool present_area = false;                                // --present-area: the window from jsp_display_present_area
    int ip_n = 0, ip_filter = JSP_PRESENT_BILINEAR;           // --index-present WxH[:zoom[:hpos:vpos]] N[:filter]: N windows out of a seek index, one sheet
    int it_dtype = -1, it_layout = JSP_TENSOR_NCHW;           // --index-tensor WxH N[:filter[:dtype[:layout]]]: the same N frames, Fit, as one dense tensor
    long tc_first = -1, tc_count = -1, tc_stride = 1;         // --transcode FIRST[:COUNT[:STRIDE]] OUT.avi: the pictures of those frames, encoded as 16-bit MSVideo1
    int proxy_w = 0, proxy_h = 0;                             // --proxy WxH FIRST[:COUNT[:STRIDE]] OUT.avi: the same of their windows, Fit into W x H
    std::string tc_path;
    std::vector<int> devices;                                 // --devices: streams sharded one per GPU (stream s -> devices[s mod G])
    for (int a = 2; a < argc; ++a) {
        const std::string o = argv[a];
        if (o == "--pipelined") pipelined = true;
        else if (o == "--quiet") quiet = true;
        else if (o == "--depth" && a + 1 < argc) depth = std::atoi(argv[++a]);
        else if (o == "--prefetch" && a + 1 < argc) g_prefetch_bytes = (size_t)(std::atof(argv[++a]) * 1048576.0);
        else if (o == "--streams" && a + 1 < argc) streams = std::atoi(argv[++a]);
        else if (o == "--repeat" && a + 1 < argc) repeat = std::atoi(argv[++a]);
        else if (o == "--seconds" && a + 1 < argc) seconds = std::atof(argv[++a]);
        else if (o == "--warmup" && a + 1 < argc) warmup = std::atoi(argv[++a]);
        else if (o == "--batch" && a + 1 < argc) batch = std::atoi(argv[++a]);
        else if (o == "--device" && a + 1 < argc) device = std::atoi(argv[++a]);
        else if (o == "--seek" && a + 1 < argc) seek_to = std::atol(argv[++a]);
        else if (o == "--skip-stills") skip_stills = true;
        else if (o == "--step-back") step_back = true;
        else if (o == "--activity") {
            if (dist) { std::fprintf(stderr, "--distance and --activity each go alone\n"); return 2; }
            act_first = 0;
            if (a + 1 < argc && argv[a + 1][0] >= '0' && argv[a + 1][0] <= '9') {
                const std::string v = argv[++a];
                const size_t colon = v.find(':');
                act_first = std::atol(v.substr(0, colon).c_str());
                if (colon != std::string::npos) act_count = std::atol(v.substr(colon + 1).c_str());
            }
        }
        else if (o == "--distance" && a + 1 < argc) {
            const std::string v = argv[++a];
            const size_t c1 = v.find(':'), c2 = c1 == std::string::npos ? c1 : v.find(':', c1 + 1);
            const bool numbers = !v.empty() && v.find_first_not_of("0123456789:-") == std::string::npos && v.find('-', 1) == std::string::npos &&
                                 v[0] != ':' && v.back() != ':' && v.find("::") == std::string::npos && v != "-";
            if (!numbers) { std::fprintf(stderr, "--distance REF[:FIRST[:COUNT]]: REF, FIRST and COUNT are numbers, REF >= -1 (got %s)\n", v.c_str()); return 2; }
            if (act_first >= 0) { std::fprintf(stderr, "--distance and --activity each go alone\n"); return 2; }
            dist = true;
            dist_ref = std::atol(v.substr(0, c1).c_str());
            act_first = c1 == std::string::npos ? 0 : std::atol(v.substr(c1 + 1, c2 == std::string::npos ? c2 : c2 - c1 - 1).c_str());
            if (c2 != std::string::npos) act_count = std::atol(v.substr(c2 + 1).c_str());
            if (act_first < 0 || (c2 != std::string::npos && act_count < 1)) { std::fprintf(stderr, "--distance REF[:FIRST[:COUNT]]: FIRST >= 0, COUNT >= 1\n"); return 2; }
        }
        else if (o == "--cut" && a + 2 < argc) {
            const std::string v = argv[++a];
            const size_t colon = v.find(':');
            cut_first = std::atol(v.substr(0, colon).c_str());
            if (colon != std::string::npos) cut_count = std::atol(v.substr(colon + 1).c_str());
            cut_path = argv[++a];
            if (cut_first < 0 || (colon != std::string::npos && cut_count < 1)) { std::fprintf(stderr, "--cut FIRST[:COUNT] OUT.avi: FIRST >= 0, COUNT >= 1\n"); return 2; }
        }
        else if ((o == "--thin" || o == "--thin-tight" || o == "--crop" || o == "--pan" || o == "--reverse" || o == "--boomerang") &&
                 a + (o == "--crop" || o == "--pan" ? 3 : 2) < argc) {
            thin_tight = o == "--thin-tight";
            if (o == "--reverse" || o == "--boomerang") {      // the whole picture through the --crop branch, frames in another order
                crop = true;
                path_mode = o == "--reverse" ? 1 : 2;
            }
            if (o == "--pan") {
                pan = true;
                std::string r = argv[++a];
                if (r.size() > 6 && r.compare(r.size() - 6, 6, ":loose") == 0) {
                    pan_tight = false;
                    r.resize(r.size() - 6);
                }
                char* end = nullptr;
                pan_size[0] = std::strtol(r.c_str(), &end, 10);
                const bool wide = end != r.c_str() && *end == 'x' && end[1];
                if (wide) pan_size[1] = std::strtol(end + 1, &end, 10);
                if (!wide || *end || pan_size[0] < 1 || pan_size[1] < 1) { std::fprintf(stderr, "--pan WxH[:loose] FIRST[:COUNT[:STRIDE]] OUT.avi: W >= 1, H >= 1\n"); return 2; }
            }
            if (o == "--crop") {
                crop = true;
                const std::string r = argv[++a];
                int got = 0;                                   // parts taken; 99: a part that is no number, or text behind ":tight"
                for (size_t at = 0; at <= r.size() && got < 99; at = std::min(r.find(':', at), r.size()) + 1) {
                    const std::string part = r.substr(at, std::min(r.find(':', at), r.size()) - at);
                    char* end = nullptr;
                    if (got < 4) {
                        crop_rect[got] = std::strtol(part.c_str(), &end, 10);
                        got = part.empty() || *end ? 99 : got + 1;
                    } else if (got == 4 && part == "tight") {
                        crop_tight = true;
                        got = 5;
                    } else got = 99;
                }
                if (got < 4 || got > 5 || crop_rect[2] < 1 || crop_rect[3] < 1) { std::fprintf(stderr, "--crop X:Y:W:H[:tight] FIRST[:COUNT[:STRIDE]] OUT.avi: W >= 1, H >= 1\n"); return 2; }
            }
            std::string v = argv[++a];
            if (path_mode && v.size() > 6 && v.compare(v.size() - 6, 6, ":tight") == 0) {   // (the frame spec's optional suffix)
                crop_tight = true;
                v.resize(v.size() - 6);
            }
            if (path_mode && (v.empty() || v.find_first_not_of("0123456789:") != std::string::npos || v.front() == ':' || v.back() == ':' ||
                              v.find("::") != std::string::npos || std::count(v.begin(), v.end(), ':') > 2)) {
                std::fprintf(stderr, "%s FIRST[:COUNT[:STRIDE]][:tight] OUT.avi: numbers, and no other suffix\n", o.c_str());
                return 2;
            }
            const size_t c1 = v.find(':'), c2 = c1 == std::string::npos ? c1 : v.find(':', c1 + 1);
            thin_first = std::atol(v.substr(0, c1).c_str());
            if (c1 != std::string::npos) thin_count = std::atol(v.substr(c1 + 1, c2 == std::string::npos ? c2 : c2 - c1 - 1).c_str());
            if (c2 != std::string::npos) thin_stride = std::atol(v.substr(c2 + 1).c_str());
            thin_path = argv[++a];
            if (thin_first < 0 || (c1 != std::string::npos && thin_count < 1) || thin_stride < 1) {
                std::fprintf(stderr, "%s FIRST[:COUNT[:STRIDE]] OUT.avi: FIRST >= 0, COUNT >= 1, STRIDE >= 1\n", o.c_str());
                return 2;
            }
        }
        else if ((o == "--transcode" && a + 2 < argc) || (o == "--proxy" && a + 3 < argc)) {
            if (o == "--proxy") {
                const std::string r = argv[++a];
                char* end = nullptr;
                proxy_w = (int)std::strtol(r.c_str(), &end, 10);
                if (end != r.c_str() && *end == 'x' && end[1]) proxy_h = (int)std::strtol(end + 1, &end, 10);
                if (proxy_w < 4 || proxy_h < 4 || proxy_w % 4 || proxy_h % 4 || *end) { std::fprintf(stderr, "--proxy WxH FIRST[:COUNT[:STRIDE]] OUT.avi: W and H positive multiples of 4\n"); return 2; }
            }
            const std::string v = argv[++a];
            const size_t c1 = v.find(':'), c2 = c1 == std::string::npos ? c1 : v.find(':', c1 + 1);
            tc_first = std::atol(v.substr(0, c1).c_str());
            if (c1 != std::string::npos) tc_count = std::atol(v.substr(c1 + 1, c2 == std::string::npos ? c2 : c2 - c1 - 1).c_str());
            if (c2 != std::string::npos) tc_stride = std::atol(v.substr(c2 + 1).c_str());
            tc_path = argv[++a];
            if (tc_first < 0 || (c1 != std::string::npos && tc_count < 1) || tc_stride < 1) {
                std::fprintf(stderr, "%s FIRST[:COUNT[:STRIDE]] OUT.avi: FIRST >= 0, COUNT >= 1, STRIDE >= 1\n", o.c_str());
                return 2;
            }
        }
        else if (o == "--filmstrip" && a + 1 < argc) {
            const std::string v = argv[++a];
            const size_t colon = v.find(':');
            strip = std::atoi(v.substr(0, colon).c_str());
            if (colon != std::string::npos) strip_scale = std::atoi(v.substr(colon + 1).c_str());
            if (strip < 1 || strip > 4096) { std::fprintf(stderr, "--filmstrip: N is 1..4096\n"); return 2; }
        }
        else if (o == "--play-index" && a + 1 < argc) {
            const std::string v = argv[++a];
            const size_t c1 = v.find(':'), c2 = c1 == std::string::npos ? std::string::npos : v.find(':', c1 + 1);
            play_first = std::atol(v.substr(0, c1).c_str());
            if (c1 != std::string::npos) play_count = std::atol(v.substr(c1 + 1, c2 == std::string::npos ? std::string::npos : c2 - c1 - 1).c_str());
            if (c2 != std::string::npos) play_stride = std::atol(v.substr(c2 + 1).c_str());
            if (play_first < 0 || (c1 != std::string::npos && play_count < 1) || play_stride < 1) { std::fprintf(stderr, "--play-index: FIRST >= 0, COUNT >= 1, STRIDE >= 1\n"); return 2; }
        }
        else if (o == "--index-run" && a + 1 < argc) {
            const std::string v = argv[++a];
            const size_t c1 = v.find(':'), c2 = c1 == std::string::npos ? std::string::npos : v.find(':', c1 + 1);
            run_first = std::atol(v.substr(0, c1).c_str());
            if (c1 != std::string::npos) run_count = std::atol(v.substr(c1 + 1, c2 == std::string::npos ? std::string::npos : c2 - c1 - 1).c_str());
            if (c2 != std::string::npos) run_stride = std::atol(v.substr(c2 + 1).c_str());
            if (run_first < 0 || (c1 != std::string::npos && run_count < 1) || run_stride < 1) { std::fprintf(stderr, "--index-run: FIRST >= 0, COUNT >= 1, STRIDE >= 1\n"); return 2; }
        }
        else if ((o == "--present" || o == "--present-area") && a + 1 < argc) {
            const std::string v = argv[++a];
            const int got = std::sscanf(v.c_str(), "%dx%d:%lf:%lf:%lf", &present_w, &present_h, &present_zoom, &present_hpos, &present_vpos);
            if ((got != 2 && got != 3 && got != 5) || present_w < 1 || present_h < 1) { std::fprintf(stderr, "%s: WxH[:zoom[:hpos:vpos]]\n", o.c_str()); return 2; }
            present_area = o == "--present-area";
        }
        else if (o == "--index-present" && a + 2 < argc) {
            const std::string v = argv[++a], m = argv[++a];
            const int got = std::sscanf(v.c_str(), "%dx%d:%lf:%lf:%lf", &present_w, &present_h, &present_zoom, &present_hpos, &present_vpos);
            const int got_n = std::sscanf(m.c_str(), "%d:%d", &ip_n, &ip_filter);
            if ((got != 2 && got != 3 && got != 5) || present_w < 1 || present_h < 1 || got_n < 1 || ip_n < 1 || ip_n > 4096 || ip_filter < 0 || ip_filter > 2) {
                std::fprintf(stderr, "--index-present: WxH[:zoom[:hpos:vpos]] N[:filter], N 1..4096, filter 0..2\n");
                return 2;
            }
        }
        else if (o == "--index-tensor" && a + 2 < argc) {
            const std::string v = argv[++a], m = argv[++a];
            char dt[8] = "f32", lay[8] = "nchw", tail = 0;
            ip_filter = JSP_PRESENT_AREA;
            const int got = std::sscanf(v.c_str(), "%dx%d%c", &present_w, &present_h, &tail);
            const int got_n = std::sscanf(m.c_str(), "%d:%d:%7[a-z0-9]:%7[a-z]%c", &ip_n, &ip_filter, dt, lay, &tail);
            const std::string d = dt, l = lay;
            it_dtype = d == "f32" ? JSP_TENSOR_F32 : d == "f16" ? JSP_TENSOR_F16 : d == "bf16" ? JSP_TENSOR_BF16 : d == "u8" ? JSP_TENSOR_U8 : -1;
            it_layout = l == "nchw" ? JSP_TENSOR_NCHW : l == "nhwc" ? JSP_TENSOR_NHWC : -1;
            if (got != 2 || present_w < 1 || present_h < 1 || got_n < 1 || got_n > 4 || ip_n < 1 || ip_n > 4096 || ip_filter < 0 || ip_filter > 2 || it_dtype < 0 ||
                it_layout < 0) {
                std::fprintf(stderr, "--index-tensor: WxH N[:filter[:dtype[:layout]]], N 1..4096, filter 0..2, dtype f32|f16|bf16|u8, layout nchw|nhwc\n");
                return 2;
            }
        }
        else if (o == "--devices" && a + 1 < argc) {
            const std::string list = argv[++a];
            for (size_t at = 0; at <= list.size();) {
                const size_t comma = list.find(',', at);
                devices.push_back(std::atoi(list.substr(at, comma == std::string::npos ? std::string::npos : comma - at).c_str()));
                if (comma == std::string::npos) break;
                at = comma + 1;
            }
        }
        else { std::fprintf(stderr, "unknown option %s\n", argv[a]); return 2; }
    }
    if (seek_to >= 0 && (pipelined || batch > 0 || !devices.empty())) { std::fprintf(stderr, "--seek goes with the plain per-frame run\n"); return 2; }
    if (skip_stills && (seek_to >= 0 || pipelined || batch > 0 || !devices.empty())) { std::fprintf(stderr, "--skip-stills goes alone\n"); return 2; }
    if (step_back && (skip_stills || seek_to >= 0 || pipelined || batch > 0 || !devices.empty())) { std::fprintf(stderr, "--step-back goes alone\n"); return 2; }
    if (act_first >= 0 && (run_first >= 0 || play_first >= 0 || ip_n > 0 || present_w > 0 || strip > 0 || step_back || skip_stills || seek_to >= 0 || pipelined || batch > 0 || !devices.empty())) { std::fprintf(stderr, "%s goes alone\n", dist ? "--distance" : "--activity"); return 2; }
    if (cut_first >= 0 && (act_first >= 0 || run_first >= 0 || play_first >= 0 || ip_n > 0 || present_w > 0 || strip > 0 || step_back || skip_stills || seek_to >= 0 || pipelined || batch > 0 || !devices.empty())) { std::fprintf(stderr, "--cut goes alone\n"); return 2; }
    if (cut_first >= 0 && clip.kind == JSP_CODEC_SCREENPRESSOR) { std::fprintf(stderr, "--cut: MSVideo1 only (a ScreenPressor key frame needs the entropy encoder)\n"); return 2; }
    if (thin_first >= 0 && (cut_first >= 0 || act_first >= 0 || run_first >= 0 || play_first >= 0 || ip_n > 0 || present_w > 0 || strip > 0 || step_back || skip_stills || seek_to >= 0 || pipelined || batch > 0 || !devices.empty())) { std::fprintf(stderr, "--thin goes alone\n"); return 2; }
    if (pan && crop) { std::fprintf(stderr, "--pan and %s do not go together\n", path_mode ? "--reverse / --boomerang" : "--crop"); return 2; }
    if (pan && clip.kind == JSP_CODEC_SCREENPRESSOR) { std::fprintf(stderr, "--pan: MSVideo1 only (ScreenPressor codes are entropy-coded in context)\n"); return 2; }
    const char* crop_opt = path_mode == 1 ? "--reverse" : path_mode == 2 ? "--boomerang" : "--crop";
    if (crop && clip.kind == JSP_CODEC_SCREENPRESSOR) { std::fprintf(stderr, "%s: MSVideo1 only (ScreenPressor codes are entropy-coded in context)\n", crop_opt); return 2; }
    if (thin_first >= 0 && clip.kind == JSP_CODEC_SCREENPRESSOR) { std::fprintf(stderr, "--thin: MSVideo1 only (a ScreenPressor frame needs the entropy encoder)\n"); return 2; }
    if (strip > 0 && (step_back || skip_stills || seek_to >= 0 || pipelined || batch > 0 || !devices.empty())) { std::fprintf(stderr, "--filmstrip goes alone\n"); return 2; }
    if (play_first >= 0 && (strip > 0 || step_back || skip_stills || seek_to >= 0 || pipelined || batch > 0 || !devices.empty())) { std::fprintf(stderr, "--play-index goes alone\n"); return 2; }
    if (play_first >= 0 && clip.kind != JSP_CODEC_SCREENPRESSOR) { std::fprintf(stderr, "--play-index: ScreenPressor only (an MSVideo1 index adopts: --seek and the plain run play on from any frame)\n"); return 2; }
    if (run_first >= 0 && (play_first >= 0 || strip > 0 || step_back || skip_stills || seek_to >= 0 || pipelined || batch > 0 || !devices.empty())) { std::fprintf(stderr, "--index-run goes alone\n"); return 2; }
    if (run_first >= 0 && clip.kind == JSP_CODEC_SCREENPRESSOR) { std::fprintf(stderr, "--index-run: MSVideo1 only (--play-index plays a ScreenPressor index)\n"); return 2; }
    if (ip_n > 0 && (run_first >= 0 || play_first >= 0 || strip > 0 || step_back || skip_stills || seek_to >= 0 || pipelined || batch > 0 || !devices.empty())) { std::fprintf(stderr, "%s goes alone\n", it_dtype >= 0 ? "--index-tensor" : "--index-present"); return 2; }
    if (ip_n == 0 && present_w > 0 && (run_first >= 0 || play_first >= 0 || strip > 0 || step_back || skip_stills || seek_to >= 0 || pipelined || batch > 0 || !devices.empty())) { std::fprintf(stderr, "--present goes with the plain per-frame run\n"); return 2; }
    if (tc_first >= 0 && (thin_first >= 0 || cut_first >= 0 || act_first >= 0 || run_first >= 0 || play_first >= 0 || ip_n > 0 || present_w > 0 || strip > 0 || step_back || skip_stills || seek_to >= 0 || pipelined || batch > 0 || !devices.empty())) { std::fprintf(stderr, "%s goes alone\n", proxy_w ? "--proxy" : "--transcode"); return 2; }
    if (tc_first >= 0 && clip.kind == JSP_CODEC_SCREENPRESSOR && clip.bpp == 16) { std::fprintf(stderr, "%s: a 16-bpp ScreenPressor clip holds 5-bit components, not 0x00RRGGBB words\n", proxy_w ? "--proxy" : "--transcode"); return 2; }
    if (batch > 0) {
        batch = batch > 1024 ? 1024 : batch;
        if (!quiet) return play_batched(clip, batch, 1, false) < 0 ? 1 : 0;
        double sec = 0;
        const long frames = play_batched(clip, batch, repeat, true, warmup, &sec);
        if (frames < 0) return 1;
        std::printf("{\"batch\": %d, \"frames\": %ld, \"seconds\": %.6f, \"mpixels_per_s\": %.1f}\n", batch, frames, sec,
                    frames * (double)clip.X * clip.Y / sec / 1e6);
        return 0;
    }
    if (!devices.empty()) {
        const int have = jsp_device_count();
        for (int d : devices)
            if (d < 0 || d >= have) { std::fprintf(stderr, "--devices: no device %d (%d visible)\n", d, have); return 2; }
        if (!pipelined || batch > 0) { std::fprintf(stderr, "--devices goes with --pipelined\n"); return 2; }
        if (streams <= 0) streams = (int)devices.size();      // one stream per listed device unless told otherwise
    }
    if (pipelined && !devices.empty() && !quiet) {
        // every stream prints what a single-device run of its file prints, under a header of its own
        depth = depth < 1 ? 1 : (depth > 16 ? 16 : depth);
        std::vector<std::string> lines(streams);
        std::vector<long> done(streams, 0);
        std::vector<std::thread> pool;
        for (int s = 0; s < streams; ++s)
            pool.emplace_back([&, s] {
                done[s] = play_pipelined(clips[(size_t)s % clips.size()], depth, 1, false, 0, nullptr, nullptr, nullptr,
                                         jsp_assign_stream(s, devices.data(), (int)devices.size()), 0, &lines[s]);
            });
        for (auto& t : pool) t.join();
        std::vector<uint64_t> per((size_t)devices.size() * 2, 0);
        for (int s = 0; s < streams; ++s) {
            if (done[s] < 0) return 1;
            const Clip& c = clips[(size_t)s % clips.size()];
            std::printf("# stream %d device %d file %zu\n%s", s, jsp_assign_stream(s, devices.data(), (int)devices.size()), (size_t)s % clips.size(), lines[s].c_str());
            per[2 * ((size_t)s % devices.size())] += (uint64_t)done[s];
            per[2 * ((size_t)s % devices.size()) + 1] += (uint64_t)done[s] * (uint64_t)c.X * (uint64_t)c.Y;
        }
        uint64_t total[2] = {0, 0};
        int via = 0;
        if (jsp_reduce_counters(devices.data(), (int)devices.size(), per.data(), total, &via) != JSP_ZERO_STATE) { std::fprintf(stderr, "counter reduce failed: %s\n", jsp_shard_last_error()); return 1; }
        std::printf("# total frames %llu pixels %llu reduce %s\n", (unsigned long long)total[0], (unsigned long long)total[1], via ? "rccl" : "host");
        return 0;
    }
    if (pipelined) {
        depth = depth < 1 ? 1 : (depth > 16 ? 16 : depth);
        if (!quiet) return play_pipelined(clip, depth, 1, false) < 0 ? 1 : 0;
        streams = streams < 1 ? 1 : streams;
        std::vector<long> done(streams, 0);
        std::vector<Clock::time_point> begin(streams), end(streams);
        std::vector<std::thread> pool;
        Gate gate;
        gate.parties = streams;
        for (int s = 0; s < streams; ++s)
            pool.emplace_back([&, s] {
                const int dev = devices.empty() ? device : jsp_assign_stream(s, devices.data(), (int)devices.size());
                done[s] = play_pipelined(clips[(size_t)s % clips.size()], depth, repeat, true, warmup, &gate, &begin[s], &end[s], dev, seconds);
            });
        for (auto& t : pool) t.join();
        Clock::time_point first = begin[0], last = end[0];
        for (int s = 1; s < streams; ++s) { if (begin[s] < first) first = begin[s]; if (end[s] > last) last = end[s]; }
        const double sec = std::chrono::duration<double>(last - first).count();
        long frames = 0;
        double compressed = 0;                                   // bytes handed to the decoders in the timed passes (what crosses the bus)
        for (int s = 0; s < streams; ++s) {
            if (done[s] < 0) return 1;
            frames += done[s];
            const Clip& c = clips[(size_t)s % clips.size()];
            double per_pass = 0;
            for (const auto& fr : c.frames) per_pass += (double)fr.second;
            compressed += per_pass * (c.frames.empty() ? 0.0 : (double)done[s] / (double)c.frames.size());
        }
        // streams sharded over several devices: the per-device counters, summed by the library (RCCL all-reduce when it loads)
        std::string shard;
        if (!devices.empty()) {
            std::vector<uint64_t> per(devices.size() * 2, 0);
            for (int s = 0; s < streams; ++s) {
                const Clip& c = clips[(size_t)s % clips.size()];
                per[2 * ((size_t)s % devices.size())] += (uint64_t)done[s];
                per[2 * ((size_t)s % devices.size()) + 1] += (uint64_t)done[s] * (uint64_t)c.X * (uint64_t)c.Y;
            }
            uint64_t total[2] = {0, 0};
            int via = 0;
            if (jsp_reduce_counters(devices.data(), (int)devices.size(), per.data(), total, &via) != JSP_ZERO_STATE || total[0] != (uint64_t)frames) {
                std::fprintf(stderr, "counter reduce failed: %s\n", jsp_shard_last_error());
                return 1;
            }
            shard = ", \"devices\": [";
            for (size_t i = 0; i < devices.size(); ++i) shard += (i ? ", " : "") + std::to_string(devices[i]);
            shard += "], \"per_device_frames\": [";
            for (size_t i = 0; i < devices.size(); ++i) shard += (i ? ", " : "") + std::to_string(per[2 * i]);
            shard += "], \"total_pixels\": " + std::to_string(total[1]) + ", \"counter_reduce\": \"" + (via ? "rccl" : "host") + "\"";
        }
        std::printf("{\"streams\": %d, \"files\": %zu, \"depth\": %d, \"frames\": %ld, \"warmup_passes\": %d, \"seconds\": %.6f, \"mpixels_per_s\": %.1f, "
                    "\"compressed_bytes\": %.0f, \"uploaded_bytes_per_s\": %.0f, \"async_reruns\": %lld, \"paired_frames\": %lld, \"prefetched_frames\": %lld%s}\n",
                    streams, clips.size(), depth, frames, warmup, sec, frames * (double)clip.X * clip.Y / sec / 1e6, compressed, compressed / sec,
                    g_async_reruns.load(), g_paired_frames.load(), g_prefetched_frames.load(), shard.c_str());
        return 0;
    }
    jsp_codec* dec = jsp_codec_create(clip.kind, clip.X, clip.Y, clip.bpp, clip.palette.empty() ? nullptr : clip.palette.data(),
                                      (int)clip.palette.size(), 0);
    if (!dec) { std::fprintf(stderr, "jsp_codec_create: %s\n", jsp_last_error()); return 1; }
    jsp_preinit(dec, kInsignificantLines);
    {
        char row[16];
        std::snprintf(row, sizeof row, "%d", kInsignificantLines);
        jsp_set_option(dec, "key_frame_compare", row);
    }
    jsp_pool* pool = jsp_pool_create(0, clip.X, clip.Y, kNumBuffers + 1);
    if (!pool) { std::fprintf(stderr, "jsp_pool_create: %s\n", jsp_last_error()); return 1; }
    const int nbuf = jsp_pool_count(pool);
    const size_t npx = (size_t)clip.X * clip.Y;
    std::vector<long> first(nbuf, -1), last(nbuf, -1);   // frames each slot currently shows (-1: free)
    std::vector<int32_t> host(npx);
    const uint8_t* prev_key = nullptr;
    size_t prev_key_len = 0;
    bool last_was_key = false;
    int rc = 0;
    size_t begin = 0;
    if (tc_first >= 0) {   // pictures that exist only as pixels, as a 16-bit MSVideo1 clip: one index build over the clip, the frames shown (--proxy: presented, Fit) a run at a time, jsp_msv1_encode_frames per run, the file, its playback
        const char* const opt = proxy_w ? "--proxy" : "--transcode";
        const size_t n = clip.frames.size();
        std::vector<int> keep;
        for (long i = tc_first; i < (long)n && (tc_count < 0 || (long)keep.size() < tc_count); i += tc_stride) keep.push_back((int)i);
        if (keep.empty() || (tc_count >= 0 && (long)keep.size() < tc_count)) {
            std::fprintf(stderr, "%s: frames %ld, %ld, ... (%ld of them) are not all in the clip (%zu frames)\n", opt, tc_first, tc_first + tc_stride, tc_count, n);
            rc = 1;
        }
        std::vector<const uint8_t*> srcs;
        std::vector<size_t> lens;
        std::vector<uint8_t> keys;
        for (size_t i = 0; rc == 0 && i <= (size_t)keep.back(); ++i) {
            srcs.push_back(clip.bytes.data() + clip.frames[i].first);
            lens.push_back(clip.frames[i].second);
            keys.push_back(i == 0 || frame_is_key(clip, dec, i) ? 1 : 0);
        }
        const bool sp = clip.kind == JSP_CODEC_SCREENPRESSOR;
        jsp_index* idx = rc == 0 && !sp ? jsp_index_build(dec, (int)srcs.size(), srcs.data(), lens.data(), keys.data(), kInsignificantLines) : nullptr;
        jsp_sp_index* sidx = rc == 0 && sp ? jsp_sp_index_build(dec, (int)srcs.size(), srcs.data(), lens.data(), keys.data(), kInsignificantLines) : nullptr;
        if (rc == 0 && !idx && !sidx) { std::fprintf(stderr, "%s: %s\n", sp ? "jsp_sp_index_build" : "jsp_index_build", jsp_last_error()); rc = 1; }
        const int W = proxy_w ? proxy_w : clip.X, H = proxy_w ? proxy_h : clip.Y;
        const int run = nbuf - 1;                                   // one buffer of the pool keeps the last picture of the run before
        const ptrdiff_t sheet_pitch = (ptrdiff_t)run * W;            // --proxy: a sheet of `run` cells in one row, two sheets in turn
        jsp_pool* sheets = rc == 0 && proxy_w ? jsp_pool_create(0, (int)sheet_pitch, H, 2) : nullptr;
        if (rc == 0 && proxy_w && !sheets) { std::fprintf(stderr, "jsp_pool_create: %s\n", jsp_last_error()); rc = 1; }
        jsp_encoder* enc = rc == 0 ? jsp_msv1_encoder_create(0, W, H) : nullptr;
        if (rc == 0 && !enc) { std::fprintf(stderr, "jsp_msv1_encoder_create: %s\n", jsp_last_error()); rc = 1; }
        size_t bound = 0;
        if (rc == 0) jsp_msv1_encode_bound(enc, &bound);
        double k = 1, dx = 0, dy = 0;
        if (rc == 0 && proxy_w && jsp_view_matrix(clip.X, clip.Y, W, H, 0.0, 0.5, 0.5, &k, &dx, &dy) != 0) { std::fprintf(stderr, "jsp_view_matrix: %s\n", jsp_last_error()); rc = 1; }
        std::vector<uint8_t> bytes;
        std::vector<size_t> out_lens;
        const int32_t* last_pic = nullptr;
        int spare = 0;                                              // the pool buffer (the sheet) that holds last_pic
        for (size_t k0 = 0, turn = 0; rc == 0 && k0 < keep.size(); k0 += (size_t)run, ++turn) {
            const int m = (int)std::min<size_t>((size_t)run, keep.size() - k0);
            std::vector<const int32_t*> pics, prevs;
            if (proxy_w) {
                int32_t* sheet = jsp_pool_buffer(sheets, (int)(turn & 1));
                const size_t ints = (size_t)sheet_pitch * H;
                const int prc = sp ? jsp_sp_index_present(dec, sidx, m, keep.data() + k0, sheet, ints, W, H, (size_t)sheet_pitch, run, k, dx, dy, JSP_DISPLAY_SETPIXELS, JSP_PRESENT_AREA, 0xFF000000u)
                                   : jsp_index_present(dec, idx, m, keep.data() + k0, sheet, ints, W, H, (size_t)sheet_pitch, run, k, dx, dy, JSP_DISPLAY_SETPIXELS, JSP_PRESENT_AREA, 0xFF000000u);
                if (prc != 0) { std::fprintf(stderr, "%s: %s\n", sp ? "jsp_sp_index_present" : "jsp_index_present", jsp_last_error()); rc = 1; break; }
                for (int i = 0; i < m; ++i) pics.push_back(sheet + (ptrdiff_t)(H - 1) * sheet_pitch + (ptrdiff_t)i * W);   // a cell by its last row
            } else {
                for (int i = 0, b = 0; i < m; ++i, ++b) {
                    if (last_pic && b == spare) ++b;
                    int32_t* dst = jsp_pool_buffer(pool, b);
                    int32_t* shown = nullptr;
                    int signif = 0;
                    const int src_rc = sp ? jsp_sp_index_show(dec, sidx, keep[k0 + i], dst, &signif) : jsp_index_show(dec, idx, keep[k0 + i], dst, 0, &shown, &signif);
                    if (src_rc != 0) { std::fprintf(stderr, "%s: %s\n", sp ? "jsp_sp_index_show" : "jsp_index_show", jsp_last_error()); rc = 1; break; }
                    pics.push_back(dst);
                    if (i == m - 1) spare = b;
                }
                if (rc != 0) break;
            }
            for (int i = 0; i < m; ++i) prevs.push_back(i == 0 ? last_pic : pics[i - 1]);
            std::vector<size_t> ls(m);
            size_t total = 0;
            const size_t at = bytes.size();
            bytes.resize(at + (size_t)m * bound);
            if (jsp_msv1_encode_frames(enc, m, pics.data(), prevs.data(), proxy_w ? -sheet_pitch : (ptrdiff_t)W, bytes.data() + at, (size_t)m * bound, ls.data(), &total, nullptr) != JSP_ZERO_STATE) {
                std::fprintf(stderr, "jsp_msv1_encode_frames: %s\n", jsp_last_error());
                rc = 1;
                break;
            }
            bytes.resize(at + total);
            out_lens.insert(out_lens.end(), ls.begin(), ls.end());
            last_pic = pics.back();
        }
        if (enc) jsp_msv1_encoder_destroy(enc);
        if (sheets) jsp_pool_destroy(sheets);
        if (idx) jsp_index_destroy(idx);
        if (sidx) jsp_sp_index_destroy(sidx);
        jsp_pool_destroy(pool);
        jsp_codec_destroy(dec);
        if (rc != 0) return rc;
        std::vector<std::pair<const uint8_t*, size_t>> out_frames;
        std::vector<uint8_t> out_keys;
        size_t at = 0;
        for (size_t j = 0; j < out_lens.size(); ++j) {
            out_frames.emplace_back(bytes.data() + at, out_lens[j]);
            out_keys.push_back(j == 0 ? 1 : 0);
            at += out_lens[j];
        }
        Clip head;                                                  // the stream the file describes: W x H, 16 bpp, the clip's frame time
        head.X = W; head.Y = H; head.bpp = 16; head.kind = JSP_CODEC_MSVIDEO1_16; head.usec = clip.usec;
        const std::vector<uint8_t> file = avi_file(head, out_frames, out_keys);
        FILE* f = std::fopen(tc_path.c_str(), "wb");
        if (!f || std::fwrite(file.data(), 1, file.size(), f) != file.size()) { std::fprintf(stderr, "cannot write %s\n", tc_path.c_str()); if (f) std::fclose(f); return 1; }
        std::fclose(f);
        // OUT.avi played back through the ordinary decode loop: frame, bytes, the CRC of its picture — and, where the encoder is exact
        // (--transcode of a 16-bit MSVideo1 clip), the CRC of the clip's own picture of that frame beside it
        Clip made;
        if (!load(tc_path.c_str(), made) || made.frames.size() != keep.size()) { std::fprintf(stderr, "cannot read %s back\n", tc_path.c_str()); return 1; }
        std::vector<uint32_t> got, want;
        if (!covered_crcs(made, made.frames.size(), got)) return 1;
        const bool exact = !proxy_w && clip.kind == JSP_CODEC_MSVIDEO1_16;
        if (exact && !covered_crcs(clip, (size_t)keep.back() + 1, want)) return 1;
        for (size_t j = 0; j < keep.size(); ++j) {
            if (exact) {
                std::printf("%d %zu %08x %08x\n", keep[j], out_lens[j], got[j], want[(size_t)keep[j]]);
                if (got[j] != want[(size_t)keep[j]]) rc = 1;
            } else std::printf("%d %zu %08x\n", keep[j], out_lens[j], got[j]);
        }
        return rc;
    }
    if (skip_stills) {   // Manager.SkipStills + SeekTo (Manager.hx:289-317), again and again: frame 0, then ONE jsp_find_change per skip
        const size_t n = clip.frames.size();
        std::vector<const uint8_t*> srcs;
        std::vector<size_t> lens;
        std::vector<uint8_t> keys;
        for (size_t i = 0; i < n; ++i) {
            srcs.push_back(clip.bytes.data() + clip.frames[i].first);
            lens.push_back(clip.frames[i].second);
            keys.push_back(i == 0 || frame_is_key(clip, dec, i) ? 1 : 0);
        }
        if (n && jsp_decompress_i(dec, srcs[0], lens[0], jsp_pool_buffer(pool, 0)) != JSP_ZERO_STATE) {
            std::fprintf(stderr, "frame 0: %s\n", jsp_last_error());
            rc = 1;
        }
        for (size_t shown = 0; rc == 0 && shown + 1 < n;) {
            const size_t s = shown + 1;   // the candidates: every frame after the one shown
            int32_t* dst = jsp_pool_buffer(pool, jsp_previous_frame(dec) == jsp_pool_buffer(pool, 0) ? 1 : 0);
            int found = -1, changed = 0;
            int32_t* data = nullptr;
            if (jsp_find_change(dec, (int)(n - s), srcs.data() + s, lens.data() + s, keys.data() + s, 0, keys[shown] ? srcs[shown] : nullptr,
                                keys[shown] ? lens[shown] : 0, kInsignificantLines, dst, &found, &changed, nullptr, &data) != JSP_ZERO_STATE) {
                std::fprintf(stderr, "jsp_find_change: %s\n", jsp_last_error());
                rc = 1;
                break;
            }
            shown = s + (size_t)found;
            uint32_t crc = 0;
            if (data && jsp_download(data, host.data(), npx) == 0) crc = crc32(reinterpret_cast<const uint8_t*>(host.data()), npx * 4);
            std::printf("%zu %s %d %08x\n", shown, keys[shown] ? "key" : "inter", changed, crc);
        }
        jsp_pool_destroy(pool);
        jsp_codec_destroy(dec);
        return rc;
    }
    if (step_back) {   // Main.on_prevframe from the last frame down to 0: one index build, then ONE jsp_index_show per step
        const size_t n = clip.frames.size();
        std::vector<const uint8_t*> srcs;
        std::vector<size_t> lens;
        std::vector<uint8_t> keys;
        for (size_t i = 0; i < n; ++i) {
            srcs.push_back(clip.bytes.data() + clip.frames[i].first);
            lens.push_back(clip.frames[i].second);
            keys.push_back(i == 0 || frame_is_key(clip, dec, i) ? 1 : 0);
        }
        if (clip.kind == JSP_CODEC_SCREENPRESSOR) {   // the host entropy stage once (jsp_sp_index_build), then ONE jsp_sp_index_show per step
            jsp_sp_index* sidx = n ? jsp_sp_index_build(dec, (int)n, srcs.data(), lens.data(), keys.data(), kInsignificantLines) : nullptr;
            if (n && !sidx) { std::fprintf(stderr, "jsp_sp_index_build: %s\n", jsp_last_error()); rc = 1; }
            for (size_t t = n; sidx && t-- > 0;) {
                int32_t* dst = jsp_pool_buffer(pool, (int)(t & 1));
                int signif = 0;
                if (jsp_sp_index_show(dec, sidx, (int)t, dst, &signif) != JSP_ZERO_STATE) {
                    std::fprintf(stderr, "jsp_sp_index_show: %s\n", jsp_last_error());
                    rc = 1;
                    break;
                }
                uint32_t crc = 0;
                if (jsp_download(dst, host.data(), npx) == 0) crc = crc32(reinterpret_cast<const uint8_t*>(host.data()), npx * 4);
                std::printf("%zu %s %d %08x\n", t, keys[t] ? "key" : "inter", signif, crc);
            }
            jsp_sp_index_destroy(sidx);
            jsp_pool_destroy(pool);
            jsp_codec_destroy(dec);
            return rc;
        }
        jsp_index* idx = n ? jsp_index_build(dec, (int)n, srcs.data(), lens.data(), keys.data(), kInsignificantLines) : nullptr;
        if (n && !idx) { std::fprintf(stderr, "jsp_index_build: %s\n", jsp_last_error()); rc = 1; }
        std::vector<int> sig(n, 0);
        if (idx) jsp_index_significance(idx, sig.data());
        for (size_t t = n; idx && t-- > 0;) {
            int32_t* dst = jsp_pool_buffer(pool, (int)(t & 1));
            int32_t* data = nullptr;
            int signif = 0;
            if (jsp_index_show(dec, idx, (int)t, dst, 0, &data, &signif) != JSP_ZERO_STATE) {
                std::fprintf(stderr, "jsp_index_show: %s\n", jsp_last_error());
                rc = 1;
                break;
            }
            uint32_t crc = 0;
            if (data && jsp_download(data, host.data(), npx) == 0) crc = crc32(reinterpret_cast<const uint8_t*>(host.data()), npx * 4);
            std::printf("%zu %s %d %08x\n", t, keys[t] ? "key" : "inter", sig[t], crc);
        }
        jsp_index_destroy(idx);
        jsp_pool_destroy(pool);
        jsp_codec_destroy(dec);
        return rc;
    }
    if (play_first >= 0) {   // play on from a shown frame: one index build, then ONE jsp_sp_index_play per batch of the pool's buffers
        const size_t n = clip.frames.size();
        std::vector<const uint8_t*> srcs;
        std::vector<size_t> lens;
        std::vector<uint8_t> keys;
        for (size_t i = 0; i < n; ++i) {
            srcs.push_back(clip.bytes.data() + clip.frames[i].first);
            lens.push_back(clip.frames[i].second);
            keys.push_back(i == 0 || frame_is_key(clip, dec, i) ? 1 : 0);
        }
        if ((size_t)play_first >= n) { std::fprintf(stderr, "--play-index %ld: the clip has %zu frames\n", play_first, n); rc = 2; }
        const long fits = rc == 0 ? ((long)n - 1 - play_first) / play_stride + 1 : 0;   // frames from FIRST to the end of the clip
        if (rc == 0 && play_count > fits) { std::fprintf(stderr, "--play-index: only %ld frames from %ld at stride %ld\n", fits, play_first, play_stride); rc = 2; }
        const long count = play_count < 0 ? fits : play_count;
        jsp_sp_index* sidx = rc == 0 ? jsp_sp_index_build(dec, (int)n, srcs.data(), lens.data(), keys.data(), kInsignificantLines) : nullptr;
        if (rc == 0 && !sidx) { std::fprintf(stderr, "jsp_sp_index_build: %s\n", jsp_last_error()); rc = 1; }
        std::vector<int32_t*> dsts;
        std::vector<int> signif((size_t)nbuf, 0);
        for (int k = 0; k < nbuf; ++k) dsts.push_back(jsp_pool_buffer(pool, k));
        for (long k0 = 0; rc == 0 && k0 < count; k0 += nbuf) {
            const int m = (int)(count - k0 < nbuf ? count - k0 : nbuf);
            const long f0 = play_first + k0 * play_stride;
            if (jsp_sp_index_play(dec, sidx, (int)f0, m, (int)play_stride, dsts.data(), signif.data()) != JSP_ZERO_STATE) {
                std::fprintf(stderr, "jsp_sp_index_play: %s\n", jsp_last_error());
                rc = 1;
                break;
            }
            for (int k = 0; k < m; ++k) {
                const size_t t = (size_t)(f0 + k * play_stride);
                uint32_t crc = 0;
                if (jsp_download(dsts[(size_t)k], host.data(), npx) == 0) crc = crc32(reinterpret_cast<const uint8_t*>(host.data()), npx * 4);
                std::printf("%zu %s %d %08x\n", t, keys[t] ? "key" : "inter", signif[(size_t)k], crc);
            }
        }
        jsp_sp_index_destroy(sidx);
        jsp_pool_destroy(pool);
        jsp_codec_destroy(dec);
        return rc;
    }
    if (run_first >= 0) {   // a run of frames out of an MSVideo1 index: one index build, then ONE jsp_index_play per batch of the pool's buffers
        const size_t n = clip.frames.size();
        std::vector<const uint8_t*> srcs;
        std::vector<size_t> lens;
        std::vector<uint8_t> keys;
        for (size_t i = 0; i < n; ++i) {
            srcs.push_back(clip.bytes.data() + clip.frames[i].first);
            lens.push_back(clip.frames[i].second);
            keys.push_back(i == 0 || frame_is_key(clip, dec, i) ? 1 : 0);
        }
        if ((size_t)run_first >= n) { std::fprintf(stderr, "--index-run %ld: the clip has %zu frames\n", run_first, n); rc = 2; }
        const long fits = rc == 0 ? ((long)n - 1 - run_first) / run_stride + 1 : 0;   // frames from FIRST to the end of the clip
        if (rc == 0 && run_count > fits) { std::fprintf(stderr, "--index-run: only %ld frames from %ld at stride %ld\n", fits, run_first, run_stride); rc = 2; }
        const long count = run_count < 0 ? fits : run_count;
        jsp_index* idx = rc == 0 ? jsp_index_build(dec, (int)n, srcs.data(), lens.data(), keys.data(), kInsignificantLines) : nullptr;
        if (rc == 0 && !idx) { std::fprintf(stderr, "jsp_index_build: %s\n", jsp_last_error()); rc = 1; }
        std::vector<int> sig(n, 0);   // the Manager's verdict per frame (what the plain run prints)
        if (idx) jsp_index_significance(idx, sig.data());
        std::vector<int32_t*> dsts, data((size_t)nbuf, nullptr);
        for (int k = 0; k < nbuf; ++k) dsts.push_back(jsp_pool_buffer(pool, k));
        for (long k0 = 0; rc == 0 && k0 < count; k0 += nbuf) {
            const int m = (int)(count - k0 < nbuf ? count - k0 : nbuf);
            const long f0 = run_first + k0 * run_stride;
            if (jsp_index_play(dec, idx, (int)f0, m, (int)run_stride, dsts.data(), -1, data.data(), nullptr) != JSP_ZERO_STATE) {
                std::fprintf(stderr, "jsp_index_play: %s\n", jsp_last_error());
                rc = 1;
                break;
            }
            for (int k = 0; k < m; ++k) {
                const size_t t = (size_t)(f0 + k * run_stride);
                uint32_t crc = 0;
                if (data[(size_t)k] && jsp_download(data[(size_t)k], host.data(), npx) == 0) crc = crc32(reinterpret_cast<const uint8_t*>(host.data()), npx * 4);
                std::printf("%zu %s %d %08x\n", t, keys[t] ? "key" : "inter", sig[t], crc);
            }
        }
        jsp_index_destroy(idx);
        jsp_pool_destroy(pool);
        jsp_codec_destroy(dec);
        return rc;
    }
    if (act_first >= 0) {   // where and when the picture changes: one index build, then ONE jsp_index_activity / jsp_sp_index_activity per 4096 frames
        const size_t n = clip.frames.size();
        std::vector<const uint8_t*> srcs;
        std::vector<size_t> lens;
        std::vector<uint8_t> keys;
        for (size_t i = 0; i < n; ++i) {
            srcs.push_back(clip.bytes.data() + clip.frames[i].first);
            lens.push_back(clip.frames[i].second);
            keys.push_back(i == 0 || frame_is_key(clip, dec, i) ? 1 : 0);
        }
        const bool sp = clip.kind == JSP_CODEC_SCREENPRESSOR;   // the same two calls on the index of either codec
        jsp_index* idx = n && !sp ? jsp_index_build(dec, (int)n, srcs.data(), lens.data(), keys.data(), kInsignificantLines) : nullptr;
        jsp_sp_index* sidx = n && sp ? jsp_sp_index_build(dec, (int)n, srcs.data(), lens.data(), keys.data(), kInsignificantLines) : nullptr;
        if (!idx && !sidx) { std::fprintf(stderr, "%s: %s\n", sp ? "jsp_sp_index_build" : "jsp_index_build", n ? jsp_last_error() : "no frames"); rc = 1; }
        const char* const call = dist ? (sp ? "jsp_sp_index_distance" : "jsp_index_distance") : sp ? "jsp_sp_index_activity" : "jsp_index_activity";
        int cols = 0, rows = 0;
        if (rc == 0 && (sp ? jsp_sp_index_activity_size(sidx, &cols, &rows) : jsp_index_activity_size(idx, &cols, &rows)) != JSP_ZERO_STATE) {
            std::fprintf(stderr, "%s_size: %s\n", call, jsp_last_error());
            rc = 1;
        }
        const long count = act_count >= 0 ? act_count : (long)n - act_first;
        if (rc == 0 && (count < 1 || act_first + count > (long)n)) { std::fprintf(stderr, "%s: frames %ld .. %ld are not all in the clip (%zu frames)\n", dist ? "--distance" : "--activity", act_first, act_first + count - 1, n); rc = 1; }
        if (rc == 0 && dist && (dist_ref < -1 || dist_ref >= (long)n)) { std::fprintf(stderr, "--distance: frame %ld is neither in the clip (%zu frames) nor -1\n", dist_ref, n); rc = 1; }
        const size_t cell = (size_t)cols * (size_t)rows;
        jsp_pool* sheet = nullptr;   // one "frame" that holds the map: cell ints a row, a row per two frames of the run
        if (rc == 0 && !(sheet = jsp_pool_create(0, (int)cell, (int)((count + 1) / 2), 1))) { std::fprintf(stderr, "jsp_pool_create: %s\n", jsp_last_error()); rc = 1; }
        if (rc == 0) {
            std::vector<int32_t> words(cell * (size_t)((count + 1) / 2));
            uint16_t* out = reinterpret_cast<uint16_t*>(jsp_pool_buffer(sheet, 0));
            for (long k = 0; rc == 0 && k < count; k += 4096) {
                const int m = (int)std::min<long>(4096, count - k);
                uint16_t* const at = out + (size_t)k * cell;
                const size_t room = (size_t)(count - k) * cell;
                const int f = (int)(act_first + k);
                const int got = dist ? (sp ? jsp_sp_index_distance(dec, sidx, (int)dist_ref, nullptr, f, m, at, room) : jsp_index_distance(dec, idx, (int)dist_ref, nullptr, f, m, at, room))
                                     : (sp ? jsp_sp_index_activity(dec, sidx, f, m, at, room) : jsp_index_activity(dec, idx, f, m, at, room));
                if (got != JSP_ZERO_STATE) {
                    std::fprintf(stderr, "%s: %s\n", call, jsp_last_error());
                    rc = 1;
                }
            }
            if (rc == 0 && jsp_download(jsp_pool_buffer(sheet, 0), words.data(), words.size()) != 0) { std::fprintf(stderr, "jsp_download: %s\n", jsp_last_error()); rc = 1; }
            const uint16_t* map = reinterpret_cast<const uint16_t*>(words.data());
            if (rc == 0 && dist) {   // per frame: the pixels that differ from the reference picture; then the frames that show it
                std::vector<long> same;
                for (long k = 0; k < count; ++k) {
                    long total = 0;
                    for (size_t e = 0; e < cell; ++e) total += map[(size_t)k * cell + e];
                    std::printf("%ld %ld\n", act_first + k, total);
                    if (total == 0) same.push_back(act_first + k);
                }
                std::printf("zero");
                for (long t : same) std::printf(" %ld", t);
                std::printf("\n");
            }
            for (long k = 0; rc == 0 && !dist && k < count; ++k) {   // per frame: changed pixels and the box of its non-zero cells, display coordinates (top row first)
                long total = 0;
                int q0 = cols, q1 = -1, r0 = rows, r1 = -1;
                for (int r = 0; r < rows; ++r)
                    for (int q = 0; q < cols; ++q) {
                        const uint16_t v = map[((size_t)k * (size_t)rows + (size_t)r) * (size_t)cols + (size_t)q];
                        if (!v) continue;
                        total += v;
                        q0 = std::min(q0, q); q1 = std::max(q1, q); r0 = std::min(r0, r); r1 = std::max(r1, r);
                    }
                if (q1 < 0) std::printf("%ld 0 -\n", act_first + k);
                else {
                    const int x0 = q0 * 16, x1 = std::min((q1 + 1) * 16, clip.X), y0 = r0 * 16, y1 = std::min((r1 + 1) * 16, clip.Y);
                    std::printf("%ld %ld %d,%d,%d,%d\n", act_first + k, total, x0, clip.Y - y1, x1 - x0, y1 - y0);
                }
            }
            if (rc == 0) std::printf("map %dx%dx%ld %08x\n", cols, rows, count, crc32(reinterpret_cast<const uint8_t*>(map), (size_t)count * cell * 2));
        }
        if (sheet) jsp_pool_destroy(sheet);
        jsp_sp_index_destroy(sidx);
        jsp_index_destroy(idx);
        jsp_pool_destroy(pool);
        jsp_codec_destroy(dec);
        return rc;
    }
    if (cut_first >= 0) {   // a clip that starts at any frame: one index build from the key frame before, ONE jsp_index_key_frame, the file, its playback
        const size_t n = clip.frames.size();
        const long count = cut_count >= 0 ? cut_count : (long)n - cut_first;
        if (count < 1 || cut_first + count > (long)n) { std::fprintf(stderr, "--cut: frames %ld .. %ld are not all in the clip (%zu frames)\n", cut_first, cut_first + count - 1, n); rc = 1; }
        std::vector<uint8_t> key_frame;
        if (rc == 0 && !frame_is_key(clip, dec, (size_t)cut_first)) {
            size_t k = (size_t)cut_first;
            while (k > 0 && !frame_is_key(clip, dec, k)) --k;   // the nearest key frame <= FIRST (frame 0 is one)
            std::vector<const uint8_t*> srcs;
            std::vector<size_t> lens;
            std::vector<uint8_t> keys;
            for (size_t i = k; i <= (size_t)cut_first; ++i) {
                srcs.push_back(clip.bytes.data() + clip.frames[i].first);
                lens.push_back(clip.frames[i].second);
                keys.push_back(i == k || frame_is_key(clip, dec, i) ? 1 : 0);
            }
            jsp_index* idx = jsp_index_build(dec, (int)srcs.size(), srcs.data(), lens.data(), keys.data(), kInsignificantLines);
            size_t bound = 0, len = 0;
            if (!idx) { std::fprintf(stderr, "jsp_index_build: %s\n", jsp_last_error()); rc = 1; }
            if (rc == 0 && jsp_index_key_frame_bound(idx, &bound) != JSP_ZERO_STATE) { std::fprintf(stderr, "jsp_index_key_frame_bound: %s\n", jsp_last_error()); rc = 1; }
            key_frame.resize(bound);
            if (rc == 0 && jsp_index_key_frame(dec, idx, (int)((size_t)cut_first - k), key_frame.data(), bound, &len) != JSP_ZERO_STATE) {
                std::fprintf(stderr, "jsp_index_key_frame: %s\n", jsp_last_error());
                rc = 1;
            }
            key_frame.resize(len);
            jsp_index_destroy(idx);
        }
        std::vector<std::pair<const uint8_t*, size_t>> out_frames;
        std::vector<uint8_t> out_keys;
        for (long i = cut_first; rc == 0 && i < cut_first + count; ++i) {   // the frames after the first: the clip's own, with their flags
            if (i == cut_first && !key_frame.empty()) out_frames.emplace_back(key_frame.data(), key_frame.size());
            else out_frames.emplace_back(clip.bytes.data() + clip.frames[(size_t)i].first, clip.frames[(size_t)i].second);
            out_keys.push_back(i == cut_first || frame_is_key(clip, dec, (size_t)i) ? 1 : 0);
        }
        jsp_pool_destroy(pool);
        jsp_codec_destroy(dec);
        if (rc != 0) return rc;
        const std::vector<uint8_t> file = avi_file(clip, out_frames, out_keys);
        FILE* f = std::fopen(cut_path.c_str(), "wb");
        if (!f || std::fwrite(file.data(), 1, file.size(), f) != file.size()) { std::fprintf(stderr, "cannot write %s\n", cut_path.c_str()); if (f) std::fclose(f); return 1; }
        std::fclose(f);
        // OUT.avi played back through the ordinary decode loop, beside the clip's own frames
        Clip cut;
        if (!load(cut_path.c_str(), cut) || cut.frames.size() != (size_t)count) { std::fprintf(stderr, "cannot read %s back\n", cut_path.c_str()); return 1; }
        std::vector<uint32_t> got, want;
        if (!covered_crcs(cut, cut.frames.size(), got) || !covered_crcs(clip, (size_t)(cut_first + count), want)) return 1;
        for (long k = 0; k < count; ++k) {
            std::printf("%ld %08x %08x\n", cut_first + k, got[(size_t)k], want[(size_t)(cut_first + k)]);
            if (got[(size_t)k] != want[(size_t)(cut_first + k)]) rc = 1;
        }
        return rc;
    }
    if (thin_first >= 0 && pan) {   // a rectangle that follows the changes: one index build, its activity map, jsp_index_pan_frames, the file, its playback
        const size_t n = clip.frames.size();
        std::vector<size_t> keep;
        for (long i = thin_first; i < (long)n && (thin_count < 0 || (long)keep.size() < thin_count); i += thin_stride) keep.push_back((size_t)i);
        if (keep.empty() || (thin_count >= 0 && (long)keep.size() < thin_count)) {
            std::fprintf(stderr, "--pan: frames %ld, %ld, ... (%ld of them) are not all in the clip (%zu frames)\n", thin_first, thin_first + thin_stride, thin_count, n);
            rc = 1;
        }
        const int nbx = clip.X / 4, nby = clip.Y / 4;
        const int bw = (int)std::min<long>((pan_size[0] + 3) / 4, nbx), bh = (int)std::min<long>((pan_size[1] + 3) / 4, nby);
        if (rc == 0 && (bw < 1 || bh < 1)) { std::fprintf(stderr, "--pan: the picture has no 4x4 block\n"); rc = 1; }
        if (rc == 0) std::printf("pan blocks %d %d\n", bw, bh);
        std::vector<uint8_t> made;
        std::vector<size_t> made_lens;
        std::vector<int> made_keys, xs, ys;                    // xs, ys: the rectangle's origin per frame kept, in blocks, table order
        if (rc == 0) {
            size_t k = keep[0];
            while (k > 0 && !frame_is_key(clip, dec, k)) --k;   // the nearest key frame <= FIRST (frame 0 is one)
            std::vector<const uint8_t*> srcs;
            std::vector<size_t> lens;
            std::vector<uint8_t> keys;
            for (size_t i = k; i <= keep.back(); ++i) {
                srcs.push_back(clip.bytes.data() + clip.frames[i].first);
                lens.push_back(clip.frames[i].second);
                keys.push_back(i == k || frame_is_key(clip, dec, i) ? 1 : 0);
            }
            jsp_index* idx = jsp_index_build(dec, (int)srcs.size(), srcs.data(), lens.data(), keys.data(), kInsignificantLines);
            if (!idx) { std::fprintf(stderr, "jsp_index_build: %s\n", jsp_last_error()); rc = 1; }
            // the activity map of the frames behind the first one kept: index frames keep[0] - k + 1 .. keep.back() - k
            int cols = 0, rows = 0;
            if (rc == 0 && jsp_index_activity_size(idx, &cols, &rows) != JSP_ZERO_STATE) { std::fprintf(stderr, "jsp_index_activity_size: %s\n", jsp_last_error()); rc = 1; }
            const long first = (long)(keep[0] - k) + 1, count = (long)(keep.back() - keep[0]);
            const size_t cell = (size_t)cols * (size_t)rows;
            std::vector<int32_t> words(cell * (size_t)((count + 1) / 2) + 1);
            jsp_pool* sheet = nullptr;
            if (rc == 0 && count > 0) {
                if (!(sheet = jsp_pool_create(0, (int)cell, (int)((count + 1) / 2), 1))) { std::fprintf(stderr, "jsp_pool_create: %s\n", jsp_last_error()); rc = 1; }
                uint16_t* out = sheet ? reinterpret_cast<uint16_t*>(jsp_pool_buffer(sheet, 0)) : nullptr;
                for (long q = 0; rc == 0 && q < count; q += 4096) {
                    const int m = (int)std::min<long>(4096, count - q);
                    if (jsp_index_activity(dec, idx, (int)(first + q), m, out + (size_t)q * cell, (size_t)(count - q) * cell) != JSP_ZERO_STATE) {
                        std::fprintf(stderr, "jsp_index_activity: %s\n", jsp_last_error());
                        rc = 1;
                    }
                }
                if (rc == 0 && jsp_download(jsp_pool_buffer(sheet, 0), words.data(), cell * (size_t)((count + 1) / 2)) != 0) { std::fprintf(stderr, "jsp_download: %s\n", jsp_last_error()); rc = 1; }
            }
            if (sheet) jsp_pool_destroy(sheet);
            // per frame kept behind the first: the box (x0, x1, y0, y1) in blocks of the non-zero cells since the frame kept before; x1 = 0: none
            const uint16_t* map = reinterpret_cast<const uint16_t*>(words.data());
            std::vector<std::array<int, 4>> boxes(keep.size(), std::array<int, 4>{0, 0, 0, 0});
            for (size_t j = 1; rc == 0 && j < keep.size(); ++j) {
                int q0 = cols, q1 = -1, r0 = rows, r1 = -1;
                for (size_t f = keep[j - 1] + 1; f <= keep[j]; ++f)
                    for (int r = 0; r < rows; ++r)
                        for (int q = 0; q < cols; ++q)
                            if (map[((f - keep[0] - 1) * (size_t)rows + (size_t)r) * (size_t)cols + (size_t)q]) {
                                q0 = std::min(q0, q); q1 = std::max(q1, q); r0 = std::min(r0, r); r1 = std::max(r1, r);
                            }
                if (q1 >= 0) boxes[j] = {q0 * 4, std::min((q1 + 1) * 4, nbx), r0 * 4, std::min((r1 + 1) * 4, nby)};
            }
            const auto floor_half = [](int v) { return v >= 0 ? v / 2 : -((1 - v) / 2); };
            const auto axis = [&](int p, int len, int b0, int b1, int room) {
                if (b1 - b0 > len) p = b0 + floor_half(b1 - b0 - len);
                else if (b0 < p) p = b0;
                else if (b1 > p + len) p = b1 - len;
                return std::max(0, std::min(p, room));
            };
            std::array<int, 4> start{0, nbx, 0, nby};           // centred on the first box, or on the picture
            for (size_t j = 1; j < keep.size(); ++j)
                if (boxes[j][1] > 0) { start = boxes[j]; break; }
            int x = std::max(0, std::min(start[0] + floor_half(start[1] - start[0] - bw), nbx - bw));
            int y = std::max(0, std::min(start[2] + floor_half(start[3] - start[2] - bh), nby - bh));
            for (size_t j = 0; j < keep.size(); ++j) {
                if (boxes[j][1] > 0) {
                    x = axis(x, bw, boxes[j][0], boxes[j][1], nbx - bw);
                    y = axis(y, bh, boxes[j][2], boxes[j][3], nby - bh);
                }
                xs.push_back(x);
                ys.push_back(y);
            }
            for (size_t g0 = 0; rc == 0 && g0 < keep.size(); g0 += 4096) {   // (a call takes 4096 pairs)
                const size_t m = std::min<size_t>(4096, keep.size() - g0);
                std::vector<int> from(m), to(m), from_xy(2 * m), to_xy(2 * m), ks(m);
                for (size_t i = 0; i < m; ++i) {
                    const size_t j = g0 + i, b = j == 0 ? 0 : j - 1;
                    from[i] = j == 0 ? JSP_CROP_KEY : (int)(keep[j - 1] - k);
                    to[i] = (int)(keep[j] - k);
                    from_xy[2 * i] = xs[b], from_xy[2 * i + 1] = ys[b];
                    to_xy[2 * i] = xs[j], to_xy[2 * i + 1] = ys[j];
                }
                std::vector<size_t> ls(m);
                size_t total = 0;
                const int flags = pan_tight ? JSP_CROP_TIGHT : 0;
                // asked twice: the lengths (cap 0 is a refusal that still sets them), then the bytes
                if (jsp_index_pan_frames(dec, idx, bw, bh, (int)m, from.data(), to.data(), from_xy.data(), to_xy.data(), flags, nullptr, 0, ls.data(), ks.data(), &total) == JSP_ZERO_STATE || total == 0) {
                    std::fprintf(stderr, "jsp_index_pan_frames: %s\n", jsp_last_error());
                    rc = 1;
                    break;
                }
                const size_t at = made.size();
                made.resize(at + total);
                if (jsp_index_pan_frames(dec, idx, bw, bh, (int)m, from.data(), to.data(), from_xy.data(), to_xy.data(), flags, made.data() + at, total, ls.data(), ks.data(), &total) != JSP_ZERO_STATE) {
                    std::fprintf(stderr, "jsp_index_pan_frames: %s\n", jsp_last_error());
                    rc = 1;
                }
                made_lens.insert(made_lens.end(), ls.begin(), ls.end());
                made_keys.insert(made_keys.end(), ks.begin(), ks.end());
            }
            if (idx) jsp_index_destroy(idx);
        }
        jsp_pool_destroy(pool);
        jsp_codec_destroy(dec);
        if (rc != 0) return rc;
        std::vector<std::pair<const uint8_t*, size_t>> out_frames;
        std::vector<uint8_t> out_keys;
        size_t at = 0;
        for (size_t j = 0; j < keep.size(); ++j) {
            out_frames.emplace_back(made.data() + at, made_lens[j]);
            out_keys.push_back(j == 0 || made_keys[j] ? 1 : 0);
            at += made_lens[j];
        }
        Clip header;                                            // the clip's stream at the rectangle's size
        header.X = 4 * bw, header.Y = 4 * bh, header.bpp = clip.bpp, header.kind = clip.kind, header.usec = clip.usec, header.palette = clip.palette;
        const std::vector<uint8_t> file = avi_file(header, out_frames, out_keys);
        FILE* f = std::fopen(thin_path.c_str(), "wb");
        if (!f || std::fwrite(file.data(), 1, file.size(), f) != file.size()) { std::fprintf(stderr, "cannot write %s\n", thin_path.c_str()); if (f) std::fclose(f); return 1; }
        std::fclose(f);
        // OUT.avi played back through the ordinary decode loop of a decoder of ITS size, beside the rectangle of the clip's own pictures
        Clip panned;
        if (!load(thin_path.c_str(), panned) || panned.frames.size() != keep.size() || panned.X != 4 * bw || panned.Y != 4 * bh) { std::fprintf(stderr, "cannot read %s back\n", thin_path.c_str()); return 1; }
        std::vector<std::pair<size_t, size_t>> origins(keep.back() + 1, {0, 0});
        for (size_t j = 0; j < keep.size(); ++j) origins[keep[j]] = {4 * (size_t)xs[j], 4 * (size_t)ys[j]};
        std::vector<uint32_t> got, want;
        if (!covered_crcs(panned, panned.frames.size(), got) || !covered_crcs(clip, keep.back() + 1, want, 0, 0, 4 * (size_t)bw, 4 * (size_t)bh, &origins)) return 1;
        for (size_t j = 0; j < keep.size(); ++j) {
            std::printf("%zu %d %d %08x %08x\n", keep[j], xs[j], ys[j], got[j], want[keep[j]]);
            if (got[j] != want[keep[j]]) rc = 1;
        }
        return rc;
    }
    if (thin_first >= 0 && crop) {   // a part of the picture: one index build from the key frame before, jsp_index_crop_frames for a key pair and every gap, the file, its playback
        // (--reverse / --boomerang: the whole picture, the frames kept in another order, ONE jsp_index_path_frames call)
        const size_t n = clip.frames.size();
        std::vector<size_t> keep;
        for (long i = thin_first; i < (long)n && (thin_count < 0 || (long)keep.size() < thin_count); i += thin_stride) keep.push_back((size_t)i);
        if (keep.empty() || (thin_count >= 0 && (long)keep.size() < thin_count)) {
            std::fprintf(stderr, "%s: frames %ld, %ld, ... (%ld of them) are not all in the clip (%zu frames)\n", crop_opt, thin_first, thin_first + thin_stride, thin_count, n);
            rc = 1;
        }
        std::vector<size_t> order = keep;                       // the frames written, in the file's order
        if (path_mode) {
            std::reverse(order.begin(), order.end());
            if (path_mode == 2) order.insert(order.begin(), keep.begin(), keep.end() - (keep.empty() ? 0 : 1));
            crop_rect[0] = crop_rect[1] = 0, crop_rect[2] = clip.X, crop_rect[3] = clip.Y;
            if (rc == 0 && order.size() > 4096) { std::fprintf(stderr, "%s: more than 4096 frames to write\n", crop_opt); rc = 1; }
        }
        // the smallest block rectangle that contains the display rectangle, clipped to the block grid; stored row = Y - 1 - display row
        const long nbx = clip.X / 4, nby = clip.Y / 4;
        const long x0 = std::max(crop_rect[0], 0l), x1 = std::min(crop_rect[0] + crop_rect[2], 4 * nbx);
        const long s0 = std::max(clip.Y - (crop_rect[1] + crop_rect[3]), 0l), s1 = std::min(clip.Y - crop_rect[1], 4 * nby);
        if (rc == 0 && (x0 >= x1 || s0 >= s1)) { std::fprintf(stderr, "%s: nothing of the rectangle lies in the picture's blocks\n", crop_opt); rc = 1; }
        const int bx = (int)(x0 / 4), by = (int)(s0 / 4), bw = (int)((x1 + 3) / 4) - bx, bh = (int)((s1 + 3) / 4) - by;
        if (rc == 0) std::printf("%s blocks %d %d %d %d display %d %ld %d %d\n", crop_opt + 2, bx, by, bw, bh, 4 * bx, clip.Y - 4l * (by + bh), 4 * bw, 4 * bh);
        const auto frames_call = path_mode ? jsp_index_path_frames : jsp_index_crop_frames;
        const char* frames_name = path_mode ? "jsp_index_path_frames" : "jsp_index_crop_frames";
        std::vector<uint8_t> made;
        std::vector<size_t> made_lens;
        std::vector<int> made_keys;
        if (rc == 0) {
            size_t k = keep[0];
            while (k > 0 && !frame_is_key(clip, dec, k)) --k;   // the nearest key frame <= FIRST (frame 0 is one)
            std::vector<const uint8_t*> srcs;
            std::vector<size_t> lens;
            std::vector<uint8_t> keys;
            for (size_t i = k; i <= keep.back(); ++i) {
                srcs.push_back(clip.bytes.data() + clip.frames[i].first);
                lens.push_back(clip.frames[i].second);
                keys.push_back(i == k || frame_is_key(clip, dec, i) ? 1 : 0);
            }
            jsp_index* idx = jsp_index_build(dec, (int)srcs.size(), srcs.data(), lens.data(), keys.data(), kInsignificantLines);
            if (!idx) { std::fprintf(stderr, "jsp_index_build: %s\n", jsp_last_error()); rc = 1; }
            for (size_t g0 = 0; rc == 0 && g0 < order.size(); g0 += 4096) {   // (a call takes 4096 pairs)
                const size_t m = std::min<size_t>(4096, order.size() - g0);
                std::vector<int> from(m), to(m), ks(m);
                for (size_t i = 0; i < m; ++i) {
                    from[i] = g0 + i == 0 ? JSP_CROP_KEY : (int)(order[g0 + i - 1] - k);
                    to[i] = (int)(order[g0 + i] - k);
                }
                std::vector<size_t> ls(m);
                size_t total = 0;
                const int flags = crop_tight ? JSP_CROP_TIGHT : 0;
                // asked twice: the lengths (cap 0 is a refusal that still sets them), then the bytes
                if (frames_call(dec, idx, bx, by, bw, bh, (int)m, from.data(), to.data(), flags, nullptr, 0, ls.data(), ks.data(), &total) == JSP_ZERO_STATE || total == 0) {
                    std::fprintf(stderr, "%s: %s\n", frames_name, jsp_last_error());
                    rc = 1;
                    break;
                }
                const size_t at = made.size();
                made.resize(at + total);
                if (frames_call(dec, idx, bx, by, bw, bh, (int)m, from.data(), to.data(), flags, made.data() + at, total, ls.data(), ks.data(), &total) != JSP_ZERO_STATE) {
                    std::fprintf(stderr, "%s: %s\n", frames_name, jsp_last_error());
                    rc = 1;
                }
                made_lens.insert(made_lens.end(), ls.begin(), ls.end());
                made_keys.insert(made_keys.end(), ks.begin(), ks.end());
            }
            if (idx) jsp_index_destroy(idx);
        }
        jsp_pool_destroy(pool);
        jsp_codec_destroy(dec);
        if (rc != 0) return rc;
        std::vector<std::pair<const uint8_t*, size_t>> out_frames;
        std::vector<uint8_t> out_keys;
        size_t at = 0;
        for (size_t j = 0; j < order.size(); ++j) {
            out_frames.emplace_back(made.data() + at, made_lens[j]);
            out_keys.push_back(j == 0 || made_keys[j] ? 1 : 0);
            at += made_lens[j];
        }
        Clip header;                                            // the clip's stream at the rectangle's size
        header.X = 4 * bw, header.Y = 4 * bh, header.bpp = clip.bpp, header.kind = clip.kind, header.usec = clip.usec, header.palette = clip.palette;
        const std::vector<uint8_t> file = avi_file(header, out_frames, out_keys);
        FILE* f = std::fopen(thin_path.c_str(), "wb");
        if (!f || std::fwrite(file.data(), 1, file.size(), f) != file.size()) { std::fprintf(stderr, "cannot write %s\n", thin_path.c_str()); if (f) std::fclose(f); return 1; }
        std::fclose(f);
        // OUT.avi played back through the ordinary decode loop of a decoder of ITS size, beside that part of the clip's own pictures
        Clip cropped;
        if (!load(thin_path.c_str(), cropped) || cropped.frames.size() != order.size() || cropped.X != 4 * bw || cropped.Y != 4 * bh) { std::fprintf(stderr, "cannot read %s back\n", thin_path.c_str()); return 1; }
        std::vector<uint32_t> got, want;
        if (!covered_crcs(cropped, cropped.frames.size(), got) || !covered_crcs(clip, keep.back() + 1, want, 4 * (size_t)bx, 4 * (size_t)by, 4 * (size_t)bw, 4 * (size_t)bh)) return 1;
        for (size_t j = 0; j < order.size(); ++j) {
            std::printf("%zu %08x %08x\n", order[j], got[j], want[order[j]]);
            if (got[j] != want[order[j]]) rc = 1;
        }
        return rc;
    }
    if (thin_first >= 0) {   // a time-lapse: one index build from the key frame before, ONE jsp_index_delta_frames (--thin-tight: jsp_index_tight_frames) for every gap, the file, its playback
        const size_t n = clip.frames.size();
        std::vector<size_t> keep;
        for (long i = thin_first; i < (long)n && (thin_count < 0 || (long)keep.size() < thin_count); i += thin_stride) keep.push_back((size_t)i);
        if (keep.empty() || (thin_count >= 0 && (long)keep.size() < thin_count)) {
            std::fprintf(stderr, "--thin: frames %ld, %ld, ... (%ld of them) are not all in the clip (%zu frames)\n", thin_first, thin_first + thin_stride, thin_count, n);
            rc = 1;
        }
        const auto gap_frames = thin_tight ? jsp_index_tight_frames : jsp_index_delta_frames;
        const char* gap_name = thin_tight ? "jsp_index_tight_frames" : "jsp_index_delta_frames";
        std::vector<uint8_t> key_frame, deltas;
        std::vector<size_t> gaps, delta_lens;                   // entries of `keep` that are inter frames over a gap, and their lengths
        for (size_t j = 1; rc == 0 && j < keep.size(); ++j)
            if (keep[j] != keep[j - 1] + 1 && !frame_is_key(clip, dec, keep[j])) gaps.push_back(j);
        const bool need_key = rc == 0 && !frame_is_key(clip, dec, keep[0]);
        if (rc == 0 && (need_key || !gaps.empty())) {
            size_t k = keep[0];
            while (k > 0 && !frame_is_key(clip, dec, k)) --k;   // the nearest key frame <= FIRST (frame 0 is one)
            std::vector<const uint8_t*> srcs;
            std::vector<size_t> lens;
            std::vector<uint8_t> keys;
            for (size_t i = k; i <= keep.back(); ++i) {
                srcs.push_back(clip.bytes.data() + clip.frames[i].first);
                lens.push_back(clip.frames[i].second);
                keys.push_back(i == k || frame_is_key(clip, dec, i) ? 1 : 0);
            }
            jsp_index* idx = jsp_index_build(dec, (int)srcs.size(), srcs.data(), lens.data(), keys.data(), kInsignificantLines);
            if (!idx) { std::fprintf(stderr, "jsp_index_build: %s\n", jsp_last_error()); rc = 1; }
            if (rc == 0 && need_key) {
                size_t bound = 0, len = 0;
                if (jsp_index_key_frame_bound(idx, &bound) != JSP_ZERO_STATE) { std::fprintf(stderr, "jsp_index_key_frame_bound: %s\n", jsp_last_error()); rc = 1; }
                key_frame.resize(bound);
                if (rc == 0 && jsp_index_key_frame(dec, idx, (int)(keep[0] - k), key_frame.data(), bound, &len) != JSP_ZERO_STATE) {
                    std::fprintf(stderr, "jsp_index_key_frame: %s\n", jsp_last_error());
                    rc = 1;
                }
                key_frame.resize(len);
            }
            for (size_t g0 = 0; rc == 0 && g0 < gaps.size(); g0 += 4096) {   // (a call takes 4096 pairs)
                const size_t m = std::min<size_t>(4096, gaps.size() - g0);
                std::vector<int> from(m), to(m);
                for (size_t i = 0; i < m; ++i) {
                    from[i] = (int)(keep[gaps[g0 + i] - 1] - k);
                    to[i] = (int)(keep[gaps[g0 + i]] - k);
                }
                std::vector<size_t> ls(m);
                size_t total = 0;
                // asked twice: the lengths (cap 0 is a refusal that still sets them), then the bytes
                if (gap_frames(dec, idx, (int)m, from.data(), to.data(), nullptr, 0, ls.data(), &total) == JSP_ZERO_STATE || total == 0) {
                    std::fprintf(stderr, "%s: %s\n", gap_name, jsp_last_error());
                    rc = 1;
                    break;
                }
                const size_t at = deltas.size();
                deltas.resize(at + total);
                if (gap_frames(dec, idx, (int)m, from.data(), to.data(), deltas.data() + at, total, ls.data(), &total) != JSP_ZERO_STATE) {
                    std::fprintf(stderr, "%s: %s\n", gap_name, jsp_last_error());
                    rc = 1;
                }
                delta_lens.insert(delta_lens.end(), ls.begin(), ls.end());
            }
            jsp_index_destroy(idx);
        }
        std::vector<std::pair<const uint8_t*, size_t>> out_frames;
        std::vector<uint8_t> out_keys;
        size_t g = 0, at = 0;
        for (size_t j = 0; rc == 0 && j < keep.size(); ++j) {
            const bool was_key = frame_is_key(clip, dec, keep[j]);
            if (j == 0 && need_key) out_frames.emplace_back(key_frame.data(), key_frame.size());
            else if (g < gaps.size() && gaps[g] == j) {
                out_frames.emplace_back(deltas.data() + at, delta_lens[g]);
                at += delta_lens[g++];
            } else out_frames.emplace_back(clip.bytes.data() + clip.frames[keep[j]].first, clip.frames[keep[j]].second);
            out_keys.push_back(j == 0 || was_key || jsp_is_key_frame(dec, out_frames.back().first, out_frames.back().second) ? 1 : 0);
        }
        jsp_pool_destroy(pool);
        jsp_codec_destroy(dec);
        if (rc != 0) return rc;
        const std::vector<uint8_t> file = avi_file(clip, out_frames, out_keys);
        FILE* f = std::fopen(thin_path.c_str(), "wb");
        if (!f || std::fwrite(file.data(), 1, file.size(), f) != file.size()) { std::fprintf(stderr, "cannot write %s\n", thin_path.c_str()); if (f) std::fclose(f); return 1; }
        std::fclose(f);
        // OUT.avi played back through the ordinary decode loop, beside the clip's own frames FIRST + k * STRIDE
        Clip thinned;
        if (!load(thin_path.c_str(), thinned) || thinned.frames.size() != keep.size()) { std::fprintf(stderr, "cannot read %s back\n", thin_path.c_str()); return 1; }
        std::vector<uint32_t> got, want;
        if (!covered_crcs(thinned, thinned.frames.size(), got) || !covered_crcs(clip, keep.back() + 1, want)) return 1;
        for (size_t j = 0; j < keep.size(); ++j) {
            std::printf("%zu %08x %08x\n", keep[j], got[j], want[keep[j]]);
            if (got[j] != want[keep[j]]) rc = 1;
        }
        return rc;
    }
    if (strip > 0) {   // the seek bar's preview pictures: one index build, then ONE jsp_index_thumbs / jsp_sp_index_thumbs for all of them
        const size_t n = clip.frames.size();
        std::vector<const uint8_t*> srcs;
        std::vector<size_t> lens;
        std::vector<uint8_t> keys;
        for (size_t i = 0; i < n; ++i) {
            srcs.push_back(clip.bytes.data() + clip.frames[i].first);
            lens.push_back(clip.frames[i].second);
            keys.push_back(i == 0 || frame_is_key(clip, dec, i) ? 1 : 0);
        }
        const bool sp = clip.kind == JSP_CODEC_SCREENPRESSOR;   // the same two calls on the index of either codec
        jsp_index* idx = n && !sp ? jsp_index_build(dec, (int)n, srcs.data(), lens.data(), keys.data(), kInsignificantLines) : nullptr;
        jsp_sp_index* sidx = n && sp ? jsp_sp_index_build(dec, (int)n, srcs.data(), lens.data(), keys.data(), kInsignificantLines) : nullptr;
        const char* const build_call = sp ? "jsp_sp_index_build" : "jsp_index_build";
        const char* const size_call = sp ? "jsp_sp_index_thumb_size" : "jsp_index_thumb_size";
        const char* const thumbs_call = sp ? "jsp_sp_index_thumbs" : "jsp_index_thumbs";
        if (!idx && !sidx) { std::fprintf(stderr, "%s: %s\n", build_call, n ? jsp_last_error() : "no frames"); rc = 1; }
        int tw = 0, th = 0;
        if (rc == 0 && (sp ? jsp_sp_index_thumb_size(sidx, strip_scale, &tw, &th) : jsp_index_thumb_size(idx, strip_scale, &tw, &th)) != JSP_ZERO_STATE) {
            std::fprintf(stderr, "%s: %s\n", size_call, jsp_last_error());
            rc = 1;
        }
        jsp_pool* sheet = nullptr;   // cols = 1: a plain [N][th][tw] array, one "frame" of tw x N th pixels
        if (rc == 0 && !(sheet = jsp_pool_create(0, tw, strip * th, 1))) { std::fprintf(stderr, "jsp_pool_create: %s\n", jsp_last_error()); rc = 1; }
        if (rc == 0) {
            std::vector<int> picks;
            for (int k = 0; k < strip; ++k) picks.push_back((int)(((long long)k * (long long)n) / strip));
            const size_t cell = (size_t)tw * th;
            std::vector<int32_t> thumbs(cell * (size_t)strip);
            int32_t* out = jsp_pool_buffer(sheet, 0);
            if ((sp ? jsp_sp_index_thumbs(dec, sidx, strip, picks.data(), strip_scale, 1, out, thumbs.size())
                    : jsp_index_thumbs(dec, idx, strip, picks.data(), strip_scale, 1, out, thumbs.size())) != JSP_ZERO_STATE ||
                jsp_download(out, thumbs.data(), thumbs.size()) != 0) {
                std::fprintf(stderr, "%s: %s\n", thumbs_call, jsp_last_error());
                rc = 1;
            }
            for (int k = 0; rc == 0 && k < strip; ++k)
                std::printf("%d %08x\n", picks[k], crc32(reinterpret_cast<const uint8_t*>(thumbs.data() + cell * (size_t)k), cell * 4));
        }
        if (sheet) jsp_pool_destroy(sheet);
        jsp_sp_index_destroy(sidx);
        jsp_index_destroy(idx);
        jsp_pool_destroy(pool);
        jsp_codec_destroy(dec);
        return rc;
    }
    if (ip_n > 0) {   // windows straight out of a seek index: one index build, then ONE jsp_index_present / jsp_sp_index_present for all of them
        const size_t n = clip.frames.size();
        std::vector<const uint8_t*> srcs;
        std::vector<size_t> lens;
        std::vector<uint8_t> keys;
        for (size_t i = 0; i < n; ++i) {
            srcs.push_back(clip.bytes.data() + clip.frames[i].first);
            lens.push_back(clip.frames[i].second);
            keys.push_back(i == 0 || frame_is_key(clip, dec, i) ? 1 : 0);
        }
        const bool sp = clip.kind == JSP_CODEC_SCREENPRESSOR;   // the same call on the index of either codec
        double k = 1, dx = 0, dy = 0;
        if (jsp_view_matrix(clip.X, clip.Y, present_w, present_h, present_zoom, present_hpos, present_vpos, &k, &dx, &dy) != 0) {
            std::fprintf(stderr, "jsp_view_matrix: %s\n", jsp_last_error());
            rc = 2;
        }
        jsp_index* idx = rc == 0 && n && !sp ? jsp_index_build(dec, (int)n, srcs.data(), lens.data(), keys.data(), kInsignificantLines) : nullptr;
        jsp_sp_index* sidx = rc == 0 && n && sp ? jsp_sp_index_build(dec, (int)n, srcs.data(), lens.data(), keys.data(), kInsignificantLines) : nullptr;
        if (rc == 0 && !idx && !sidx) { std::fprintf(stderr, "%s: %s\n", sp ? "jsp_sp_index_build" : "jsp_index_build", n ? jsp_last_error() : "no frames"); rc = 1; }
        const bool tensor = it_dtype >= 0;   // --index-tensor: 3 elements a pixel, of at most 4 bytes each — three "frames" of W x N H ints hold them
        jsp_pool* sheet = nullptr;   // cols = 1: a plain [N][H][W] array, one "frame" of W x N H pixels
        if (rc == 0 && !(sheet = jsp_pool_create(0, present_w, ip_n * present_h * (tensor ? 3 : 1), 1))) { std::fprintf(stderr, "jsp_pool_create: %s\n", jsp_last_error()); rc = 1; }
        std::vector<int> picks;
        for (int i = 0; i < ip_n; ++i) picks.push_back((int)(((long long)i * (long long)n) / ip_n));
        const int mode = clip.bpp == 16 && sp ? JSP_DISPLAY_CANVAS_RGB15 : JSP_DISPLAY_CANVAS;
        if (rc == 0 && tensor) {
            const size_t esize = it_dtype == JSP_TENSOR_F32 ? 4 : it_dtype == JSP_TENSOR_U8 ? 1 : 2;
            const size_t slice = (size_t)3 * present_w * present_h * esize, bytes = slice * (size_t)ip_n;
            std::vector<int32_t> host((bytes + 3) / 4);
            int32_t* out = jsp_pool_buffer(sheet, 0);
            const float scale[3] = {1.0f / 255.0f, 1.0f / 255.0f, 1.0f / 255.0f}, bias[3] = {0.0f, 0.0f, 0.0f};
            if ((sp ? jsp_sp_index_tensor(dec, sidx, ip_n, picks.data(), out, bytes, present_w, present_h, k, dx, dy, mode, ip_filter, 0xFF000000u, it_dtype, it_layout, scale, bias)
                    : jsp_index_tensor(dec, idx, ip_n, picks.data(), out, bytes, present_w, present_h, k, dx, dy, mode, ip_filter, 0xFF000000u, it_dtype, it_layout, scale, bias)) != JSP_ZERO_STATE ||
                jsp_download(out, host.data(), host.size()) != 0) {
                std::fprintf(stderr, "%s: %s\n", sp ? "jsp_sp_index_tensor" : "jsp_index_tensor", jsp_last_error());
                rc = 1;
            }
            for (int i = 0; rc == 0 && i < ip_n; ++i)
                std::printf("%d %08x\n", picks[i], crc32(reinterpret_cast<const uint8_t*>(host.data()) + slice * (size_t)i, slice));
        } else if (rc == 0) {
            const size_t cell = (size_t)present_w * present_h;
            std::vector<int32_t> cells(cell * (size_t)ip_n);
            int32_t* out = jsp_pool_buffer(sheet, 0);
            if ((sp ? jsp_sp_index_present(dec, sidx, ip_n, picks.data(), out, cells.size(), present_w, present_h, (size_t)present_w, 1, k, dx, dy, mode, ip_filter, 0xFF000000u)
                    : jsp_index_present(dec, idx, ip_n, picks.data(), out, cells.size(), present_w, present_h, (size_t)present_w, 1, k, dx, dy, mode, ip_filter, 0xFF000000u)) != JSP_ZERO_STATE ||
                jsp_download(out, cells.data(), cells.size()) != 0) {
                std::fprintf(stderr, "%s: %s\n", sp ? "jsp_sp_index_present" : "jsp_index_present", jsp_last_error());
                rc = 1;
            }
            for (int i = 0; rc == 0 && i < ip_n; ++i)
                std::printf("%d %08x\n", picks[i], crc32(reinterpret_cast<const uint8_t*>(cells.data() + cell * (size_t)i), cell * 4));
        }
        if (sheet) jsp_pool_destroy(sheet);
        jsp_sp_index_destroy(sidx);
        jsp_index_destroy(idx);
        jsp_pool_destroy(pool);
        jsp_codec_destroy(dec);
        return rc;
    }
    if (seek_to >= 0) {   // the seek branch of GetDecompressedFrame: frames [nearest key frame, N] in one call, into slot 0
        if ((size_t)seek_to >= clip.frames.size()) { std::fprintf(stderr, "--seek %ld: the clip has %zu frames\n", seek_to, clip.frames.size()); return 2; }
        size_t k = (size_t)seek_to;
        while (k > 0 && !frame_is_key(clip, dec, k)) --k;
        std::vector<const uint8_t*> srcs;
        std::vector<size_t> lens;
        std::vector<uint8_t> keys;
        for (size_t i = k; i <= (size_t)seek_to; ++i) {
            srcs.push_back(clip.bytes.data() + clip.frames[i].first);
            lens.push_back(clip.frames[i].second);
            keys.push_back(frame_is_key(clip, dec, i) ? 1 : 0);
        }
        int32_t* dst = jsp_pool_buffer(pool, 0);
        int32_t* shown_ptr = nullptr;
        int signif = -1;
        if (jsp_seek(dec, (int)srcs.size(), srcs.data(), lens.data(), keys.data(), dst, &shown_ptr, &signif) != JSP_ZERO_STATE) {
            std::fprintf(stderr, "jsp_seek: %s\n", jsp_last_error());
            jsp_pool_destroy(pool);
            jsp_codec_destroy(dec);
            return 1;
        }
        const int shown = shown_ptr == dst ? 0 : -1;
        if (shown == 0) first[0] = last[0] = seek_to;
        uint32_t crc = 0;
        if (shown >= 0 && jsp_download(dst, host.data(), npx) == 0) crc = crc32(reinterpret_cast<const uint8_t*>(host.data()), npx * 4);
        last_was_key = keys.back() != 0;
        if (last_was_key) { prev_key = srcs.back(); prev_key_len = lens.back(); }
        std::printf("%ld %s %d %d %08x\n", seek_to, last_was_key ? "key" : "inter", shown, last_was_key ? -1 : signif, crc);
        begin = (size_t)seek_to + 1;
    }
    // --present: the window Main.on_stage_resize would draw (Main.hx:301-318), one launch per frame shown; the display mode as
    // Manager.hx:121 chooses convert_fromRGB15
    jsp_pool* window = nullptr;
    std::vector<int32_t> window_host;
    double view_k = 1, view_dx = 0, view_dy = 0;
    const int present_mode = clip.bpp == 16 && clip.kind == JSP_CODEC_SCREENPRESSOR ? JSP_DISPLAY_CANVAS_RGB15 : JSP_DISPLAY_CANVAS;
    if (present_w > 0) {
        if (jsp_view_matrix(clip.X, clip.Y, present_w, present_h, present_zoom, present_hpos, present_vpos, &view_k, &view_dx, &view_dy) != 0) {
            std::fprintf(stderr, "--present: %s\n", jsp_last_error());
            jsp_pool_destroy(pool);
            jsp_codec_destroy(dec);
            return 2;
        }
        window = jsp_pool_create(0, present_w, present_h, 1);
        if (!window) { std::fprintf(stderr, "jsp_pool_create: %s\n", jsp_last_error()); jsp_pool_destroy(pool); jsp_codec_destroy(dec); return 1; }
        window_host.resize((size_t)present_w * present_h);
    }
    for (size_t i = begin; i < clip.frames.size(); ++i) {
        const uint8_t* src = clip.bytes.data() + clip.frames[i].first;
        const size_t len = clip.frames[i].second;
        const bool key = frame_is_key(clip, dec, i);
        int32_t* prev = jsp_previous_frame(dec);
        int prev_slot = -1, slot = -1;
        for (int k = 0; k < nbuf; ++k) if (prev && jsp_pool_buffer(pool, k) == prev) prev_slot = k;
        {   // a free slot, else the one showing the oldest frames already behind the frame of interest
            long oldest = 1L << 60;
            int victim = -1;
            for (int k = 0; k < nbuf && slot < 0; ++k) {
                if (k == prev_slot) continue;
                if (first[k] < 0) slot = k;
                else if (last[k] < (long)i && first[k] < oldest) { oldest = first[k]; victim = k; }
            }
            if (slot < 0) { slot = victim; if (slot >= 0) first[slot] = last[slot] = -1; }
        }
        if (slot < 0) { std::fprintf(stderr, "no free frame buffer\n"); rc = 1; break; }
        int32_t* dst = jsp_pool_buffer(pool, slot);
        int shown = slot, signif = -1;
        if (key) {
            const int state = jsp_decompress_i(dec, src, len, dst);
            if (state != JSP_ZERO_STATE) { std::printf("%zu key error %d %s\n", i, state, jsp_last_error()); last_was_key = true; continue; }
            first[slot] = last[slot] = (long)i;
            if (i == 0) signif = 1;
            else if (last_was_key && prev_key) signif = !(prev_key_len == len && !std::memcmp(prev_key, src, len));
            else if (!prev) signif = 1;
            else { signif = jsp_key_frame_differs(dec); if (signif < 0) signif = 1; }
            prev_key = src;
            prev_key_len = len;
        } else {
            int32_t* shown_ptr = nullptr;
            if (jsp_decompress_p(dec, src, len, dst, &shown_ptr, &signif) != 0) {
                std::printf("%zu inter raised %s\n", i, jsp_last_error());
                last_was_key = false;
                continue;
            }
            if (shown_ptr && shown_ptr == prev && prev_slot >= 0) {          // "no changes": the old slot keeps showing
                last[prev_slot] = (long)i;
                shown = prev_slot;
            } else if (shown_ptr) {
                first[slot] = last[slot] = (long)i;
            } else
                shown = -1;
        }
        last_was_key = key;
        uint32_t crc = 0;
        if (shown >= 0 && jsp_download(jsp_pool_buffer(pool, shown), host.data(), npx) == 0)
            crc = crc32(reinterpret_cast<const uint8_t*>(host.data()), npx * 4);
        if (window) {
            uint32_t wcrc = 0;
            if (shown >= 0) {
                int32_t* win = jsp_pool_buffer(window, 0);
                const int prc = present_area
                    ? jsp_display_present_area(jsp_pool_buffer(pool, shown), clip.X, clip.Y, win, present_w, present_h, (size_t)present_w, view_k, view_dx, view_dy,
                                               present_mode, 0xFF000000u, nullptr)
                    : jsp_display_present(jsp_pool_buffer(pool, shown), clip.X, clip.Y, win, present_w, present_h, (size_t)present_w, view_k, view_dx, view_dy,
                                          present_mode, JSP_PRESENT_BILINEAR, 0xFF000000u, nullptr);
                if (prc != 0) {
                    std::fprintf(stderr, "%s: %s\n", present_area ? "jsp_display_present_area" : "jsp_display_present", jsp_last_error());
                    rc = 1;
                    break;
                }
                if (jsp_download(win, window_host.data(), window_host.size()) == 0)
                    wcrc = crc32(reinterpret_cast<const uint8_t*>(window_host.data()), window_host.size() * 4);
            }
            std::printf("%zu %s %d %d %08x %08x\n", i, key ? "key" : "inter", shown, signif, crc, wcrc);
        } else
            std::printf("%zu %s %d %d %08x\n", i, key ? "key" : "inter", shown, signif, crc);
    }
    if (window) jsp_pool_destroy(window);
    jsp_pool_destroy(pool);
    jsp_codec_destroy(dec);
    return rc;
}
