// MSVideo1_16bit / MSVideo1_8bit behind the IVideoCodec-shaped C ABI.
// Host side = control flow of MSVideo1.hx:106-209 / 293-393 (early-outs, changes, block_changes,
// adoption of dst as prevFrame); pixels are produced by msv1_kernels.hip.  The descriptor table is
// built either by the sequential host parser (msv1_host.cpp) or on the GPU
// (msv1_parse_kernels.hip, option "msv1_parse" = "gpu").
#include <algorithm>
#include <atomic>
#include <memory>
#include <exception>
#include <thread>
#include <unordered_set>

#include "codec.h"
#include "msv1.h"
#include "msv1_seek.h"
#include <msv1_fused_hooks.h>   // (angle brackets: a lab build puts its own in front on the include path, see the Makefile)

namespace jsp {
namespace {

// Published tile tables carry the launch's epoch; 0 is what freshly zeroed memory reads as, so the counter skips it when it wraps.
inline uint32_t next_epoch(uint32_t& e) { if (++e == 0) ++e; return e; }

// Bytes of a staged batch's published tile words (d_agg, d_agg_emit), the lab build's counters behind them included (msv1.h).
inline size_t agg_bytes(size_t tiles) { return sizeof(unsigned long long) * (MSV1_AGG_PUBLISHED + MSV1_AGG_LAB_CLOCKS) * std::max<size_t>(tiles, 1); }

// One tile's record for msv1_fused_kernel (msv1.h): tile k of `ntiles` (the first is number `first_tile` of the launch's published words), `tile_bytes`
// each, of the frame whose bytes start at `beg` of the stream buffer; `even_end`: the end without an odd last byte, `data_end`: of what may be read.
inline Msv1TileRec tile_rec(uint32_t beg, uint32_t even_end, uint32_t data_end, uint32_t k, uint32_t tile_bytes, uint32_t first_tile, uint32_t ntiles,
                            int32_t* dst, const int32_t* prev, uint32_t* signif, uint32_t cmp_row_lo, uint32_t flags) {
    Msv1TileRec r{};
    r.byte0 = beg + k * tile_bytes;
    r.frame_end = even_end;
    r.data_end = data_end;
    r.k = k;
    r.first_tile = first_tile;
    r.ntiles = ntiles;
    r.cmp_row_lo = cmp_row_lo;
    r.flags = flags;
    r.dst = dst;
    r.prev = prev;
    r.signif = signif;
    r.pad = 0;
    return r;
}

// Launch order of the tiles of frames [f0, f1), frame i having ntiles[i] of them: emit(i, k) for every tile, in that order.
// Tile-major over the frames — tile j of every frame before tile j + 1 of any — so that when a tile starts, its predecessor in the frame is long done
// and has published where the chain stands (the kernel's one-word look-back).
// ... and the frames do not march in step: frame i starts ((i - f0) mod stagger) rounds late, so that at any time the batch's write
// fronts stand at different depths of their frames instead of all at tile j.  What the memory system makes of
// hundreds of fronts depends on where the frames lie in physical memory; staggered by 64, the same frames
// take 2 - 6 % less time whichever way they lie (one process, same buffers: profiles/archive/r03_stagger_one_process.txt).  stagger 0: in step.
constexpr uint32_t MSV1_TILE_STAGGER = 64;
template <class Emit>
inline void staggered_tile_order(int f0, int f1, const std::vector<uint32_t>& ntiles, uint32_t stagger, Emit&& emit) {
    uint32_t maxt = 0;
    for (int i = f0; i < f1; ++i) maxt = std::max(maxt, ntiles[i]);
    for (uint32_t j = 0; j < maxt + stagger; ++j)
        for (int i = f0; i < f1; ++i) {
            const uint32_t late = stagger ? (uint32_t)(i - f0) % stagger : 0u;
            if (j >= late && j - late < ntiles[i]) emit(i, j - late);
        }
}

// Significance of a frame, MSVideo1.hx:187-204 / 372-388: 1, 0, or -1 = stage 2 decides (the compare with the previous frame, on the GPU).
// `s1`: a coded block lies in a significant block row; `compares`: a 16-bit codec whose Preinit set insign_lines.  Key frames report none.
inline int msv1_significance(bool s1, bool have_prev, bool key, bool compares) {
    if (!s1 || key) return 0;
    if (!have_prev) return 1;
    return compares ? -1 : 0;   // 8-bit: NaN loop bound -> no pixel is compared -> false
}

// What the phases of Msv1Codec::stage() hand on to each other about the batch being staged.
struct StagePlan {
    std::vector<size_t> beg;               // where each frame's bytes start in the batch's stream buffer
    size_t total_stream = 0;
    std::vector<uint8_t> in_pinned;        // the frame's bytes are uploaded from where the caller keeps them
    Msv1ParseFrame* h_pf = nullptr;        // on-GPU parse: the frames' parse records ...
    const Msv1FrameInfo* h_info = nullptr; // ... and what the parse kernels counted in each
    struct Attr { bool dependent, noop, special, edge; };
    std::vector<Attr> attr;
    std::vector<uint64_t> frame_stream;    // stream bytes each frame's codes occupy
    bool pframes_dirty = false;            // some frame went to the host parser after the parse records were uploaded
    bool vec_ok = true;
    double h2d_ms = 0, gpu_parse_ms = 0;
};

struct Msv1Staged : jsp_staged {
    Msv1Geometry geo{};
    const int32_t* d_palette = nullptr;
    bool vec_ok = true;
    int nframes = 0;
    DeviceBuffer d_stream, d_desc, d_frames;
    PinnedBuffer h_stream, h_desc, h_frames;
    struct Group {
        int first, count;
        bool edge_compare;
        bool temporal;   // inter-frame group: one launch, frames walked in registers per spatial tile
        bool fused;      // parse + reconstruction in one launch straight from the stream bytes (no descriptor table)
    };
    std::vector<Group> groups;
    bool need_signif = false;  // some frame asked for the stage-2 compare

    // on-GPU parse state
    bool gpu_parse = false;
    int ntiles = 0, max_tiles = 0, insignificant_blocks = 0;
    DeviceBuffer d_pframes, d_tile_frame, d_tile_tab, d_tile_entry, d_tile_block0, d_info;
    PinnedBuffer h_pframes, h_tile_frame, h_info;
    // fused parse + reconstruction (msv1_fused_kernel): published tile tables, ticket / fault words
    DeviceBuffer d_agg, d_sync, d_recs, d_recs_emit, d_agg_emit;
    int ntiles_emit = 0;       // tiles of the table-writing form: it parses in 8 KiB tiles (twice the workgroups per CU, half the serial work in each)
    PinnedBuffer h_fault, h_recs, h_recs_emit;
    uint32_t epoch = 0;
    bool needs_desc = false;   // some launch reads the descriptor table the parse kernels build
    std::vector<uint32_t> scrub;   // (tests: option "msv1_scrub_tables") frames whose table a replay rewrites: poisoned before it does
    bool any_fused = false;
    // (Round 4 also wrote the replay's tables in PIECES of frames on a second stream, beside the launches that read the piece before — option
    // "msv1_parse_pieces": bit-exact and 12 - 50 % slower in every split, profiles/r04_msv1_parse_pieces.txt; removed in round 5, commit history has it.)

    // Replays of an inter-frame batch (round 6, option "msv1_parse_ahead", default on): the table-writing parse of the NEXT replay runs on the codec's
    // second stream beside this replay's temporal launch, into the OTHER of two table sets — the parse reads nothing but the stream bytes, so only the
    // tables' readers and writers have to be kept apart (events below).  Every replay still costs one parse launch and its reconstruction launches; what
    // changes is that the parse (0.15 - 0.19 ms of a 1.02 ms step at 512 x 1080p) no longer stands in front of the launch that needs it.
    hipStream_t side = nullptr;        // the codec's second stream; null: everything in line on the caller's stream
    hipEvent_t ev_fork = nullptr, ev_tables = nullptr;   // "the stream has reached this replay's reconstruction launches" / "the tables written ahead are complete"
    int cur_set = 0;                   // which set this replay's launches read
    bool ahead_valid = false;          // the tables of cur_set were written ahead (on `side`) and ev_tables says when
    // What a replay writes and reads: 4-byte block tables.  Set 0 is d_desc itself (what staging built: the first decode and the look-back fall-back always
    // read that); set 1 is a copy of it, with table-writing records of its own, made by the first replay that parses ahead.  Tables a replay does not
    // rewrite (frames the host parser settled) come along in the copy.
    struct TableSet {
        DeviceBuffer wide, recs;
        bool made = false;
        void drop() { wide.release(); recs.release(); made = false; }
    } sets[2];
    uint32_t* wide_tables(int i) { return (i == 0 ? d_desc : sets[i].wide).as<uint32_t>(); }
    void make_set(int i, hipStream_t stream) {
        TableSet& t = sets[i];
        if (t.made) return;
        if (i != 0) {
            std::vector<Msv1TileRec> recs((size_t)ntiles_emit);
            std::memcpy(recs.data(), h_recs_emit.p, sizeof(Msv1TileRec) * recs.size());
            const size_t table_bytes = sizeof(uint32_t) * (size_t)std::max(geo.nblocks, 1) * (size_t)nframes;
            t.wide.reserve(table_bytes);
            JSP_HIP(hipMemcpyAsync(t.wide.p, d_desc.p, table_bytes, hipMemcpyDeviceToDevice, stream));
            for (auto& r : recs) r.dst = reinterpret_cast<int32_t*>(t.wide.as<uint32_t>() + (reinterpret_cast<uint32_t*>(r.dst) - d_desc.as<uint32_t>()));
            t.recs.reserve(sizeof(Msv1TileRec) * std::max<size_t>(recs.size(), 1));
            JSP_HIP(hipMemcpy(t.recs.p, recs.data(), sizeof(Msv1TileRec) * recs.size(), hipMemcpyHostToDevice));
        }
        t.made = true;
    }
    void launch_table_parse(int set, hipStream_t on) {
        make_set(set, on);
        const TableSet& t = sets[set];
        for (uint32_t i : scrub)
            JSP_HIP(hipMemsetAsync(wide_tables(set) + (size_t)i * (size_t)std::max(geo.nblocks, 1), 0xEE, sizeof(uint32_t) * (size_t)geo.nblocks, on));
        msv1_launch_fused_tables(geo, fused_batch(t.recs.p ? t.recs : d_recs_emit, d_agg_emit, ntiles_emit, 0, ntiles_emit), on);
    }
    // A launch of one of the kernel's batch forms over tiles [tile0, tile0 + n) of `recs`, which publish in `agg` (sized for `agg_tiles` tiles).
    Msv1FusedBatch fused_batch(const DeviceBuffer& recs, const DeviceBuffer& agg, int agg_tiles, uint32_t tile0, int n) {
        Msv1FusedBatch b;
        b.stream = d_stream.as<const uint8_t>(); b.recs = recs.as<const Msv1TileRec>(); b.palette = d_palette;
        b.agg = agg.as<unsigned long long>();    b.agg_tiles = (uint32_t)agg_tiles;     b.epoch = next_epoch(epoch);
        b.tile0 = tile0;                         b.ntiles = n;                          b.fault = d_sync.as<uint32_t>();
        return b;
    }
    void drop_sets() { for (auto& t : sets) t.drop(); }
    void quiesce_side() {              // nothing of this batch is left running beside the stream (before its buffers are reused or freed)
        if (side) (void)hipStreamSynchronize(side);
        ahead_valid = false;
        cur_set = 0;
    }
    ~Msv1Staged() override {
        if (side) (void)hipStreamSynchronize(side);
        if (ev_fork) (void)hipEventDestroy(ev_fork);
        if (ev_tables) (void)hipEventDestroy(ev_tables);
    }

    void launch_parse(hipStream_t stream) {
        msv1_launch_parse(geo, d_stream.as<const uint8_t>(), d_pframes.as<const Msv1ParseFrame>(), nframes, d_tile_frame.as<const uint32_t>(), ntiles, max_tiles,
                          d_tile_tab.as<uint32_t>(), d_tile_entry.as<uint32_t>(), d_tile_block0.as<uint32_t>(), d_desc.as<uint32_t>(), d_info.as<Msv1FrameInfo>(),
                          insignificant_blocks, stream);
    }

    void decode(hipStream_t stream) override {
        if (nframes == 0) return;
        last_stream = stream;
        // A replay re-executes the whole device pipeline: with the on-GPU parse that includes the
        // parse kernels, so a staged batch can be timed from raw stream bytes.  (The first decode
        // uses the tables the staging pass left behind.)
        const bool replay = gpu_parse && decoded && needs_desc;    // one launch: the fused kernel's parse, writing block tables instead of pixels
        const bool run_ahead = side != nullptr && gpu_parse && needs_desc && ntiles_emit > 0;
        if (replay) {
            if (run_ahead && ahead_valid) JSP_HIP(hipStreamWaitEvent(stream, ev_tables, 0));   // written beside the replay before this one
            else launch_table_parse(cur_set, stream);
        }
        const uint32_t* tables = replay ? wide_tables(cur_set) : d_desc.as<const uint32_t>();
        if (run_ahead && decoded) {
            // the next replay's tables, into the other set, beside the launches below: the other set's last readers (the replay before this one) and the
            // last table-writing launch (it shares the published tile words and the fault word) are all in front of `ev_fork` on the stream
            try {
                make_set(cur_set ^ 1, stream);
            } catch (const std::exception&) {          // no room for a second table set: this batch's replays parse in line from now on
                (void)hipGetLastError();
                sets[cur_set ^ 1].drop();
                side = nullptr;
            }
        }
        if (run_ahead && decoded && side) {
            if (!ev_fork) JSP_HIP(hipEventCreateWithFlags(&ev_fork, hipEventDisableTiming));
            if (!ev_tables) JSP_HIP(hipEventCreateWithFlags(&ev_tables, hipEventDisableTiming));
            JSP_HIP(hipEventRecord(ev_fork, stream));
            JSP_HIP(hipStreamWaitEvent(side, ev_fork, 0));
            launch_table_parse(cur_set ^ 1, side);
            JSP_HIP(hipEventRecord(ev_tables, side));
        }
        launch_groups(tables, /*fused=*/true, stream);
        if (any_fused || needs_desc)
            JSP_HIP(hipMemcpyAsync(h_fault.p, d_sync.p, sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
        ++clock_launches;
        if (run_ahead && decoded && side) { cur_set ^= 1; ahead_valid = true; }   // the next replay reads what was just started beside this one
        decoded = true;
    }
    // ---- stage(), phase 5: the launch plan ----
    // "special" frames (abort, partially written) run alone with the per-frame kernel.  Between
    // them: a run of frames none of which reads its predecessor is one launch with grid.y = frame;
    // a run containing inter frames is one launch of the temporal kernel (tile per workgroup,
    // frames walked in registers) when the buffers allow 16-byte rows, else one launch per frame.
    void plan_launches(const std::vector<jsp_frame_in>& frames, const StagePlan& plan) {
        const auto& attr = plan.attr;
        const int nf = nframes;
        int i = 0;
        while (i < nf) {
            if (attr[i].special) { groups.push_back({i, 1, attr[i].edge, false, false}); ++i; continue; }
            int j = i;
            bool any_dep = false;
            while (j < nf && !attr[j].special) { any_dep |= attr[j].dependent; ++j; }
            std::unordered_set<const void*> seen;
            if (any_dep && vec_ok) {
                // every access to a tile, in whichever buffer, comes from the same workgroup in
                // program order, so buffers may even repeat inside the group
                bool edge = false;
                for (int k = i; k < j; ++k) edge |= attr[k].edge;
                groups.push_back({i, j - i, edge, true, false});
            } else {
                // frames that do not read their predecessor: one launch per run of them with grid.y = frame —
                // or, straight from the stream bytes, one fused launch per run of GPU-parsed frames
                bool closed = true;
                for (int k = i; k < j; ++k) {
                    const bool writes = !attr[k].noop;
                    const bool fusable = gpu_parse && vec_ok && !attr[k].dependent && !attr[k].noop && !plan.h_pf[k].host_parsed;
                    if (attr[k].dependent || closed || (writes && seen.count(frames[k].dst)) || groups.back().fused != fusable) {
                        groups.push_back({k, 1, attr[k].edge, false, fusable});
                        seen.clear();
                        closed = attr[k].dependent;
                    } else {
                        groups.back().count++;
                    }
                    if (writes) seen.insert(frames[k].dst);
                }
            }
            i = j;
        }
    }

    // ---- stage(), phase 6: what the plan launches and moves (info.*, kernels, needs_desc, any_fused) ----
    void account(const StagePlan& plan) {
        const int nf = nframes;
        const auto* h_frames = this->h_frames.as<const Msv1FrameArgs>();
        need_signif = false;
        for (int v : significant) need_signif |= v < 0;
        info.frames = nf;
        info.pixels = (uint64_t)geo.X * geo.Y * nf;
        info.descriptor_bytes = sizeof(uint32_t) * (uint64_t)geo.nblocks * nf + sizeof(Msv1FrameArgs) * nf;
        // A = S + 64*N_coded + 128*N_skipped
        info.algorithmic_bytes = info.stream_bytes + 64 * info.units_coded + 128 * info.units_copied;
        // Fused launches read their frames' stream bytes once and write every block
        // once.  Descriptor launches read stream + table, write the blocks, and read a previous frame per skipped /
        // compared block (per-frame kernel) or once per tile (temporal launch); when the table of any of them comes from
        // the parse kernels, every replay also runs tiles + chain + emit over the whole batch (two more reads of the
        // stream, one write of the table).
        needs_desc = false;
        any_fused = false;
        kernels.clear();
        const uint64_t table_bytes_per_frame = sizeof(uint32_t) * (uint64_t)geo.nblocks;
        uint64_t moved = 0;
        for (const auto& g : groups) {
            uint64_t written = 0, prev_reads = 0, sbytes = 0;
            bool uses_prev = false, gpu_table = false;
            for (int k = g.first; k < g.first + g.count; ++k) {
                if (!plan.attr[k].noop) written += (uint64_t)geo.nblocks;
                uses_prev |= (h_frames[k].pad & MSV1_FRAME_USES_PREV) != 0;
                if (h_frames[k].pad & MSV1_FRAME_USES_PREV) prev_reads += (uint64_t)geo.nblocks;
                sbytes += plan.frame_stream[k];
                gpu_table |= gpu_parse && !plan.h_pf[k].host_parsed;
            }
            moved += sbytes + 64 * written;
            if (g.fused) {
                any_fused = true;
                note_kernel("msv1_fused_kernel");
            } else {
                needs_desc |= gpu_table;
                moved += table_bytes_per_frame * g.count +
                         64 * (g.temporal ? (uses_prev ? (uint64_t)geo.nblocks : 0) : prev_reads);
                note_kernel(g.temporal ? "msv1_blocks_temporal_kernel" : "msv1_blocks_kernel");
            }
            if (g.edge_compare) note_kernel("msv1_edge_compare_kernel");
        }
        if (needs_desc) {   // (a replay: msv1_fused_kernel in its descriptor form reads the stream once and writes the tables)
            moved += info.stream_bytes + table_bytes_per_frame * nf;
            if (!any_fused) kernels = "msv1_fused_kernel" + (kernels.empty() ? std::string() : " + " + kernels);
        }
        info.moved_bytes = moved;
        info.kernel_launches = groups.size() + (needs_desc ? 1 : 0);
    }

    // ---- stage(), phase 7: what msv1_fused_kernel needs to know about every tile, for the launches that write pixels and the one that writes tables ----
    void build_tile_records(const std::vector<jsp_frame_in>& frames, const StagePlan& plan, bool scrub_tables, hipStream_t stream) {
        if (!any_fused && !needs_desc) return;
        d_agg.reserve(agg_bytes((size_t)ntiles));
        d_sync.reserve(MSV1_SYNC_BYTES);
        h_fault.reserve(sizeof(uint32_t));
        *h_fault.as<uint32_t>() = 0;
        epoch = 0;
        build_pixel_records(plan, stream);
        if (needs_desc) build_table_records(frames, plan, scrub_tables, stream);
        // published tile tables carry the launch epoch (first launch: 1), so stale words must read as epoch 0
        JSP_HIP(hipMemsetAsync(d_agg.p, 0, agg_bytes((size_t)ntiles), stream));
        JSP_HIP(hipMemsetAsync(d_sync.p, 0, MSV1_SYNC_BYTES, stream));   // the fault word
    }
    // one record per 16 KiB tile, in stream order; then in launch order inside every fused launch
    void build_pixel_records(const StagePlan& plan, hipStream_t stream) {
        const int nf = nframes;
        const Msv1ParseFrame* h_pf = plan.h_pf;
        const auto* h_frames = this->h_frames.as<const Msv1FrameArgs>();
        h_recs.reserve(sizeof(Msv1TileRec) * (size_t)std::max(ntiles, 1));
        d_recs.reserve(sizeof(Msv1TileRec) * (size_t)std::max(ntiles, 1));
        auto* recs = h_recs.as<Msv1TileRec>();
        std::vector<uint32_t> nt16((size_t)nf);
        for (int i = 0; i < nf; ++i) {
            nt16[i] = h_pf[i].ntiles;
            for (uint32_t k = 0; k < h_pf[i].ntiles; ++k)   // (byte0 == (first_tile + k) * tile: frames start on tile boundaries)
                recs[h_pf[i].first_tile + k] = tile_rec(h_pf[i].beg, h_pf[i].end, geo.bits == 16 ? h_pf[i].end : h_frames[i].stream_end, k, msv1_parse_tile_bytes(),
                                                        h_pf[i].first_tile, h_pf[i].ntiles, h_frames[i].dst, h_frames[i].prev, h_frames[i].signif,
                                                        h_frames[i].cmp_row_lo, h_pf[i].host_parsed ? MSV1_TILE_SKIP : 0u);
        }
        // Launch order (staggered_tile_order): a launch covers the contiguous record range of its frames; the records are
        // permuted inside that range (a record carries its own byte offset and its number in stream order).
        auto tile_major = [&](int f0, int f1) {   // frames [f0, f1)
            if (f1 - f0 < 2) return;
            const uint32_t t0 = h_pf[f0].first_tile, t1 = h_pf[f1 - 1].first_tile + h_pf[f1 - 1].ntiles;
            const std::vector<Msv1TileRec> tmp(recs + t0, recs + t1);
            uint32_t o = t0;
            staggered_tile_order(f0, f1, nt16, MSV1_TILE_STAGGER, [&](int i, uint32_t k) { recs[o++] = tmp[h_pf[i].first_tile - t0 + k]; });
        };
        for (const auto& g : groups)
            if (g.fused) tile_major(g.first, g.first + g.count);
        JSP_HIP(hipMemcpyAsync(d_recs.p, recs, sizeof(Msv1TileRec) * (size_t)ntiles, hipMemcpyHostToDevice, stream));
    }
    // The same for the descriptor form: `dst` = the frame's block table; frames whose table nobody reads (fused groups) or that came from the
    // host parser are skipped.
    // The table-writing form has no pixel stores to hide its parse behind: it runs in 8 KiB tiles (msv1_fused_kernel<BITS, 4, 16>: 64 VGPRs and
    // 19 KB of LDS, eight workgroups per CU instead of four, half the serial work per tile).  Frames start on 16 KiB boundaries of the
    // stream buffer, so a frame's 8 KiB tiles are numbered from twice its first 16 KiB tile... minus the halves that are all padding: the
    // tiles are counted per frame, records and published words (d_agg_emit) are this form's own.
    void build_table_records(const std::vector<jsp_frame_in>& frames, const StagePlan& plan, bool scrub_tables, hipStream_t stream) {
        const int nf = nframes;
        const Msv1ParseFrame* h_pf = plan.h_pf;
        const auto* h_frames = this->h_frames.as<const Msv1FrameArgs>();
        const size_t nblk = (size_t)std::max(geo.nblocks, 1);
        const uint32_t tile8 = msv1_small_tile_bytes();
        std::vector<uint32_t> first8((size_t)nf), n8((size_t)nf);
        uint32_t nt8 = 0;
        for (int i = 0; i < nf; ++i) {
            first8[i] = nt8;
            n8[i] = h_pf[i].ntiles ? (uint32_t)((frames[i].n + tile8 - 1) / tile8) : 0u;
            nt8 += n8[i];
        }
        ntiles_emit = (int)nt8;
        h_recs_emit.reserve(sizeof(Msv1TileRec) * (size_t)std::max<uint32_t>(nt8, 1));
        d_recs_emit.reserve(sizeof(Msv1TileRec) * (size_t)std::max<uint32_t>(nt8, 1));
        d_agg_emit.reserve(agg_bytes(nt8));
        auto* er = h_recs_emit.as<Msv1TileRec>();
        std::vector<uint8_t> in_fused(nf, 0);
        for (const auto& g : groups)
            if (g.fused) std::fill(in_fused.begin() + g.first, in_fused.begin() + g.first + g.count, 1);
        // written straight in launch order: over the whole batch
        uint32_t o = 0;
        staggered_tile_order(0, nf, n8, MSV1_TILE_STAGGER, [&](int i, uint32_t k) {
            er[o++] = tile_rec(h_pf[i].beg, h_pf[i].end, geo.bits == 16 ? h_pf[i].end : h_frames[i].stream_end, k, tile8, first8[i], n8[i],
                               reinterpret_cast<int32_t*>(d_desc.as<uint32_t>() + (size_t)i * nblk), nullptr, h_frames[i].signif, 0xFFFFFFFFu,
                               (h_pf[i].host_parsed || in_fused[i]) ? MSV1_TILE_SKIP : 0u);
        });
        JSP_HIP(hipMemcpyAsync(d_recs_emit.p, er, sizeof(Msv1TileRec) * (size_t)nt8, hipMemcpyHostToDevice, stream));
        JSP_HIP(hipMemsetAsync(d_agg_emit.p, 0, agg_bytes(nt8), stream));
        scrub.clear();
        if (scrub_tables)
            for (int i = 0; i < nf; ++i)
                if (!h_pf[i].host_parsed && !in_fused[i]) scrub.push_back((uint32_t)i);
    }

    // The batch's reconstruction launches in plan order, reading the block tables at `tables`, and the significance words' way back.  `fused`: groups
    // planned as fused launches go straight from the stream bytes; else (the look-back fall-back) they paint from the tables like the others.
    void launch_groups(const uint32_t* tables, bool fused, hipStream_t stream) {
        if (need_signif) JSP_HIP(hipMemsetAsync(d_signif.p, 0, sizeof(uint32_t) * nframes, stream));
        const auto* frames = d_frames.as<const Msv1FrameArgs>();
        for (const Group& g : groups) {
            if (g.fused && fused) {
                const auto* pf = h_pframes.as<const Msv1ParseFrame>();
                const uint32_t tile0 = pf[g.first].first_tile;
                const Msv1ParseFrame& last = pf[g.first + g.count - 1];
                msv1_launch_fused_pixels(geo, fused_batch(d_recs, d_agg, ntiles, tile0, (int)(last.first_tile + last.ntiles - tile0)), stream);
            } else if (g.temporal) {
                msv1_launch_blocks_temporal(geo, d_stream.as<const uint8_t>(), tables, frames + g.first, g.count, d_palette, stream);
            } else {
                msv1_launch_blocks(geo, d_stream.as<const uint8_t>(), tables, frames + g.first, g.count, d_palette, vec_ok, stream);
            }
            if (g.edge_compare) msv1_launch_edge_compare(geo, frames + g.first, g.count, stream);
        }
        JSP_HIP(hipGetLastError());
        if (need_signif) JSP_HIP(hipMemcpyAsync(h_signif.p, d_signif.p, sizeof(uint32_t) * nframes, hipMemcpyDeviceToHost, stream));
    }
    int clock_launches = 0;                                    // (read by the lab build's phase clocks only: msv1_fused_hooks.h)
    void after_sync() override {
        if (kFusedClocks && clock_launches) {   // lab build only: per-phase cycle sums since the last sync (see JSP_CLOCK), printed and cleared
            std::vector<unsigned long long> c((size_t)ntiles * MSV1_AGG_LAB_CLOCKS);
            unsigned long long* dev = d_agg.as<unsigned long long>() + (size_t)ntiles * MSV1_AGG_PUBLISHED;   // (behind `agg_tiles` tiles' published words)
            JSP_HIP(hipMemcpy(c.data(), dev, c.size() * 8, hipMemcpyDeviceToHost));
            JSP_HIP(hipMemset(dev, 0, c.size() * 8));
            unsigned long long h[8] = {0, 0, 0, 0, 0, 0, 0, 0};
            for (size_t i = 0; i < c.size(); ++i) h[i & 7] += c[i];
            const unsigned long long n = (unsigned long long)ntiles * clock_launches;
            std::fprintf(stderr, "fused clocks per tile (cycles; %d tiles x %d launches): load %llu | tables+trees %llu | look-back %llu | down %llu | replay %llu | decode %llu\n",
                         ntiles, clock_launches, h[0] / n, h[1] / n, h[2] / n, h[3] / n, h[4] / n, h[5] / n);
        }
        clock_launches = 0;
        if ((any_fused || needs_desc) && (*h_fault.as<const uint32_t>() || inject_fault)) {
            // A tile gave up waiting for the tile before it.  That says something about the GPU's timing (shared with other
            // work, serialised by a profiler), nothing about the stream: the batch is decoded again through the descriptor
            // path — msv1_parse_tiles / _chain / _emit build the block tables in three launches with no hand-off inside a
            // launch, the block kernels paint from them — and only what that path reports counts.
            inject_fault = false;
            ++fallback_runs;
            if (fallback_total) ++*fallback_total;
            note_kernel("msv1_parse_tiles (look-back fallback)");
            *h_fault.as<uint32_t>() = 0;
            hipStream_t stream = last_stream;
            quiesce_side();                            // (a table-writing launch may be running beside the stream: it shares the fault word, and its tables are not to be trusted either)
            JSP_HIP(hipMemsetAsync(d_sync.p, 0, MSV1_SYNC_BYTES, stream));
            launch_parse(stream);
            launch_groups(d_desc.as<const uint32_t>(), /*fused=*/false, stream);
            JSP_HIP(hipStreamSynchronize(stream));
        }
    }
    hipStream_t last_stream = nullptr;   // where decode() queued its launches
    bool inject_fault = false;           // tests (option "msv1_inject_fault"): the next after_sync() behaves as if a tile had given up
    int fallback_runs = 0;
    std::shared_ptr<std::atomic<long long>> fallback_total;   // the codec's jsp_counter("lookback_fallbacks")
};

// One frame on the asynchronous path (jsp_decompress_*_async) with the on-GPU parse.  Nothing here waits for the GPU; what the
// host could not know (stage-1 / stage-2 significance, a stream the host parser has to settle) is read from the frame's
// report once its event has fired (Msv1Codec::async_finish).  Frames of up to MSV1_MERGED_MAX_TILES tiles take ONE launch
// (msv1_fused_kernel mode 3: parse, frame-wide verdict, then the pixels or nothing; the record is a kernel argument, the
// report lands in pinned memory); larger ones, or "msv1_async" = "two_launches", a scout launch and a decode launch it may
// veto, with per-tile records and the report copied up and down.
struct Msv1AsyncStaged : jsp_staged {
    Msv1AsyncStaged() { verdict_pending = true; }
    Msv1Geometry geo{};
    Msv1AsyncShared shared;                   // the codec's palette, insignificant blocks and veto word, and this frame's tile size
    int ntiles = 0;
    size_t nbytes = 0;
    bool have_prev = false, compare = false, key = false;
    bool key_compare = false;                 // a key frame whose stage-2 compare answers option "key_frame_compare" (the kernel compares as it decodes)
    DeviceBuffer d_stream, d_meta, d_agg;     // d_meta = [tile records | Msv1AsyncInfo] (two-launch form)
    PinnedBuffer h_stream, h_meta, h_info;
    uint32_t epoch = 0;                        // never reset: d_agg is zeroed only when it is (re)allocated
    size_t agg_tiles = 0;
    // one-launch form (frames of at most MSV1_MERGED_MAX_TILES tiles): the record all tiles share travels as a kernel
    // argument, the report comes back through pinned memory, and the kernel reads the frame's bytes from pinned host
    // memory itself (the caller's, or h_stream), leaving a copy in d_stream: no copy is queued at all
    bool merged = false;
    bool deaf = false;                        // tests: see MSV1_LAB_DEAF
    Msv1TileRec rec{};
    DeviceBuffer d_report;                    // one Msv1AsyncInfo, allocated (and zeroed) once: its counters run on
    uint32_t want = 0;                        // ... to this value once every launch so far is through
    const uint8_t* src_dev = nullptr;         // device-side address of the frame's bytes in pinned host memory
    hipEvent_t uploaded = nullptr;            // (copy-engine form) the frame's bytes are in d_stream
    bool dma = false;
    // where the codec kept the last fully parsed frame's bytes before this frame was staged (Msv1Codec::async_reset puts it back)
    bool stale_before = false;
    const void* full_dev_before = nullptr;
    size_t full_dev_bytes_before = 0;
    ~Msv1AsyncStaged() override { if (uploaded) (void)hipEventDestroy(uploaded); }

    Msv1AsyncInfo* d_info() const {
        if (merged) return d_report.as<Msv1AsyncInfo>();
        return reinterpret_cast<Msv1AsyncInfo*>(d_meta.as<uint8_t>() + sizeof(Msv1TileRec) * (size_t)ntiles);
    }
    uint32_t bad_mask() const { return MSV1_ASYNC_SHORT | MSV1_ASYNC_END | MSV1_ASYNC_STUCK | (have_prev ? 0u : MSV1_ASYNC_SKIPCODE) | (deaf ? MSV1_LAB_DEAF : 0u); }
    // This frame as the one-launch form takes it (msv1.h, Msv1GroupFrame); the launch it goes into is counted on: `want` and the epoch move on, and
    // `stream` waits for the frame's bytes where the copy engine brings them up.
    Msv1GroupFrame group_frame(hipStream_t stream) {
        want += (uint32_t)ntiles;
        if (dma) JSP_HIP(hipStreamWaitEvent(stream, uploaded, 0));
        Msv1GroupFrame f;
        f.stream = src_dev;  f.keep = dma ? nullptr : d_stream.as<uint8_t>();  f.rec = rec;
        f.info = d_info();   f.host_info = h_info.as<Msv1AsyncInfo>();         f.want = want;
        f.agg = d_agg.as<unsigned long long>();  f.epoch = next_epoch(epoch);  f.bad_mask = bad_mask();
        return f;
    }
    // This frame and the ones submitted right behind it (at most MSV1_MAX_RIDERS) in ONE launch: all one-launch frames with the same tile
    // size (msv1.h, Msv1Riders).
    void decode_with(const std::vector<Msv1AsyncStaged*>& behind, hipStream_t stream) {
        Msv1GroupFrame frames[1 + MSV1_MAX_RIDERS] = {group_frame(stream)};
        int n = 1;
        for (Msv1AsyncStaged* next : behind) frames[n++] = next->group_frame(stream);
        msv1_launch_fused_group(geo, frames, n, shared, stream);
        JSP_HIP(hipGetLastError());
        decoded = true;
        for (Msv1AsyncStaged* next : behind) next->decoded = true;
    }
    void decode(hipStream_t stream) override {
        if (merged) { decode_with({}, stream); return; }
        Msv1FusedPass pass;
        pass.stream = d_stream.as<const uint8_t>();  pass.recs = d_meta.as<const Msv1TileRec>();  pass.ntiles = ntiles;
        pass.agg = d_agg.as<unsigned long long>();   pass.info = d_info();  pass.bad_mask = bad_mask();  pass.shared = shared;
        pass.epoch = next_epoch(epoch);
        msv1_launch_fused_scout(geo, pass, stream);
        pass.epoch = next_epoch(epoch);
        msv1_launch_fused_decode(geo, pass, stream);   // (the scout may have vetoed it)
        JSP_HIP(hipGetLastError());
        JSP_HIP(hipMemcpyAsync(h_info.p, pass.info, sizeof(Msv1AsyncInfo), hipMemcpyDeviceToHost, stream));
        decoded = true;
    }
};

// MSVideo1 codec instances of this process that have used the asynchronous one-launch path (see "msv1_async" = "auto")
std::atomic<int> g_async_streams{0};
constexpr int kDmaStreams = 3;

struct Msv1Codec : jsp_codec {
    Msv1Geometry geo{};
    size_t size_of_just_skips = 0;
    int insignificant_blocks = 0;
    bool insign_lines_set = false;  // the 8-bit Preinit never sets it (MSVideo1.hx:281-291)
    int insign_lines = 0;
    std::vector<uint8_t> block_changes;  // persists across calls, like the reference's member
    std::vector<uint8_t> palette_bytes;
    int32_t palette[256];
    DeviceBuffer d_palette;
    bool opt_gpu_parse = true;    // "msv1_parse": frames are parsed on the GPU unless the caller asks for the host parser
    bool opt_scrub_tables = false;
    bool opt_inject_fault = false;
    bool opt_inject_deaf = false;        // tests ("msv1_inject_fault" = "2"): the next one-launch asynchronous frame never sees all its tiles report
    std::shared_ptr<std::atomic<long long>> lookback_fallbacks = std::make_shared<std::atomic<long long>>(0);
    long long counter(const char* name) override {
        if (std::strcmp(name, "prefetched_frames") == 0) return prefetched_frames;
        if (std::strcmp(name, "paired_frames") == 0) return paired_frames;
        if (std::strcmp(name, "host_parsed_frames") == 0) return host_parsed_frames;
        if (std::strcmp(name, "msv1_block_changes") == 0) {   // (tests) the per-row flags of block rows 0..61 as bits
            std::vector<uint8_t> rows;
            try {
                if (!msv1_block_changes_now(this, rows)) return -1;
            } catch (const std::exception&) {
                return -1;
            }
            long long m = 0;
            for (size_t r = 0; r < rows.size() && r < 62; ++r) m |= (long long)(rows[r] != 0) << r;
            return m;
        }
        return std::strcmp(name, "lookback_fallbacks") == 0 ? lookback_fallbacks->load() : -1;
    }
    bool opt_async_merged = true, opt_async_dma = true, opt_async_auto = true;
    bool counted_async = false;   // this instance is in g_async_streams
    // The copy engine takes a frame's bytes up on a stream of its own, next to the previous frame's kernel.  One such stream is enough: a
    // megabyte per copy goes at ~30 GB/s on one stream where the bus takes 57 (bench.py: e2e.h2d_ceiling_GBs), but taking consecutive frames up
    // on 2 - 4 streams in turn changes nothing for one player stream (55.5 Gpixels/s with 1, 2, 3 or 4: the frames'
    // kernels follow each other on one HIP stream, 37 us apiece, and that chain is the bound) and costs 3 - 40 % with two (profiles/
    // r04_msv1_up_streams.txt).
    hipStream_t up_stream = nullptr;
    // jsp_prefetch: ranges of the caller's host memory that are (being) copied to the device in ONE piece each, on a stream of their own.
    // An asynchronous frame whose bytes lie inside such a range takes them from the device copy: no copy of its own is queued and
    // nothing crosses the bus inside its kernel.  A megabyte per copy goes at 24 - 39 GB/s, 64 MB at 57 (bench.py: e2e.h2d_ceiling_GBs),
    // and sixteen player streams that each queue a copy, an event and a wait per frame are bound by those queues, not by the bus.
    // A ring: the range prefetched kRanges calls ago is given up (after the kernels that read it: `last_use`).
    struct UpRange {
        const uint8_t* host = nullptr;
        size_t bytes = 0, skew = 0;           // the device copy starts at dev.p + skew: same offset inside a 64-byte line as `host`
        DeviceBuffer dev;
        hipEvent_t up = nullptr, last_use = nullptr;
        bool waited = false;                  // the codec's stream (`waited_on`) already waits for `up`
        hipStream_t waited_on = nullptr;
        bool used = false;                    // some kernel read it since it was uploaded
    };
    static constexpr int kRanges = 4;
    UpRange ranges[kRanges];
    unsigned range_next = 0;
    hipStream_t prefetch_stream = nullptr;
    long long prefetched_frames = 0;          // jsp_counter("prefetched_frames"): asynchronous frames that found their bytes on the device
    long long host_parsed_frames = 0;         // jsp_counter("host_parsed_frames"): frames staged with the on-GPU parse on that the host parser settled (frame_parse)
    int prefetch(const void* host, size_t n) override {
        if (!host || n == 0) {                // give every range up (the caller's memory changes or goes away)
            for (UpRange& r : ranges) { r.host = nullptr; r.bytes = 0; }
            return 0;
        }
        if (!opt_gpu_parse) return 0;         // (the host parser reads the caller's bytes: nothing to take up)
        launch_held();                        // (frames held for their successors may read the range that is about to be given up: their kernels go out first)
        UpRange& r = ranges[range_next++ % kRanges];
        r.host = nullptr;                     // (not to be found while it is being replaced)
        r.bytes = 0;
        if (!prefetch_stream) JSP_HIP(hipStreamCreateWithFlags(&prefetch_stream, hipStreamNonBlocking));
        if (!r.up) {
            JSP_HIP(hipEventCreateWithFlags(&r.up, hipEventDisableTiming));
            JSP_HIP(hipEventCreateWithFlags(&r.last_use, hipEventDisableTiming));
        }
        if (r.used) {                         // kernels queued so far may still read what the range held: the copy goes behind them
            JSP_HIP(hipEventRecord(r.last_use, stream));
            JSP_HIP(hipStreamWaitEvent(prefetch_stream, r.last_use, 0));
        }
        r.dev.reserve(n + 128);               // (growing frees the old copy: hipFree waits for the device)
        r.skew = (size_t)(reinterpret_cast<uintptr_t>(host) & 63u);
        JSP_HIP(hipMemcpyAsync(r.dev.as<uint8_t>() + r.skew, host, n, hipMemcpyHostToDevice, prefetch_stream));
        JSP_HIP(hipEventRecord(r.up, prefetch_stream));
        r.host = static_cast<const uint8_t*>(host);
        r.bytes = n;
        r.waited = false;
        r.used = false;
        return 0;
    }
    UpRange* range_of(const uint8_t* src, size_t n) {
        // NEWEST first: a caller that hands the same host address over again (a ring of file chunks, a file played again) means the bytes that
        // are there NOW — an older copy of that address may hold what was there before.  (Oldest first, until round 4, decoded from a copy two
        // passes old when a short file was played over and over.)
        for (int k = kRanges - 1; k >= 0; --k) {
            UpRange& r = ranges[(range_next + (unsigned)k) % kRanges];
            if (r.host && src >= r.host && n <= r.bytes && (size_t)(src - r.host) <= r.bytes - n) return &r;
        }
        return nullptr;
    }
    ~Msv1Codec() override {
        if (prefetch_stream) (void)hipStreamSynchronize(prefetch_stream);
        for (UpRange& r : ranges) {
            if (r.up) (void)hipEventDestroy(r.up);
            if (r.last_use) (void)hipEventDestroy(r.last_use);
        }
        if (prefetch_stream) (void)hipStreamDestroy(prefetch_stream);
        if (up_stream) (void)hipStreamDestroy(up_stream);
        if (counted_async) g_async_streams.fetch_sub(1);
    }
    // block_changes is only maintained by the host parser; after frames parsed on the GPU it is
    // rebuilt on demand from the bytes of the last fully parsed frame
    bool block_changes_stale = false;
    std::vector<uint8_t> last_full_frame;
    // asynchronous path: the last fully parsed frame's bytes stay where they are, in HBM, until somebody needs them
    const void* last_full_dev = nullptr;
    size_t last_full_dev_bytes = 0;
    DeviceBuffer d_poison;   // asynchronous path: set by a vetoed decode pass, cleared by async_reset()
    void async_reset(jsp_staged* failed) override {
        held.clear();            // (frames held for their successors are among those about to be re-run: they are never launched)
        if (d_poison.p) JSP_HIP(hipMemsetAsync(d_poison.p, 0, sizeof(uint32_t), stream));
        // stage_async() named the failed frame (and the frames behind it) as the last fully parsed one; it is not — an end marker, a
        // short stream.  The host parser that re-runs it must rebuild block_changes from the frame that was, as before the failed one
        if (auto* st = dynamic_cast<Msv1AsyncStaged*>(failed)) {
            block_changes_stale = st->stale_before;
            last_full_dev = st->full_dev_before;
            last_full_dev_bytes = st->full_dev_bytes_before;
        }
    }
    // Replays of staged inter-frame batches (Msv1Staged::decode): "msv1_parse_ahead" (default on).
    bool opt_parse_ahead = true;
    // Several frames per launch (option "msv1_async_pairs", default on): a one-launch frame is HELD until enough frames are submitted behind it
    // — half of what may be in flight ("async_depth"), at most 1 + MSV1_MAX_RIDERS — and they go out together (Msv1AsyncStaged::decode_with);
    // or with whatever is held, as soon as anybody waits for one of them or anything else needs the stream.
    bool opt_async_pairs = true;
    std::vector<jsp_async_job*> held;
    long long paired_frames = 0;      // jsp_counter("paired_frames"): frames that shared a launch with others
    int frames_per_launch() const {
        const int k = async_depth / 2;
        return k < 1 ? 1 : (k > 1 + MSV1_MAX_RIDERS ? 1 + MSV1_MAX_RIDERS : k);
    }
    void launch_held() {
        if (held.empty()) return;
        activate();
        std::vector<jsp_async_job*> group;
        group.swap(held);
        auto* first = static_cast<Msv1AsyncStaged*>(group[0]->st.get());
        if (group.size() == 1) {
            first->decode(stream);
        } else {
            std::vector<Msv1AsyncStaged*> behind;
            for (size_t i = 1; i < group.size(); ++i) behind.push_back(static_cast<Msv1AsyncStaged*>(group[i]->st.get()));
            first->decode_with(behind, stream);
            paired_frames += (long long)group.size();
        }
        for (jsp_async_job* j : group) JSP_HIP(hipEventRecord(j->done, stream));
    }
    bool async_launch(jsp_async_job& j) override {
        auto* st = dynamic_cast<Msv1AsyncStaged*>(j.st.get());
        const int k = frames_per_launch();
        if (!st || !st->merged || !opt_async_pairs || k < 2) { launch_held(); return false; }
        if (!held.empty() && static_cast<Msv1AsyncStaged*>(held[0]->st.get())->shared.small_tiles != st->shared.small_tiles) launch_held();
        held.push_back(&j);
        if ((int)held.size() >= k) launch_held();
        return true;
    }
    void async_flush(const jsp_async_job* only_if_held) override {
        if (held.empty()) return;
        if (!only_if_held || std::find(held.begin(), held.end(), only_if_held) != held.end()) launch_held();
    }
    void worker_drain() override { launch_held(); }   // (every call that needs the stream's work queued, or waits for it, comes through here)

    Msv1Codec(int bits, int w, int h, const uint8_t* pal, int pal_bytes) {
        kind = bits == 16 ? JSP_CODEC_MSVIDEO1_16 : JSP_CODEC_MSVIDEO1_8;
        X = w;
        Y = h;
        geo.bits = bits;
        geo.X = w;
        geo.Y = h;
        geo.nbx = w >> 2;
        geo.nby = h >> 2;
        geo.nblocks = geo.nbx * geo.nby;
        size_of_just_skips = (size_t)(geo.nblocks / 1023) * 2 + 10;  // MSVideo1.hx:29-30
        block_changes.assign(std::max(geo.nby, 0), 0);
        std::memset(palette, 0, sizeof palette);
        if (pal && pal_bytes > 0) palette_bytes.assign(pal, pal + pal_bytes);
    }

    int preinit(int lines) override {
        launch_held();                        // (frames held for a group launch were staged under the settings so far)
        insignificant_blocks = (lines + 3) >> 2;
        if (geo.bits == 16) {
            insign_lines = lines;
            insign_lines_set = true;
        } else {
            // readUnsignedInt() on the strf palette bytes, little-endian
            size_t pos = 0;
            int i = 0;
            while (i < 256 && palette_bytes.size() - pos >= 4) {
                uint32_t v;
                std::memcpy(&v, palette_bytes.data() + pos, 4);
                palette[i++] = (int32_t)v;
                pos += 4;
            }
            activate();
            d_palette.reserve(sizeof palette);
            JSP_HIP(hipMemcpy(d_palette.p, palette, sizeof palette, hipMemcpyHostToDevice));
        }
        return JSP_ZERO_STATE;
    }

    int is_key_frame(const uint8_t* src, size_t n) override { return msv1_is_key_frame(geo, src, n); }
    int needs_index() override { return 1; }
    bool may_leave_pixels(const jsp_frame_in&) override {
        // remainders outside the block grid are never written; an 8-bit end marker or an abort
        // can leave more.  Cheap to be conservative: only exact multiples of 4 with a 16-bit
        // stream are guaranteed to be fully written.
        // ... and while there is no previous frame a skip code aborts the frame (the reference raises), leaving
        // every block after it as the caller had it
        return (X & 3) || (Y & 3) || geo.bits == 8 || !prev_dev;
    }
    int set_option(const char* key, const char* value) override {
        if (std::strcmp(key, "msv1_parse") == 0) {
            if (std::strcmp(value, "gpu") == 0) { opt_gpu_parse = true; return 0; }
            if (std::strcmp(value, "host") == 0) { opt_gpu_parse = false; return 0; }
        }
        if (std::strcmp(key, "msv1_inject_fault") == 0) {   // tests: the next staged batch behaves as if a tile's look-back had timed out
            opt_inject_fault = std::strcmp(value, "1") == 0;
            opt_inject_deaf = std::strcmp(value, "2") == 0;   // ... or the next one-launch asynchronous frame as if its verdict wait had
            return 0;
        }
        if (std::strcmp(key, "msv1_async_pairs") == 0) {    // one-launch asynchronous frames two to a launch (on) or one by one (off)
            if (std::strcmp(value, "on") != 0 && std::strcmp(value, "off") != 0) return JSP_ERROR_OCCURED;
            launch_held();
            opt_async_pairs = std::strcmp(value, "on") == 0;
            return 0;
        }
        if (std::strcmp(key, "msv1_parse_ahead") == 0) {    // replays of an inter-frame batch: the next replay's table-writing parse beside this replay's launches (on), or in front of them (off)
            if (std::strcmp(value, "on") != 0 && std::strcmp(value, "off") != 0) return JSP_ERROR_OCCURED;
            opt_parse_ahead = std::strcmp(value, "on") == 0;
            return 0;
        }
        if (std::strcmp(key, "msv1_seek_chunk_frames") == 0) {   // jsp_seek: frames staged and composed per chunk ("auto": by a byte budget)
            if (std::strcmp(value, "auto") == 0) { seek_chunk_frames = 0; return 0; }
            char* end = nullptr;
            const long v = std::strtol(value, &end, 10);
            if (end == value || *end || v < 1 || v > (1 << 24)) return -1;
            seek_chunk_frames = (int)v;
            return 0;
        }
        if (std::strcmp(key, "msv1_index_play_segments") == 0) {   // jsp_index_play: segments of the run along grid.y ("auto": ~8 waves per SIMD)
            if (std::strcmp(value, "auto") == 0) { index_play_segments = 0; return 0; }
            char* end = nullptr;
            const long v = std::strtol(value, &end, 10);
            if (end == value || *end || v < 1 || v > 64) return -1;
            index_play_segments = (int)v;
            return 0;
        }
        if (std::strcmp(key, "msv1_index_activity_segments") == 0) {   // jsp_index_activity: segments of the run along grid.y ("auto": as Play's)
            if (std::strcmp(value, "auto") == 0) { index_activity_segments = 0; return 0; }
            char* end = nullptr;
            const long v = std::strtol(value, &end, 10);
            if (end == value || *end || v < 1 || v > 64) return -1;
            index_activity_segments = (int)v;
            return 0;
        }
        if (std::strcmp(key, "msv1_index_delta_slice") == 0) {   // jsp_index_delta_frames: pairs per slice ("auto": by a byte budget of scratch)
            if (std::strcmp(value, "auto") == 0) { index_delta_slice = 0; return 0; }
            char* end = nullptr;
            const long v = std::strtol(value, &end, 10);
            if (end == value || *end || v < 1 || v > 4096) return -1;
            index_delta_slice = (int)v;
            return 0;
        }
        if (std::strcmp(key, "msv1_scrub_tables") == 0) {   // tests: a replay must rebuild every block table it reads
            opt_scrub_tables = std::strcmp(value, "1") == 0;
            return 0;
        }
        if (std::strcmp(key, "msv1_async") == 0) {   // frames of up to MSV1_MERGED_MAX_TILES tiles: one launch, or scout + decode
            if (std::strcmp(value, "auto") == 0) { opt_async_merged = true; opt_async_auto = true; return 0; }
            if (std::strcmp(value, "one_launch") == 0) { opt_async_merged = true; opt_async_auto = false; opt_async_dma = false; return 0; }
            if (std::strcmp(value, "one_launch_dma") == 0) { opt_async_merged = true; opt_async_auto = false; opt_async_dma = true; return 0; }
            if (std::strcmp(value, "two_launches") == 0) { opt_async_merged = false; return 0; }
        }
        return -1;
    }

    // Host parse of one frame into `desc`, keeping block_changes exact.
    void host_parse(const uint8_t* src, size_t n, uint32_t base, uint32_t* desc, Msv1Parse& pr) {
        if (block_changes_stale && last_full_dev) {   // (asynchronous path) fetch that frame's bytes from HBM first
            JSP_HIP(hipStreamSynchronize(stream));
            last_full_frame.resize(last_full_dev_bytes);
            if (last_full_dev_bytes) JSP_HIP(hipMemcpy(last_full_frame.data(), last_full_dev, last_full_dev_bytes, hipMemcpyDeviceToHost));
            last_full_dev = nullptr;
        }
        if (block_changes_stale) {  // replay the last GPU-parsed frame to recover the per-row flags
            std::vector<uint32_t> scratch((size_t)std::max(geo.nblocks, 1));
            Msv1Parse tmp;
            msv1_parse(geo, last_full_frame.data(), last_full_frame.size(), true, 0, insignificant_blocks, 0,
                       scratch.data(), block_changes, tmp);
            block_changes_stale = false;
        }
        msv1_parse(geo, src, n, prev_dev != nullptr, size_of_just_skips, insignificant_blocks, base, desc,
                   block_changes, pr);
    }

    // What the host can tell about a frame without parsing it: `changes` (a coded block is on the chain — the chain
    // starts at byte 0 and leading skip codes are one slot each, so the first coded block is found by walking them) and
    // whether the frame is one the asynchronous path leaves to the synchronous one.
    struct Prescan { bool sync_path, changes; };
    Prescan prescan(const uint8_t* src, size_t n) const {
        if (n < 2 || (geo.bits == 16 && n < size_of_just_skips)) return {true, false};   // early-outs / tiny frames: host parser
        long covered = 0;
        for (size_t si = 0; si + 1 < n && covered < geo.nblocks; si += 2) {
            const unsigned a = src[si], b = src[si + 1];
            if (geo.bits == 8 && a == 0 && b == 0) return {true, false};                 // end marker at the head of the chain
            if ((b & 0xFC) != 0x84) return {false, true};                                // a coded block
            const long cnt = (long)(((b - 0x84) << 8) + a);
            if (cnt == 0) return {true, false};                                          // "skip -1": everything left is copied
            covered += cnt;
        }
        return {covered < geo.nblocks, false};   // all skip codes: nothing coded; too short = host parser
    }

    // frames the scout + vetoable decode pair cannot take: they go through the synchronous staging
    bool sync_staging(const jsp_frame_in& f, const Prescan& ps) const {
        const bool aligned = (X & 3) == 0 && !(reinterpret_cast<uintptr_t>(f.dst) & 15) && !(reinterpret_cast<uintptr_t>(prev_dev) & 15);
        return !opt_gpu_parse || !aligned || (Y & 3) || ps.sync_path || geo.nblocks <= 0 || geo.nblocks >= (1 << 20) ||
               f.n + msv1_parse_tile_bytes() > 0xFFFFFFF0u || (geo.bits == 8 && !d_palette.p);
    }
    bool async_settle_first(const jsp_frame_in& f) override { return sync_staging(f, prescan(f.src, f.n)); }
    bool sync_through_async() const override { return opt_gpu_parse; }

    // the buffers of an asynchronous frame of `nt` tiles: kept from frame to frame, grown (and zeroed where the kernel counts on it) when a frame needs more
    void reserve_async_buffers(Msv1AsyncStaged& st, int nt, size_t tile_bytes) {
        st.d_stream.reserve((size_t)nt * tile_bytes + 64);
        st.h_info.reserve(sizeof(Msv1AsyncInfo));
        if ((size_t)nt > st.agg_tiles) {   // published tile tables carry the launch epoch: fresh memory must read as epoch 0
            st.d_agg.reserve(sizeof(unsigned long long) * 9 * (size_t)nt);
            st.agg_tiles = st.d_agg.cap / (sizeof(unsigned long long) * 9);
            JSP_HIP(hipMemsetAsync(st.d_agg.p, 0, st.d_agg.cap, stream));
        }
        if (st.merged && !st.d_report.p) {
            st.d_report.reserve(sizeof(Msv1AsyncInfo));
            JSP_HIP(hipMemsetAsync(st.d_report.p, 0, sizeof(Msv1AsyncInfo), stream));
            st.want = 0;
        }
        if (!st.merged) {
            const size_t meta_bytes = sizeof(Msv1TileRec) * (size_t)nt + sizeof(Msv1AsyncInfo);
            st.d_meta.reserve(meta_bytes);
            st.h_meta.reserve(meta_bytes);
        }
    }

    // An asynchronous frame's bytes: on the device already when the caller had the range prefetched (jsp_prefetch); else from where they are
    // when the caller keeps them in pinned memory, else through our own.  `up`: where a copy reads them, `up_dev`: where a kernel does.
    struct FrameBytes { const void* up; const uint8_t* up_dev; UpRange* range; };
    FrameBytes frame_bytes(const jsp_frame_in& f, Msv1AsyncStaged& st) {
        hipPointerAttribute_t attr{};
        UpRange* range = range_of(f.src, f.n);
        if (range) {
            if (!range->waited || range->waited_on != stream) {   // the first frame out of the range: the frames' stream waits for the range's copy once
                JSP_HIP(hipStreamWaitEvent(stream, range->up, 0));
                range->waited = true;
                range->waited_on = stream;
            }
            range->used = true;
            ++prefetched_frames;
            return {f.src, range->dev.as<const uint8_t>() + range->skew + (f.src - range->host), range};
        }
        if (hipPointerGetAttributes(&attr, f.src) == hipSuccess && attr.type == hipMemoryTypeHost)
            return {f.src, static_cast<const uint8_t*>(attr.devicePointer ? attr.devicePointer : f.src), nullptr};
        (void)hipGetLastError();
        st.h_stream.reserve(f.n + 16);
        std::memcpy(st.h_stream.p, f.src, f.n);
        return {st.h_stream.p, st.h_stream.as<const uint8_t>(), nullptr};
    }

    // The bytes of the last fully parsed frame stay in the staged object that brought them up, and two parties may come back for them:
    // the codec (block_changes_stale: host_parse / msv1_block_changes_now replay last_full_dev) and a frame in flight that the GPU may yet
    // veto (async_reset puts back full_dev_before).  A staged object whose buffer either of them may still read is not written again:
    // stage_async() sets the buffer aside first — a swap with d_aside, no copy, no wait.  One spare is enough while the ring is used in
    // order: with nothing in flight only the codec's pointer counts (async_depth 1: every frame is staged into the object of the frame
    // before it), and of the frames in flight only the oldest has the frame before it in an object that is free to be staged again.
    DeviceBuffer d_aside;
    bool a_rerun_reads(const void* p) const {
        if (!p) return false;
        if (block_changes_stale && last_full_dev == p) return true;
        for (uint64_t t = oldest_ticket; t < next_ticket; ++t) {
            auto* a = dynamic_cast<const Msv1AsyncStaged*>(jobs[t % (uint64_t)async_depth].st.get());
            if (a && a->stale_before && a->full_dev_before == p) return true;
        }
        return false;
    }
    void set_aside_what_a_rerun_reads(Msv1AsyncStaged& st) {
        if (!a_rerun_reads(st.d_stream.p)) return;
        if (a_rerun_reads(d_aside.p)) {   // (the spare is spoken for as well: not while the ring is used in order — settle for a host copy)
            forget_device_bytes(st.d_stream.p);
            return;
        }
        std::swap(d_aside.p, st.d_stream.p);
        std::swap(d_aside.cap, st.d_stream.cap);
    }
    // Nobody keeps a pointer to the bytes in `p` after this: the codec's go to last_full_frame; a frame in flight that is vetoed replays
    // last_full_frame as it then is (live memory; its flags past an end marker may be older than the reference's)
    void forget_device_bytes(const void* p) {
        if (block_changes_stale && last_full_dev == p) {
            JSP_HIP(hipStreamSynchronize(stream));
            last_full_frame.resize(last_full_dev_bytes);
            if (last_full_dev_bytes) JSP_HIP(hipMemcpy(last_full_frame.data(), last_full_dev, last_full_dev_bytes, hipMemcpyDeviceToHost));
            last_full_dev = nullptr;
        }
        for (uint64_t t = oldest_ticket; t < next_ticket; ++t) {
            auto* a = dynamic_cast<Msv1AsyncStaged*>(jobs[t % (uint64_t)async_depth].st.get());
            if (a && a->full_dev_before == p) { a->full_dev_before = nullptr; a->full_dev_bytes_before = 0; }
        }
    }

    jsp_staged* stage_async(const jsp_frame_in& f, jsp_staged* reuse) override {
        activate();
        const bool small_tiles = f.n <= MSV1_SMALL_TILE_FRAME_BYTES;
        const size_t tile_bytes = small_tiles ? msv1_small_tile_bytes() : msv1_parse_tile_bytes();
        const Prescan ps = prescan(f.src, f.n);
        if (sync_staging(f, ps)) {
            // the synchronous staging (it may wait for the GPU: tiny, odd or pre-parsed frames only)
            return stage(std::vector<jsp_frame_in>{f}, dynamic_cast<Msv1Staged*>(reuse));
        }
        const double t0 = now_ms();
        auto* st = dynamic_cast<Msv1AsyncStaged*>(reuse);
        std::unique_ptr<Msv1AsyncStaged> guard;
        if (!st) { st = new Msv1AsyncStaged(); guard.reset(st); }
        else set_aside_what_a_rerun_reads(*st);
        st->geo = geo;
        st->shared.palette = d_palette.as<const int32_t>();
        st->shared.insignificant_blocks = insignificant_blocks;
        st->decoded = false;
        st->why.clear();
        st->status.assign(1, JSP_ZERO_STATE);
        st->adopted.assign(1, ps.changes ? 1 : 0);
        st->significant.assign(1, 0);
        st->cleared.assign(1, 0);
        st->nbytes = f.n;
        st->have_prev = prev_dev != nullptr;
        st->key = f.key;
        if (!d_poison.p) {
            d_poison.reserve(sizeof(uint32_t));
            JSP_HIP(hipMemsetAsync(d_poison.p, 0, sizeof(uint32_t), stream));
        }
        st->shared.poison = d_poison.as<uint32_t>();
        // inter frames with a previous frame are compared against it in any case (whether the result counts is known
        // only with the stage-1 flag the kernel reports)
        st->compare = geo.bits == 16 && insign_lines_set && !f.key && prev_dev != nullptr;
        // option "key_frame_compare": a key frame is compared with the frame before it by the very kernel that decodes it (the stage-2
        // compare of the inter frames, MSVideo1.hx:195-204, from the Manager's row on) — when the block grid covers the frame
        st->key_compare = f.key && key_compare_row >= 0 && prev_dev != nullptr && ps.changes && (X & 3) == 0 && (Y & 3) == 0;
        st->key_differs.assign(1, st->key_compare ? -3 : -2);   // -3: async_finish() says (jsp_api.cpp)
        if (st->key_compare) st->compare = true;
        const size_t n_even = f.n & ~size_t(1);
        const int nt = (int)((f.n + tile_bytes - 1) / tile_bytes);
        st->ntiles = nt;
        st->merged = opt_async_merged && nt <= MSV1_MERGED_MAX_TILES;
        st->shared.small_tiles = small_tiles;
        st->deaf = st->merged && opt_inject_deaf;
        if (st->deaf) opt_inject_deaf = false;
        reserve_async_buffers(*st, nt, tile_bytes);
        const size_t meta_bytes = sizeof(Msv1TileRec) * (size_t)nt + sizeof(Msv1AsyncInfo);
        auto* info_dev = st->d_info();
        const uint32_t cmp_row_lo = st->key_compare ? (uint32_t)key_compare_row : st->compare ? (uint32_t)std::max(insign_lines, 0) : 0xFFFFFFFFu;
        auto rec = [&](int k) {
            return tile_rec(0, (uint32_t)n_even, geo.bits == 16 ? (uint32_t)n_even : (uint32_t)f.n, (uint32_t)k, (uint32_t)tile_bytes, 0, (uint32_t)nt, f.dst, prev_dev,
                            &info_dev->signif, cmp_row_lo, 0);
        };
        const FrameBytes fb = frame_bytes(f, *st);
        if (st->merged) {
            st->rec = rec(0);
            st->src_dev = fb.up_dev;
            if (!counted_async) { counted_async = true; g_async_streams.fetch_add(1); }
            // a few streams: the copy engine works next to the kernels; many: its queues become the bottleneck (16 streams on one
            // GPU: 57 against 68 Gpixels/s), the kernels then fetch the bytes themselves
            st->dma = opt_async_auto ? g_async_streams.load() <= kDmaStreams : opt_async_dma;
            if (fb.range) st->dma = false;      // (the kernel reads the device copy of the range and leaves the frame's own copy in d_stream, as when it reads pinned memory)
            if (st->dma) {   // the copy engine brings the bytes up on a stream of its own, next to the previous frame's kernel
                if (!up_stream) JSP_HIP(hipStreamCreateWithFlags(&up_stream, hipStreamNonBlocking));
                if (!st->uploaded) JSP_HIP(hipEventCreateWithFlags(&st->uploaded, hipEventDisableTiming));
                JSP_HIP(hipMemcpyAsync(st->d_stream.p, fb.up, f.n, hipMemcpyHostToDevice, up_stream));
                JSP_HIP(hipEventRecord(st->uploaded, up_stream));
                st->src_dev = st->d_stream.as<const uint8_t>();
            }
        } else {
            auto* recs = st->h_meta.as<Msv1TileRec>();
            for (int k = 0; k < nt; ++k) recs[k] = rec(k);
            std::memset(recs + nt, 0, sizeof(Msv1AsyncInfo));
            if (fb.range) JSP_HIP(hipMemcpyAsync(st->d_stream.p, fb.up_dev, f.n, hipMemcpyDeviceToDevice, stream));   // (larger frames: from the range's copy to the frame's own)
            else JSP_HIP(hipMemcpyAsync(st->d_stream.p, fb.up, f.n, hipMemcpyHostToDevice, stream));
            JSP_HIP(hipMemcpyAsync(st->d_meta.p, recs, meta_bytes, hipMemcpyHostToDevice, stream));
        }
        // codec state, as the synchronous path leaves it — a frame that is fully parsed: should the GPU find that it is not, async_reset()
        // puts back what is overwritten here before the frame is re-run
        st->stale_before = block_changes_stale;
        st->full_dev_before = last_full_dev;
        st->full_dev_bytes_before = last_full_dev_bytes;
        if (ps.changes) prev_dev = f.dst;
        block_changes_stale = true;
        last_full_dev = st->d_stream.p;
        last_full_dev_bytes = f.n;
        st->info = jsp_staged_info{};
        st->info.frames = 1;
        st->info.pixels = (uint64_t)X * Y;
        st->info.stream_bytes = f.n;
        st->info.kernel_launches = st->merged ? 1 : 2;
        st->info.host_stage_ms = now_ms() - t0;
        st->kernels = "msv1_fused_kernel";
        guard.release();
        return st;
    }

    bool async_finish(jsp_staged* base) override {
        auto* st = dynamic_cast<Msv1AsyncStaged*>(base);
        if (!st) return true;                                    // went through the synchronous staging: already settled
        const Msv1AsyncInfo& in = *st->h_info.as<const Msv1AsyncInfo>();
        if (in.fault) return false;                              // a tile gave up waiting (timing, not the stream): the host path settles the frame
        if ((in.flags & (MSV1_ASYNC_SHORT | MSV1_ASYNC_END | MSV1_ASYNC_STUCK)) || ((in.flags & MSV1_ASYNC_SKIPCODE) && !st->have_prev))
            return false;                                        // the host parser has to settle this stream
        const int sg = msv1_significance(st->adopted[0] && (in.flags & MSV1_ASYNC_S1), st->have_prev, st->key, st->compare);
        st->significant[0] = sg < 0 ? (in.signif ? 1 : 0) : sg;   // (stage 2 ran with the frame: its word is in the report)
        if (st->key_compare) st->key_differs[0] = in.signif ? 1 : 0;
        return true;
    }

    // The synchronous staging of a batch, phase by phase; what the phases hand on to each other is in StagePlan.
    jsp_staged* stage(const std::vector<jsp_frame_in>& frames, jsp_staged* reuse) override {
        activate();
        const double t0 = now_ms();
        auto* st = dynamic_cast<Msv1Staged*>(reuse);
        if (!st) st = new Msv1Staged();
        std::unique_ptr<Msv1Staged> guard(reuse ? nullptr : st);
        StagePlan plan;
        reset_batch(*st, (int)frames.size());
        lay_out_and_gather(frames, *st, plan);
        if (st->gpu_parse && !frames.empty()) parse_on_gpu(frames, *st, plan);
        decide_frames(frames, *st, plan);
        st->plan_launches(frames, plan);
        st->account(plan);
        st->build_tile_records(frames, plan, opt_scrub_tables, stream);
        st->info.host_stage_ms = now_ms() - t0 - plan.gpu_parse_ms;
        final_uploads(*st, plan);
        st->info.h2d_ms = plan.h2d_ms;
        st->info.device_parse_ms = plan.gpu_parse_ms;
        guard.release();
        return st;
    }

    void upload(void* d, const void* h, size_t bytes) {   // queued on the codec's stream and waited for once, where the host needs them
        if (bytes) JSP_HIP(hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, stream));
    }

    // ---- phase 1: the batch object as a fresh one would be, its side stream, the palette ----
    void reset_batch(Msv1Staged& st, int nf) {
        st.quiesce_side();                             // (a reused batch: nothing of its last replay still runs beside the stream)
        st.drop_sets();
        st.side = nullptr;
        if (opt_parse_ahead) {
            if (!side_stream) JSP_HIP(hipStreamCreateWithFlags(&side_stream, hipStreamNonBlocking));
            st.side = side_stream;
        }
        st.geo = geo;
        st.nframes = nf;
        st.decoded = false;
        st.groups.clear();
        st.status.assign(nf, JSP_ZERO_STATE);
        st.adopted.assign(nf, 0);
        st.significant.assign(nf, 0);
        st.info = jsp_staged_info{};
        st.why.clear();
        st.insignificant_blocks = insignificant_blocks;
        st.inject_fault = opt_inject_fault;
        st.fallback_total = lookback_fallbacks;
        // the on-GPU parse packs block counts in 20 bits
        st.gpu_parse = opt_gpu_parse && geo.nblocks > 0 && geo.nblocks < (1 << 20);
        if (geo.bits == 8 && !d_palette.p) {  // Preinit not called: all-zero palette
            d_palette.reserve(sizeof palette);
            JSP_HIP(hipMemcpy(d_palette.p, palette, sizeof palette, hipMemcpyHostToDevice));
        }
        st.d_palette = d_palette.as<const int32_t>();
    }

    // ---- phase 2: lay the frames out in one stream buffer (16-byte aligned starts) and gather those that are not in pinned memory ----
    // With the on-GPU parse every frame starts on a tile boundary of the stream buffer, so tile t of the batch is the
    // bytes [t * tile, (t + 1) * tile): a workgroup of the fused kernel knows where its bytes are from its index alone.
    void lay_out_and_gather(const std::vector<jsp_frame_in>& frames, Msv1Staged& st, StagePlan& plan) {
        const int nf = (int)frames.size();
        const size_t nblk = (size_t)std::max(geo.nblocks, 1);
        plan.beg.resize(nf);
        const size_t frame_align = st.gpu_parse ? (size_t)msv1_parse_tile_bytes() : 16;
        for (int i = 0; i < nf; ++i) {
            plan.beg[i] = plan.total_stream;
            plan.total_stream += (frames[i].n + frame_align - 1) / frame_align * frame_align;
        }
        if (plan.total_stream + 64 > 0xFFFFFFF0u) throw std::runtime_error("batch stream exceeds 4 GiB");
        // Where the frames' bytes are: a frame in pinned host memory (jsp_host_alloc, or memory the caller registered) is uploaded
        // from where it is; the others are first gathered in the batch's own pinned buffer.
        plan.in_pinned.assign(nf, 0);
        size_t gather_bytes = 0;
        for (int i = 0; i < nf; ++i) {
            if (st.gpu_parse && frames[i].n >= 4096) {
                hipPointerAttribute_t attr{};
                if (hipPointerGetAttributes(&attr, frames[i].src) == hipSuccess && attr.type == hipMemoryTypeHost) plan.in_pinned[i] = 1;
                else (void)hipGetLastError();      // plain malloc'd memory: not known to HIP
            }
            if (!plan.in_pinned[i]) gather_bytes += frames[i].n;
        }
        if (gather_bytes || !st.gpu_parse) st.h_stream.reserve(plan.total_stream + 64);
        // (host-built block tables: every frame's with the host parser, else only those of the frames the GPU cannot settle —
        // allocated when the first such frame turns up: a quarter of a gigabyte of pinned memory for 512 frames)
        if (!st.gpu_parse) st.h_desc.reserve(sizeof(uint32_t) * nblk * std::max(nf, 1));
        st.h_frames.reserve(sizeof(Msv1FrameArgs) * std::max(nf, 1));
        st.d_signif.reserve(sizeof(uint32_t) * std::max(nf, 1));
        st.h_signif.reserve(sizeof(uint32_t) * std::max(nf, 1));
        st.d_stream.reserve(plan.total_stream + 64);
        st.d_desc.reserve(sizeof(uint32_t) * nblk * std::max(nf, 1));
        st.d_frames.reserve(sizeof(Msv1FrameArgs) * std::max(nf, 1));
        // gathered on several threads when there is much to gather: one thread copies ~6 GB/s, a batch of 512 1080p frames
        // is half a gigabyte
        auto* h_stream = st.h_stream.as<uint8_t>();
        auto gather = [&](int lo, int hi) {
            for (int i = lo; i < hi; ++i) {
                if (plan.in_pinned[i]) continue;
                if (frames[i].n) std::memcpy(h_stream + plan.beg[i], frames[i].src, frames[i].n);
                const size_t padded = (frames[i].n + 15) & ~size_t(15);   // (the rest of the frame's slot is never read)
                std::memset(h_stream + plan.beg[i] + frames[i].n, 0, padded - frames[i].n);
            }
        };
        const int nthreads = gather_bytes > (32u << 20) ? (int)std::min<size_t>(8, (size_t)std::max(1, usable_cpus() / 2)) : 1;
        if (nthreads > 1) {
            std::vector<std::thread> pool;
            std::exception_ptr failed;
            try {
                for (int t = 1; t < nthreads; ++t) pool.emplace_back(gather, (int)((long)nf * t / nthreads), (int)((long)nf * (t + 1) / nthreads));
                gather(0, nf / nthreads);
            } catch (...) {
                failed = std::current_exception();
            }
            for (auto& th : pool) th.join();
            if (failed) std::rethrow_exception(failed);
        } else {
            gather(0, nf);
        }
    }

    // the batch's stream buffer in HBM: runs of gathered frames go up in one copy each, pinned frames one by one
    void upload_stream(const std::vector<jsp_frame_in>& frames, Msv1Staged& st, const StagePlan& plan) {
        const int nf = (int)frames.size();
        const auto* h_stream = st.h_stream.as<const uint8_t>();
        auto* d_stream = st.d_stream.as<uint8_t>();
        int i = 0;
        while (i < nf) {
            if (plan.in_pinned[i]) {
                upload(d_stream + plan.beg[i], frames[i].src, frames[i].n);
                ++i;
                continue;
            }
            int j = i;
            while (j < nf && !plan.in_pinned[j]) ++j;
            const size_t lo = plan.beg[i], hi = j < nf ? plan.beg[j] : plan.total_stream;
            if (hi > lo) upload(d_stream + lo, h_stream + lo, hi - lo);
            i = j;
        }
    }

    // ---- phase 3, on-GPU parse: upload the raw bytes, parse, read the per-frame counters back ----
    void parse_on_gpu(const std::vector<jsp_frame_in>& frames, Msv1Staged& st, StagePlan& plan) {
        const int nf = (int)frames.size();
        const size_t nblk = (size_t)std::max(geo.nblocks, 1);
        const uint32_t tile_bytes = msv1_parse_tile_bytes();
        st.h_pframes.reserve(sizeof(Msv1ParseFrame) * nf);
        Msv1ParseFrame* h_pf = plan.h_pf = st.h_pframes.as<Msv1ParseFrame>();
        int ntiles = 0, max_tiles = 1;
        for (int i = 0; i < nf; ++i) {
            // an odd trailing byte is left to the host parser (it only matters when the chain reaches it,
            // and then the stream counts as too short)
            const size_t n_even = frames[i].n & ~size_t(1);
            // the frame's slot in the stream buffer, in tiles (the last one is all padding when an odd trailing
            // byte is the only thing in it: it parses as "covers nothing")
            const int t = (int)((frames[i].n + tile_bytes - 1) / tile_bytes);
            // 16-bit early-outs (MSVideo1.hx:109-110) are settled by the host parser
            const bool pre_host = geo.bits == 16 && frames[i].n < size_of_just_skips;
            h_pf[i] = Msv1ParseFrame{(uint32_t)plan.beg[i], (uint32_t)(plan.beg[i] + n_even), (uint32_t)(i * nblk), (uint32_t)ntiles,
                                     (uint32_t)t, pre_host || t == 0 ? 1u : 0u, 0, 0};
            ntiles += t;
            max_tiles = std::max(max_tiles, t);
        }
        st.ntiles = ntiles;
        st.max_tiles = max_tiles;
        st.h_tile_frame.reserve(sizeof(uint32_t) * std::max(ntiles, 1));
        auto* h_tf = st.h_tile_frame.as<uint32_t>();
        for (int i = 0; i < nf; ++i)
            for (uint32_t k = 0; k < h_pf[i].ntiles; ++k) h_tf[h_pf[i].first_tile + k] = (uint32_t)i;
        st.d_pframes.reserve(sizeof(Msv1ParseFrame) * nf);
        st.d_tile_frame.reserve(sizeof(uint32_t) * std::max(ntiles, 1));
        st.d_tile_tab.reserve(sizeof(uint32_t) * 9 * std::max(ntiles, 1));
        st.d_tile_entry.reserve(sizeof(uint32_t) * std::max(ntiles, 1));
        st.d_tile_block0.reserve(sizeof(uint32_t) * std::max(ntiles, 1));
        st.d_info.reserve(sizeof(Msv1FrameInfo) * nf);
        st.h_info.reserve(sizeof(Msv1FrameInfo) * nf);
        const double tu = now_ms();
        upload_stream(frames, st, plan);
        upload(st.d_pframes.p, h_pf, sizeof(Msv1ParseFrame) * nf);
        upload(st.d_tile_frame.p, h_tf, sizeof(uint32_t) * ntiles);
        st.launch_parse(stream);
        JSP_HIP(hipGetLastError());
        JSP_HIP(hipMemcpyAsync(st.h_info.p, st.d_info.p, sizeof(Msv1FrameInfo) * nf, hipMemcpyDeviceToHost, stream));
        JSP_HIP(hipStreamSynchronize(stream));   // the one wait of the staging pass: counters are needed now
        plan.gpu_parse_ms = now_ms() - tu;        // uploads + parse, not separable without more waits
        plan.h_info = st.h_info.as<const Msv1FrameInfo>();
    }

    // block_changes is rebuilt on demand from the bytes of the last frame parsed on the GPU: they are kept before the host parser needs them, and
    // before the caller's memory goes away
    void keep_last_gpu_frame(const std::vector<jsp_frame_in>& frames, int last_gpu_frame) {
        if (last_gpu_frame < 0 || !block_changes_stale) return;
        const jsp_frame_in& g = frames[last_gpu_frame];
        last_full_frame.assign(g.src, g.src + g.n);
        last_full_dev = nullptr;
    }

    // What frame i's parse found: the GPU's counters where they settle the frame (then `last_gpu_frame` = i), else the host parser's, whose block
    // table goes up in place of the GPU's.
    Msv1Parse frame_parse(const std::vector<jsp_frame_in>& frames, int i, Msv1Staged& st, StagePlan& plan, int& last_gpu_frame) {
        const jsp_frame_in& f = frames[i];
        const size_t nblk = (size_t)std::max(geo.nblocks, 1);
        Msv1Parse pr;
        if (st.gpu_parse && !plan.h_pf[i].host_parsed) {
            const Msv1FrameInfo& fi = plan.h_info[i];
            const bool needs_host = fi.total_blocks < (uint32_t)geo.nblocks ||      // stream too short
                                    (fi.flags & MSV1_INFO_END_MARKER) ||             // 8-bit end marker
                                    (fi.n_skip_codes && !prev_dev);                   // the reference raises
            if (!needs_host) {
                pr.changes = fi.n_coded != 0;
                pr.s1 = pr.changes && (fi.flags & MSV1_INFO_S1);
                pr.n_coded = fi.n_coded;
                pr.n_skipped = (uint64_t)geo.nblocks - fi.n_coded;
                pr.consumed = std::min<uint64_t>(fi.consumed, f.n);
                last_gpu_frame = i;
                block_changes_stale = true;
                return pr;
            }
        }
        keep_last_gpu_frame(frames, last_gpu_frame);
        st.h_desc.reserve(sizeof(uint32_t) * nblk * std::max(st.nframes, 1));   // (on-GPU parse: allocated when the first such frame turns up)
        uint32_t* desc = st.h_desc.as<uint32_t>() + (size_t)i * nblk;
        host_parse(f.src, f.n, (uint32_t)plan.beg[i], desc, pr);
        if (pr.early_out) std::fill(desc, desc + geo.nblocks, MSV1_DESC_UNTOUCHED);
        if (st.gpu_parse) {  // this frame's table comes from the host from now on
            ++host_parsed_frames;
            plan.h_pf[i].host_parsed = 1;
            plan.pframes_dirty = true;
            upload(st.d_desc.as<uint32_t>() + (size_t)i * nblk, desc, sizeof(uint32_t) * geo.nblocks);
        }
        return pr;
    }

    // ---- phase 4: per-frame protocol decisions, in stream order ----
    void decide_frames(const std::vector<jsp_frame_in>& frames, Msv1Staged& st, StagePlan& plan) {
        const int nf = (int)frames.size();
        const size_t nblk = (size_t)std::max(geo.nblocks, 1);
        auto* h_frames = st.h_frames.as<Msv1FrameArgs>();
        auto* d_signif = st.d_signif.as<uint32_t>();
        plan.vec_ok = (X & 3) == 0;
        plan.attr.assign(nf, StagePlan::Attr{false, false, false, false});
        plan.frame_stream.assign(nf, 0);
        int last_gpu_frame = -1;
        for (int i = 0; i < nf; ++i) {
            const jsp_frame_in& f = frames[i];
            const Msv1Parse pr = frame_parse(frames, i, st, plan, last_gpu_frame);
            Msv1FrameArgs& fa = h_frames[i];
            fa.dst = f.dst;
            fa.prev = prev_dev;
            fa.signif = d_signif + i;
            fa.stream_end = (uint32_t)(plan.beg[i] + f.n);
            fa.desc_base = (uint32_t)((size_t)i * nblk);
            fa.cmp_row_lo = 0xFFFFFFFFu;
            fa.pad = 0;
            if ((reinterpret_cast<uintptr_t>(f.dst) & 15) || (reinterpret_cast<uintptr_t>(prev_dev) & 15))
                plan.vec_ok = false;
            bool dependent = pr.n_skipped != 0;  // reads its predecessor
            if (pr.early_out) {
                // nothing to paint: every block untouched, the frame rides along as a no-op
            } else if (pr.aborted) {
                st.status[i] = JSP_ERROR_OCCURED;  // the reference raises out of DecompressP here
                st.why = "skip code before any frame was decoded: the reference raises here";
            } else {
                const int sg = msv1_significance(pr.s1, prev_dev != nullptr, f.key, geo.bits == 16 && insign_lines_set);
                if (sg < 0) {   // stage 2 on the GPU; result lands in the frame's signif word
                    fa.cmp_row_lo = (uint32_t)std::max(insign_lines, 0);
                    dependent = true;
                }
                st.significant[i] = sg;
                if (pr.changes) st.adopted[i] = 1;
            }
            if (dependent && prev_dev) fa.pad |= MSV1_FRAME_USES_PREV;
            st.info.units_coded += pr.n_coded;
            st.info.units_copied += pr.n_skipped;
            st.info.stream_bytes += pr.consumed;
            plan.frame_stream[i] = pr.consumed;

            plan.attr[i].dependent = dependent;
            plan.attr[i].noop = pr.early_out;
            plan.attr[i].special = pr.aborted || (pr.n_untouched > 0 && !pr.early_out);
            plan.attr[i].edge = fa.cmp_row_lo != 0xFFFFFFFFu && ((X & 3) || (Y & 3));
            if (pr.early_out) fa.pad |= MSV1_FRAME_NOOP;
            if (st.adopted[i]) prev_dev = f.dst;
        }
        keep_last_gpu_frame(frames, last_gpu_frame);
        st.vec_ok = plan.vec_ok;
    }

    // ---- phase 8: what the launches still need, queued behind whatever is on the stream; jsp_staged_decode queues behind them in turn ----
    // (The pinned staging buffers belong to the staged batch and outlive the copies.)
    void final_uploads(Msv1Staged& st, StagePlan& plan) {
        const int nf = st.nframes;
        if (!nf) return;
        const double tu = now_ms();
        if (!st.gpu_parse) {
            upload(st.d_stream.p, st.h_stream.p, plan.total_stream);
            upload(st.d_desc.p, st.h_desc.p, sizeof(uint32_t) * (size_t)std::max(geo.nblocks, 1) * nf);
        } else if (plan.pframes_dirty) {
            upload(st.d_pframes.p, plan.h_pf, sizeof(Msv1ParseFrame) * nf);
        }
        upload(st.d_frames.p, st.h_frames.p, sizeof(Msv1FrameArgs) * nf);
        if (nf > 1) {   // batches: report the upload time; single frames skip the wait
            JSP_HIP(hipStreamSynchronize(stream));
            plan.h2d_ms += now_ms() - tu;
        }
    }
};

}  // namespace

bool msv1_seek_view(jsp_staged* base, Msv1SeekView& out) {
    auto* st = dynamic_cast<Msv1Staged*>(base);
    if (!st) return false;
    out.geo = st->geo;
    out.d_stream = st->d_stream.as<const uint8_t>();
    out.d_desc = st->d_desc.as<const uint32_t>();
    out.desc_pitch = (size_t)std::max(st->geo.nblocks, 1);
    out.d_frames = st->d_frames.as<const Msv1FrameArgs>();
    out.h_frames = st->h_frames.as<const Msv1FrameArgs>();
    out.d_palette = st->d_palette;
    out.d_signif = st->d_signif.as<uint32_t>();
    out.h_signif = st->h_signif.as<uint32_t>();
    out.nframes = st->nframes;
    return true;
}

bool msv1_save_state(jsp_codec* base, Msv1HostState& out) {
    auto* c = dynamic_cast<Msv1Codec*>(base);
    if (!c) return false;
    out.prev_dev = c->prev_dev;
    out.block_changes = c->block_changes;
    out.block_changes_stale = c->block_changes_stale;
    out.last_full_frame = c->last_full_frame;
    out.last_full_dev = c->last_full_dev;
    out.last_full_dev_bytes = c->last_full_dev_bytes;
    return true;
}

void msv1_restore_state(jsp_codec* base, const Msv1HostState& s) {
    auto* c = dynamic_cast<Msv1Codec*>(base);
    if (!c) return;
    c->prev_dev = s.prev_dev;
    c->block_changes = s.block_changes;
    c->block_changes_stale = s.block_changes_stale;
    c->last_full_frame = s.last_full_frame;
    c->last_full_dev = s.last_full_dev;
    c->last_full_dev_bytes = s.last_full_dev_bytes;
}

bool msv1_block_changes_now(jsp_codec* base, std::vector<uint8_t>& out) {
    auto* c = dynamic_cast<Msv1Codec*>(base);
    if (!c) return false;
    out = c->block_changes;
    if (!c->block_changes_stale) return true;
    std::vector<uint8_t> bytes;   // as host_parse rebuilds them, on a copy
    if (c->last_full_dev) {
        JSP_HIP(hipStreamSynchronize(c->stream));
        bytes.resize(c->last_full_dev_bytes);
        if (!bytes.empty()) JSP_HIP(hipMemcpy(bytes.data(), c->last_full_dev, bytes.size(), hipMemcpyDeviceToHost));
    }
    const std::vector<uint8_t>& src = c->last_full_dev ? bytes : c->last_full_frame;
    std::vector<uint32_t> scratch((size_t)std::max(c->geo.nblocks, 1));
    Msv1Parse tmp;
    msv1_parse(c->geo, src.data(), src.size(), true, 0, c->insignificant_blocks, 0, scratch.data(), out, tmp);
    return true;
}

bool msv1_take_batch(jsp_staged* base, DeviceBuffer& stream, DeviceBuffer& desc, DeviceBuffer& frames) {
    auto* st = dynamic_cast<Msv1Staged*>(base);
    if (!st) return false;
    auto take = [](DeviceBuffer& to, DeviceBuffer& from) {
        to.release();
        std::swap(to.p, from.p);
        std::swap(to.cap, from.cap);
    };
    take(stream, st->d_stream);
    take(desc, st->d_desc);
    take(frames, st->d_frames);
    return true;
}

}  // namespace jsp

jsp_codec* jsp_make_msv1(int bits, int w, int h, const uint8_t* palette, int palette_bytes) {
    return new jsp::Msv1Codec(bits, w, h, palette, palette_bytes);
}
