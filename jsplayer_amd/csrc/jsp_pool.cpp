// The frame pool of the C ABI (jsp_pool_*, include/jsplayer_amd.h): where the destination frames of a batch lie in device memory.
//
// A pool large enough for batches (the staged-batch calls write tile j of EVERY frame at about the same time: as many write fronts as frames) is
// PLACED: the same store shape gets 5.4 - 7.0 TB/s from one set of allocations or another of the same process, persistently — a property of where
// the frames lie in physical memory, relative to each other, that no query reveals (tools/front_lab.hip).  So the pool measures
// what it was given, candidate by candidate (a few milliseconds each), against what a plain fill takes from the same device:
//   1. the mapped forms (search_mapped): one address range over physical allocations of the pool's own making;
//   2. only when no mapped form can be made, or on request (JSP_POOL_PROBE_THOROUGH=1) when none came within 3 % of the fill, the hipMalloc forms:
//      the form that won the last probe of this process, a run of chunks (search_chunks), the round of older forms (search_older).
// What the probe may hold while it chooses is bounded: JSP_POOL_PROBE_MAX candidates and a quarter of the free device memory (ProbeOptions below) — a
// caller with 8 such pools to make must not find the seventh refused because the sixth was still holding 68 GB of rejects.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdarg>
#include <cstdlib>
#include <numeric>

#include "codec.h"

namespace jsp {
double pool_store_rate(uint32_t* const* d_frames, int nframes, int X, int Y, uint32_t fill);
double pool_fill_rate(uint32_t* slab, size_t nbytes);
}  // namespace jsp

namespace {

// Device memory put together by hand: one address range, backed by physical allocations (hipMemCreate) mapped into it.  What hipMalloc gives for
// a multi-gigabyte request and what it gives for a run of smaller ones differ, board by board, in what the decode kernels' store shapes get from them
// (5.6 - 7.0 TB/s); memory made this way took 6.8 - 7.0 TB/s from all three shapes in every arrangement on every board it was tried on
// (profiles/r06_vmm_pool_board*.txt), holds exactly the pool and is set up in under a millisecond.  Move-only: the range goes back when its owner does.
struct MappedRange {
    void* va = nullptr;
    size_t bytes = 0, handle_bytes = 0, mapped = 0;      // (mapped: how many of `handles` are mapped, in order from the range's start)
    std::vector<hipMemGenericAllocationHandle_t> handles;
    MappedRange() = default;
    MappedRange(MappedRange&& o) noexcept { *this = std::move(o); }
    MappedRange& operator=(MappedRange&& o) noexcept {
        if (this != &o) { release(); std::swap(va, o.va); std::swap(bytes, o.bytes); std::swap(handle_bytes, o.handle_bytes); std::swap(mapped, o.mapped); handles.swap(o.handles); }
        return *this;
    }
    ~MappedRange() { release(); }
    bool empty() const { return va == nullptr; }
    void release() {
        if (va) {
            for (size_t h = 0; h < mapped; ++h) (void)hipMemUnmap(static_cast<char*>(va) + h * handle_bytes, handle_bytes);   // piece by piece: a range only partly mapped (a failed make) unmaps what it has
            for (auto h : handles) (void)hipMemRelease(h);
            (void)hipMemAddressFree(va, bytes);
            (void)hipGetLastError();
        }
        va = nullptr; bytes = handle_bytes = mapped = 0; handles.clear();
    }
    // `nbuf` frames of `frame_bytes`, `per` to a physical allocation; `dealt`: frame i and i + 1 never share one (frame i lies in allocation i mod n),
    // else the frames lie in order.  False (and nothing held) when the device or the runtime does not do this.
    bool make(int device, size_t frame_bytes, int nbuf, std::vector<int32_t*>& frames, int per, bool dealt) {
        hipMemAllocationProp prop{};
        prop.type = hipMemAllocationTypePinned;
        prop.location.type = hipMemLocationTypeDevice;
        prop.location.id = device;
        size_t gran = 0;
        if (hipMemGetAllocationGranularity(&gran, &prop, hipMemAllocationGranularityMinimum) != hipSuccess || gran == 0) { (void)hipGetLastError(); return false; }
        const int kPer = per < 1 ? 1 : per;
        const size_t align = std::max<size_t>(gran, (size_t)2 << 20);
        const size_t stride = (frame_bytes + gran - 1) / gran * gran;
        handle_bytes = (stride * kPer + align - 1) / align * align;
        const size_t nh = ((size_t)nbuf + kPer - 1) / kPer;
        bytes = nh * handle_bytes;
        if (hipMemAddressReserve(&va, bytes, align, nullptr, 0) != hipSuccess) { (void)hipGetLastError(); va = nullptr; bytes = handle_bytes = 0; return false; }
        bool ok = true;
        for (size_t h = 0; h < nh && ok; ++h) {
            hipMemGenericAllocationHandle_t handle;
            ok = hipMemCreate(&handle, handle_bytes, &prop, 0) == hipSuccess;
            if (ok) {
                handles.push_back(handle);
                ok = hipMemMap(static_cast<char*>(va) + h * handle_bytes, handle_bytes, 0, handle, 0) == hipSuccess;
                if (ok) ++mapped;
            }
        }
        hipMemAccessDesc acc{};
        acc.location = prop.location;
        acc.flags = hipMemAccessFlagsProtReadWrite;
        ok = ok && hipMemSetAccess(va, bytes, &acc, 1) == hipSuccess;
        // (the rest of the library — and the caller's torch — must see these addresses as device memory)
        hipPointerAttribute_t at{};
        ok = ok && hipPointerGetAttributes(&at, va) == hipSuccess && at.type == hipMemoryTypeDevice;
        if (!ok) {
            (void)hipGetLastError();
            release();
            return false;
        }
        frames.clear();
        for (int i = 0; i < nbuf; ++i) {
            const size_t h = dealt ? (size_t)i % nh : (size_t)i / (size_t)kPer, slot = dealt ? (size_t)i / nh : (size_t)i % (size_t)kPer;
            frames.push_back(reinterpret_cast<int32_t*>(static_cast<char*>(va) + h * handle_bytes + slot * stride));
        }
        return true;
    }
};

// Frames and the memory under them: hipMalloc'ed allocations, or one mapped range.  Move-only; what it owns goes back to the device with it.
struct Candidate {
    std::vector<void*> allocs;
    MappedRange mapped;
    std::vector<int32_t*> frames;
    double rate = 0;               // GB/s it took from the probe
    int form = -1;                 // 0 .. 2: the older forms (make_older); -1: chunked or mapped
    Candidate() = default;
    Candidate(Candidate&&) noexcept = default;
    Candidate& operator=(Candidate&& o) noexcept {
        if (this != &o) { release(); allocs.swap(o.allocs); mapped = std::move(o.mapped); frames.swap(o.frames); o.frames.clear(); rate = o.rate; form = o.form; }   // (release() left `allocs` empty: so is the source's now)
        return *this;
    }
    ~Candidate() { release(); }
    void release() {
        for (void* d : allocs) (void)hipFree(d);
        allocs.clear();
        mapped.release();
    }
};

}  // namespace

struct jsp_pool {
    int device = 0;
    Candidate placed;              // the frames (jsp_pool_buffer) and their memory; placed.rate: GB/s the pool took from the probe (0: not probed)
    std::vector<double> tried;     // what each candidate the probe measured took
    double probe_ms = 0;           // wall time of the placement probe (allocations, launches, releases)
    uint64_t held_peak = 0;        // most device memory the probe held at one time, candidates kept while asking for the next
    uint64_t hold_limit = 0;       // ... and what it was allowed to hold
};

namespace {

// Which of the older forms won the last probe of this process (-1: a chunked or mapped candidate, or nothing yet): boards differ in which form their memory likes,
// a board does not change its mind between two pools — the next pool tries that form first instead of finding it again behind seven others.
// (Per device: a process that shards streams over several GPUs, jsp_shard.cpp, has as many boards as devices.)
constexpr int kHintDevices = 64;
std::atomic<int> g_pool_form_hint[kHintDevices];
struct HintInit { HintInit() { for (auto& h : g_pool_form_hint) h.store(-1); } } g_hint_init;
std::atomic<int>* pool_form_hint(int device) { return &g_pool_form_hint[device >= 0 && device < kHintDevices ? device : 0]; }

// The environment, read once per jsp_pool_create (callers change it between pools).
struct ProbeOptions {
    static const char* env(const char* name, const char* unset) { const char* v = std::getenv(name); return v ? v : unset; }
    bool probe = std::atoi(env("JSP_POOL_PROBE", "1")) != 0;                   // =0: no probe, one allocation per frame, first come
    int max_candidates = std::max(1, std::min(64, std::atoi(env("JSP_POOL_PROBE_MAX", "16"))));   // candidates measured at most
    double hold_gb = std::atof(env("JSP_POOL_PROBE_HOLD_GB", "-1"));           // what the probe may hold, when that is less than a quarter of the free device memory (unset: that quarter)
    bool mapped = std::atoi(env("JSP_POOL_PROBE_MAPPED", "1")) != 0;           // =0: skip the mapped forms (lab)
    bool thorough = std::atoi(env("JSP_POOL_PROBE_THOROUGH", "0")) != 0;       // =1: the hipMalloc forms too, unless a mapped form came within 3 % of the fill
    double budget_ms = std::max(0.0, std::atof(env("JSP_POOL_PROBE_MS", "250")));   // no further mapped candidate of the second phase once the probe has taken this long
    int form = std::atoi(env("JSP_POOL_PROBE_FORM", "-1"));                    // 0 | 1 | 2: the older form to start with, whatever the process remembers
    bool log = std::getenv("JSP_POOL_PROBE_LOG") != nullptr;                   // a line per candidate on stderr
};

// One probe: the pool's shape, what was measured so far and everything held meanwhile.  (The members' order is the order of release when a
// measurement throws: the candidates, the chunk run, the table last.)
struct Probe {
    const ProbeOptions opt;
    jsp_pool* const p;
    const int device, width, height, nbuf;
    const size_t bytes;                                  // of a frame
    const uint64_t one;                                  // ... and of the pool
    const std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    double yardstick = 0;                                // GB/s of a plain fill: what the candidates are held against
    Candidate table;                                     // the frame table the probe kernel reads, on the device
    Candidate run;                                       // the run of chunk allocations behind the chunked candidates (search_chunks)
    std::vector<Candidate> cands;                        // what is held to choose from
    int best = -1, chunked = -1;                         // among `cands`: the best so far, the chunked candidate

    Probe(const ProbeOptions& o, jsp_pool* pool, int dev, int w, int h, int n)
        : opt(o), p(pool), device(dev), width(w), height(h), nbuf(n), bytes((size_t)w * h * sizeof(int32_t)), one((uint64_t)bytes * (uint64_t)n) {
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) { (void)hipGetLastError(); free_b = 0; }
        uint64_t limit = free_b ? (uint64_t)free_b / 4 : ~0ull;
        if (opt.hold_gb >= 0) limit = std::min(limit, (uint64_t)(opt.hold_gb * 1e9));
        p->hold_limit = std::max(limit, one);            // (the pool itself is always allowed)
        void* d = nullptr;
        JSP_HIP(hipMalloc(&d, sizeof(uint32_t*) * (size_t)nbuf));
        table.allocs.push_back(d);
    }
    double spent_ms() const { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); }
    int tried() const { return (int)p->tried.size(); }
    bool may_try() const { return tried() < opt.max_candidates; }
    bool within(double share, double rate) const { return yardstick > 0 && rate >= share * yardstick; }
    void holding(uint64_t held) { p->held_peak = std::max(p->held_peak, held); }
    double measure(const std::vector<int32_t*>& frames) {
        uint32_t** d_table = static_cast<uint32_t**>(table.allocs[0]);
        JSP_HIP(hipMemcpy(d_table, frames.data(), sizeof(uint32_t*) * (size_t)nbuf, hipMemcpyHostToDevice));
        const double rate = jsp::pool_store_rate(d_table, nbuf, width, height, 0u);
        p->tried.push_back(rate);
        return rate;
    }
    __attribute__((format(printf, 4, 5))) void log(int index, double rate, const char* fmt, ...) const {
        if (!opt.log) return;
        char what[256];
        va_list ap;
        va_start(ap, fmt);
        std::vsnprintf(what, sizeof what, fmt, ap);
        va_end(ap);
        std::fprintf(stderr, "[jsp_pool] candidate %d (%s): %.0f GB/s (plain fill %.0f)\n", index, what, rate, yardstick);
    }
    // the yardstick when no mapped form can be made (else it is measured on the first mapped candidate's own memory: a 2 GB slab costs a quarter
    // of a second in hipMalloc alone on most boards)
    void slab_yardstick() {
        void* slab = nullptr;
        const size_t slab_bytes = (size_t)std::min<uint64_t>(one, 2ull << 30);
        if (hipMalloc(&slab, slab_bytes) == hipSuccess) {
            yardstick = jsp::pool_fill_rate(static_cast<uint32_t*>(slab), slab_bytes);
            (void)hipFree(slab);
        } else (void)hipGetLastError();
    }
};

// The mapped forms (MappedRange), in up to three arrangements: an allocation per frame; sixteen frames per physical allocation and the frames dealt
// over them; sixteen per allocation, frames in order (the order: on the one board of five where the three differed, an allocation per frame took
// 7.2 TB/s and sixteen per allocation 6.3 - 6.5, profiles/r06_j_bench_default.json).  Each holds the pool and nothing else, costs a few milliseconds
// to set up and one probe launch.  Phase one: the three arrangements, the best so far held while the next is measured.  Phase two, while none has
// come within 3 % of the plain fill: up to six more candidates of the first arrangement, each made while the ones before it are still held —
// different physical memory every time.  What a pool gets from its memory is a property of WHERE that memory lies that lasts as long as the
// allocation does (profiles/r06_time_lab_memory.txt) — unless the whole board is in its slow state (r06_time_lab_slow_state.txt: everything
// 5.4 - 5.8, kept or fresh).  So the best of up to nine is worth ~10 ms apiece and a transient hold of up to nine pools within the hold limit, and
// within the time budget: a physical allocation is usually made in microseconds, but right after gigabytes have been given back the driver can take
// half a second over the next ones (profiles/r06_w_pool_probe_log.txt).  The best is kept even when none is good: the hipMalloc forms cost half a
// second and a pool's worth of memory EACH to try and were not better on such boards (profiles/r06_h_bench_default_slow_board.json,
// r06_y_bench_default_final_slow_state_board.json).  Returns the best; one without a mapped range: no mapped form could be made.
Candidate search_mapped(Probe& pr) {
    struct Form { int per; bool dealt; const char* what; };
    static const Form forms[] = {{1, true, "a physical allocation per frame"}, {16, true, "16 frames per physical allocation, frames dealt"}, {16, false, "16 frames per physical allocation, frames in order"}};
    std::vector<Candidate> rejects;                      // kept allocated until the search ends: the next candidate is then made of OTHER memory
    uint64_t rejects_bytes = 0;
    Candidate held;                                      // the best so far
    for (int k = 0; k < 9 && pr.may_try() && (k < 3 || pr.spent_ms() < pr.opt.budget_ms); ++k) {
        const bool second_phase = k >= 3;
        if (second_phase && !(pr.yardstick > 0 && held.rate < 0.97 * pr.yardstick)) break;   // a fill that measured nothing (yardstick 0): no second phase.  (A candidate within 3 % has ended the loop below.)
        if (!held.mapped.empty() && (uint64_t)held.mapped.bytes + rejects_bytes + pr.one > pr.p->hold_limit) break;   // (the best so far stays held while the next is measured)
        const Form& form = forms[second_phase ? 0 : k];
        // (frames far smaller than the 2 MB a physical allocation is rounded up to share one: "an allocation per frame" is an allocation per 2 MB of frames)
        const int per = form.per == 1 ? (int)std::max<size_t>(1, ((size_t)2 << 20) / std::max<size_t>(pr.bytes, 1)) : form.per;
        Candidate c;
        if (!c.mapped.make(pr.device, pr.bytes, pr.nbuf, c.frames, per, form.dealt)) break;
        if (pr.yardstick <= 0) pr.yardstick = jsp::pool_fill_rate(static_cast<uint32_t*>(c.mapped.va), (size_t)std::min<uint64_t>((uint64_t)c.mapped.bytes, 2ull << 30));
        c.rate = pr.measure(c.frames);
        pr.log(pr.tried() - 1, c.rate, "one address range over %zu physical allocations: %s%s", c.mapped.handles.size(), form.what, second_phase ? ", other memory" : "");
        pr.holding((uint64_t)c.mapped.bytes + (uint64_t)held.mapped.bytes + rejects_bytes);
        const bool good = pr.within(0.97, c.rate);
        if (c.rate > held.rate) std::swap(c, held);   // c: the loser from here on
        if (good) { c.release(); break; }
        if (!c.mapped.empty()) {
            rejects_bytes += c.mapped.bytes;
            rejects.push_back(std::move(c));
        }
    }
    for (auto& r : rejects) r.release();
    return held;
}

// The older forms, made with hipMalloc: 0 two frames per allocation, 1 all frames in one allocation, 2 an allocation per frame; the frames
// taken in a strided order.  False (nothing held, nothing measured): the device memory ran out.
bool make_older(Probe& pr, int form, Candidate& c) {
    const int per = form == 1 ? pr.nbuf : form == 0 ? 2 : 1;
    for (int i = 0; i < pr.nbuf; i += per) {
        void* d = nullptr;
        const int k = std::min(per, pr.nbuf - i);
        if (hipMalloc(&d, pr.bytes * (size_t)k) != hipSuccess) { (void)hipGetLastError(); c.release(); c.frames.clear(); return false; }
        c.allocs.push_back(d);
        for (int q = 0; q < k; ++q) c.frames.push_back(static_cast<int32_t*>(d) + (size_t)q * pr.width * pr.height);
    }
    // consecutive frames must not be neighbours in memory (search_chunks): frame i takes slot (i x K) mod n, K coprime to n
    int K = 1;
    for (int cand : {17, 19, 23, 29, 31, 37, 41, 43})
        if (cand < pr.nbuf && std::gcd(cand, pr.nbuf) == 1) { K = cand; break; }
    if (K > 1) {
        std::vector<int32_t*> in_order(c.frames.size());
        for (int i = 0; i < pr.nbuf; ++i) in_order[i] = c.frames[(size_t)((long long)i * K % pr.nbuf)];
        c.frames.swap(in_order);
    }
    c.rate = pr.measure(c.frames);
    c.form = form;
    pr.log(pr.tried() - 1, c.rate, "%s", form == 1 ? "one allocation" : form == 0 ? "two frames per allocation" : "one allocation per frame");
    return true;
}

// Which chunks of a run of `total` the k-th chunked candidate takes, `nch` of them.  "Every fourth" is not always the answer: in some sessions all
// four such candidates are slow (5.7 - 6.4 TB/s) while a form made of many small allocations is fast (profiles/r05_q_bench_all.jsonl:
// candidates_GBs) — the run's chunks do not always lie in memory in the order they were asked for.  So the candidates differ in kind: every
// fourth from the first, a pseudo-random choice, every third from the second, another pseudo-random choice.
std::vector<int> pick_chunks(int k, int nch, int spread, int total) {
    std::vector<int> ids;
    if (k == 0 || (k == 2 && spread < 3)) {
        for (int ch = 0; ch < nch; ++ch) ids.push_back(ch * spread + (k ? 1 : 0));
    } else if (k == 2) {
        for (int ch = 0; ch < nch; ++ch) ids.push_back(1 + ch * 3);
    } else {                                             // a partial Fisher-Yates shuffle, seeded by the candidate
        std::vector<int> all(total);
        for (int i = 0; i < total; ++i) all[i] = i;
        uint64_t seed = 0x9E3779B97F4A7C15ull * (uint64_t)(k + 1);
        for (int i = 0; i < nch; ++i) {
            seed = seed * 6364136223846793005ull + 1442695040888963407ull;
            const int j = i + (int)((seed >> 33) % (uint64_t)(total - i));
            std::swap(all[i], all[j]);
            ids.push_back(all[i]);
        }
    }
    return ids;
}

// The chunk run (tools/front_lab.hip; profiles/r05_front_lab_chunks.txt, r05_front_lab_spread.txt, r05_front_lab_frame_order.txt).  Two things
// make a pool slow, and neither is visible to any query:
//  (1) frames lying NEXT TO each other.  Separately allocated chunks of 16 frames take 5.6 - 6.0 TB/s as neighbours and 7.0 when only every fourth
//      of them is used; kernels whose workgroups WALK the frames are hit hardest: the same 512 slots of one allocation give their store shapes
//      5.0 / 5.9 TB/s when frame i lies in slot i and 6.3 / 6.9 when it lies in slot 17 i mod 512 — consecutive frames must not be neighbours;
//  (2) stretches of memory that are slow whatever the arrangement (5.7 against 7.0, the first 4 GB a process gets in one session).
// So: four times the chunks the pool needs (fewer when the hold limit says so), allocated in one run; a candidate takes a quarter of them
// (pick_chunks), its frames DEALT round-robin over its chunks (frame i and frame i + 1 in different chunks); up to four are measured, the first
// that comes within 1.5 % of a plain fill ends it; the best is returned, a candidate like any other, and the other chunks are given back.
// Returns a candidate without frames when the run cannot be made or held, or nothing may be measured any more.
Candidate search_chunks(Probe& pr) {
    const int kChunkFrames = 16;
    const int nch = (pr.nbuf + kChunkFrames - 1) / kChunkFrames;
    // (what a run of s x the pool really holds: whole chunks, so up to 15 frames more per s than s pools)
    auto run_bytes = [&](int s) { return (uint64_t)nch * (uint64_t)s * (uint64_t)kChunkFrames * (uint64_t)pr.bytes; };
    int spread = 4;
    while (spread > 1 && run_bytes(spread) + (uint64_t)pr.cands.size() * pr.one > pr.p->hold_limit) --spread;
    Candidate c;
    if (spread == 1) return c;
    std::vector<void*>& run = pr.run.allocs;
    for (int q = 0; q < nch * spread; ++q) {
        void* d = nullptr;
        if (hipMalloc(&d, pr.bytes * (size_t)kChunkFrames) != hipSuccess) { (void)hipGetLastError(); pr.run.release(); return c; }   // (whole chunks all: any chunk of the run can stand for any chunk of the pool)
        run.push_back(d);
    }
    pr.holding(run_bytes(spread) + (uint64_t)pr.cands.size() * pr.one);
    auto deal = [&](const std::vector<int>& ids) {        // the candidate's frames, dealt round-robin over its chunks
        std::vector<int32_t*> dealt;
        for (int slot = 0; slot < kChunkFrames; ++slot)
            for (int ch = 0; ch < nch; ++ch)
                if (slot < std::min(kChunkFrames, pr.nbuf - ch * kChunkFrames)) dealt.push_back(static_cast<int32_t*>(run[(size_t)ids[(size_t)ch]]) + (size_t)slot * pr.width * pr.height);
        return dealt;
    };
    int best_k = -1;
    for (int k = 0; k < 4 && pr.may_try(); ++k) {
        const double rate = pr.measure(deal(pick_chunks(k, nch, spread, (int)run.size())));
        pr.log(k, rate, "chunks of 16 frames out of a run of %d x the pool: %s; frames dealt over them", spread, k == 0 ? "every fourth" : k == 2 ? "every third" : "a pseudo-random choice");
        if (rate > c.rate) { c.rate = rate; best_k = k; }
        if (pr.within(0.985, rate)) break;
    }
    if (best_k < 0) { pr.run.release(); return c; }         // none was measured (JSP_POOL_PROBE_MAX used up by the hinted form): the run goes back whole
    const std::vector<int> ids = pick_chunks(best_k, nch, spread, (int)run.size());
    c.frames = deal(ids);
    std::vector<char> kept(run.size(), 0);
    for (int id : ids) kept[(size_t)id] = 1;
    for (size_t q = 0; q < run.size(); ++q) {
        if (kept[q]) c.allocs.push_back(run[q]);
        else (void)hipFree(run[q]);
    }
    run.clear();
    return c;
}

// The round of older forms, each candidate held while the next is made (else the allocator hands the same pages back), until one takes what a
// plain fill takes, the candidates or the hold limit are used up, or the memory is.  `hint`: the form that has had its try already (-1: none).
void search_older(Probe& pr, int hint) {
    for (int a = 0; pr.may_try(); ++a) {
        if (pr.best >= 0 && (uint64_t)(pr.cands.size() + 1) * pr.one > pr.p->hold_limit) break;   // holding another candidate would pass the limit
        Candidate c;
        if (!make_older(pr, (a + (hint >= 0 ? hint + 1 : 0)) % 3, c)) {   // the memory ran out while candidates were being held: the best so far it is
            if (pr.best >= 0) break;
            throw std::runtime_error("out of device memory for the frame pool");
        }
        pr.cands.push_back(std::move(c));
        pr.holding((uint64_t)pr.cands.size() * pr.one);
        if (pr.best < 0 || pr.cands.back().rate > pr.cands[pr.best].rate * (pr.best == pr.chunked ? 1.03 : 1.0)) pr.best = (int)pr.cands.size() - 1;
        if (pr.within(0.985, pr.cands[pr.best].rate)) break;   // as good as it gets (the fast kind takes what a plain fill takes)
    }
}

// The searches in their order; leaves the winner in p->placed.
void place(Probe& pr) {
    Candidate first = pr.opt.mapped ? search_mapped(pr) : Candidate();
    const bool mapped = !first.mapped.empty();
    if (mapped) { pr.cands.push_back(std::move(first)); pr.best = 0; }
    else pr.slab_yardstick();                            // (the hipMalloc forms are held against a slab's fill)
    // With a mapped candidate the search ends here, unless the hipMalloc forms are asked for and that candidate is not within 3 % of the plain fill.
    // (An earlier version tried one run of hipMalloc chunks whenever nine mapped candidates stayed a tenth under the fill: on boards in their slow state
    // — the only ones where that happens — it cost 0.4 - 1 s per pool and never found anything.)
    bool settled = mapped && (!pr.opt.thorough || pr.within(0.97, pr.cands[0].rate));
    const int hint = pr.opt.form >= 0 && pr.opt.form < 3 ? pr.opt.form : pool_form_hint(pr.device)->load();
    if (!settled && hint >= 0 && hint < 3) {             // the form this board liked last time, next
        Candidate c;
        if (make_older(pr, hint, c)) {
            pr.cands.push_back(std::move(c));
            pr.holding((uint64_t)pr.cands.size() * pr.one);
            if (pr.best < 0 || pr.cands.back().rate > pr.cands[pr.best].rate) pr.best = (int)pr.cands.size() - 1;
            settled = pr.within(0.985, pr.cands[pr.best].rate);
        }
    }
    Candidate chunks = settled ? Candidate() : search_chunks(pr);
    if (!chunks.frames.empty()) {
        pr.cands.push_back(std::move(chunks));
        pr.chunked = (int)pr.cands.size() - 1;
        // (an older form — its frames lie densely — must beat the chunked candidate by 3 % to stand before it: the probe's shape does not mind density,
        // the key-frame kernel's does, profiles/r05_front_lab_frame_order.txt.  Against a mapped candidate the better probe wins, no allowance.)
        if (pr.best < 0 || pr.cands[pr.chunked].rate * (pr.cands[pr.best].mapped.empty() ? 1.03 : 1.0) > pr.cands[pr.best].rate) pr.best = pr.chunked;
    }
    const bool good_enough = settled || (pr.chunked >= 0 && pr.best == pr.chunked && (pr.yardstick <= 0 || pr.cands[pr.chunked].rate >= 0.95 * pr.yardstick));
    if (!good_enough) search_older(pr, hint);
    if (pr.best >= 0) pool_form_hint(pr.device)->store(pr.cands[pr.best].form);
    pr.table.release();
    if (pr.best < 0) throw std::runtime_error("out of device memory for the frame pool");   // (no candidate could be made at all)
    for (int i = 0; i < (int)pr.cands.size(); ++i) if (i != pr.best) pr.cands[i].release();
    pr.p->placed = std::move(pr.cands[pr.best]);
}

}  // namespace

jsp_pool* jsp_pool_create(int device_id, int width, int height, int nbuf) {
    try {
        if (width <= 0 || height <= 0 || nbuf <= 0) throw std::runtime_error("bad pool shape");
        int count = 0;
        JSP_HIP(hipGetDeviceCount(&count));
        if (device_id < 0 || device_id >= count) throw std::runtime_error("device_id out of range");
        JSP_HIP(hipSetDevice(device_id));
        auto p = std::make_unique<jsp_pool>();
        p->device = device_id;
        const size_t bytes = (size_t)width * height * sizeof(int32_t);
        const ProbeOptions opt;
        constexpr int kProbeFrom = 32;                   // smaller pools (a player's num_buffers + 1) are not written by batches
        const bool probe = opt.probe && nbuf >= kProbeFrom && (width & 3) == 0 && (height & 3) == 0 &&
                           (size_t)nbuf * (size_t)((width / 4) * (height / 4) + 8191) / 8192 * 256 < (1ull << 32);   // (the probe: one launch, fewer than 2^32 lanes)
        if (!probe) {                                    // one allocation per frame, first come
            for (int i = 0; i < nbuf; ++i) {
                void* d = nullptr;
                JSP_HIP(hipMalloc(&d, bytes));
                p->placed.allocs.push_back(d);
                p->placed.frames.push_back(static_cast<int32_t*>(d));
                JSP_HIP(hipMemset(d, 0, bytes));
            }
            return p.release();
        }
        Probe pr(opt, p.get(), device_id, width, height, nbuf);
        place(pr);
        MappedRange& range = p->placed.mapped;
        if (!range.empty()) JSP_HIP(hipMemset(range.va, 0, range.bytes));   // (one call for the whole range: a memset per frame is a fifth of a millisecond each)
        else for (int32_t* f : p->placed.frames) JSP_HIP(hipMemset(f, 0, bytes));
        p->probe_ms = pr.spent_ms();
        return p.release();
    } catch (const std::exception& e) {
        jsp::set_error("%s", e.what());
        return nullptr;
    }
}
int32_t* jsp_pool_buffer(jsp_pool* p, int i) {
    return (p && i >= 0 && i < (int)p->placed.frames.size()) ? p->placed.frames[i] : nullptr;
}
int jsp_pool_count(jsp_pool* p) { return p ? (int)p->placed.frames.size() : 0; }
void jsp_pool_destroy(jsp_pool* p) {
    if (!p) return;
    (void)hipSetDevice(p->device);
    delete p;
}
double jsp_pool_store_rate(jsp_pool* p, int* attempts) {
    if (attempts) *attempts = p ? (int)p->tried.size() : 0;
    return p ? p->placed.rate : 0.0;
}
int jsp_pool_probe_info(jsp_pool* p, double* probe_ms, uint64_t* held_peak_bytes, uint64_t* hold_limit_bytes) {
    if (!p) return -1;
    if (probe_ms) *probe_ms = p->probe_ms;
    if (held_peak_bytes) *held_peak_bytes = p->held_peak;
    if (hold_limit_bytes) *hold_limit_bytes = p->hold_limit;
    return 0;
}
int jsp_pool_probe_rates(jsp_pool* p, double* rates, int cap) {
    if (!p) return -1;
    for (int i = 0; rates && i < cap && i < (int)p->tried.size(); ++i) rates[i] = p->tried[(size_t)i];
    return (int)p->tried.size();
}
