// TEST INFRASTRUCTURE: a characterisation trace of the frame pool's placement probe, without a GPU.  Built with the product's host layers, the stub
// HIP runtime and the kernel stubs under tests/tsan/ (tests/test_pool_probe_trace_cpu.py); calls the public C ABI only.  The two measurements the probe
// rests on are scripted here, scenario by scenario, every memory call of the stub runtime is observed, and what the probe did is printed symbolically:
// allocations by the order they were made in ("a7"), frames as allocation + byte offset, no address anywhere; long lists by their head and a digest.  tests/golden/pool_probe_trace.txt is
// this program's output, all groups one after the other, as recorded before jsp_pool_create was taken apart.
// Usage: trace [--full] <group> | trace --list        (the form that won a probe is remembered by the process: a group is an ordered run of pools in ONE process)
#include <hip/hip_runtime.h>
#include <unistd.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/jsplayer_amd.h"

namespace {
struct Live { int ordinal; size_t bytes; };
std::map<const char*, Live> g_live;              // hipMalloc'ed memory and reserved ranges, by base address
std::map<const void*, int> g_handles;            // physical allocations (hipMemCreate)
int g_next_ordinal = 0;

std::vector<double> g_rates;                     // the scenario's script: what pool_store_rate returns, call by call (the last value again when it runs out)
double g_fill = 0;
int g_rate_calls = 0, g_throw_at = 0;            // g_throw_at: pool_store_rate throws at that call (1-based; 0: never)
std::string g_rate_args;                         // what the last pool_store_rate call of this pool was given beside the frames
bool g_budget_once = false;                      // the allocation budget is lifted after its first refusal

std::string where(const void* p) {               // "a<ordinal>+<offset>"
    auto it = g_live.upper_bound(static_cast<const char*>(p));
    if (it != g_live.begin()) {
        --it;
        const size_t off = (size_t)(static_cast<const char*>(p) - it->first);
        if (off < it->second.bytes) return "a" + std::to_string(it->second.ordinal) + "+" + std::to_string(off);
    }
    return p ? "?" : "null";
}

// Lists are printed short: up to four items in full, of a longer one the first three, the count and a digest (FNV-1a) of the whole list
// (`trace --full <group>` prints every item).  The record pins the digest, so it pins every item.
bool g_full = false;
std::string listed(const std::vector<std::string>& items) {
    std::string all, head;
    for (size_t i = 0; i < items.size(); ++i) {
        all += " " + items[i];
        if (i < 3) head += " " + items[i];
    }
    if (g_full || items.size() <= 4) return all;
    uint64_t h = 1469598103934665603ull;
    for (unsigned char c : all) h = (h ^ c) * 1099511628211ull;
    char tail[64];
    std::snprintf(tail, sizeof tail, " ... (%zu, digest %016llx)", items.size(), (unsigned long long)h);
    return head + tail;
}

// Consecutive calls of one kind and size are one line: "hipMalloc x32 (12288 bytes): a5 a6 a7 ...".  A hipMemCreate and the hipMemMap of its handle are one call here.
struct Call { std::string name; size_t bytes; std::string item; };
Call g_created;                                  // a hipMemCreate whose hipMemMap may follow
bool g_created_open = false;
std::string g_run_name;
size_t g_run_bytes = 0;
std::vector<std::string> g_run;
bool g_line_open = false;                        // the calls between two measurements share a line
void flush_run() {
    if (g_run.empty()) return;
    std::printf("%s%s", g_line_open ? "; " : "  ", g_run_name.c_str());
    g_line_open = true;
    if (g_run.size() > 1) std::printf(" x%zu", g_run.size());
    if (g_run_bytes) std::printf(" (%zu bytes)", g_run_bytes);
    if (!g_run[0].empty()) std::printf(":%s", listed(g_run).c_str());
    g_run.clear();
}
void add(const Call& c) {
    if (!g_run.empty() && (c.name != g_run_name || c.bytes != g_run_bytes)) flush_run();
    g_run_name = c.name;
    g_run_bytes = c.bytes;
    g_run.push_back(c.item);
}
void flush(const char* then = "\n") {             // before anything else is printed; a measurement follows the calls before it on their line
    if (g_created_open) add(g_created);
    g_created_open = false;
    flush_run();
    std::printf("%s", g_line_open ? then : then[0] == '\n' ? "" : "  ");
    g_line_open = false;
}

void observe(const char* call, hipError_t result, const void* p, size_t bytes, const void* handle) {
    const std::string c = call;
    if (result != hipSuccess) {
        flush();
        std::printf("  %s (%zu bytes) FAILS\n", call, bytes);
        if (g_budget_once) stub_alloc_budget(~(size_t)0, -1);
        return;
    }
    if (c == "hipMemMap" && g_created_open && g_created.bytes == bytes && g_created.item == "h" + std::to_string(g_handles.at(handle))) {
        g_created_open = false;
        add({"hipMemCreate + hipMemMap", bytes, g_created.item + "@" + where(p)});
        return;
    }
    if (g_created_open) add(g_created);
    g_created_open = false;
    if (c == "hipMalloc" || c == "hipMemAddressReserve") {
        g_live[static_cast<const char*>(p)] = Live{g_next_ordinal, bytes ? bytes : 1};
        add({c, bytes, "a" + std::to_string(g_next_ordinal++)});
    } else if (c == "hipFree" || c == "hipMemAddressFree") {
        add({c, 0, where(p)});
        g_live.erase(static_cast<const char*>(p));
    } else if (c == "hipMemCreate") {
        g_handles[handle] = g_next_ordinal;
        g_created = {c, bytes, "h" + std::to_string(g_next_ordinal++)};
        g_created_open = true;
    } else if (c == "hipMemRelease") {
        add({c, 0, "h" + std::to_string(g_handles.at(handle))});
        g_handles.erase(handle);
    } else if (c == "hipMemMap") {
        add({c, bytes, "h" + std::to_string(g_handles.at(handle)) + "@" + where(p)});
    } else if (c == "hipMemGetInfo") {
        add({c, 0, ""});
    } else {                                     // hipMemUnmap, hipMemset
        add({c, bytes, where(p)});
    }
}
}  // namespace

namespace jsp {
double pool_store_rate(uint32_t* const* d_frames, int nframes, int X, int Y, uint32_t fill) {
    flush(" => ");
    ++g_rate_calls;
    std::vector<std::string> frames;
    for (int i = 0; i < nframes; ++i) frames.push_back(where(d_frames[i]));
    char args[128];                                  // (said when they change: the first time, that is)
    std::snprintf(args, sizeof args, " (table %s, %d x %d, fill %u)", where(d_frames).c_str(), X, Y, fill);
    std::printf("store rate #%d%s:%s", g_rate_calls, g_rate_args == args ? "" : args, listed(frames).c_str());
    g_rate_args = args;
    if (g_rate_calls == g_throw_at) {
        std::printf(" -> throws\n");
        throw std::runtime_error("scripted failure of the store-rate measurement");
    }
    const double r = g_rates.empty() ? 0.0 : g_rates[std::min((size_t)g_rate_calls, g_rates.size()) - 1];
    std::printf(" -> %.0f\n", r);
    return r;
}
double pool_fill_rate(uint32_t* slab, size_t nbytes) {
    flush(" => ");
    std::printf("fill rate (%s, %zu bytes) -> %.0f\n", where(slab).c_str(), nbytes, g_fill);
    return g_fill;
}
}  // namespace jsp

namespace {
struct Pool {
    const char* env;                             // "_MAX=2 _MS=0": suffixes of JSP_POOL_PROBE (a bare "=0" is JSP_POOL_PROBE itself); every knob not named is unset
    int w, h, n;
    std::vector<double> rates;
    double fill = 7000;
    int throw_at = 0;
    size_t budget_bytes = ~(size_t)0;
    long budget_calls = -1;
    bool budget_once = false;
    int device = 0;
};
struct Group { const char* name; std::vector<Pool> pools; };

const char* kKnobs[] = {"", "_MAX", "_HOLD_GB", "_LOG", "_MAPPED", "_THOROUGH", "_MS", "_FORM"};

void set_env(const char* spec) {
    for (const char* k : kKnobs) unsetenv((std::string("JSP_POOL_PROBE") + k).c_str());
    std::string s = spec;
    size_t at = 0;
    while (at < s.size()) {
        size_t end = s.find(' ', at);
        if (end == std::string::npos) end = s.size();
        const std::string tok = s.substr(at, end - at);
        const size_t eq = tok.find('=');
        if (!tok.empty()) setenv(("JSP_POOL_PROBE" + tok.substr(0, eq)).c_str(), tok.substr(eq + 1).c_str(), 1);
        at = end + 1;
    }
}

void run(const Pool& s, int index) {
    std::printf("pool %d: %d frames of %d x %d on device %d, env [%s], fill %.0f, rates [", index, s.n, s.w, s.h, s.device, s.env, s.fill);
    for (size_t i = 0; i < s.rates.size(); ++i) std::printf("%s%.0f", i ? " " : "", s.rates[i]);
    std::printf("]");
    if (s.throw_at) std::printf(", measurement %d throws", s.throw_at);
    if (s.budget_bytes != ~(size_t)0) std::printf(", %zu bytes of device memory", s.budget_bytes);
    if (s.budget_calls >= 0) std::printf(", %ld allocations succeed", s.budget_calls);
    if (s.budget_once) std::printf(", one refusal");
    std::printf("\n");
    set_env(s.env);
    g_rates = s.rates;
    g_fill = s.fill;
    g_rate_calls = 0;
    g_rate_args.clear();
    g_throw_at = s.throw_at;
    g_budget_once = s.budget_once;
    g_next_ordinal = 0;
    stub_alloc_budget(s.budget_bytes, s.budget_calls);
    jsp_pool* p = jsp_pool_create(s.device, s.w, s.h, s.n);
    stub_alloc_budget(~(size_t)0, -1);
    flush();
    if (!p) {
        std::string why = jsp_last_error();       // (a failed HIP call is reported with the file and line it stands in: not part of the record)
        const size_t at = why.rfind(" (");
        if (at != std::string::npos && why.back() == ')' && why.find(".cpp:", at) != std::string::npos) why = why.substr(0, at) + " (FILE:LINE)";
        std::printf(" failed: %s\n", why.c_str());
    } else {
        int attempts = -1;
        const double rate = jsp_pool_store_rate(p, &attempts);
        double ms = -1, rates[64];
        uint64_t peak = 0, limit = 0;
        const int rc = jsp_pool_probe_info(p, &ms, &peak, &limit);
        const int n = jsp_pool_probe_rates(p, rates, 64);
        std::printf(" store rate %.0f, %d attempts, probe_ms %s, held peak %llu, hold limit %llu (%d), tried %d:", rate, attempts, ms > 0 ? ">0" : ms == 0 ? "==0" : "<0",
                    (unsigned long long)peak, (unsigned long long)limit, rc, n);
        for (int i = 0; i < n && i < 64; ++i) std::printf(" %.0f", rates[i]);
        std::vector<std::string> buffers;
        for (int i = 0; i < jsp_pool_count(p); ++i) buffers.push_back(where(jsp_pool_buffer(p, i)));
        std::printf("\n buffers:%s; past the end: %s %s; destroy:\n", listed(buffers).c_str(), where(jsp_pool_buffer(p, -1)).c_str(), where(jsp_pool_buffer(p, jsp_pool_count(p))).c_str());
        jsp_pool_destroy(p);
        flush();
    }
    std::printf(" outstanding: %zu allocations, %zu physical\n", g_live.size(), g_handles.size());
    if (!g_live.empty() || !g_handles.empty()) std::exit(3);
}

const std::vector<double> kFlat{6000};
// what the issue's table lists: four chunk picks, then the older forms until one comes within 1.5 % of the fill
const std::vector<double> kClimb{6000, 6100, 6200, 6300, 6500, 6800, 6200, 6950};

std::vector<Group> groups() {
    std::vector<Group> g;
    // the mapped arrangements: the 3 % bound from both sides, which of the three wins, the second phase and its nine candidates, the time budget
    g.push_back({"mapped", {
        {"_MS=1e12", 64, 48, 32, {6790}},
        {"_MS=1e12", 64, 48, 32, {6789, 6900}},
        {"_MS=1e12", 64, 48, 32, {6000, 6100, 6800}},
        {"_LOG=1 _MS=1e12", 64, 48, 32, {6000, 6500, 6200, 6100, 6600, 6300, 6400, 6550, 6450, 9999}},
        {"_MS=1e12", 64, 48, 32, {6000, 6500, 6200, 6100, 6789, 6790, 9999}},
        {"_MS=0", 64, 48, 32, {6000, 6500, 6200, 9999}},
        {"_MS=0", 64, 48, 32, kFlat},
        {"_MS=1e12", 64, 48, 33, {6000, 6500, 6200, 6100, 6600}},
        {"_MS=1e12 _FORM=7", 64, 48, 47, {6500, 6000, 6790}},
    }});
    // a plain fill that measures nothing: the second phase has no yardstick and ends at once; under THOROUGH nothing is ever "good"
    g.push_back({"fill_zero", {
        {"_MS=1e12", 64, 48, 32, {6000, 6500, 6200, 9999}, 0},
        {"_MS=1e12 _THOROUGH=1", 64, 48, 32, {6000, 6100, 6200, 6300, 6400, 6500, 6600, 9999}, 0},
        {"_MAPPED=0", 64, 48, 32, {6000, 6100, 6200, 6300, 9999}, 0},
        {"_MAPPED=0 _FORM=2 _MAX=8", 64, 48, 32, {6500, 6000, 6100, 6200, 6300, 9999}, 0},
    }});
    g.push_back({"max", {
        {"_MS=1e12 _MAX=1", 64, 48, 32, kFlat},
        {"_MS=1e12 _MAX=2", 64, 48, 32, kFlat},
        {"_MS=1e12 _MAX=3", 64, 48, 32, kFlat},
        {"_MS=1e12 _MAX=0", 64, 48, 32, kFlat},
        {"_MS=1e12 _MAX=17 _THOROUGH=1", 64, 48, 32, kFlat},
        {"_MAPPED=0 _MAX=1", 64, 48, 32, kFlat},
        {"_MAPPED=0 _MAX=2", 64, 48, 32, kFlat},
        {"_MAPPED=0 _MAX=3", 64, 48, 32, kFlat},
        {"_MAPPED=0 _MAX=1 _FORM=0", 64, 48, 32, kFlat},
        {"_MAPPED=0 _MAX=5 _FORM=1", 64, 48, 32, kFlat},
        {"_MS=0 _THOROUGH=1 _MAX=4", 64, 48, 32, kFlat},
    }});
    // the hold limit: below one pool; with a form hinted by the pool before, the hinted candidate counts against it (the run shrinks further, or is not made); the older forms stopped by it
    g.push_back({"hold", {
        {"_MS=1e12 _HOLD_GB=0.0001", 64, 48, 32, kFlat},
        {"_MS=1e12 _HOLD_GB=0.005", 64, 48, 32, kFlat},
        {"_MS=1e12 _HOLD_GB=0.0001 _THOROUGH=1", 64, 48, 32, kFlat},
        {"_MAPPED=0 _HOLD_GB=0.0001", 64, 48, 32, kFlat},
        {"_LOG=1 _MAPPED=0 _HOLD_GB=0.0012", 64, 48, 32, kClimb},
        {"_LOG=1 _MAPPED=0 _HOLD_GB=0.0008", 64, 48, 32, kClimb},
        {"_MAPPED=0 _HOLD_GB=0.0008 _FORM=1", 64, 48, 32, kClimb},
        {"_MAPPED=0 _HOLD_GB=0.0013", 64, 48, 33, kClimb},
    }});
    // THOROUGH: the hipMalloc forms behind the mapped ones; sixteen candidates at most
    g.push_back({"thorough", {
        {"_MS=1e12 _THOROUGH=1", 64, 48, 32, kFlat},
        {"_LOG=1 _MS=0 _THOROUGH=1", 64, 48, 32, kFlat},
        {"_MS=0 _THOROUGH=1", 64, 48, 32, {6500, 6400, 6300, 6000, 6501, 6100, 6200, 6600, 6696, 6697, 6896}},   // the better probe wins against a mapped candidate, no allowance; an older form needs 3 % over the chunked one
        {"_MS=0 _THOROUGH=1", 64, 48, 32, {6500, 6400, 6300, 6000, 6500, 6100, 6200, 6501, 6400, 6895}},         // ... and none against a mapped one
        {"_MS=0 _THOROUGH=1", 64, 48, 32, {6000, 6790}},                                                         // good enough: THOROUGH asks for nothing more
        {"_MS=0 _THOROUGH=1 _FORM=2 _MAX=12", 64, 48, 32, {6500, 6400, 6300, 6600, 6000, 6100, 6200, 6300, 6000, 6000, 6700}},
        {"_MS=0 _THOROUGH=1 _FORM=0", 64, 48, 32, {6500, 6400, 6300, 6895}},
        {"_MS=0 _THOROUGH=1 _FORM=0", 64, 48, 32, {6500, 6400, 6300, 6200, 6895}},
    }});
    // without the mapped forms: the chunk run's four picks and where they stop, "good enough", the 3 % allowance, the round of older forms
    g.push_back({"chunks", {
        {"_MAPPED=0", 64, 48, 32, {6000, 6895}},
        {"_MAPPED=0", 64, 48, 32, {6000, 6894, 6100, 6200}},
        {"_MAPPED=0", 64, 48, 32, {6000, 6650, 6100, 6200}},
        {"_MAPPED=0", 64, 48, 32, {6000, 6649, 6100, 6200, 6848, 6849, 6000, 6895}},
        {"_MAPPED=0", 64, 48, 32, {6895}},
        {"_MAPPED=0 _MAX=8", 64, 48, 32, {6000, 6100, 6300, 6200, 6400, 6000}},
    }});
    // the form that won is remembered: by the process (the same pool twice holds a different peak) and from JSP_POOL_PROBE_FORM
    g.push_back({"hint", {
        {"_MAPPED=0", 64, 48, 32, kClimb},
        {"_MAPPED=0", 64, 48, 32, kClimb},
        {"_MS=0 _THOROUGH=1", 64, 48, 32, {6000, 6100, 6200, 6500, 6000, 6000, 6000, 6000, 6800, 6900}},
        {"_MAPPED=0", 64, 48, 32, {6895}},
        {"_MAPPED=0", 64, 48, 32, {6500, 6000, 6100, 6200, 6312, 6000, 6895}},        // the chunked candidate within 3 % of the hinted form: it stands before it
        {"_MAPPED=0", 64, 48, 32, {6000, 6895}},                                      // ... and a chunked candidate won: nothing is hinted any more
    }});
    g.push_back({"form", {
        {"_LOG=1 _MAPPED=0 _FORM=0", 64, 48, 32, {6500, 6000, 6100, 6200, 6310, 6000, 6000, 6895}},   // 6310 x 1.03 < 6500: the hinted form stays in front
        {"_MAPPED=0 _FORM=1", 64, 48, 32, {6895}},
        {"_MAPPED=0 _FORM=2", 64, 48, 32, {6500, 6000, 6100, 6200, 6312, 6503, 6504, 6895}},   // 6312 x 1.03 > 6500; then an older form needs 3 % over 6312
        {"_MAPPED=0 _FORM=1", 64, 48, 32, {6894, 6000, 6895}},
        {"_MAPPED=0 _FORM=-1", 64, 48, 32, {6000, 6895}},
        {"_MAPPED=0 _FORM=3", 64, 48, 32, {6000, 6895}},
    }});
    // every search on pools whose last chunk is short (33, 34, 47), whose strided order takes 19 for 17 (34) and on larger ones
    std::vector<Pool> sizes;
    for (int n : {32, 33, 34, 40, 47}) {
        sizes.push_back({"_MS=0 _THOROUGH=1 _MAX=10", 64, 48, n, kFlat});
        sizes.push_back({"_MAPPED=0", 64, 48, n, kClimb});
    }
    sizes.push_back({"_MS=1e12", 64, 48, 64, {6000, 6500, 6200, 6100, 6900}});
    g.push_back({"sizes", sizes});
    // frames just over 2 MB ("a physical allocation per frame" is one), of 0.75 MB (two to an allocation) and far smaller than a page
    g.push_back({"large_frames", {
        {"_LOG=1 _MS=1e12 _HOLD_GB=0.5", 768, 704, 32, kFlat},
        {"_MS=0 _THOROUGH=1 _MAX=8", 768, 704, 33, kFlat},
        {"_MS=0", 512, 384, 35, {6000, 6100, 6200}},
    }});
    g.push_back({"small_frames", {
        {"_MS=0 _THOROUGH=1 _MAX=10", 16, 12, 40, kFlat},
        {"_MS=1e12", 4, 4, 32, {6000, 6100, 6200, 6300, 6790}},
        {"_MAPPED=0", 16, 16, 600, {6000, 6100, 6895}},
    }});
    // pools that are not probed, and pools that are refused
    g.push_back({"not_probed", {
        {"", 64, 48, 31, kFlat},
        {"", 66, 48, 32, kFlat},
        {"", 64, 50, 32, kFlat},
        {"=0", 64, 48, 32, kFlat},
        {"=1 _MS=0", 64, 48, 32, kFlat},
        {"", 64, 48, 1, kFlat},
        {"", 0, 48, 32, kFlat},
        {"", 64, -1, 32, kFlat},
        {"", 64, 48, 0, kFlat},
        {"", 64, 48, 32, kFlat, 7000, 0, ~(size_t)0, -1, false, 1},
        {"", 64, 48, 32, kFlat, 7000, 0, ~(size_t)0, -1, false, -1},
    }});
    // device memory running out.  (64 x 48: a frame 12 288 bytes, a pool of 32 393 216, a chunk 196 608, the chunk run 1 572 864)
    g.push_back({"out_of_memory", {
        {"_MAPPED=0", 64, 48, 32, kClimb, 7000, 0, 1000000},                          // inside the chunk run: the older forms, as many as fit
        {"_MAPPED=0", 64, 48, 32, kClimb, 7000, 0, 300000},                           // ... and inside the first older form, nothing held: refused
        {"_MAPPED=0 _FORM=1", 64, 48, 32, kClimb, 7000, 0, 300000},
        {"_MAPPED=0 _FORM=2", 64, 48, 32, kClimb, 7000, 0, 600000},                   // the hinted form held, the run refused, an older form refused half-way
        {"_MAPPED=0 _HOLD_GB=0.0008", 64, 48, 32, kClimb, 7000, 0, 1000000},
        {"_MS=1e12", 768, 704, 32, kClimb, 7000, 0, ~(size_t)0, 2, true},             // hipMemCreate refused at the second handle: a partly mapped range, the slab yardstick, the hipMalloc forms
        {"_MS=1e12", 768, 704, 32, kClimb, 7000, 0, ~(size_t)0, 1, true},             // ... at the first
        {"_MS=1e12", 64, 48, 32, {6000, 6100, 6200}, 7000, 0, ~(size_t)0, 3, true},   // ... inside the second arrangement: the first is kept
    }});
    // the measurement throwing, in each kind of candidate, with and without others held
    g.push_back({"throws", {
        {"_MS=1e12", 64, 48, 32, kFlat, 7000, 1},
        {"_MS=1e12", 64, 48, 32, {6000, 5900}, 7000, 3},
        {"_MS=1e12", 64, 48, 32, kFlat, 7000, 6},
        {"_MAPPED=0", 64, 48, 32, kFlat, 7000, 1},
        {"_MAPPED=0", 64, 48, 32, kFlat, 7000, 3},
        {"_MAPPED=0", 64, 48, 32, kFlat, 7000, 5},
        {"_MAPPED=0", 64, 48, 32, kFlat, 7000, 7},
        {"_MAPPED=0 _FORM=0", 64, 48, 32, kFlat, 7000, 1},
        {"_MAPPED=0 _FORM=0", 64, 48, 32, kFlat, 7000, 3},
        {"_MS=0 _THOROUGH=1", 64, 48, 32, kFlat, 7000, 5},
        {"_MS=0 _THOROUGH=1", 64, 48, 32, kFlat, 7000, 9},
        {"_MS=0", 64, 48, 32, kFlat},                                                  // and the process is none the worse for it
    }});
    // a measurement of 0 GB/s: such a candidate is never "the best so far"
    // the hold limit shrinks the chunk run's spread from 4 to 3 (on 32 and on 33 frames) and to 2, where the third pick changes form.  Nothing is
    // hinted: a chunked candidate wins the first two pools.
    g.push_back({"spread", {
        {"_LOG=1 _MAPPED=0 _HOLD_GB=0.0013", 64, 48, 32, {6000, 6100, 6200, 6650}},
        {"_MAPPED=0 _HOLD_GB=0.002", 64, 48, 33, {6000, 6100, 6650, 6200}},
        {"_LOG=1 _MAPPED=0 _HOLD_GB=0.0008", 64, 48, 32, kClimb},
    }});
    g.push_back({"rate_zero", {
        {"_MS=0", 64, 48, 32, {0, 6000, 5000}},
        {"_MS=0 _MAX=9", 64, 48, 32, {0}},
        {"_MAPPED=0 _MAX=6", 64, 48, 32, {0, 0, 0, 0, 0, 6000}},
    }});
    // NOT part of the record (their names begin with "new_", --list leaves them out): what the code does differently from the recorded commit, which
    // leaked the frames of a pool that is not probed when one of their allocations failed, and cast a negative JSP_POOL_PROBE_HOLD_GB to an unsigned
    // number (undefined).  tests/test_pool_probe_trace_cpu.py holds what is expected of them.
    g.push_back({"new_failures", {
        {"", 64, 48, 8, kFlat, 7000, 0, 50000},                                               // a pool that is not probed, the fifth frame refused: nothing outstanding
        {"_MS=0", 64, 48, 32, kFlat, 7000, 0, ~(size_t)0, 0},                                 // not even the table
        {"_MS=0 _HOLD_GB=-1", 64, 48, 32, kFlat},                                             // a negative limit is none: a quarter of the free memory
    }});
    return g;
}
}  // namespace

int main(int argc, char** argv) {
    dup2(1, 2);                                  // the probe's log lines (stderr) take their place among the calls
    setvbuf(stdout, nullptr, _IONBF, 0);
    const std::vector<Group> all = groups();
    if (argc == 3 && std::strcmp(argv[1], "--full") == 0) { g_full = true; --argc; ++argv; }
    if (argc == 2 && std::strcmp(argv[1], "--list") == 0) {
        for (const Group& g : all) if (std::strncmp(g.name, "new_", 4) != 0) std::printf("%s\n", g.name);
        return 0;
    }
    stub_mem_observer = observe;
    for (const Group& g : all) {
        if (argc != 2 || std::strcmp(argv[1], g.name) != 0) continue;
        std::printf("==== group %s\n", g.name);
        for (size_t i = 0; i < g.pools.size(); ++i) run(g.pools[i], (int)i);
        return 0;
    }
    std::fprintf(stderr, "usage: trace [--full] <group> | trace --list\n");
    return 2;
}
