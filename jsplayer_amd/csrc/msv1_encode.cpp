// The host side of the MSVideo1 16-bit encoder (jsp_msv1_encoder_create / jsp_msv1_encode_frames; the rule and the two kernels:
// msv1_encode_kernels.hip).  An encoder is a size and its scratch: no codec is involved and no frame buffer is written.  A call
// runs in slices of pictures so that the scratch stays bounded, in the order of the clip calls (msv1_seek.cpp, clip_frames): a sizes
// launch per slice first — the lengths of ALL frames are known before a byte reaches `out` — then a sizes and a gather launch per
// slice (one slice: its records and slots are still there, the gather alone).
#include <algorithm>
#include <vector>

#include "../../include/jsplayer_amd.h"
#include "common.h"
#include "msv1_encode.h"
#include "msv1_seek.h"

using namespace jsp;

struct jsp_encoder {
    int device = 0;
    int width = 0, height = 0, nbx = 0, nb = 0;
    DeviceBuffer d;   // one slice: the picture lists and bases, totals and first coded blocks, records, slots, the frames at their bound
    PinnedBuffer h;   // the host's side of the lists, the bases and the totals
};

namespace {
constexpr int kEncodeMaxSlice = 16;                   // pictures a slice at most ...
constexpr uint64_t kEncodeSliceBudget = 64ull << 20;  // ... and fewer when their scratch would pass this (one picture always goes)

int fail(const char* fmt, const char* what = "") {
    set_error(fmt, what);
    return JSP_ERROR_OCCURED;
}

size_t align16(size_t v) { return (v + 15) & ~(size_t)15; }

// Where the parts of a slice of S pictures of nb blocks (nwg workgroups) lie in the device buffer; the host buffer mirrors [0, first_at).
struct EncodeLayout {
    size_t pictures_at, previous_at, bases_at, totals_at, first_at, records_at, slots_at, out_at, bytes;
    EncodeLayout(size_t S, size_t nb, size_t nwg) {
        pictures_at = 0;
        previous_at = pictures_at + S * sizeof(void*);
        bases_at = previous_at + S * sizeof(void*);
        totals_at = bases_at + S * sizeof(uint64_t);
        first_at = totals_at + S * nwg * sizeof(uint32_t);
        records_at = first_at + S * nwg * sizeof(uint32_t);
        slots_at = align16(records_at + S * nb * sizeof(uint32_t));
        out_at = align16(slots_at + S * nb * MSV1_ENCODE_SLOT_WORDS * sizeof(uint32_t));
        bytes = out_at + S * nb * 18 + 16;
    }
};
}  // namespace

extern "C" jsp_encoder* jsp_msv1_encoder_create(int device_id, int width, int height) {
    if (width < 4 || height < 4 || width > 16384 || height > 16384) {
        set_error("msv1_encode: width and height must be 4 .. 16384 (got %d x %d)", width, height);
        return nullptr;
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device_id < 0 || device_id >= ndev) {
        (void)hipGetLastError();
        set_error("msv1_encode: no device %d", device_id);
        return nullptr;
    }
    jsp_encoder* e = new jsp_encoder;
    e->device = device_id;
    e->width = width;
    e->height = height;
    e->nbx = width >> 2;
    e->nb = (width >> 2) * (height >> 2);
    return e;
}

extern "C" void jsp_msv1_encoder_destroy(jsp_encoder* e) {
    if (!e) return;
    (void)hipSetDevice(e->device);
    delete e;
}

extern "C" int jsp_msv1_encode_bound(const jsp_encoder* e, size_t* bytes) {
    if (!e || !bytes) return fail("msv1_encode: null argument");
    *bytes = (size_t)e->nb * 18u;
    return JSP_ZERO_STATE;
}

extern "C" int jsp_msv1_encode_frames(jsp_encoder* e, int n, const int32_t* const* pictures, const int32_t* const* previous, ptrdiff_t pitch,
                                      uint8_t* out, size_t cap, size_t* lens, size_t* total, void* hip_stream) {
    const bool n_ok = n >= 1 && n <= 4096;
    const auto zero = [&] {
        if (total) *total = 0;
        if (lens && n_ok) std::fill(lens, lens + n, (size_t)0);
    };
    zero();
    if (!e || !pictures || !lens || !total || (!out && cap)) return fail("msv1_encode: null argument");
    if ((pitch < 0 ? -pitch : pitch) < (ptrdiff_t)e->width) return fail("msv1_encode: |pitch| is smaller than the width");
    if (!n_ok) return fail("msv1_encode: n is outside 1..4096");
    for (int i = 0; i < n; ++i)
        if (!pictures[i]) return fail("msv1_encode: null argument (a picture)");
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    try {
        JSP_HIP(hipSetDevice(e->device));
        const size_t N = (size_t)n, nb = (size_t)e->nb, nwg = (size_t)msv1_keyframe_workgroups(e->nb), bound = nb * 18u;
        size_t S = std::clamp<uint64_t>(kEncodeSliceBudget / EncodeLayout(1, nb, nwg).bytes, 1, kEncodeMaxSlice);
        S = std::min(S, N);
        const EncodeLayout l(S, nb, nwg);
        e->d.reserve(l.bytes);
        e->h.reserve(l.first_at);
        uint8_t* d = e->d.as<uint8_t>();
        uint8_t* h = e->h.as<uint8_t>();
        const Msv1EncodeArgs k{reinterpret_cast<const int32_t* const*>(d + l.pictures_at),
                               reinterpret_cast<const int32_t* const*>(d + l.previous_at),
                               pitch,
                               e->nbx,
                               e->nb,
                               reinterpret_cast<const uint64_t*>(d + l.bases_at),
                               reinterpret_cast<uint32_t*>(d + l.totals_at),
                               reinterpret_cast<uint32_t*>(d + l.first_at),
                               reinterpret_cast<uint32_t*>(d + l.records_at),
                               reinterpret_cast<uint32_t*>(d + l.slots_at),
                               d + l.out_at};
        std::vector<size_t> length(N, 0);
        // pictures [j0, j0 + m) and where their frames start go to the device, then the sizes launch (not when its results are there)
        const auto upload = [&](size_t j0, size_t m, bool launch) {
            const int32_t** hp = reinterpret_cast<const int32_t**>(h + l.pictures_at);
            const int32_t** hq = reinterpret_cast<const int32_t**>(h + l.previous_at);
            uint64_t* hb = reinterpret_cast<uint64_t*>(h + l.bases_at);
            uint64_t at = 0;
            bool vec = pitch % 4 == 0;
            for (size_t i = 0; i < m; ++i) {
                hp[i] = pictures[j0 + i];
                hq[i] = previous ? previous[j0 + i] : nullptr;
                hb[i] = at;
                at += length[j0 + i];
                vec = vec && (reinterpret_cast<uintptr_t>(hp[i]) | reinterpret_cast<uintptr_t>(hq[i])) % 16 == 0;
            }
            JSP_HIP(hipMemcpyAsync(d, h, l.totals_at, hipMemcpyHostToDevice, stream));
            if (!launch) return;
            msv1_launch_encode_sizes(k, (int)m, vec, stream);
            JSP_HIP(hipGetLastError());
        };
        for (size_t j0 = 0; j0 < N; j0 += S) {
            const size_t m = std::min(S, N - j0);
            upload(j0, m, true);
            JSP_HIP(hipMemcpyAsync(h + l.totals_at, d + l.totals_at, l.first_at - l.totals_at, hipMemcpyDeviceToHost, stream));
            JSP_HIP(hipStreamSynchronize(stream));
            const uint32_t* totals = reinterpret_cast<const uint32_t*>(h + l.totals_at);
            for (size_t i = 0; i < m; ++i) {
                for (size_t g = 0; g < nwg; ++g) length[j0 + i] += totals[i * nwg + g];
                if (length[j0 + i] > bound) throw std::runtime_error("msv1_encode: a frame is longer than its bound");
            }
        }
        size_t sum = 0;
        for (size_t j = 0; j < N; ++j) sum += (lens[j] = length[j]);
        *total = sum;
        if (cap < sum) return fail("msv1_encode: cap is smaller than the frames (*total has their length, lens[] each frame's)");
        size_t at = 0;
        for (size_t j0 = 0; j0 < N; j0 += S) {
            const size_t m = std::min(S, N - j0);
            upload(j0, m, S < N);
            msv1_launch_encode_gather(k, (int)m, stream);
            JSP_HIP(hipGetLastError());
            size_t bytes = 0;
            for (size_t i = 0; i < m; ++i) bytes += length[j0 + i];
            JSP_HIP(hipMemcpyAsync(out + at, k.out, bytes, hipMemcpyDeviceToHost, stream));
            JSP_HIP(hipStreamSynchronize(stream));
            at += bytes;
        }
        return JSP_ZERO_STATE;
    } catch (const std::exception& ex) {
        zero();
        set_error("%s", ex.what());
        return JSP_ERROR_OCCURED;
    }
}
