// What the reference leaves to the browser's compositor (Main.on_stage_resize, Main.hx:288-319: the bitmap drawn through the display
// matrix  (sx, sy) = (k x - dx, -k y + win_h + dy)  with bitmap.smoothing, Main.hx:948), as ONE HBM-bound HIP kernel:
//   display_present : frame buffer (bottom-up, stride frame_w) -> the canvas pixels of a win_w x win_h window, top row first —
//                     Manager.fill_bitmap_data's conversion, the row flip, the crop and the resampling in one pass.
// The resampling rule is this project's own, in integers (include/jsplayer_amd.h, jsp_display_present): 16.16 bitmap coordinates of
// each output pixel's centre, X = ax + ox * step, Y = ay - oy * step; nearest = the pixel at (X >> 16, Y >> 16); bilinear = four taps
// around (X - 32768, Y - 32768) with 8-bit weights, every byte of the converted words blended separately.
//
// Shape: a lane owns kPresentRun consecutive pixels of a row (one 16-byte non-temporal store where `out` and its pitch allow, scalar
// stores otherwise and for the row's remainder), a workgroup is one wave — kPresentSpanX pixels of kPresentBandRows output rows.  A
// lane's horizontal taps and weights do not depend on the row: they are worked out once per band (in 64 bits; a covered pixel's fit
// 31) and stay in registers.  Bilinear keeps the two source rows it blended horizontally last (two 16-bit sums per word, four words
// per pixel): for k >= 1 the next output row needs at least one of them again, and which is a scalar decision — the rows depend on
// blockIdx.y alone.  mode and filter are template parameters.  No LDS, no full-size converted frame.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstddef>
#include <cstdint>

#include "../../include/jsplayer_amd.h"
#include "common.h"

namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

constexpr int kPresentRun = 4;                               // pixels per lane: one 16-byte store
constexpr int kPresentLanes = 64;                            // lanes per workgroup (one wave)
constexpr int kPresentSpanX = kPresentLanes * kPresentRun;   // output pixels a workgroup covers in x
constexpr int kPresentBandRows = 8;                          // output rows a workgroup covers

struct PresentArgs {
    const uint32_t* src;
    uint32_t* dst;
    int fw, fh, ww, wh;
    size_t pitch;
    long long ax, ay;      // 16.16 bitmap coordinates of the centre of output pixel (0, 0)
    int step;              // 16.16 bitmap pixels per output pixel
    uint32_t bg;
    int vec;               // every row of `dst` starts on a 16-byte boundary
};

// the four conversions of display_kernels.hip's convert(), bit for bit
template <int MODE>
__device__ __forceinline__ uint32_t convert(uint32_t c) {
    if (MODE == JSP_DISPLAY_CANVAS) return 0xFF000000u | ((c & 0xFFu) << 16) | (c & 0xFF00u) | ((c >> 16) & 0xFFu);   // Manager.hx:379
    if (MODE == JSP_DISPLAY_CANVAS_RGB15) return 0xFF000000u | (c << 3);                                               // :370
    if (MODE == JSP_DISPLAY_SETPIXELS) return 0xFF000000u | c;                                                         // :351
    return c << 11;                                                                                                    // :340
}

// p0 * (256 - w) + p1 * w for the four bytes of two converted words: bytes 0 and 2 in the halves of .e, bytes 1 and 3 in those of .o
// (a byte times 256 at most: each sum fits its 16 bits)
struct HSum { uint32_t e, o; };
__device__ __forceinline__ HSum hblend(uint32_t p0, uint32_t p1, uint32_t w) {
    const uint32_t v = 256u - w;
    return HSum{(p0 & 0x00FF00FFu) * v + (p1 & 0x00FF00FFu) * w, ((p0 >> 8) & 0x00FF00FFu) * v + ((p1 >> 8) & 0x00FF00FFu) * w};
}
__device__ __forceinline__ uint32_t vblend(HSum a, HSum b, uint32_t w) {
    const uint32_t v = 256u - w;
    const uint32_t b0 = ((a.e & 0xFFFFu) * v + (b.e & 0xFFFFu) * w + 32768u) >> 16;
    const uint32_t b2 = ((a.e >> 16) * v + (b.e >> 16) * w + 32768u) >> 16;
    const uint32_t b1 = ((a.o & 0xFFFFu) * v + (b.o & 0xFFFFu) * w + 32768u) >> 16;
    const uint32_t b3 = ((a.o >> 16) * v + (b.o >> 16) * w + 32768u) >> 16;
    return b0 | (b1 << 8) | (b2 << 16) | (b3 << 24);
}

template <int MODE, int FILTER>
__global__ __launch_bounds__(kPresentLanes) void display_present_kernel(const PresentArgs a) {
    const int ox0 = ((int)blockIdx.x * kPresentLanes + (int)threadIdx.x) * kPresentRun;
    if (ox0 >= a.ww) return;
    const int n = min(kPresentRun, a.ww - ox0);
    const int oy0 = (int)blockIdx.y * kPresentBandRows, oy1 = min(oy0 + kPresentBandRows, a.wh);
    const long long x_end = (long long)a.fw << 16, y_end = (long long)a.fh << 16;

    // the lane's columns: covered or not, tap indices (clamped into the picture; 0 where not covered: any valid index) and weight
    bool in[kPresentRun];
    int x0[kPresentRun], x1[kPresentRun];
    uint32_t wx[kPresentRun];
#pragma unroll
    for (int j = 0; j < kPresentRun; ++j) {
        const long long X = a.ax + (long long)(ox0 + j) * a.step;
        in[j] = j < n && X >= 0 && X < x_end;
        x0[j] = x1[j] = 0;
        wx[j] = 0;
        if (in[j]) {
            if (FILTER == JSP_PRESENT_NEAREST) {
                x0[j] = (int)(X >> 16);
            } else {
                const int U = (int)X - 32768;                  // (covered: X < 2^30)
                const int t = U >> 16;                         // -1 .. fw - 1
                x0[j] = max(t, 0);
                x1[j] = min(t + 1, a.fw - 1);
                wx[j] = (uint32_t)(U & 0xFFFF) >> 8;
            }
        }
    }

    int ra = -1, rb = -1;                                      // the source rows held in ha / hb
    HSum ha[kPresentRun], hb[kPresentRun];
#pragma unroll
    for (int j = 0; j < kPresentRun; ++j) ha[j] = hb[j] = HSum{0u, 0u};

    for (int oy = oy0; oy < oy1; ++oy) {
        const long long Y = a.ay - (long long)oy * a.step;
        uint32_t px[kPresentRun];
#pragma unroll
        for (int j = 0; j < kPresentRun; ++j) px[j] = a.bg;
        if (Y >= 0 && Y < y_end) {                             // (uniform)
            if (FILTER == JSP_PRESENT_NEAREST) {
                const uint32_t* row = a.src + (size_t)(Y >> 16) * a.fw;
#pragma unroll
                for (int j = 0; j < kPresentRun; ++j) {
                    const uint32_t c = convert<MODE>(row[x0[j]]);
                    if (in[j]) px[j] = c;
                }
            } else {
                const int V = (int)Y - 32768;
                const int t = V >> 16;
                const int r0 = max(t, 0), r1 = min(t + 1, a.fh - 1);
                const uint32_t wy = (uint32_t)(V & 0xFFFF) >> 8;
                HSum na[kPresentRun], nb[kPresentRun];
                if (r0 == ra) {
#pragma unroll
                    for (int j = 0; j < kPresentRun; ++j) na[j] = ha[j];
                } else if (r0 == rb) {
#pragma unroll
                    for (int j = 0; j < kPresentRun; ++j) na[j] = hb[j];
                } else {
                    const uint32_t* row = a.src + (size_t)r0 * a.fw;
#pragma unroll
                    for (int j = 0; j < kPresentRun; ++j) na[j] = hblend(convert<MODE>(row[x0[j]]), convert<MODE>(row[x1[j]]), wx[j]);
                }
                if (r1 == r0) {
#pragma unroll
                    for (int j = 0; j < kPresentRun; ++j) nb[j] = na[j];
                } else if (r1 == ra) {
#pragma unroll
                    for (int j = 0; j < kPresentRun; ++j) nb[j] = ha[j];
                } else if (r1 == rb) {
#pragma unroll
                    for (int j = 0; j < kPresentRun; ++j) nb[j] = hb[j];
                } else {
                    const uint32_t* row = a.src + (size_t)r1 * a.fw;
#pragma unroll
                    for (int j = 0; j < kPresentRun; ++j) nb[j] = hblend(convert<MODE>(row[x0[j]]), convert<MODE>(row[x1[j]]), wx[j]);
                }
                ra = r0;
                rb = r1;
#pragma unroll
                for (int j = 0; j < kPresentRun; ++j) {
                    ha[j] = na[j];
                    hb[j] = nb[j];
                    if (in[j]) px[j] = vblend(na[j], nb[j], wy);
                }
            }
        }
        uint32_t* d = a.dst + (size_t)oy * a.pitch + ox0;
        if (a.vec && n == kPresentRun) {
            __builtin_nontemporal_store(u32x4{px[0], px[1], px[2], px[3]}, reinterpret_cast<u32x4*>(d));
        } else {
#pragma unroll
            for (int j = 0; j < kPresentRun; ++j)
                if (j < n) d[j] = px[j];
        }
    }
}

template <int MODE>
void launch_filter(int filter, dim3 grid, hipStream_t s, const PresentArgs& a) {
    if (filter == JSP_PRESENT_NEAREST) hipLaunchKernelGGL((display_present_kernel<MODE, JSP_PRESENT_NEAREST>), grid, dim3(kPresentLanes), 0, s, a);
    else hipLaunchKernelGGL((display_present_kernel<MODE, JSP_PRESENT_BILINEAR>), grid, dim3(kPresentLanes), 0, s, a);
}

// F(v) = floor(v * 65536 + 0.5) as a 64-bit integer.  A value beyond +-2^62 (a far-away dx or dy) is held there: with ox * step below
// 2^36 every pixel of such a window lies outside the picture either way, so the window is the one the unbounded integer gives.
long long fixed16(double v) {
    const double f = std::floor(v * 65536.0 + 0.5), lim = 4611686018427387904.0;
    if (f >= lim) return 1ll << 62;
    if (f <= -lim) return -(1ll << 62);
    return (long long)f;
}

}  // namespace

extern "C" {

int jsp_display_present(const int32_t* frame, int frame_w, int frame_h, int32_t* out, int win_w, int win_h, size_t out_pitch,
                        double k, double dx, double dy, int mode, int filter, uint32_t background, void* hip_stream) {
    try {
        if (!frame || !out) throw std::runtime_error("null pointer");
        if (frame_w < 1 || frame_w > 16384 || frame_h < 1 || frame_h > 16384) throw std::runtime_error("frame size outside 1..16384");
        if (win_w < 1 || win_w > 16384 || win_h < 1 || win_h > 16384) throw std::runtime_error("window size outside 1..16384");
        if (out_pitch < (size_t)win_w) throw std::runtime_error("out_pitch below win_w");
        if (!std::isfinite(k) || !std::isfinite(dx) || !std::isfinite(dy)) throw std::runtime_error("k, dx, dy must be finite");
        if (k < 1.0 / 64.0 || k > 64.0) throw std::runtime_error("k outside 1/64..64");
        if (mode < JSP_DISPLAY_CANVAS || mode > JSP_DISPLAY_SETPIXELS_RGB15) throw std::runtime_error("unknown mode");
        if (filter != JSP_PRESENT_NEAREST && filter != JSP_PRESENT_BILINEAR) throw std::runtime_error("unknown filter");
        PresentArgs a;
        a.src = reinterpret_cast<const uint32_t*>(frame);
        a.dst = reinterpret_cast<uint32_t*>(out);
        a.fw = frame_w; a.fh = frame_h; a.ww = win_w; a.wh = win_h;
        a.pitch = out_pitch;
        a.step = (int)fixed16(1.0 / k);                        // 1024 .. 64 * 65536
        a.ax = fixed16((0.5 + dx) / k);
        a.ay = fixed16(((double)win_h + dy - 0.5) / k);
        a.bg = background;
        a.vec = ((reinterpret_cast<uintptr_t>(out) & 15) == 0 && (out_pitch & 3) == 0) ? 1 : 0;
        const dim3 grid((unsigned)((win_w + kPresentSpanX - 1) / kPresentSpanX), (unsigned)((win_h + kPresentBandRows - 1) / kPresentBandRows));
        hipStream_t s = static_cast<hipStream_t>(hip_stream);
        switch (mode) {
            case JSP_DISPLAY_CANVAS: launch_filter<JSP_DISPLAY_CANVAS>(filter, grid, s, a); break;
            case JSP_DISPLAY_CANVAS_RGB15: launch_filter<JSP_DISPLAY_CANVAS_RGB15>(filter, grid, s, a); break;
            case JSP_DISPLAY_SETPIXELS: launch_filter<JSP_DISPLAY_SETPIXELS>(filter, grid, s, a); break;
            default: launch_filter<JSP_DISPLAY_SETPIXELS_RGB15>(filter, grid, s, a); break;
        }
        JSP_HIP(hipGetLastError());
        return 0;
    } catch (const std::exception& e) {
        jsp::set_error("display_present: %s", e.what());
        return JSP_ERROR_OCCURED;
    }
}
}
