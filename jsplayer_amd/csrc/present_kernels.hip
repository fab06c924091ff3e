// What the reference leaves to the browser's compositor (Main.on_stage_resize, Main.hx:288-319: the bitmap drawn through the display
// matrix  (sx, sy) = (k x - dx, -k y + win_h + dy)  with bitmap.smoothing, Main.hx:948), as ONE HBM-bound HIP kernel:
//   display_present : frame buffer (bottom-up, stride frame_w) -> the canvas pixels of a win_w x win_h window, top row first —
//                     Manager.fill_bitmap_data's conversion, the row flip, the crop and the resampling in one pass.
// The resampling rule is this project's own, in integers (include/jsplayer_amd.h, jsp_display_present): 16.16 bitmap coordinates of
// each output pixel's centre, X = ax + ox * step, Y = ay - oy * step; nearest = the pixel at (X >> 16, Y >> 16); bilinear = four taps
// around (X - 32768, Y - 32768) with 8-bit weights, every byte of the converted words blended separately.  Its arithmetic is not
// written here: fixed16, the geometry and the shared bounds are present_rule.h's, convert, taps, hblend and vblend
// present_rule_device.h's, where the index kernels (index_present_device.h) take them from too.
//
// Shape: a lane owns kPresentRun consecutive pixels of a row (one 16-byte non-temporal store where `out` and its pitch allow, scalar
// stores otherwise and for the row's remainder), a workgroup is one wave — kPresentSpanX pixels of kPresentBandRows output rows.  A
// lane's horizontal taps and weights do not depend on the row: they are worked out once per band (in 64 bits; a covered pixel's fit
// 31) and stay in registers.  Bilinear keeps the two source rows it blended horizontally last (two 16-bit sums per word, four words
// per pixel): for k >= 1 the next output row needs at least one of them again, and which is a scalar decision — the rows depend on
// blockIdx.y alone.  mode and filter are template parameters.  No LDS, no full-size converted frame.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "../../include/jsplayer_amd.h"
#include "common.h"
#include "present_rule_device.h"

namespace {

using namespace jsp::present_rule;

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
                const Taps tx = taps((int)X, a.fw);            // (covered: X < 2^30)
                x0[j] = tx.t0;
                x1[j] = tx.t1;
                wx[j] = tx.w;
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
                    const uint32_t c = convert(row[x0[j]], MODE);
                    if (in[j]) px[j] = c;
                }
            } else {
                const Taps ty = taps((int)Y, a.fh);
                const int r0 = ty.t0, r1 = ty.t1;
                const uint32_t wy = ty.w;
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
                    for (int j = 0; j < kPresentRun; ++j) na[j] = hblend(convert(row[x0[j]], MODE), convert(row[x1[j]], MODE), wx[j]);
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
                    for (int j = 0; j < kPresentRun; ++j) nb[j] = hblend(convert(row[x0[j]], MODE), convert(row[x1[j]], MODE), wx[j]);
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

}  // namespace

extern "C" {

int jsp_display_present(const int32_t* frame, int frame_w, int frame_h, int32_t* out, int win_w, int win_h, size_t out_pitch,
                        double k, double dx, double dy, int mode, int filter, uint32_t background, void* hip_stream) {
    try {
        if (!frame || !out) throw std::runtime_error("null pointer");
        if (frame_w < 1 || frame_w > 16384 || frame_h < 1 || frame_h > 16384) throw std::runtime_error("frame size outside 1..16384");
        if (const char* why = window_refusal(win_w, win_h)) throw std::runtime_error(why);
        if (out_pitch < (size_t)win_w) throw std::runtime_error("out_pitch below win_w");
        if (const char* why = view_refusal(k, dx, dy, mode)) throw std::runtime_error(why);
        if (filter != JSP_PRESENT_NEAREST && filter != JSP_PRESENT_BILINEAR) throw std::runtime_error("unknown filter");
        const Geometry g = geometry(win_h, k, dx, dy);
        PresentArgs a;
        a.src = reinterpret_cast<const uint32_t*>(frame);
        a.dst = reinterpret_cast<uint32_t*>(out);
        a.fw = frame_w; a.fh = frame_h; a.ww = win_w; a.wh = win_h;
        a.pitch = out_pitch;
        a.step = g.step; a.ax = g.ax; a.ay = g.ay;
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
