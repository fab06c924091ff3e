// jsp_display_present_area: the window of jsp_display_present (present_kernels.hip — the same display matrix, the same 16.16 centres
// X = ax + ox * step, Y = ay - oy * step, the same pixels covered), but every covered pixel is the AREA AVERAGE of the converted source
// pixels under a step x step box around its centre instead of one or four samples of them: what "Fit" of a screen recording into a
// small window needs.  The rule is in integers (include/jsplayer_amd.h): per axis a footprint [lo', hi') in 1/256 source pixels,
// clipped to the picture; source column x weighs its overlap with it (0 .. 256), rows likewise; each byte of the converted words is
// floor((S + (D >> 1)) / D) with S the doubly weighted sum and D = Wx * Wy the clipped footprint's area.  Its arithmetic is not written
// here: convert, Span / footprint / weight and small_quotient are present_rule_device.h's, fixed16, the geometry, the shared bounds and
// constant_byte present_rule.h's, where the index kernels (index_present_device.h) take them from too.
//
// Shape: a lane owns ONE output pixel, a workgroup kAreaLanes pixels of kAreaBandRows output rows.  A shrunk window is small and every
// pixel of it waits for a chain of loads, so the work is cut fine — 640 x 360 is 3 600 waves — and neighbouring lanes read neighbouring
// few-pixel runs of a source row.  (Four pixels a lane with 16-byte stores, display_present_kernel's shape, was measured and is 2 - 3
// times slower here, and bands of 8 rows four times: DESIGN.md §1.1.  A wave's 64 dwords are one 256-byte run either way.)  A lane's
// columns do not depend on the row and are worked out once per band; the source rows of an output row and their weights depend on
// blockIdx.y and oy alone, so they are scalar.
//   TAPS = 3 (step >> 8 <= 512, k >= 1/2) and 5 (<= 1024, k >= 1/4) — what Fit mostly is: a footprint touches TAPS columns and rows
//     at most.  The column indices (held at the last column behind it, with weight 0) and weights stay in registers, a row's
//     loads are issued side by side, and all sums fit 32 bits (S < 255 * 2^20).
//   TAPS = 0 (down to k = 1/64, 65 x 65 taps: must be right, need not be fast): first and last column times their weights, the
//     columns between them (weight 256) summed two bytes to a word; a row's weighted sum of one byte is below 2^22; the first and last
//     row of a footprint go, times their weights (512 together at most), into `edge` (< 2^31), the rows between them unweighted into
//     `mid` (63 rows at most: < 2^28); S = edge + 256 * mid (< 2^36) is 64-bit.
// The quotient (255 at most) is a float estimate, within one of the truth, put right by the 64-bit remainder.  A byte that `mode`
// makes a constant (the alpha 0xFF of the three canvas modes, the low byte 0 of c << 11) is not summed: the mean of a constant is that
// constant under the rule.  mode and TAPS are template parameters.  No LDS, no full-size converted frame.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "../../include/jsplayer_amd.h"
#include "common.h"
#include "present_rule_device.h"

namespace {

using namespace jsp::present_rule;

constexpr int kAreaLanes = 64;                         // lanes, and output pixels in x, per workgroup (one wave)
constexpr int kAreaBandRows = 1;                       // output rows a workgroup covers
// a footprint step >> 8 = s wide touches (s + 254) / 256 + 1 columns, and rows, at most: 3 up to s = 512 (k >= 1/2), 5 up to 1024 (k >= 1/4)
constexpr int kAreaNarrow3 = 512, kAreaNarrow5 = 1024;

struct AreaArgs {
    const uint32_t* src;
    uint32_t* dst;
    int fw, fh, ww, wh;
    size_t pitch;
    long long ax, ay;      // 16.16 bitmap coordinates of the centre of output pixel (0, 0)
    int step;              // 16.16 bitmap pixels per output pixel
    uint32_t bg;
};

// TAPS: 3 or 5 — the launch's promise that no footprint touches more columns or rows; 0 — any footprint
template <int MODE, int TAPS>
__global__ __launch_bounds__(kAreaLanes) void display_present_area_kernel(const AreaArgs a) {
    const int ox = (int)blockIdx.x * kAreaLanes + (int)threadIdx.x;
    if (ox >= a.ww) return;
    const int oy0 = (int)blockIdx.y * kAreaBandRows, oy1 = min(oy0 + kAreaBandRows, a.wh);
    const int s = a.step >> 8;                                 // 4 .. 16384

    // the lane's column: covered or not, and its footprint (column 0 with no weight where not covered: any valid index)
    const long long X = a.ax + (long long)ox * a.step;
    const bool in = X >= 0 && X < ((long long)a.fw << 16);
    const Span cx = in ? footprint((int)X, s, a.fw) : Span{0, 0, 0u, 0u, 1u};
    constexpr bool NARROW = TAPS > 0;
    int tx[NARROW ? TAPS : 1];
    uint32_t tw[NARROW ? TAPS : 1];
    if (NARROW) {
#pragma unroll
        for (int t = 0; t < TAPS; ++t) {
            tx[t] = min(cx.first + t, cx.last);
            tw[t] = weight(cx, cx.first + t);
        }
    }

    for (int oy = oy0; oy < oy1; ++oy) {
        const long long Y = a.ay - (long long)oy * a.step;
        uint32_t px = a.bg;
        if (Y >= 0 && Y < ((long long)a.fh << 16)) {           // (uniform, as everything about the rows)
            const Span cy = footprint((int)Y, s, a.fh);
            unsigned long long S[4];
            if (NARROW) {
                uint32_t sum[4] = {0u, 0u, 0u, 0u};
                for (int y = cy.first; y <= cy.last; ++y) {
                    const uint32_t* row = a.src + (size_t)y * a.fw;
                    const uint32_t wy = weight(cy, y);
                    uint32_t p[NARROW ? TAPS : 1];
#pragma unroll
                    for (int t = 0; t < TAPS; ++t) p[t] = convert(row[tx[t]], MODE);
#pragma unroll
                    for (int b = 0; b < 4; ++b) {
                        if (constant_byte(MODE, b)) continue;
                        uint32_t r = 0u;
#pragma unroll
                        for (int t = 0; t < TAPS; ++t) r += ((p[t] >> (8 * b)) & 0xFFu) * tw[t];
                        sum[b] += r * wy;
                    }
                }
#pragma unroll
                for (int b = 0; b < 4; ++b) S[b] = sum[b];
            } else {
                uint32_t edge[4] = {0u, 0u, 0u, 0u}, mid[4] = {0u, 0u, 0u, 0u};
                for (int y = cy.first; y <= cy.last; ++y) {
                    const uint32_t* row = a.src + (size_t)y * a.fw;
                    const bool outer = y == cy.first || y == cy.last;
                    const uint32_t wy = weight(cy, y);
                    const uint32_t pf = convert(row[cx.first], MODE), pl = convert(row[cx.last], MODE);
                    uint32_t e = 0u, o = 0u;                   // bytes 0 and 2, 1 and 3 of the columns between: 63 of 255 at most fit 16 bits
#pragma unroll 8
                    for (int x = cx.first + 1; x < cx.last; ++x) {
                        const uint32_t p = convert(row[x], MODE);
                        e += p & 0x00FF00FFu;
                        o += (p >> 8) & 0x00FF00FFu;
                    }
                    const uint32_t between[4] = {e & 0xFFFFu, o & 0xFFFFu, e >> 16, o >> 16};
#pragma unroll
                    for (int b = 0; b < 4; ++b) {
                        const uint32_t r = ((pf >> (8 * b)) & 0xFFu) * cx.wf + (between[b] << 8) + ((pl >> (8 * b)) & 0xFFu) * cx.wl;
                        if (outer) edge[b] += r * wy;
                        else mid[b] += r;
                    }
                }
#pragma unroll
                for (int b = 0; b < 4; ++b) S[b] = edge[b] + ((unsigned long long)mid[b] << 8);
            }
            const uint32_t D = cx.W * cy.W;                    // <= 2^28
            uint32_t v = constant_bits(MODE);
#pragma unroll
            for (int b = 0; b < 4; ++b)
                if (!constant_byte(MODE, b)) v |= small_quotient(S[b] + (D >> 1), D) << (8 * b);
            if (in) px = v;
        }
        __builtin_nontemporal_store(px, a.dst + (size_t)oy * a.pitch + ox);
    }
}

template <int MODE>
void launch(dim3 grid, hipStream_t s, const AreaArgs& a) {
    if ((a.step >> 8) <= kAreaNarrow3) hipLaunchKernelGGL((display_present_area_kernel<MODE, 3>), grid, dim3(kAreaLanes), 0, s, a);
    else if ((a.step >> 8) <= kAreaNarrow5) hipLaunchKernelGGL((display_present_area_kernel<MODE, 5>), grid, dim3(kAreaLanes), 0, s, a);
    else hipLaunchKernelGGL((display_present_area_kernel<MODE, 0>), grid, dim3(kAreaLanes), 0, s, a);
}

}  // namespace

extern "C" {

int jsp_display_present_area(const int32_t* frame, int frame_w, int frame_h, int32_t* out, int win_w, int win_h, size_t out_pitch,
                             double k, double dx, double dy, int mode, uint32_t background, void* hip_stream) {
    try {
        if (!frame || !out) throw std::runtime_error("null pointer");
        if (frame_w < 1 || frame_w > 16384 || frame_h < 1 || frame_h > 16384) throw std::runtime_error("frame size outside 1..16384");
        if (const char* why = window_refusal(win_w, win_h)) throw std::runtime_error(why);
        if (out_pitch < (size_t)win_w) throw std::runtime_error("out_pitch below win_w");
        if (const char* why = view_refusal(k, dx, dy, mode)) throw std::runtime_error(why);
        const Geometry g = geometry(win_h, k, dx, dy);
        AreaArgs a;
        a.src = reinterpret_cast<const uint32_t*>(frame);
        a.dst = reinterpret_cast<uint32_t*>(out);
        a.fw = frame_w; a.fh = frame_h; a.ww = win_w; a.wh = win_h;
        a.pitch = out_pitch;
        a.step = g.step; a.ax = g.ax; a.ay = g.ay;
        a.bg = background;
        const dim3 grid((unsigned)((win_w + kAreaLanes - 1) / kAreaLanes), (unsigned)((win_h + kAreaBandRows - 1) / kAreaBandRows));
        hipStream_t s = static_cast<hipStream_t>(hip_stream);
        switch (mode) {
            case JSP_DISPLAY_CANVAS: launch<JSP_DISPLAY_CANVAS>(grid, s, a); break;
            case JSP_DISPLAY_CANVAS_RGB15: launch<JSP_DISPLAY_CANVAS_RGB15>(grid, s, a); break;
            case JSP_DISPLAY_SETPIXELS: launch<JSP_DISPLAY_SETPIXELS>(grid, s, a); break;
            default: launch<JSP_DISPLAY_SETPIXELS_RGB15>(grid, s, a); break;
        }
        JSP_HIP(hipGetLastError());
        return 0;
    } catch (const std::exception& e) {
        jsp::set_error("display_present_area: %s", e.what());
        return JSP_ERROR_OCCURED;
    }
}
}
