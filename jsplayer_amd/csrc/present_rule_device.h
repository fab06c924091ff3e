// THE RULE of jsp_display_present / jsp_display_present_area (include/jsplayer_amd.h), the device's part, stated once for every
// kernel that applies it: display_convert_kernel (display_kernels.hip: the conversions), display_present_kernel (present_kernels.hip:
// nearest, bilinear), display_present_area_kernel (present_area_kernels.hip: area) and, through index_present_device.h, the index
// present and tensor kernels of both codecs.  How a kernel meets its source — rows of a frame in global memory, a tile in LDS — is
// its own; the arithmetic of a pixel is here.  The host's part is present_rule.h.
#pragma once
#include <hip/hip_runtime.h>

#include "present_rule.h"

namespace jsp {
namespace present_rule {

// Manager.fill_bitmap_data's four conversions (Manager.hx:325-390).  A kernel that has `mode` as a template parameter passes the
// constant: the switch folds away.
__device__ __forceinline__ uint32_t convert(uint32_t c, int mode) {
    switch (mode) {
        case JSP_DISPLAY_CANVAS: return 0xFF000000u | ((c & 0xFFu) << 16) | (c & 0xFF00u) | ((c >> 16) & 0xFFu);  // :379
        case JSP_DISPLAY_CANVAS_RGB15: return 0xFF000000u | (c << 3);                                           // :370
        case JSP_DISPLAY_SETPIXELS: return 0xFF000000u | c;                                                      // :351
        default: return c << 11;                                                                                  // :340
    }
}

// ---- bilinear ---------------------------------------------------------------------------------------------------------------------
// One axis of a covered pixel's taps: centre c16 (16.16, inside the picture: c16 < 2^30), picture size n.  t0 and t1 are the two taps
// around c16 - 32768, clamped into the picture, w the 8-bit weight of t1.
struct Taps { int t0, t1; uint32_t w; };
__device__ __forceinline__ Taps taps(int c16, int n) {
    const int U = c16 - 32768;
    const int t = U >> 16;                                     // -1 .. n - 1
    return Taps{max(t, 0), min(t + 1, n - 1), (uint32_t)(U & 0xFFFF) >> 8};
}

// p0 * (256 - w) + p1 * w for the four bytes of two converted words: bytes 0 and 2 in the halves of .e, bytes 1 and 3 in those of .o
// (a byte times 256 at most: each sum fits its 16 bits)
struct HSum { uint32_t e, o; };
__device__ __forceinline__ HSum hblend(uint32_t p0, uint32_t p1, uint32_t w) {
    const uint32_t v = 256u - w;
    return HSum{(p0 & 0x00FF00FFu) * v + (p1 & 0x00FF00FFu) * w, ((p0 >> 8) & 0x00FF00FFu) * v + ((p1 >> 8) & 0x00FF00FFu) * w};
}
// (a * (256 - w) + b * w + 32768) >> 16 for each of the four 16-bit sums of two rows: the bytes of the finished word
__device__ __forceinline__ uint32_t vblend(HSum a, HSum b, uint32_t w) {
    const uint32_t v = 256u - w;
    const uint32_t b0 = ((a.e & 0xFFFFu) * v + (b.e & 0xFFFFu) * w + 32768u) >> 16;
    const uint32_t b2 = ((a.e >> 16) * v + (b.e >> 16) * w + 32768u) >> 16;
    const uint32_t b1 = ((a.o & 0xFFFFu) * v + (b.o & 0xFFFFu) * w + 32768u) >> 16;
    const uint32_t b3 = ((a.o >> 16) * v + (b.o >> 16) * w + 32768u) >> 16;
    return b0 | (b1 << 8) | (b2 << 16) | (b3 << 24);
}

// ---- area -------------------------------------------------------------------------------------------------------------------------
// One axis of a covered pixel's footprint: centre c16 (16.16, inside the picture), s = step >> 8, picture size n.  first .. last are
// the source columns (rows) the clipped footprint [lo', hi') touches, wf and wl the weights of the two (wl = 0 where they are one:
// that column then weighs W through wf), W = hi' - lo'.
struct Span { int first, last; uint32_t wf, wl, W; };
__device__ __forceinline__ Span footprint(int c16, int s, int n) {
    const int c = c16 >> 8;                                // (covered: c16 < 2^30)
    const int lo = max(c - (s >> 1), 0);
    const int hi = min(c - (s >> 1) + s, n << 8);          // hi > lo: the centre lies in the picture and s >= 4
    Span f;
    f.first = lo >> 8;
    f.last = (hi - 1) >> 8;
    f.W = (uint32_t)(hi - lo);
    f.wf = (uint32_t)(min(hi, (f.first + 1) << 8) - lo);
    f.wl = f.last > f.first ? (uint32_t)(hi - (f.last << 8)) : 0u;
    return f;
}
// the weight of column (row) x of a footprint: wf, 256 .. 256, wl.  They add up to W <= 2^14 (s <= 16384), so a row's weighted sum of
// one byte is below 2^22, the doubly weighted sum S below 2^36, and D = Wx * Wy is 2^28 at most.
__device__ __forceinline__ uint32_t weight(const Span& f, int x) { return x == f.first ? f.wf : x < f.last ? 256u : x == f.last ? f.wl : 0u; }

// floor(n / d) for n < 2^37, 0 < d <= 2^28 and a quotient of 255 at most: the float estimate is within one of the truth, put right
// by the 64-bit remainder
__device__ __forceinline__ uint32_t small_quotient(unsigned long long n, uint32_t d) {
    uint32_t q = (uint32_t)((float)n / (float)d);
    long long r = (long long)n - (long long)((unsigned long long)q * d);
    if (r < 0) { --q; r += d; }
    if (r >= (long long)d) ++q;
    return q;
}

}  // namespace present_rule
}  // namespace jsp
