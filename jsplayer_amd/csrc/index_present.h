// jsp_index_present / jsp_sp_index_present (include/jsplayer_amd.h): what the two calls share on the host — the sheet, the refusals and
// the output rectangle a workgroup owns; the window's fixed-point geometry and the bounds are the display calls', from
// present_rule.h.  The kernels are msv1_index_present_kernel
// (msv1_index_present_kernels.hip) and sp_index_present_kernel (sp_index_present_kernels.hip); what they share on the device is
// index_present_device.h.  Plain C++: msv1_seek.cpp and sp_index.cpp include it too.  At the end: what jsp_index_tensor and
// jsp_sp_index_tensor add to it — the tensor's arguments, refusals and size arithmetic, once for both codecs.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>

#include "../../include/jsplayer_amd.h"
#include "present_rule.h"

namespace jsp {

constexpr int kIndexPresentWG = 256;     // lanes per workgroup
constexpr int kIndexPresentTile = 64;    // a source tile in LDS: 64 x 64 unconverted pixels, 16 KiB
constexpr int kIndexPresentRun = 4;      // output pixels per lane: one 16-byte store

// One call's window and sheet, as the kernels take them.
struct IndexPresentArgs {
    uint32_t* out;
    size_t pitch;          // ints from one sheet row to the next
    int cols;              // cells per sheet row
    int fw, fh, ww, wh;    // picture and window (= cell) size
    long long ax, ay;      // 16.16 picture coordinates of the centre of a cell's pixel (0, 0)
    int step;              // 16.16 picture pixels per output pixel
    uint32_t bg;
    int rw, rh;            // the output rectangle of a workgroup: rw (a multiple of 4, <= 64) x rh pixels, (rw / 4) * rh <= 256 lanes
    int vec;               // every cell row starts on a 16-byte boundary
};

// What of the call can be refused without the codec or the index (null when nothing is wrong): the BOUNDS of the header (those of the
// display calls from present_rule.h), the sheet.
inline const char* index_present_refusal(int n, size_t out_ints, int win_w, int win_h, size_t out_pitch, int cols, double k, double dx, double dy,
                                         int mode, int filter) {
    if (n < 1 || n > 4096) return "n is outside 1..4096";
    if (const char* why = present_rule::window_refusal(win_w, win_h)) return why;
    if (const char* why = present_rule::view_refusal(k, dx, dy, mode)) return why;
    if (filter != JSP_PRESENT_NEAREST && filter != JSP_PRESENT_BILINEAR && filter != JSP_PRESENT_AREA) return "unknown filter";
    if (cols < 1) return "cols must be at least 1";
    if ((uint64_t)out_pitch / (uint64_t)win_w < (uint64_t)cols) return "out_pitch below cols * win_w";
    const uint64_t sheet_rows = ((uint64_t)n + (uint64_t)cols - 1) / (uint64_t)cols;
    // (rows * win_h <= 2^26 and cols * win_w <= out_pitch: the products below overflow only with out_pitch beyond 2^37, which no out_ints covers)
    const long double sheet = (long double)(sheet_rows * (uint64_t)win_h - 1) * (long double)out_pitch + (long double)cols * (long double)win_w;
    if ((long double)out_ints < sheet) return "out_ints is smaller than the sheet";
    return nullptr;
}

// Source pixels, per axis, that the taps or footprints of m consecutive output pixels reach at most.
inline long long index_present_reach(int m, int step, int filter) {
    const long long span = (((long long)(m - 1) * step) >> 16) + 2;   // from the first tap of the first pixel to that of the last
    if (filter == JSP_PRESENT_NEAREST) return span;
    if (filter == JSP_PRESENT_BILINEAR) return span + 1;
    return span + (step >> 16) + 2;
}

// The arguments of a validated call.  `align`: what the kernel aligns a source tile's origin down to (the codec's block size), so a
// rectangle's source pixels fit ONE tile when they reach kIndexPresentTile - align pixels at most per axis; the rectangle is the
// largest such, at least 4 x 1 (then the kernel loops over tiles).
inline IndexPresentArgs index_present_args(int32_t* out, int n, int fw, int fh, int win_w, int win_h, size_t out_pitch, int cols, double k, double dx,
                                           double dy, int filter, uint32_t background, int align) {
    IndexPresentArgs a{};
    a.out = reinterpret_cast<uint32_t*>(out);
    a.pitch = out_pitch;
    a.cols = cols;
    a.fw = fw; a.fh = fh; a.ww = win_w; a.wh = win_h;
    const present_rule::Geometry g = present_rule::geometry(win_h, k, dx, dy);
    a.step = g.step; a.ax = g.ax; a.ay = g.ay;
    a.bg = background;
    const int room = kIndexPresentTile - align;
    int m = 1;                                                           // output pixels per axis whose source fits one tile
    while (m < 64 && index_present_reach(m + 1, a.step, filter) <= room) ++m;
    const int ww4 = (win_w + 3) & ~3;
    a.rw = std::min(std::max(m & ~3, kIndexPresentRun), std::min(ww4, 64));
    a.rh = std::max(1, std::min(std::min(m, win_h), kIndexPresentWG / (a.rw / kIndexPresentRun)));
    const bool one_column = cols == 1 || n == 1;
    a.vec = ((reinterpret_cast<uintptr_t>(out) & 15) == 0 && (out_pitch & 3) == 0 && (one_column || (win_w & 3) == 0)) ? 1 : 0;
    return a;
}

// ---- jsp_index_tensor / jsp_sp_index_tensor: the same windows as a dense tensor (msv1_index_tensor_kernel, sp_index_tensor_kernel) ----

// What the tensor kernels take beside the window (IndexPresentArgs with one column of cells; its out, pitch and vec are not used).
struct IndexTensorArgs {
    void* out;
    int dtype, layout;
    int vec;               // every chunk of four elements (index_present_device.h) starts on a boundary of 4 * esize bytes
    float scale[3], bias[3];
};

inline size_t index_tensor_esize(int dtype) { return dtype == JSP_TENSOR_F32 ? 4 : dtype == JSP_TENSOR_U8 ? 1 : 2; }

// What of a tensor call can be refused without the codec or the index (null when nothing is wrong): dtype, layout, mode, the BOUNDS of
// jsp_index_present that still apply, scale and bias, the size and the alignment of `out`.
inline const char* index_tensor_refusal(int n, const void* out, size_t out_bytes, int win_w, int win_h, double k, double dx, double dy, int mode,
                                        int filter, int dtype, int layout, const float* scale, const float* bias) {
    if (dtype < JSP_TENSOR_F32 || dtype > JSP_TENSOR_U8) return "unknown dtype";
    if (layout != JSP_TENSOR_NCHW && layout != JSP_TENSOR_NHWC) return "unknown layout";
    if (mode != JSP_DISPLAY_CANVAS && mode != JSP_DISPLAY_CANVAS_RGB15) return "mode must be JSP_DISPLAY_CANVAS or JSP_DISPLAY_CANVAS_RGB15";
    if (const char* why = index_present_refusal(n, SIZE_MAX, win_w, win_h, (size_t)std::max(win_w, 1), 1, k, dx, dy, mode, filter)) return why;
    if (dtype != JSP_TENSOR_U8) {
        if (!scale || !bias) return "scale and bias are required for a float dtype";
        for (int ch = 0; ch < 3; ++ch)
            if (!std::isfinite(scale[ch]) || !std::isfinite(bias[ch])) return "scale and bias must be finite";
    }
    // (n <= 2^12, win_w and win_h <= 2^14, esize <= 4: below 2^44)
    const uint64_t bytes = (uint64_t)n * 3u * (uint64_t)win_h * (uint64_t)win_w * (uint64_t)index_tensor_esize(dtype);
    if ((uint64_t)out_bytes < bytes) return "out_bytes is smaller than the tensor";
    if (reinterpret_cast<uintptr_t>(out) % index_tensor_esize(dtype) != 0) return "out is not aligned to its element";
    return nullptr;
}

// The arguments of a validated tensor call; the window's come from index_present_args(nullptr, n, ..., out_pitch = win_w, cols = 1, ...).
inline IndexTensorArgs index_tensor_args(void* out, int win_w, int dtype, int layout, const float* scale, const float* bias) {
    IndexTensorArgs t{};
    t.out = out;
    t.dtype = dtype;
    t.layout = layout;
    t.vec = ((win_w & 3) == 0 && reinterpret_cast<uintptr_t>(out) % (4 * index_tensor_esize(dtype)) == 0) ? 1 : 0;
    for (int ch = 0; ch < 3; ++ch) {
        t.scale[ch] = dtype == JSP_TENSOR_U8 ? 1.0f : scale[ch];
        t.bias[ch] = dtype == JSP_TENSOR_U8 ? 0.0f : bias[ch];
    }
    return t;
}

}  // namespace jsp
