// What msv1_index_present_kernel and sp_index_present_kernel share: a workgroup owns one rectangle of output pixels of one cell of the
// sheet, composes the source pixels the rectangle's taps or footprints reach into a 64 x 64 tile in LDS (phase 1: the codec's part, a
// functor), and every lane resamples its four output pixels from the tile (phase 2: here).
//
// THE RULE is that of jsp_display_present (filter 0 / 1) and jsp_display_present_area (filter 2), bit for bit.  Their kernels
// (display_present_kernel in present_kernels.hip, display_present_area_kernel in present_area_kernels.hip) read a frame buffer in
// global memory row by row; this one and they take the arithmetic — convert, taps, hblend, vblend, Span / footprint / weight,
// small_quotient, constant_byte — from ONE statement of it, present_rule_device.h and present_rule.h.  Here it is applied to a source
// that arrives tile by tile:
//   nearest   the one tap (X >> 16, Y >> 16), taken from the tile that holds it;
//   bilinear  the four taps, each kept (unconverted) from the tile that holds it; hblend / vblend after the last tile;
//   area      S per byte = sum of byte * wx * wy over the footprint, added up tile by tile — integer sums, so the order does not
//             matter — and floor((S + (D >> 1)) / D) after the last tile.  S < 255 * 2^20 fits 32 bits while step >> 8 <= 1024
//             (WIDE = false); beyond, S < 2^36 is kept in 64 bits (WIDE = true).
// A rectangle's source pixels usually fit ONE tile (the host sizes the rectangle so: index_present.h); where they do not — always
// for area below k of about 1/14 (MSVideo1) or 1/11 (ScreenPressor), where even 4 x 1 pixels reach 4 / k + 4 source pixels — the
// workgroup loops over the tiles of their bounding box, partial results in registers.  A pixel whose centre lies outside the picture
// is `background`; a workgroup with no centre inside composes nothing.
#pragma once
#include <hip/hip_runtime.h>

#include "index_present.h"
#include "present_rule_device.h"

namespace jsp {
namespace ipresent {
namespace {

typedef uint32_t p_u32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) uint32_t p_gu32;
typedef __attribute__((address_space(1))) p_u32x4 p_gu32x4;

constexpr int T = kIndexPresentTile;
constexpr int RUN = kIndexPresentRun;

using namespace present_rule;

// The source columns (rows) [s0, s1] that the output pixels with centres lo16 .. hi16 (16.16, both inside the picture, n wide) reach:
// the first tap of the first and the last tap of the last — taps and footprints move monotonically with the centre.
template <int FILTER>
__device__ __forceinline__ void reach(int lo16, int hi16, int step, int n, int& s0, int& s1) {
    if (FILTER == JSP_PRESENT_NEAREST) {
        s0 = lo16 >> 16;
        s1 = hi16 >> 16;
    } else if (FILTER == JSP_PRESENT_BILINEAR) {
        s0 = taps(lo16, n).t0;
        s1 = taps(hi16, n).t1;
    } else {
        s0 = footprint(lo16, step >> 8, n).first;
        s1 = footprint(hi16, step >> 8, n).last;
    }
}

// What a lane has of its workgroup's rectangle once phase 2 is over: the finished words of output pixels (ox0 .. ox0 + n - 1, oy) of the
// cell, n <= RUN; px[j] is defined for j < n (a pixel whose centre lies outside the picture holds `background`).
struct PresentLane {
    uint32_t px[RUN];
    int n, ox0, oy;
};

// The rectangle of the workgroup (blockIdx.x, blockIdx.y) of a cell: phases 1 and 2, up to the lane's finished words in `out`; false
// for a lane that has no pixel (all barriers are behind it then, too).  `tile`: T * T words of LDS.
// compose(tx0, ty0, sx0, sy0, sx1, sy1), called by every lane: fill the tile whose pixel (0, 0) is picture pixel (tx0, ty0) — both
// multiples of ALIGN — with the picture's pixels of [sx0, sx1] x [sy0, sy1] (inside the picture) that it holds; the rest of the tile
// may hold anything.  The barriers around it are here.
template <int MODE, int FILTER, bool WIDE, int ALIGN, class Compose>
__device__ __forceinline__ bool present_words(const IndexPresentArgs& a, const uint32_t* tile, Compose&& compose, PresentLane& out) {
    typedef typename std::conditional<WIDE, unsigned long long, uint32_t>::type Sum;
    const int lanes_x = a.rw / RUN;
    const int ly = (int)threadIdx.x / lanes_x, lx = (int)threadIdx.x - ly * lanes_x;
    const int rx0 = (int)blockIdx.x * a.rw, ry0 = (int)blockIdx.y * a.rh;
    const int rx1 = min(rx0 + a.rw, a.ww), ry1 = min(ry0 + a.rh, a.wh);        // the rectangle: [rx0, rx1) x [ry0, ry1), not empty
    const int ox0 = rx0 + lx * RUN, oy = ry0 + ly;
    const bool live = ly < a.rh && ox0 < rx1 && oy < ry1;
    const int n = live ? min(RUN, a.ww - ox0) : 0;
    const long long x_end = (long long)a.fw << 16, y_end = (long long)a.fh << 16;
    const int s = a.step >> 8;

    // ---- the lane's four pixels: covered or not, taps / footprints ----------------------------------------------------------------
    const long long Y = a.ay - (long long)oy * a.step;
    const bool iny = live && Y >= 0 && Y < y_end;
    bool in[RUN];
    int X16[RUN];
#pragma unroll
    for (int j = 0; j < RUN; ++j) {
        const long long X = a.ax + (long long)(ox0 + j) * a.step;
        in[j] = iny && j < n && X >= 0 && X < x_end;
        X16[j] = in[j] ? (int)X : 0;                                           // (covered: X < 2^30)
    }
    const int Y16 = iny ? (int)Y : 0;
    uint32_t px[RUN];                                                          // nearest: the result so far
    uint32_t tap[RUN][4];                                                      // bilinear: (x0, r0) (x1, r0) (x0, r1) (x1, r1), unconverted
    Sum S[RUN][4];                                                             // area: the doubly weighted sum per byte so far
    const Taps ty = taps(Y16, a.fh);
    const Span cy = footprint(Y16, s, a.fh);
#pragma unroll
    for (int j = 0; j < RUN; ++j) {
        px[j] = a.bg;
#pragma unroll
        for (int b = 0; b < 4; ++b) { tap[j][b] = 0u; S[j][b] = 0; }
    }

    // ---- the source pixels the rectangle reaches (workgroup-uniform) --------------------------------------------------------------
    const long long Xa = a.ax + (long long)rx0 * a.step, Xb = a.ax + (long long)(rx1 - 1) * a.step;      // Xa <= Xb
    const long long Yb = a.ay - (long long)ry0 * a.step, Ya = a.ay - (long long)(ry1 - 1) * a.step;      // Ya <= Yb
    if (Xb >= 0 && Xa < x_end && Yb >= 0 && Ya < y_end) {
        int sx0, sx1, sy0, sy1;
        reach<FILTER>((int)max(Xa, 0ll), (int)min(Xb, x_end - 1), a.step, a.fw, sx0, sx1);
        reach<FILTER>((int)max(Ya, 0ll), (int)min(Yb, y_end - 1), a.step, a.fh, sy0, sy1);
        for (int ty0 = sy0 & ~(ALIGN - 1); ty0 <= sy1; ty0 += T) {
            for (int tx0 = sx0 & ~(ALIGN - 1); tx0 <= sx1; tx0 += T) {
                __syncthreads();                                               // (the tile before this one has been read)
                compose(tx0, ty0, sx0, sy0, sx1, sy1);
                __syncthreads();
                auto held = [&](int x, int y) { return (unsigned)(x - tx0) < (unsigned)T && (unsigned)(y - ty0) < (unsigned)T; };
                auto at = [&](int x, int y) { return tile[(y - ty0) * T + (x - tx0)]; };
#pragma unroll
                for (int j = 0; j < RUN; ++j) {
                    if (!in[j]) continue;
                    if (FILTER == JSP_PRESENT_NEAREST) {
                        const int x = X16[j] >> 16, y = Y16 >> 16;
                        if (held(x, y)) px[j] = convert(at(x, y), MODE);
                    } else if (FILTER == JSP_PRESENT_BILINEAR) {
                        const Taps tx = taps(X16[j], a.fw);
                        if (held(tx.t0, ty.t0)) tap[j][0] = at(tx.t0, ty.t0);
                        if (held(tx.t1, ty.t0)) tap[j][1] = at(tx.t1, ty.t0);
                        if (held(tx.t0, ty.t1)) tap[j][2] = at(tx.t0, ty.t1);
                        if (held(tx.t1, ty.t1)) tap[j][3] = at(tx.t1, ty.t1);
                    } else {
                        const Span cx = footprint(X16[j], s, a.fw);
                        const int xa = max(cx.first, tx0), xb = min(cx.last, tx0 + T - 1);
                        const int ya = max(cy.first, ty0), yb = min(cy.last, ty0 + T - 1);
                        for (int y = ya; y <= yb; ++y) {
                            uint32_t r[4] = {0u, 0u, 0u, 0u};                  // a row of the tile: 64 * 255 * 256 < 2^22 per byte
                            for (int x = xa; x <= xb; ++x) {
                                const uint32_t p = convert(at(x, y), MODE), wx = weight(cx, x);
#pragma unroll
                                for (int b = 0; b < 4; ++b)
                                    if (!constant_byte(MODE, b)) r[b] += ((p >> (8 * b)) & 0xFFu) * wx;
                            }
                            const uint32_t wy = weight(cy, y);
#pragma unroll
                            for (int b = 0; b < 4; ++b) S[j][b] += (Sum)r[b] * wy;
                        }
                    }
                }
            }
        }
    }
    out.n = n;
    out.ox0 = ox0;
    out.oy = oy;
    if (!live) return false;

    // ---- finish ---------------------------------------------------------------------------------------------------------------------------
#pragma unroll
    for (int j = 0; j < RUN; ++j) {
        if (!in[j]) continue;
        if (FILTER == JSP_PRESENT_BILINEAR) {
            const uint32_t wx = taps(X16[j], a.fw).w;
            px[j] = vblend(hblend(convert(tap[j][0], MODE), convert(tap[j][1], MODE), wx),
                           hblend(convert(tap[j][2], MODE), convert(tap[j][3], MODE), wx), ty.w);
        } else if (FILTER == JSP_PRESENT_AREA) {
            const uint32_t D = footprint(X16[j], s, a.fw).W * cy.W;            // <= 2^28
            uint32_t v = constant_bits(MODE);
#pragma unroll
            for (int b = 0; b < 4; ++b)
                if (!constant_byte(MODE, b)) v |= small_quotient((unsigned long long)S[j][b] + (D >> 1), D) << (8 * b);
            px[j] = v;
        }
    }
#pragma unroll
    for (int j = 0; j < RUN; ++j) out.px[j] = px[j];
    return true;
}

// The epilogue of the present kernels: the lane's words into its cell of the sheet, 16 bytes at once where a.vec allows.
__device__ __forceinline__ void store_words(const IndexPresentArgs& a, uint32_t* cell, const PresentLane& l) {
    uint32_t* d = cell + (size_t)l.oy * a.pitch + l.ox0;
    if (a.vec && l.n == RUN) {
        __builtin_nontemporal_store(p_u32x4{l.px[0], l.px[1], l.px[2], l.px[3]}, (p_gu32x4*)d);
    } else {
#pragma unroll
        for (int j = 0; j < RUN; ++j)
            if (j < l.n) *(p_gu32*)(d + j) = l.px[j];
    }
}

// present_words, then store_words into `cell`: a present kernel's whole rectangle.
template <int MODE, int FILTER, bool WIDE, int ALIGN, class Compose>
__device__ __forceinline__ void present_rect(const IndexPresentArgs& a, uint32_t* cell, const uint32_t* tile, Compose&& compose) {
    PresentLane l;
    if (present_words<MODE, FILTER, WIDE, ALIGN>(a, tile, compose, l)) store_words(a, cell, l);
}

// ---- the epilogue of the tensor kernels (jsp_index_tensor / jsp_sp_index_tensor) ------------------------------------------------------
typedef uint32_t p_u32x2 __attribute__((ext_vector_type(2)));
typedef __attribute__((address_space(1))) p_u32x2 p_gu32x2;
typedef __attribute__((address_space(1))) uint16_t p_gu16;
typedef __attribute__((address_space(1))) uint8_t p_gu8;

// The element of byte v (0..255) of channel ch, as the bits that are stored: THE RULE of the header — the product is exact in double, so
// the fma rounds once to double as the sum does; one rounding to float; f16 / bf16 round that float to nearest-even.
template <int DTYPE>
__device__ __forceinline__ uint32_t tensor_element(const IndexTensorArgs& t, uint32_t v, int ch) {
    if (DTYPE == JSP_TENSOR_U8) return v;
    const float f = (float)__builtin_fma((double)v, (double)t.scale[ch], (double)t.bias[ch]);
    const uint32_t bits = __float_as_uint(f);
    if (DTYPE == JSP_TENSOR_F32) return bits;
    if (DTYPE == JSP_TENSOR_F16) {
        const _Float16 h = (_Float16)f;
        return (uint32_t)__builtin_bit_cast(uint16_t, h);
    }
    return (bits + 0x7FFFu + ((bits >> 16) & 1u)) >> 16;
}

// The lane's pixels as elements of cell blockIdx.z of the dense tensor, for one dtype and layout.  In both layouts they are three CHUNKS
// of four elements, each chunk consecutive in memory: NCHW — chunk c is the four pixels of plane c; NHWC — the twelve interleaved
// elements cut in three, element m = 4 c + q being channel m % 3 of pixel m / 3.  A chunk goes out in one store of 4 * esize bytes
// where t.vec says every chunk starts on such a boundary and the lane has all four pixels; element by element otherwise.
template <int DTYPE, bool NCHW>
__device__ __forceinline__ void store_elements_as(const IndexPresentArgs& a, const IndexTensorArgs& t, const PresentLane& l) {
    const size_t W = (size_t)a.ww, H = (size_t)a.wh, z = blockIdx.z;
    const size_t first = NCHW ? (z * 3 * H + (size_t)l.oy) * W + (size_t)l.ox0      // the lane's first pixel in plane 0
                              : ((z * H + (size_t)l.oy) * W + (size_t)l.ox0) * 3;   // ... its first element
    const size_t stride = NCHW ? H * W : 4;                                         // from a chunk to the next
    uint32_t w[3][4];
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int j = NCHW ? q : (4 * c + q) / 3, ch = NCHW ? c : (4 * c + q) % 3;
            w[c][q] = tensor_element<DTYPE>(t, (l.px[j] >> (8 * ch)) & 0xFFu, ch);
        }
    if (t.vec && l.n == RUN) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const size_t at = first + (size_t)c * stride;
            if (DTYPE == JSP_TENSOR_F32)
                __builtin_nontemporal_store(p_u32x4{w[c][0], w[c][1], w[c][2], w[c][3]}, (p_gu32x4*)((uint32_t*)t.out + at));
            else if (DTYPE == JSP_TENSOR_U8)
                __builtin_nontemporal_store(w[c][0] | (w[c][1] << 8) | (w[c][2] << 16) | (w[c][3] << 24), (p_gu32*)((uint8_t*)t.out + at));
            else
                __builtin_nontemporal_store(p_u32x2{w[c][0] | (w[c][1] << 16), w[c][2] | (w[c][3] << 16)}, (p_gu32x2*)((uint16_t*)t.out + at));
        }
    } else {
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                if ((NCHW ? q : (4 * c + q) / 3) >= l.n) continue;
                const size_t at = first + (size_t)c * stride + (size_t)q;
                if (DTYPE == JSP_TENSOR_F32) *(p_gu32*)((uint32_t*)t.out + at) = w[c][q];
                else if (DTYPE == JSP_TENSOR_U8) *(p_gu8*)((uint8_t*)t.out + at) = (uint8_t)w[c][q];
                else *(p_gu16*)((uint16_t*)t.out + at) = (uint16_t)w[c][q];
            }
    }
}

// dtype and layout are workgroup-uniform and are branched on ONCE, here: one straight-line epilogue per pair inside every tensor kernel,
// and no instantiation of a kernel per pair.
__device__ __forceinline__ void store_elements(const IndexPresentArgs& a, const IndexTensorArgs& t, const PresentLane& l) {
    const bool nchw = t.layout == JSP_TENSOR_NCHW;
    switch (t.dtype) {
        case JSP_TENSOR_F32: nchw ? store_elements_as<JSP_TENSOR_F32, true>(a, t, l) : store_elements_as<JSP_TENSOR_F32, false>(a, t, l); break;
        case JSP_TENSOR_F16: nchw ? store_elements_as<JSP_TENSOR_F16, true>(a, t, l) : store_elements_as<JSP_TENSOR_F16, false>(a, t, l); break;
        case JSP_TENSOR_BF16: nchw ? store_elements_as<JSP_TENSOR_BF16, true>(a, t, l) : store_elements_as<JSP_TENSOR_BF16, false>(a, t, l); break;
        default: nchw ? store_elements_as<JSP_TENSOR_U8, true>(a, t, l) : store_elements_as<JSP_TENSOR_U8, false>(a, t, l); break;
    }
}

// the cell of blockIdx.z
__device__ __forceinline__ uint32_t* sheet_cell(const IndexPresentArgs& a) {
    const unsigned z = blockIdx.z, row = z / (unsigned)a.cols, col = z - row * (unsigned)a.cols;
    return a.out + (size_t)row * (size_t)a.wh * a.pitch + (size_t)col * (size_t)a.ww;
}

// Host: f(integral_constant<int, FILTER>, bool_constant<WIDE>) for the instantiation `filter` and `step` select.
template <class F>
inline void dispatch_filter(int filter, int step, F&& f) {
    if (filter == JSP_PRESENT_NEAREST) f(std::integral_constant<int, JSP_PRESENT_NEAREST>{}, std::false_type{});
    else if (filter == JSP_PRESENT_BILINEAR) f(std::integral_constant<int, JSP_PRESENT_BILINEAR>{}, std::false_type{});
    else if ((step >> 8) <= 1024) f(std::integral_constant<int, JSP_PRESENT_AREA>{}, std::false_type{});
    else f(std::integral_constant<int, JSP_PRESENT_AREA>{}, std::true_type{});
}
template <class F>
inline void dispatch_mode(int mode, F&& f) {
    switch (mode) {
        case JSP_DISPLAY_CANVAS: f(std::integral_constant<int, JSP_DISPLAY_CANVAS>{}); break;
        case JSP_DISPLAY_CANVAS_RGB15: f(std::integral_constant<int, JSP_DISPLAY_CANVAS_RGB15>{}); break;
        case JSP_DISPLAY_SETPIXELS: f(std::integral_constant<int, JSP_DISPLAY_SETPIXELS>{}); break;
        default: f(std::integral_constant<int, JSP_DISPLAY_SETPIXELS_RGB15>{}); break;
    }
}
// the tensor kernels: `mode` is one of the two canvas conversions (index_tensor_refusal)
template <class F>
inline void dispatch_canvas_mode(int mode, F&& f) {
    if (mode == JSP_DISPLAY_CANVAS_RGB15) f(std::integral_constant<int, JSP_DISPLAY_CANVAS_RGB15>{});
    else f(std::integral_constant<int, JSP_DISPLAY_CANVAS>{});
}
inline dim3 present_grid(const IndexPresentArgs& a, int n) {
    return dim3((unsigned)((a.ww + a.rw - 1) / a.rw), (unsigned)((a.wh + a.rh - 1) / a.rh), (unsigned)n);
}

}  // namespace
}  // namespace ipresent
}  // namespace jsp
