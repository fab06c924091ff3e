// THE RULE of jsp_display_present / jsp_display_present_area (include/jsplayer_amd.h), the host's part, stated once for every call
// that promises it — the two display calls (present_kernels.hip, present_area_kernels.hip) and, through index_present.h, the index
// present and tensor calls of both codecs: the window's fixed-point geometry, the BOUNDS they share and which bytes a mode makes
// constant.  The device's part is present_rule_device.h.  Plain C++: msv1_seek.cpp and sp_index.cpp reach it too.
#pragma once
#include <cmath>
#include <cstdint>

#include "../../include/jsplayer_amd.h"

namespace jsp {
namespace present_rule {

// F(v) = floor(v * 65536 + 0.5) as a 64-bit integer.  A value beyond +-2^62 (a far-away dx or dy) is held there: with ox * step below
// 2^36 every pixel of such a window lies outside the picture either way, so the window is the one the unbounded integer gives.
inline long long fixed16(double v) {
    const double f = std::floor(v * 65536.0 + 0.5), lim = 4611686018427387904.0;
    if (f >= lim) return 1ll << 62;
    if (f <= -lim) return -(1ll << 62);
    return (long long)f;
}

// The display matrix in 16.16: output pixel (ox, oy) has its centre at X = ax + ox * step, Y = ay - oy * step of the bitmap.
struct Geometry {
    int step;              // 16.16 bitmap pixels per output pixel
    long long ax, ay;      // 16.16 bitmap coordinates of the centre of output pixel (0, 0)
};
inline Geometry geometry(int win_h, double k, double dx, double dy) {
    Geometry g;
    g.step = (int)fixed16(1.0 / k);                            // 1024 .. 64 * 65536
    g.ax = fixed16((0.5 + dx) / k);
    g.ay = fixed16(((double)win_h + dy - 0.5) / k);
    return g;
}

// The BOUNDS every call shares, in two checks so that each call keeps the order of its refusals: the message, or null when nothing
// is wrong.
inline const char* window_refusal(int win_w, int win_h) {
    if (win_w < 1 || win_w > 16384 || win_h < 1 || win_h > 16384) return "window size outside 1..16384";
    return nullptr;
}
inline const char* view_refusal(double k, double dx, double dy, int mode) {
    if (!std::isfinite(k) || !std::isfinite(dx) || !std::isfinite(dy)) return "k, dx, dy must be finite";
    if (k < 1.0 / 64.0 || k > 64.0) return "k outside 1/64..64";
    if (mode < JSP_DISPLAY_CANVAS || mode > JSP_DISPLAY_SETPIXELS_RGB15) return "unknown mode";
    return nullptr;
}

// byte b of every converted word is the same: 0xFF in the top byte of the canvas modes, 0 in the low byte of c << 11
constexpr bool constant_byte(int mode, int b) { return mode == JSP_DISPLAY_SETPIXELS_RGB15 ? b == 0 : b == 3; }
constexpr uint32_t constant_bits(int mode) { return mode == JSP_DISPLAY_SETPIXELS_RGB15 ? 0u : 0xFF000000u; }

}  // namespace present_rule
}  // namespace jsp
