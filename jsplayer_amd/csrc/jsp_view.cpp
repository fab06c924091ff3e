// The view geometry of the reference's Main (Main.on_stage_resize, Main.hx:301-315), in doubles: which part of a frame a window shows
// under "Fit", "100%", "200%" and the two view positions.  Pure host arithmetic: no device is touched.
#include <cmath>

#include "../../include/jsplayer_amd.h"
#include "common.h"

namespace {
double fit(double a, double mn, double mx) {   // Main.hx:282-286
    if (a < mn) return mn;
    if (a > mx) return mx;
    return a;
}
}  // namespace

extern "C" int jsp_view_matrix(int frame_w, int frame_h, int win_w, int win_h, double zoom, double hor_view_pos, double ver_view_pos,
                               double* k, double* dx, double* dy) {
#pragma clang fp contract(off)                 // every product and difference rounded on its own, as the reference's doubles are
    const char* why = nullptr;
    if (!k || !dx || !dy) why = "null output";
    else if (frame_w <= 0 || frame_h <= 0 || win_w <= 0 || win_h <= 0) why = "sizes must be positive";
    else if (!std::isfinite(zoom) || zoom < 0) why = "zoom must be finite and not negative";
    else if (!std::isfinite(hor_view_pos) || hor_view_pos < 0 || !std::isfinite(ver_view_pos) || ver_view_pos < 0) why = "view positions must be finite and not negative";
    if (why) {
        jsp::set_error("view_matrix: %s", why);
        return JSP_ERROR_OCCURED;
    }
    const double vx = frame_w, vy = frame_h, width = win_w, height = win_h;
    if (zoom == 0) {                           // "Fit"
        const double kx = width / vx, ky = height / vy;
        *k = kx < ky ? kx : ky;
        *dx = 0;
        *dy = 0;
        return 0;
    }
    *k = zoom;
    *dx = fit(vx * zoom * hor_view_pos - width / 2, 0, vx * zoom - width);
    *dy = fit(vy * zoom * (1 - ver_view_pos) - height / 2, 0, vy * zoom - height);
    return 0;
}
