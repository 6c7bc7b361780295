// The arithmetic of the depth renderer (include/dcn_hip.h section 16), stated once: every kernel path of render_kernels.hip
// -- one work-item per small triangle, a screen tile per workgroup for the large ones -- goes through setup() and shade() below,
// so a pixel's value does not depend on the path that drew it.  tests/render_common.py states the same rules in numpy, from the
// header's text and not from this file.
//
// Every float64 step is ONE correctly rounded IEEE operation (products and sums the compiler may not contract, as
// frame_kernels.hip's camera_row and crossscene_kernels.hip write the rigid inverse), every other step is integer:
//   (a) world-to-camera = the rigid inverse of the camera-to-world pose: rows (R^T | -R^T t), the translation summed left to right
//   (b) camera-frame vertex: ((a0 * x + a1 * y) + a2 * z) + a3 per row
//   (c) a triangle with a vertex that is not at z >= z_near is dropped whole (NEAR); nothing is clipped
//   (d) u = (fx * x) / z + cx, v = (fy * y) / z + cy, snapped to 1/256 pixel: rint(u * 256) with ties to even; a triangle with a
//       snapped coordinate outside +-2^30 (2^22 pixels; NaN and infinity included) is dropped whole (GUARD)
//   (e) coverage of the pixel centre (256 px + 128, 256 py + 128) by three int64 edge functions, top-left fill rule; a triangle
//       of negative area has two vertices exchanged first (both windings draw), one of zero area is skipped
//   (f) z = (E0 + E1 + E2) / ((E0 / z0 + E1 / z1) + E2 / z2), the integers converted to float64 first (ties to even);
//       z = z0 when z0 == z1 == z2
//   (g) mm = trunc(z * 1000); a fragment with mm == 0 or mm >= 65536 leaves the pixel alone
//   (h) the pixel keeps the minimum mm: an unsigned 32-bit atomicMin, whatever the order
// Ranges: |x|, |y| <= 2^30 and the centre inside 2^14 pixels keep every edge function and the doubled area below 2^63.
#pragma once
#include <math.h>

#include "dcn_common.h"

namespace dcn {
namespace raster {

#if defined(DCN_HOSTEMU_BUILD)
inline double mul(double a, double b) { return a * b; }
inline double add(double a, double b) { return a + b; }
inline double quot(double a, double b) { return a / b; }
inline double from_int(int64_t a) { return (double)a; }
#else
__device__ __forceinline__ double mul(double a, double b) { return __dmul_rn(a, b); }
__device__ __forceinline__ double add(double a, double b) { return __dadd_rn(a, b); }
__device__ __forceinline__ double quot(double a, double b) { return __ddiv_rn(a, b); }
__device__ __forceinline__ double from_int(int64_t a) { return __ll2double_rn((long long)a); }
#endif

constexpr int kSubpixel = 256;                    // snapped units per pixel
constexpr double kGuard = 1073741824.0;           // 2^30 snapped units = 2^22 pixels
constexpr int kMaxSide = 16384;                   // h, w at most

enum Verdict { kDraw = 0, kNear = 1, kOutside = 2, kNoArea = 3 };

struct Camera {
    double a[12];                                 // world-to-camera, rows of (R^T | -R^T t)
    double fx, fy, cx, cy, z_near;
};

struct Tri {                                      // snapped vertices, positive doubled area, camera-frame depths
    int64_t x0, y0, x1, y1, x2, y2;
    double z0, z1, z2;
};

// (a): pose float [16] row-major camera-to-world
__device__ __forceinline__ void camera_from_pose(const float* __restrict__ pose, Camera& c) {
    double p[12];
#pragma unroll
    for (int e = 0; e < 12; ++e) p[e] = (double)pose[e];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int k = 0; k < 3; ++k) c.a[4 * i + k] = p[4 * k + i];
        double s = mul(p[i], p[3]);
        s = add(s, mul(p[4 + i], p[7]));
        s = add(s, mul(p[8 + i], p[11]));
        c.a[4 * i + 3] = -s;
    }
}

// (b)
__device__ __forceinline__ double camera_coord(const double* row, double x, double y, double z) {
    return add(add(add(mul(row[0], x), mul(row[1], y)), mul(row[2], z)), row[3]);
}

// (d): false when the snapped coordinate is outside the guard band
__device__ __forceinline__ bool snap(double f, double x, double z, double c, int64_t& out) {
    const double s = rint(mul(add(quot(mul(f, x), z), c), (double)kSubpixel));
    const bool ok = fabs(s) <= kGuard;            // (false for NaN)
    out = ok ? (int64_t)s : 0;
    return ok;
}

// (e): the edge function of a -> b at p
__device__ __forceinline__ int64_t edge(int64_t ax, int64_t ay, int64_t bx, int64_t by, int64_t px, int64_t py) {
    return (bx - ax) * (py - ay) - (by - ay) * (px - ax);
}

// (a)-(e): the triangle of three world-frame vertices (float [3] each) as the camera sees it
__device__ __forceinline__ int setup(const Camera& c, const float* __restrict__ v0, const float* __restrict__ v1,
                                     const float* __restrict__ v2, Tri& t) {
    const float* v[3] = {v0, v1, v2};
    double cx[3], cy[3], cz[3];
    bool near = false;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const double x = (double)v[i][0], y = (double)v[i][1], z = (double)v[i][2];
        cx[i] = camera_coord(c.a, x, y, z);
        cy[i] = camera_coord(c.a + 4, x, y, z);
        cz[i] = camera_coord(c.a + 8, x, y, z);
        near = near || !(cz[i] >= c.z_near);
    }
    if (near) return kNear;
    int64_t sx[3], sy[3];
    bool inside = true;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const bool okx = snap(c.fx, cx[i], cz[i], c.cx, sx[i]);
        const bool oky = snap(c.fy, cy[i], cz[i], c.cy, sy[i]);
        inside = inside && okx && oky;
    }
    if (!inside) return kOutside;
    const int64_t area = edge(sx[0], sy[0], sx[1], sy[1], sx[2], sy[2]);
    if (area == 0) return kNoArea;
    const bool flip = area < 0;                   // exchange vertices 1 and 2
    t.x0 = sx[0];
    t.y0 = sy[0];
    t.z0 = cz[0];
    t.x1 = flip ? sx[2] : sx[1];
    t.y1 = flip ? sy[2] : sy[1];
    t.z1 = flip ? cz[2] : cz[1];
    t.x2 = flip ? sx[1] : sx[2];
    t.y2 = flip ? sy[1] : sy[2];
    t.z2 = flip ? cz[1] : cz[2];
    return kDraw;
}

// The pixels whose centres can lie inside the triangle, clipped to the image: empty when x1 < x0 or y1 < y0
struct Box {
    int x0, y0, x1, y1;
};
__device__ __forceinline__ int64_t min3(int64_t a, int64_t b, int64_t c) { return a < b ? (a < c ? a : c) : (b < c ? b : c); }
__device__ __forceinline__ int64_t max3(int64_t a, int64_t b, int64_t c) { return a > b ? (a > c ? a : c) : (b > c ? b : c); }
__device__ __forceinline__ Box box_of(const Tri& t, int h, int w) {
    // centre 256 p + 128 in [lo, hi]  <=>  ceil((lo - 128) / 256) <= p <= floor((hi - 128) / 256); >> 8 is the floor
    const int64_t half = kSubpixel / 2;
    int64_t x0 = (min3(t.x0, t.x1, t.x2) - half + (kSubpixel - 1)) >> 8, x1 = (max3(t.x0, t.x1, t.x2) - half) >> 8;
    int64_t y0 = (min3(t.y0, t.y1, t.y2) - half + (kSubpixel - 1)) >> 8, y1 = (max3(t.y0, t.y1, t.y2) - half) >> 8;
    Box b;
    b.x0 = (int)(x0 < 0 ? 0 : (x0 > w ? w : x0));
    b.y0 = (int)(y0 < 0 ? 0 : (y0 > h ? h : y0));
    b.x1 = (int)(x1 >= w ? w - 1 : (x1 < -1 ? -1 : x1));
    b.y1 = (int)(y1 >= h ? h - 1 : (y1 < -1 ? -1 : y1));
    return b;
}

// Top-left rule for a triangle of positive area in this orientation (y down): an edge a -> b owns the centres on it when it
// runs upwards (the triangle is to its right: a left edge) or level towards larger x (the triangle is below: a top edge)
__device__ __forceinline__ bool covers(int64_t e, int64_t ax, int64_t ay, int64_t bx, int64_t by) {
    const int64_t dx = bx - ax, dy = by - ay;
    return e > 0 || (e == 0 && (dy < 0 || (dy == 0 && dx > 0)));
}

// (e)-(g): is the centre of pixel (px, py) covered, and by which millimetre value
__device__ __forceinline__ bool shade(const Tri& t, int px, int py, unsigned& mm) {
    const int64_t cx = (int64_t)kSubpixel * px + kSubpixel / 2, cy = (int64_t)kSubpixel * py + kSubpixel / 2;
    const int64_t e0 = edge(t.x1, t.y1, t.x2, t.y2, cx, cy);
    const int64_t e1 = edge(t.x2, t.y2, t.x0, t.y0, cx, cy);
    const int64_t e2 = edge(t.x0, t.y0, t.x1, t.y1, cx, cy);
    if (!(covers(e0, t.x1, t.y1, t.x2, t.y2) && covers(e1, t.x2, t.y2, t.x0, t.y0) && covers(e2, t.x0, t.y0, t.x1, t.y1)))
        return false;
    double z = t.z0;                              // a triangle facing the camera: its depth as it is
    if (!(t.z0 == t.z1 && t.z1 == t.z2)) {
        const double s = add(add(quot(from_int(e0), t.z0), quot(from_int(e1), t.z1)), quot(from_int(e2), t.z2));
        z = quot(from_int(e0 + e1 + e2), s);
    }
    const double q = mul(z, 1000.0);
    if (!(q >= 1.0 && q < 65536.0)) return false;
    mm = (unsigned)q;                             // truncation
    return true;
}

}  // namespace raster
}  // namespace dcn
