// The arithmetic of painting mesh vertices from their views (include/dcn_hip.h section 18), stated once for the kernels of
// paint_kernels.hip.  tests/paint_common.py states the same rules in numpy, from the header's text and not from this file.
//
// As in render_raster.h and fusion_rules.h every float64 step is ONE correctly rounded IEEE operation (mul / add / quot of
// render_raster.h: the compiler may not contract them) and every other step is integer.  Pose convention, rigid inverse,
// camera-frame point and projection are rules 16(a), 16(b) and 17a.4: camera_from_pose of render_raster.h and project of
// fusion_rules.h, used as they are.
#pragma once
#include <math.h>

#include "dcn_common.h"
#include "fusion_rules.h"

namespace dcn {
namespace paint {

namespace rs = dcn::raster;
namespace fu = dcn::fusion;

constexpr int kMaxChannels = 32;

// 18a, steps 1-6 for one vertex and one frame: the pixel (py * w + px) whose value the vertex takes, -1 when the frame does not
// see it.  depth, mask (or NULL): the frame's images.
__device__ __forceinline__ int visible(const double* cam, const fu::Pinhole& k, double wx, double wy, double wz,
                                       const uint16_t* __restrict__ depth, const uint8_t* __restrict__ mask, int h, int w,
                                       double margin_mm) {
    double z;
    int pixel;
    if (!fu::project(cam, k, wx, wy, wz, h, w, z, pixel)) return -1;       // steps 1-3
    const int mm = depth[pixel];
    if (mm == 0) return -1;                                                // step 4
    const double e = rs::add(rs::mul(z, 1000.0), -(double)mm);             // step 5 (a + (-b) is a - b, one rounding)
    if (!(e >= -margin_mm && e <= margin_mm)) return -1;
    if (mask && mask[pixel] == 0) return -1;                               // step 6
    return pixel;
}

// 18a, step 7 for one channel
__device__ __forceinline__ void take(double x, double& sum, double& sumsq) {
    sum = rs::add(sum, x);
    sumsq = rs::add(sumsq, rs::mul(x, x));
}

// 18b: the mean of one channel in float64, unrounded
__device__ __forceinline__ double mean_of(double sum, int n) { return rs::quot(sum, (double)n); }

// 18b: one channel's variance; a negative result counts as 0 (a NaN stays)
__device__ __forceinline__ double variance_of(double sum, double sumsq, int n) {
    const double m = mean_of(sum, n);
    const double v = rs::add(rs::quot(sumsq, (double)n), -rs::mul(m, m));
    return v < 0.0 ? 0.0 : v;
}

// 18b: the colour byte of a float64 mean between lo and hi
__device__ __forceinline__ uint8_t colour_byte(double mean, double lo, double hi) {
    const double t = rs::quot(rs::add(mean, -lo), rs::add(hi, -lo));
    if (hi == lo || !(t == t)) return 0;
    const double clipped = t < 0.0 ? 0.0 : (t > 1.0 ? 1.0 : t);
    return (uint8_t)(int)rint(rs::mul(clipped, 255.0));                    // ties to even
}

}  // namespace paint
}  // namespace dcn
