// The reprojection and occlusion test of one candidate pixel (correspondence_finder.py batch_find_pixel_correspondences,
// :486-619), shared by project_kernel (pairgen_kernels.hip) and the batched sample builder (sample_kernels.hip).  fp32 in
// the reference's evaluation order (mm rows as a0*x0 + a1*x1 + a2*x2 [+ a3]); the build passes -ffp-contract=off.
#pragma once
#include "dcn_common.h"

namespace dcn {

__device__ __forceinline__ float row3(const float* m, float x, float y, float z) { return m[0] * x + m[1] * y + m[2] * z; }
__device__ __forceinline__ float row4(const float* m, float x, float y, float z) {
    return m[0] * x + m[1] * y + m[2] * z + m[3] * 1.f;
}

// Candidate (u, v) of image a: depth lookup -> unproject (K^-1) -> world (Ta) -> camera b (Tbinv) -> project (K) -> prune
// (no depth return / outside the field of view, an exactly-zero coordinate included, as `torch.nonzero` drops it /
// occluded or no return in image b, 3 mm margin).  Returns 1 when the match survives; (u2, v2) = the projection (0 when
// there is no depth in image a).
__device__ __forceinline__ unsigned char project_candidate(const unsigned short* __restrict__ depth_a,
                                                           const unsigned short* __restrict__ depth_b, int h, int w,
                                                           const float* K, const float* Kinv, const float* Ta,
                                                           const float* Tbinv, int64_t u, int64_t v, float& u2, float& v2) {
    unsigned char ok = 0;
    u2 = 0.f;
    v2 = 0.f;
    if (u >= 0 && u < w && v >= 0 && v < h) {
        const float d = (float)depth_a[v * w + u] * 1.0f / 1000.0f;
        if (d != 0.f) {
            const float fx = (float)u * d, fy = (float)v * d, fz = d;
            const float cx = row3(Kinv, fx, fy, fz), cy = row3(Kinv + 3, fx, fy, fz), cz = row3(Kinv + 6, fx, fy, fz);
            const float wx = row4(Ta, cx, cy, cz), wy = row4(Ta + 4, cx, cy, cz), wz = row4(Ta + 8, cx, cy, cz);
            const float bx = row4(Tbinv, wx, wy, wz), by = row4(Tbinv + 4, wx, wy, wz), bz = row4(Tbinv + 8, wx, wy, wz);
            const float px = row3(K, bx, by, bz), py = row3(K + 3, bx, by, bz), pz = row3(K + 6, bx, by, bz);
            u2 = px / pz;
            v2 = py / pz;
            const float ub = (float)w * 1.0f - 1e-3f, vb = (float)h * 1.0f - 1e-3f;
            // (u2 != 0) & in range, written so that NaN coordinates are rejected
            if (u2 > 0.f && u2 <= ub && v2 > 0.f && v2 <= vb) {
                const int64_t fb = (int64_t)v2 * w + (int64_t)u2;            // truncation, as `.type(LongTensor)`
                const float d2 = (float)depth_b[fb] * 1.0f / 1000.f;
                const float z2 = pz - 0.003f;
                ok = (d2 > 0.f && !(d2 < z2)) ? 1 : 0;
            }
        }
    }
    return ok;
}

}  // namespace dcn
