// The search and the row finishing of the match statistics, shared by the single-image entry (match_kernels.hip: queries and
// flat ground-truth indices as given), the pair-wise entry (evaluate_kernels.hip: a query's descriptor, depth and camera row come
// from image a of its pair) and the grouped entry (crossscene_kernels.hip: every row carries its own).  One text for all, so
// the entries compute the same bits for the same rows.  The search primitives (key, reductions, QueryStats) are match_search.h's.
//
//   stats_ground_truth / stats_scan   one query tile of a statistics kernel (kMT pixels x up to kEvalQT queries staged in an
//                                     EvalTile): per query one QueryStats::add, wavefront reductions, then per workgroup and
//                                     query at most one commit_min_key and one integer add per count and sum.
//   finish_row / empty_row            one row of the table from its keys, counts and sums; the depth / 3D half
//                                     (evaluation.py:1102-1135, :1148-1164) in float64 from the row's fp32 camera row.
//   stats_workspace_bytes / prepare_stats_scratch   (host) the workspace both table entries carve, its fills and the offsets check.
#pragma once
#include "dcn_common.h"
#include "eval_rows.h"
#include "match_search.h"

namespace dcn {

constexpr int kEvalQT = 32;     // queries staged in LDS at a time

// clip_pixel_to_image_size_and_round (evaluation.py:604-607): min(int(round(x)), size - 1), Python 2's round (half away from
// zero: roundf).  NaN or a negative result reads 0 and sets `bad`.
__device__ __forceinline__ int clip_round(float x, int size, int& bad) {
    if (!(x == x)) {
        bad |= DCN_EVAL_BAD_INDEX;
        return 0;
    }
    const float r = roundf(x);
    if (r < 0.f) {
        bad |= DCN_EVAL_BAD_INDEX;
        return 0;
    }
    return r >= (float)size ? size - 1 : (int)r;
}

// The LDS of one query tile: the kernel declares it __shared__, fills sq / sgu / sgv (and skip), and synchronizes
struct EvalTile {
    float sq[kEvalQT * kMaxD];         // query descriptors, [query][D]
    float st[kEvalQT];                 // squared ground-truth distance
    int sgu[kEvalQT], sgv[kEvalQT];    // ground-truth pixel in the searched image
    unsigned long long skey[2][kEvalQT][kMT / 64];
    int scnt[2][kEvalQT][kMT / 64];
    unsigned long long ssum[2][kEvalQT][kMT / 64];
    unsigned char skip[kEvalQT];       // (grouped entry) the row takes no part in the search
};

// Work-items < qn: the squared distance between query q and the searched image at q's ground truth -> s.st; the first
// workgroup of the image also stores its root at gt_d[q].  Needs s.sq, s.sgu, s.sgv; the caller synchronizes afterwards.
__device__ __forceinline__ void stats_ground_truth(EvalTile& s, const float* __restrict__ res, int D, int w, int qn,
                                                   bool first_workgroup, float* gt_d) {
    if ((int)threadIdx.x < qn) {
        const int64_t g = (int64_t)s.sgv[threadIdx.x] * w + s.sgu[threadIdx.x];
        float t2 = 0.f;
        for (int k = 0; k < D; ++k) {
            const float t = res[g * D + k] - s.sq[threadIdx.x * D + k];
            t2 = fmaf(t, t, t2);
        }
        s.st[threadIdx.x] = t2;
        if (first_workgroup) gt_d[threadIdx.x] = sqrtf(t2);
    }
}

// This work-item's pixel (descriptor v, flat index pix = pv * w + pu, `in` the image, `onm` the mask) against the tile's qn
// queries; results go to rows row0 .. row0 + qn - 1 of best / count / dist_sum ([2][max_rows]: image, masked).  SKIP: queries
// with s.skip set are passed over (uniform per workgroup) and nothing is written for them.  Needs s.st; ends after the
// atomics, the caller synchronizes before it refills the tile.
template <int DT, bool SKIP>
__device__ __forceinline__ void stats_scan(EvalTile& s, const float (&v)[DT > 0 ? DT : kMaxD], int D, int qn, bool in,
                                           bool onm, int64_t pix, int pu, int pv, unsigned long long* best, int32_t* count,
                                           unsigned long long* dist_sum, int64_t max_rows, int64_t row0) {
    const int wv = threadIdx.x >> 6;
    for (int q = 0; q < qn; ++q) {
        if (SKIP && __builtin_amdgcn_readfirstlane((int)s.skip[q])) continue;   // (one scalar branch per query)
        QueryStats t;
        t.add(in, sqrtf(dist2<DT>(v, s.sq + q * D, D)), onm, (unsigned)pix, sqrtf(s.st[q]), pu, pv, s.sgu[q], s.sgv[q]);
        // the six reductions of wave_min_key / wave_sum, step by step side by side: six independent shuffles in flight per
        // step (one after the other they cost group_stats_kernel 6 % at D = 16, profiles/match_search_refactor_bench.json)
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const unsigned long long x = __shfl_down(t.k0, off, 64), y = __shfl_down(t.k1, off, 64);
            t.k0 = x < t.k0 ? x : t.k0;
            t.k1 = y < t.k1 ? y : t.k1;
            t.n0 += __shfl_down(t.n0, off, 64);
            t.n1 += __shfl_down(t.n1, off, 64);
            t.s0 += __shfl_down(t.s0, off, 64);
            t.s1 += __shfl_down(t.s1, off, 64);
        }
        if ((threadIdx.x & 63) == 0) {
            s.skey[0][q][wv] = t.k0; s.skey[1][q][wv] = t.k1;
            s.scnt[0][q][wv] = t.n0; s.scnt[1][q][wv] = t.n1;
            s.ssum[0][q][wv] = t.s0; s.ssum[1][q][wv] = t.s1;
        }
    }
    __syncthreads();
    if ((int)threadIdx.x < 2 * qn) {
        const int which = threadIdx.x / qn, q = threadIdx.x - which * qn;
        if (!(SKIP && s.skip[q])) {
            int n = s.scnt[which][q][0];
            unsigned long long sum = s.ssum[which][q][0];
#pragma unroll
            for (int x = 1; x < kMT / 64; ++x) {
                n += s.scnt[which][q][x];
                sum += s.ssum[which][q][x];
            }
            const int64_t o = (int64_t)which * max_rows + row0 + q;
            commit_min_key(best + o, block_min_key(s.skey[which][q]));
            if (n) {
                atomicAdd(count + o, n);
                atomicAdd(dist_sum + o, sum);
            }
        }
    }
}

// The table's outputs, every row dimension max_rows
struct EvalRowOut {
    double* col;                   // [DCN_EVAL_COLUMNS][R]
    uint8_t* is_valid;             // [2][R]
    int32_t* pred_uv;              // [4][R]
    int32_t* row_pair;             // [R]
    int64_t max_rows;
};

struct EvalVec3 {
    double x, y, z;
};

// compute_3d_position (evaluation.py:1181-1200): pose * (z * K^-1 * (u, v, 1)); Ki = K^-1 (row-major), R / t the pose's rows
__device__ __forceinline__ EvalVec3 eval_position(const double* Ki, const double* R, const double* t, int u, int v, double z) {
    const double cx = z * (Ki[0] * u + Ki[1] * v + Ki[2]);
    const double cy = z * (Ki[3] * u + Ki[4] * v + Ki[5]);
    const double cz = z * (Ki[6] * u + Ki[7] * v + Ki[8]);
    EvalVec3 o;
    o.x = R[0] * cx + R[1] * cy + R[2] * cz + t[0];
    o.y = R[3] * cx + R[4] * cy + R[5] * cz + t[1];
    o.z = R[6] * cx + R[7] * cy + R[8] * cz + t[2];
    return o;
}

__device__ __forceinline__ double eval_norm3(const EvalVec3& a, const EvalVec3& b) {
    const double x = a.x - b.x, y = a.y - b.y, z = a.z - b.z;
    return sqrt(x * x + y * y + z * z);
}

__device__ __forceinline__ bool eval_depth_valid(double d) { return d > 0.0 && d < 10.0; }   // is_depth_valid (:961-972)

// A row past the last one, cut off a bad list, left out, or without a key: NaN columns, zero flags, -1
__device__ __forceinline__ void empty_row(const EvalRowOut& o, int64_t r) {
    const int64_t R = o.max_rows;
    const double nan = __builtin_nan("");
#pragma unroll
    for (int c = 0; c < DCN_EVAL_COLUMNS; ++c) o.col[(int64_t)c * R + r] = nan;
    o.is_valid[r] = 0;
    o.is_valid[R + r] = 0;
#pragma unroll
    for (int c = 0; c < 4; ++c) o.pred_uv[(int64_t)c * R + r] = -1;
    o.row_pair[r] = -1;
}

// Row r of pair / group p from its keys k0, k1 (image, masked), counts c0, c1 and distance sums s0, s1: query pixel (ua, va)
// whose depth is da_mm millimetres, ground truth (gu, gv) in the searched image, whose depth plane is db and whose mask has nm
// pixels; cam: the row's K, K^-1, pose a, pose b^-1 (fp32).
__device__ __forceinline__ void finish_row(const EvalRowOut& o, int64_t r, int p, unsigned long long k0, unsigned long long k1,
                                           int ua, int va, uint16_t da_mm, int gu, int gv, const uint16_t* __restrict__ db,
                                           const float* __restrict__ cam, float gt_d, int c0, int c1, unsigned long long s0,
                                           unsigned long long s1, int nm, int64_t hw, int w) {
    const int64_t R = o.max_rows;
    const double nan = __builtin_nan("");
    const int i0 = (int)key_pixel(k0), i1 = (int)key_pixel(k1);
    const int u0 = i0 % w, v0 = i0 / w, u1 = i1 % w, v1 = i1 / w;
    o.row_pair[r] = p;
    o.pred_uv[r] = u0;
    o.pred_uv[R + r] = v0;
    o.pred_uv[2 * R + r] = u1;
    o.pred_uv[3 * R + r] = v1;
    o.col[(int64_t)DCN_EVAL_COL_NORM_DIFF_DESCRIPTOR_GROUND_TRUTH * R + r] = (double)gt_d;
    o.col[(int64_t)DCN_EVAL_COL_NORM_DIFF_DESCRIPTOR * R + r] = (double)key_norm(k0);
    o.col[(int64_t)DCN_EVAL_COL_NORM_DIFF_DESCRIPTOR_MASKED * R + r] = (double)key_norm(k1);
    {
        const double du = (double)(gu - u0), dv = (double)(gv - v0), dum = (double)(gu - u1), dvm = (double)(gv - v1);
        o.col[(int64_t)DCN_EVAL_COL_PIXEL_MATCH_ERROR_L2 * R + r] = sqrt(du * du + dv * dv);
        o.col[(int64_t)DCN_EVAL_COL_PIXEL_MATCH_ERROR_L2_MASKED * R + r] = sqrt(dum * dum + dvm * dvm);
        o.col[(int64_t)DCN_EVAL_COL_PIXEL_MATCH_ERROR_L1 * R + r] = fabs(du) + fabs(dv);
    }
    o.col[(int64_t)DCN_EVAL_COL_FRACTION_CLOSER * R + r] = (double)c0 * 1.0 / (double)hw;
    o.col[(int64_t)DCN_EVAL_COL_FRACTION_CLOSER_MASKED * R + r] = nm > 0 ? (double)c1 * 1.0 / (double)nm : nan;
    o.col[(int64_t)DCN_EVAL_COL_AVERAGE_L2_FALSE_POSITIVES * R + r] = c0 ? (double)s0 / kEvalSumScale / (double)c0 : 0.0;
    o.col[(int64_t)DCN_EVAL_COL_AVERAGE_L2_FALSE_POSITIVES_MASKED * R + r] = c1 ? (double)s1 / kEvalSumScale / (double)c1 : 0.0;
    // ---- depth / 3D half, float64
    const double za = (double)da_mm / 1000.0, zb = (double)db[(int64_t)gv * w + gu] / 1000.0;
    const double z0 = (double)db[i0] / 1000.0, z1 = (double)db[i1] / 1000.0;
    const bool valid0 = eval_depth_valid(z0), valid1 = eval_depth_valid(z1), validb = eval_depth_valid(zb);
    o.is_valid[r] = valid0 ? 1 : 0;
    o.is_valid[R + r] = valid1 ? 1 : 0;
    double K[9], Ki[9], Ra[9], ta[3], Rb[9], tb[3];
#pragma unroll
    for (int i = 0; i < 9; ++i) K[i] = (double)cam[i];
    {   // inverse of K by its adjugate
        const double c00 = K[4] * K[8] - K[5] * K[7], c01 = K[5] * K[6] - K[3] * K[8], c02 = K[3] * K[7] - K[4] * K[6];
        const double det = K[0] * c00 + K[1] * c01 + K[2] * c02;
        Ki[0] = c00 / det;
        Ki[1] = (K[2] * K[7] - K[1] * K[8]) / det;
        Ki[2] = (K[1] * K[5] - K[2] * K[4]) / det;
        Ki[3] = c01 / det;
        Ki[4] = (K[0] * K[8] - K[2] * K[6]) / det;
        Ki[5] = (K[2] * K[3] - K[0] * K[5]) / det;
        Ki[6] = c02 / det;
        Ki[7] = (K[1] * K[6] - K[0] * K[7]) / det;
        Ki[8] = (K[0] * K[4] - K[1] * K[3]) / det;
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            Ra[3 * i + j] = (double)cam[18 + 4 * i + j];
            Rb[3 * i + j] = (double)cam[34 + 4 * j + i];                  // (R_b^-1)^T
        }
        ta[i] = (double)cam[18 + 4 * i + 3];
    }
    {
        const double t0 = (double)cam[34 + 3], t1 = (double)cam[34 + 7], t2 = (double)cam[34 + 11];
#pragma unroll
        for (int i = 0; i < 3; ++i) tb[i] = -(Rb[3 * i] * t0 + Rb[3 * i + 1] * t1 + Rb[3 * i + 2] * t2);
    }
    const EvalVec3 pa = eval_position(Ki, Ra, ta, ua, va, za), pb = eval_position(Ki, Rb, tb, gu, gv, zb);
    const EvalVec3 p0 = eval_position(Ki, Rb, tb, u0, v0, z0), p1 = eval_position(Ki, Rb, tb, u1, v1, z1);
    o.col[(int64_t)DCN_EVAL_COL_NORM_DIFF_GROUND_TRUTH_3D * R + r] = validb ? eval_norm3(pb, pa) : nan;
    o.col[(int64_t)DCN_EVAL_COL_NORM_DIFF_PRED_3D * R + r] = (validb && valid0) ? eval_norm3(pb, p0) : nan;
    o.col[(int64_t)DCN_EVAL_COL_NORM_DIFF_PRED_3D_MASKED * R + r] = (validb && valid1) ? eval_norm3(pb, p1) : nan;
}

// ---- the host half: the scratch both entries carve from their workspace
// best [2][R] u64 | dist_sum [2][R] u64 | gt_d [R] float | offsets_bad int32
inline size_t stats_workspace_bytes(int64_t max_rows) {
    const size_t r = (size_t)(max_rows > 0 ? max_rows : 1);
    return 2 * align256(r * 2 * sizeof(unsigned long long)) + align256(r * sizeof(float)) + 256;
}

// Carves `workspace` into best, dist_sum, gt_d and flag, clears them and what the search accumulates into (closer [2][R],
// mask_pixels [groups], status) and launches check_offsets_kernel over the `groups` row lists
inline int prepare_stats_scratch(void* workspace, int64_t max_rows, int32_t* closer, int32_t* mask_pixels, int groups,
                                 int32_t* status, const int64_t* offsets, hipStream_t st, unsigned long long*& best,
                                 unsigned long long*& dist_sum, float*& gt_d, int32_t*& flag) {
    char* ws = (char*)workspace;
    const size_t R = (size_t)max_rows;
    best = (unsigned long long*)ws;
    dist_sum = (unsigned long long*)(ws + align256(R * 2 * sizeof(unsigned long long)));
    gt_d = (float*)((char*)dist_sum + align256(R * 2 * sizeof(unsigned long long)));
    flag = (int32_t*)((char*)gt_d + align256(R * sizeof(float)));
    int rc = fill_bytes_async(best, 0xFF, R * 2 * sizeof(unsigned long long), st);
    if (rc == DCN_OK) rc = fill_bytes_async(closer, 0, R * 2 * sizeof(int32_t), st);
    if (rc == DCN_OK) rc = fill_bytes_async(dist_sum, 0, R * 2 * sizeof(unsigned long long), st);
    if (rc == DCN_OK) rc = fill_bytes_async(gt_d, 0, align256(R * sizeof(float)), st);
    if (rc == DCN_OK) rc = fill_bytes_async(mask_pixels, 0, (size_t)groups * sizeof(int32_t), st);
    if (rc == DCN_OK) rc = fill_bytes_async(status, 0, sizeof(int32_t), st);
    if (rc == DCN_OK) rc = fill_bytes_async(flag, 0, sizeof(int32_t), st);
    if (rc != DCN_OK) return rc;
    hipLaunchKernelGGL(check_offsets_kernel, dim3(ceil_div(groups, 256)), dim3(256), 0, st, offsets, groups, max_rows, flag,
                       status);
    return DCN_OK;
}

}  // namespace dcn
