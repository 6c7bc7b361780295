// Match statistics for a BATCH of image pairs (include/dcn_hip.h section 11b): every column of the reference's evaluation table
// (DCNEvaluationPandaTemplate, evaluation.py:37-63) that compute_descriptor_match_statistics (:1045-1175) fills, for all chosen
// matches of all pairs, in two launches.
//
//   pair_stats_kernel   grid (pixel tiles, pairs).  match_stats_kernel's scheme (match_kernels.hip) per pair: one work-item per
//                       pixel of res_b[p] with its descriptor in registers, the queries of THAT pair staged in LDS (their
//                       descriptors gathered from res_a[p] here), packed-key min (norm bits << 32 | pixel: ties go to the
//                       smallest index, as np.argmin), wave64 shuffle reductions, then per workgroup and query at most one
//                       64-bit atomicMin -- after a plain load, for the reason given there: thousands of workgroups target the
//                       same few words and almost every key loses.  Also counts the pair's non-zero mask pixels.
//                       HBM traffic: P * HW * D * 4 bytes of res_b once, plus P * HW mask bytes; with at most a few dozen
//                       queries per pair a launch per pair would be mostly launch and drain.
//   pair_rows_kernel    one work-item per row: unpacks the keys and finishes the columns; the depth / 3D half (:1102-1135,
//                       :1148-1164) in float64 from the fp32 camera row.
#include "dcn_common.h"
#include "eval_rows.h"

namespace {

using dcn::check_offsets_kernel;
using dcn::pair_rows;

constexpr int kMT = 256;    // work-items (pixels) per workgroup
constexpr int kQT = 32;     // queries staged in LDS at a time
constexpr int kMaxD = 64;
constexpr int kCam = DCN_SAMPLE_CAM_FLOATS;
constexpr double kSumScale = 1048576.0;   // pixel distances are summed as integers of 2^-20 pixel: the sum does not depend on the order

struct PairStats {
    const float* res_a;            // [P][hw][D]
    const float* res_b;
    const uint8_t* mask_b;         // [P][hw]
    const int64_t* u_a;            // [rows]
    const int64_t* v_a;
    const float* u_b;
    const float* v_b;
    const int64_t* offsets;        // [P + 1]
    const int32_t* offsets_bad;    // [1] set by check_offsets_kernel
    unsigned long long* best;      // [2][R] packed (norm bits << 32 | pixel): image, masked
    int32_t* count;                // [2][R]
    unsigned long long* dist_sum;  // [2][R] sum of pixel distances in units of 2^-20 pixel
    float* gt_d;                   // [R]
    int32_t* mask_pixels;          // [P]
    int32_t* status;
    int64_t hw, max_rows;
    int w, h, d, max_pair_rows;
};

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

template <int DT>
__global__ void __launch_bounds__(kMT) pair_stats_kernel(PairStats a) {
    __shared__ float sq[kQT * kMaxD];
    __shared__ float st[kQT];          // squared ground-truth distance
    __shared__ int sgu[kQT], sgv[kQT];
    __shared__ int64_t sqa[kQT];       // query pixel in image a
    __shared__ unsigned long long skey[2][kQT][kMT / 64];
    __shared__ int scnt[2][kQT][kMT / 64];
    __shared__ unsigned long long ssum[2][kQT][kMT / 64];
    const int D = DT > 0 ? DT : a.d;
    const int p = blockIdx.y, w = a.w;
    const int64_t hw = a.hw;
    const int64_t pix = (int64_t)blockIdx.x * kMT + threadIdx.x;
    const bool in = pix < hw;
    const bool onm = in && a.mask_b[(size_t)p * hw + pix] != 0;
    const int wv = threadIdx.x >> 6;
    {   // num_pixels_in_masked_image (evaluation.py:1085)
        const int n = dcn::wave_sum<int>(onm ? 1 : 0);
        if ((threadIdx.x & 63) == 0 && n) atomicAdd(a.mask_pixels + p, n);
    }
    int bad = 0;
    int64_t lo;
    int nq;
    pair_rows(a.offsets, a.offsets_bad, p, a.max_rows, a.max_pair_rows, lo, nq, bad);
    if (bad && blockIdx.x == 0 && threadIdx.x == 0) atomicOr(a.status, bad);
    if (nq == 0) return;               // (uniform per workgroup)
    const float* res = a.res_b + (size_t)p * hw * D;
    const float* resa = a.res_a + (size_t)p * hw * D;
    const int pu = in ? (int)(pix % w) : 0, pv = in ? (int)(pix / w) : 0;
    float v[DT > 0 ? DT : kMaxD];
#pragma unroll
    for (int k = 0; k < (DT > 0 ? DT : kMaxD); ++k) v[k] = (in && k < D) ? res[pix * D + k] : 0.f;
    for (int q0 = 0; q0 < nq; q0 += kQT) {
        const int qn = min(kQT, nq - q0);
        __syncthreads();
        if ((int)threadIdx.x < qn) {
            const int64_t r = lo + q0 + threadIdx.x;
            int rb = 0;
            int64_t ua = a.u_a[r], va = a.v_a[r];
            if (ua < 0 || ua >= w || va < 0 || va >= a.h) {
                rb |= DCN_EVAL_BAD_INDEX;
                ua = va = 0;
            }
            sqa[threadIdx.x] = va * w + ua;
            sgu[threadIdx.x] = clip_round(a.u_b[r], w, rb);
            sgv[threadIdx.x] = clip_round(a.v_b[r], a.h, rb);
            if (rb && blockIdx.x == 0) atomicOr(a.status, rb);
        }
        __syncthreads();
        for (int i = threadIdx.x; i < qn * D; i += kMT) {
            const int q = i / D;
            sq[i] = resa[sqa[q] * D + (i - q * D)];
        }
        __syncthreads();
        if ((int)threadIdx.x < qn) {
            const int64_t g = (int64_t)sgv[threadIdx.x] * w + sgu[threadIdx.x];
            float t2 = 0.f;
            for (int k = 0; k < D; ++k) {
                const float t = res[g * D + k] - sq[threadIdx.x * D + k];
                t2 = fmaf(t, t, t2);
            }
            st[threadIdx.x] = t2;
            if (blockIdx.x == 0) a.gt_d[lo + q0 + threadIdx.x] = sqrtf(t2);
        }
        __syncthreads();
        for (int q = 0; q < qn; ++q) {
            float d2 = 0.f;
#pragma unroll
            for (int k = 0; k < (DT > 0 ? DT : kMaxD); ++k) {
                if (k < D) { const float t = v[k] - sq[q * D + k]; d2 = fmaf(t, t, d2); }
            }
            const float dd = sqrtf(d2), tt = sqrtf(st[q]);
            const float dm = onm ? dd : dd + 1e6f;                         // masked_norm_diffs
            unsigned long long k0 = in ? (((unsigned long long)__float_as_uint(dd)) << 32) | (unsigned)pix : ~0ull;
            unsigned long long k1 = in ? (((unsigned long long)__float_as_uint(dm)) << 32) | (unsigned)pix : ~0ull;
            const bool c0 = in && dd < tt, c1 = in && dm < tt;
            const float du = (float)(pu - sgu[q]), dv = (float)(pv - sgv[q]);
            const float pd = sqrtf(du * du + dv * dv);
            int n0 = c0 ? 1 : 0, n1 = c1 ? 1 : 0;
            const unsigned long long pf = (unsigned long long)((double)pd * kSumScale + 0.5);
            unsigned long long s0 = c0 ? pf : 0ull, s1 = c1 ? pf : 0ull;
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
                const unsigned long long x = __shfl_down(k0, off, 64), y = __shfl_down(k1, off, 64);
                k0 = x < k0 ? x : k0;
                k1 = y < k1 ? y : k1;
                n0 += __shfl_down(n0, off, 64);
                n1 += __shfl_down(n1, off, 64);
                s0 += __shfl_down(s0, off, 64);
                s1 += __shfl_down(s1, off, 64);
            }
            if ((threadIdx.x & 63) == 0) {
                skey[0][q][wv] = k0; skey[1][q][wv] = k1;
                scnt[0][q][wv] = n0; scnt[1][q][wv] = n1;
                ssum[0][q][wv] = s0; ssum[1][q][wv] = s1;
            }
        }
        __syncthreads();
        if ((int)threadIdx.x < 2 * qn) {
            const int which = threadIdx.x / qn, q = threadIdx.x - which * qn;
            unsigned long long key = skey[which][q][0];
            int n = scnt[which][q][0];
            unsigned long long s = ssum[which][q][0];
#pragma unroll
            for (int x = 1; x < kMT / 64; ++x) {
                key = skey[which][q][x] < key ? skey[which][q][x] : key;
                n += scnt[which][q][x];
                s += ssum[which][q][x];
            }
            const int64_t o = (int64_t)which * a.max_rows + lo + q0 + q;
            unsigned long long* slot = a.best + o;
            if (key != ~0ull && key < __atomic_load_n(slot, __ATOMIC_RELAXED)) atomicMin(slot, key);
            if (n) {
                atomicAdd(a.count + o, n);
                atomicAdd(a.dist_sum + o, s);
            }
        }
    }
}

struct PairRows {
    const uint8_t* mask_b;
    const uint16_t* depth_a;       // [P][hw]
    const uint16_t* depth_b;
    const float* cams;             // [P][kCam]: K, K^-1, pose a, pose b^-1
    const int64_t* u_a;
    const int64_t* v_a;
    const float* u_b;
    const float* v_b;
    const int64_t* offsets;
    const int32_t* offsets_bad;
    const unsigned long long* best;
    const int32_t* count;          // [2][R] (the `closer` output)
    const unsigned long long* dist_sum;
    const float* gt_d;
    const int32_t* mask_pixels;
    double* col;                   // [DCN_EVAL_COLUMNS][R]
    uint8_t* is_valid;             // [2][R]
    int32_t* pred_uv;              // [4][R]
    int32_t* row_pair;             // [R]
    int64_t hw, max_rows;
    int w, h, np, max_pair_rows;
};

struct Vec3 {
    double x, y, z;
};

// compute_3d_position (evaluation.py:1181-1200): pose * (z * K^-1 * (u, v, 1)); Ki = K^-1 (row-major), R / t the pose's rows
__device__ __forceinline__ Vec3 position(const double* Ki, const double* R, const double* t, int u, int v, double z) {
    const double cx = z * (Ki[0] * u + Ki[1] * v + Ki[2]);
    const double cy = z * (Ki[3] * u + Ki[4] * v + Ki[5]);
    const double cz = z * (Ki[6] * u + Ki[7] * v + Ki[8]);
    Vec3 o;
    o.x = R[0] * cx + R[1] * cy + R[2] * cz + t[0];
    o.y = R[3] * cx + R[4] * cy + R[5] * cz + t[1];
    o.z = R[6] * cx + R[7] * cy + R[8] * cz + t[2];
    return o;
}

__device__ __forceinline__ double norm3(const Vec3& a, const Vec3& b) {
    const double x = a.x - b.x, y = a.y - b.y, z = a.z - b.z;
    return sqrt(x * x + y * y + z * z);
}

__device__ __forceinline__ bool depth_valid(double d) { return d > 0.0 && d < 10.0; }   // is_depth_valid (:961-972)

__global__ void __launch_bounds__(256) pair_rows_kernel(PairRows a) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= a.max_rows) return;
    const int64_t R = a.max_rows;
    const double nan = __builtin_nan("");
    // the pair of row r: the last p with offsets[p] <= r among the pairs that have rows
    int lo = 0, hi = a.np;
    while (lo < hi) {                                       // first p with offsets[p + 1] > r
        const int mid = (lo + hi) >> 1;
        if (a.offsets[mid + 1] > r) hi = mid;
        else lo = mid + 1;
    }
    const int p = lo;
    int bad = 0;
    int64_t first = 0;
    int n = 0;
    if (p < a.np) pair_rows(a.offsets, a.offsets_bad, p, a.max_rows, a.max_pair_rows, first, n, bad);
    const bool mine = p < a.np && r >= first && r < first + n;
    const unsigned long long k0 = mine ? a.best[r] : ~0ull, k1 = mine ? a.best[R + r] : ~0ull;
    if (!mine || k0 == ~0ull || k1 == ~0ull) {              // past the last row, cut off a bad list, or no key written
#pragma unroll
        for (int c = 0; c < DCN_EVAL_COLUMNS; ++c) a.col[(int64_t)c * R + r] = nan;
        a.is_valid[r] = 0;
        a.is_valid[R + r] = 0;
#pragma unroll
        for (int c = 0; c < 4; ++c) a.pred_uv[(int64_t)c * R + r] = -1;
        a.row_pair[r] = -1;
        return;
    }
    const int w = a.w, h = a.h;
    const int i0 = (int)(unsigned)(k0 & 0xffffffffull), i1 = (int)(unsigned)(k1 & 0xffffffffull);
    const int u0 = i0 % w, v0 = i0 / w, u1 = i1 % w, v1 = i1 / w;
    int ua = (int)a.u_a[r], va = (int)a.v_a[r];
    if (a.u_a[r] < 0 || a.u_a[r] >= w || a.v_a[r] < 0 || a.v_a[r] >= h) ua = va = 0;
    const int gu = clip_round(a.u_b[r], w, bad), gv = clip_round(a.v_b[r], h, bad);
    a.row_pair[r] = p;
    a.pred_uv[r] = u0;
    a.pred_uv[R + r] = v0;
    a.pred_uv[2 * R + r] = u1;
    a.pred_uv[3 * R + r] = v1;
    a.col[(int64_t)DCN_EVAL_COL_NORM_DIFF_DESCRIPTOR_GROUND_TRUTH * R + r] = (double)a.gt_d[r];
    a.col[(int64_t)DCN_EVAL_COL_NORM_DIFF_DESCRIPTOR * R + r] = (double)__uint_as_float((unsigned)(k0 >> 32));
    a.col[(int64_t)DCN_EVAL_COL_NORM_DIFF_DESCRIPTOR_MASKED * R + r] = (double)__uint_as_float((unsigned)(k1 >> 32));
    {
        const double du = (double)(gu - u0), dv = (double)(gv - v0), dum = (double)(gu - u1), dvm = (double)(gv - v1);
        a.col[(int64_t)DCN_EVAL_COL_PIXEL_MATCH_ERROR_L2 * R + r] = sqrt(du * du + dv * dv);
        a.col[(int64_t)DCN_EVAL_COL_PIXEL_MATCH_ERROR_L2_MASKED * R + r] = sqrt(dum * dum + dvm * dvm);
        a.col[(int64_t)DCN_EVAL_COL_PIXEL_MATCH_ERROR_L1 * R + r] = fabs(du) + fabs(dv);
    }
    {
        const int c0 = a.count[r], c1 = a.count[R + r], nm = a.mask_pixels[p];
        a.col[(int64_t)DCN_EVAL_COL_FRACTION_CLOSER * R + r] = (double)c0 * 1.0 / (double)a.hw;
        a.col[(int64_t)DCN_EVAL_COL_FRACTION_CLOSER_MASKED * R + r] = nm > 0 ? (double)c1 * 1.0 / (double)nm : nan;
        a.col[(int64_t)DCN_EVAL_COL_AVERAGE_L2_FALSE_POSITIVES * R + r] = c0 ? (double)a.dist_sum[r] / kSumScale / (double)c0 : 0.0;
        a.col[(int64_t)DCN_EVAL_COL_AVERAGE_L2_FALSE_POSITIVES_MASKED * R + r] = c1 ? (double)a.dist_sum[R + r] / kSumScale / (double)c1 : 0.0;
    }
    // ---- depth / 3D half, float64
    const uint16_t* da = a.depth_a + (size_t)p * a.hw;
    const uint16_t* db = a.depth_b + (size_t)p * a.hw;
    const double za = (double)da[(int64_t)va * w + ua] / 1000.0, zb = (double)db[(int64_t)gv * w + gu] / 1000.0;
    const double z0 = (double)db[i0] / 1000.0, z1 = (double)db[i1] / 1000.0;
    const bool valid0 = depth_valid(z0), valid1 = depth_valid(z1), validb = depth_valid(zb);
    a.is_valid[r] = valid0 ? 1 : 0;
    a.is_valid[R + r] = valid1 ? 1 : 0;
    const float* cam = a.cams + (size_t)p * kCam;
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
    const Vec3 pa = position(Ki, Ra, ta, ua, va, za), pb = position(Ki, Rb, tb, gu, gv, zb);
    const Vec3 p0 = position(Ki, Rb, tb, u0, v0, z0), p1 = position(Ki, Rb, tb, u1, v1, z1);
    a.col[(int64_t)DCN_EVAL_COL_NORM_DIFF_GROUND_TRUTH_3D * R + r] = validb ? norm3(pb, pa) : nan;
    a.col[(int64_t)DCN_EVAL_COL_NORM_DIFF_PRED_3D * R + r] = (validb && valid0) ? norm3(pb, p0) : nan;
    a.col[(int64_t)DCN_EVAL_COL_NORM_DIFF_PRED_3D_MASKED * R + r] = (validb && valid1) ? norm3(pb, p1) : nan;
}

inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

}  // namespace

// best [2][R] u64 | dist_sum [2][R] u64 | gt_d [R] float | offsets_bad int32
extern "C" size_t dcn_match_statistics_pairs_workspace(int64_t max_rows) {
    const size_t r = (size_t)(max_rows > 0 ? max_rows : 1);
    return 2 * align256(r * 2 * sizeof(unsigned long long)) + align256(r * sizeof(float)) + 256;
}

extern "C" int dcn_match_statistics_pairs(int p, int h, int w, int d, const float* res_a, const float* res_b,
                                          const uint8_t* mask_b, const uint16_t* depth_a, const uint16_t* depth_b,
                                          const float* cams, const int64_t* u_a, const int64_t* v_a, const float* u_b,
                                          const float* v_b, const int64_t* offsets, int64_t max_rows, int max_pair_rows,
                                          double* columns, uint8_t* is_valid, int32_t* pred_uv, int32_t* closer,
                                          int32_t* row_pair, int32_t* mask_pixels, int32_t* status, void* workspace,
                                          void* stream) {
    const int64_t hw = (int64_t)h * w;
    if (p < 1 || p > 65535 || h < 1 || w < 1 || hw >= ((int64_t)1 << 31) || d < 1 || d > kMaxD || !res_a || !res_b || !mask_b ||
        !depth_a || !depth_b || !cams || !u_a || !v_a || !u_b || !v_b || !offsets || max_rows < 1 ||
        max_pair_rows < 1 || !columns || !is_valid || !pred_uv || !closer || !row_pair || !mask_pixels || !status || !workspace)
        return DCN_E_INVALID;
    hipStream_t st = (hipStream_t)stream;
    char* ws = (char*)workspace;
    const size_t R = (size_t)max_rows;
    PairStats a;
    a.best = (unsigned long long*)ws;
    a.dist_sum = (unsigned long long*)(ws + align256(R * 2 * sizeof(unsigned long long)));
    a.gt_d = (float*)((char*)a.dist_sum + align256(R * 2 * sizeof(unsigned long long)));
    a.count = closer;
    int32_t* flag = (int32_t*)((char*)a.gt_d + align256(R * sizeof(float)));
    a.offsets_bad = flag;
    int rc = dcn::fill_bytes_async(a.best, 0xFF, R * 2 * sizeof(unsigned long long), st);
    if (rc == DCN_OK) rc = dcn::fill_bytes_async(closer, 0, R * 2 * sizeof(int32_t), st);
    if (rc == DCN_OK) rc = dcn::fill_bytes_async(a.dist_sum, 0, R * 2 * sizeof(unsigned long long), st);
    if (rc == DCN_OK) rc = dcn::fill_bytes_async(a.gt_d, 0, align256(R * sizeof(float)), st);
    if (rc == DCN_OK) rc = dcn::fill_bytes_async(mask_pixels, 0, (size_t)p * sizeof(int32_t), st);
    if (rc == DCN_OK) rc = dcn::fill_bytes_async(status, 0, sizeof(int32_t), st);
    if (rc == DCN_OK) rc = dcn::fill_bytes_async(flag, 0, sizeof(int32_t), st);
    if (rc != DCN_OK) return rc;
    hipLaunchKernelGGL(check_offsets_kernel, dim3(dcn::ceil_div(p, 256)), dim3(256), 0, st, offsets, p, max_rows, flag, status);
    a.res_a = res_a;
    a.res_b = res_b;
    a.mask_b = mask_b;
    a.u_a = u_a;
    a.v_a = v_a;
    a.u_b = u_b;
    a.v_b = v_b;
    a.offsets = offsets;
    a.mask_pixels = mask_pixels;
    a.status = status;
    a.hw = hw;
    a.max_rows = max_rows;
    a.w = w;
    a.h = h;
    a.d = d;
    a.max_pair_rows = max_pair_rows;
    const dim3 grid((unsigned)dcn::ceil_div64(hw, kMT), (unsigned)p), block(kMT);
#define DCN_PS(DT) hipLaunchKernelGGL((pair_stats_kernel<DT>), grid, block, 0, st, a)
    switch (d) {
        case 3: DCN_PS(3); break;
        case 4: DCN_PS(4); break;
        case 8: DCN_PS(8); break;
        case 16: DCN_PS(16); break;
        case 32: DCN_PS(32); break;
        default: DCN_PS(0); break;
    }
#undef DCN_PS
    PairRows b;
    b.mask_b = mask_b;
    b.depth_a = depth_a;
    b.depth_b = depth_b;
    b.cams = cams;
    b.u_a = u_a;
    b.v_a = v_a;
    b.u_b = u_b;
    b.v_b = v_b;
    b.offsets = offsets;
    b.offsets_bad = flag;
    b.best = a.best;
    b.count = closer;
    b.dist_sum = a.dist_sum;
    b.gt_d = a.gt_d;
    b.mask_pixels = mask_pixels;
    b.col = columns;
    b.is_valid = is_valid;
    b.pred_uv = pred_uv;
    b.row_pair = row_pair;
    b.hw = hw;
    b.max_rows = max_rows;
    b.w = w;
    b.h = h;
    b.np = p;
    b.max_pair_rows = max_pair_rows;
    hipLaunchKernelGGL(pair_rows_kernel, dim3((unsigned)dcn::ceil_div64(max_rows, 256)), dim3(256), 0, st, b);
    return dcn::check_launch();
}
