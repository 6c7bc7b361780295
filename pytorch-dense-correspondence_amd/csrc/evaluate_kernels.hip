// Match statistics for a BATCH of image pairs (include/dcn_hip.h section 11b): every column of the reference's evaluation table
// (DCNEvaluationPandaTemplate, evaluation.py:37-63) that compute_descriptor_match_statistics (:1045-1175) fills, for all chosen
// matches of all pairs, in two launches.
//
//   pair_stats_kernel   grid (pixel tiles, pairs).  match_stats_kernel's scheme (match_kernels.hip) per pair: one work-item per
//                       pixel of res_b[p] with its descriptor in registers, the queries of THAT pair staged in LDS (their
//                       descriptors gathered from res_a[p] here), then match_search.h's keys and reductions.  Also counts the
//                       pair's non-zero mask pixels.
//                       HBM traffic: P * HW * D * 4 bytes of res_b once, plus P * HW mask bytes; with at most a few dozen
//                       queries per pair a launch per pair would be mostly launch and drain.
//   pair_rows_kernel    one work-item per row: unpacks the keys and finishes the columns; the depth / 3D half (:1102-1135,
//                       :1148-1164) in float64 from the fp32 camera row.
// The per-pixel loop and the row finishing are eval_stats.h's, shared with the grouped entry (crossscene_kernels.hip).
#include "dcn_common.h"
#include "eval_rows.h"
#include "eval_stats.h"

namespace {

using dcn::clip_round;
using dcn::pair_rows;

using dcn::kMT;
using dcn::kMaxD;
constexpr int kQT = dcn::kEvalQT;
constexpr int kCam = DCN_SAMPLE_CAM_FLOATS;

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

template <int DT>
__global__ void __launch_bounds__(kMT) pair_stats_kernel(PairStats a) {
    __shared__ dcn::EvalTile s;
    __shared__ int64_t sqa[kQT];       // query pixel in image a
    const int D = DT > 0 ? DT : a.d;
    const int p = blockIdx.y, w = a.w;
    const int64_t hw = a.hw;
    const int64_t pix = (int64_t)blockIdx.x * kMT + threadIdx.x;
    const bool in = pix < hw;
    const bool onm = in && a.mask_b[(size_t)p * hw + pix] != 0;
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
            s.sgu[threadIdx.x] = clip_round(a.u_b[r], w, rb);
            s.sgv[threadIdx.x] = clip_round(a.v_b[r], a.h, rb);
            if (rb && blockIdx.x == 0) atomicOr(a.status, rb);
        }
        __syncthreads();
        for (int i = threadIdx.x; i < qn * D; i += kMT) {
            const int q = i / D;
            s.sq[i] = resa[sqa[q] * D + (i - q * D)];
        }
        __syncthreads();
        dcn::stats_ground_truth(s, res, D, w, qn, blockIdx.x == 0, a.gt_d + lo + q0);
        __syncthreads();
        dcn::stats_scan<DT, false>(s, v, D, qn, in, onm, pix, pu, pv, a.best, a.count, a.dist_sum, a.max_rows, lo + q0);
    }
}

struct PairRows {
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
    dcn::EvalRowOut out;
    int64_t hw;
    int w, h, np, max_pair_rows;
};

__global__ void __launch_bounds__(256) pair_rows_kernel(PairRows a) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t R = a.out.max_rows;
    if (r >= R) return;
    const int p = dcn::row_owner(a.offsets, a.np, r);
    const bool mine = dcn::row_in_pair(a.offsets, a.offsets_bad, p, a.np, r, R, a.max_pair_rows);
    const unsigned long long k0 = mine ? a.best[r] : dcn::kNoKey, k1 = mine ? a.best[R + r] : dcn::kNoKey;
    int bad = 0;
    if (!mine || k0 == dcn::kNoKey || k1 == dcn::kNoKey) {  // past the last row, cut off a bad list, or no key written
        dcn::empty_row(a.out, r);
        return;
    }
    const int w = a.w, h = a.h;
    int ua = (int)a.u_a[r], va = (int)a.v_a[r];
    if (a.u_a[r] < 0 || a.u_a[r] >= w || a.v_a[r] < 0 || a.v_a[r] >= h) ua = va = 0;
    const int gu = clip_round(a.u_b[r], w, bad), gv = clip_round(a.v_b[r], h, bad);
    dcn::finish_row(a.out, r, p, k0, k1, ua, va, a.depth_a[(size_t)p * a.hw + (int64_t)va * w + ua], gu, gv,
                    a.depth_b + (size_t)p * a.hw, a.cams + (size_t)p * kCam, a.gt_d[r], a.count[r], a.count[R + r],
                    a.dist_sum[r], a.dist_sum[R + r], a.mask_pixels[p], a.hw, w);
}

}  // namespace

extern "C" size_t dcn_match_statistics_pairs_workspace(int64_t max_rows) { return dcn::stats_workspace_bytes(max_rows); }

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
    PairStats a;
    int32_t* flag;
    const int rc = dcn::prepare_stats_scratch(workspace, max_rows, closer, mask_pixels, p, status, offsets, st, a.best,
                                              a.dist_sum, a.gt_d, flag);
    if (rc != DCN_OK) return rc;
    a.count = closer;
    a.offsets_bad = flag;
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
    DCN_LAUNCH_FOR_D(d, pair_stats_kernel, grid, block, st, a);
    PairRows b;
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
    b.out.col = columns;
    b.out.is_valid = is_valid;
    b.out.pred_uv = pred_uv;
    b.out.row_pair = row_pair;
    b.out.max_rows = max_rows;
    b.hw = hw;
    b.w = w;
    b.h = h;
    b.np = p;
    b.max_pair_rows = max_pair_rows;
    hipLaunchKernelGGL(pair_rows_kernel, dim3((unsigned)dcn::ceil_div64(max_rows, 256)), dim3(256), 0, st, b);
    return dcn::check_launch();
}
