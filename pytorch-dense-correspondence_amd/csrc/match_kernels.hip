// Best-match search over a dense descriptor image ("next" row 1) -- the evaluation-side hot loop
//   norm_diffs = sqrt(sum(square(res_b - descriptor), axis=2));  argmin      (dense_correspondence_network.py:517-523, :541-547)
// which the reference runs in numpy on the CPU once per query pixel (100 full-image scans per image pair,
// evaluation.py:932-950).  Here ALL queries of an image are answered by one pass over the descriptor image:
// HBM-bound, algorithmic traffic = HW * D * 4 bytes once (+ Q * HW * 4 when the distance images are requested).
// One work-item per pixel keeps its descriptor in registers and loops over the queries (LDS broadcast reads); per query the
// packed key goes through match_search.h's reductions: the wavefront, the workgroup's wavefronts through LDS, then at most one
// 64-bit atomicMin per WORKGROUP.  That header says why the key holds the norm and why a plain load precedes the atomic.
#include "dcn_common.h"
#include "eval_stats.h"
#include "match_search.h"

namespace {

using dcn::kMT;
using dcn::kMaxD;
using dcn::kNoKey;
constexpr int kQT = dcn::kEvalQT;

template <int DT>
__global__ void __launch_bounds__(kMT)
best_match_kernel(const float* __restrict__ res, int64_t hw, int d_rt, const float* __restrict__ queries, int nq,
                  const unsigned char* __restrict__ mask, unsigned long long* __restrict__ best,
                  float* __restrict__ norm_diffs) {
    __shared__ float sq[kQT * kMaxD];
    __shared__ unsigned long long skey[kQT][kMT / 64];
    const int D = DT > 0 ? DT : d_rt;
    const int64_t pix = (int64_t)blockIdx.x * kMT + threadIdx.x;
    const bool in = pix < hw;
    const bool cand = in && (!mask || mask[pix] != 0);
    float v[DT > 0 ? DT : kMaxD];
#pragma unroll
    for (int k = 0; k < (DT > 0 ? DT : kMaxD); ++k) v[k] = (in && k < D) ? res[pix * D + k] : 0.f;
    for (int q0 = 0; q0 < nq; q0 += kQT) {
        const int qn = min(kQT, nq - q0);
        __syncthreads();
        for (int i = threadIdx.x; i < qn * D; i += kMT) sq[i] = queries[(int64_t)q0 * D + i];
        __syncthreads();
        for (int q = 0; q < qn; ++q) {
            const float dd = sqrtf(dcn::dist2<DT>(v, sq + q * D, D));
            if (norm_diffs && in) norm_diffs[(int64_t)(q0 + q) * hw + pix] = dd;
            dcn::park_key(skey[q], dcn::wave_min_key(cand ? dcn::match_key(dd, (unsigned)pix) : kNoKey));
        }
        __syncthreads();
        if ((int)threadIdx.x < qn) dcn::commit_min_key(best + q0 + threadIdx.x, dcn::block_min_key(skey[threadIdx.x]));
    }
}

__global__ void __launch_bounds__(256)
best_match_unpack_kernel(const unsigned long long* __restrict__ best, int nq, int64_t* __restrict__ idx,
                         float* __restrict__ dist) {
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= nq) return;
    const unsigned long long k = best[q];
    if (k == kNoKey) { idx[q] = -1; dist[q] = INFINITY; return; }  // empty mask
    idx[q] = (int64_t)dcn::key_pixel(k);
    dist[q] = dcn::key_norm(k);   // (already the norm, not its square)
}

// ------------------------------------------------------------------------------------------------ match statistics
// evaluation.py:1046-1100 for all query matches of an image pair in one pass over res_b.  Per query q (descriptor
// queries[q] = res_a[uv_a], ground-truth pixel gt[q] in image b):
//   best match over the image and over the mask (argmin of d, resp. of d + (1 - mask) * 1e6, first index on ties),
//   t = ||queries[q] - res_b[gt[q]]||, the number of pixels with d < t (image / mask) and the sum of their pixel distances to
//   gt[q] (for "average_l2_distance_for_false_positives").  d = sqrt(sum_k (res_b - query)^2) in fp32.
// The scan is eval_stats.h's, one text with the batched entries; no mask given: every pixel is on it, and the two halves are
// equal bit for bit.  best, dist_sum: [2][nq] in the workspace (image, masked).
template <int DT>
__global__ void __launch_bounds__(kMT)
match_stats_kernel(const float* __restrict__ res, int64_t hw, int w, int d_rt, const float* __restrict__ queries,
                   const int64_t* __restrict__ gt, int nq, const unsigned char* __restrict__ mask, unsigned long long* best,
                   int32_t* count, unsigned long long* dist_sum, float* gt_d) {
    __shared__ dcn::EvalTile s;
    const int D = DT > 0 ? DT : d_rt;
    const int64_t pix = (int64_t)blockIdx.x * kMT + threadIdx.x;
    const bool in = pix < hw;
    const bool onm = in && (!mask || mask[pix] != 0);
    const int pu = in ? (int)(pix % w) : 0, pv = in ? (int)(pix / w) : 0;
    float v[DT > 0 ? DT : kMaxD];
#pragma unroll
    for (int k = 0; k < (DT > 0 ? DT : kMaxD); ++k) v[k] = (in && k < D) ? res[pix * D + k] : 0.f;
    for (int q0 = 0; q0 < nq; q0 += kQT) {
        const int qn = min(kQT, nq - q0);
        __syncthreads();
        for (int i = threadIdx.x; i < qn * D; i += kMT) s.sq[i] = queries[(int64_t)q0 * D + i];
        if ((int)threadIdx.x < qn) {
            const int64_t g = gt[q0 + threadIdx.x];
            s.sgu[threadIdx.x] = (int)(g % w);
            s.sgv[threadIdx.x] = (int)(g / w);
        }
        __syncthreads();
        dcn::stats_ground_truth(s, res, D, w, qn, blockIdx.x == 0, gt_d + q0);
        __syncthreads();
        dcn::stats_scan<DT, false>(s, v, D, qn, in, onm, pix, pu, pv, best, count, dist_sum, nq, q0);
    }
}

__global__ void __launch_bounds__(256)
match_stats_unpack_kernel(const unsigned long long* __restrict__ best, const unsigned long long* __restrict__ sum, int nq,
                          int64_t* __restrict__ idx, float* __restrict__ dist, float* __restrict__ dist_sum) {
    const int q = blockIdx.x * 256 + threadIdx.x;   // over 2 * nq
    if (q >= 2 * nq) return;
    idx[q] = (int64_t)dcn::key_pixel(best[q]);
    dist[q] = dcn::key_norm(best[q]);   // (already the norm, not its square)
    dist_sum[q] = (float)((double)sum[q] / dcn::kEvalSumScale);
}

}  // namespace

// best [2][Q] u64 | dist_sum [2][Q] u64
extern "C" size_t dcn_match_statistics_workspace(int q) { return (size_t)(q > 0 ? q : 1) * 4 * sizeof(unsigned long long); }

// best_idx / best_dist: [2][Q] (image, masked); count: [2][Q] int32; dist_sum: [2][Q]; gt_dist: [Q].  mask may be NULL
// (then the "masked" half equals the image half, bit for bit).
extern "C" int dcn_match_statistics(const float* res, int64_t hw, int w, int d, const float* queries, const int64_t* gt_idx,
                                    int q, const unsigned char* mask, int64_t* best_idx, float* best_dist, int32_t* count,
                                    float* dist_sum, float* gt_dist, void* workspace, void* stream) {
    if (!res || !queries || !gt_idx || !best_idx || !best_dist || !count || !dist_sum || !gt_dist || !workspace || hw < 1 ||
        hw >= ((int64_t)1 << 32) || w < 1 || d < 1 || d > kMaxD || q < 1)
        return DCN_E_INVALID;
    hipStream_t st = (hipStream_t)stream;
    unsigned long long* best = (unsigned long long*)workspace;
    unsigned long long* sum = best + (size_t)q * 2;
    if (dcn::fill_bytes_async(best, 0xFF, (size_t)q * 2 * sizeof(unsigned long long), st) != DCN_OK) return DCN_E_LAUNCH;
    if (dcn::fill_bytes_async(sum, 0, (size_t)q * 2 * sizeof(unsigned long long), st) != DCN_OK) return DCN_E_LAUNCH;
    if (dcn::fill_bytes_async(count, 0, (size_t)q * 2 * sizeof(int32_t), st) != DCN_OK) return DCN_E_LAUNCH;
    const dim3 grid((unsigned)dcn::ceil_div64(hw, kMT)), block(kMT);
    DCN_LAUNCH_FOR_D(d, match_stats_kernel, grid, block, st, res, hw, w, d, queries, gt_idx, q, mask, best, count, sum, gt_dist);
    hipLaunchKernelGGL(match_stats_unpack_kernel, dim3(dcn::ceil_div(2 * q, 256)), dim3(256), 0, st,
                       (const unsigned long long*)best, (const unsigned long long*)sum, q, best_idx, best_dist, dist_sum);
    return dcn::check_launch();
}

extern "C" size_t dcn_find_best_match_workspace(int q) { return (size_t)(q > 0 ? q : 1) * sizeof(unsigned long long); }

extern "C" int dcn_find_best_match(const float* res, int64_t hw, int d, const float* queries, int q,
                                   const unsigned char* mask, int64_t* best_idx, float* best_dist, float* norm_diffs,
                                   void* workspace, void* stream) {
    if (!res || !queries || !best_idx || !best_dist || !workspace || hw < 1 || hw >= ((int64_t)1 << 32) || d < 1 ||
        d > kMaxD || q < 1)
        return DCN_E_INVALID;
    hipStream_t st = (hipStream_t)stream;
    unsigned long long* best = (unsigned long long*)workspace;
    if (dcn::fill_bytes_async(best, 0xFF, (size_t)q * sizeof(unsigned long long), st) != DCN_OK) return DCN_E_LAUNCH;
    const dim3 grid((unsigned)dcn::ceil_div64(hw, kMT)), block(kMT);
    DCN_LAUNCH_FOR_D(d, best_match_kernel, grid, block, st, res, hw, d, queries, q, mask, best, norm_diffs);
    hipLaunchKernelGGL(best_match_unpack_kernel, dim3(dcn::ceil_div(q, 256)), dim3(256), 0, st,
                       (const unsigned long long*)best, q, best_idx, best_dist);
    return dcn::check_launch();
}
