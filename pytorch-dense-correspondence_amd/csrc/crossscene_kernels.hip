// Cross-scene evaluation on the frame store (include/dcn_hip.h section 11d): what
// single_cross_scene_image_pair_quantitative_analysis (evaluation.py:610-781) runs per human-labelled match and per extra view.
//
//   reproject_kernel    one work-item per request (src frame, u, v, dst frame) over the store itself: the labelled pixel
//                       reprojected into another view, batch_find_pixel_correspondences(..., uv_a=<one pixel>).  pairgen_project.h's
//                       project_candidate on camera entries made as frame_kernels.hip's camera_row makes them (pose a in fp32;
//                       pose b^-1 from float64, left-to-right sums), so a request gets the answer dcn_eval_matches would give
//                       that candidate.  A few dozen bytes per request.
//   group_stats_kernel  grid (pixel tiles, groups).  pair_stats_kernel's scheme (evaluate_kernels.hip; the per-pixel loop IS
//                       eval_stats.h's), but group g's rows all search the ONE image res_b[g], and each row brings its own query
//                       descriptor: image b of an annotated pair is searched by its labelled rows and by every a-view's row
//                       without being copied once per row.  A row with keep == 0 is passed over.
//                       HBM traffic: G * HW * D * 4 bytes of res_b once, G * HW mask bytes, and R * D query floats per
//                       workgroup from L2.
//   wide_stats_kernel   grid (pixel strips, blocks of 256 rows, groups): the same search transposed, for groups of MANY rows
//                       (the keypoint table: every labelled image is searched by (images - 1) * keypoints rows).  A work-item
//                       holds one ROW -- its query, ground truth, two keys, two counts, two sums -- and the strip's pixels pass
//                       by all of them through an LDS tile read at one address by every lane (a broadcast, no bank conflict):
//                       no shuffle and no barrier in the inner loop, and per row and strip at most one atomic per word.  The
//                       per-(pixel, row) arithmetic is the one QueryStats::add (match_search.h) that stats_scan calls, and
//                       every accumulation is an integer one, so the two kernels write the same bits.
//   group_rows_kernel   one work-item per row: eval_stats.h's finish_row with the row's own depth and camera row.
#include "dcn_common.h"
#include "eval_rows.h"
#include "eval_stats.h"
#include "pairgen_project.h"

namespace {

using dcn::clip_round;
using dcn::pair_rows;

using dcn::kMT;
using dcn::kMaxD;
constexpr int kQT = dcn::kEvalQT;
constexpr int kCam = DCN_SAMPLE_CAM_FLOATS;

// float64 products and sums that the compiler may not contract (the rigid inverse, as frame_kernels.hip's camera_row)
#if defined(DCN_HOSTEMU_BUILD)
inline double mul_rn(double a, double b) { return a * b; }
inline double add_rn(double a, double b) { return a + b; }
#else
__device__ __forceinline__ double mul_rn(double a, double b) { return __dmul_rn(a, b); }
__device__ __forceinline__ double add_rn(double a, double b) { return __dadd_rn(a, b); }
#endif

struct Reproject {
    const uint16_t* depth;         // the store's [F][hw]
    const double* poses;           // the store's [F][16]
    const float* kcam;             // [18]: K, K^-1
    const int32_t* requests;       // [V][4]: src frame, u, v, dst frame
    uint8_t* found;                // [V]
    float* u2;                     // [V] the projection
    float* v2;
    int32_t* uv;                   // [2][V] clip_pixel_to_image_size_and_round of it (-1 when not found)
    int32_t* status;
    int64_t num_frames, hw;
    int v, h, w;
};

__global__ void __launch_bounds__(256) reproject_kernel(Reproject a) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= a.v) return;
    const int64_t fa = a.requests[4 * (size_t)i], fb = a.requests[4 * (size_t)i + 3];
    const int64_t u = a.requests[4 * (size_t)i + 1], v = a.requests[4 * (size_t)i + 2];
    unsigned char ok = 0;
    float pu = 0.f, pv = 0.f;
    if (fa < 0 || fa >= a.num_frames || fb < 0 || fb >= a.num_frames || u < 0 || u >= a.w || v < 0 || v >= a.h) {
        atomicOr(a.status, DCN_EVAL_BAD_FRAME);
    } else {
        const double* pa = a.poses + fa * 16;
        const double* pb = a.poses + fb * 16;
        float Ta[12], Tb[12];
#pragma unroll
        for (int e = 0; e < 12; ++e) Ta[e] = (float)pa[e];
#pragma unroll
        for (int r = 0; r < 3; ++r) {
#pragma unroll
            for (int c = 0; c < 3; ++c) Tb[4 * r + c] = (float)pb[4 * c + r];          // (R^T)_rc
            double s = mul_rn(pb[r], pb[3]);                                           // -(R^T t)_r, summed left to right
            s = add_rn(s, mul_rn(pb[4 + r], pb[7]));
            s = add_rn(s, mul_rn(pb[8 + r], pb[11]));
            Tb[4 * r + 3] = (float)(-s);
        }
        ok = dcn::project_candidate(a.depth + fa * a.hw, a.depth + fb * a.hw, a.h, a.w, a.kcam, a.kcam + 9, Ta, Tb, u, v, pu, pv);
    }
    int bad = 0;
    a.found[i] = ok;
    a.u2[i] = pu;
    a.v2[i] = pv;
    a.uv[i] = ok ? clip_round(pu, a.w, bad) : -1;
    a.uv[(size_t)a.v + i] = ok ? clip_round(pv, a.h, bad) : -1;
}

struct GroupStats {
    const float* res_b;            // [G][hw][D]
    const uint8_t* mask_b;         // [G][hw]
    const float* queries;          // [rows][D]
    const int64_t* u_a;            // [rows] the query pixel (only checked here)
    const int64_t* v_a;
    const float* u_b;              // [rows] ground truth in the group's image
    const float* v_b;
    const uint8_t* keep;           // [rows]
    const int64_t* offsets;        // [G + 1]
    const int32_t* offsets_bad;    // [1] set by check_offsets_kernel
    unsigned long long* best;      // [2][R] packed (norm bits << 32 | pixel): image, masked
    int32_t* count;                // [2][R]
    unsigned long long* dist_sum;  // [2][R] sum of pixel distances in units of 2^-20 pixel
    float* gt_d;                   // [R]
    int32_t* mask_pixels;          // [G]
    int32_t* status;
    int64_t hw, max_rows;
    int w, h, d, max_group_rows;
};

template <int DT>
__global__ void __launch_bounds__(kMT) group_stats_kernel(GroupStats a) {
    __shared__ dcn::EvalTile s;
    const int D = DT > 0 ? DT : a.d;
    const int g = blockIdx.y, w = a.w;
    const int64_t hw = a.hw;
    const int64_t pix = (int64_t)blockIdx.x * kMT + threadIdx.x;
    const bool in = pix < hw;
    const bool onm = in && a.mask_b[(size_t)g * hw + pix] != 0;
    {   // num_pixels_in_masked_image (evaluation.py:1085)
        const int n = dcn::wave_sum<int>(onm ? 1 : 0);
        if ((threadIdx.x & 63) == 0 && n) atomicAdd(a.mask_pixels + g, n);
    }
    int bad = 0;
    int64_t lo;
    int nq;
    pair_rows(a.offsets, a.offsets_bad, g, a.max_rows, a.max_group_rows, lo, nq, bad);
    if (bad && blockIdx.x == 0 && threadIdx.x == 0) atomicOr(a.status, bad);
    if (nq == 0) return;               // (uniform per workgroup)
    const float* res = a.res_b + (size_t)g * hw * D;
    const int pu = in ? (int)(pix % w) : 0, pv = in ? (int)(pix / w) : 0;
    float v[DT > 0 ? DT : kMaxD];
#pragma unroll
    for (int k = 0; k < (DT > 0 ? DT : kMaxD); ++k) v[k] = (in && k < D) ? res[pix * D + k] : 0.f;
    for (int q0 = 0; q0 < nq; q0 += kQT) {
        const int qn = min(kQT, nq - q0);
        __syncthreads();
        if ((int)threadIdx.x < qn) {
            const int64_t r = lo + q0 + threadIdx.x;
            const bool kept = a.keep[r] != 0;
            int rb = 0, gu = 0, gv = 0;
            if (kept) {                // (what a row left out carries is never looked at)
                if (a.u_a[r] < 0 || a.u_a[r] >= w || a.v_a[r] < 0 || a.v_a[r] >= a.h) rb |= DCN_EVAL_BAD_INDEX;
                gu = clip_round(a.u_b[r], w, rb);
                gv = clip_round(a.v_b[r], a.h, rb);
            }
            s.skip[threadIdx.x] = kept ? 0 : 1;
            s.sgu[threadIdx.x] = gu;
            s.sgv[threadIdx.x] = gv;
            if (rb && blockIdx.x == 0) atomicOr(a.status, rb);
        }
        for (int i = threadIdx.x; i < qn * D; i += kMT) s.sq[i] = a.queries[(lo + q0) * D + i];
        __syncthreads();
        dcn::stats_ground_truth(s, res, D, w, qn, blockIdx.x == 0, a.gt_d + lo + q0);
        __syncthreads();
        dcn::stats_scan<DT, true>(s, v, D, qn, in, onm, pix, pu, pv, a.best, a.count, a.dist_sum, a.max_rows, lo + q0);
    }
}

constexpr int kWR = 256;          // rows (work-items) per workgroup of the wide kernel
constexpr int kWT = 128;          // pixels per LDS tile (a quarter of it on the generic path, whose queries live in LDS too)

struct WideStats {
    GroupStats a;
    int64_t strip;                 // pixels per workgroup
};

template <int DT>
__global__ void __launch_bounds__(kWR) wide_stats_kernel(WideStats b) {
    constexpr int TP = DT > 0 ? kWT : kWT / 4;          // (72 KiB of LDS on the generic path: two workgroups per CU)
    constexpr int DM = DT > 0 ? DT : kMaxD;
    __shared__ float s_pix[TP * DM];                       // the tile's descriptors, as they lie in memory: [pixel][D]
    __shared__ unsigned char s_mask[TP];
    __shared__ float s_q[DT > 0 ? 1 : kMaxD * kWR];        // generic path: the queries as [k][work-item]
    const GroupStats& a = b.a;
    const int D = DT > 0 ? DT : a.d;
    const int g = blockIdx.z, w = a.w, tid = threadIdx.x;
    const int64_t hw = a.hw;
    const int64_t p0 = (int64_t)blockIdx.x * b.strip, p1 = p0 + b.strip < hw ? p0 + b.strip : hw;
    const uint8_t* mask = a.mask_b + (size_t)g * hw;
    if (blockIdx.y == 0) {   // num_pixels_in_masked_image (evaluation.py:1085), once per image: the first row block's strips
        int n = 0;
        for (int64_t p = p0 + tid; p < p1; p += kWR) n += mask[p] != 0 ? 1 : 0;
        n = dcn::wave_sum<int>(n);
        if ((tid & 63) == 0 && n) atomicAdd(a.mask_pixels + g, n);
    }
    int bad = 0;
    int64_t lo;
    int nq;
    pair_rows(a.offsets, a.offsets_bad, g, a.max_rows, a.max_group_rows, lo, nq, bad);
    if (bad && blockIdx.x == 0 && blockIdx.y == 0 && tid == 0) atomicOr(a.status, bad);
    const int q0 = (int)blockIdx.y * kWR;
    if (q0 >= nq) return;              // (uniform per workgroup)
    const float* res = a.res_b + (size_t)g * hw * D;
    const int64_t r = lo + q0 + tid;
    const bool active = q0 + tid < nq && a.keep[r] != 0;   // a row left out and the work-items past the group's end idle
    float q[DT > 0 ? DT : 1];
    int gu = 0, gv = 0;
    float tt = 0.f;
    if (active) {
        int rb = 0;
        if (a.u_a[r] < 0 || a.u_a[r] >= w || a.v_a[r] < 0 || a.v_a[r] >= a.h) rb |= DCN_EVAL_BAD_INDEX;
        gu = clip_round(a.u_b[r], w, rb);
        gv = clip_round(a.v_b[r], a.h, rb);
        if (rb && blockIdx.x == 0) atomicOr(a.status, rb);
        const float* qs = a.queries + (size_t)r * D;
        const float* gt = res + ((int64_t)gv * w + gu) * D;
        float t2 = 0.f;                                    // stats_ground_truth's chain
        if constexpr (DT > 0) {
#pragma unroll
            for (int k = 0; k < DT; ++k) q[k] = qs[k];
            t2 = dcn::dist2<DT>(q, gt, D);
        } else {
            for (int k = 0; k < D; ++k) {
                const float qk = qs[k];
                s_q[k * kWR + tid] = qk;                   // (read back by this work-item only: no barrier)
                const float t = gt[k] - qk;
                t2 = fmaf(t, t, t2);
            }
        }
        tt = sqrtf(t2);
        if (blockIdx.x == 0) a.gt_d[r] = tt;               // once per row
    }
    dcn::QueryStats st;
    for (int64_t t0 = p0; t0 < p1; t0 += TP) {
        const int tn = p1 - t0 < TP ? (int)(p1 - t0) : TP;
        __syncthreads();
        for (int i = tid; i < tn * D; i += kWR) s_pix[i] = res[t0 * D + i];
        if (tid < tn) s_mask[tid] = mask[t0 + tid];
        __syncthreads();
        if (!active) continue;
        int pu = (int)(t0 % w), pv = (int)(t0 / w);
        for (int p = 0; p < tn; ++p) {                     // pixel t0 + p against this work-item's row
            const bool onm = s_mask[p] != 0;               // (read with the descriptor, not after the square root)
            float d2 = 0.f;
            if constexpr (DT > 0) {
                d2 = dcn::dist2<DT>(q, s_pix + p * DT, D);
            } else {
                for (int k = 0; k < D; ++k) {
                    const float t = s_pix[p * D + k] - s_q[k * kWR + tid];
                    d2 = fmaf(t, t, d2);
                }
            }
            const float dd = sqrtf(d2);
            if (dd < tt) st.add(true, dd, onm, (unsigned)(t0 + p), tt, pu, pv, gu, gv);
            else st.offer(true, dd, onm, (unsigned)(t0 + p));              // (few pixels are closer: no float64 step)
            if (++pu == w) { pu = 0; ++pv; }
        }
    }
    if (active) {
        const int64_t o0 = r, o1 = a.max_rows + r;
        dcn::commit_min_key(a.best + o0, st.k0);
        dcn::commit_min_key(a.best + o1, st.k1);
        if (st.n0) {
            atomicAdd(a.count + o0, st.n0);
            atomicAdd(a.dist_sum + o0, st.s0);
        }
        if (st.n1) {
            atomicAdd(a.count + o1, st.n1);
            atomicAdd(a.dist_sum + o1, st.s1);
        }
    }
}

struct GroupRows {
    const uint16_t* depth_b;       // [G][hw]
    const uint16_t* depth_q;       // [rows] depth at the query pixel, millimetres
    const float* cams;             // [rows][kCam]: K, K^-1, pose a, pose b^-1
    const int64_t* u_a;
    const int64_t* v_a;
    const float* u_b;
    const float* v_b;
    const uint8_t* keep;
    const int64_t* offsets;
    const int32_t* offsets_bad;
    const unsigned long long* best;
    const int32_t* count;          // [2][R] (the `closer` output)
    const unsigned long long* dist_sum;
    const float* gt_d;
    const int32_t* mask_pixels;
    dcn::EvalRowOut out;
    int64_t hw;
    int w, h, ng, max_group_rows;
};

__global__ void __launch_bounds__(256) group_rows_kernel(GroupRows a) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t R = a.out.max_rows;
    if (r >= R) return;
    const int g = dcn::row_owner(a.offsets, a.ng, r);
    const bool mine = dcn::row_in_pair(a.offsets, a.offsets_bad, g, a.ng, r, R, a.max_group_rows) && a.keep[r] != 0;
    const unsigned long long k0 = mine ? a.best[r] : dcn::kNoKey, k1 = mine ? a.best[R + r] : dcn::kNoKey;
    int bad = 0;
    if (!mine || k0 == dcn::kNoKey || k1 == dcn::kNoKey) {  // past the last row, cut off a bad list, left out, or no key written
        dcn::empty_row(a.out, r);
        return;
    }
    const int w = a.w, h = a.h;
    int ua = (int)a.u_a[r], va = (int)a.v_a[r];
    if (a.u_a[r] < 0 || a.u_a[r] >= w || a.v_a[r] < 0 || a.v_a[r] >= h) ua = va = 0;
    const int gu = clip_round(a.u_b[r], w, bad), gv = clip_round(a.v_b[r], h, bad);
    dcn::finish_row(a.out, r, g, k0, k1, ua, va, a.depth_q[r], gu, gv, a.depth_b + (size_t)g * a.hw, a.cams + (size_t)r * kCam,
                    a.gt_d[r], a.count[r], a.count[R + r], a.dist_sum[r], a.dist_sum[R + r], a.mask_pixels[g], a.hw, w);
}

}  // namespace

extern "C" int dcn_reproject_pixels(int v, const dcn_frame_store* store, const float* kcam, const int32_t* requests,
                                    uint8_t* found, float* u2, float* v2, int32_t* uv, int32_t* status, void* stream) {
    if (v < 1 || !store || store->num_frames < 1 || store->h < 1 || store->w < 1 || !store->depth || !store->poses || !kcam ||
        !requests || !found || !u2 || !v2 || !uv || !status)
        return DCN_E_INVALID;
    hipStream_t st = (hipStream_t)stream;
    const int rc = dcn::fill_bytes_async(status, 0, sizeof(int32_t), st);
    if (rc != DCN_OK) return rc;
    Reproject a;
    a.depth = store->depth;
    a.poses = store->poses;
    a.kcam = kcam;
    a.requests = requests;
    a.found = found;
    a.u2 = u2;
    a.v2 = v2;
    a.uv = uv;
    a.status = status;
    a.num_frames = store->num_frames;
    a.hw = (int64_t)store->h * store->w;
    a.v = v;
    a.h = store->h;
    a.w = store->w;
    hipLaunchKernelGGL(reproject_kernel, dim3(dcn::ceil_div(v, 256)), dim3(256), 0, st, a);
    return dcn::check_launch();
}

extern "C" size_t dcn_match_statistics_groups_workspace(int64_t max_rows) { return dcn::stats_workspace_bytes(max_rows); }

namespace {

// The grouped statistics: the fills, the offsets check, the search (wide: wide_stats_kernel with strips of strip_pixels, 0 =
// automatic; otherwise group_stats_kernel) and group_rows_kernel
int run_groups(bool wide, int64_t strip_pixels, int g, int h, int w, int d, const float* res_b, const uint8_t* mask_b,
               const uint16_t* depth_b, const float* queries, const int64_t* u_a, const int64_t* v_a, const uint16_t* depth_q,
               const float* u_b, const float* v_b, const float* cams, const uint8_t* keep, const int64_t* offsets,
               int64_t max_rows, int max_group_rows, double* columns, uint8_t* is_valid, int32_t* pred_uv, int32_t* closer,
               int32_t* row_pair, int32_t* mask_pixels, int32_t* status, void* workspace, void* stream) {
    const int64_t hw = (int64_t)h * w;
    if (g < 1 || g > 65535 || h < 1 || w < 1 || hw >= ((int64_t)1 << 31) || d < 1 || d > kMaxD || !res_b || !mask_b || !depth_b ||
        !queries || !u_a || !v_a || !depth_q || !u_b || !v_b || !cams || !keep || !offsets || max_rows < 1 ||
        max_group_rows < 1 || !columns || !is_valid || !pred_uv || !closer || !row_pair || !mask_pixels || !status || !workspace)
        return DCN_E_INVALID;
    const int row_blocks = dcn::ceil_div64(max_group_rows, kWR);
    if (wide && (strip_pixels < 0 || row_blocks > 65535)) return DCN_E_INVALID;
    hipStream_t st = (hipStream_t)stream;
    GroupStats a;
    int32_t* flag;
    const int rc = dcn::prepare_stats_scratch(workspace, max_rows, closer, mask_pixels, g, status, offsets, st, a.best,
                                              a.dist_sum, a.gt_d, flag);
    if (rc != DCN_OK) return rc;
    a.count = closer;
    a.offsets_bad = flag;
    a.res_b = res_b;
    a.mask_b = mask_b;
    a.queries = queries;
    a.u_a = u_a;
    a.v_a = v_a;
    a.u_b = u_b;
    a.v_b = v_b;
    a.keep = keep;
    a.offsets = offsets;
    a.mask_pixels = mask_pixels;
    a.status = status;
    a.hw = hw;
    a.max_rows = max_rows;
    a.w = w;
    a.h = h;
    a.d = d;
    a.max_group_rows = max_group_rows;
    if (wide) {
        WideStats ww;
        ww.a = a;
        if (strip_pixels > 0) {
            ww.strip = strip_pixels < hw ? strip_pixels : hw;
        } else {   // about four workgroups per CU of the 256: a keypoint-sized problem (8 images x 1 row block) gets 128 strips
            const int64_t blocks = (int64_t)g * row_blocks;
            const int64_t strips = blocks >= 1024 ? 1 : dcn::ceil_div64(1024, blocks);
            int64_t sp = dcn::ceil_div64(hw, strips);
            sp = sp < 4 * kWT ? 4 * kWT : sp;              // (at least four tiles between a row's atomics)
            ww.strip = dcn::ceil_div64(sp, kWT) * kWT;
        }
        const dim3 grid((unsigned)dcn::ceil_div64(hw, ww.strip), (unsigned)row_blocks, (unsigned)g), block(kWR);
        DCN_LAUNCH_FOR_D(d, wide_stats_kernel, grid, block, st, ww);
    } else {
        const dim3 grid((unsigned)dcn::ceil_div64(hw, kMT), (unsigned)g), block(kMT);
        DCN_LAUNCH_FOR_D(d, group_stats_kernel, grid, block, st, a);
    }
    GroupRows b;
    b.depth_b = depth_b;
    b.depth_q = depth_q;
    b.cams = cams;
    b.u_a = u_a;
    b.v_a = v_a;
    b.u_b = u_b;
    b.v_b = v_b;
    b.keep = keep;
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
    b.ng = g;
    b.max_group_rows = max_group_rows;
    hipLaunchKernelGGL(group_rows_kernel, dim3((unsigned)dcn::ceil_div64(max_rows, 256)), dim3(256), 0, st, b);
    return dcn::check_launch();
}

}  // namespace

extern "C" int dcn_match_statistics_groups(int g, int h, int w, int d, const float* res_b, const uint8_t* mask_b,
                                           const uint16_t* depth_b, const float* queries, const int64_t* u_a, const int64_t* v_a,
                                           const uint16_t* depth_q, const float* u_b, const float* v_b, const float* cams,
                                           const uint8_t* keep, const int64_t* offsets, int64_t max_rows, int max_group_rows,
                                           double* columns, uint8_t* is_valid, int32_t* pred_uv, int32_t* closer,
                                           int32_t* row_pair, int32_t* mask_pixels, int32_t* status, void* workspace,
                                           void* stream) {
    return run_groups(false, 0, g, h, w, d, res_b, mask_b, depth_b, queries, u_a, v_a, depth_q, u_b, v_b, cams, keep, offsets,
                      max_rows, max_group_rows, columns, is_valid, pred_uv, closer, row_pair, mask_pixels, status, workspace,
                      stream);
}

extern "C" int dcn_match_statistics_groups_wide(int g, int h, int w, int d, const float* res_b, const uint8_t* mask_b,
                                                const uint16_t* depth_b, const float* queries, const int64_t* u_a,
                                                const int64_t* v_a, const uint16_t* depth_q, const float* u_b, const float* v_b,
                                                const float* cams, const uint8_t* keep, const int64_t* offsets, int64_t max_rows,
                                                int max_group_rows, int64_t strip_pixels, double* columns, uint8_t* is_valid,
                                                int32_t* pred_uv, int32_t* closer, int32_t* row_pair, int32_t* mask_pixels,
                                                int32_t* status, void* workspace, void* stream) {
    return run_groups(true, strip_pixels, g, h, w, d, res_b, mask_b, depth_b, queries, u_a, v_a, depth_q, u_b, v_b, cams, keep,
                      offsets, max_rows, max_group_rows, columns, is_valid, pred_uv, closer, row_pair, mask_pixels, status,
                      workspace, stream);
}
