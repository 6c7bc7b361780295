// Across-object evaluation for a BATCH of image pairs (include/dcn_hip.h section 11c): what
// single_across_object_image_pair_quantitative_analysis (evaluation.py:784-859) does per pair on the host --
// random_sample_from_masked_image (correspondence_finder.py:68-90) on mask a, then find_best_match
// (dense_correspondence_network.py:488-550) over the WHOLE of image b for every sampled pixel -- for all pairs at once.
//
// Queries (dcn_across_object_queries):
//   mask_count_kernel    grid (runs of kSegsPerBlock segments, pairs).  A wavefront counts the non-zero pixels of a segment
//                        of kSeg pixels (coalesced byte loads) into seg_count[p][segment]; per pair the total goes to
//                        mask_pixels[p] with integer atomics.
//   across_pick_kernel   one workgroup of 1024 per pair.  offsets from all pairs' totals (every workgroup derives its own
//                        base; workgroup 0 writes them), the tail of the outputs' capacity, then for a pair with rows: the
//                        exclusive prefix of its segment counts (in place), its Q ranks -- replayed from sample_order, or the
//                        Q smallest (hashed key, rank) of order_seeds[p] found by a bisection on the key value -- and per
//                        rank the pixel with that position in row-major non-zero order: a binary search over the prefixes,
//                        then ballots over the segment's four 64-pixel rows.  The pixel's descriptor is gathered from res_a.
// Search (dcn_best_match_pairs):
//   pair_search_kernel   grid (pixel chunks, pairs).  A work-item keeps K pixels of res_b[p] in registers (16-byte loads where
//                        D % 4 == 0), K chosen by D; the pair's query descriptors pass through LDS kQT at a time.  Per query:
//                        sqrt(sum_k (res_b - d)^2) in fp32 for the K pixels in increasing pixel order with a strict
//                        comparison (first minimum), then match_search.h's key and reductions: ONE wavefront reduction for
//                        the K x 64 pixels, the workgroup's four wavefronts through LDS, at most one commit_min_key per
//                        workgroup and query.  Integer minima only: the result is the same bit for bit from run to run, ties
//                        go to the smallest pixel.
//                        HBM traffic: P * HW * D * 4 bytes of res_b, read once whatever the number of queries.
//   pair_finish_kernel   one work-item per row: unpacks the key.
#include "dcn_common.h"
#include "eval_rows.h"
#include "hashed_order.h"
#include "match_search.h"

namespace {

using dcn::align256;
using dcn::check_offsets_kernel;
using dcn::kMT;
using dcn::kMaxD;
using dcn::order_key;
using dcn::pair_rows;

constexpr int kMaxPairs = 1024;
constexpr int kMaxQ = 1024;

// ------------------------------------------------------------------------------------------------ queries
constexpr int kSeg = 256;            // pixels per segment: four rows of 64
constexpr int kSegsPerBlock = 16;    // segments a workgroup of mask_count_kernel counts, four per wavefront
constexpr int kPT = 1024;            // work-items of across_pick_kernel
constexpr int kList = 2 * kMaxQ;     // candidates of the seeded pick: the Q smallest keys plus the ties of the Q-th

__global__ void __launch_bounds__(256) mask_count_kernel(const uint8_t* __restrict__ mask, int64_t hw, int segs,
                                                         int32_t* __restrict__ seg_count, int32_t* __restrict__ mask_pixels) {
    const int p = blockIdx.y, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const uint8_t* m = mask + (size_t)p * hw;
    int total = 0;
    for (int i = wv; i < kSegsPerBlock; i += 4) {
        const int s = blockIdx.x * kSegsPerBlock + i;
        if (s >= segs) break;                               // (uniform per wavefront)
        int n = 0;
#pragma unroll
        for (int j = 0; j < kSeg / 64; ++j) {
            const int64_t pix = (int64_t)s * kSeg + j * 64 + lane;
            n += (pix < hw && m[pix] != 0) ? 1 : 0;
        }
        n = dcn::wave_sum<int>(n);
        if (lane == 0) seg_count[(size_t)p * segs + s] = n;
        total += n;
    }
    if (lane == 0 && total) atomicAdd(mask_pixels + p, total);
}

struct PickArgs {
    const uint8_t* mask;           // [P][hw]
    const float* res;              // [P][hw][D]
    const int32_t* order;          // [P][Q] replay ranks, or null
    const int64_t* seeds;          // [P] (order == null)
    const int32_t* mask_pixels;    // [P]
    int32_t* seg_prefix;           // [P][segs]: counts in, exclusive prefixes out
    int64_t* ua;                   // [P * Q]
    int64_t* va;
    float* queries;                // [P * Q][D]
    int64_t* offsets;              // [P + 1]
    int32_t* status;
    int64_t hw;
    int np, w, d, q, segs;
};

// Sum of v over the workgroup, in every work-item.  red holds kPT / 64 + 1 values.
__device__ __forceinline__ int block_total(int v, int* red) {
    v = dcn::wave_sum<int>(v);
    __syncthreads();                                        // (red may still be read from the previous call)
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    int t = 0;
#pragma unroll
    for (int i = 0; i < kPT / 64; ++i) t += red[i];
    return t;
}

__global__ void __launch_bounds__(kPT) across_pick_kernel(PickArgs a) {
    __shared__ int32_t cnt_s[kMaxPairs];                    // the pairs' mask pixels, then this pair's partial segment sums
    __shared__ int32_t rank_s[kMaxQ];
    __shared__ unsigned long long list_s[kList];
    __shared__ int red_s[kPT / 64 + 1];
    __shared__ int64_t base_s[2];                           // this pair's first row, offsets[P]
    __shared__ int fill_s;
    const int p = blockIdx.x, tid = threadIdx.x, Q = a.q, D = a.d;
    for (int i = tid; i < a.np; i += kPT) cnt_s[i] = a.mask_pixels[i];
    if (tid == 0) fill_s = 0;
    __syncthreads();
    if (tid == 0) {                                         // a pair has Q rows or none
        int64_t o = 0;
        if (p == 0) a.offsets[0] = 0;
        for (int i = 0; i < a.np; ++i) {
            if (i == p) base_s[0] = o;
            o += cnt_s[i] >= Q ? Q : 0;
            if (p == 0) a.offsets[i + 1] = o;
        }
        base_s[1] = o;
    }
    __syncthreads();
    const int n = cnt_s[p];
    const int64_t base = base_s[0], end = base_s[1];
    if (tid == 0 && n > 0 && n < Q) atomicOr(a.status, DCN_ACROSS_TOO_FEW_MASK_PIXELS);   // random.sample raises there
    for (int e = tid; e < Q; e += kPT) {                    // this pair's share of the capacity's tail
        const int64_t g = (int64_t)p * Q + e;
        if (g >= end) {
            a.ua[g] = -1;
            a.va[g] = -1;
            for (int k = 0; k < D; ++k) a.queries[g * D + k] = 0.f;
        }
    }
    if (n < Q) return;                                      // (uniform per workgroup)
    __syncthreads();                                        // (cnt_s is reused)
    // ---- exclusive prefix of the segment counts, in place: a run of segments per work-item
    int32_t* pre = a.seg_prefix + (size_t)p * a.segs;
    const int run = dcn::ceil_div(a.segs, kPT);
    const int s0 = min(tid * run, a.segs), s1 = min(s0 + run, a.segs);
    {
        int t = 0;
        for (int s = s0; s < s1; ++s) t += pre[s];
        cnt_s[tid] = t;
    }
    __syncthreads();
    if (tid == 0) {
        int o = 0;
        for (int i = 0; i < kPT; ++i) {
            const int t = cnt_s[i];
            cnt_s[i] = o;
            o += t;
        }
    }
    __syncthreads();
    {
        int o = cnt_s[tid];
        for (int s = s0; s < s1; ++s) {
            const int t = pre[s];
            pre[s] = o;
            o += t;
        }
    }
    // ---- the Q ranks
    for (int e = tid; e < Q; e += kPT) rank_s[e] = 0;
    __syncthreads();
    if (a.order) {
        int bad = 0;
        if (tid < Q) {
            int r = a.order[(size_t)p * Q + tid];
            if (r < 0 || r >= n) {
                bad = DCN_EVAL_BAD_DRAWS;
                r = 0;
            }
            rank_s[tid] = r;
        }
        __syncthreads();
        if (tid < Q) {
            const int r = rank_s[tid];
            for (int j = 0; j < tid; ++j) bad |= rank_s[j] == r ? DCN_EVAL_BAD_DRAWS : 0;   // (random.sample never repeats)
            if (bad) atomicOr(a.status, bad);
        }
    } else {
        // the smallest key value T with at least Q keys <= T: fewer than Q keys lie below it
        const uint64_t seed = (uint64_t)a.seeds[p];
        uint64_t lo = 0, hi = 0xffffffffull;
        while (lo < hi) {                                   // (uniform: 32 rounds)
            const uint32_t mid = (uint32_t)((lo + hi) >> 1);
            int c = 0;
            for (int i = tid; i < n; i += kPT) c += order_key(seed, (uint32_t)i) <= mid ? 1 : 0;
            if (block_total(c, red_s) >= Q) hi = mid;
            else lo = (uint64_t)mid + 1;
        }
        const uint32_t T = (uint32_t)lo;
        for (int i = tid; i < n; i += kPT) {
            const uint32_t k = order_key(seed, (uint32_t)i);
            if (k <= T) {
                const int slot = atomicAdd(&fill_s, 1);
                if (slot < kList) list_s[slot] = ((unsigned long long)k << 32) | (unsigned)i;
            }
        }
        __syncthreads();
        int m = fill_s;
        if (m > kList) {                                    // (more than 1024 ranks share ONE 32-bit key value)
            if (tid == 0) atomicOr(a.status, DCN_EVAL_BAD_DRAWS);
            m = kList;
        }
        for (int e = tid; e < m; e += kPT) {                // row = position in (key, rank) order
            const unsigned long long me = list_s[e];
            int r = 0;
            for (int j = 0; j < m; ++j) r += list_s[j] < me ? 1 : 0;
            if (r < Q) rank_s[r] = (int)(unsigned)(me & 0xffffffffull);
        }
    }
    __syncthreads();
    // ---- rank -> pixel -> descriptor, a wavefront per query
    const int lane = tid & 63;
    const uint8_t* m = a.mask + (size_t)p * a.hw;
    for (int e = tid >> 6; e < Q; e += kPT / 64) {
        const int r = rank_s[e];
        int slo = 0, shi = a.segs - 1;                      // the last segment whose prefix is <= r
        while (slo < shi) {
            const int mid = (slo + shi + 1) >> 1;
            if (pre[mid] <= r) slo = mid;
            else shi = mid - 1;
        }
        int rem = r - pre[slo];
        unsigned long long on[kSeg / 64];
#pragma unroll
        for (int j = 0; j < kSeg / 64; ++j) {
            const int64_t pix = (int64_t)slo * kSeg + j * 64 + lane;
            on[j] = __ballot(pix < a.hw && m[pix] != 0);
        }
        int64_t pix = -1;
#pragma unroll
        for (int j = 0; j < kSeg / 64; ++j) {
            const int c = __builtin_popcountll(on[j]);
            if (pix < 0 && rem < c) {                       // bit number rem of this row
                const unsigned long long below = on[j] & ((1ull << lane) - 1ull);
                const unsigned long long it = __ballot(((on[j] >> lane) & 1ull) && __builtin_popcountll(below) == rem);
                pix = (int64_t)slo * kSeg + j * 64 + (it ? __builtin_ctzll(it) : 0);
            }
            rem -= c;
        }
        if (pix < 0 || pix >= a.hw) pix = 0;                // (cannot happen while the counts describe the mask)
        const int64_t row = base + e;
        if (lane == 0) {
            a.ua[row] = pix % a.w;
            a.va[row] = pix / a.w;
        }
        const float* src = a.res + ((size_t)p * a.hw + pix) * D;
        for (int k = lane; k < D; k += 64) a.queries[row * D + k] = src[k];
    }
}

// ------------------------------------------------------------------------------------------------ search
constexpr int kQT = 64;     // queries staged in LDS at a time

struct SearchArgs {
    const float* res;              // [P][hw][D]
    const float* queries;          // [R][D]
    const int64_t* offsets;        // [P + 1]
    const int32_t* offsets_bad;    // [1] set by check_offsets_kernel
    unsigned long long* best;      // [R] packed (norm bits << 32 | pixel)
    int32_t* status;
    int64_t hw, max_rows;
    int d, max_pair_rows;
};

struct alignas(16) F4 {
    float x, y, z, w;
};

// DT: the descriptor dimension (0: any, read from a.d); K: pixels per work-item; VEC: 16-byte loads (DT % 4 == 0 and an
// aligned base)
template <int DT, int K, bool VEC>
__global__ void __launch_bounds__(kMT) pair_search_kernel(SearchArgs a) {
    constexpr int DV = DT > 0 ? DT : kMaxD;                 // registers per pixel
    constexpr int DP = (DV + 3) & ~3;                       // floats per query in LDS
    __shared__ __attribute__((aligned(16))) float sq[kQT * DP];
    __shared__ unsigned long long skey[kQT][kMT / 64];
    const int D = DT > 0 ? DT : a.d;
    const int p = blockIdx.y;
    int bad = 0;
    int64_t lo;
    int nq;
    pair_rows(a.offsets, a.offsets_bad, p, a.max_rows, a.max_pair_rows, lo, nq, bad);
    if (bad && blockIdx.x == 0 && threadIdx.x == 0) atomicOr(a.status, bad);
    if (nq == 0) return;                                    // (uniform per workgroup)
    const int64_t hw = a.hw;
    const int64_t pix0 = (int64_t)blockIdx.x * (kMT * K) + threadIdx.x;   // pixel k of this work-item: pix0 + k * kMT
    const float* res = a.res + (size_t)p * hw * D;
    float v[K][DV];
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const int64_t pix = pix0 + k * kMT;
        const float* src = res + (pix < hw ? pix : hw - 1) * D;   // (past the end: the last pixel again, never chosen)
        if (VEC) {
#pragma unroll
            for (int c = 0; c < DV / 4; ++c) {
                const F4 t = *(const F4*)(src + 4 * c);
                v[k][4 * c] = t.x;
                v[k][4 * c + 1] = t.y;
                v[k][4 * c + 2] = t.z;
                v[k][4 * c + 3] = t.w;
            }
        } else {
#pragma unroll
            for (int c = 0; c < DV; ++c) v[k][c] = c < D ? src[c] : 0.f;
        }
    }
    const float inf = __builtin_inff();
    for (int q0 = 0; q0 < nq; q0 += kQT) {
        const int qn = min(kQT, nq - q0);
        __syncthreads();
        for (int i = threadIdx.x; i < qn * D; i += kMT) {
            const int q = i / D;
            sq[q * DP + (i - q * D)] = a.queries[(lo + q0) * D + i];
        }
        __syncthreads();
        for (int q = 0; q < qn; ++q) {
            float best = inf;
            unsigned bi = (unsigned)pix0;
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const float d2 = dcn::dist2<DT>(v[k], sq + q * DP, D);
                const float s = pix0 + k * kMT < hw ? sqrtf(d2) : inf;
                const bool take = s < best;                 // strict, pixels increasing: the first minimum
                best = take ? s : best;
                bi = take ? (unsigned)(pix0 + k * kMT) : bi;
            }
            dcn::park_key(skey[q], dcn::wave_min_key(pix0 < hw ? dcn::match_key(best, bi) : dcn::kNoKey));
        }
        __syncthreads();
        if ((int)threadIdx.x < qn) dcn::commit_min_key(a.best + lo + q0 + threadIdx.x, dcn::block_min_key(skey[threadIdx.x]));
    }
}

__global__ void __launch_bounds__(256) pair_finish_kernel(const unsigned long long* __restrict__ best,
                                                          const int64_t* __restrict__ offsets,
                                                          const int32_t* __restrict__ offsets_bad, int np, int w,
                                                          int64_t max_rows, int max_pair_rows, float* __restrict__ norm_diff,
                                                          int32_t* __restrict__ best_uv, int32_t* __restrict__ row_pair) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= max_rows) return;
    const int p = dcn::row_owner(offsets, np, r);
    const bool mine = dcn::row_in_pair(offsets, offsets_bad, p, np, r, max_rows, max_pair_rows);
    const unsigned long long k = mine ? best[r] : dcn::kNoKey;
    if (k == dcn::kNoKey) {                                 // past the last row, cut off a bad list, or no key written
        norm_diff[r] = __builtin_nanf("");
        best_uv[r] = -1;
        best_uv[max_rows + r] = -1;
        row_pair[r] = -1;
        return;
    }
    const int i = (int)dcn::key_pixel(k);
    norm_diff[r] = dcn::key_norm(k);
    best_uv[r] = i % w;
    best_uv[max_rows + r] = i / w;
    row_pair[r] = p;
}

inline bool shape_ok(int p, int h, int w, int d) {
    return p >= 1 && p <= kMaxPairs && h >= 1 && w >= 1 && (int64_t)h * w < ((int64_t)1 << 31) && d >= 1 && d <= kMaxD;
}

template <int DT, int K>
inline void launch_search(const SearchArgs& a, int p, bool vec, hipStream_t st) {
    const dim3 grid((unsigned)dcn::ceil_div64(a.hw, (int64_t)kMT * K), (unsigned)p), block(kMT);
    if (DT > 0 && DT % 4 == 0 && vec) hipLaunchKernelGGL((pair_search_kernel<DT, K, (DT > 0 && DT % 4 == 0)>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((pair_search_kernel<DT, K, false>), grid, block, 0, st, a);
}

}  // namespace

// seg_count / seg_prefix int32 [p][segments]
extern "C" size_t dcn_across_object_queries_workspace(int p, int h, int w) {
    if (p < 1 || p > kMaxPairs || h < 1 || w < 1 || (int64_t)h * w >= ((int64_t)1 << 31)) return 0;
    return align256((size_t)p * (size_t)dcn::ceil_div64((int64_t)h * w, kSeg) * sizeof(int32_t));
}

extern "C" int dcn_across_object_queries(int p, int h, int w, int d, const uint8_t* mask_a, const float* res_a, int q,
                                         const int32_t* sample_order, const int64_t* order_seeds, int64_t* u_a, int64_t* v_a,
                                         float* queries, int64_t* offsets, int32_t* mask_pixels, int32_t* status,
                                         void* workspace, void* stream) {
    if (!shape_ok(p, h, w, d) || !mask_a || !res_a || q < 1 || q > kMaxQ || (!sample_order && !order_seeds) || !u_a || !v_a ||
        !queries || !offsets || !mask_pixels || !status || !workspace)
        return DCN_E_INVALID;
    hipStream_t st = (hipStream_t)stream;
    const int64_t hw = (int64_t)h * w;
    const int segs = (int)dcn::ceil_div64(hw, kSeg);
    int rc = dcn::fill_bytes_async(mask_pixels, 0, (size_t)p * sizeof(int32_t), st);
    if (rc == DCN_OK) rc = dcn::fill_bytes_async(status, 0, sizeof(int32_t), st);
    if (rc != DCN_OK) return rc;
    int32_t* seg = (int32_t*)workspace;
    hipLaunchKernelGGL(mask_count_kernel, dim3((unsigned)dcn::ceil_div(segs, kSegsPerBlock), (unsigned)p), dim3(256), 0, st,
                       mask_a, hw, segs, seg, mask_pixels);
    PickArgs a;
    a.mask = mask_a;
    a.res = res_a;
    a.order = sample_order;
    a.seeds = order_seeds;
    a.mask_pixels = mask_pixels;
    a.seg_prefix = seg;
    a.ua = u_a;
    a.va = v_a;
    a.queries = queries;
    a.offsets = offsets;
    a.status = status;
    a.hw = hw;
    a.np = p;
    a.w = w;
    a.d = d;
    a.q = q;
    a.segs = segs;
    hipLaunchKernelGGL(across_pick_kernel, dim3((unsigned)p), dim3(kPT), 0, st, a);
    return dcn::check_launch();
}

// best [R] u64 | offsets_bad int32
extern "C" size_t dcn_best_match_pairs_workspace(int64_t max_rows) {
    return align256((size_t)(max_rows > 0 ? max_rows : 1) * sizeof(unsigned long long)) + 256;
}

extern "C" int dcn_best_match_pairs(int p, int h, int w, int d, const float* res_b, const float* queries,
                                    const int64_t* offsets, int64_t max_rows, int max_pair_rows, float* norm_diff,
                                    int32_t* best_uv, int32_t* row_pair, int32_t* status, void* workspace, void* stream) {
    if (!shape_ok(p, h, w, d) || !res_b || !queries || !offsets || max_rows < 1 || max_pair_rows < 1 || !norm_diff ||
        !best_uv || !row_pair || !status || !workspace)
        return DCN_E_INVALID;
    hipStream_t st = (hipStream_t)stream;
    const size_t R = (size_t)max_rows;
    SearchArgs a;
    a.best = (unsigned long long*)workspace;
    int32_t* flag = (int32_t*)((char*)workspace + align256(R * sizeof(unsigned long long)));
    int rc = dcn::fill_bytes_async(a.best, 0xFF, R * sizeof(unsigned long long), st);
    if (rc == DCN_OK) rc = dcn::fill_bytes_async(status, 0, sizeof(int32_t), st);
    if (rc == DCN_OK) rc = dcn::fill_bytes_async(flag, 0, sizeof(int32_t), st);
    if (rc != DCN_OK) return rc;
    hipLaunchKernelGGL(check_offsets_kernel, dim3(dcn::ceil_div(p, 256)), dim3(256), 0, st, offsets, p, max_rows, flag, status);
    a.res = res_b;
    a.queries = queries;
    a.offsets = offsets;
    a.offsets_bad = flag;
    a.status = status;
    a.hw = (int64_t)h * w;
    a.max_rows = max_rows;
    a.d = d;
    a.max_pair_rows = max_pair_rows;
    const bool vec = ((uintptr_t)res_b & 15) == 0;
    switch (d) {                                            // pixels per work-item: about 32 floats of res_b in registers
        case 1: launch_search<1, 8>(a, p, vec, st); break;
        case 3: launch_search<3, 8>(a, p, vec, st); break;
        case 4: launch_search<4, 8>(a, p, vec, st); break;
        case 8: launch_search<8, 4>(a, p, vec, st); break;
        case 16: launch_search<16, 2>(a, p, vec, st); break;
        case 32: launch_search<32, 1>(a, p, vec, st); break;
        default: launch_search<0, 1>(a, p, vec, st); break;
    }
    hipLaunchKernelGGL(pair_finish_kernel, dim3((unsigned)dcn::ceil_div64(max_rows, 256)), dim3(256), 0, st,
                       (const unsigned long long*)a.best, offsets, (const int32_t*)flag, p, w, max_rows, max_pair_rows,
                       norm_diff, best_uv, row_pair);
    return dcn::check_launch();
}
