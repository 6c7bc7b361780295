// The primitives of every best-match search (match_kernels.hip, acrossobj_kernels.hip, and through eval_stats.h
// evaluate_kernels.hip and crossscene_kernels.hip).  A work-item holds a pixel's descriptor in registers and loops over queries
// staged in LDS; per query the candidates are reduced as packed 64-bit keys: over the wavefront by shuffles, over the
// workgroup's wavefronts through LDS, over the workgroups by at most one atomic minimum each.
//
// The key is norm bits << 32 | pixel: the norms are not negative, so their bit patterns order as they do, and of two pixels with
// one norm the smaller index wins, as np.argmin's first occurrence.  It holds the NORM, sqrtf(dist2), not dist2: the square root
// maps about two neighbouring squared distances onto one norm, and np.argmin sees the norms -- of two pixels with one norm it
// returns the first, whichever has the smaller squared distance.  So the returned pixel is the first argmin of the norm_diffs
// image, in every kernel that keys with match_key.
#pragma once
#include "dcn_common.h"

namespace dcn {

constexpr int kMT = 256;        // work-items per workgroup of a search kernel: four wavefronts
constexpr int kMaxD = 64;
constexpr double kEvalSumScale = 1048576.0;   // pixel distances are summed as integers of 2^-20 pixel: the sum does not depend on the order
constexpr unsigned long long kNoKey = ~0ull;  // no candidate: loses against every key

__device__ __forceinline__ unsigned long long match_key(float norm, unsigned pix) {
    return (((unsigned long long)__float_as_uint(norm)) << 32) | pix;
}
__device__ __forceinline__ unsigned key_pixel(unsigned long long k) { return (unsigned)(k & 0xffffffffull); }
__device__ __forceinline__ float key_norm(unsigned long long k) { return __uint_as_float((unsigned)(k >> 32)); }

// The register load of a descriptor, v[k] = (in && k < D) ? res[pix * D + k] : 0.f under #pragma unroll, stays written out in
// each kernel: filled through a function, v is promoted to one vector value instead of DT scalars, and the kernels grow by up
// to 90 % in instructions (profiles/match_search_refactor_isa.txt).
//
// sum_k (v[k] - q[k])^2 as one fma chain over the channels 0 .. D - 1
template <int DT>
__device__ __forceinline__ float dist2(const float (&v)[DT > 0 ? DT : kMaxD], const float* q, int D) {
    float d2 = 0.f;
#pragma unroll
    for (int k = 0; k < (DT > 0 ? DT : kMaxD); ++k) {
        if (k < D) { const float t = v[k] - q[k]; d2 = fmaf(t, t, d2); }
    }
    return d2;
}

// The minimum of the wavefront's keys, in lane 0
__device__ __forceinline__ unsigned long long wave_min_key(unsigned long long key) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long o = __shfl_down(key, off, 64);
        key = o < key ? o : key;
    }
    return key;
}

// Across the workgroup's wavefronts: lane 0 parks wave_min_key's result in its slot of the query's LDS row; after a barrier one
// work-item per query takes the row's minimum
__device__ __forceinline__ void park_key(unsigned long long (&row)[kMT / 64], unsigned long long key) {
    if ((threadIdx.x & 63) == 0) row[threadIdx.x >> 6] = key;
}
__device__ __forceinline__ unsigned long long block_min_key(const unsigned long long (&row)[kMT / 64]) {
    unsigned long long key = row[0];
#pragma unroll
    for (int x = 1; x < kMT / 64; ++x) key = row[x] < key ? row[x] : key;
    return key;
}

// *slot = min(*slot, key), with a plain load in front of the 64-bit atomic: thousands of workgroups target the same few words,
// and after the first few almost every key loses; without the look a kernel is serialised on those atomics (12 us -> 1 us per
// query in best_match_kernel).
__device__ __forceinline__ void commit_min_key(unsigned long long* slot, unsigned long long key) {
    if (key != kNoKey && key < __atomic_load_n(slot, __ATOMIC_RELAXED)) atomicMin(slot, key);
}

// The statistics of one query over the pixels it has been shown (evaluation.py:1046-1100): best match over the image (0) and
// over the mask (1: masked_norm_diffs, + 1e6 off the mask), the number of pixels closer than the ground truth, and the sum of
// their pixel distances to it, in units of 1 / kEvalSumScale pixel.  Integer accumulations only: the order does not matter.
struct QueryStats {
    unsigned long long k0 = kNoKey, k1 = kNoKey;
    int n0 = 0, n1 = 0;
    unsigned long long s0 = 0ull, s1 = 0ull;

    // Pixel pix at descriptor distance dd, on the mask or not, competes for the two best matches.  `in`: the pixel exists (a
    // work-item past the image's end offers nothing).  Returns masked_norm_diffs' value for the pixel.
    __device__ __forceinline__ float offer(bool in, float dd, bool onm, unsigned pix) {
        const float dm = onm ? dd : dd + 1e6f;
        const unsigned long long c0k = in ? match_key(dd, pix) : kNoKey, c1k = in ? match_key(dm, pix) : kNoKey;
        k0 = c0k < k0 ? c0k : k0;
        k1 = c1k < k1 ? c1k : k1;
        return dm;
    }

    // offer(), and pixel pix = (pu, pv) is counted where it is closer than the query's ground truth (gu, gv), which lies at
    // descriptor distance tt.  Straight-line: where dd >= tt nothing is counted (the masked distance is never below dd), and a
    // caller that tests that itself may call offer() alone and skip the float64 step.
    __device__ __forceinline__ void add(bool in, float dd, bool onm, unsigned pix, float tt, int pu, int pv, int gu, int gv) {
        const float dm = offer(in, dd, onm, pix);
        const bool c0 = in && dd < tt, c1 = in && dm < tt;
        const float du = (float)(pu - gu), dv = (float)(pv - gv);
        const float pd = sqrtf(du * du + dv * dv);
        const unsigned long long pf = (unsigned long long)((double)pd * kEvalSumScale + 0.5);
        n0 += c0 ? 1 : 0;
        n1 += c1 ? 1 : 0;
        s0 += c0 ? pf : 0ull;
        s1 += c1 ? pf : 0ull;
    }
};

}  // namespace dcn
