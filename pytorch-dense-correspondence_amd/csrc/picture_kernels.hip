// Qualitative evaluation (include/dcn_hip.h section 15): the arithmetic that turns descriptor images into pictures -- the
// three normalisations of dense_correspondence/evaluation/plotting.py:5-87 as plot_descriptor_colormaps
// (evaluation.py:530-601) uses them, the bytes matplotlib's imshow shows for the result, and the distance heat map of
// compute_gaussian_kernel_heatmap_from_norm_diffs (dense_correspondence_manipulation/utils/visualization.py:27-31).
//
// Ranges (dcn_descriptor_ranges):
//   range_partial_kernel   grid (workgroups per image, 2 P images).  descstats_kernels.hip's walk: a workgroup owns a run of
//                          pixels, a work-item keeps ONE channel and takes its elements in batches of 8 loads.  Four
//                          accumulators -- min and max over the image, min and max over the products x * m that numpy counts as
//                          non-zero -- and three flags (NaN in the image, NaN among the products, any product at all).  Folded
//                          over the pixel slots through LDS as a binary tree, one partial per workgroup and channel.
//                          HBM traffic: 2 P * hw * (4 d + 1) bytes, read once.
//   range_finish_kernel    one workgroup per pair: work-item (image, channel) folds that channel's partials in workgroup
//                          order, then the pair's ranges by Python's min(a, b) / max(a, b), the images' scalar ranges and the
//                          pair's status.
// Normalise (dcn_descriptor_normalize): norm_kernel, grid (workgroups per image, 2 P images).  A picture is written as whole
//   dwords: a work-item assembles four consecutive bytes of the picture (four elements of the image) and stores them at a
//   4-byte aligned address; the bytes in front of the first and behind the last aligned dword of a picture go through a byte
//   path of at most 3 + 3 stores.  The pictures of both families are written in one pass over the image; the float images,
//   where asked for, in a pass of their own each, element by element (4- and 8-byte stores).
//   HBM traffic per image: hw * (4 d + 1) bytes read per pass, the outputs written once.
// Heat maps (dcn_heat_maps): heat_levels_kernel (one workgroup) turns the exact formula into 255 thresholds on the squared
//   distance; heat_kernel, grid (pixel tiles, pairs), finds every byte from them, so no float64 exponential is in its loop.
//   A work-item keeps K consecutive pixels of res_b[p] in registers (K = 16, 8, 4 by D; read from memory per row for D > 16),
//   the pair's query descriptors pass through LDS 64 at a
//   time.  Per row the K bytes (3 K with a colour table, looked up in LDS) are packed into dwords in TILE order; the row's
//   plane starts at an arbitrary byte, so a wavefront shifts its dwords by the row's misalignment with one neighbour exchange
//   (__shfl_down) and every work-item stores K / 4 (3 K / 4) consecutive aligned dwords in one piece; the at most 3 + 3 bytes at
//   the two ends of the wavefront's segment are byte stores by its first and last work-item.  The last, partial segment of an
//   image is written byte by byte.  HBM traffic per pair: hw * d * 4 bytes read once, rows * hw (* 3) bytes written.
// No floating-point atomics: every output is the same bit for bit from run to run.
#include "dcn_common.h"
#include "eval_rows.h"

namespace {

using dcn::check_offsets_kernel;
using dcn::pair_rows;

constexpr int kMaxD = 64;
constexpr int kMaxPairs = 1024;

// ------------------------------------------------------------------------------------------------ ranges
constexpr int kRT = 256;          // work-items of the partial kernel
constexpr int kSteps = 16;        // steps of (kRT / d) pixels a workgroup takes at least
constexpr int kBatch = 8;         // elements a work-item loads before it accumulates them
constexpr int kMaxBlocks = 256;   // workgroups per image at most: the finish kernel folds them one after another
constexpr int kFT = 2 * kMaxD;    // work-items of the finish kernel: (image of the pair, channel)
constexpr int kNanImage = 1, kNanProduct = 2, kAnyProduct = 4;

struct Split {
    int64_t pixels_per_block;
    int blocks;
};
__host__ __device__ inline Split split_image(int64_t hw, int d) {
    int64_t ppb = (int64_t)(kRT / d) * kSteps;
    const int64_t least = (hw + kMaxBlocks - 1) / kMaxBlocks;
    if (ppb < least) ppb = least;
    Split s;
    s.pixels_per_block = ppb;
    s.blocks = (int)((hw + ppb - 1) / ppb);
    return s;
}

// a := a (+) b.  The comparisons drop NaN; the flags carry it.
__device__ __forceinline__ void range_fold(float& lo0, float& hi0, float& lo1, float& hi1, int& flags, float blo0, float bhi0,
                                           float blo1, float bhi1, int bflags) {
    lo0 = blo0 < lo0 ? blo0 : lo0;
    hi0 = bhi0 > hi0 ? bhi0 : hi0;
    lo1 = blo1 < lo1 ? blo1 : lo1;
    hi1 = bhi1 > hi1 ? bhi1 : hi1;
    flags |= bflags;
}

struct RangeArgs {
    const float* res[2];        // image a, image b (null: no second image): [P][hw][d]
    const uint8_t* mask[2];     // [P][hw] or null
    float* part_lohi;           // [2 P][blocks][4][d]: min, max, product min, product max
    int32_t* part_flags;        // [2 P][blocks][d]
    int64_t hw;
    int np, d;
};

__global__ void __launch_bounds__(kRT) range_partial_kernel(RangeArgs a) {
    __shared__ float s_lohi[4][kRT];
    __shared__ int s_flags[kRT];
    const int d = a.d;
    const Split sp = split_image(a.hw, d);
    const int img = blockIdx.y, side = img / a.np, p = img - side * a.np, b = blockIdx.x, tid = threadIdx.x;
    const int per_step = kRT / d;                           // pixel slots; work-item tid is slot tid / d, channel tid % d
    const int slot = tid / d, c = tid - slot * d;
    const bool active = slot < per_step;
    const int64_t p0 = (int64_t)b * sp.pixels_per_block;
    const int64_t p1 = p0 + sp.pixels_per_block < a.hw ? p0 + sp.pixels_per_block : a.hw;
    const float inf = __builtin_inff();
    float lo0 = inf, hi0 = -inf, lo1 = inf, hi1 = -inf;
    int flags = 0;
    const float* r = a.res[side];
    if (r && active && p0 + slot < p1) {
        r += (size_t)p * (size_t)a.hw * (size_t)d;
        const uint8_t* m = a.mask[side] ? a.mask[side] + (size_t)p * (size_t)a.hw : nullptr;
        const int mine = (int)((p1 - (p0 + slot) + per_step - 1) / per_step);   // this work-item's elements: one per step
        const float* rp = r + (p0 + slot) * d + c;
        const uint8_t* mp = m ? m + (p0 + slot) : nullptr;
        for (int i = 0; i < mine; i += kBatch) {
            float x[kBatch];
            uint8_t on[kBatch];
#pragma unroll
            for (int k = 0; k < kBatch; ++k) {              // all loads first; past the last element: the last element again
                const int j = i + k < mine ? i + k : mine - 1;
                x[k] = rp[(int64_t)j * per_step * d];
                on[k] = mp ? mp[(int64_t)j * per_step] : (uint8_t)1;
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int k = 0; k < kBatch; ++k) {
                const bool in = i + k < mine;
                const float v = x[k];
                const bool isnan = !(v == v);
                lo0 = (in && v < lo0) ? v : lo0;
                hi0 = (in && v > hi0) ? v : hi0;
                // the product x * m, m in {0, 1}: x under the mask; outside it +-0, or NaN for a non-finite x.  numpy's
                // nonzero keeps NaN and drops both zeros.
                const bool finite = v - v == 0.f;
                const bool bad = in && (on[k] != 0 ? isnan : !finite);
                const bool take = in && on[k] != 0 && !isnan && v != 0.f;
                lo1 = (take && v < lo1) ? v : lo1;
                hi1 = (take && v > hi1) ? v : hi1;
                flags |= (in && isnan ? kNanImage : 0) | (bad ? kNanProduct | kAnyProduct : 0) | (take ? kAnyProduct : 0);
            }
        }
    }
    // a binary tree over the pixel slot: slot i takes slot i + half, always in the same order
    int half = 1;
    while (half < per_step) half <<= 1;
    for (half >>= 1; half > 0; half >>= 1) {
        if (active && slot >= half && slot < 2 * half) {
            s_lohi[0][tid] = lo0;
            s_lohi[1][tid] = hi0;
            s_lohi[2][tid] = lo1;
            s_lohi[3][tid] = hi1;
            s_flags[tid] = flags;
        }
        __syncthreads();
        if (active && slot < half && slot + half < per_step) {
            const int o = tid + half * d;                   // (slot + half, c): o < per_step * d <= kRT
            range_fold(lo0, hi0, lo1, hi1, flags, s_lohi[0][o], s_lohi[1][o], s_lohi[2][o], s_lohi[3][o], s_flags[o]);
        }
    }
    if (tid < d) {
        const size_t blk = (size_t)img * sp.blocks + b;
        a.part_lohi[(blk * 4 + 0) * d + c] = lo0;
        a.part_lohi[(blk * 4 + 1) * d + c] = hi0;
        a.part_lohi[(blk * 4 + 2) * d + c] = lo1;
        a.part_lohi[(blk * 4 + 3) * d + c] = hi1;
        a.part_flags[blk * d + c] = flags;
    }
}

// Python's min(a, b) / max(a, b): b only when the comparison with a holds -- a NaN in a stays, a NaN in b alone is dropped
__device__ __forceinline__ float py_min(float a, float b) { return b < a ? b : a; }
__device__ __forceinline__ float py_max(float a, float b) { return b > a ? b : a; }

__global__ void __launch_bounds__(kFT) range_finish_kernel(RangeArgs a, float* __restrict__ image_ranges,
                                                           float* __restrict__ pair_ranges, float* __restrict__ scalar_ranges,
                                                           int32_t* __restrict__ status) {
    __shared__ float s_r[2][4][kMaxD];
    __shared__ int s_f[2][kMaxD];
    const int d = a.d, p = blockIdx.x, tid = threadIdx.x;
    const int side = tid / kMaxD, c = tid - side * kMaxD;
    const Split sp = split_image(a.hw, d);
    const float qnan = __builtin_nanf(""), inf = __builtin_inff();
    const bool two = a.res[1] != nullptr, masked = a.mask[0] != nullptr;
    if (c < d && (side == 0 || two)) {
        float lo0 = inf, hi0 = -inf, lo1 = inf, hi1 = -inf;
        int flags = 0;
        for (int b = 0; b < sp.blocks; ++b) {
            const size_t blk = ((size_t)side * a.np + p) * sp.blocks + b;
            range_fold(lo0, hi0, lo1, hi1, flags, a.part_lohi[(blk * 4 + 0) * d + c], a.part_lohi[(blk * 4 + 1) * d + c],
                       a.part_lohi[(blk * 4 + 2) * d + c], a.part_lohi[(blk * 4 + 3) * d + c], a.part_flags[blk * d + c]);
        }
        // np.min / np.max: a NaN propagates; of no element at all: the reference raises (EMPTY_RANGE), NaN here
        const bool n0 = flags & kNanImage, n1 = (flags & kNanProduct) || !(flags & kAnyProduct) || !masked;
        float v[4] = {n0 ? qnan : lo0, n0 ? qnan : hi0, n1 ? qnan : lo1, n1 ? qnan : hi1};
        float* o = image_ranges + (((size_t)side * a.np + p) * 4) * d + c;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            o[k * d] = v[k];
            s_r[side][k][c] = v[k];
        }
        s_f[side][c] = flags;
    }
    __syncthreads();
    if (side == 0 && c < d) {
        float* o = pair_ranges + ((size_t)p * 4) * d + c;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float x = s_r[0][k][c], y = two ? s_r[1][k][c] : x;
            o[k * d] = (k & 1) ? py_max(x, y) : py_min(x, y);
        }
    }
    if (c == 0 && (side == 0 || two)) {                     // res.min(), res.max() over every channel: NaN propagates
        float lo = inf, hi = -inf;
        bool nan = false;
        for (int k = 0; k < d; ++k) {
            const float l = s_r[side][0][k], h = s_r[side][1][k];
            nan = nan || !(l == l);
            lo = l < lo ? l : lo;
            hi = h > hi ? h : hi;
        }
        scalar_ranges[((size_t)side * a.np + p) * 2 + 0] = nan ? qnan : lo;
        scalar_ranges[((size_t)side * a.np + p) * 2 + 1] = nan ? qnan : hi;
    }
    if (tid == 0) {
        int word = 0;
        if (masked)
            for (int s = 0; s < (two ? 2 : 1); ++s)
                for (int k = 0; k < d; ++k) word |= (s_f[s][k] & kAnyProduct) ? 0 : DCN_PICTURE_EMPTY_RANGE;
        status[p] = word;
    }
}

// ------------------------------------------------------------------------------------------------ normalise
constexpr int kNT = 256;          // work-items
constexpr int kNormBlocks = 512;  // workgroups per image at most

struct NormArgs {
    const float* res[2];          // [P][hw][d]; res[1] null: one image per "pair"
    const uint8_t* mask[2];       // [P][hw] or null
    const float* pair_ranges;     // [P][4][d] (modes PAIR, MASKED_PAIR)
    const float* scalar_ranges;   // [2][P][2] (mode SCALAR)
    const double* stats[2];       // family 0, family 1: [2][d] min, max (the STATS modes)
    void* normed[2];              // per family: [2][P][hw][d] float (double for the STATS modes) or null
    uint8_t* picture[2];          // per family: picture of (side, pair) at side * side_stride + pair * pair_stride, or null
    int64_t side_stride[2], pair_stride[2];
    int64_t hw;
    int mode[2];                  // DCN_NORM_* per family
    int np, d, pc;                // pc: channels of a picture (1 or 3)
    int channel[3];               // the image channels a picture shows
};

__device__ __forceinline__ bool is_f64(int mode) { return mode == DCN_NORM_STATS || mode == DCN_NORM_STATS_MASKED; }

// One element of family f: the value in the precision the reference computes it in (T = float or double)
template <class T>
__device__ __forceinline__ T norm_value(const NormArgs& a, int f, int side, int p, int c, float x, float mf);

template <>
__device__ __forceinline__ float norm_value<float>(const NormArgs& a, int f, int side, int p, int c, float x, float mf) {
    const int mode = a.mode[f];
    if (mode == DCN_NORM_SCALAR) {                          // (x - res_min) / ((res_max - res_min) + eps), float32 throughout
        const float mn = a.scalar_ranges[((size_t)side * a.np + p) * 2], mx = a.scalar_ranges[((size_t)side * a.np + p) * 2 + 1];
        const float scale = (mx - mn) + 1e-10f;
        return (x - mn) / scale;
    }
    const float* pr = a.pair_ranges + ((size_t)p * 4 + (mode == DCN_NORM_MASKED_PAIR ? 2 : 0)) * a.d + c;
    const float mn = pr[0], mx = pr[a.d];
    const float scale = mx - mn;
    const float v = (x - mn) / scale;
    return mode == DCN_NORM_MASKED_PAIR ? v * mf : v;
}

template <>
__device__ __forceinline__ double norm_value<double>(const NormArgs& a, int f, int side, int p, int c, float x, float mf) {
    // np.clip(res, min, max) of a float32 image against float64 arrays: float64 from there on
    const bool masked = a.mode[f] == DCN_NORM_STATS_MASKED;
    const float xin = masked ? x * mf : x;                   // (mask * res in float32, plot_descriptor_colormaps :588-589)
    const double mn = a.stats[f][c], mx = a.stats[f][a.d + c];
    double v = (double)xin;
    v = v < mn ? mn : v;
    v = v > mx ? mx : v;
    const double scale = (mx - mn) + 1e-10;
    v = (v - mn) / scale;
    return masked ? v * (double)mf : v;
}

// uint8(255 * clip(v, 0, 1)), the product in the precision of v, truncated; NaN gives 0
__device__ __forceinline__ unsigned picture_byte(float v) {
    const float t = v < 0.f ? 0.f : (v > 1.f ? 1.f : v);
    return v == v ? (unsigned)(int)(255.f * t) : 0u;
}
__device__ __forceinline__ unsigned picture_byte(double v) {
    const double t = v < 0. ? 0. : (v > 1. ? 1. : v);
    return v == v ? (unsigned)(int)(255. * t) : 0u;
}

__device__ __forceinline__ unsigned norm_byte(const NormArgs& a, int f, int side, int p, const float* r, const uint8_t* m,
                                              int64_t byte) {
    const int64_t pix = a.pc == 3 ? byte / 3 : byte;
    const int c = a.channel[(int)(byte - pix * a.pc)];
    const float x = r[pix * a.d + c];
    const float mf = (m && m[pix] == 0) ? 0.f : 1.f;
    return is_f64(a.mode[f]) ? picture_byte(norm_value<double>(a, f, side, p, c, x, mf))
                                       : picture_byte(norm_value<float>(a, f, side, p, c, x, mf));
}

__global__ void __launch_bounds__(kNT) norm_kernel(NormArgs a) {
    const int img = blockIdx.y, side = img / a.np, p = img - side * a.np;
    const float* r = a.res[side];
    if (!r) return;
    r += (size_t)p * (size_t)a.hw * (size_t)a.d;
    const uint8_t* m = a.mask[side] ? a.mask[side] + (size_t)p * (size_t)a.hw : nullptr;
    const int64_t first = (int64_t)blockIdx.x * kNT + threadIdx.x, step = (int64_t)gridDim.x * kNT;
#pragma unroll
    for (int f = 0; f < 2; ++f) {
        if (a.mode[f] == DCN_NORM_NONE) continue;
        // ---- the float image, element by element
        if (a.normed[f]) {
            const int64_t n = a.hw * a.d, base = ((int64_t)side * a.np + p) * n;
            for (int64_t i = first; i < n; i += step) {
                const int64_t pix = i / a.d;
                const int c = (int)(i - pix * a.d);
                const float mf = (m && m[pix] == 0) ? 0.f : 1.f;
                if (is_f64(a.mode[f])) ((double*)a.normed[f])[base + i] = norm_value<double>(a, f, side, p, c, r[i], mf);
                else ((float*)a.normed[f])[base + i] = norm_value<float>(a, f, side, p, c, r[i], mf);
            }
        }
    }
    // ---- the pictures: whole aligned dwords, then the bytes in front of the first and behind the last.  The families' pictures
    // are written in ONE pass over the image: dword number wd of either covers the same elements up to 3 bytes, so the second
    // family's loads hit the lines the first one fetched.
    const int64_t n = a.hw * a.pc;
    uint8_t* pic[2];
    int64_t head[2], words[2];
#pragma unroll
    for (int f = 0; f < 2; ++f) {
        pic[f] = (a.mode[f] != DCN_NORM_NONE && a.picture[f]) ? a.picture[f] + side * a.side_stride[f] + p * a.pair_stride[f]
                                                              : nullptr;
        head[f] = (int64_t)((4 - ((uintptr_t)pic[f] & 3)) & 3);
        if (head[f] > n) head[f] = n;
        words[f] = pic[f] ? (n - head[f]) / 4 : 0;
    }
    const int64_t most = words[0] > words[1] ? words[0] : words[1];
    for (int64_t wd = first; wd < most; wd += step) {
#pragma unroll
        for (int f = 0; f < 2; ++f) {
            if (wd < words[f]) {
                const int64_t b0 = head[f] + 4 * wd;
                unsigned v = 0;
#pragma unroll
                for (int j = 0; j < 4; ++j) v |= norm_byte(a, f, side, p, r, m, b0 + j) << (8 * j);
                *(unsigned*)(pic[f] + b0) = v;
            }
        }
    }
    if (blockIdx.x == 0 && threadIdx.x < 6) {               // at most 3 bytes in front, 3 behind
#pragma unroll
        for (int f = 0; f < 2; ++f) {
            if (!pic[f]) continue;
            const int64_t tail0 = head[f] + 4 * words[f];
            const int64_t b = (int)threadIdx.x < 3 ? (int64_t)threadIdx.x : tail0 + ((int)threadIdx.x - 3);
            const bool mine = (int)threadIdx.x < 3 ? b < head[f] : b < n;
            if (mine) pic[f][b] = (uint8_t)norm_byte(a, f, side, p, r, m, b);
        }
    }
}

// ------------------------------------------------------------------------------------------------ heat maps
constexpr int kHT = 256;    // work-items per workgroup
constexpr int kQT = 64;     // queries staged in LDS at a time

struct HeatArgs {
    const float* res;              // [P][hw][D]
    const float* queries;          // [R][D]
    const int64_t* offsets;        // [P + 1]
    const int32_t* offsets_bad;    // [1] set by check_offsets_kernel
    const uint8_t* table;          // [256][3] or null
    const float* level;            // [kLevels] set by heat_levels_kernel
    uint8_t* out;                  // [R][hw] or [R][hw][3]
    int32_t* status;
    int64_t hw, max_rows;
    float scale;                   // log2(e) / variance
    int d;
};

// uint8(exp(-d / variance) * 255): the quotient and the product in fp32, the exponential in float64 rounded to fp32 once
__device__ __forceinline__ unsigned heat_byte(float dist, float variance) {
    const float q = (-dist) / variance;
    const float e = (float)exp((double)q);
    const float t = e * 255.f;
    return t == t ? (unsigned)(int)(t < 255.f ? t : 255.f) : 0u;   // (a NaN distance: 0; variance <= 0 is refused on the host)
}

// The byte is a non-increasing step function of the SQUARED distance s (sqrtf, the quotient, the exponential rounded once, the
// product and the truncation are each monotone), so it is fixed by 255 thresholds: byte(s) >= k  <=>  s <= level[k].  They are
// found once per launch chain with the exact formula above -- a bisection over the bit patterns of the non-negative floats,
// which order like unsigned integers -- and the float64 exponential, some 30 instructions per pixel and row, leaves the
// inner loop: there a pixel takes an estimate from the hardware's approximate root and exponential, which is at most one level
// off, and two comparisons against the thresholds give the exact byte.
constexpr int kLevels = 257;   // level[0] = +inf (every s), level[1 .. 255], level[256] = -1 (no s)

__global__ void __launch_bounds__(256) heat_levels_kernel(float variance, float* __restrict__ level) {
    const int k = threadIdx.x;
    if (k == 0) {
        level[0] = __builtin_inff();
        level[256] = -1.f;
        return;
    }
    unsigned lo = 0u, hi = 0x7f800000u;                      // byte(0) = 255 >= k; byte(inf) = 0 < k
    while (hi - lo > 1u) {
        const unsigned mid = lo + ((hi - lo) >> 1);
        if (heat_byte(sqrtf(__uint_as_float(mid)), variance) >= (unsigned)k) lo = mid;
        else hi = mid;
    }
    level[k] = __uint_as_float(lo);
}

#if defined(DCN_HOSTEMU_BUILD)
__device__ __forceinline__ float approx_sqrt(float x) { return sqrtf(x); }
__device__ __forceinline__ float approx_exp2(float x) { return exp2f(x); }
#else
__device__ __forceinline__ float approx_sqrt(float x) { return __builtin_amdgcn_sqrtf(x); }
__device__ __forceinline__ float approx_exp2(float x) { return __builtin_amdgcn_exp2f(x); }
#endif

// The byte of the squared distance s from the thresholds in LDS.  scale = log2(e) / variance.
__device__ __forceinline__ unsigned heat_byte_of(float s, float scale, const float* level) {
    const float est = 255.f * approx_exp2(-(approx_sqrt(s) * scale));
    int b = (int)(est < 255.f ? est : 255.f);                // (NaN compares false: 255, corrected below or zeroed)
    b = b < 0 ? 0 : b;
    const float up = level[b + 1], down = level[b];
    b = s <= up ? b + 1 : (s > down ? b - 1 : b);
    return s == s ? (unsigned)b : 0u;
}

typedef unsigned Words4 __attribute__((ext_vector_type(4)));   // (a vector type: the four dwords stay one store)
typedef Words4 Words4A __attribute__((aligned(4)));

// A wavefront's segment of a row: work-item `lane` holds ND dwords w[] = bytes [lane * 4 ND, (lane + 1) * 4 ND) of the segment,
// which starts at the byte address dst (any alignment).  Every aligned dword inside the segment is stored whole -- ND consecutive
// dwords per work-item in one piece --, the at most 3 bytes in front of the first and behind the last one byte by byte.
template <int ND>
__device__ __forceinline__ void store_segment(uint8_t* dst, unsigned (&w)[ND], int lane) {
    const int s = (int)((4 - ((uintptr_t)dst & 3)) & 3);    // bytes in front of the first aligned dword (uniform)
    const unsigned next = __shfl_down(w[0], 1, 64);          // (every work-item takes part)
    unsigned o[ND];
    if (s == 0) {
#pragma unroll
        for (int i = 0; i < ND; ++i) o[i] = w[i];
    } else {
#pragma unroll
        for (int i = 0; i < ND; ++i) o[i] = (w[i] >> (8 * s)) | ((i + 1 < ND ? w[i + 1] : next) << (32 - 8 * s));
    }
    uint8_t* at = dst + s + (size_t)lane * (4 * ND);         // 4-byte aligned
    const bool last = lane == 63 && s != 0;                  // its last dword reaches past the segment
    if (ND % 4 == 0) {                                       // 16-byte pieces (4-byte aligned): ONE vector store each
        const int whole = last ? ND - 4 : ND;
#pragma unroll
        for (int i = 0; i + 4 <= ND; i += 4) {
            if (i < whole) {
                Words4 v = {o[i], o[i + 1], o[i + 2], o[i + 3]};
                *(Words4A*)(at + 4 * i) = v;
            }
        }
        if (last) {
#pragma unroll
            for (int i = (ND >= 4 ? ND - 4 : 0); i < ND - 1; ++i) *(unsigned*)(at + 4 * i) = o[i];
        }
    } else {
#pragma unroll
        for (int i = 0; i < ND; ++i)
            if (!(last && i == ND - 1)) *(unsigned*)(at + 4 * i) = o[i];
    }
    if (s != 0) {
        if (lane == 0) {
            for (int j = 0; j < s; ++j) dst[j] = (uint8_t)(w[0] >> (8 * j));
        }
        if (lane == 63) {                                    // the segment's last 4 - s bytes
            for (int j = s; j < 4; ++j) dst[(size_t)64 * 4 * ND - 4 + j] = (uint8_t)(w[ND - 1] >> (8 * j));
        }
    }
}

// DT: the descriptor dimension kept in registers (0: read from memory per row, any D); K: pixels per work-item (a multiple of
// 4); COLOUR: three bytes per pixel from the table
template <int DT, int K, bool COLOUR>
__global__ void __launch_bounds__(kHT) heat_kernel(HeatArgs a) {
    constexpr int DV = DT > 0 ? DT : 1;
    constexpr int DP = DT > 0 ? ((DT + 3) & ~3) : kMaxD;    // floats per query in LDS
    constexpr int BPP = COLOUR ? 3 : 1;                      // bytes per pixel
    constexpr int ND = K * BPP / 4;                          // dwords per work-item and row
    __shared__ float sq[kQT * DP];
    __shared__ uint8_t stable[COLOUR ? 768 : 4];
    __shared__ float slevel[kLevels];
    const int D = DT > 0 ? DT : a.d;
    const int p = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    int bad = 0, nq;
    int64_t lo;
    pair_rows(a.offsets, a.offsets_bad, p, a.max_rows, 1 << 30, lo, nq, bad);
    if (bad && blockIdx.x == 0 && tid == 0) atomicOr(a.status, bad);
    if (nq == 0) return;                                     // (uniform per workgroup)
    if (COLOUR)
        for (int i = tid; i < 768; i += kHT) stable[i] = a.table[i];
    for (int i = tid; i < kLevels; i += kHT) slevel[i] = a.level[i];   // (the loop below starts with a barrier)
    const int64_t hw = a.hw;
    const int64_t seg0 = ((int64_t)blockIdx.x * (kHT / 64) + wv) * (64 * K);   // the wavefront's segment of 64 K pixels
    const int64_t pix0 = seg0 + (int64_t)lane * K;           // this work-item's pixels: pix0 .. pix0 + K - 1
    const bool full = seg0 + 64 * K <= hw;                    // (uniform per wavefront)
    const float* res = a.res + (size_t)p * hw * D;
    float v[K][DV];
    if (DT > 0) {
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const float* src = res + (pix0 + k < hw ? pix0 + k : hw - 1) * D;   // (past the end: the last pixel, never stored)
#pragma unroll
            for (int c = 0; c < DV; ++c) v[k][c] = src[c];
        }
    }
    for (int q0 = 0; q0 < nq; q0 += kQT) {
        const int qn = min(kQT, nq - q0);
        __syncthreads();
        for (int i = tid; i < qn * D; i += kHT) {
            const int q = i / D;
            sq[q * DP + (i - q * D)] = a.queries[(lo + q0) * D + i];
        }
        __syncthreads();
        if (seg0 >= hw) continue;                            // (uniform per wavefront; it still meets the barriers)
        for (int q = 0; q < qn; ++q) {
            unsigned w[ND];
#pragma unroll
            for (int i = 0; i < ND; ++i) w[i] = 0;
#pragma unroll
            for (int k = 0; k < K; ++k) {
                float d2 = 0.f;
                if (DT > 0) {
#pragma unroll
                    for (int c = 0; c < DV; ++c) { const float t = v[k][c] - sq[q * DP + c]; d2 = fmaf(t, t, d2); }
                } else {
                    const float* src = res + (pix0 + k < hw ? pix0 + k : hw - 1) * D;
                    for (int c = 0; c < D; ++c) { const float t = src[c] - sq[q * DP + c]; d2 = fmaf(t, t, d2); }
                }
                const unsigned b = heat_byte_of(d2, a.scale, slevel);
                if (COLOUR) {
#pragma unroll
                    for (int j = 0; j < 3; ++j) w[(3 * k + j) >> 2] |= (unsigned)stable[3 * b + j] << (8 * ((3 * k + j) & 3));
                } else {
                    w[k >> 2] |= b << (8 * (k & 3));
                }
            }
            uint8_t* row = a.out + (size_t)(lo + q0 + q) * (size_t)hw * BPP;
            if (full) {
                store_segment<ND>(row + seg0 * BPP, w, lane);
            } else {                                         // the image's last, partial segment: byte by byte
#pragma unroll
                for (int j = 0; j < K * BPP; ++j)
                    if (pix0 + j / BPP < hw) row[pix0 * BPP + j] = (uint8_t)(w[j >> 2] >> (8 * (j & 3)));
            }
        }
    }
}

inline bool shape_ok(int p, int h, int w, int d) {
    return p >= 1 && p <= kMaxPairs && h >= 1 && w >= 1 && (int64_t)h * w < ((int64_t)1 << 31) && d >= 1 && d <= kMaxD;
}

template <int DT, int K>
inline void launch_heat(const HeatArgs& a, int p, hipStream_t st) {
    const dim3 grid((unsigned)dcn::ceil_div64(a.hw, (int64_t)kHT * K), (unsigned)p), block(kHT);
    if (a.table) hipLaunchKernelGGL((heat_kernel<DT, K, true>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((heat_kernel<DT, K, false>), grid, block, 0, st, a);
}

}  // namespace

// lohi float [2 p][blocks][4][d] | flags int32 [2 p][blocks][d]
extern "C" size_t dcn_descriptor_ranges_workspace(int p, int h, int w, int d) {
    if (!shape_ok(p, h, w, d)) return 0;
    const size_t nb = (size_t)2 * p * split_image((int64_t)h * w, d).blocks;
    return dcn::align256(nb * 4 * d * sizeof(float)) + dcn::align256(nb * d * sizeof(int32_t));
}

extern "C" int dcn_descriptor_ranges(int p, int h, int w, int d, const float* res_a, const float* res_b, const uint8_t* mask_a,
                                     const uint8_t* mask_b, float* image_ranges, float* pair_ranges, float* scalar_ranges,
                                     int32_t* status, void* workspace, void* stream) {
    if (!shape_ok(p, h, w, d) || !res_a || (mask_a && res_b && !mask_b) || (!mask_a && mask_b) || !image_ranges || !pair_ranges ||
        !scalar_ranges || !status || !workspace)
        return DCN_E_INVALID;
    RangeArgs a;
    a.res[0] = res_a;
    a.res[1] = res_b;
    a.mask[0] = mask_a;
    a.mask[1] = res_b ? mask_b : nullptr;
    a.hw = (int64_t)h * w;
    a.np = p;
    a.d = d;
    const Split sp = split_image(a.hw, d);
    const size_t nb = (size_t)2 * p * sp.blocks;
    a.part_lohi = (float*)workspace;
    a.part_flags = (int32_t*)((char*)workspace + dcn::align256(nb * 4 * d * sizeof(float)));
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(range_partial_kernel, dim3((unsigned)sp.blocks, (unsigned)(res_b ? 2 * p : p)), dim3(kRT), 0, st, a);
    hipLaunchKernelGGL(range_finish_kernel, dim3((unsigned)p), dim3(kFT), 0, st, a, image_ranges, pair_ranges, scalar_ranges,
                       status);
    return dcn::check_launch();
}

extern "C" int dcn_descriptor_normalize(int p, int h, int w, int d, const float* res_a, const float* res_b,
                                        const uint8_t* mask_a, const uint8_t* mask_b, const float* pair_ranges,
                                        const float* scalar_ranges, const struct dcn_picture_family* families, void* stream) {
    if (!shape_ok(p, h, w, d) || !res_a || !families || (mask_a && res_b && !mask_b) || (!mask_a && mask_b)) return DCN_E_INVALID;
    NormArgs a;
    a.res[0] = res_a;
    a.res[1] = res_b;
    a.mask[0] = mask_a;
    a.mask[1] = res_b ? mask_b : nullptr;
    a.pair_ranges = pair_ranges;
    a.scalar_ranges = scalar_ranges;
    a.hw = (int64_t)h * w;
    a.np = p;
    a.d = d;
    a.pc = 0;
    bool any = false;
    for (int f = 0; f < 2; ++f) {
        const dcn_picture_family& fam = families[f];
        a.mode[f] = fam.mode;
        a.stats[f] = fam.stats;
        a.normed[f] = fam.normed;
        a.picture[f] = (uint8_t*)fam.picture;
        a.side_stride[f] = fam.side_stride;
        a.pair_stride[f] = fam.pair_stride;
        if (fam.mode == DCN_NORM_NONE) continue;
        if (!fam.normed && !fam.picture) return DCN_E_INVALID;
        any = true;
        switch (fam.mode) {
            case DCN_NORM_PAIR: if (!pair_ranges) return DCN_E_INVALID; break;
            case DCN_NORM_MASKED_PAIR: if (!pair_ranges || !mask_a) return DCN_E_INVALID; break;
            case DCN_NORM_STATS: if (!fam.stats) return DCN_E_INVALID; break;
            case DCN_NORM_STATS_MASKED: if (!fam.stats || !mask_a) return DCN_E_INVALID; break;
            case DCN_NORM_SCALAR: if (!scalar_ranges) return DCN_E_INVALID; break;
            default: return DCN_E_INVALID;
        }
        if (fam.picture) {
            const int pc = fam.picture_channels;
            if ((pc != 1 && pc != 3) || (a.pc && a.pc != pc)) return DCN_E_INVALID;
            a.pc = pc;
            for (int j = 0; j < 3; ++j) {
                const int ch = j < pc ? fam.channel[j] : 0;
                if (ch < 0 || ch >= d || (f == 1 && a.picture[0] && ch != a.channel[j])) return DCN_E_INVALID;
                a.channel[j] = ch;
            }
        }
    }
    if (!any) return DCN_E_INVALID;
    if (!a.pc) {
        a.pc = 1;
        a.channel[0] = a.channel[1] = a.channel[2] = 0;
    }
    const int64_t units = a.hw * (d > a.pc ? d : a.pc);
    int blocks = (int)dcn::ceil_div64(units, (int64_t)kNT * 4);
    if (blocks > kNormBlocks) blocks = kNormBlocks;
    hipLaunchKernelGGL(norm_kernel, dim3((unsigned)blocks, (unsigned)(res_b ? 2 * p : p)), dim3(kNT), 0, (hipStream_t)stream, a);
    return dcn::check_launch();
}

extern "C" int dcn_heat_maps(int p, int h, int w, int d, const float* res_b, const float* queries, const int64_t* offsets,
                             int64_t max_rows, float variance, const uint8_t* colour_table, uint8_t* out, int32_t* status,
                             void* workspace, void* stream) {
    if (!shape_ok(p, h, w, d) || !res_b || !queries || !offsets || max_rows < 1 || !(variance > 0.f) || !out || !status ||
        !workspace)
        return DCN_E_INVALID;
    hipStream_t st = (hipStream_t)stream;
    int32_t* flag = (int32_t*)workspace;
    int rc = dcn::fill_bytes_async(status, 0, sizeof(int32_t), st);
    if (rc == DCN_OK) rc = dcn::fill_bytes_async(flag, 0, sizeof(int32_t), st);
    if (rc != DCN_OK) return rc;
    hipLaunchKernelGGL(check_offsets_kernel, dim3(dcn::ceil_div(p, 256)), dim3(256), 0, st, offsets, p, max_rows, flag, status);
    HeatArgs a;
    a.res = res_b;
    a.queries = queries;
    a.offsets = offsets;
    a.offsets_bad = flag;
    a.table = colour_table;
    a.out = out;
    a.status = status;
    a.hw = (int64_t)h * w;
    a.max_rows = max_rows;
    a.level = (const float*)((char*)workspace + 256);
    a.scale = (float)(1.4426950408889634 / (double)variance);
    hipLaunchKernelGGL(heat_levels_kernel, dim3(1), dim3(256), 0, st, variance, (float*)((char*)workspace + 256));
    a.d = d;
    switch (d) {                                            // pixels per work-item: at most 64 floats of res_b in registers
        case 1: launch_heat<1, 16>(a, p, st); break;
        case 3: launch_heat<3, 16>(a, p, st); break;
        case 4: launch_heat<4, 16>(a, p, st); break;
        case 8: launch_heat<8, 8>(a, p, st); break;
        case 16: launch_heat<16, 4>(a, p, st); break;
        default: launch_heat<0, 4>(a, p, st); break;
    }
    return dcn::check_launch();
}
