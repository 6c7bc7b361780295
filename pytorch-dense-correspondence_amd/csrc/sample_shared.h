// The device functions, kernels and launch helpers the sample builders share: sample_kernels.hip (include/dcn_hip.h sections 9
// and 11a) and synthetic_kernels.hip (section 9a).  One text for the random numbers (`uniform`), `pick`, the ordered compaction,
// the within-scene candidate / match kernels and the writer of the concatenated lists; every translation unit that includes
// this header gets its own copy of the kernels (internal linkage).
#pragma once
#include "dcn_common.h"
#include "hashed_order.h"
#include "pairgen_project.h"

namespace {

enum Src { SRC_A0 = 0, SRC_B0 = 1, SRC_FLAGS = 2, SRC_BLIND = 3, SRC_MB = 4, SRC_MBINV = 5, NSRC = 6 };
enum Site { SITE_CAND = 0, SITE_MASKED = 1, SITE_BACKGROUND = 2, SITE_BLIND = 3, SITE_ACROSS_A = 4, SITE_ACROSS_B = 5 };

constexpr int kThreads = 256;
constexpr int kPer = 16;                       // elements per work-item and segment
constexpr int kSeg = kThreads * kPer;          // elements per segment
constexpr int kWaves = kThreads / dcn::kWave;
constexpr int kMaxPairs = 1024;                // the writer keeps 4n + 1 offsets in LDS
constexpr int kRun = 4;                        // output entries per work-item of the writer
struct alignas(16) I64x2 {
    int64_t x, y;
};

struct Draws {
    const int64_t* seeds;          // [n] or null (replay)
    const float* rand;             // replay values
    const int64_t* roff;           // [kSites][n + 1] offsets into rand
    int n;
};

using dcn::mix32;

// Uniform number `idx` of stream `site` of pair p: the hash of (seed, site, idx) on torch.rand's grid (k / 2^24), or the
// caller's value; a replay stream that is too short reads 0 and raises DCN_SAMPLE_BAD_DRAWS.
__device__ __forceinline__ float uniform(const Draws& d, int p, int site, int64_t idx, int& bad) {
    if (d.seeds) {
        const uint64_t s = (uint64_t)d.seeds[p];
        const uint32_t k0 = mix32((uint32_t)s ^ mix32((uint32_t)site * 0x9E3779B9U + 0x7F4A7C15U));
        const uint32_t k1 = mix32((uint32_t)(s >> 32) ^ k0);
        const uint32_t r = mix32(mix32((uint32_t)idx ^ k0) ^ (k1 + (uint32_t)(idx >> 32)));
        return (float)(r >> 8) * (1.0f / 16777216.0f);
    }
    const int64_t* o = d.roff + (size_t)site * (d.n + 1);
    const int64_t lo = o[p], hi = o[p + 1];
    if (idx < 0 || lo + idx >= hi) {
        bad |= DCN_SAMPLE_BAD_DRAWS;
        return 0.f;
    }
    return d.rand[lo + idx];
}

// list[floor(r * count)] (random_sample_from_masked_image_torch, :92-121; create_non_correspondences, :319-324)
__device__ __forceinline__ int64_t pick(const int32_t* list, int64_t count, float r) {
    int64_t j = (int64_t)floorf(r * (float)count);
    j = j < 0 ? 0 : (j >= count ? count - 1 : j);      // (r < 1: only a rounding of r * count up to count reaches the clamp)
    return list[j];
}

__device__ __forceinline__ uint32_t flips_of(const int32_t* params, int rec) {
    return params ? (uint32_t)params[(size_t)rec * DCN_AUG_PARAM_WORDS] & (DCN_AUG_FLIP_V | DCN_AUG_FLIP_H) : 0u;
}

struct Common {
    const uint8_t* mask_a;         // [n][hw] 0/1, unrotated
    const uint8_t* mask_b;
    const uint8_t* mask_b_or;      // null, or a second mask b: the pair's mask b is (mask_b | mask_b_or) != 0 (a merged mask)
    const int32_t* params;         // [2n][DCN_AUG_PARAM_WORDS]: a's records, then b's (flips), or null
    int32_t* lists;                // workspace [NSRC - src0][n][ls] compacted element indices (ls = max(hw, attempts))
    int64_t* counts;               // workspace [NSRC - src0][n]
    int32_t* seg;                  // workspace [NSRC - src0][n][segs] per-segment counts
    const uint8_t* flags;          // workspace [n][attempts]
    const uint8_t* matched;        // workspace [n][hw]
    int n, h, w, segs;
    int64_t hw, attempts, ls;
    uint32_t src_mask;             // the sources compacted by this launch pair
    int src0;                      // the first source the workspace arrays hold (0: all of them)
};

// Row of (source s, pair p) in the workspace arrays
__device__ __forceinline__ size_t src_row(const Common& c, int s, int p) { return (size_t)(s - c.src0) * c.n + p; }

__device__ __forceinline__ int64_t src_len(const Common& c, int s) { return s == SRC_FLAGS ? c.attempts : c.hw; }

// Predicate of element e of source s, pair p
__device__ __forceinline__ uint32_t pred(const Common& c, int s, int p, int64_t e) {
    if (s == SRC_FLAGS) return c.flags[(size_t)p * c.attempts + e] != 0;
    if (s == SRC_A0) return c.mask_a[(size_t)p * c.hw + e] != 0;
    if (s == SRC_B0) return c.mask_b[(size_t)p * c.hw + e] != 0;
    // the rotated mask of the pair's record: output pixel (y, x) shows source pixel (fv ? h-1-y : y, fh ? w-1-x : x)
    const bool side_b = s != SRC_BLIND;
    const uint32_t f = flips_of(c.params, side_b ? c.n + p : p);
    const int64_t y = e / c.w, x = e - y * c.w;
    const int64_t sy = (f & DCN_AUG_FLIP_V) ? c.h - 1 - y : y, sx = (f & DCN_AUG_FLIP_H) ? c.w - 1 - x : x;
    uint32_t m = (side_b ? c.mask_b : c.mask_a)[(size_t)p * c.hw + sy * c.w + sx] != 0;
    if (side_b && c.mask_b_or) m |= c.mask_b_or[(size_t)p * c.hw + sy * c.w + sx] != 0;
    if (s == SRC_BLIND) return m != (uint32_t)c.matched[(size_t)p * c.hw + e];   // mask_a - matched != 0
    return s == SRC_MB ? m : 1u - m;
}

// grid (segs, n * NSRC): bitmask of the 16 elements of this work-item; the segment's count to seg[]
__global__ void __launch_bounds__(kThreads) compact_count_kernel(Common c) {
    __shared__ int32_t scratch[kWaves];
    const int s = blockIdx.y / c.n, p = blockIdx.y - s * c.n;
    if (!((c.src_mask >> s) & 1u)) return;
    const int64_t len = src_len(c, s), e0 = (int64_t)blockIdx.x * kSeg + (int64_t)threadIdx.x * kPer;
    if ((int64_t)blockIdx.x * kSeg >= len) {
        if (threadIdx.x == 0) c.seg[src_row(c, s, p) * c.segs + blockIdx.x] = 0;
        return;
    }
    int32_t cnt = 0;
    for (int k = 0; k < kPer; ++k)
        if (e0 + k < len) cnt += (int32_t)pred(c, s, p, e0 + k);
    cnt = dcn::block_sum<kThreads>(cnt, scratch);
    if (threadIdx.x == 0) c.seg[src_row(c, s, p) * c.segs + blockIdx.x] = cnt;
}

// grid (segs, n * NSRC): this segment's elements to lists[s][p][base + rank], in order; the last segment writes the count.
__global__ void __launch_bounds__(kThreads) compact_write_kernel(Common c) {
    __shared__ int32_t scratch[kWaves];
    __shared__ int32_t wave_tot[kWaves];
    __shared__ int32_t base_s;
    const int s = blockIdx.y / c.n, p = blockIdx.y - s * c.n;
    if (!((c.src_mask >> s) & 1u)) return;
    const int64_t len = src_len(c, s), e0 = (int64_t)blockIdx.x * kSeg + (int64_t)threadIdx.x * kPer;
    const int32_t* seg = c.seg + src_row(c, s, p) * c.segs;
    // 1. elements before this segment (and, in the last segment, in all of them)
    int32_t before = 0;
    for (int q = threadIdx.x; q < (int)blockIdx.x; q += kThreads) before += seg[q];
    before = dcn::block_sum<kThreads>(before, scratch);
    if (threadIdx.x == 0) base_s = before;
    if ((int64_t)blockIdx.x * kSeg >= len) return;                 // (uniform per workgroup)
    // 2. this work-item's elements and its rank among the workgroup's
    uint32_t bits = 0;
    for (int k = 0; k < kPer; ++k)
        if (e0 + k < len && pred(c, s, p, e0 + k)) bits |= 1u << k;
    const int32_t mine = __builtin_popcount(bits);
    const int lane = threadIdx.x & (dcn::kWave - 1), wv = threadIdx.x / dcn::kWave;
    int32_t incl = mine;                                           // inclusive scan over the wave
#pragma unroll
    for (int off = 1; off < dcn::kWave; off <<= 1) {
        const int32_t t = __shfl(incl, lane >= off ? lane - off : 0, dcn::kWave);
        if (lane >= off) incl += t;
    }
    __syncthreads();
    if (lane == dcn::kWave - 1) wave_tot[wv] = incl;
    __syncthreads();
    int32_t pos = base_s + incl - mine, total = base_s;
    for (int q = 0; q < kWaves; ++q) {
        if (q < wv) pos += wave_tot[q];
        total += wave_tot[q];
    }
    int32_t* out = c.lists + src_row(c, s, p) * c.ls;
    for (int k = 0; k < kPer; ++k)
        if ((bits >> k) & 1u) out[pos++] = (int32_t)(e0 + k);
    if (threadIdx.x == 0 && (int64_t)(blockIdx.x + 1) * kSeg >= len) c.counts[src_row(c, s, p)] = total;
}

struct CandArgs {
    const uint16_t* depth_a;       // [n][hw]
    const uint16_t* depth_b;
    const float* cams;             // [n][DCN_SAMPLE_CAM_FLOATS]: K, K^-1, pose a, pose b^-1
    Draws d;
    uint8_t* flags;                // [n][attempts]
    float* u2;                     // [n][attempts]
    float* v2;
    int32_t* pix;                  // [n][attempts] flat candidate pixel
    const int32_t* list_a;         // [n][ls] mask a's pixels
    const int64_t* count_a;        // [n]
    int32_t* status;
    int64_t attempts, hw, ls;
    int n, h, w, from_mask;
};

// Candidate i of pair p, drawn from stream `site`: a pixel of the mask's list (`from_mask`; none, u = v = -1, when the mask
// is empty) or uniform over the image
__device__ __forceinline__ void draw_candidate(const Draws& d, int p, int site, int64_t i, int64_t attempts, int from_mask,
                                               const int32_t* list, int64_t cnt, int h, int w, int64_t& u, int64_t& v, int& bad) {
    u = v = -1;
    if (from_mask) {
        if (cnt > 0) {
            const int64_t px = pick(list, cnt, uniform(d, p, site, i, bad));
            u = px % w;
            v = px / w;
        }
    } else {                                                        // pytorch_rand_select_pixel (:29-34): torch.rand(2, A)
        u = (int64_t)floorf(uniform(d, p, site, i, bad) * (float)w);
        v = (int64_t)floorf(uniform(d, p, site, attempts + i, bad) * (float)h);
    }
}

// grid (ceil(attempts / 256), n)
__global__ void __launch_bounds__(kThreads) candidate_kernel(CandArgs a) {
    const int p = blockIdx.y;
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= a.attempts) return;
    int bad = 0;
    int64_t u, v;
    draw_candidate(a.d, p, SITE_CAND, i, a.attempts, a.from_mask, a.list_a + (size_t)p * a.ls, a.from_mask ? a.count_a[p] : 0,
                   a.h, a.w, u, v, bad);
    const float* cam = a.cams + (size_t)p * DCN_SAMPLE_CAM_FLOATS;
    float u2 = 0.f, v2 = 0.f;
    unsigned char ok = 0;
    if (u >= 0)
        ok = dcn::project_candidate(a.depth_a + (size_t)p * a.hw, a.depth_b + (size_t)p * a.hw, a.h, a.w, cam, cam + 9,
                                    cam + 18, cam + 34, u, v, u2, v2);
    const size_t k = (size_t)p * a.attempts + i;
    a.flags[k] = ok;
    a.u2[k] = u2;
    a.v2[k] = v2;
    a.pix[k] = (int32_t)(u >= 0 ? v * a.w + u : 0);
    if (bad) atomicOr(a.status, bad);
}

struct MatchArgs {
    const int32_t* sel;            // [n][ls]-strided lists of SRC_FLAGS: kept candidate indices
    const int64_t* count;          // [n] kept candidates
    const int32_t* pix;
    const float* u2;
    const float* v2;
    // import mode (complete_samples): external lists, pair p at [off[p], off[p+1])
    const int64_t *ua, *va;
    const void *ub, *vb;
    const int64_t* off;
    int64_t ext_count;
    int ub_float;
    const int32_t* params;
    int64_t* ma;                   // [n][stride] flattened a index of match e of pair p
    int64_t* mb;
    int64_t* mcount;               // [n]
    uint8_t* matched;              // [n][hw]
    int32_t* status;
    int64_t attempts, hw, stride, ls;
    int n, h, w;
};

__device__ __forceinline__ void flip_pixel(uint32_t f, int h, int w, int64_t& u, int64_t& v) {
    if (f & DCN_AUG_FLIP_H) u = (int64_t)(w - 1) - u;
    if (f & DCN_AUG_FLIP_V) v = (int64_t)(h - 1) - v;
}

// grid (ceil(stride / 256), n): match e of pair p after the pair's rotation (flip_uv's arithmetic: int64 for a, float32
// (W-1) - u for b, then `.long()`), flattened v * W + u, and the matched map of the rotated image a.
__global__ void __launch_bounds__(kThreads) match_kernel(MatchArgs a) {
    const int p = blockIdx.y;
    const int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    int64_t cnt, ua, va;
    float ub, vb;
    const uint32_t fa = flips_of(a.params, p), fb = flips_of(a.params, a.n + p);
    if (a.off) {
        int64_t lo = a.off[p], hi = a.off[p + 1];
        if (lo < 0 || hi < lo || hi > a.ext_count) {
            if (e == 0) {
                atomicOr(a.status, DCN_SAMPLE_BAD_OFFSETS);
                a.mcount[p] = 0;
            }
            return;
        }
        cnt = hi - lo;
        if (e == 0) a.mcount[p] = cnt;
        if (e >= cnt) return;
        ua = a.ua[lo + e];
        va = a.va[lo + e];
        if (a.ub_float) {
            ub = ((const float*)a.ub)[lo + e];
            vb = ((const float*)a.vb)[lo + e];
        } else {
            ub = (float)((const int64_t*)a.ub)[lo + e];
            vb = (float)((const int64_t*)a.vb)[lo + e];
        }
        if (ua < 0 || ua >= a.w || va < 0 || va >= a.h || !(ub > -1.f && ub < (float)a.w) || !(vb > -1.f && vb < (float)a.h)) {
            atomicOr(a.status, DCN_SAMPLE_BAD_INDEX);   // the entry stays in its list: both indices clamp to pixel 0
            ua = va = 0;
            ub = vb = 0.f;
        }
    } else {
        cnt = a.count[p];
        if (e == 0) a.mcount[p] = cnt;
        if (e >= cnt) return;
        const int64_t k = (int64_t)p * a.attempts + a.sel[(size_t)p * a.ls + e];
        const int64_t px = a.pix[k];
        ua = px % a.w;
        va = px / a.w;
        ub = a.u2[k];
        vb = a.v2[k];
    }
    flip_pixel(fa, a.h, a.w, ua, va);
    if (fb & DCN_AUG_FLIP_H) ub = (float)(a.w - 1) - ub;
    if (fb & DCN_AUG_FLIP_V) vb = (float)(a.h - 1) - vb;
    const size_t o = (size_t)p * a.stride + e;
    const int64_t fa_idx = va * a.w + ua;
    a.ma[o] = fa_idx;
    a.mb[o] = (int64_t)vb * a.w + (int64_t)ub;                     // flatten_uv_tensor: v.long() * W + u.long()
    a.matched[(size_t)p * a.hw + fa_idx] = 1;                      // (racing writes of the same value)
}

struct OutArgs {
    const int64_t* counts;         // [NSRC][n]
    const int64_t* mcount;         // [n] matches (within)
    const int64_t* ma;
    const int64_t* mb;
    const int32_t* lists;          // [NSRC][n][ls]
    const int32_t* params;
    Draws d;
    int64_t* offsets;              // [4n + 1]
    uint8_t* empty;                // [n]
    int32_t* type;                 // [n]
    int32_t* status;
    int64_t* idx_a;                // [cap]
    int64_t* idx_b;
    int64_t cap, hw, stride, samples, ls;
    int n, h, w, k1, k2, across, inv, data_type;
    int site_masked, site_background;   // the streams of the masked / background non-matches
};

// one workgroup: lengths of the 4n lists -> offsets, empty, type (the writer reads them back)
__global__ void __launch_bounds__(1024) offsets_kernel(OutArgs a) {
    __shared__ int64_t part[1024 / dcn::kWave];
    __shared__ int64_t carry;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    for (int p0 = 0; p0 < a.n; p0 += 1024) {
        const int p = p0 + threadIdx.x;
        int64_t len[4] = {0, 0, 0, 0};
        if (p < a.n) {
            bool ok;
            if (a.across) {
                ok = a.counts[(size_t)SRC_A0 * a.n + p] > 0 && a.counts[(size_t)SRC_B0 * a.n + p] > 0;
                len[3] = ok ? a.samples : 0;
            } else {
                const int64_t m = a.mcount[p], nb = a.counts[(size_t)SRC_BLIND * a.n + p],
                              cb = a.counts[(size_t)SRC_MB * a.n + p];
                ok = m > 0;
                if (ok) {
                    len[0] = m;
                    len[1] = m * a.k1;
                    len[2] = m * a.k2;
                    len[3] = (nb > 0 && cb > 0) ? nb : 0;
                }
            }
            a.empty[p] = ok ? 0 : 1;
            a.type[p] = ok ? a.data_type : -1;
        }
        const int64_t tot = len[0] + len[1] + len[2] + len[3];
        // exclusive scan of `tot` over the workgroup
        const int lane = threadIdx.x & (dcn::kWave - 1), wv = threadIdx.x / dcn::kWave;
        int64_t incl = tot;
#pragma unroll
        for (int off = 1; off < dcn::kWave; off <<= 1) {
            const int64_t t = __shfl(incl, lane >= off ? lane - off : 0, dcn::kWave);
            if (lane >= off) incl += t;
        }
        if (lane == dcn::kWave - 1) part[wv] = incl;
        __syncthreads();
        int64_t pos = carry + incl - tot, all = carry;
        for (int q = 0; q < 1024 / dcn::kWave; ++q) {
            if (q < wv) pos += part[q];
            all += part[q];
        }
        if (p < a.n)
            for (int t = 0; t < 4; ++t) {
                a.offsets[4 * p + t] = pos;
                pos += len[t];
            }
        __syncthreads();
        if (threadIdx.x == 0) carry = all;
        __syncthreads();
    }
    if (threadIdx.x == 0) a.offsets[4 * a.n] = carry;
}

// Entry e of list t of pair p -> (a, b) flattened pixel indices
__device__ __forceinline__ void entry(const OutArgs& a, int p, int t, int64_t e, int64_t& ia, int64_t& ib, int& bad) {
    const size_t n = a.n;
    const int32_t* lists = a.lists;
    auto list = [&](int s) { return lists + ((size_t)s * n + p) * a.ls; };
    auto count = [&](int s) { return a.counts[(size_t)s * n + p]; };
    if (a.across) {                   // blind slot: mask samples of the unrotated masks, then rotated (:1085-1107)
        int64_t px = pick(list(SRC_A0), count(SRC_A0), uniform(a.d, p, SITE_ACROSS_A, e, bad));
        int64_t u = px % a.w, v = px / a.w;
        flip_pixel(flips_of(a.params, p), a.h, a.w, u, v);
        ia = v * a.w + u;
        px = pick(list(SRC_B0), count(SRC_B0), uniform(a.d, p, SITE_ACROSS_B, e, bad));
        u = px % a.w;
        v = px / a.w;
        flip_pixel(flips_of(a.params, (int)n + p), a.h, a.w, u, v);
        ib = v * a.w + u;
        return;
    }
    const size_t mo = (size_t)p * a.stride;
    if (t == 0) {
        ia = a.ma[mo + e];
        ib = a.mb[mo + e];
        return;
    }
    if (t == 3) {                     // blind: (mask_a - matched).nonzero(), b from mask b's pixels (:735-771)
        ia = list(SRC_BLIND)[e];
        ib = pick(list(SRC_MB), count(SRC_MB), uniform(a.d, p, SITE_BLIND, e, bad));
        return;
    }
    // masked (t = 1) / background (t = 2): a = match e / k repeated k times in a row (create_non_matches, :841-858); b from
    // mask b's (1 - mask b's) pixels, or uniform over the image when that set is empty / not used (:276-405)
    const int k = t == 1 ? a.k1 : a.k2;
    const int site = t == 1 ? a.site_masked : a.site_background;
    ia = a.ma[mo + e / k];
    const int s = t == 1 ? SRC_MB : SRC_MBINV;
    const int64_t c = (t == 1 || a.inv) ? count(s) : 0;
    if (c > 0) {
        ib = pick(list(s), c, uniform(a.d, p, site, e, bad));
    } else {
        const int64_t nn = a.mcount[p] * k;
        const int64_t u = (int64_t)floorf(uniform(a.d, p, site, e, bad) * (float)a.w);
        const int64_t v = (int64_t)floorf(uniform(a.d, p, site, nn + e, bad) * (float)a.h);
        ib = v * a.w + u;
    }
}

// grid-stride over the capacity, kRun consecutive entries per work-item
__global__ void __launch_bounds__(kThreads) write_kernel(OutArgs a) {
    __shared__ int64_t off[4 * kMaxPairs + 1];
    const int nl = 4 * a.n;
    for (int i = threadIdx.x; i <= nl; i += kThreads) off[i] = a.offsets[i];
    __syncthreads();
    const int64_t total = off[nl];
    int bad = 0;
    for (int64_t i0 = ((int64_t)blockIdx.x * kThreads + threadIdx.x) * kRun; i0 < a.cap;
         i0 += (int64_t)gridDim.x * kThreads * kRun) {
        int64_t va[kRun], vb[kRun];
        // list l of the first entry: the largest l with off[l] <= i0 (then walk forward)
        int l = 0;
        if (i0 < total) {
            int lo = 0, hi = nl - 1;
            while (lo < hi) {
                const int mid = (lo + hi + 1) >> 1;
                if (off[mid] <= i0) lo = mid; else hi = mid - 1;
            }
            l = lo;
        }
#pragma unroll
        for (int r = 0; r < kRun; ++r) {
            const int64_t i = i0 + r;
            va[r] = vb[r] = -1;
            if (i < total) {
                while (off[l + 1] <= i) ++l;
                entry(a, l >> 2, l & 3, i - off[l], va[r], vb[r], bad);
            }
        }
        if (i0 + kRun <= a.cap) {
            int64_t* pa = a.idx_a + i0;
            int64_t* pb = a.idx_b + i0;
            *reinterpret_cast<I64x2*>(pa) = I64x2{va[0], va[1]};
            *reinterpret_cast<I64x2*>(pa + 2) = I64x2{va[2], va[3]};
            *reinterpret_cast<I64x2*>(pb) = I64x2{vb[0], vb[1]};
            *reinterpret_cast<I64x2*>(pb + 2) = I64x2{vb[2], vb[3]};
        } else {
            for (int r = 0; r < kRun && i0 + r < a.cap; ++r) {
                a.idx_a[i0 + r] = va[r];
                a.idx_b[i0 + r] = vb[r];
            }
        }
    }
    if (bad) atomicOr(a.status, bad);
}

using dcn::align256;

struct Workspace {
    int32_t *lists, *seg, *pix;
    int64_t *counts, *mcount, *ma, *mb;
    uint8_t *flags, *matched;
    float *u2, *v2;
};

// The stride of the compacted lists: a source has hw elements (a mask) or `attempts` (the candidate flags)
inline int64_t list_stride(int64_t hw, int64_t attempts) { return hw > attempts ? hw : attempts; }

inline int segs_of(int64_t hw, int64_t attempts) { return (int)dcn::ceil_div64(list_stride(hw, attempts), kSeg); }

// stride: match slots per pair (within: attempts; complete: the external lists' total)
inline size_t carve(Workspace* w, char* base, int n, int64_t hw, int64_t attempts, int64_t stride) {
    stride = stride > 0 ? stride : 1;
    size_t o = 0;
    auto take = [&](size_t bytes) { const size_t at = o; o += align256(bytes); return base ? base + at : nullptr; };
    char* p;
    p = take((size_t)NSRC * n * list_stride(hw, attempts) * 4); if (w) w->lists = (int32_t*)p;
    p = take((size_t)NSRC * n * segs_of(hw, attempts) * 4); if (w) w->seg = (int32_t*)p;
    p = take((size_t)NSRC * n * 8);                    if (w) w->counts = (int64_t*)p;
    p = take((size_t)n * 8);                           if (w) w->mcount = (int64_t*)p;
    p = take((size_t)n * attempts * 4);                if (w) w->pix = (int32_t*)p;
    p = take((size_t)n * attempts * 4);                if (w) w->u2 = (float*)p;
    p = take((size_t)n * attempts * 4);                if (w) w->v2 = (float*)p;
    p = take((size_t)n * attempts);                    if (w) w->flags = (uint8_t*)p;
    p = take((size_t)n * stride * 8);                  if (w) w->ma = (int64_t*)p;
    p = take((size_t)n * stride * 8);                  if (w) w->mb = (int64_t*)p;
    p = take((size_t)n * hw);                          if (w) w->matched = (uint8_t*)p;
    return o;
}

inline void compact(Common c, uint32_t src_mask, hipStream_t st) {
    c.src_mask = src_mask;
    const dim3 grid((unsigned)c.segs, (unsigned)(NSRC * c.n));
    hipLaunchKernelGGL(compact_count_kernel, grid, dim3(kThreads), 0, st, c);
    hipLaunchKernelGGL(compact_write_kernel, grid, dim3(kThreads), 0, st, c);
}

inline void write_out(OutArgs o, hipStream_t st) {
    hipLaunchKernelGGL(offsets_kernel, dim3(1), dim3(1024), 0, st, o);
    int64_t blocks = dcn::ceil_div64(dcn::ceil_div64(o.cap, kRun), kThreads);
    blocks = blocks < 1 ? 1 : (blocks > 2048 ? 2048 : blocks);
    hipLaunchKernelGGL(write_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, st, o);
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

inline bool shape_ok(int n, int h, int w) {
    return n >= 1 && n <= kMaxPairs && h >= 1 && w >= 1 && (int64_t)h * w < (1LL << 30) && (int64_t)NSRC * n <= 65535;
}

// ---- the clauses the entry points' argument tests are built from
inline bool random_source_ok(const int64_t* seeds, const float* rand, const int64_t* rand_offsets) {
    return seeds || (rand && rand_offsets);
}

// the five outputs, the status word and the workspace are there, and the lists take the writer's 16-byte stores
inline bool outputs_ok(const int64_t* idx_a, const int64_t* idx_b, const int64_t* offsets, const uint8_t* empty,
                       const int32_t* type, const int32_t* status, const void* workspace) {
    return idx_a && idx_b && offsets && empty && type && status && workspace && aligned16(idx_a) && aligned16(idx_b);
}

// The opening fills: the status word and, where matches are marked, the matched plane [n][hw] (to its 256-byte boundary)
inline int begin(int32_t* status, uint8_t* matched, int n, int64_t hw, hipStream_t st) {
    int rc = dcn::fill_bytes_async(status, 0, 4, st);
    if (rc == DCN_OK && matched) rc = dcn::fill_bytes_async(matched, 0, align256((size_t)n * hw), st);
    return rc;
}

inline Draws draws_of(int n, const int64_t* seeds, const float* rand, const int64_t* rand_offsets) {
    Draws d;
    d.seeds = seeds;
    d.rand = rand;
    d.roff = rand_offsets;
    d.n = n;
    return d;
}

inline Common common_of(const Workspace& ws, int n, int h, int w, int64_t attempts, const uint8_t* mask_a, const uint8_t* mask_b,
                        const int32_t* params) {
    Common c;
    c.mask_a = mask_a;
    c.mask_b = mask_b;
    c.params = params;
    c.lists = ws.lists;
    c.counts = ws.counts;
    c.seg = ws.seg;
    c.flags = ws.flags;
    c.matched = ws.matched;
    c.n = n;
    c.h = h;
    c.w = w;
    c.hw = (int64_t)h * w;
    c.attempts = attempts;
    c.ls = list_stride(c.hw, attempts);
    c.segs = segs_of(c.hw, attempts);
    c.src_mask = 0;
    c.src0 = 0;
    c.mask_b_or = nullptr;
    return c;
}

inline CandArgs cand_of(const Workspace& ws, const Common& c, const uint16_t* depth_a, const uint16_t* depth_b, const float* cams,
                        Draws d, int32_t* status, int from_mask) {
    CandArgs ca;
    ca.depth_a = depth_a;
    ca.depth_b = depth_b;
    ca.cams = cams;
    ca.d = d;
    ca.flags = ws.flags;
    ca.u2 = ws.u2;
    ca.v2 = ws.v2;
    ca.pix = ws.pix;
    ca.list_a = ws.lists + (size_t)SRC_A0 * c.n * c.ls;
    ca.count_a = ws.counts + (size_t)SRC_A0 * c.n;
    ca.status = status;
    ca.attempts = c.attempts;
    ca.hw = c.hw;
    ca.ls = c.ls;
    ca.n = c.n;
    ca.h = c.h;
    ca.w = c.w;
    ca.from_mask = from_mask;
    return ca;
}

// mask a's pixel list (when the candidates come from it), the candidates, then the list of those that passed
inline void find_candidates(const Common& c, const CandArgs& ca, hipStream_t st) {
    if (ca.from_mask) compact(c, 1u << SRC_A0, st);
    hipLaunchKernelGGL(candidate_kernel, dim3((unsigned)dcn::ceil_div64(c.attempts, kThreads), (unsigned)c.n), dim3(kThreads), 0,
                       st, ca);
    compact(c, 1u << SRC_FLAGS, st);
}

// The writer's arguments, within / complete form: `stride` match slots per pair in ma / mb, k1 / k2 non-matches per match,
// `inv`: the background non-matches from 1 - mask b
inline OutArgs out_of(const Workspace& ws, const Common& c, Draws d, int64_t* idx_a, int64_t* idx_b, int64_t cap, int64_t* offsets,
                      uint8_t* empty, int32_t* type, int32_t* status, int data_type, int64_t stride, int k1, int k2, int inv) {
    OutArgs o;
    o.counts = ws.counts;
    o.mcount = ws.mcount;
    o.ma = ws.ma;
    o.mb = ws.mb;
    o.lists = ws.lists;
    o.params = c.params;
    o.d = d;
    o.offsets = offsets;
    o.empty = empty;
    o.type = type;
    o.status = status;
    o.idx_a = idx_a;
    o.idx_b = idx_b;
    o.cap = cap;
    o.hw = c.hw;
    o.ls = c.ls;
    o.stride = stride;
    o.samples = 0;
    o.n = c.n;
    o.h = c.h;
    o.w = c.w;
    o.k1 = k1;
    o.k2 = k2;
    o.across = 0;
    o.inv = inv;
    o.data_type = data_type;
    o.site_masked = SITE_MASKED;
    o.site_background = SITE_BACKGROUND;
    return o;
}

// ... across form: `samples` pixels of each mask in the blind slot, nothing else
inline OutArgs across_of(const Workspace& ws, const Common& c, Draws d, int64_t* idx_a, int64_t* idx_b, int64_t cap,
                         int64_t* offsets, uint8_t* empty, int32_t* type, int32_t* status, int data_type, int64_t samples) {
    OutArgs o = out_of(ws, c, d, idx_a, idx_b, cap, offsets, empty, type, status, data_type, 0, 1, 1, 0);
    o.across = 1;
    o.samples = samples;
    return o;
}

}  // namespace
