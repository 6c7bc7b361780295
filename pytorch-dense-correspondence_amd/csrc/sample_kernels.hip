// Training samples on the device: the within-scene and across-scene samples of the reference's loader
// (dense_correspondence/dataset/spartan_dataset_masked.py get_within_scene_data :577-839, get_across_scene_data :1056-1141)
// for B image pairs, as the eight pixel lists the loss takes, concatenated in loss order (match | masked | background | blind
// per pair) with device offsets.  Nothing waits for the host; every count stays on the device.
//
//   compact_count_kernel / compact_write_kernel   ordered (torch.nonzero order) compaction of up to 6 per-pair "sources" in
//       one launch pair: mask a / mask b as given, the candidate flags, and -- read through the pair's 180-degree rotation
//       record -- mask a minus the matched map (blind set), mask b and 1 - mask b.  Segments of 4096 elements, 16 per
//       work-item; pass 2 sums the preceding segments' counts itself (integer adds, no atomics, no third pass).
//   candidate_kernel    A draws per pair (from mask a's list or uniform), then the reprojection test of project_kernel
//                       (pairgen_project.h, the same arithmetic).
//   match_kernel        the kept candidates in order (or match lists found elsewhere: complete_samples) -> flattened a / b
//                       indices after the pair's rotation, and the matched map of the rotated image a.
//   offsets_kernel      counts -> offsets [4n + 1], empty, type.
//   write_kernel        ONE pass over the whole output capacity: each work-item owns 4 consecutive entries, finds its
//                       (pair, list, entry) by a binary search over the offsets held in LDS, writes idx_a / idx_b int64
//                       (16-byte stores) and -1 past offsets[4n].
//   eval_offsets_kernel / eval_select_kernel   matches only (section 11a, the evaluation): the kept candidates with their
//                       float projections, subsampled like random.sample, in match_list order.
//
// Random numbers: uniform on torch.rand's 24-bit grid from a counter-based hash of (pair seed, site, index), or replayed from
// the caller's streams (include/dcn_hip.h section 9).
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
    const int32_t* params;         // [2n][DCN_AUG_PARAM_WORDS]: a's records, then b's (flips), or null
    int32_t* lists;                // workspace [NSRC][n][ls] compacted element indices (ls = max(hw, attempts))
    int64_t* counts;               // workspace [NSRC][n]
    int32_t* seg;                  // workspace [NSRC][n][segs] per-segment counts
    const uint8_t* flags;          // workspace [n][attempts]
    const uint8_t* matched;        // workspace [n][hw]
    int n, h, w, segs;
    int64_t hw, attempts, ls;
    uint32_t src_mask;             // the sources compacted by this launch pair
};

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
    const uint32_t m = (side_b ? c.mask_b : c.mask_a)[(size_t)p * c.hw + sy * c.w + sx] != 0;
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
        if (threadIdx.x == 0) c.seg[((size_t)s * c.n + p) * c.segs + blockIdx.x] = 0;
        return;
    }
    int32_t cnt = 0;
    for (int k = 0; k < kPer; ++k)
        if (e0 + k < len) cnt += (int32_t)pred(c, s, p, e0 + k);
    cnt = dcn::block_sum<kThreads>(cnt, scratch);
    if (threadIdx.x == 0) c.seg[((size_t)s * c.n + p) * c.segs + blockIdx.x] = cnt;
}

// grid (segs, n * NSRC): this segment's elements to lists[s][p][base + rank], in order; the last segment writes the count.
__global__ void __launch_bounds__(kThreads) compact_write_kernel(Common c) {
    __shared__ int32_t scratch[kWaves];
    __shared__ int32_t wave_tot[kWaves];
    __shared__ int32_t base_s;
    const int s = blockIdx.y / c.n, p = blockIdx.y - s * c.n;
    if (!((c.src_mask >> s) & 1u)) return;
    const int64_t len = src_len(c, s), e0 = (int64_t)blockIdx.x * kSeg + (int64_t)threadIdx.x * kPer;
    const int32_t* seg = c.seg + ((size_t)s * c.n + p) * c.segs;
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
    int32_t* out = c.lists + ((size_t)s * c.n + p) * c.ls;
    for (int k = 0; k < kPer; ++k)
        if ((bits >> k) & 1u) out[pos++] = (int32_t)(e0 + k);
    if (threadIdx.x == 0 && (int64_t)(blockIdx.x + 1) * kSeg >= len) c.counts[(size_t)s * c.n + p] = total;
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

// grid (ceil(attempts / 256), n)
__global__ void __launch_bounds__(kThreads) candidate_kernel(CandArgs a) {
    const int p = blockIdx.y;
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= a.attempts) return;
    int bad = 0;
    int64_t u = -1, v = -1;
    if (a.from_mask) {
        const int64_t cnt = a.count_a[p];
        if (cnt > 0) {
            const int64_t px = pick(a.list_a + (size_t)p * a.ls, cnt, uniform(a.d, p, SITE_CAND, i, bad));
            u = px % a.w;
            v = px / a.w;
        }
    } else {                                                        // pytorch_rand_select_pixel (:29-34): torch.rand(2, A)
        u = (int64_t)floorf(uniform(a.d, p, SITE_CAND, i, bad) * (float)a.w);
        v = (int64_t)floorf(uniform(a.d, p, SITE_CAND, a.attempts + i, bad) * (float)a.h);
    }
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
    const int site = t == 1 ? SITE_MASKED : SITE_BACKGROUND;
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

inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

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

// ---- matches only, for the evaluation (include/dcn_hip.h section 11a): the kept candidates with their FLOAT projections, then
// the subsample random.sample(range(total), min(num_matches, total)) of evaluation.py:919-921.
struct EvalArgs {
    const int32_t* sel;            // [n][ls]-strided lists of SRC_FLAGS: kept candidate indices
    const int64_t* count;          // [n] kept candidates
    const int32_t* pix;
    const float* u2;
    const float* v2;
    const int32_t* order;          // [n][num_matches] replay positions, -1 padded, or null
    const int64_t* seeds;          // [n] (order == null)
    int64_t* ua;                   // [n * rpp]
    int64_t* va;
    float* ub;
    float* vb;
    int64_t* offsets;              // [n + 1]
    int32_t* totals;               // [n]
    int32_t* status;
    int64_t attempts, ls;
    int n, w, num_matches, rpp;    // rpp = min(num_matches, attempts): rows per pair at most
};

// one workgroup: offsets[p + 1] = offsets[p] + min(num_matches, total_p)
__global__ void __launch_bounds__(1024) eval_offsets_kernel(EvalArgs a) {
    __shared__ int32_t k_s[kMaxPairs];
    for (int p = threadIdx.x; p < a.n; p += 1024) {
        const int64_t t = a.count[p];
        a.totals[p] = (int32_t)t;
        k_s[p] = (int32_t)(t < a.num_matches ? t : a.num_matches);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int64_t o = 0;
        a.offsets[0] = 0;
        for (int p = 0; p < a.n; ++p) {
            o += k_s[p];
            a.offsets[p + 1] = o;
        }
    }
}

using dcn::order_key;

// grid (ceil(attempts / 256), n): work-item e of pair p.  Replay: e < k is output row e, survivor order[p][e].  Seeded: e <
// total is survivor e, whose rank among the total hashed keys (ties by index) is its row when below k.  Every work-item with
// e < rpp also owns entry p * rpp + e of the outputs' tail (-1 / 0 from offsets[n] on).
__global__ void __launch_bounds__(kThreads) eval_select_kernel(EvalArgs a) {
    const int p = blockIdx.y;
    const int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    const int64_t total = a.count[p], k = total < a.num_matches ? total : a.num_matches;
    const int64_t base = a.offsets[p], end = a.offsets[a.n];
    if (e < a.rpp) {
        const int64_t g = (int64_t)p * a.rpp + e;
        if (g >= end) {
            a.ua[g] = -1;
            a.va[g] = -1;
            a.ub[g] = 0.f;
            a.vb[g] = 0.f;
        }
    }
    int64_t row = -1, i = 0;
    if (a.order) {
        if (e < k) {
            row = e;
            i = a.order[(size_t)p * a.num_matches + e];
            if (i < 0 || i >= total) {
                atomicOr(a.status, DCN_SAMPLE_BAD_DRAWS);
                i = 0;
            }
        }
    } else if (e < total) {
        const uint64_t s = (uint64_t)a.seeds[p];
        const uint32_t mine = order_key(s, (uint32_t)e);
        int64_t rank = 0;
        for (int64_t j = 0; j < total; ++j) {
            const uint32_t o = order_key(s, (uint32_t)j);
            rank += (o < mine || (o == mine && j < e)) ? 1 : 0;
        }
        if (rank < k) {
            row = rank;
            i = e;
        }
    }
    if (row < 0) return;
    const int64_t c = (int64_t)p * a.attempts + a.sel[(size_t)p * a.ls + i];
    const int64_t px = a.pix[c];
    a.ua[base + row] = px % a.w;
    a.va[base + row] = px / a.w;
    a.ub[base + row] = a.u2[c];
    a.vb[base + row] = a.v2[c];
}

// stages 4 - 6 after the matches (ma / mb / mcount / matched are in the workspace)
inline int finish_within(const Common& c, const OutArgs& o, hipStream_t st) {
    compact(c, (1u << SRC_BLIND) | (1u << SRC_MB) | (o.inv ? (1u << SRC_MBINV) : 0u), st);
    write_out(o, st);
    return dcn::check_launch();
}

}  // namespace

extern "C" size_t dcn_sample_workspace(int n, int h, int w, int64_t attempts, int64_t match_slots) {
    if (n < 1 || h < 1 || w < 1 || attempts < 0 || match_slots < 0) return 0;
    return carve(nullptr, nullptr, n, (int64_t)h * w, attempts, match_slots);
}

extern "C" size_t dcn_eval_matches_workspace(int n, int h, int w, int64_t attempts) {
    if (n < 1 || h < 1 || w < 1 || attempts < 1) return 0;
    return carve(nullptr, nullptr, n, (int64_t)h * w, attempts, 1);
}

extern "C" int dcn_eval_matches(int n, int h, int w, const uint16_t* depth_a, const uint16_t* depth_b, const uint8_t* mask_a,
                                const float* cams, int64_t attempts, const int64_t* seeds, const float* rand,
                                const int64_t* rand_offsets, int num_matches, const int32_t* match_order,
                                const int64_t* order_seeds, int64_t* u_a, int64_t* v_a, float* u_b, float* v_b, int64_t* offsets,
                                int32_t* totals, int32_t* status, void* workspace, void* stream) {
    const int64_t hw = (int64_t)h * w;
    if (!shape_ok(n, h, w) || !depth_a || !depth_b || !mask_a || !cams || attempts < 1 || attempts > 4096 ||
        !random_source_ok(seeds, rand, rand_offsets) || num_matches < 1 || (!match_order && !order_seeds) || !u_a || !v_a ||
        !u_b || !v_b || !offsets || !totals || !status || !workspace)
        return DCN_E_INVALID;
    hipStream_t st = (hipStream_t)stream;
    Workspace ws;
    carve(&ws, (char*)workspace, n, hw, attempts, 1);
    const int rc = begin(status, nullptr, n, hw, st);
    if (rc != DCN_OK) return rc;
    const Common c = common_of(ws, n, h, w, attempts, mask_a, mask_a, nullptr);
    find_candidates(c, cand_of(ws, c, depth_a, depth_b, cams, draws_of(n, seeds, rand, rand_offsets), status, 1), st);
    const int64_t ls = c.ls;
    EvalArgs e;
    e.sel = ws.lists + (size_t)SRC_FLAGS * n * ls;
    e.count = ws.counts + (size_t)SRC_FLAGS * n;
    e.pix = ws.pix;
    e.u2 = ws.u2;
    e.v2 = ws.v2;
    e.order = match_order;
    e.seeds = order_seeds;
    e.ua = u_a;
    e.va = v_a;
    e.ub = u_b;
    e.vb = v_b;
    e.offsets = offsets;
    e.totals = totals;
    e.status = status;
    e.attempts = attempts;
    e.ls = ls;
    e.n = n;
    e.w = w;
    e.num_matches = num_matches;
    e.rpp = (int)(num_matches < attempts ? num_matches : attempts);
    hipLaunchKernelGGL(eval_offsets_kernel, dim3(1), dim3(1024), 0, st, e);
    hipLaunchKernelGGL(eval_select_kernel, dim3((unsigned)dcn::ceil_div64(attempts, kThreads), (unsigned)n), dim3(kThreads), 0, st,
                       e);
    return dcn::check_launch();
}

extern "C" int dcn_within_scene_samples(int n, int h, int w, const uint16_t* depth_a, const uint16_t* depth_b,
                                        const uint8_t* mask_a, const uint8_t* mask_b, const float* cams, int64_t attempts,
                                        int k_masked, int k_background, int flags, const int32_t* aug_params,
                                        const int64_t* seeds, const float* rand, const int64_t* rand_offsets, int data_type,
                                        int64_t* idx_a, int64_t* idx_b, int64_t capacity, int64_t* offsets, uint8_t* empty,
                                        int32_t* type, int32_t* status, void* workspace, void* stream) {
    const int64_t hw = (int64_t)h * w;
    if (!shape_ok(n, h, w) || !depth_a || !depth_b || !mask_a || !mask_b || !cams || attempts < 1 || attempts > (1LL << 30) ||
        k_masked < 1 || k_background < 1 || (flags & ~(DCN_SAMPLE_ONLY_OFF_MASK | DCN_SAMPLE_MASK_INV)) ||
        !random_source_ok(seeds, rand, rand_offsets) || !outputs_ok(idx_a, idx_b, offsets, empty, type, status, workspace) ||
        capacity != (int64_t)n * (attempts * (1 + (int64_t)k_masked + k_background) + hw))
        return DCN_E_INVALID;
    hipStream_t st = (hipStream_t)stream;
    Workspace ws;
    carve(&ws, (char*)workspace, n, hw, attempts, attempts);
    const Draws d = draws_of(n, seeds, rand, rand_offsets);
    const int rc = begin(status, ws.matched, n, hw, st);
    if (rc != DCN_OK) return rc;
    const Common c = common_of(ws, n, h, w, attempts, mask_a, mask_b, aug_params);
    find_candidates(c, cand_of(ws, c, depth_a, depth_b, cams, d, status, (flags & DCN_SAMPLE_ONLY_OFF_MASK) ? 1 : 0), st);
    const int64_t ls = c.ls;
    MatchArgs m = {};
    m.sel = ws.lists + (size_t)SRC_FLAGS * n * ls;
    m.count = ws.counts + (size_t)SRC_FLAGS * n;
    m.pix = ws.pix;
    m.u2 = ws.u2;
    m.v2 = ws.v2;
    m.params = aug_params;
    m.ma = ws.ma;
    m.mb = ws.mb;
    m.mcount = ws.mcount;
    m.matched = ws.matched;
    m.status = status;
    m.attempts = attempts;
    m.hw = hw;
    m.stride = attempts;
    m.ls = ls;
    m.n = n;
    m.h = h;
    m.w = w;
    hipLaunchKernelGGL(match_kernel, dim3((unsigned)dcn::ceil_div64(attempts, kThreads), (unsigned)n), dim3(kThreads), 0, st, m);
    return finish_within(c, out_of(ws, c, d, idx_a, idx_b, capacity, offsets, empty, type, status, data_type, attempts, k_masked,
                                   k_background, (flags & DCN_SAMPLE_MASK_INV) ? 1 : 0), st);
}

extern "C" int dcn_complete_samples(int n, int h, int w, const int64_t* u_a, const int64_t* v_a, const void* u_b,
                                    const void* v_b, int uv_b_dtype, const int64_t* list_offsets, int64_t count,
                                    const uint8_t* mask_a, const uint8_t* mask_b, int k_masked, int k_background, int flags,
                                    const int32_t* aug_params, const int64_t* seeds, const float* rand,
                                    const int64_t* rand_offsets, int data_type, int64_t* idx_a, int64_t* idx_b,
                                    int64_t capacity, int64_t* offsets, uint8_t* empty, int32_t* type, int32_t* status,
                                    void* workspace, void* stream) {
    const int64_t hw = (int64_t)h * w;
    if (!shape_ok(n, h, w) || count < 0 || (count > 0 && (!u_a || !v_a || !u_b || !v_b)) || !list_offsets || !mask_a ||
        !mask_b || k_masked < 1 || k_background < 1 || (flags & ~DCN_SAMPLE_MASK_INV) ||
        (uv_b_dtype != DCN_UV_INT64 && uv_b_dtype != DCN_UV_FLOAT32) || !random_source_ok(seeds, rand, rand_offsets) ||
        !outputs_ok(idx_a, idx_b, offsets, empty, type, status, workspace) ||
        capacity != count * (1 + (int64_t)k_masked + k_background) + (int64_t)n * hw)
        return DCN_E_INVALID;
    hipStream_t st = (hipStream_t)stream;
    const int64_t stride = count > 0 ? count : 1;
    Workspace ws;
    carve(&ws, (char*)workspace, n, hw, 0, stride);
    const int rc = begin(status, ws.matched, n, hw, st);
    if (rc != DCN_OK) return rc;
    MatchArgs m = {};
    m.ua = u_a;
    m.va = v_a;
    m.ub = u_b;
    m.vb = v_b;
    m.ub_float = uv_b_dtype == DCN_UV_FLOAT32;
    m.off = list_offsets;
    m.ext_count = count;
    m.params = aug_params;
    m.ma = ws.ma;
    m.mb = ws.mb;
    m.mcount = ws.mcount;
    m.matched = ws.matched;
    m.status = status;
    m.hw = hw;
    m.stride = stride;
    m.n = n;
    m.h = h;
    m.w = w;
    hipLaunchKernelGGL(match_kernel, dim3((unsigned)dcn::ceil_div64(stride, kThreads), (unsigned)n), dim3(kThreads), 0, st, m);
    const Common c = common_of(ws, n, h, w, 0, mask_a, mask_b, aug_params);
    return finish_within(c, out_of(ws, c, draws_of(n, seeds, rand, rand_offsets), idx_a, idx_b, capacity, offsets, empty, type,
                                   status, data_type, stride, k_masked, k_background, (flags & DCN_SAMPLE_MASK_INV) ? 1 : 0), st);
}

extern "C" int dcn_across_scene_samples(int n, int h, int w, const uint8_t* mask_a, const uint8_t* mask_b, int64_t num_samples,
                                        const int32_t* aug_params, const int64_t* seeds, const float* rand,
                                        const int64_t* rand_offsets, int data_type, int64_t* idx_a, int64_t* idx_b,
                                        int64_t capacity, int64_t* offsets, uint8_t* empty, int32_t* type, int32_t* status,
                                        void* workspace, void* stream) {
    const int64_t hw = (int64_t)h * w;
    if (!shape_ok(n, h, w) || !mask_a || !mask_b || num_samples < 1 || !random_source_ok(seeds, rand, rand_offsets) ||
        !outputs_ok(idx_a, idx_b, offsets, empty, type, status, workspace) || capacity != (int64_t)n * num_samples)
        return DCN_E_INVALID;
    hipStream_t st = (hipStream_t)stream;
    Workspace ws;
    carve(&ws, (char*)workspace, n, hw, 0, 0);
    const int rc = begin(status, nullptr, n, hw, st);
    if (rc != DCN_OK) return rc;
    const Common c = common_of(ws, n, h, w, 0, mask_a, mask_b, aug_params);
    compact(c, (1u << SRC_A0) | (1u << SRC_B0), st);
    write_out(across_of(ws, c, draws_of(n, seeds, rand, rand_offsets), idx_a, idx_b, capacity, offsets, empty, type, status,
                        data_type, num_samples), st);
    return dcn::check_launch();
}

// ------------------------------------------------------------------------------------------------ joining sample batches
// dcn_concat_samples: the outputs of up to kMaxGroups calls above as ONE batch -- pairs in the order given, lists compacted.
//   concat_offsets_kernel   one workgroup: checks every group's offsets (from 0, increasing, within its capacity), shifts them
//                           by the entries of the groups in front, ORs the status words.
//   concat_write_kernel     write_kernel's pass over the output capacity: each work-item owns 4 consecutive entries, finds its
//                           (pair, list, entry) by a binary search over the joined offsets held in LDS, copies the entry from
//                           the pair's group (16-byte stores) and writes -1 past offsets[4n].
namespace {

constexpr int kMaxGroups = DCN_CONCAT_MAX_GROUPS;

struct ConcatArgs {
    const int64_t* src_a[kMaxGroups];
    const int64_t* src_b[kMaxGroups];
    const int64_t* src_off[kMaxGroups];        // [4 * n_g + 1]
    const int32_t* src_status[kMaxGroups];     // [1] or null
    int64_t src_cap[kMaxGroups];
    int base[kMaxGroups + 1];                  // first output pair of group g; base[groups] = n
    int groups, n;
    int64_t* idx_a;                            // [cap]
    int64_t* idx_b;
    int64_t* offsets;                          // [4n + 1]
    int32_t* status;
    int64_t cap;
};

__global__ void __launch_bounds__(1024) concat_offsets_kernel(ConcatArgs a) {
    __shared__ int bad[kMaxGroups];
    __shared__ int64_t shift[kMaxGroups + 1];
    if (threadIdx.x < kMaxGroups) bad[threadIdx.x] = 0;
    __syncthreads();
#pragma unroll
    for (int g = 0; g < kMaxGroups; ++g) {
        if (g >= a.groups) break;
        const int64_t* o = a.src_off[g];
        const int nl = 4 * (a.base[g + 1] - a.base[g]);
        int b = 0;
        for (int i = threadIdx.x; i < nl; i += 1024) b |= o[i + 1] < o[i];
        if (threadIdx.x == 0) b |= o[0] != 0 || o[nl] > a.src_cap[g];
        if (b) bad[g] = 1;                      // (racing writes of the same value)
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int st = 0;
        int64_t pos = 0;
#pragma unroll
        for (int g = 0; g < kMaxGroups; ++g) {
            if (g >= a.groups) break;
            shift[g] = pos;
            if (bad[g]) st |= DCN_SAMPLE_BAD_OFFSETS;          // the group's pairs keep their slots, with empty lists
            else pos += a.src_off[g][4 * (a.base[g + 1] - a.base[g])];
            if (a.src_status[g]) st |= a.src_status[g][0];
        }
        if (pos > a.cap) st |= DCN_SAMPLE_BAD_OFFSETS;
        a.offsets[4 * a.n] = pos;
        a.status[0] = st;
    }
    __syncthreads();
#pragma unroll
    for (int g = 0; g < kMaxGroups; ++g) {
        if (g >= a.groups) break;
        const int64_t* o = a.src_off[g];
        const int nl = 4 * (a.base[g + 1] - a.base[g]);
        int64_t* out = a.offsets + 4 * a.base[g];
        for (int i = threadIdx.x; i < nl; i += 1024) out[i] = shift[g] + (bad[g] ? 0 : o[i]);
    }
}

__global__ void __launch_bounds__(kThreads) concat_write_kernel(ConcatArgs a) {
    __shared__ int64_t off[4 * kMaxPairs + 1];
    __shared__ const int64_t* sa[kMaxGroups];
    __shared__ const int64_t* sb[kMaxGroups];
    __shared__ int base[kMaxGroups + 1];
    const int nl = 4 * a.n;
    for (int i = threadIdx.x; i <= nl; i += kThreads) off[i] = a.offsets[i];
    if (threadIdx.x == 0) {
#pragma unroll
        for (int g = 0; g < kMaxGroups; ++g) {
            sa[g] = a.src_a[g];
            sb[g] = a.src_b[g];
            base[g] = a.base[g];                                // (= n from the last group on)
        }
        base[kMaxGroups] = a.n;
    }
    __syncthreads();
    const int64_t total = off[nl] < a.cap ? off[nl] : a.cap;
    for (int64_t i0 = ((int64_t)blockIdx.x * kThreads + threadIdx.x) * kRun; i0 < a.cap;
         i0 += (int64_t)gridDim.x * kThreads * kRun) {
        int64_t va[kRun], vb[kRun];
        int l = 0, g = 0;
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
                while (off[l + 1] <= i) ++l;                    // entry i - off[l] of list l & 3 of pair l >> 2
                while (base[g + 1] <= (l >> 2)) ++g;            // ... which is entry i - off[4 * base[g]] of its group's lists
                const int64_t e = i - off[4 * base[g]];
                va[r] = sa[g][e];
                vb[r] = sb[g][e];
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
}

}  // namespace

extern "C" int dcn_concat_samples(int groups, const int* n, const int64_t* const* idx_a, const int64_t* const* idx_b,
                                  const int64_t* const* offsets, const int64_t* capacity_in, const int32_t* const* status_in,
                                  int64_t* idx_a_out, int64_t* idx_b_out, int64_t capacity, int64_t* offsets_out,
                                  int32_t* status, void* stream) {
    if (groups < 1 || groups > kMaxGroups || !n || !idx_a || !idx_b || !offsets || !capacity_in || !offsets_out || !status ||
        capacity < 0 || (capacity > 0 && (!idx_a_out || !idx_b_out)) || !aligned16(idx_a_out) || !aligned16(idx_b_out))
        return DCN_E_INVALID;
    ConcatArgs a;
    int total = 0;
    for (int g = 0; g < kMaxGroups; ++g) {
        const bool on = g < groups;
        if (on && (n[g] < 1 || !offsets[g] || capacity_in[g] < 0 || (capacity_in[g] > 0 && (!idx_a[g] || !idx_b[g]))))
            return DCN_E_INVALID;
        a.src_a[g] = on ? idx_a[g] : nullptr;
        a.src_b[g] = on ? idx_b[g] : nullptr;
        a.src_off[g] = on ? offsets[g] : nullptr;
        a.src_status[g] = on && status_in ? status_in[g] : nullptr;
        a.src_cap[g] = on ? capacity_in[g] : 0;
        a.base[g] = total;
        if (on) total += n[g];
        if (total > kMaxPairs) return DCN_E_INVALID;
    }
    a.base[kMaxGroups] = total;
    a.groups = groups;
    a.n = total;
    a.idx_a = idx_a_out;
    a.idx_b = idx_b_out;
    a.offsets = offsets_out;
    a.status = status;
    a.cap = capacity;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(concat_offsets_kernel, dim3(1), dim3(1024), 0, st, a);
    int64_t blocks = dcn::ceil_div64(dcn::ceil_div64(capacity, kRun), kThreads);
    blocks = blocks < 1 ? 1 : (blocks > 2048 ? 2048 : blocks);
    hipLaunchKernelGGL(concat_write_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, st, a);
    return dcn::check_launch();
}
