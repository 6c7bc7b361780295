// SYNTHETIC_MULTI_OBJECT training samples on the device: the reference's get_synthetic_multi_object_within_scene_data
// (dense_correspondence/dataset/spartan_dataset_masked.py:890-1053) for B samples of four frames each (object a's frames a1,
// a2 and object b's b1, b2), as the loss's concatenated pair lists (include/dcn_hip.h section 9a).  One chain on the caller's
// stream, nothing waits for the host:
//
//   compact (sample_shared.h)   mask a1's and mask b1's pixel lists, 2B rows in one launch pair (candidates off the mask)
//   syn_candidate_kernel        2B rows (object a's B searches, then object b's) x A candidates: the draw and the reprojection
//                               test of the within-scene search (draw_candidate, project_candidate), then the occlusion prune
//                               of merge_rules.h on the survivor's frame-1 pixel and truncated frame-2 pixel.  A keep byte per
//                               candidate; per workgroup one word: did a candidate survive the SEARCH, was a stream too short.
//   compact                     the kept candidates of the 2B rows, in candidate order
//   syn_match_kernel            sample s: object a's kept entries, then object b's (merge_matches) -> the match slots the writer
//                               reads; a sample with an empty a or b list (or marked empty by the caller) has none.  Object
//                               b's short-stream bit counts only when object a's search found something (the reference never
//                               searches b's scene otherwise).
//   compact                     the merged frame-2 mask (mask a2 | mask b2) and its inverse
//   offsets_kernel / write_kernel (sample_shared.h)   the four lists per sample; the blind list stays empty (:1053)
//   dcn_merge_images            the merged network inputs and masks (merge_kernels.hip: one text for that arithmetic)
//
// The per-object non-matches and blind sets that a composition of dcn_within_scene_samples would build and drop never exist.
#include "merge_rules.h"
#include "sample_shared.h"

namespace {

enum SynSite { SYN_CAND_A = DCN_SYNTHETIC_SITE_CAND_A, SYN_CAND_B = DCN_SYNTHETIC_SITE_CAND_B,
               SYN_MASKED = DCN_SYNTHETIC_SITE_MASKED, SYN_BACKGROUND = DCN_SYNTHETIC_SITE_BACKGROUND };

constexpr int kSurvived = 0x100;                // row word: a candidate passed the reprojection test

struct SynArgs {
    const uint16_t* depth;         // [4][n][hw]: a1, a2, b1, b2
    const uint8_t* mask;           // [4][n][hw]
    const float* cams;             // [2][n][DCN_SAMPLE_CAM_FLOATS]: a1 -> a2, b1 -> b2
    const int32_t* fg;             // [n][2] foreground records
    const uint8_t* empty_in;       // [n] or null
    Draws d;
    const int32_t* list1;          // [2n][ls] pixels of mask a1 / b1
    const int64_t* count1;         // [2n]
    uint8_t* keep;                 // [2n][attempts]
    float* u2;                     // [2n][attempts]
    float* v2;
    int32_t* pix;                  // [2n][attempts] flat frame-1 pixel
    int32_t* words;                // [2n][blocks] per-workgroup words (kSurvived | DCN_SAMPLE_BAD_DRAWS)
    const int32_t* sel;            // [2n][attempts] kept candidate indices
    const int64_t* kept;           // [2n]
    int64_t* ma;                   // [n][2 * attempts]
    int64_t* mb;
    int64_t* mcount;               // [n]
    int64_t* blind_count;          // [n]: the writer's blind-set sizes, zeroed here
    int32_t* status;
    int64_t attempts, hw, ls;
    int n, h, w, from_mask, blocks;
};

// Frame f (0 / 1) of object o (0 = a, 1 = b), sample s, in the [4][n] slot order a1, a2, b1, b2
__device__ __forceinline__ size_t slot(const SynArgs& a, int o, int f, int s) { return ((size_t)(2 * o + f) * a.n + s) * a.hw; }

// grid (blocks = ceil(attempts / 256), 2n): row r = o * n + s
__global__ void __launch_bounds__(kThreads) syn_candidate_kernel(SynArgs a) {
    __shared__ int32_t scratch[kWaves];
    const int r = blockIdx.y, o = r >= a.n ? 1 : 0, s = r - o * a.n;
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    int bad = 0;
    unsigned char ok = 0, keep = 0;
    float u2 = 0.f, v2 = 0.f;
    int64_t u = -1, v = -1;
    const bool live = i < a.attempts && !(a.empty_in && a.empty_in[s]);
    if (live) {
        draw_candidate(a.d, s, o ? SYN_CAND_B : SYN_CAND_A, i, a.attempts, a.from_mask, a.list1 + (size_t)r * a.ls,
                       a.from_mask ? a.count1[r] : 0, a.h, a.w, u, v, bad);
        const float* cam = a.cams + (size_t)r * DCN_SAMPLE_CAM_FLOATS;
        if (u >= 0)
            ok = dcn::project_candidate(a.depth + slot(a, o, 0, s), a.depth + slot(a, o, 1, s), a.h, a.w, cam, cam + 9, cam + 18,
                                        cam + 34, u, v, u2, v2);
        if (ok) {   // a survivor's projection lies inside the image (project_candidate): truncation as `.long()`
            const int64_t p1 = v * a.w + u, p2 = (int64_t)v2 * a.w + (int64_t)u2;
            keep = !dcn::occluded(a.fg, s, 0, o, a.mask + slot(a, 1 - o, 0, s), p1) &&
                   !dcn::occluded(a.fg, s, 1, o, a.mask + slot(a, 1 - o, 1, s), p2);
        }
    }
    if (i < a.attempts) {
        const size_t k = (size_t)r * a.attempts + i;
        a.keep[k] = keep;
        a.u2[k] = u2;
        a.v2[k] = v2;
        a.pix[k] = (int32_t)(u >= 0 ? v * a.w + u : 0);
    }
    const int32_t nok = dcn::block_sum<kThreads>((int32_t)ok, scratch);
    const int32_t nbad = dcn::block_sum<kThreads>((int32_t)(bad != 0), scratch);
    if (threadIdx.x == 0) a.words[(size_t)r * a.blocks + blockIdx.x] = (nok ? kSurvived : 0) | (nbad ? DCN_SAMPLE_BAD_DRAWS : 0);
}

// grid (ceil(2 * attempts / 256), n): match slot e of sample s
__global__ void __launch_bounds__(kThreads) syn_match_kernel(SynArgs a) {
    __shared__ int32_t scratch[kWaves];
    const int s = blockIdx.y;
    if (blockIdx.x == 0) {   // (uniform per workgroup) the status bits of the two searches
        int32_t wa = 0, wb = 0;
        for (int q = threadIdx.x; q < a.blocks; q += kThreads) {
            wa |= a.words[(size_t)s * a.blocks + q];
            wb |= a.words[(size_t)(a.n + s) * a.blocks + q];
        }
        const int32_t a_found = dcn::block_sum<kThreads>((int32_t)((wa & kSurvived) != 0), scratch);
        const int32_t a_bad = dcn::block_sum<kThreads>((int32_t)((wa & DCN_SAMPLE_BAD_DRAWS) != 0), scratch);
        const int32_t b_bad = dcn::block_sum<kThreads>((int32_t)((wb & DCN_SAMPLE_BAD_DRAWS) != 0), scratch);
        if (threadIdx.x == 0 && (a_bad || (a_found && b_bad))) atomicOr(a.status, DCN_SAMPLE_BAD_DRAWS);
    }
    const int64_t ka = a.kept[s], kb = a.kept[a.n + s];
    const int64_t m = (ka > 0 && kb > 0 && !(a.empty_in && a.empty_in[s])) ? ka + kb : 0;
    const int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (e == 0) {
        a.mcount[s] = m;
        a.blind_count[s] = 0;
    }
    if (e >= m) return;
    const int r = e < ka ? s : a.n + s;
    const int64_t k = (int64_t)r * a.attempts + a.sel[(size_t)r * a.attempts + (e < ka ? e : e - ka)];
    const size_t out = (size_t)s * 2 * a.attempts + e;
    a.ma[out] = a.pix[k];
    a.mb[out] = (int64_t)a.v2[k] * a.w + (int64_t)a.u2[k];          // flatten_uv_tensor: v.long() * W + u.long()
}

struct SynWorkspace {
    Workspace ws;                  // n rows: the mask lists, the match slots (2 * attempts per sample)
    int32_t *sel, *seg, *pix, *words;
    int64_t* kept;
    float *u2, *v2;
    uint8_t* keep;
};

inline int cand_blocks(int64_t attempts) { return (int)dcn::ceil_div64(attempts, kThreads); }

inline size_t carve_synthetic(SynWorkspace* w, char* base, int n, int64_t hw, int64_t attempts) {
    size_t o = carve(w ? &w->ws : nullptr, base, n, hw, 0, 2 * attempts);
    const size_t rows = 2 * (size_t)n;
    auto take = [&](size_t bytes) { const size_t at = o; o += align256(bytes); return base ? base + at : nullptr; };
    char* p;
    p = take(rows * attempts * 4);                                    if (w) w->sel = (int32_t*)p;
    p = take(rows * dcn::ceil_div64(attempts, kSeg) * 4);             if (w) w->seg = (int32_t*)p;
    p = take(rows * 8);                                               if (w) w->kept = (int64_t*)p;
    p = take(rows * attempts * 4);                                    if (w) w->pix = (int32_t*)p;
    p = take(rows * attempts * 4);                                    if (w) w->u2 = (float*)p;
    p = take(rows * attempts * 4);                                    if (w) w->v2 = (float*)p;
    p = take(rows * attempts);                                        if (w) w->keep = (uint8_t*)p;
    p = take(rows * cand_blocks(attempts) * 4);                       if (w) w->words = (int32_t*)p;
    return o;
}

inline bool synthetic_sizes_ok(int n, int h, int w, int64_t attempts) {
    return shape_ok(n, h, w) && attempts >= 1 && attempts <= (1LL << 30) && (int64_t)NSRC * 2 * n <= 65535;
}

}  // namespace

extern "C" size_t dcn_synthetic_workspace(int n, int h, int w, int64_t attempts) {
    if (!synthetic_sizes_ok(n, h, w, attempts)) return 0;
    return carve_synthetic(nullptr, nullptr, n, (int64_t)h * w, attempts);
}

extern "C" int dcn_synthetic_samples(int n, int h, int w, const uint16_t* depth, const uint8_t* mask, const uint8_t* rgb,
                                     const float* cams, int64_t attempts, int k_masked, int k_background, int flags,
                                     const int32_t* foreground, const uint8_t* empty_in, const int64_t* seeds,
                                     const float* rand, const int64_t* rand_offsets, const float* mean, const float* std,
                                     float* net_1, float* net_2, float* mask_1, float* mask_2, int64_t* idx_a, int64_t* idx_b,
                                     int64_t capacity, int64_t* offsets, uint8_t* empty, int32_t* type, int32_t* status,
                                     void* workspace, void* stream) {
    if (!synthetic_sizes_ok(n, h, w, attempts) || !depth || !mask || !cams || k_masked < 1 || k_background < 1 ||
        (flags & ~(DCN_SAMPLE_ONLY_OFF_MASK | DCN_SAMPLE_MASK_INV)) || !foreground ||
        !random_source_ok(seeds, rand, rand_offsets) || !outputs_ok(idx_a, idx_b, offsets, empty, type, status, workspace) ||
        (rgb && (!mean || !std)) || (!rgb && (net_1 || net_2 || mask_1 || mask_2)) ||
        capacity != (int64_t)n * 2 * attempts * (1 + (int64_t)k_masked + k_background))
        return DCN_E_INVALID;
    hipStream_t st = (hipStream_t)stream;
    const int64_t hw = (int64_t)h * w;
    const size_t plane = (size_t)n * hw;                  // one slot of the [4][n] inputs: a1, a2, b1, b2
    SynWorkspace sw;
    carve_synthetic(&sw, (char*)workspace, n, hw, attempts);
    const Draws d = draws_of(n, seeds, rand, rand_offsets);
    const int rc = begin(status, nullptr, n, hw, st);
    if (rc != DCN_OK) return rc;
    const int from_mask = (flags & DCN_SAMPLE_ONLY_OFF_MASK) ? 1 : 0, inv = (flags & DCN_SAMPLE_MASK_INV) ? 1 : 0;
    // 1. candidates of both objects: mask a1's / b1's lists land in rows SRC_A0 * n + s / SRC_B0 * n + s = o * n + s
    const Common c1 = common_of(sw.ws, n, h, w, 0, mask, mask + 2 * plane, nullptr);
    if (from_mask) compact(c1, (1u << SRC_A0) | (1u << SRC_B0), st);
    SynArgs a;
    a.depth = depth;
    a.mask = mask;
    a.cams = cams;
    a.fg = foreground;
    a.empty_in = empty_in;
    a.d = d;
    a.list1 = sw.ws.lists;
    a.count1 = sw.ws.counts;
    a.keep = sw.keep;
    a.u2 = sw.u2;
    a.v2 = sw.v2;
    a.pix = sw.pix;
    a.words = sw.words;
    a.sel = sw.sel;
    a.kept = sw.kept;
    a.ma = sw.ws.ma;
    a.mb = sw.ws.mb;
    a.mcount = sw.ws.mcount;
    a.blind_count = sw.ws.counts + (size_t)SRC_BLIND * n;
    a.status = status;
    a.attempts = attempts;
    a.hw = hw;
    a.ls = c1.ls;
    a.n = n;
    a.h = h;
    a.w = w;
    a.from_mask = from_mask;
    a.blocks = cand_blocks(attempts);
    hipLaunchKernelGGL(syn_candidate_kernel, dim3((unsigned)a.blocks, (unsigned)(2 * n)), dim3(kThreads), 0, st, a);
    // 2. the kept candidates of the 2n rows, in order
    Common c2 = c1;
    c2.mask_a = c2.mask_b = nullptr;
    c2.lists = sw.sel;
    c2.counts = sw.kept;
    c2.seg = sw.seg;
    c2.flags = sw.keep;
    c2.n = 2 * n;
    c2.attempts = attempts;
    c2.ls = attempts;
    c2.segs = (int)dcn::ceil_div64(attempts, kSeg);
    c2.src0 = SRC_FLAGS;
    compact(c2, 1u << SRC_FLAGS, st);
    // 3. a's kept matches then b's, per sample
    hipLaunchKernelGGL(syn_match_kernel, dim3((unsigned)dcn::ceil_div64(2 * attempts, kThreads), (unsigned)n), dim3(kThreads), 0,
                       st, a);
    // 4. non-matches on the merged frame-2 mask; no blind list
    Common c3 = common_of(sw.ws, n, h, w, 0, mask, mask + plane, nullptr);
    c3.mask_b_or = mask + 3 * plane;
    compact(c3, (1u << SRC_MB) | (inv ? (1u << SRC_MBINV) : 0u), st);
    OutArgs o = out_of(sw.ws, c3, d, idx_a, idx_b, capacity, offsets, empty, type, status, DCN_SYNTHETIC_DATA_TYPE, 2 * attempts,
                       k_masked, k_background, inv);
    o.site_masked = SYN_MASKED;
    o.site_background = SYN_BACKGROUND;
    write_out(o, st);
    const int rc2 = dcn::check_launch();
    if (rc2 != DCN_OK || !rgb) return rc2;
    // 5. the merged images and masks
    const size_t img = plane * 3;
    return dcn_merge_images(n, 2, h, w, foreground, rgb, rgb + 2 * img, rgb + img, rgb + 3 * img, mask, mask + 2 * plane,
                            mask + plane, mask + 3 * plane, mean, std, net_1, net_2, mask_1, mask_2, nullptr, nullptr, stream);
}
