// Training samples on the device: the within-scene and across-scene samples of the reference's loader
// (dense_correspondence/dataset/spartan_dataset_masked.py get_within_scene_data :577-839, get_across_scene_data :1056-1141)
// for B image pairs, as the eight pixel lists the loss takes, concatenated in loss order (match | masked | background | blind
// per pair) with device offsets.  Nothing waits for the host; every count stays on the device.
// The kernels and launch helpers up to the writer live in sample_shared.h, which synthetic_kernels.hip includes too:
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
#include "sample_shared.h"

namespace {

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
