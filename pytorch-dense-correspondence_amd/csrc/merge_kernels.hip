// Synthetic multi-object samples on the device: the SYNTHETIC_MULTI_OBJECT sample of the reference
// (dense_correspondence/dataset/spartan_dataset_masked.py:890-960), i.e. dense_correspondence/correspondence_tools/
// correspondence_augmentation.py
//   merge_images_with_occlusions (:217-297): the foreground object's image pasted over the background object's,
//       fg*m + bg*(1-m) in uint8 arithmetic (m = the foreground mask), merged mask = clip(mask_a + mask_b, 0, 1) (uint8 sum)
//   prune_matches_if_occluded (:300-335): the background object's match pair loses every entry whose first (u, v) is
//       inside the foreground mask; order is kept
//   merge_matches (:337-345): object a's matches, then object b's
// for B samples of two frames each, one foreground decision per (sample, frame).
//
//   merge_kernel         one pass over B samples x 2 frames: uint8 HWC RGB + uint8 mask of both objects in; float NCHW network
//                        input, float merged mask and uint8 merged RGB out (each optional).  24 bytes per pixel-frame with the
//                        network input and the mask: HBM bound -- the layout of augment_kernel (two groups of 4 pixels per
//                        work-item, all loads issued before the normalization table, 16-byte stores: image_norm.h).
//   prune_count_kernel   pass 1 of the prune + concatenation: (partition, list) workgroups decide every entry (in range, not
//                        occluded in frame 1 or 2) and write a keep byte per entry plus one record per partition (its kept
//                        count and status bits).
//   prune_write_kernel   pass 2: each workgroup loads its first chunk, then sums the 2B x parts records (integer adds:
//                        order-independent), then writes its partition's kept entries in order (64-bit ballots + a
//                        per-chunk LDS table of wave counts), fills the unused tail with -1 and writes offsets / empty / status.
#include "dcn_common.h"
#include "image_norm.h"
#include "merge_rules.h"

namespace {

constexpr int kMergeThreads = 256;
constexpr int kMergePix = 4;      // pixels per group
constexpr int kMergeGroups = 2;   // groups per work-item

struct MergeArgs {
    const unsigned char* rgb[2][2];   // [frame][object a, b]: [n][h][w][3]
    const unsigned char* mask[2][2];  // [frame][object]: [n][h][w]
    const int32_t* fg;                // [n][2]: DCN_MERGE_FG_B when object b is in front in that frame
    float* net[2];                    // [frame]: [n][3][h][w] or null
    float* mask_out[2];               // [frame]: [n][h][w] or null
    unsigned char* rgb_out[2];        // [frame]: [n][h][w][3] or null
    float mean[3], std[3];
    int n, h, w, vec;
};

// One pixel: fg*m + (1-m)*bg per channel and clip(m + mb, 0, 1), in the reference's uint8 arithmetic.
__device__ __forceinline__ void merge_pixel(const uint32_t fg[3], const uint32_t bg[3], uint32_t m, uint32_t mb, uint32_t out[3],
                                            float& mout) {
    const uint32_t mc = (1U - m) & 0xffU;
    for (int c = 0; c < 3; ++c) out[c] = (fg[c] * m + mc * bg[c]) & 0xffU;
    mout = ((m + mb) & 0xffU) ? 1.0f : 0.0f;
}

__device__ __forceinline__ uint32_t byte_of(const uint32_t* words, int b) { return (words[b >> 2] >> (8 * (b & 3))) & 0xffU; }

// Work-item t of workgroup x owns the 4-pixel groups x * kMergeThreads * kMergeGroups + t + j * kMergeThreads, j <
// kMergeGroups, of image blockIdx.y = frame * n + sample.
__global__ void __launch_bounds__(kMergeThreads) merge_kernel(MergeArgs a) {
    __shared__ float lut[3][256];
    const int f = (int)blockIdx.y >= a.n ? 1 : 0, s = (int)blockIdx.y - f * a.n;
    const int front = a.fg[2 * s + f] == DCN_MERGE_FG_B ? 1 : 0;
    const int64_t hw = (int64_t)a.h * a.w;
    const unsigned char* fg_rgb = a.rgb[f][front] + (size_t)s * hw * 3;
    const unsigned char* bg_rgb = a.rgb[f][1 - front] + (size_t)s * hw * 3;
    const unsigned char* fg_msk = a.mask[f][front] + (size_t)s * hw;
    const unsigned char* bg_msk = a.mask[f][1 - front] + (size_t)s * hw;
    float* net = a.net[f] ? a.net[f] + (size_t)s * 3 * hw : nullptr;
    float* mask_out = a.mask_out[f] ? a.mask_out[f] + (size_t)s * hw : nullptr;
    unsigned char* rgb_out = a.rgb_out[f] ? a.rgb_out[f] + (size_t)s * hw * 3 : nullptr;
    const int64_t g0 = (int64_t)blockIdx.x * kMergeThreads * kMergeGroups + threadIdx.x;
    if (!a.vec) {   // any width / alignment: pixel by pixel
        if (net) dcn::build_norm_table<kMergeThreads>(lut, a.mean, a.std);
        for (int g = 0; g < kMergeGroups; ++g) {
            for (int j = 0; j < kMergePix; ++j) {
                const int64_t p = (g0 + (int64_t)g * kMergeThreads) * kMergePix + j;
                if (p >= hw) break;
                const uint32_t fg[3] = {fg_rgb[p * 3], fg_rgb[p * 3 + 1], fg_rgb[p * 3 + 2]};
                const uint32_t bg[3] = {bg_rgb[p * 3], bg_rgb[p * 3 + 1], bg_rgb[p * 3 + 2]};
                uint32_t px[3];
                float m;
                merge_pixel(fg, bg, fg_msk[p], bg_msk[p], px, m);
                dcn::store_pixel(lut, p, hw, px, m, net, rgb_out, mask_out);
            }
        }
        return;
    }
    // w % 4 == 0, aligned pointers: a group's 4 pixels share a row
    uint32_t fw[kMergeGroups][3], bw[kMergeGroups][3], fm[kMergeGroups], bm[kMergeGroups];
#pragma unroll
    for (int g = 0; g < kMergeGroups; ++g) {
        const int64_t p0 = (g0 + (int64_t)g * kMergeThreads) * kMergePix;
        fm[g] = bm[g] = 0u;
        for (int k = 0; k < 3; ++k) fw[g][k] = bw[g][k] = 0u;
        if (p0 < hw) {
            const uint32_t* f32 = reinterpret_cast<const uint32_t*>(fg_rgb + p0 * 3);
            const uint32_t* b32 = reinterpret_cast<const uint32_t*>(bg_rgb + p0 * 3);
            for (int k = 0; k < 3; ++k) {
                fw[g][k] = f32[k];
                bw[g][k] = b32[k];
            }
            fm[g] = *reinterpret_cast<const uint32_t*>(fg_msk + p0);
            bm[g] = *reinterpret_cast<const uint32_t*>(bg_msk + p0);
        }
    }
    if (net) dcn::build_norm_table<kMergeThreads>(lut, a.mean, a.std);
#pragma unroll
    for (int g = 0; g < kMergeGroups; ++g) {
        const int64_t p0 = (g0 + (int64_t)g * kMergeThreads) * kMergePix;
        if (p0 >= hw) continue;
        uint32_t px[kMergePix][3];
        float mv[kMergePix];
#pragma unroll
        for (int j = 0; j < kMergePix; ++j) {
            uint32_t fg[3], bg[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                fg[c] = byte_of(fw[g], 3 * j + c);
                bg[c] = byte_of(bw[g], 3 * j + c);
            }
            merge_pixel(fg, bg, (fm[g] >> (8 * j)) & 0xffU, (bm[g] >> (8 * j)) & 0xffU, px[j], mv[j]);
        }
        dcn::store_pixels4(lut, p0, hw, px, mv, net, rgb_out, mask_out);
    }
}

constexpr int kPruneThreads = 256;
constexpr int kPruneRows = 4;                                 // entries per work-item and chunk
constexpr int kPruneChunk = kPruneThreads * kPruneRows;      // entries per workgroup iteration
constexpr int kPruneWaves = kPruneThreads / dcn::kWave;
constexpr int kPruneMaxParts = 16;
constexpr int kRecordBadShift = 56;                         // partition record: kept count | status bits << 56

struct PruneList {
    const int64_t *u1, *v1, *u2, *v2;   // [count]: the entry's pixel in frame 1 / frame 2
    const int64_t* off;                 // [n + 1] or null (count == 0)
    int64_t count;
};

struct PruneArgs {
    PruneList list[2];                  // object a, object b
    const unsigned char* mask[2][2];    // [frame][object]: [n][h][w] or null (that mask occludes nothing)
    const int32_t* fg;                  // [n][2]
    int64_t *u_1, *v_1, *u_2, *v_2;     // [cap]
    int64_t* offsets;                   // [n + 1]
    unsigned char* empty;               // [n]
    int32_t* status;                    // [1]
    int64_t* part;                      // workspace [2n][parts]: partition records
    unsigned char* keep;                // workspace [cap]: object a's entries, then object b's
    int64_t cap;                        // count_a + count_b
    int n, h, w, parts, drop_empty;
};

// Entries [lo, hi) of list o for sample s; malformed offsets give an empty range and DCN_MERGE_BAD_OFFSETS.
__device__ __forceinline__ int list_range(const PruneArgs& a, int s, int o, int64_t& lo, int64_t& hi) {
    const PruneList& L = a.list[o];
    lo = hi = 0;
    if (!L.off) return 0;
    const int64_t x = L.off[s], y = L.off[s + 1];
    if (x < 0 || y < x || y > L.count) return DCN_MERGE_BAD_OFFSETS;
    lo = x;
    hi = y;
    return 0;
}

// Partition p of `parts` of [lo, hi)
__device__ __forceinline__ void partition(int64_t lo, int64_t hi, int p, int parts, int64_t& b0, int64_t& b1) {
    const int64_t len = dcn::ceil_div64(hi - lo, parts);
    b0 = lo + len * p;
    b1 = b0 + len < hi ? b0 + len : hi;
    if (b0 > hi) b0 = hi;
}

__global__ void __launch_bounds__(kPruneThreads) prune_count_kernel(PruneArgs a) {
    __shared__ int64_t scratch[kPruneWaves];
    __shared__ int bad_s;
    const int p = blockIdx.x, l = blockIdx.y, s = l >> 1, o = l & 1;
    if (threadIdx.x == 0) bad_s = 0;
    int64_t lo, hi, b0, b1;
    int bad = list_range(a, s, o, lo, hi);
    partition(lo, hi, p, a.parts, b0, b1);
    const PruneList L = a.list[o];
    const int64_t hw = (int64_t)a.h * a.w;
    // frame f: (u_f, v_f) is range-checked when the other object's frame-f mask is given, and tested against it when the
    // record puts the other object in front
    bool chk[2];
    const unsigned char* occ[2];
    for (int f = 0; f < 2; ++f) {
        const unsigned char* m = a.mask[f][1 - o];
        const bool other_in_front = dcn::other_in_front(a.fg, s, f, o);
        chk[f] = m != nullptr;
        occ[f] = (m && other_in_front) ? m + (size_t)s * hw : nullptr;
    }
    unsigned char* keep = a.keep + (o ? a.list[0].count : 0);
    __syncthreads();
    int64_t cnt = 0;
    for (int64_t c0 = b0; c0 < b1; c0 += kPruneChunk) {
        int64_t u[kPruneRows][2], v[kPruneRows][2];
#pragma unroll
        for (int j = 0; j < kPruneRows; ++j) {
            const int64_t e = c0 + j * kPruneThreads + threadIdx.x;
            u[j][0] = v[j][0] = u[j][1] = v[j][1] = 0;
            if (e < b1) {
                if (chk[0]) {
                    u[j][0] = L.u1[e];
                    v[j][0] = L.v1[e];
                }
                if (chk[1]) {
                    u[j][1] = L.u2[e];
                    v[j][1] = L.v2[e];
                }
            }
        }
        uint32_t k[kPruneRows], hit[kPruneRows][2];
#pragma unroll
        for (int j = 0; j < kPruneRows; ++j) {
            const int64_t e = c0 + j * kPruneThreads + threadIdx.x;
            k[j] = e < b1 ? 1u : 0u;
#pragma unroll
            for (int f = 0; f < 2; ++f) {
                hit[j][f] = 0u;
                if (!k[j] || !chk[f]) continue;
                if (u[j][f] < 0 || u[j][f] >= a.w || v[j][f] < 0 || v[j][f] >= a.h) {
                    bad |= DCN_MERGE_BAD_INDEX;
                    k[j] = 0u;
                } else if (occ[f]) {
                    hit[j][f] = occ[f][v[j][f] * a.w + u[j][f]];
                }
            }
        }
#pragma unroll
        for (int j = 0; j < kPruneRows; ++j) {
            const int64_t e = c0 + j * kPruneThreads + threadIdx.x;
            if (e >= b1) continue;
            const uint32_t kj = (k[j] && !hit[j][0] && !hit[j][1]) ? 1u : 0u;
            keep[e] = (unsigned char)kj;
            cnt += kj;
        }
    }
    if (bad) atomicOr(&bad_s, bad);
    cnt = dcn::block_sum<kPruneThreads>(cnt, scratch);
    if (threadIdx.x == 0) a.part[(size_t)l * a.parts + p] = cnt | ((int64_t)bad_s << kRecordBadShift);
}

struct PruneChunk {
    uint32_t k[kPruneRows];
    int64_t x[kPruneRows][4];
};

__device__ __forceinline__ void load_chunk(const PruneList& L, const unsigned char* keep, int64_t c0, int64_t b1, PruneChunk& d) {
#pragma unroll
    for (int j = 0; j < kPruneRows; ++j) {
        const int64_t e = c0 + j * kPruneThreads + threadIdx.x;
        d.k[j] = 0u;
        d.x[j][0] = d.x[j][1] = d.x[j][2] = d.x[j][3] = 0;
        if (e < b1) {
            d.k[j] = keep[e];
            d.x[j][0] = L.u1[e];
            d.x[j][1] = L.v1[e];
            d.x[j][2] = L.u2[e];
            d.x[j][3] = L.v2[e];
        }
    }
}

__global__ void __launch_bounds__(kPruneThreads) prune_write_kernel(PruneArgs a) {
    __shared__ int64_t scratch[kPruneWaves];
    __shared__ int64_t sh[3];                        // kept entries in all samples, first output index of this partition
    __shared__ int64_t own[2];                       // sample s: kept entries of a, of b
    __shared__ int bad_s, ok_s;
    __shared__ int wave_cnt[2][kPruneRows][kPruneWaves];
    const int p = blockIdx.x, l = blockIdx.y, s = l >> 1, o = l & 1;
    const int P = a.parts;
    // this partition's first chunk is loaded before the counts are summed (it does not depend on them)
    int64_t lo, hi, b0, b1;
    list_range(a, s, o, lo, hi);
    partition(lo, hi, p, P, b0, b1);
    const PruneList L = a.list[o];
    const unsigned char* keep = a.keep + (o ? a.list[0].count : 0);
    PruneChunk d;
    load_chunk(L, keep, b0, b1, d);
    if (threadIdx.x == 0) bad_s = 0;
    __syncthreads();
    // 1. the counts this workgroup needs, summed by every workgroup itself (integer adds: no third pass, no atomics on them).
    //    Work-item t takes samples t, t + 256, ...; all records of a sample are loaded at once.
    int64_t before = 0, total = 0, mine = 0;
    int bad = 0;
    for (int s2 = threadIdx.x; s2 < a.n; s2 += kPruneThreads) {
        int64_t r[2][kPruneMaxParts];
#pragma unroll
        for (int o2 = 0; o2 < 2; ++o2)
#pragma unroll
            for (int q = 0; q < kPruneMaxParts; ++q) r[o2][q] = q < P ? a.part[(size_t)(2 * s2 + o2) * P + q] : 0;
        int64_t c[2] = {0, 0};
#pragma unroll
        for (int o2 = 0; o2 < 2; ++o2)
#pragma unroll
            for (int q = 0; q < kPruneMaxParts; ++q) {
                const int64_t cq = r[o2][q] & ((1LL << kRecordBadShift) - 1);
                c[o2] += cq;
                bad |= (int)(r[o2][q] >> kRecordBadShift);
                if (s2 == s && o2 == o && q < p) mine += cq;
            }
        const int64_t v = (!a.drop_empty || (c[0] && c[1])) ? c[0] + c[1] : 0;
        total += v;
        if (s2 < s) before += v;
        if (s2 == s) {
            own[0] = c[0];
            own[1] = c[1];
        }
    }
    if (bad) atomicOr(&bad_s, bad);
    total = dcn::block_sum<kPruneThreads>(total, scratch);
    if (threadIdx.x == 0) sh[0] = total;
    before = dcn::block_sum<kPruneThreads>(before, scratch);
    if (threadIdx.x == 0) sh[1] = before;
    mine = dcn::block_sum<kPruneThreads>(mine, scratch);
    if (threadIdx.x == 0) {
        const bool malformed = (bad_s & DCN_MERGE_BAD_OFFSETS) != 0;
        const int64_t ca = own[0], cb = own[1];
        const bool ok = !malformed && (!a.drop_empty || (ca && cb));
        if (malformed) before = sh[0] = 0;
        sh[1] = before + (o ? ca : 0) + mine;
        ok_s = ok ? 1 : 0;
        if (p == 0 && o == 0) {
            a.offsets[s + 1] = before + (ok ? ca + cb : 0);
            a.empty[s] = (malformed || !ca || !cb) ? 1 : 0;
            if (s == 0) {
                a.offsets[0] = 0;
                *a.status = bad_s;
            }
        }
    }
    __syncthreads();
    // 2. the unused tail [total, cap) of the outputs, spread over all workgroups
    const int64_t nwg = (int64_t)gridDim.x * gridDim.y;
    for (int64_t i = sh[0] + ((int64_t)blockIdx.y * gridDim.x + p) * kPruneThreads + threadIdx.x; i < a.cap;
         i += nwg * kPruneThreads)
        a.u_1[i] = a.v_1[i] = a.u_2[i] = a.v_2[i] = -1;
    if (!ok_s) return;
    // 3. this partition's kept entries, in order, from output index sh[1] on
    const int lane = threadIdx.x & (dcn::kWave - 1), wv = threadIdx.x / dcn::kWave;
    const uint64_t below = (1ull << lane) - 1ull;
    int64_t run = sh[1];
    int buf = 0;
    for (int64_t c0 = b0; c0 < b1; buf ^= 1) {
        uint64_t bal[kPruneRows];
#pragma unroll
        for (int j = 0; j < kPruneRows; ++j) {
            bal[j] = __ballot(d.k[j] != 0u);
            if (lane == 0) wave_cnt[buf][j][wv] = __builtin_popcountll(bal[j]);
        }
        __syncthreads();
        int64_t pos = run;
        int chunk_total = 0;
#pragma unroll
        for (int j = 0; j < kPruneRows; ++j) {
#pragma unroll
            for (int q = 0; q < kPruneWaves; ++q) {
                const int c = wave_cnt[buf][j][q];
                chunk_total += c;
                if (q < wv) pos += c;
            }
            if (d.k[j]) {
                const int64_t dst = pos + __builtin_popcountll(bal[j] & below);
                if (dst < a.cap) {
                    a.u_1[dst] = d.x[j][0];
                    a.v_1[dst] = d.x[j][1];
                    a.u_2[dst] = d.x[j][2];
                    a.v_2[dst] = d.x[j][3];
                }
            }
            // entries of the following rows come after every entry of this row
            for (int q = wv; q < kPruneWaves; ++q) pos += wave_cnt[buf][j][q];
        }
        run += chunk_total;
        c0 += kPruneChunk;
        if (c0 < b1) load_chunk(L, keep, c0, b1, d);
    }
}

inline bool aligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

inline int prune_parts(int n, int64_t count_a, int64_t count_b) {
    const int64_t per_list = dcn::ceil_div64(count_a + count_b, 2 * (int64_t)n);
    const int64_t parts = dcn::ceil_div64(per_list, kPruneChunk);
    return (int)(parts < 1 ? 1 : (parts > kPruneMaxParts ? kPruneMaxParts : parts));
}

using dcn::align256;

}  // namespace

extern "C" int dcn_merge_images(int n, int frames, int h, int w, const int32_t* foreground, const uint8_t* rgb_a1,
                                const uint8_t* rgb_b1, const uint8_t* rgb_a2, const uint8_t* rgb_b2, const uint8_t* mask_a1,
                                const uint8_t* mask_b1, const uint8_t* mask_a2, const uint8_t* mask_b2, const float* mean,
                                const float* std, float* net_1, float* net_2, float* mask_1, float* mask_2, uint8_t* rgb_1,
                                uint8_t* rgb_2, void* stream) {
    if (n < 1 || (frames != 1 && frames != 2) || h < 1 || w < 1 || (int64_t)h * w > (1LL << 30) ||
        (int64_t)frames * n > 65535 || !foreground || !rgb_a1 || !rgb_b1 || !mask_a1 || !mask_b1 || !mean || !std ||
        (frames == 2 && (!rgb_a2 || !rgb_b2 || !mask_a2 || !mask_b2)) || (frames == 1 && (net_2 || mask_2 || rgb_2)))
        return DCN_E_INVALID;
    MergeArgs a;
    a.rgb[0][0] = rgb_a1;
    a.rgb[0][1] = rgb_b1;
    a.rgb[1][0] = rgb_a2;
    a.rgb[1][1] = rgb_b2;
    a.mask[0][0] = mask_a1;
    a.mask[0][1] = mask_b1;
    a.mask[1][0] = mask_a2;
    a.mask[1][1] = mask_b2;
    a.fg = foreground;
    a.net[0] = net_1;
    a.net[1] = net_2;
    a.mask_out[0] = mask_1;
    a.mask_out[1] = mask_2;
    a.rgb_out[0] = rgb_1;
    a.rgb_out[1] = rgb_2;
    for (int c = 0; c < 3; ++c) {
        a.mean[c] = mean[c];
        a.std[c] = std[c];
    }
    a.n = n;
    a.h = h;
    a.w = w;
    bool vec = (w % kMergePix) == 0;
    const void* p16[] = {net_1, net_2, mask_1, mask_2};
    const void* p4[] = {rgb_a1, rgb_b1, rgb_a2, rgb_b2, mask_a1, mask_b1, mask_a2, mask_b2, rgb_1, rgb_2};
    for (const void* p : p16) vec = vec && aligned(p, 16);
    for (const void* p : p4) vec = vec && aligned(p, 4);
    a.vec = vec ? 1 : 0;
    const int64_t groups = dcn::ceil_div64((int64_t)h * w, kMergePix);
    const dim3 grid((unsigned)dcn::ceil_div64(groups, kMergeThreads * kMergeGroups), (unsigned)(frames * n));
    hipLaunchKernelGGL(merge_kernel, grid, dim3(kMergeThreads), 0, (hipStream_t)stream, a);
    return dcn::check_launch();
}

extern "C" size_t dcn_merge_prune_workspace(int n, int64_t count_a, int64_t count_b) {
    if (n < 1 || count_a < 0 || count_b < 0) return 0;
    const size_t parts = (size_t)prune_parts(n, count_a, count_b) * 2 * (size_t)n;
    return align256(parts * sizeof(int64_t)) + align256((size_t)(count_a + count_b));
}

extern "C" int dcn_merge_prune(int n, int h, int w, const int32_t* foreground, const uint8_t* mask_a1, const uint8_t* mask_b1,
                               const uint8_t* mask_a2, const uint8_t* mask_b2, const int64_t* u_a1, const int64_t* v_a1,
                               const int64_t* u_a2, const int64_t* v_a2, const int64_t* offsets_a, int64_t count_a,
                               const int64_t* u_b1, const int64_t* v_b1, const int64_t* u_b2, const int64_t* v_b2,
                               const int64_t* offsets_b, int64_t count_b, int flags, int64_t* u_1, int64_t* v_1, int64_t* u_2,
                               int64_t* v_2, int64_t* offsets, uint8_t* empty, int32_t* status, void* workspace,
                               void* stream) {
    const int64_t cap = count_a + count_b;
    if (n < 1 || h < 1 || w < 1 || 2LL * n > 65535 || count_a < 0 || count_b < 0 || !foreground || !offsets || !empty ||
        !status || !workspace || (cap > 0 && (!u_1 || !v_1 || !u_2 || !v_2)) ||
        (count_a > 0 && (!u_a1 || !v_a1 || !u_a2 || !v_a2 || !offsets_a)) ||
        (count_b > 0 && (!u_b1 || !v_b1 || !u_b2 || !v_b2 || !offsets_b)) || (flags & ~DCN_MERGE_DROP_EMPTY))
        return DCN_E_INVALID;
    PruneArgs a;
    a.list[0] = PruneList{u_a1, v_a1, u_a2, v_a2, count_a > 0 ? offsets_a : nullptr, count_a};
    a.list[1] = PruneList{u_b1, v_b1, u_b2, v_b2, count_b > 0 ? offsets_b : nullptr, count_b};
    a.mask[0][0] = mask_a1;
    a.mask[0][1] = mask_b1;
    a.mask[1][0] = mask_a2;
    a.mask[1][1] = mask_b2;
    a.fg = foreground;
    a.u_1 = u_1;
    a.v_1 = v_1;
    a.u_2 = u_2;
    a.v_2 = v_2;
    a.offsets = offsets;
    a.empty = empty;
    a.status = status;
    a.parts = prune_parts(n, count_a, count_b);
    const size_t np = (size_t)a.parts * 2 * (size_t)n;
    char* ws = (char*)workspace;
    a.part = (int64_t*)ws;
    a.keep = (unsigned char*)(ws + align256(np * sizeof(int64_t)));
    a.cap = cap;
    a.n = n;
    a.h = h;
    a.w = w;
    a.drop_empty = (flags & DCN_MERGE_DROP_EMPTY) ? 1 : 0;
    const dim3 grid((unsigned)a.parts, (unsigned)(2 * n));
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(prune_count_kernel, grid, dim3(kPruneThreads), 0, st, a);
    hipLaunchKernelGGL(prune_write_kernel, grid, dim3(kPruneThreads), 0, st, a);
    return dcn::check_launch();
}
