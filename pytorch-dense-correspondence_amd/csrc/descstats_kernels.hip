// Descriptor statistics of a batch of descriptor images (include/dcn_hip.h section 12): what
// compute_descriptor_statistics_on_dataset (evaluation.py:2177-2292) computes per image with eight torch operations and a
// torch.nonzero -- per-channel min, max and mean over the whole image and over the object mask -- for n images in one pass,
// and its update_stats loop over the images as one small launch.
//
//   stats_partial_kernel   grid (blocks per image, images).  A workgroup owns a run of pixels of one image and walks its
//                          [pixels][d] floats as a flat array with a stride of S = (256 / d) * d elements, so a work-item
//                          keeps ONE channel (its index modulo d) and six accumulators -- min, max, float64 sum, for the image
//                          and for the mask -- plus the NaN flags, and a wavefront's loads are consecutive dwords.  A work-item
//                          takes its elements in batches of 8: the 8 floats and the 8 mask bytes are loaded into registers
//                          (clamped addresses past the end of the run), then accumulated with selects, no branch on the mask.
//                          The mask byte of a pixel is read by the d work-items of that pixel (one cache line, one HBM read).
//                          The accumulators of the S / d work-items of a channel are folded through LDS as a binary tree over
//                          the pixel slot (a fixed order), and the workgroup writes one partial per channel.
//                          HBM traffic: n * hw * (4 d + 1) bytes read once; the partials are 36 d + 4 bytes per workgroup.
//   stats_finish_kernel    grid (images, groups of 8 channels).  Folds an image's partials of its channels in a fixed order
//                          (1024 / channels interleaved runs of workgroups, then the same tree over the runs), divides the
//                          float64 sums by the float64 counts and rounds to fp32 once.
//   stats_combine_kernel   one workgroup of 64: work-item c replays update_stats (:2237-2263) for channel c over the images
//                          in order, then the scaling of :2289-2290.
// No floating-point atomics anywhere: the result is the same bit for bit from run to run.
#include "dcn_common.h"

namespace {

constexpr int kST = 256;        // work-items per workgroup of the partial kernel
constexpr int kSteps = 16;      // steps of S elements a workgroup takes at least (unless capped by kMaxBlocks)
constexpr int kBatch = 8;       // elements a work-item loads before it accumulates them
constexpr int kMaxBlocks = 1024;
constexpr int kMaxD = 64;
constexpr int kFT = 1024;       // work-items of the finish kernel: kFT / channels interleaved runs of workgroups x channels
constexpr int kFC = 8;          // channels a workgroup of the finish kernel folds
constexpr int kNanImage = 1, kNanMask = 2;

// pixels a workgroup owns / workgroups per image: the same on the host (workspace size, grid) and in the kernels
struct Split {
    int64_t pixels_per_block;
    int blocks;
};
__host__ __device__ inline Split split_image(int64_t hw, int d) {
    const int64_t per_step = kST / d;                       // pixels per step of S = per_step * d elements
    int64_t ppb = per_step * kSteps;
    const int64_t least = (hw + kMaxBlocks - 1) / kMaxBlocks;
    if (ppb < least) ppb = least;
    Split s;
    s.pixels_per_block = ppb;
    s.blocks = (int)((hw + ppb - 1) / ppb);
    return s;
}

// a := a (+) b, b the LATER run of pixels.  Comparisons drop NaN (the flags carry it); the sums carry it by themselves.
__device__ __forceinline__ void acc_fold(float& lo0, float& lo1, float& hi0, float& hi1, double& s0, double& s1, int& nan,
                                         int& count, float blo0, float blo1, float bhi0, float bhi1, double bs0, double bs1,
                                         int bnan, int bcount) {
    lo0 = blo0 < lo0 ? blo0 : lo0;
    lo1 = blo1 < lo1 ? blo1 : lo1;
    hi0 = bhi0 > hi0 ? bhi0 : hi0;
    hi1 = bhi1 > hi1 ? bhi1 : hi1;
    s0 += bs0;
    s1 += bs1;
    nan |= bnan;
    count += bcount;
}

// Folds the accumulators of the `slots` work-items of every channel (work-item tid = slot * d + c) into slot 0: a binary tree
// over the slot in LDS, slot i takes slot i + half -- always the same order.  Every work-item of the workgroup calls it.
template <int NT>
__device__ __forceinline__ void block_fold(float& lo0, float& lo1, float& hi0, float& hi1, double& s0, double& s1, int& nan,
                                           int& count, int tid, int slot, int slots, int d, double (*s_sum)[NT],
                                           float (*s_lohi)[NT], int* s_nan, int* s_count) {
    const bool active = slot < slots;
    int half = 1;
    while (half < slots) half <<= 1;
    for (half >>= 1; half > 0; half >>= 1) {                // (a round writes slots [half, 2 half): never what an earlier one reads)
        if (active && slot >= half && slot < 2 * half) {
            s_sum[0][tid] = s0;
            s_sum[1][tid] = s1;
            s_lohi[0][tid] = lo0;
            s_lohi[1][tid] = lo1;
            s_lohi[2][tid] = hi0;
            s_lohi[3][tid] = hi1;
            s_nan[tid] = nan;
            s_count[tid] = count;
        }
        __syncthreads();
        if (active && slot < half && slot + half < slots) {
            const int o = tid + half * d;                   // (slot + half, c): o < slots * d <= NT
            acc_fold(lo0, lo1, hi0, hi1, s0, s1, nan, count, s_lohi[0][o], s_lohi[1][o], s_lohi[2][o], s_lohi[3][o],
                     s_sum[0][o], s_sum[1][o], s_nan[o], s_count[o]);
        }
    }
}

struct Partials {
    double* sum;       // [n][blocks][2][d]
    float* lohi;       // [n][blocks][4][d]: min image, min mask, max image, max mask
    int32_t* nan;      // [n][blocks][d]
    int32_t* count;    // [n][blocks]
};

__global__ void __launch_bounds__(kST) stats_partial_kernel(const float* __restrict__ res, const uint8_t* __restrict__ mask,
                                                            int64_t hw, int d, Partials out) {
    __shared__ double s_sum[2][kST];
    __shared__ float s_lohi[4][kST];
    __shared__ int s_nan[kST];
    __shared__ int s_count[kST];
    const Split sp = split_image(hw, d);
    const int img = blockIdx.y, b = blockIdx.x, tid = threadIdx.x;
    const int per_step = kST / d;                           // pixel slots; work-item tid is slot tid / d, channel tid % d
    const int slot = tid / d, c = tid - slot * d;
    const bool active = slot < per_step;
    const int64_t p0 = (int64_t)b * sp.pixels_per_block;
    const int64_t p1 = p0 + sp.pixels_per_block < hw ? p0 + sp.pixels_per_block : hw;
    const float* r = res + (size_t)img * (size_t)hw * (size_t)d;
    const uint8_t* m = mask + (size_t)img * (size_t)hw;
    float lo0 = __builtin_inff(), lo1 = __builtin_inff(), hi0 = -__builtin_inff(), hi1 = -__builtin_inff();
    double s0 = 0.0, s1 = 0.0;
    int nan = 0, count = 0;
    if (active && p0 + slot < p1) {
        const int mine = (int)((p1 - (p0 + slot) + per_step - 1) / per_step);   // this work-item's elements: one per step
        const float* rp = r + (p0 + slot) * d + c;          // element i at rp[i * per_step * d], its mask byte at mp[i * per_step]
        const uint8_t* mp = m + (p0 + slot);
        for (int i = 0; i < mine; i += kBatch) {
            float x[kBatch];
            uint8_t on[kBatch];
#pragma unroll
            for (int k = 0; k < kBatch; ++k) {              // all loads first; past the last element: the last element again
                const int j = i + k < mine ? i + k : mine - 1;
                x[k] = rp[(int64_t)(j * per_step * d)];      // (mine * 256 < 2^31: a run has at most 2^21 pixels)
                on[k] = mp[(int64_t)(j * per_step)];
            }
            __builtin_amdgcn_sched_barrier(0);              // (keeps the compiler from sinking loads between the selects)
#pragma unroll
            for (int k = 0; k < kBatch; ++k) {
                const bool in = i + k < mine, im = in && on[k] != 0;
                const bool isnan = !(x[k] == x[k]);
                lo0 = (in && x[k] < lo0) ? x[k] : lo0;
                hi0 = (in && x[k] > hi0) ? x[k] : hi0;
                s0 += in ? (double)x[k] : 0.0;
                lo1 = (im && x[k] < lo1) ? x[k] : lo1;
                hi1 = (im && x[k] > hi1) ? x[k] : hi1;
                s1 += im ? (double)x[k] : 0.0;
                nan |= (in && isnan ? kNanImage : 0) | (im && isnan ? kNanMask : 0);
                count += (im && c == 0) ? 1 : 0;
            }
        }
    }
    block_fold<kST>(lo0, lo1, hi0, hi1, s0, s1, nan, count, tid, slot, per_step, d, s_sum, s_lohi, s_nan, s_count);
    if (tid < d) {                                          // slot 0: the workgroup's partial of channel c = tid
        const size_t blk = (size_t)img * sp.blocks + b;
        out.sum[(blk * 2 + 0) * d + c] = s0;
        out.sum[(blk * 2 + 1) * d + c] = s1;
        out.lohi[(blk * 4 + 0) * d + c] = lo0;
        out.lohi[(blk * 4 + 1) * d + c] = lo1;
        out.lohi[(blk * 4 + 2) * d + c] = hi0;
        out.lohi[(blk * 4 + 3) * d + c] = hi1;
        out.nan[blk * d + c] = nan;
        if (c == 0) out.count[blk] = count;
    }
}

__global__ void __launch_bounds__(kFT) stats_finish_kernel(Partials in, int64_t hw, int d, float* __restrict__ per_image,
                                                           int32_t* __restrict__ mask_pixels) {
    __shared__ double s_sum[2][kFT];
    __shared__ float s_lohi[4][kFT];
    __shared__ int s_nan[kFT];
    __shared__ int s_count[kFT];
    const Split sp = split_image(hw, d);
    const int img = blockIdx.x, tid = threadIdx.x;
    const int c0 = blockIdx.y * kFC, dc = d - c0 < kFC ? d - c0 : kFC;   // this workgroup's channels [c0, c0 + dc)
    const int runs = kFT / dc;                              // run r folds workgroups r, r + runs, r + 2 runs, ... in that order
    const int run = tid / dc, c = c0 + (tid - run * dc);
    float lo0 = __builtin_inff(), lo1 = __builtin_inff(), hi0 = -__builtin_inff(), hi1 = -__builtin_inff();
    double s0 = 0.0, s1 = 0.0;
    int nan = 0, count = 0;
    if (run < runs) {
        for (int b = run; b < sp.blocks; b += runs) {
            const size_t blk = (size_t)img * sp.blocks + b;
            acc_fold(lo0, lo1, hi0, hi1, s0, s1, nan, count, in.lohi[(blk * 4 + 0) * d + c], in.lohi[(blk * 4 + 1) * d + c],
                     in.lohi[(blk * 4 + 2) * d + c], in.lohi[(blk * 4 + 3) * d + c], in.sum[(blk * 2 + 0) * d + c],
                     in.sum[(blk * 2 + 1) * d + c], in.nan[blk * d + c], in.count[blk]);
        }
    }
    block_fold<kFT>(lo0, lo1, hi0, hi1, s0, s1, nan, count, tid, run, runs, dc, s_sum, s_lohi, s_nan, s_count);
    if (tid >= dc) return;
    // torch: a NaN in a channel makes its min, max and mean NaN (the sum carries it); an empty mask has no statistics
    const float qnan = __builtin_nanf("");
    float* o = per_image + (size_t)img * 6 * d + c;         // [2][3][d]: (image, mask) x (min, max, mean)
    o[0 * d] = (nan & kNanImage) ? qnan : lo0;
    o[1 * d] = (nan & kNanImage) ? qnan : hi0;
    o[2 * d] = (float)(s0 / (double)hw);
    const bool none = count == 0, bad = none || (nan & kNanMask);
    o[3 * d] = bad ? qnan : lo1;
    o[4 * d] = bad ? qnan : hi1;
    o[5 * d] = none ? qnan : (float)(s1 / (double)count);
    if (c == 0) mask_pixels[img] = count;
}

// torch.min / torch.max of two tensors: NaN if either is
__device__ __forceinline__ float min_nan(float a, float b) { return (a != a || b != b) ? __builtin_nanf("") : (b < a ? b : a); }
__device__ __forceinline__ float max_nan(float a, float b) { return (a != a || b != b) ? __builtin_nanf("") : (b > a ? b : a); }

__global__ void __launch_bounds__(kMaxD) stats_combine_kernel(const float* __restrict__ per_image,
                                                              const int32_t* __restrict__ mask_pixels, int n, int d,
                                                              float scale, float* __restrict__ stats,
                                                              int32_t* __restrict__ used) {
    const int c = threadIdx.x;
    if (c >= d) return;
    const float qnan = __builtin_nanf("");
    float lo[2] = {qnan, qnan}, hi[2] = {qnan, qnan}, mean[2] = {qnan, qnan};
    int count = 0;
    for (int i = 0; i < n; ++i) {
        if (mask_pixels[i] == 0) continue;                  // "Mask was empty, skipping" (:2280-2282): BOTH sets of statistics
        const float* s = per_image + (size_t)i * 6 * d + c;
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const float l = s[(3 * k + 0) * d], h = s[(3 * k + 1) * d], m = s[(3 * k + 2) * d];
            lo[k] = count == 0 ? l : min_nan(lo[k], l);
            hi[k] = count == 0 ? h : max_nan(hi[k], h);
            mean[k] = count == 0 ? m : mean[k] + m;         // stats_dict['mean'] += mean_temp, in fp32, in image order
        }
        ++count;
    }
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        stats[(3 * k + 0) * d + c] = lo[k];
        stats[(3 * k + 1) * d + c] = hi[k];
        stats[(3 * k + 2) * d + c] = count ? scale * mean[k] : qnan;   // 1.0 / num_images * val['mean'] (:2290)
    }
    if (c == 0) *used = count;
}

using dcn::align256;

inline bool shape_ok(int n, int h, int w, int d) {
    return n >= 1 && n <= 65535 && h >= 1 && w >= 1 && (int64_t)h * w < ((int64_t)1 << 31) && d >= 1 && d <= kMaxD;
}

}  // namespace

// sum [n][blocks][2][d] double | lohi [n][blocks][4][d] float | nan [n][blocks][d] int32 | count [n][blocks] int32
extern "C" size_t dcn_descriptor_statistics_workspace(int n, int h, int w, int d) {
    if (!shape_ok(n, h, w, d)) return 0;
    const size_t nb = (size_t)n * split_image((int64_t)h * w, d).blocks;
    return align256(nb * 2 * d * sizeof(double)) + align256(nb * 4 * d * sizeof(float)) + align256(nb * d * sizeof(int32_t)) +
           align256(nb * sizeof(int32_t));
}

extern "C" int dcn_descriptor_statistics(int n, int h, int w, int d, const float* res, const uint8_t* mask, float* per_image,
                                         int32_t* mask_pixels, void* workspace, void* stream) {
    if (!shape_ok(n, h, w, d) || !res || !mask || !per_image || !mask_pixels || !workspace) return DCN_E_INVALID;
    const int64_t hw = (int64_t)h * w;
    const Split sp = split_image(hw, d);
    const size_t nb = (size_t)n * sp.blocks;
    char* ws = (char*)workspace;
    Partials p;
    p.sum = (double*)ws;
    ws += align256(nb * 2 * d * sizeof(double));
    p.lohi = (float*)ws;
    ws += align256(nb * 4 * d * sizeof(float));
    p.nan = (int32_t*)ws;
    ws += align256(nb * d * sizeof(int32_t));
    p.count = (int32_t*)ws;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(stats_partial_kernel, dim3((unsigned)sp.blocks, (unsigned)n), dim3(kST), 0, st, res, mask, hw, d, p);
    hipLaunchKernelGGL(stats_finish_kernel, dim3((unsigned)n, (unsigned)dcn::ceil_div(d, kFC)), dim3(kFT), 0, st, p, hw, d, per_image, mask_pixels);
    return dcn::check_launch();
}

extern "C" int dcn_descriptor_statistics_combine(int n, int d, const float* per_image, const int32_t* mask_pixels,
                                                 int num_images, float* stats, int32_t* used, void* stream) {
    if (n < 1 || d < 1 || d > kMaxD || !per_image || !mask_pixels || num_images < 1 || !stats || !used) return DCN_E_INVALID;
    const float scale = (float)(1.0 / (double)num_images);
    hipLaunchKernelGGL(stats_combine_kernel, dim3(1), dim3(kMaxD), 0, (hipStream_t)stream, per_image, mask_pixels, n, d, scale,
                       stats, used);
    return dcn::check_launch();
}
