// Painting mesh vertices from their views (include/dcn_hip.h section 18): colour fusion (uint8 RGB views) and the
// descriptor-coloured mesh (float descriptor views) as ONE operation -- per vertex and view: project, decide whether the view
// sees the vertex, read the view's pixel, accumulate count, sum and sum of squares in float64.  The arithmetic is paint_rules.h's.
//
// dcn_mesh_paint, per chunk of frames (at most 64 per launch):
//   paint_kernel<T, CT>   one work-item per vertex (integrate_kernel's pattern).  The chunk's world-to-camera rows (12 float64 per
//                         frame) are built once per workgroup into LDS by its first work-items and read from there as broadcasts.
//                         CT is the smallest of 4, 8, 16, 32 that holds the c channels (a kernel instance each): the 2 * CT
//                         float64 sums stay in registers over the chunk -- every index into them is a constant after unrolling,
//                         so nothing spills -- and take ONE read-modify-write per vertex and launch.  (Smaller tiles walked in an
//                         outer loop, projecting again per tile, were slower at every size: profiles/EXPERIMENTS.md.)  One
//                         gathered 2-byte depth read, one mask byte and one pixel of c values per (vertex, frame) that sees the
//                         vertex; the pixel's channels are contiguous and are read as 16-byte (float) or 4-byte (uint8) words
//                         where c is a multiple of four.
// dcn_mesh_paint_finish:
//   finish_kernel         one work-item per vertex: means, the variance summed over the channels, the colour bytes.
// No atomics: a vertex owns its state.  No host synchronisation.
#include "dcn_common.h"
#include "paint_rules.h"

namespace {

namespace pt = dcn::paint;
namespace fu = dcn::fusion;
namespace rs = dcn::raster;

constexpr int kNT = 256;                  // work-items of both kernels
constexpr int kMaxChunk = 64;             // frames per launch at most, and the default

inline unsigned blocks_of(int64_t n) { return (unsigned)dcn::ceil_div64(n > 0 ? n : 1, kNT); }

struct PaintArgs {
    fu::Pinhole k;
    const float* vertices;
    const int32_t* valid;         // device int32 [1] or NULL
    const void* images;           // this chunk's [frames][h][w][c]
    const uint16_t* depth;        // this chunk's [frames][h][w]
    const uint8_t* mask;          // this chunk's [frames][h][w] or NULL
    const float* poses;           // this chunk's [frames][16]
    int32_t* count;
    double* sum;
    double* sumsq;
    double margin;
    int v, h, w, c, frames, wide; // wide: c is a multiple of four and the images are aligned for whole words of four channels
};

__device__ __forceinline__ void load4(const float* p, double* x) {
    const float4 q = *reinterpret_cast<const float4*>(p);
    x[0] = (double)q.x;
    x[1] = (double)q.y;
    x[2] = (double)q.z;
    x[3] = (double)q.w;
}

__device__ __forceinline__ void load4(const uint8_t* p, double* x) {
    const uint32_t q = *reinterpret_cast<const uint32_t*>(p);
    x[0] = (double)(q & 255u);
    x[1] = (double)((q >> 8) & 255u);
    x[2] = (double)((q >> 16) & 255u);
    x[3] = (double)(q >> 24);
}

// step 7 for the channels [0, left) of the pixel at p; every index into sum / sumsq is a constant after unrolling
template <typename T, int CT>
__device__ __forceinline__ void take_tile(const T* __restrict__ p, int left, bool wide, double* sum, double* sumsq) {
    if (wide) {
#pragma unroll
        for (int j = 0; j < CT; j += 4) {
            if (j < left) {                                  // (left is a multiple of four here)
                double x[4];
                load4(p + j, x);
#pragma unroll
                for (int e = 0; e < 4; ++e) pt::take(x[e], sum[j + e], sumsq[j + e]);
            }
        }
    } else {
#pragma unroll
        for (int j = 0; j < CT; ++j)
            if (j < left) pt::take((double)p[j], sum[j], sumsq[j]);
    }
}

template <typename T, int CT>
__global__ void __launch_bounds__(kNT) paint_kernel(PaintArgs a) {
    __shared__ double s_cam[kMaxChunk * 12];
    const int tid = threadIdx.x;
    if (tid < a.frames) {
        rs::Camera c;
        rs::camera_from_pose(a.poses + (size_t)tid * 16, c);
#pragma unroll
        for (int e = 0; e < 12; ++e) s_cam[12 * tid + e] = c.a[e];
    }
    __syncthreads();
    int limit = a.v;
    if (a.valid) {
        const int n = a.valid[0];
        limit = n < 0 ? 0 : (n < limit ? n : limit);
    }
    const int64_t idx = (int64_t)blockIdx.x * kNT + tid;
    if (idx >= limit) return;
    const double wx = (double)a.vertices[3 * idx], wy = (double)a.vertices[3 * idx + 1], wz = (double)a.vertices[3 * idx + 2];
    const size_t hw = (size_t)a.h * (size_t)a.w;
    const T* images = static_cast<const T*>(a.images);
    double* g_sum = a.sum + (size_t)idx * a.c;
    double* g_sumsq = a.sumsq + (size_t)idx * a.c;
    double sum[CT], sumsq[CT];                               // (a.c <= CT)
#pragma unroll
    for (int j = 0; j < CT; ++j) {
        sum[j] = j < a.c ? g_sum[j] : 0.0;
        sumsq[j] = j < a.c ? g_sumsq[j] : 0.0;
    }
    int seen = 0;
    for (int f = 0; f < a.frames; ++f) {
        const int pixel = pt::visible(&s_cam[12 * f], a.k, wx, wy, wz, a.depth + (size_t)f * hw,
                                      a.mask ? a.mask + (size_t)f * hw : nullptr, a.h, a.w, a.margin);
        if (pixel < 0) continue;
        ++seen;
        take_tile<T, CT>(images + ((size_t)f * hw + (size_t)pixel) * a.c, a.c, a.wide != 0, sum, sumsq);
    }
#pragma unroll
    for (int j = 0; j < CT; ++j) {
        if (j < a.c) {
            g_sum[j] = sum[j];
            g_sumsq[j] = sumsq[j];
        }
    }
    a.count[idx] += seen;
}

struct FinishArgs {
    const int32_t* count;
    const double* sum;
    const double* sumsq;
    const double* lo;
    const double* hi;
    float* mean;
    float* variance;
    uint8_t* colours;             // or NULL
    int v, c, min_views;
    int channel[3];
    uint8_t unseen[3];
};

__global__ void __launch_bounds__(kNT) finish_kernel(FinishArgs a) {
    const int64_t idx = (int64_t)blockIdx.x * kNT + threadIdx.x;
    if (idx >= a.v) return;
    const int n = a.count[idx];
    const bool painted = n >= a.min_views;
    const double* sum = a.sum + (size_t)idx * a.c;
    const double* sumsq = a.sumsq + (size_t)idx * a.c;
    float* mean = a.mean + (size_t)idx * a.c;
    double total = 0.0;
    for (int ch = 0; ch < a.c; ++ch) {
        mean[ch] = painted ? (float)pt::mean_of(sum[ch], n) : 0.0f;
        if (painted) total = rs::add(total, pt::variance_of(sum[ch], sumsq[ch], n));
    }
    a.variance[idx] = painted ? (float)total : __builtin_nanf("");
    if (a.colours) {
#pragma unroll
        for (int e = 0; e < 3; ++e) {
            const int ch = a.channel[e];
            a.colours[3 * idx + e] = painted ? pt::colour_byte(pt::mean_of(sum[ch], n), a.lo[ch], a.hi[ch]) : a.unseen[e];
        }
    }
}

template <typename T>
inline void launch_paint(unsigned blocks, hipStream_t st, const PaintArgs& a) {      // the smallest tile that holds a.c
    if (a.c <= 4)
        hipLaunchKernelGGL((paint_kernel<T, 4>), dim3(blocks), dim3(kNT), 0, st, a);
    else if (a.c <= 8)
        hipLaunchKernelGGL((paint_kernel<T, 8>), dim3(blocks), dim3(kNT), 0, st, a);
    else if (a.c <= 16)
        hipLaunchKernelGGL((paint_kernel<T, 16>), dim3(blocks), dim3(kNT), 0, st, a);
    else
        hipLaunchKernelGGL((paint_kernel<T, 32>), dim3(blocks), dim3(kNT), 0, st, a);
}

inline bool is_finite(double x) { return x - x == 0.0; }

}  // namespace

extern "C" int dcn_mesh_paint(int v, const float* vertices, const int32_t* valid_vertices, int f, int h, int w, int c,
                              int image_type, const void* images, const uint16_t* depth, const uint8_t* mask,
                              const float* camera_to_world, double fx, double fy, double cx, double cy, double pixel_offset,
                              double margin_mm, int frames_per_launch, int32_t* count, double* sum, double* sumsq, void* stream) {
    if (v < 0 || f < 1 || h < 1 || h > rs::kMaxSide || w < 1 || w > rs::kMaxSide || c < 1 || c > pt::kMaxChannels ||
        (image_type != DCN_PAINT_UINT8 && image_type != DCN_PAINT_FLOAT) || !images || !depth || !camera_to_world ||
        !(margin_mm >= 0.0) || !is_finite(margin_mm) || frames_per_launch == 0 || frames_per_launch > kMaxChunk ||
        !(fx == fx && fy == fy && cx == cx && cy == cy && pixel_offset == pixel_offset) || ((uintptr_t)depth & 1) ||
        (image_type == DCN_PAINT_FLOAT && ((uintptr_t)images & 3)))
        return DCN_E_INVALID;
    if (v == 0) return DCN_OK;
    if (!vertices || !count || !sum || !sumsq || ((uintptr_t)sum & 7) || ((uintptr_t)sumsq & 7)) return DCN_E_INVALID;
    const int chunk = frames_per_launch < 0 ? kMaxChunk : frames_per_launch;
    const size_t pixel_bytes = (size_t)c * (image_type == DCN_PAINT_FLOAT ? 4 : 1);
    PaintArgs a;
    a.k.fx = fx;
    a.k.fy = fy;
    a.k.cx = cx;
    a.k.cy = cy;
    a.k.offset = pixel_offset;
    a.vertices = vertices;
    a.valid = valid_vertices;
    a.count = count;
    a.sum = sum;
    a.sumsq = sumsq;
    a.margin = margin_mm;
    a.v = v;
    a.h = h;
    a.w = w;
    a.c = c;
    a.wide = (c % 4 == 0 && ((uintptr_t)images & (image_type == DCN_PAINT_FLOAT ? 15 : 3)) == 0) ? 1 : 0;
    const size_t hw = (size_t)h * (size_t)w;
    for (int f0 = 0; f0 < f; f0 += chunk) {
        a.frames = f - f0 < chunk ? f - f0 : chunk;
        a.images = (const char*)images + (size_t)f0 * hw * pixel_bytes;
        a.depth = depth + (size_t)f0 * hw;
        a.mask = mask ? mask + (size_t)f0 * hw : nullptr;
        a.poses = camera_to_world + (size_t)f0 * 16;
        if (image_type == DCN_PAINT_FLOAT)
            launch_paint<float>(blocks_of(v), (hipStream_t)stream, a);
        else
            launch_paint<uint8_t>(blocks_of(v), (hipStream_t)stream, a);
    }
    return dcn::check_launch();
}

extern "C" int dcn_mesh_paint_finish(int v, int c, const int32_t* count, const double* sum, const double* sumsq, int min_views,
                                     float* mean, float* variance, int channel0, int channel1, int channel2, const double* lo,
                                     const double* hi, int unseen_red, int unseen_green, int unseen_blue, uint8_t* colours,
                                     void* stream) {
    if (v < 0 || c < 1 || c > pt::kMaxChannels || min_views < 1) return DCN_E_INVALID;
    FinishArgs a;
    a.channel[0] = channel0;
    a.channel[1] = channel1;
    a.channel[2] = channel2;
    const int unseen[3] = {unseen_red, unseen_green, unseen_blue};
    for (int e = 0; e < 3; ++e) {
        if (colours && (a.channel[e] < 0 || a.channel[e] >= c || unseen[e] < 0 || unseen[e] > 255)) return DCN_E_INVALID;
        a.unseen[e] = (uint8_t)unseen[e];
    }
    if (colours && (!lo || !hi)) return DCN_E_INVALID;
    if (v == 0) return DCN_OK;
    if (!count || !sum || !sumsq || !mean || !variance) return DCN_E_INVALID;
    a.count = count;
    a.sum = sum;
    a.sumsq = sumsq;
    a.lo = lo;
    a.hi = hi;
    a.mean = mean;
    a.variance = variance;
    a.colours = colours;
    a.v = v;
    a.c = c;
    a.min_views = min_views;
    hipLaunchKernelGGL(finish_kernel, dim3(blocks_of(v)), dim3(kNT), 0, (hipStream_t)stream, a);
    return dcn::check_launch();
}
