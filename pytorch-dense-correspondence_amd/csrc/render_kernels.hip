// Depth images and foreground masks of a triangle mesh seen from many camera poses (include/dcn_hip.h section 16): what the
// reference's data collection renders through director / VTK / OpenGL windows (modules/dense_correspondence_manipulation/
// change_detection/change_detection.py: ChangeDetection.run :336-408, render_depth_images :410-) as a z-buffer rasteriser whose
// every step is an integer or a correctly rounded float64 operation.  The arithmetic is render_raster.h's, for every path.
//
// dcn_render_depth, per group of frames (as many as the workspace holds, several per launch):
//   fill_words_kernel     the group's z-buffer (uint32 per pixel, all ones = no surface), the large-triangle counters
//   raster_small_kernel   grid (triangles / 256, frames).  A work-item sets up ONE triangle for its frame (9 gathered floats,
//                         12 float64 rows, 6 divisions), counts it when rule (c) or (d) drops it, and walks its bounding box:
//                         three int64 edge functions per pixel centre, and for a covered centre the perspective-correct depth
//                         and ONE global atomicMin on the pixel's millimetre value.  A triangle whose clipped box holds more
//                         than `large_threshold` pixels is not walked: its index goes to the frame's list (an atomic counter;
//                         the list's order varies from run to run, the image does not depend on it).
//   raster_large_kernel   grid (screen tiles of 64 x 16 pixels, frames).  Listed triangles are set up 64 at a time into LDS
//                         (one work-item each), then every work-item tests its own 4 pixels against those that touch the tile
//                         and keeps the minimum in registers -- a pixel has one owner, so the only memory operation per pixel
//                         is the final atomicMin into the z-buffer the small path wrote.
//   pack_kernel           z-buffer -> uint16 millimetres (all ones -> 0), two pixels per dword store; the at most one pixel
//                         in front of the first and behind the last aligned dword of the group is a 2-byte store.
//   HBM traffic per frame: T * (12 + 36) bytes of triangle reads (vertices gathered, mostly from L2), hw * (4 + 4 + 2) bytes
//   of z-buffer fill, read-back and image, one 4-byte atomic per covered (triangle, pixel centre).
// dcn_render_masks: one pass, four pixels per work-item, whole dwords (an 8-byte store for the depth image).
// Integer atomics only: every output is the same bit for bit from run to run.
#include "dcn_common.h"
#include "render_raster.h"

namespace {

namespace rs = dcn::raster;

#if defined(DCN_HOSTEMU_BUILD)
inline unsigned atomicMin(unsigned* p, unsigned v) {
    unsigned old = __atomic_load_n(p, __ATOMIC_RELAXED);
    while (v < old && !__atomic_compare_exchange_n(p, &old, v, false, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {}
    return old;
}
#endif

constexpr int kST = 256;                  // work-items of the small-triangle kernel: one triangle each
constexpr int kLT = 256;                  // work-items of the large-triangle kernel
constexpr int kTileW = 64, kTileH = 16;   // its screen tile: work-item (lx, ly) owns pixels (lx, ly + 4 k), k < 4
constexpr int kTilePix = kTileW * kTileH / kLT;
constexpr int kBatch = 64;                // listed triangles set up per round
constexpr int kMaxFrames = 64;            // frames per launch at most
constexpr int kDefaultLarge = 1024;       // pixels of a clipped bounding box above which a triangle is "large"
constexpr size_t kListBudget = (size_t)64 << 20;   // bytes of large-triangle lists per launch (one frame's list: 4 T bytes)
constexpr unsigned kEmpty = 0xffffffffu;

inline int frames_per_launch(int f, int64_t t) {
    int64_t n = (int64_t)(kListBudget / 4) / (t > 0 ? t : 1);
    n = n < 1 ? 1 : n;
    n = n > kMaxFrames ? kMaxFrames : n;
    return (int)(n > f ? f : n);
}

struct RenderArgs {
    const float* vertices;        // [V][3]
    const int32_t* triangles;     // [T][3]
    const float* poses;           // this group's [frames][16]
    unsigned* zbuf;               // [frames][hw]
    int32_t* large_count;         // [frames]
    int32_t* large_list;          // [frames][T]
    int32_t* status;              // this group's [frames][2]
    double fx, fy, cx, cy, z_near;
    int64_t t;
    int v, h, w, large_threshold;
};

__device__ __forceinline__ void camera_of(const RenderArgs& a, int f, rs::Camera& c) {
    rs::camera_from_pose(a.poses + (size_t)f * 16, c);
    c.fx = a.fx;
    c.fy = a.fy;
    c.cx = a.cx;
    c.cy = a.cy;
    c.z_near = a.z_near;
}

// Triangle i of the mesh in frame f: rs::kDraw and the triangle, or why not.  An index outside the vertex array (refused by the
// Python Mesh) draws nothing and is not counted.
__device__ __forceinline__ int triangle_of(const RenderArgs& a, const rs::Camera& c, int64_t i, rs::Tri& t) {
    const int32_t* ix = a.triangles + 3 * i;
    const int i0 = ix[0], i1 = ix[1], i2 = ix[2];
    if (i0 < 0 || i0 >= a.v || i1 < 0 || i1 >= a.v || i2 < 0 || i2 >= a.v) return rs::kNoArea;
    return rs::setup(c, a.vertices + 3 * (size_t)i0, a.vertices + 3 * (size_t)i1, a.vertices + 3 * (size_t)i2, t);
}

__global__ void __launch_bounds__(kST) raster_small_kernel(RenderArgs a) {
    __shared__ int s_dropped[2];
    const int f = blockIdx.y, tid = threadIdx.x;
    if (tid < 2) s_dropped[tid] = 0;
    __syncthreads();
    const int64_t i = (int64_t)blockIdx.x * kST + tid;
    if (i < a.t) {
        rs::Camera c;
        camera_of(a, f, c);
        rs::Tri t;
        const int verdict = triangle_of(a, c, i, t);
        if (verdict == rs::kNear) atomicAdd(&s_dropped[0], 1);
        if (verdict == rs::kOutside) atomicAdd(&s_dropped[1], 1);
        if (verdict == rs::kDraw) {
            const rs::Box b = rs::box_of(t, a.h, a.w);
            if (b.x1 >= b.x0 && b.y1 >= b.y0) {
                const int64_t pixels = (int64_t)(b.x1 - b.x0 + 1) * (b.y1 - b.y0 + 1);
                if (pixels > a.large_threshold) {
                    const int at = atomicAdd(&a.large_count[f], 1);          // (at < T: a triangle is listed once per frame)
                    a.large_list[(size_t)f * (size_t)a.t + at] = (int32_t)i;
                } else {
                    unsigned* z = a.zbuf + (size_t)f * (size_t)a.h * (size_t)a.w;
                    for (int py = b.y0; py <= b.y1; ++py)
                        for (int px = b.x0; px <= b.x1; ++px) {
                            unsigned mm;
                            if (rs::shade(t, px, py, mm)) atomicMin(&z[(size_t)py * a.w + px], mm);
                        }
                }
            }
        }
    }
    __syncthreads();
    if (tid < 2 && s_dropped[tid] != 0) atomicAdd(&a.status[2 * f + tid], s_dropped[tid]);
}

__global__ void __launch_bounds__(kLT) raster_large_kernel(RenderArgs a) {
    __shared__ int64_t s_xy[6][kBatch];
    __shared__ double s_z[3][kBatch];
    __shared__ int s_box[4][kBatch];
    const int f = blockIdx.y, tid = threadIdx.x;
    const int n = a.large_count[f];
    if (n == 0) return;                                      // (uniform per workgroup)
    const int tiles_x = dcn::ceil_div(a.w, kTileW);
    const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const int px = tx * kTileW + (tid & (kTileW - 1)), py0 = ty * kTileH + tid / kTileW;
    const int tile_x0 = tx * kTileW, tile_x1 = tile_x0 + kTileW - 1, tile_y0 = ty * kTileH, tile_y1 = tile_y0 + kTileH - 1;
    unsigned best[kTilePix];
#pragma unroll
    for (int k = 0; k < kTilePix; ++k) best[k] = kEmpty;
    rs::Camera c;
    camera_of(a, f, c);
    for (int j0 = 0; j0 < n; j0 += kBatch) {
        const int jn = n - j0 < kBatch ? n - j0 : kBatch;
        __syncthreads();                                     // the round before is read
        if (tid < jn) {
            rs::Tri t;
            rs::Box b;
            b.x0 = b.y0 = 0;
            b.x1 = b.y1 = -1;
            const int64_t i = a.large_list[(size_t)f * (size_t)a.t + j0 + tid];
            if (i >= 0 && i < a.t && triangle_of(a, c, i, t) == rs::kDraw) {
                b = rs::box_of(t, a.h, a.w);
                s_xy[0][tid] = t.x0;
                s_xy[1][tid] = t.y0;
                s_xy[2][tid] = t.x1;
                s_xy[3][tid] = t.y1;
                s_xy[4][tid] = t.x2;
                s_xy[5][tid] = t.y2;
                s_z[0][tid] = t.z0;
                s_z[1][tid] = t.z1;
                s_z[2][tid] = t.z2;
            }
            s_box[0][tid] = b.x0;
            s_box[1][tid] = b.y0;
            s_box[2][tid] = b.x1;
            s_box[3][tid] = b.y1;
        }
        __syncthreads();
        for (int j = 0; j < jn; ++j) {
            if (s_box[0][j] > tile_x1 || s_box[2][j] < tile_x0 || s_box[1][j] > tile_y1 || s_box[3][j] < tile_y0)
                continue;                                    // (uniform: the box misses the tile, or is empty)
            rs::Tri t;
            t.x0 = s_xy[0][j];
            t.y0 = s_xy[1][j];
            t.x1 = s_xy[2][j];
            t.y1 = s_xy[3][j];
            t.x2 = s_xy[4][j];
            t.y2 = s_xy[5][j];
            t.z0 = s_z[0][j];
            t.z1 = s_z[1][j];
            t.z2 = s_z[2][j];
#pragma unroll
            for (int k = 0; k < kTilePix; ++k) {
                const int py = py0 + k * (kLT / kTileW);
                unsigned mm;
                if (px < a.w && py < a.h && rs::shade(t, px, py, mm)) best[k] = mm < best[k] ? mm : best[k];
            }
        }
    }
    unsigned* z = a.zbuf + (size_t)f * (size_t)a.h * (size_t)a.w;
#pragma unroll
    for (int k = 0; k < kTilePix; ++k) {
        const int py = py0 + k * (kLT / kTileW);
        if (best[k] != kEmpty && px < a.w && py < a.h) atomicMin(&z[(size_t)py * a.w + px], best[k]);
    }
}

__device__ __forceinline__ unsigned millimetres(unsigned z) { return z == kEmpty ? 0u : z; }

// z [n] -> out [n] uint16 (out 2-byte aligned): pixel `head` is the first at a 4-byte aligned address
__global__ void __launch_bounds__(256) pack_kernel(const unsigned* __restrict__ z, uint16_t* __restrict__ out, int64_t n) {
    const int64_t head = (((uintptr_t)out & 2) != 0 && n > 0) ? 1 : 0;
    const int64_t words = (n - head) / 2;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < words; i += (int64_t)gridDim.x * 256) {
        const int64_t p = head + 2 * i;
        *(unsigned*)(out + p) = millimetres(z[p]) | (millimetres(z[p + 1]) << 16);
    }
    if (blockIdx.x == 0 && threadIdx.x < 2) {
        const int64_t p = threadIdx.x == 0 ? 0 : head + 2 * words;
        const bool mine = threadIdx.x == 0 ? head == 1 : p < n;
        if (mine) out[p] = (uint16_t)millimetres(z[p]);
    }
}

struct MaskArgs {
    const uint16_t* depth_f;      // [n]
    const uint16_t* depth_b;      // [n] or null: the crop rule
    uint8_t* mask;                // [n] 0 / 1
    uint8_t* visible;             // [n] 0 / 255, or null
    uint16_t* depth_change;       // [n] mask * depth_f, or null
    int64_t n;
    int threshold;
};

// computeForegroundMask / computeForegroundMaskFromDepthImagePair in int32 with zeros as INT32_MAX; without an image b,
// computeForegroundMaskUsingCropStrategy
__device__ __forceinline__ unsigned mask_of(const MaskArgs& a, unsigned f, unsigned b) {
    if (!a.depth_b) return f > 0u ? 1u : 0u;
    const int32_t fi = f == 0u ? INT32_MAX : (int32_t)f, bi = b == 0u ? INT32_MAX : (int32_t)b;
    return (bi - fi) > a.threshold ? 1u : 0u;              // (both in [1, INT32_MAX]: the difference is an int32)
}

__global__ void __launch_bounds__(256) mask_kernel(MaskArgs a) {
    const int64_t groups = a.n / 4;
    for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < groups; g += (int64_t)gridDim.x * 256) {
        const uint2 f = *(const uint2*)(a.depth_f + 4 * g);
        uint2 b = f;
        if (a.depth_b) b = *(const uint2*)(a.depth_b + 4 * g);
        const unsigned fv[4] = {f.x & 0xffffu, f.x >> 16, f.y & 0xffffu, f.y >> 16};
        const unsigned bv[4] = {b.x & 0xffffu, b.x >> 16, b.y & 0xffffu, b.y >> 16};
        unsigned m = 0, d[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const unsigned on = mask_of(a, fv[k], bv[k]);
            m |= on << (8 * k);
            d[k] = on ? fv[k] : 0u;                         // (on: depth_f is a real depth, below 65536)
        }
        *(unsigned*)(a.mask + 4 * g) = m;
        if (a.visible) *(unsigned*)(a.visible + 4 * g) = m * 255u;
        if (a.depth_change) {
            uint2 o;
            o.x = d[0] | (d[1] << 16);
            o.y = d[2] | (d[3] << 16);
            *(uint2*)(a.depth_change + 4 * g) = o;
        }
    }
    if (blockIdx.x == 0 && threadIdx.x < 3) {                // the last n % 4 pixels singly
        const int64_t p = 4 * groups + threadIdx.x;
        if (p < a.n) {
            const unsigned f = a.depth_f[p], b = a.depth_b ? a.depth_b[p] : 0u;
            const unsigned on = mask_of(a, f, b);
            a.mask[p] = (uint8_t)on;
            if (a.visible) a.visible[p] = (uint8_t)(on * 255u);
            if (a.depth_change) a.depth_change[p] = (uint16_t)(on ? f : 0u);
        }
    }
}

inline bool render_shape_ok(int v, int64_t t, int f, int h, int w) {
    return v >= 0 && t >= 0 && t < ((int64_t)1 << 31) && f >= 1 && h >= 1 && h <= rs::kMaxSide && w >= 1 && w <= rs::kMaxSide;
}

inline unsigned blocks_for(int64_t units) {
    int64_t b = dcn::ceil_div64(units, 256);
    return (unsigned)(b < 1 ? 1 : (b > 4096 ? 4096 : b));
}

}  // namespace

// z-buffer uint32 [fc][h * w] | large_count int32 [fc] | large_list int32 [fc][t], fc = frames per launch
extern "C" size_t dcn_render_depth_workspace(int v, int64_t t, int f, int h, int w) {
    if (!render_shape_ok(v, t, f, h, w)) return 0;
    const size_t fc = (size_t)frames_per_launch(f, t);
    return dcn::align256(fc * (size_t)h * (size_t)w * sizeof(unsigned)) + dcn::align256(fc * sizeof(int32_t)) +
           dcn::align256(fc * (size_t)(t > 0 ? t : 1) * sizeof(int32_t));
}

extern "C" int dcn_render_depth(int v, int64_t t, int f, int h, int w, const float* vertices, const int32_t* triangles,
                                const float* camera_to_world, double fx, double fy, double cx, double cy, double z_near,
                                int large_threshold, uint16_t* depth, int32_t* status, void* workspace, void* stream) {
    if (!render_shape_ok(v, t, f, h, w) || (t > 0 && (!vertices || !triangles || v < 1)) || !camera_to_world || !depth ||
        !status || !workspace || !(z_near > 0.0) || !(z_near < 65.536) || !(fx == fx && fy == fy && cx == cx && cy == cy) ||
        ((uintptr_t)depth & 1))
        return DCN_E_INVALID;
    hipStream_t st = (hipStream_t)stream;
    const int fc = frames_per_launch(f, t);
    const size_t hw = (size_t)h * (size_t)w;
    RenderArgs a;
    a.vertices = vertices;
    a.triangles = triangles;
    a.zbuf = (unsigned*)workspace;
    a.large_count = (int32_t*)((char*)workspace + dcn::align256((size_t)fc * hw * sizeof(unsigned)));
    a.large_list = (int32_t*)((char*)a.large_count + dcn::align256((size_t)fc * sizeof(int32_t)));
    a.fx = fx;
    a.fy = fy;
    a.cx = cx;
    a.cy = cy;
    a.z_near = z_near;
    a.t = t;
    a.v = v;
    a.h = h;
    a.w = w;
    a.large_threshold = large_threshold < 0 ? kDefaultLarge : large_threshold;
    int rc = dcn::fill_bytes_async(status, 0, (size_t)f * 2 * sizeof(int32_t), st);
    const unsigned tiles = (unsigned)(dcn::ceil_div(w, kTileW) * dcn::ceil_div(h, kTileH));
    for (int f0 = 0; f0 < f && rc == DCN_OK; f0 += fc) {
        const int fn = f - f0 < fc ? f - f0 : fc;
        a.poses = camera_to_world + (size_t)f0 * 16;
        a.status = status + (size_t)f0 * 2;
        rc = dcn::fill_bytes_async(a.zbuf, 0xff, (size_t)fn * hw * sizeof(unsigned), st);
        if (rc == DCN_OK) rc = dcn::fill_bytes_async(a.large_count, 0, (size_t)fn * sizeof(int32_t), st);
        if (rc != DCN_OK) break;
        if (t > 0) {
            hipLaunchKernelGGL(raster_small_kernel, dim3((unsigned)dcn::ceil_div64(t, kST), (unsigned)fn), dim3(kST), 0, st, a);
            hipLaunchKernelGGL(raster_large_kernel, dim3(tiles, (unsigned)fn), dim3(kLT), 0, st, a);
        }
        const int64_t n = (int64_t)fn * (int64_t)hw;
        hipLaunchKernelGGL(pack_kernel, dim3(blocks_for(n / 2)), dim3(256), 0, st, (const unsigned*)a.zbuf,
                           depth + (size_t)f0 * hw, n);
        rc = dcn::check_launch();
    }
    return rc;
}

extern "C" int dcn_render_masks(int64_t n, const uint16_t* depth_f, const uint16_t* depth_b, int threshold, uint8_t* mask,
                                uint8_t* visible, uint16_t* depth_change, void* stream) {
    if (n < 1 || !depth_f || !mask || threshold < 0 || ((uintptr_t)depth_f & 7) || (depth_b && ((uintptr_t)depth_b & 7)) ||
        ((uintptr_t)mask & 3) || (visible && ((uintptr_t)visible & 3)) || (depth_change && ((uintptr_t)depth_change & 7)))
        return DCN_E_INVALID;
    MaskArgs a;
    a.depth_f = depth_f;
    a.depth_b = depth_b;
    a.mask = mask;
    a.visible = visible;
    a.depth_change = depth_change;
    a.n = n;
    a.threshold = threshold;
    hipLaunchKernelGGL(mask_kernel, dim3(blocks_for(n / 4)), dim3(256), 0, (hipStream_t)stream, a);
    return dcn::check_launch();
}
