// TSDF fusion of logged depth images, surface extraction and the box crop (include/dcn_hip.h section 17): what the reference's
// data processing gets from its collaborators -- a CUDA tsdf-fusion binary, marching cubes and director's cropToBox
// (doc/data_processing_single_scene.md, fusion_reconstruction.py) -- with every step an integer or a correctly rounded float64
// operation.  The arithmetic is fusion_rules.h's.
//
// dcn_tsdf_integrate, per chunk of frames (at most 64 per launch):
//   integrate_kernel      one work-item per voxel, x fastest.  The chunk's world-to-camera rows (12 float64 per frame) are built
//                         once per workgroup into LDS by its first work-items and read from there as broadcasts; sum and weight
//                         stay in registers over the chunk: ONE 8-byte read-modify-write per voxel and launch, one gathered
//                         2-byte depth read per (voxel, frame) that projects into the image.  Frames are walked in order, so the
//                         saturated voxels take exactly the frames a walk over all frames would give them.
// dcn_tsdf_extract (marching tetrahedra on the Kuhn split):
//   cube_kernel           per voxel: the inside bits of the 8 corners of its cube and whether the cube is valid
//   count_kernel          per voxel: which of its 7 edges carry a vertex, how many triangles its cube emits
//   the scan (below)      exclusive scans of both counts
//   vertex_kernel         per voxel: its vertices, at their scanned rows
//   triangle_kernel       per voxel: its cube's triangles; a vertex id is the scanned offset of the edge's lower voxel plus the
//                         number of lower edge bits
// dcn_mesh_crop: mark_kernel (surviving triangles, vertices in use), the scan of both, compact_kernel.
// The scan is reduce-then-scan over workgroups of 256 counts: scan_reduce_kernel (a workgroup's total, int64),
// scan_blocks_kernel (ONE workgroup scans the totals), scan_apply_kernel (the scan inside a workgroup in LDS plus its offset).
// Integers only: no order dependence, no waiting of one workgroup for another.
#include "dcn_common.h"
#include "fusion_rules.h"

namespace {

namespace fu = dcn::fusion;
namespace rs = dcn::raster;

constexpr int kNT = 256;                  // work-items of every kernel here
constexpr int kMaxChunk = 64;             // frames per launch at most
constexpr int kDefaultChunk = 32;

inline unsigned blocks_of(int64_t n) { return (unsigned)dcn::ceil_div64(n > 0 ? n : 1, kNT); }

struct Grid {
    double ox, oy, oz, s;
    int64_t n;
    int nx, ny, nz;
};

__device__ __forceinline__ void voxel_of(const Grid& g, int64_t idx, int& i, int& j, int& k) {
    const int64_t row = idx / g.nx;
    i = (int)(idx - row * g.nx);
    k = (int)(row / g.ny);
    j = (int)(row - (int64_t)k * g.ny);
}

// ------------------------------------------------------------------------------------------------ 17a
struct IntegrateArgs {
    Grid g;
    fu::Pinhole k;
    int32_t* sum;
    int32_t* weight;
    int32_t* status;
    const uint16_t* depth;        // this chunk's [frames][h][w]
    const float* poses;           // this chunk's [frames][16]
    double mu;
    int h, w, max_mm, frames;
};

__global__ void __launch_bounds__(kNT) integrate_kernel(IntegrateArgs a) {
    __shared__ double s_cam[kMaxChunk * 12];
    __shared__ int s_full;
    const int tid = threadIdx.x;
    if (tid == 0) s_full = 0;
    if (tid < a.frames) {
        rs::Camera c;
        rs::camera_from_pose(a.poses + (size_t)tid * 16, c);
#pragma unroll
        for (int e = 0; e < 12; ++e) s_cam[12 * tid + e] = c.a[e];
    }
    __syncthreads();
    const int64_t idx = (int64_t)blockIdx.x * kNT + tid;
    int full = 0;
    if (idx < a.g.n) {
        int i, j, k;
        voxel_of(a.g, idx, i, j, k);
        const double wx = fu::voxel_centre(a.g.ox, a.g.s, i), wy = fu::voxel_centre(a.g.oy, a.g.s, j),
                     wz = fu::voxel_centre(a.g.oz, a.g.s, k);
        int sum = a.sum[idx], weight = a.weight[idx];
        const size_t hw = (size_t)a.h * (size_t)a.w;
        for (int f = 0; f < a.frames; ++f) {
            int q;
            if (!fu::observe(&s_cam[12 * f], a.k, wx, wy, wz, a.depth + (size_t)f * hw, a.h, a.w, a.max_mm, a.mu, q)) continue;
            if (weight >= fu::kMaxWeight) {
                ++full;
            } else {
                sum += q;
                ++weight;
            }
        }
        a.sum[idx] = sum;
        a.weight[idx] = weight;
    }
    if (full) atomicAdd(&s_full, full);
    __syncthreads();
    if (tid == 0 && s_full != 0) atomicAdd(&a.status[0], s_full);
}

// ------------------------------------------------------------------------------------------------ the scan
// counts int32 [n] -> their exclusive scan in place (saturating at INT32_MAX), the total int64.  totals: int64 [blocks_of(n) + 1]
__global__ void __launch_bounds__(kNT) scan_reduce_kernel(const int32_t* __restrict__ counts, int64_t n, int64_t* __restrict__ totals) {
    __shared__ int s_sum;                                   // (256 counts of one workgroup: every count here is below 2^23)
    if (threadIdx.x == 0) s_sum = 0;
    __syncthreads();
    const int64_t idx = (int64_t)blockIdx.x * kNT + threadIdx.x;
    const int c = idx < n ? counts[idx] : 0;
    if (c) atomicAdd(&s_sum, c);
    __syncthreads();
    if (threadIdx.x == 0) totals[blockIdx.x] = s_sum;
}

// ONE workgroup: totals [nb] -> their exclusive scan in place, totals[nb] = the sum.  A work-item owns a contiguous run.
__global__ void __launch_bounds__(kNT) scan_blocks_kernel(int64_t* __restrict__ totals, int64_t nb) {
    __shared__ int64_t s_run[kNT];
    const int tid = threadIdx.x;
    const int64_t per = dcn::ceil_div64(nb, kNT), b0 = per * tid, b1 = b0 + per < nb ? b0 + per : nb;
    int64_t mine = 0;
    for (int64_t b = b0; b < b1; ++b) mine += totals[b];
    s_run[tid] = mine;
    __syncthreads();
    if (tid == 0) {
        int64_t at = 0;
        for (int t = 0; t < kNT; ++t) {
            const int64_t r = s_run[t];
            s_run[t] = at;
            at += r;
        }
        totals[nb] = at;
    }
    __syncthreads();
    int64_t at = s_run[tid];
    for (int64_t b = b0; b < b1; ++b) {
        const int64_t r = totals[b];
        totals[b] = at;
        at += r;
    }
}

__global__ void __launch_bounds__(kNT) scan_apply_kernel(int32_t* __restrict__ counts, int64_t n, const int64_t* __restrict__ totals) {
    __shared__ int s_scan[2][kNT];
    const int tid = threadIdx.x;
    const int64_t idx = (int64_t)blockIdx.x * kNT + tid;
    const int c = idx < n ? counts[idx] : 0;
    int cur = 0;
    s_scan[0][tid] = c;
    __syncthreads();
    for (int step = 1; step < kNT; step <<= 1) {            // inclusive scan, doubling
        const int v = s_scan[cur][tid] + (tid >= step ? s_scan[cur][tid - step] : 0);
        s_scan[cur ^ 1][tid] = v;
        cur ^= 1;
        __syncthreads();
    }
    if (idx < n) {
        const int64_t at = totals[blockIdx.x] + (int64_t)(s_scan[cur][tid] - c);
        counts[idx] = at > (int64_t)INT32_MAX ? INT32_MAX : (int32_t)at;
    }
}

// totals must hold blocks_of(n) + 1 values; afterwards totals[blocks_of(n)] is the sum
inline void scan_in_place(int32_t* counts, int64_t n, int64_t* totals, hipStream_t st) {
    const unsigned nb = blocks_of(n);
    hipLaunchKernelGGL(scan_reduce_kernel, dim3(nb), dim3(kNT), 0, st, (const int32_t*)counts, n, totals);
    hipLaunchKernelGGL(scan_blocks_kernel, dim3(1), dim3(kNT), 0, st, totals, (int64_t)nb);
    hipLaunchKernelGGL(scan_apply_kernel, dim3(nb), dim3(kNT), 0, st, counts, n, (const int64_t*)totals);
}

__device__ __forceinline__ int32_t clamp_count(int64_t v) { return v > (int64_t)INT32_MAX ? INT32_MAX : (int32_t)v; }

__global__ void publish_counts_kernel(const int64_t* v_total, const int64_t* t_total, int32_t* counts) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        counts[0] = clamp_count(*v_total);
        counts[1] = clamp_count(*t_total);
    }
}

// ------------------------------------------------------------------------------------------------ 17b
struct ExtractArgs {
    Grid g;
    const int32_t* sum;
    const int32_t* weight;
    uint16_t* cube;               // [n] bits 0-7: corner c is inside, bit 8: the cube is valid
    uint8_t* edges;               // [n] bit d: the edge of direction d from this voxel carries a vertex
    int32_t* v_at;                // [n] vertices per voxel, then their exclusive scan
    int32_t* t_at;                // [n] triangles per cube, then their exclusive scan
    float* vertices;
    int32_t* triangles;
    int min_weight, max_v, max_t;
};

constexpr unsigned kCubeValid = 0x100u;

__global__ void __launch_bounds__(kNT) cube_kernel(ExtractArgs a) {
    const int64_t idx = (int64_t)blockIdx.x * kNT + threadIdx.x;
    if (idx >= a.g.n) return;
    int i, j, k;
    voxel_of(a.g, idx, i, j, k);
    unsigned code = 0;
    if (i + 1 < a.g.nx && j + 1 < a.g.ny && k + 1 < a.g.nz) {
        bool valid = true;
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const int64_t at = idx + (c & 1) + (int64_t)(c >> 1 & 1) * a.g.nx + (int64_t)(c >> 2) * a.g.nx * a.g.ny;
            valid = valid && a.weight[at] >= a.min_weight;
            code |= (a.sum[at] < 0 ? 1u : 0u) << c;
        }
        code = valid ? (code | kCubeValid) : 0u;
    }
    a.cube[idx] = (uint16_t)code;
}

__device__ __forceinline__ int triangles_of_cube(unsigned code) {
    int n = 0;
#pragma unroll
    for (int tet = 0; tet < 6; ++tet) {
        unsigned m = 0;
#pragma unroll
        for (int v = 0; v < 4; ++v) m |= ((code >> fu::tet_corner(tet, v)) & 1u) << v;
        n += (int)((fu::kTetCases[m] >> 16) & 3u);
    }
    return n;
}

__global__ void __launch_bounds__(kNT) count_kernel(ExtractArgs a) {
    const int64_t idx = (int64_t)blockIdx.x * kNT + threadIdx.x;
    if (idx >= a.g.n) return;
    int i, j, k;
    voxel_of(a.g, idx, i, j, k);
    const int64_t sy = a.g.nx, sz = (int64_t)a.g.nx * a.g.ny;
    const bool in_a = a.sum[idx] < 0;
    unsigned edges = 0;
#pragma unroll
    for (int d = 0; d < 7; ++d) {
        const unsigned b = fu::direction_bits(d);
        const int bx = b & 1u, by = (b >> 1) & 1u, bz = b >> 2;
        if (i + bx >= a.g.nx || j + by >= a.g.ny || k + bz >= a.g.nz) continue;
        if ((a.sum[idx + bx + by * sy + bz * sz] < 0) == in_a) continue;
        // a valid cube with both ends among its corners: its origin is this voxel, stepped back along the axes b leaves alone
        bool held = false;
#pragma unroll
        for (unsigned e = 0; e < 8; ++e) {
            if (e & b) continue;
            const int ex = e & 1u, ey = (e >> 1) & 1u, ez = e >> 2;
            if (i < ex || j < ey || k < ez) continue;
            held = held || (a.cube[idx - ex - ey * sy - ez * sz] & kCubeValid) != 0;
        }
        if (held) edges |= 1u << d;
    }
    const unsigned code = a.cube[idx];
    a.edges[idx] = (uint8_t)edges;
    a.v_at[idx] = __builtin_popcount(edges);
    a.t_at[idx] = (code & kCubeValid) ? triangles_of_cube(code) : 0;
}

__global__ void __launch_bounds__(kNT) vertex_kernel(ExtractArgs a) {
    const int64_t idx = (int64_t)blockIdx.x * kNT + threadIdx.x;
    if (idx >= a.g.n) return;
    const unsigned edges = a.edges[idx];
    if (!edges) return;
    int i, j, k;
    voxel_of(a.g, idx, i, j, k);
    const int64_t sy = a.g.nx, sz = (int64_t)a.g.nx * a.g.ny;
    const int sum_a = a.sum[idx], weight_a = a.weight[idx];
    int64_t row = a.v_at[idx];
#pragma unroll
    for (int d = 0; d < 7; ++d) {
        if (!((edges >> d) & 1u)) continue;
        if (row < a.max_v) {
            const unsigned b = fu::direction_bits(d);
            const int64_t at = idx + (b & 1u) + ((b >> 1) & 1u) * sy + (b >> 2) * sz;
            float p[3];
            fu::edge_vertex(i, j, k, b, sum_a, weight_a, a.sum[at], a.weight[at], a.g.ox, a.g.oy, a.g.oz, a.g.s, p);
            a.vertices[3 * row] = p[0];
            a.vertices[3 * row + 1] = p[1];
            a.vertices[3 * row + 2] = p[2];
        }
        ++row;
    }
}

// The vertex id of the cube edge between corners c0 and c1 of the cube at idx; -1 when that vertex has no row
__device__ __forceinline__ int32_t vertex_id(const ExtractArgs& a, int64_t idx, unsigned c0, unsigned c1) {
    const unsigned lo = c0 & c1;                             // (Kuhn split: one end dominates the other)
    const int d = fu::direction_id(c0 ^ c1);
    const int64_t at = idx + (lo & 1u) + (int64_t)((lo >> 1) & 1u) * a.g.nx + (int64_t)(lo >> 2) * a.g.nx * a.g.ny;
    const int64_t id = (int64_t)a.v_at[at] + __builtin_popcount((unsigned)a.edges[at] & ((1u << d) - 1u));
    return id < a.max_v ? (int32_t)id : -1;
}

__global__ void __launch_bounds__(kNT) triangle_kernel(ExtractArgs a) {
    const int64_t idx = (int64_t)blockIdx.x * kNT + threadIdx.x;
    if (idx >= a.g.n) return;
    const unsigned code = a.cube[idx];
    if (!(code & kCubeValid)) return;
    int64_t row = a.t_at[idx];
#pragma unroll
    for (int tet = 0; tet < 6; ++tet) {
        unsigned m = 0;
#pragma unroll
        for (int v = 0; v < 4; ++v) m |= ((code >> fu::tet_corner(tet, v)) & 1u) << v;
        const unsigned word = fu::kTetCases[m];
        const int nt = (int)((word >> 16) & 3u);
        if (nt == 0) continue;
        const bool flip = (((word >> 18) ^ (fu::kOddTets >> tet)) & 1u) != 0;
        int32_t e0 = 0, e1 = 0, e2 = 0, e3 = 0;
        e0 = vertex_id(a, idx, fu::tet_corner(tet, word & 3u), fu::tet_corner(tet, (word >> 2) & 3u));
        e1 = vertex_id(a, idx, fu::tet_corner(tet, (word >> 4) & 3u), fu::tet_corner(tet, (word >> 6) & 3u));
        e2 = vertex_id(a, idx, fu::tet_corner(tet, (word >> 8) & 3u), fu::tet_corner(tet, (word >> 10) & 3u));
        if (nt == 2) e3 = vertex_id(a, idx, fu::tet_corner(tet, (word >> 12) & 3u), fu::tet_corner(tet, (word >> 14) & 3u));
        if (row < a.max_t) {
            const bool whole = e0 >= 0 && e1 >= 0 && e2 >= 0;
            a.triangles[3 * row] = whole ? e0 : -1;
            a.triangles[3 * row + 1] = whole ? (flip ? e2 : e1) : -1;
            a.triangles[3 * row + 2] = whole ? (flip ? e1 : e2) : -1;
        }
        ++row;
        if (nt == 2) {
            if (row < a.max_t) {
                const bool whole = e0 >= 0 && e2 >= 0 && e3 >= 0;
                a.triangles[3 * row] = whole ? e0 : -1;
                a.triangles[3 * row + 1] = whole ? (flip ? e3 : e2) : -1;
                a.triangles[3 * row + 2] = whole ? (flip ? e2 : e3) : -1;
            }
            ++row;
        }
    }
}

// ------------------------------------------------------------------------------------------------ 17c
struct CropArgs {
    double seg[21];               // per box axis: point1 [3], axis' [3], length'
    const float* vertices;
    const int32_t* triangles;
    int32_t* v_at;                // [v] 1: in use, then the exclusive scan
    int32_t* t_at;                // [t] 1: survives, then the exclusive scan
    uint8_t* keep;                // [t]
    float* out_vertices;
    int32_t* out_triangles;
    int64_t t;
    int v, max_v, max_t;
};

__device__ __forceinline__ bool point_survives(const CropArgs& a, int i) {
    const double x = (double)a.vertices[3 * (size_t)i], y = (double)a.vertices[3 * (size_t)i + 1],
                 z = (double)a.vertices[3 * (size_t)i + 2];
    return fu::inside_segment(a.seg, x, y, z) && fu::inside_segment(a.seg + 7, x, y, z) && fu::inside_segment(a.seg + 14, x, y, z);
}

__global__ void __launch_bounds__(kNT) mark_kernel(CropArgs a) {
    const int64_t i = (int64_t)blockIdx.x * kNT + threadIdx.x;
    if (i >= a.t) return;
    const int i0 = a.triangles[3 * i], i1 = a.triangles[3 * i + 1], i2 = a.triangles[3 * i + 2];
    bool keep = i0 >= 0 && i0 < a.v && i1 >= 0 && i1 < a.v && i2 >= 0 && i2 < a.v;
    keep = keep && point_survives(a, i0) && point_survives(a, i1) && point_survives(a, i2);
    a.keep[i] = keep ? 1 : 0;
    a.t_at[i] = keep ? 1 : 0;
    if (keep) {                                              // (every writer stores the same 1)
        a.v_at[i0] = 1;
        a.v_at[i1] = 1;
        a.v_at[i2] = 1;
    }
}

// in_use: the marks before the scan, kept apart as bytes by flag_kernel
__global__ void __launch_bounds__(kNT) flag_kernel(const int32_t* __restrict__ marks, uint8_t* __restrict__ flags, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * kNT + threadIdx.x;
    if (i < n) flags[i] = marks[i] != 0 ? 1 : 0;
}

__global__ void __launch_bounds__(kNT) compact_kernel(CropArgs a, const uint8_t* __restrict__ in_use, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * kNT + threadIdx.x;
    if (i >= n) return;
    if (i < a.v && in_use[i] && a.v_at[i] < a.max_v) {
        const size_t row = (size_t)a.v_at[i];
        a.out_vertices[3 * row] = a.vertices[3 * i];
        a.out_vertices[3 * row + 1] = a.vertices[3 * i + 1];
        a.out_vertices[3 * row + 2] = a.vertices[3 * i + 2];
    }
    if (i < a.t && a.keep[i] && a.t_at[i] < a.max_t) {
        const size_t row = (size_t)a.t_at[i];
        const int32_t n0 = a.v_at[a.triangles[3 * i]], n1 = a.v_at[a.triangles[3 * i + 1]], n2 = a.v_at[a.triangles[3 * i + 2]];
        const bool whole = n0 < a.max_v && n1 < a.max_v && n2 < a.max_v;
        a.out_triangles[3 * row] = whole ? n0 : -1;
        a.out_triangles[3 * row + 1] = whole ? n1 : -1;
        a.out_triangles[3 * row + 2] = whole ? n2 : -1;
    }
}

inline bool grid_ok(int nx, int ny, int nz) {
    return nx >= 1 && nx <= fu::kMaxDim && ny >= 1 && ny <= fu::kMaxDim && nz >= 1 && nz <= fu::kMaxDim;
}

inline Grid grid_of(int nx, int ny, int nz, const double* origin, double s) {
    Grid g;
    g.ox = origin[0];
    g.oy = origin[1];
    g.oz = origin[2];
    g.s = s;
    g.nx = nx;
    g.ny = ny;
    g.nz = nz;
    g.n = (int64_t)nx * ny * nz;
    return g;
}

inline size_t totals_bytes(int64_t n) { return dcn::align256(((size_t)blocks_of(n) + 1) * sizeof(int64_t)); }

}  // namespace

extern "C" int dcn_tsdf_integrate(int nx, int ny, int nz, const double* origin, double voxel_size, double trunc_margin, int f,
                                  int h, int w, const uint16_t* depth, const float* camera_to_world, double fx, double fy,
                                  double cx, double cy, double pixel_offset, int max_depth_mm, int frames_per_launch,
                                  int32_t* sum, int32_t* weight, int32_t* status, void* stream) {
    if (!grid_ok(nx, ny, nz) || !origin || !(voxel_size > 0.0) || !(trunc_margin > 0.0) || f < 1 || h < 1 || h > rs::kMaxSide ||
        w < 1 || w > rs::kMaxSide || !depth || !camera_to_world || !sum || !weight || !status || max_depth_mm < 0 ||
        max_depth_mm > 65535 || frames_per_launch == 0 || frames_per_launch > kMaxChunk ||
        !(fx == fx && fy == fy && cx == cx && cy == cy && pixel_offset == pixel_offset) || ((uintptr_t)depth & 1))
        return DCN_E_INVALID;
    const int chunk = frames_per_launch < 0 ? kDefaultChunk : frames_per_launch;
    IntegrateArgs a;
    a.g = grid_of(nx, ny, nz, origin, voxel_size);
    a.k.fx = fx;
    a.k.fy = fy;
    a.k.cx = cx;
    a.k.cy = cy;
    a.k.offset = pixel_offset;
    a.sum = sum;
    a.weight = weight;
    a.status = status;
    a.mu = trunc_margin;
    a.h = h;
    a.w = w;
    a.max_mm = max_depth_mm;
    for (int f0 = 0; f0 < f; f0 += chunk) {
        a.frames = f - f0 < chunk ? f - f0 : chunk;
        a.depth = depth + (size_t)f0 * (size_t)h * (size_t)w;
        a.poses = camera_to_world + (size_t)f0 * 16;
        hipLaunchKernelGGL(integrate_kernel, dim3(blocks_of(a.g.n)), dim3(kNT), 0, (hipStream_t)stream, a);
    }
    return dcn::check_launch();
}

// cube uint16 [n] | edges uint8 [n] | v_at int32 [n] | t_at int32 [n] | two scans' totals int64 [n / 256 + 2] each
extern "C" size_t dcn_tsdf_extract_workspace(int nx, int ny, int nz) {
    if (!grid_ok(nx, ny, nz)) return 0;
    const size_t n = (size_t)nx * ny * nz;
    return dcn::align256(n * 2) + dcn::align256(n) + 2 * dcn::align256(n * 4) + 2 * totals_bytes((int64_t)n);
}

extern "C" int dcn_tsdf_extract(int nx, int ny, int nz, const double* origin, double voxel_size, const int32_t* sum,
                                const int32_t* weight, int min_weight, int max_vertices, int max_triangles, float* vertices,
                                int32_t* triangles, int32_t* counts, void* workspace, void* stream) {
    if (!grid_ok(nx, ny, nz) || !origin || !(voxel_size > 0.0) || !sum || !weight || min_weight < 1 || max_vertices < 0 ||
        max_triangles < 0 || (max_vertices > 0 && !vertices) || (max_triangles > 0 && !triangles) || !counts || !workspace)
        return DCN_E_INVALID;
    hipStream_t st = (hipStream_t)stream;
    ExtractArgs a;
    a.g = grid_of(nx, ny, nz, origin, voxel_size);
    const size_t n = (size_t)a.g.n;
    char* p = (char*)workspace;
    a.cube = (uint16_t*)p;
    p += dcn::align256(n * 2);
    a.edges = (uint8_t*)p;
    p += dcn::align256(n);
    a.v_at = (int32_t*)p;
    p += dcn::align256(n * 4);
    a.t_at = (int32_t*)p;
    p += dcn::align256(n * 4);
    int64_t* v_totals = (int64_t*)p;
    int64_t* t_totals = (int64_t*)(p + totals_bytes(a.g.n));
    a.sum = sum;
    a.weight = weight;
    a.vertices = vertices;
    a.triangles = triangles;
    a.min_weight = min_weight;
    a.max_v = max_vertices;
    a.max_t = max_triangles;
    const unsigned nb = blocks_of(a.g.n);
    int rc = dcn::fill_bytes_async(triangles, 0xff, (size_t)max_triangles * 3 * sizeof(int32_t), st);
    if (rc != DCN_OK) return rc;
    hipLaunchKernelGGL(cube_kernel, dim3(nb), dim3(kNT), 0, st, a);
    hipLaunchKernelGGL(count_kernel, dim3(nb), dim3(kNT), 0, st, a);
    scan_in_place(a.v_at, a.g.n, v_totals, st);
    scan_in_place(a.t_at, a.g.n, t_totals, st);
    hipLaunchKernelGGL(publish_counts_kernel, dim3(1), dim3(64), 0, st, (const int64_t*)(v_totals + nb), (const int64_t*)(t_totals + nb),
                       counts);
    hipLaunchKernelGGL(vertex_kernel, dim3(nb), dim3(kNT), 0, st, a);
    hipLaunchKernelGGL(triangle_kernel, dim3(nb), dim3(kNT), 0, st, a);
    return dcn::check_launch();
}

// v_at int32 [v] | t_at int32 [t] | keep uint8 [t] | in_use uint8 [v] | two scans' totals
extern "C" size_t dcn_mesh_crop_workspace(int v, int64_t t) {
    if (v < 0 || t < 0 || t >= ((int64_t)1 << 31)) return 0;
    const size_t vv = (size_t)(v > 0 ? v : 1), tt = (size_t)(t > 0 ? t : 1);
    return dcn::align256(vv * 4) + dcn::align256(tt * 4) + dcn::align256(tt) + dcn::align256(vv) + totals_bytes(v) + totals_bytes(t);
}

extern "C" int dcn_mesh_crop(int v, int64_t t, const float* vertices, const int32_t* triangles, const double* segments,
                             int max_vertices, int max_triangles, float* out_vertices, int32_t* out_triangles, int32_t* counts,
                             void* workspace, void* stream) {
    if (v < 0 || t < 0 || t >= ((int64_t)1 << 31) || (t > 0 && (!vertices || !triangles || v < 1)) || !segments ||
        max_vertices < 0 || max_triangles < 0 || (max_vertices > 0 && !out_vertices) || (max_triangles > 0 && !out_triangles) ||
        !counts || !workspace)
        return DCN_E_INVALID;
    for (int e = 0; e < 21; ++e)
        if (!(segments[e] == segments[e])) return DCN_E_INVALID;
    hipStream_t st = (hipStream_t)stream;
    CropArgs a;
    for (int e = 0; e < 21; ++e) a.seg[e] = segments[e];
    const size_t vv = (size_t)(v > 0 ? v : 1), tt = (size_t)(t > 0 ? t : 1);
    char* p = (char*)workspace;
    a.v_at = (int32_t*)p;
    p += dcn::align256(vv * 4);
    a.t_at = (int32_t*)p;
    p += dcn::align256(tt * 4);
    a.keep = (uint8_t*)p;
    p += dcn::align256(tt);
    uint8_t* in_use = (uint8_t*)p;
    p += dcn::align256(vv);
    int64_t* v_totals = (int64_t*)p;
    int64_t* t_totals = (int64_t*)(p + totals_bytes(v));
    a.vertices = vertices;
    a.triangles = triangles;
    a.out_vertices = out_vertices;
    a.out_triangles = out_triangles;
    a.t = t;
    a.v = v;
    a.max_v = max_vertices;
    a.max_t = max_triangles;
    int rc = dcn::fill_bytes_async(out_triangles, 0xff, (size_t)max_triangles * 3 * sizeof(int32_t), st);
    if (rc == DCN_OK) rc = dcn::fill_bytes_async(a.v_at, 0, vv * 4, st);
    if (rc == DCN_OK) rc = dcn::fill_bytes_async(a.t_at, 0, tt * 4, st);
    if (rc != DCN_OK) return rc;
    if (t > 0) hipLaunchKernelGGL(mark_kernel, dim3(blocks_of(t)), dim3(kNT), 0, st, a);
    hipLaunchKernelGGL(flag_kernel, dim3(blocks_of(v)), dim3(kNT), 0, st, (const int32_t*)a.v_at, in_use, (int64_t)v);
    scan_in_place(a.v_at, v, v_totals, st);
    scan_in_place(a.t_at, t, t_totals, st);
    hipLaunchKernelGGL(publish_counts_kernel, dim3(1), dim3(64), 0, st, (const int64_t*)(v_totals + blocks_of(v)),
                       (const int64_t*)(t_totals + blocks_of(t)), counts);
    const int64_t n = (int64_t)v > t ? (int64_t)v : t;
    if (n > 0) hipLaunchKernelGGL(compact_kernel, dim3(blocks_of(n)), dim3(kNT), 0, st, a, (const uint8_t*)in_use, n);
    return dcn::check_launch();
}
