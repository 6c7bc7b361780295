// The arithmetic of TSDF fusion, surface extraction and the box crop (include/dcn_hip.h section 17), stated once for the kernels
// of fusion_kernels.hip.  tests/fusion_common.py states the same rules in numpy, from the header's text and not from this file.
//
// As in render_raster.h every float64 step is ONE correctly rounded IEEE operation (mul / add / quot of that file: the compiler
// may not contract them) and every other step is integer.  The pose convention, the rigid inverse and the camera-frame point are
// rules 16(a) and 16(b): camera_from_pose and camera_coord of render_raster.h, used as they are.
#pragma once
#include <math.h>

#include "dcn_common.h"
#include "render_raster.h"

namespace dcn {
namespace fusion {

namespace rs = dcn::raster;

constexpr int kMaxDim = 1024;                     // voxels per axis at most
constexpr int kMaxWeight = 65535;                 // a voxel with this weight takes no further frame
constexpr double kQuantum = 32768.0;              // q = rint(t * 2^15): |sum| <= 65535 * 2^15 < 2^31

struct Pinhole {
    double fx, fy, cx, cy, offset;
};

// 17a, step 1: the world coordinate of voxel index i on an axis
__device__ __forceinline__ double voxel_centre(double origin, double s, int i) { return rs::add(origin, rs::mul(s, (double)i)); }

// 17a, steps 2-4 for one world point and one frame (also 18a, steps 1-3): its camera-frame depth z and the pixel that holds its
// projection, pixel = py * w + px; false when the frame does not see the point.  cam: the 12 entries of 16(a).
__device__ __forceinline__ bool project(const double* cam, const Pinhole& k, double wx, double wy, double wz, int h, int w,
                                        double& z, int& pixel) {
    z = rs::camera_coord(cam + 8, wx, wy, wz);
    if (!(z > 0.0)) return false;                                          // (NaN: skipped)
    const double x = rs::camera_coord(cam, wx, wy, wz), y = rs::camera_coord(cam + 4, wx, wy, wz);
    const double pu = floor(rs::add(rs::add(rs::quot(rs::mul(k.fx, x), z), k.cx), k.offset));
    const double pv = floor(rs::add(rs::add(rs::quot(rs::mul(k.fy, y), z), k.cy), k.offset));
    if (!(pu >= 0.0 && pu < (double)w && pv >= 0.0 && pv < (double)h)) return false;   // (NaN, infinity: skipped)
    pixel = (int)pv * w + (int)pu;                                         // (h, w <= 16384: below 2^28)
    return true;
}

// 17a, steps 2-8 for one voxel centre and one frame: does the frame reach the voxel, and with which q.  depth: the frame's image.
__device__ __forceinline__ bool observe(const double* cam, const Pinhole& k, double wx, double wy, double wz,
                                        const uint16_t* __restrict__ depth, int h, int w, int max_mm, double mu, int& q) {
    double z;
    int pixel;
    if (!project(cam, k, wx, wy, wz, h, w, z, pixel)) return false;
    const int mm = depth[pixel];
    if (mm == 0 || mm > max_mm) return false;
    const double diff = rs::add(rs::quot((double)mm, 1000.0), -z);         // (a + (-b) is a - b, one rounding)
    if (!(diff > -mu)) return false;
    const double t = rs::quot(diff, mu);
    q = (int)rint(rs::mul(t < 1.0 ? t : 1.0, kQuantum));                   // ties to even
    return true;
}

// ---- 17b.  Corner c of a cube is at (bit 0, bit 1, bit 2) of c along (x, y, z).  The six tetrahedra of the Kuhn split, in the
// lexicographic order of the axis permutations (a, b, c): vertices corner 0, e_a, e_a + e_b, corner 7; three bits per vertex.
// A tetrahedron of an odd permutation is the mirror image of one of an even permutation.
static __device__ const unsigned kTetCorners[6] = {0u | 1u << 3 | 3u << 6 | 7u << 9, 0u | 1u << 3 | 5u << 6 | 7u << 9,
                                                   0u | 2u << 3 | 3u << 6 | 7u << 9, 0u | 2u << 3 | 6u << 6 | 7u << 9,
                                                   0u | 4u << 3 | 5u << 6 | 7u << 9, 0u | 4u << 3 | 6u << 6 | 7u << 9};
__device__ __forceinline__ unsigned tet_corner(int tet, int k) { return (kTetCorners[tet] >> (3 * k)) & 7u; }
constexpr unsigned kOddTets = 0x26u;              // bit tet: (x, z, y), (y, x, z), (z, y, x)

// The 16 cases by the inside bits of the tetrahedron's four vertices: bits 0-15 four crossed edges (p | q << 2 each, p inside,
// q outside), bits 16-17 the number of triangles, bit 18: exchange the last two vertices of each triangle in a tetrahedron of
// an EVEN permutation (in an odd one exactly when the bit is clear), so that the normal points to the outside.  One triangle:
// edges 0, 1, 2.  Two: (0, 1, 2) and (0, 2, 3).  tests/fusion_common.py derives the same table from the rule.
static __device__ const unsigned kTetCases[16] = {0x00000u, 0x10c84u, 0x50d91u, 0x29dc8u, 0x10e62u, 0x66ec4u, 0x22ed1u, 0x10edcu,
                                                  0x50b73u, 0x27b84u, 0x63b91u, 0x50b98u, 0x23762u, 0x10764u, 0x50321u, 0x00000u};

// direction id (x, y, z, xy, xz, yz, xyz = 0 .. 6) of an edge whose ends differ in the corner bits b (1 .. 7)
__device__ __forceinline__ int direction_id(unsigned b) { return (int)((0x65423100u >> (4 * b)) & 7u); }
__device__ __forceinline__ unsigned direction_bits(int d) { return (0x7653421u >> (4 * d)) & 7u; }

// The vertex of a crossed edge from voxel A = (ia, ja, ka) along direction bits b: sums and weights of both ends
__device__ __forceinline__ void edge_vertex(int ia, int ja, int ka, unsigned b, int sum_a, int weight_a, int sum_b, int weight_b,
                                            double ox, double oy, double oz, double s, float* out) {
    const double fa = rs::quot((double)sum_a, (double)weight_a), fb = rs::quot((double)sum_b, (double)weight_b);
    const double t = rs::quot(fa, rs::add(fa, -fb));
    const double gx = (b & 1u) ? rs::add((double)ia, t) : (double)ia;
    const double gy = (b & 2u) ? rs::add((double)ja, t) : (double)ja;
    const double gz = (b & 4u) ? rs::add((double)ka, t) : (double)ka;
    out[0] = (float)rs::add(ox, rs::mul(s, gx));
    out[1] = (float)rs::add(oy, rs::mul(s, gy));
    out[2] = (float)rs::add(oz, rs::mul(s, gz));
}

// ---- 17c.  seg: per box axis point1 [3], axis' [3], length' (7 doubles).  Does the point survive the axis?
__device__ __forceinline__ bool inside_segment(const double* seg, double x, double y, double z) {
    const double d0 = rs::add(x, -seg[0]), d1 = rs::add(y, -seg[1]), d2 = rs::add(z, -seg[2]);
    const double sc = rs::add(rs::add(rs::mul(d0, seg[3]), rs::mul(d1, seg[4])), rs::mul(d2, seg[5]));
    return sc >= 0.0 && sc <= seg[6];
}

}  // namespace fusion
}  // namespace dcn
