// Columns of an evaluation table reduced to the reference's curves on the device (include/dcn_hip.h section 14):
// DenseCorrespondenceEvaluationPlotter.make_cdf_plot and compute_area_above_curve
// (dense_correspondence/evaluation/evaluation.py:2658-2674, :2844-2863), that is scipy.stats.cumfreq(data, num_bins) with
// defaultreallimits=None -- numpy.histogram over np.linspace edges -- times 1 / len(data), and binsize * sum(1 - cdf).
//   eval_curves_kernel   one workgroup of 1024 per curve; 16 KB of LDS for the bin counters
//     pass 1  rows in a strided loop: count, NaNs dropped, min, max, flags (wavefront butterfly, then LDS)
//     pass 2  the same rows again: bin index as numpy computes it, INTEGER LDS atomics (the counts do not depend on the order)
//     pass 3  wavefront 0 scans the counters 64 at a time, writes cumcount and cdf and adds the area's terms in a fixed order
// Every product and sum below is rounded on its own, as numpy rounds them: an fma in i * step + first or around x - first
// moves an edge by an ulp and a value sitting on it into the neighbouring bin.
#pragma clang fp contract(off)
#include "dcn_common.h"

namespace {

constexpr int kCurveThreads = 1024;
constexpr int kCurveWaves = kCurveThreads / dcn::kWave;
constexpr int kCurveMaxBins = 4096;
constexpr int kCurveUnroll = 4;                // rows a work-item has in flight

struct CurveEdges {                            // np.linspace(first, last, num_bins + 1)
    double first, last, delta, step;
    int num_bins;
};

__device__ __forceinline__ double curve_edge(const CurveEdges& e, int i) {
    if (i >= e.num_bins) return e.last;        // y[-1] = stop
    double y;
    if (e.step == 0.0) {                       // numpy's path for a denormal delta: y / div * delta
        y = (double)i / (double)e.num_bins;
        y = y * e.delta;
    } else {
        y = (double)i * e.step;
    }
    return y + e.first;
}

__device__ __forceinline__ bool curve_finite(double x) { return x - x == 0.0; }

// numpy.histogram's uniform-bin index (numpy/lib/_histograms_impl.py): the estimate by division, corrected against the edges
__device__ __forceinline__ int curve_bin(const CurveEdges& e, double x) {
    const int nb = e.num_bins;
    double f = (x - e.first) / e.delta;
    f = f * (double)nb;
    int idx = f >= (double)nb ? nb - 1 : (f > 0.0 ? (int)f : 0);
    if (x < curve_edge(e, idx)) idx -= 1;
    if (idx < 0) idx = 0;                      // (x >= first: not reached; keeps the LDS index in range whatever comes in)
    if (idx != nb - 1 && x >= curve_edge(e, idx + 1)) idx += 1;
    return idx;
}

__global__ void __launch_bounds__(kCurveThreads)
eval_curves_kernel(int64_t rows, int64_t ld, const double* __restrict__ values, const int32_t* __restrict__ row_pair,
                   const uint8_t* __restrict__ drop_nan, int num_bins, int64_t* __restrict__ cumcount, double* __restrict__ cdf,
                   double* __restrict__ summary, int32_t* __restrict__ status) {
    __shared__ int hist[kCurveMaxBins];
    __shared__ long long s_n[kCurveWaves], s_dropped[kCurveWaves];
    __shared__ double s_mn[kCurveWaves], s_mx[kCurveWaves];
    __shared__ int s_flags[kCurveWaves];
    const int k = (int)blockIdx.x, tid = (int)threadIdx.x, lane = tid & (dcn::kWave - 1), wave = tid / dcn::kWave;
    const double* __restrict__ v = values + (size_t)k * (size_t)ld;
    const bool drop = drop_nan[k] != 0;
    const double inf = __builtin_huge_val();
    const int64_t stride = (int64_t)kCurveThreads * kCurveUnroll;

    // ---- pass 1
    long long n = 0, dropped = 0;
    double mn = inf, mx = -inf;
    int flags = 0;
    for (int64_t r0 = tid; r0 < rows; r0 += stride) {
        double x[kCurveUnroll];
        bool in[kCurveUnroll];
#pragma unroll
        for (int j = 0; j < kCurveUnroll; ++j) {
            const int64_t r = r0 + (int64_t)j * kCurveThreads;
            in[j] = r < rows && (row_pair == nullptr || row_pair[r] >= 0);
            x[j] = in[j] ? v[r] : 0.0;
        }
#pragma unroll
        for (int j = 0; j < kCurveUnroll; ++j) {
            if (!in[j]) continue;
            if (x[j] != x[j]) {
                if (drop) ++dropped;
                else flags |= DCN_CURVE_NAN;
                continue;
            }
            if (x[j] == inf || x[j] == -inf) flags |= DCN_CURVE_NONFINITE;
            ++n;
            mn = x[j] < mn ? x[j] : mn;
            mx = x[j] > mx ? x[j] : mx;
        }
    }
#pragma unroll
    for (int off = dcn::kWave / 2; off > 0; off >>= 1) {
        n += __shfl_xor(n, off, dcn::kWave);
        dropped += __shfl_xor(dropped, off, dcn::kWave);
        const double a = __shfl_xor(mn, off, dcn::kWave), b = __shfl_xor(mx, off, dcn::kWave);
        mn = a < mn ? a : mn;
        mx = b > mx ? b : mx;
        flags |= __shfl_xor(flags, off, dcn::kWave);
    }
    if (lane == 0) {
        s_n[wave] = n;
        s_dropped[wave] = dropped;
        s_mn[wave] = mn;
        s_mx[wave] = mx;
        s_flags[wave] = flags;
    }
    for (int i = tid; i < num_bins; i += kCurveThreads) hist[i] = 0;
    __syncthreads();
    n = 0, dropped = 0, mn = inf, mx = -inf, flags = 0;
    for (int w = 0; w < kCurveWaves; ++w) {    // every work-item folds the 16 partials in the same order
        n += s_n[w];
        dropped += s_dropped[w];
        mn = s_mn[w] < mn ? s_mn[w] : mn;
        mx = s_mx[w] > mx ? s_mx[w] : mx;
        flags |= s_flags[w];
    }

    // ---- the range: scipy's _histogram, then numpy's _get_outer_edges
    const double nan = inf - inf;
    double lowerlimit = nan, binsize = nan;
    CurveEdges e;
    e.num_bins = num_bins;
    e.first = e.last = e.delta = e.step = nan;
    if (flags == 0 && n == 0) flags = DCN_CURVE_EMPTY;
    if (flags == 0) {
        const double s = (mx - mn) / (2. * ((double)num_bins - 1.));
        lowerlimit = mn - s;
        const double upper = mx + s;
        e.first = lowerlimit;
        e.last = upper;
        if (e.first == e.last) {
            e.first = e.first - 0.5;
            e.last = e.last + 0.5;
        }
        e.delta = e.last - e.first;
        e.step = e.delta / (double)num_bins;
        // finite values whose range is not (mx - mn overflows): numpy refuses [-inf, inf] in the same words
        if (!curve_finite(lowerlimit) || !curve_finite(upper) || !curve_finite(e.delta) || !(e.delta > 0.0))
            flags = DCN_CURVE_NONFINITE;
        binsize = curve_edge(e, 1) - curve_edge(e, 0);
    }
    int64_t* __restrict__ cc = cumcount + (size_t)k * (size_t)num_bins;
    double* __restrict__ cd = cdf + (size_t)k * (size_t)num_bins;
    double* __restrict__ out = summary + (size_t)k * DCN_CURVE_SUMMARY_DOUBLES;
    if (flags != 0) {                          // uniform over the workgroup
        for (int i = tid; i < num_bins; i += kCurveThreads) {
            cc[i] = 0;
            cd[i] = nan;
        }
        if (tid == 0) {
            const bool known = (flags & DCN_CURVE_NAN) == 0 && n > 0;   // numpy's min and max of data with a NaN are NaN
            out[0] = (double)n;
            out[1] = (double)dropped;
            out[2] = known ? mn : nan;
            out[3] = known ? mx : nan;
            out[4] = nan;
            out[5] = nan;
            out[6] = nan;
            out[7] = (double)flags;
            atomicOr(status, flags);
        }
        return;
    }

    // ---- pass 2
    for (int64_t r0 = tid; r0 < rows; r0 += stride) {
        double x[kCurveUnroll];
        bool in[kCurveUnroll];
#pragma unroll
        for (int j = 0; j < kCurveUnroll; ++j) {
            const int64_t r = r0 + (int64_t)j * kCurveThreads;
            in[j] = r < rows && (row_pair == nullptr || row_pair[r] >= 0);
            x[j] = in[j] ? v[r] : nan;
        }
#pragma unroll
        for (int j = 0; j < kCurveUnroll; ++j)
            if (in[j] && x[j] == x[j]) atomicAdd(&hist[curve_bin(e, x[j])], 1);
    }
    __syncthreads();

    // ---- pass 3
    if (wave != 0) return;
    const double inv = 1.0 / (double)n;        // cumhist *= 1.0 / len(data)
    long long carry = 0;
    double above = 0.0;
    for (int base = 0; base < num_bins; base += dcn::kWave) {
        const int i = base + lane;
        long long c = i < num_bins ? (long long)hist[i] : 0;
#pragma unroll
        for (int d = 1; d < dcn::kWave; d <<= 1) {
            const long long o = __shfl(c, lane >= d ? lane - d : lane, dcn::kWave);
            if (lane >= d) c += o;
        }
        c += carry;
        double term = 0.0;
        if (i < num_bins) {
            const double f = (double)c * inv;
            cc[i] = (int64_t)c;
            cd[i] = f;
            term = 1.0 - f;
        }
#pragma unroll
        for (int off = dcn::kWave / 2; off > 0; off >>= 1) term += __shfl_xor(term, off, dcn::kWave);
        above += term;                         // 64 bins as a butterfly, the groups of 64 in order: one fixed order
        carry = __shfl(c, dcn::kWave - 1, dcn::kWave);
    }
    if (lane == 0) {
        out[0] = (double)n;
        out[1] = (double)dropped;
        out[2] = mn;
        out[3] = mx;
        out[4] = lowerlimit;
        out[5] = binsize;
        out[6] = binsize * above;
        out[7] = 0.0;
    }
}

}  // namespace

extern "C" int dcn_eval_curves(int c, int64_t rows, int64_t ld, const double* values, const int32_t* row_pair,
                               const uint8_t* drop_nan, int num_bins, int64_t* cumcount, double* cdf, double* summary,
                               int32_t* status, void* stream) {
    if (c < 1 || c > 64 || num_bins < 2 || num_bins > kCurveMaxBins || rows < 0 || ld < rows) return DCN_E_INVALID;
    if (!drop_nan || !cumcount || !cdf || !summary || !status || (rows > 0 && !values)) return DCN_E_INVALID;
    hipStream_t st = (hipStream_t)stream;
    if (int rc = dcn::fill_bytes_async(status, 0, sizeof(int32_t), st)) return rc;
    hipLaunchKernelGGL(eval_curves_kernel, dim3((unsigned)c), dim3(kCurveThreads), 0, st, rows, ld, values, row_pair, drop_nan,
                       num_bins, cumcount, cdf, summary, status);
    return dcn::check_launch();
}
