// The row lists of the batched evaluation kernels (evaluate_kernels.hip, acrossobj_kernels.hip, crossscene_kernels.hip,
// picture_kernels.hip): pair p's rows are [offsets[p], offsets[p + 1]) of the row arrays, the offsets live on the device and are
// checked there.  pair_rows: from a pair to its rows; row_owner / row_in_pair: from a row to its pair.
#pragma once
#include "dcn_common.h"

namespace dcn {

// offsets must increase from >= 0 to <= max_rows over ALL pairs (no pair's rows may overlap another's): one violation
// anywhere raises DCN_EVAL_BAD_OFFSETS and sets *flag, and then every pair is empty.
static __global__ void __launch_bounds__(256) check_offsets_kernel(const int64_t* __restrict__ offsets, int np,
                                                                   int64_t max_rows, int32_t* flag, int32_t* status) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= np) return;
    const int64_t lo = offsets[p], hi = offsets[p + 1];
    if (lo < 0 || hi < lo || hi > max_rows) {
        atomicOr(flag, 1);
        atomicOr(status, DCN_EVAL_BAD_OFFSETS);
    }
}

// Rows [lo, lo + n) of pair p; none when the offsets failed check_offsets_kernel; a list longer than max_pair_rows is cut
// (DCN_EVAL_BAD_OFFSETS)
__device__ __forceinline__ void pair_rows(const int64_t* offsets, const int32_t* offsets_bad, int p, int64_t max_rows,
                                          int max_pair_rows, int64_t& lo, int& n, int& bad) {
    lo = offsets[p];
    int64_t hi = offsets[p + 1];
    if (*offsets_bad || lo < 0 || hi < lo || hi > max_rows) {
        bad |= DCN_EVAL_BAD_OFFSETS;
        lo = 0;
        hi = 0;
    }
    if (hi - lo > max_pair_rows) {
        bad |= DCN_EVAL_BAD_OFFSETS;
        hi = lo + max_pair_rows;
    }
    n = (int)(hi - lo);
}

// The pair whose list holds row r: the first p with offsets[p + 1] > r; np when r lies past the last list
__device__ __forceinline__ int row_owner(const int64_t* offsets, int np, int64_t r) {
    int lo = 0, hi = np;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (offsets[mid + 1] > r) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

// Whether row r is one of the rows pair_rows gives pair p = row_owner(r): not past the last list, nor cut off a bad or long one
__device__ __forceinline__ bool row_in_pair(const int64_t* offsets, const int32_t* offsets_bad, int p, int np, int64_t r,
                                            int64_t max_rows, int max_pair_rows) {
    int bad = 0, n = 0;
    int64_t first = 0;
    if (p < np) pair_rows(offsets, offsets_bad, p, max_rows, max_pair_rows, first, n, bad);
    return p < np && r >= first && r < first + n;
}

}  // namespace dcn
