// The occlusion rule of the synthetic multi-object merge (correspondence_augmentation.py prune_matches_if_occluded, :300-335,
// as spartan_dataset_masked.py:929-955 applies it to frame 1's pair and to frame 2's swapped pair), shared by the prune of
// given match lists (merge_kernels.hip) and the fused sample builder (synthetic_kernels.hip).
#pragma once
#include "dcn_common.h"

namespace dcn {

// In frame f (0 / 1) of sample s the OTHER object lies in front of object o (0 = a, 1 = b): foreground [n][2] records
__device__ __forceinline__ bool other_in_front(const int32_t* fg, int s, int f, int o) {
    return (fg[2 * s + f] == DCN_MERGE_FG_B) == (o == 0);
}

// An entry of object o at flat pixel `px` of frame f is dropped when the other object is in front there and covers the pixel:
// `other_mask` is the other object's 0/1 mask of that frame and sample
__device__ __forceinline__ bool occluded(const int32_t* fg, int s, int f, int o, const unsigned char* other_mask, int64_t px) {
    return other_in_front(fg, s, f, o) && other_mask[px] != 0;
}

}  // namespace dcn
