// The network-input side shared by the image kernels (augment_kernels.hip, merge_kernels.hip): torch's ToTensor + Normalize
// (spartan_dataset_masked.py:297-304 of the reference) as a per-workgroup (c, x) -> (x / 255 - mean_c) / std_c table, and the
// store path of an output pixel -- float NCHW network input, uint8 HWC RGB and float mask, each optional.
#pragma once
#include "dcn_common.h"

#pragma clang fp contract(off)   // (the build passes -ffp-contract=off as well)

namespace dcn {

// (c, x) -> (x / 255 - mean_c) / std_c, one IEEE operation at a time (bitwise torch's result).  Ends with a barrier.
template <int kThreads>
__device__ __forceinline__ void build_norm_table(float (*lut)[256], const float mean[3], const float std[3]) {
    for (int k = threadIdx.x; k < 768; k += kThreads) {
        const int c = k >> 8;
        lut[c][k & 255] = ((float)(k & 255) / 255.0f - mean[c]) / std[c];
    }
    __syncthreads();
}

// One output pixel p of an image of hw pixels: px = its RGB bytes, m = its mask value.
__device__ __forceinline__ void store_pixel(const float (*lut)[256], int64_t p, int64_t hw, const uint32_t px[3], float m,
                                            float* net, unsigned char* rgb_out, float* mask_out) {
    for (int c = 0; c < 3; ++c) {
        if (rgb_out) rgb_out[p * 3 + c] = (unsigned char)px[c];
        if (net) net[(size_t)c * hw + p] = lut[c][px[c]];
    }
    if (mask_out) mask_out[p] = m;
}

// Four output pixels op .. op + 3 of one row (op % 4 == 0; net / mask_out 16-byte and rgb_out 4-byte aligned): px[j] = pixel
// j's RGB bytes, m[j] its mask value.  Three 4-byte RGB stores, one 16-byte store per network-input plane and for the mask.
__device__ __forceinline__ void store_pixels4(const float (*lut)[256], int64_t op, int64_t hw, const uint32_t px[4][3],
                                              const float m[4], float* net, unsigned char* rgb_out, float* mask_out) {
    if (rgb_out) {
        uint32_t o[3] = {0u, 0u, 0u};
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int c = 0; c < 3; ++c) o[(3 * j + c) >> 2] |= px[j][c] << (8 * ((3 * j + c) & 3));
        uint32_t* d = reinterpret_cast<uint32_t*>(rgb_out + op * 3);
        d[0] = o[0];
        d[1] = o[1];
        d[2] = o[2];
    }
    if (net) {
#pragma unroll
        for (int c = 0; c < 3; ++c)
            *reinterpret_cast<float4*>(net + (size_t)c * hw + op) =
                make_float4(lut[c][px[0][c]], lut[c][px[1][c]], lut[c][px[2][c]], lut[c][px[3][c]]);
    }
    if (mask_out) *reinterpret_cast<float4*>(mask_out + op) = make_float4(m[0], m[1], m[2], m[3]);
}

}  // namespace dcn
