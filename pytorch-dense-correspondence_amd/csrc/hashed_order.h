// The counter-based hash behind the device-side random numbers (sample_kernels.hip) and the hashed-key order that stands in
// for random.sample: element i of a population gets the key order_key(seed, i); ordered by (key, i) the population is in a
// uniform random order, and its first k entries are a sample without replacement (sample_kernels.hip eval_select_kernel,
// acrossobj_kernels.hip).
#pragma once
#include <stdint.h>

namespace dcn {

__device__ __forceinline__ uint32_t mix32(uint32_t x) {
    x ^= x >> 16;
    x *= 0x7feb352dU;
    x ^= x >> 15;
    x *= 0x846ca68bU;
    x ^= x >> 16;
    return x;
}

__device__ __forceinline__ uint32_t order_key(uint64_t s, uint32_t i) {
    const uint32_t k0 = mix32((uint32_t)s ^ 0x2545F491U);
    return mix32(mix32(i ^ k0) ^ (mix32((uint32_t)(s >> 32) ^ k0) + 0x9E3779B9U));
}

}  // namespace dcn
