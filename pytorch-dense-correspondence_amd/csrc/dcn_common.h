// Shared device helpers for the gfx950 kernels (wave64 reductions, launch checking).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dcn_hip.h"

// Counted waits of the LDS-DMA pipelines (conv_hl_kernels.hip): inline asm, so that the counts stay exactly where they are
// written (the compiler's own s_waitcnt insertion does not see them).  The test-only host emulation (tests/hostemu) defines
// its own versions before this header is read.
#ifndef DCN_WAIT_VMCNT
#define DCN_WAIT_VMCNT(n) asm volatile("s_waitcnt vmcnt(" #n ")" ::: "memory")
#define DCN_WAIT_LGKMCNT0() asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory")
#define DCN_OPAQUE_INT(v) asm volatile("" : "+v"(v))   // the optimiser forgets what it knew about v (no loop-invariant hoisting)
#endif

// Register cap of a kernel (the allocator's budget, in VGPRs per lane).  Empty in the host emulation, which compiles the
// same sources for the CPU.
#if defined(DCN_HOSTEMU_BUILD)
#define DCN_MAX_VGPRS(n)
#else
#define DCN_MAX_VGPRS(n) __attribute__((amdgpu_num_vgpr(n)))
#endif

// The optimiser forgets what it knew about a UNIFORM integer (kept in a scalar register): nothing computed from it is hoisted
// out of a loop into registers that then stay occupied across it.
#if defined(DCN_HOSTEMU_BUILD)
#define DCN_OPAQUE_UNIFORM(v) ((void)(v))
#else
#define DCN_OPAQUE_UNIFORM(v) asm volatile("" : "+s"(v))
#endif

// Nothing is scheduled across this point: neither by the instruction scheduler nor (memory accesses) by the passes in front of it.
#define DCN_SCHED_FENCE() do { asm volatile("" ::: "memory"); __builtin_amdgcn_sched_barrier(0); } while (0)

namespace dcn {

constexpr int kWave = 64;  // CDNA wavefront

template <class T> __device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) v += __shfl_down(v, off, kWave);
    return v;  // valid in lane 0
}

// Sum over a workgroup of NT threads (NT multiple of 64).  Result valid in thread 0.  `scratch` holds NT/64 values.
template <int NT, class T> __device__ __forceinline__ T block_sum(T v, T* scratch) {
    v = wave_sum(v);
    const int lane = threadIdx.x & (kWave - 1), wv = threadIdx.x / kWave;
    __syncthreads();  // scratch may still be read from a previous reduction
    if (lane == 0) scratch[wv] = v;
    __syncthreads();
    T r = scratch[0];
    if (threadIdx.x == 0) {
#pragma unroll
        for (int i = 1; i < NT / kWave; ++i) r += scratch[i];
    }
    return r;
}

// Stream-ordered fill of n bytes (n % 4 == 0) with a byte value, as a KERNEL: unlike hipMemsetAsync it is an ordinary
// kernel node when the caller's stream is being captured into a hipGraph.
static __global__ void __launch_bounds__(256) fill_words_kernel(unsigned* __restrict__ p, unsigned v, size_t words) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < words; i += (size_t)gridDim.x * 256) p[i] = v;
}
inline int fill_bytes_async(void* p, int byte_value, size_t n, hipStream_t st) {
    if (n == 0) return DCN_OK;
    if (n % 4) return DCN_E_INVALID;
    const unsigned b = (unsigned)byte_value & 0xffu, v = b | (b << 8) | (b << 16) | (b << 24);
    const size_t words = n / 4;
    size_t blocks = (words + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(fill_words_kernel, dim3((unsigned)blocks), dim3(256), 0, st, (unsigned*)p, v, words);
    return hipGetLastError() == hipSuccess ? DCN_OK : DCN_E_LAUNCH;
}

inline int check_launch() { return hipGetLastError() == hipSuccess ? DCN_OK : DCN_E_LAUNCH; }

__host__ __device__ inline int64_t ceil_div64(int64_t a, int64_t b) { return (a + b - 1) / b; }
__host__ __device__ inline int ceil_div(int a, int b) { return (a + b - 1) / b; }

inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }   // (the parts of a carved workspace start 256-aligned)

}  // namespace dcn

// Launches the instance of the kernel template K<int DT> for descriptor dimension d: the dimensions that have an instance of
// their own, every other one by the generic K<0>, which reads D at run time.
#define DCN_LAUNCH_FOR_D(d, K, grid, block, st, ...)                                       \
    switch (d) {                                                                           \
        case 3: hipLaunchKernelGGL((K<3>), grid, block, 0, st, __VA_ARGS__); break;        \
        case 4: hipLaunchKernelGGL((K<4>), grid, block, 0, st, __VA_ARGS__); break;        \
        case 8: hipLaunchKernelGGL((K<8>), grid, block, 0, st, __VA_ARGS__); break;        \
        case 16: hipLaunchKernelGGL((K<16>), grid, block, 0, st, __VA_ARGS__); break;      \
        case 32: hipLaunchKernelGGL((K<32>), grid, block, 0, st, __VA_ARGS__); break;      \
        default: hipLaunchKernelGGL((K<0>), grid, block, 0, st, __VA_ARGS__); break;       \
    }
