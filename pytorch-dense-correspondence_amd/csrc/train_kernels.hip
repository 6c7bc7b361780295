// The bookkeeping of the reference's training loop (dense_correspondence/training/training.py:290-456) decided on the device,
// so that a training fed from a frame store never waits for the host (include/dcn_hip.h section 13):
//   train_advance_kernel        1 work-item   reads B types, writes the 48-byte state: is the iteration empty (:304-306), the
//                                             learning-rate decay that runs after that `continue` (:544-558), Adam's step count
//                                             and bias corrections
//   adam_step_guarded_kernel    HBM-bound     dcn_adam_step's pass (28 bytes per element) + one uniform 4-byte load of
//                                             state->active per workgroup; an inactive workgroup touches nothing
//   guarded_copy_kernel         < 100 KB      the batch-norm buffers of a skipped iteration put back (108 small buffers)
//   train_log_kernel            1 workgroup   one 128-byte row of the history: reads 5 B floats and B types
#include "adam_update.h"

namespace {

typedef struct dcn_train_state TrainState;

__global__ void __launch_bounds__(64)
train_advance_kernel(TrainState* __restrict__ state, const int32_t* __restrict__ types, int B, int64_t iteration,
                     int64_t steps_between_decay, double decay, double beta1, double beta2) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    int active = 0;
    for (int p = 0; p < B; ++p) active |= (types[p] != -1);
    state->active = active;
    if (!active) {
        state->num_skipped += 1;
        return;
    }
    double lr = state->lr;
    if (iteration % steps_between_decay == 0) lr = lr * decay;
    const int64_t t = state->t + 1;
    float step_size, bc2_sqrt;
    dcn::adam_bias_corrections(lr, beta1, beta2, t, &step_size, &bc2_sqrt);
    state->lr = lr;
    state->t = t;
    state->step_size = step_size;
    state->bc2_sqrt = bc2_sqrt;
    state->num_active += 1;
}

__global__ void __launch_bounds__(256)
adam_step_guarded_kernel(dcn::AdamTable t, const TrainState* __restrict__ state) {
    if (state->active == 0) return;            // wave-uniform: the whole workgroup leaves before it touches p, g, m or v
    dcn::AdamScalars s = t.s;
    s.step_size = state->step_size;
    s.bc2_sqrt = state->bc2_sqrt;
    dcn::adam_update_chunk(t, s);
}

constexpr int kCopyBatch = 128;                // 128 x 24 bytes + header < 4 KB of kernel arguments
struct CopyTable {
    uint32_t* dst[kCopyBatch];
    const uint32_t* src[kCopyBatch];
    int words[kCopyBatch];
    int when_active;                           // < 0: unconditional
};

__global__ void __launch_bounds__(256)
guarded_copy_kernel(CopyTable t, const TrainState* state) {
    if (t.when_active >= 0 && (state->active != 0) != (t.when_active != 0)) return;
    uint32_t* __restrict__ dst = t.dst[blockIdx.x];
    const uint32_t* __restrict__ src = t.src[blockIdx.x];
    const int words = t.words[blockIdx.x];
    for (int i = (int)threadIdx.x; i < words; i += 256) dst[i] = src[i];
}

// which of the five terms (loss, match, masked, background, blind) a pair of this type composes: bit k for term k
__device__ __forceinline__ unsigned composed_terms(int type) {
    if (type == 0 || type == 3 || type == 4) return 0x1fu;   // within scene, multi object, synthetic multi object
    if (type == 1 || type == 2) return 0x11u;                // across scene, different object: the loss and the blind term
    return 0u;
}

__global__ void __launch_bounds__(64)
train_log_kernel(double* __restrict__ history, int64_t row, int64_t iteration, const TrainState* __restrict__ state,
                 const float* __restrict__ loss, const float* __restrict__ terms, const int32_t* __restrict__ types, int B) {
    double* out = history + row * DCN_TRAIN_LOG_COLUMNS;
    const int k = (int)threadIdx.x;
    if (k < 5) {                               // term k: pairs in order, in double
        double sum = 0.0;
        int count = 0;
        for (int p = 0; p < B; ++p) {
            if (composed_terms(types[p]) >> k & 1u) {
                sum += (double)terms[(size_t)p * 5 + k];
                ++count;
            }
        }
        out[5 + 2 * k] = count ? sum / (double)count : 0.0;
        out[6 + 2 * k] = (double)count;
    } else if (k == 5) {
        int valid = 0, first = -1;
        for (int p = 0; p < B; ++p) {
            const int ty = types[p];
            if (ty >= 0 && ty < DCN_LOSS_NUM_TYPES) ++valid;
            if (first < 0 && ty != -1) first = ty;
        }
        out[0] = (double)iteration;
        out[1] = (double)state->active;
        out[2] = state->lr;
        out[3] = (double)valid;
        out[4] = (double)loss[0];
        out[15] = (double)first;
    }
}

}  // namespace

extern "C" int dcn_train_advance(struct dcn_train_state* state, const int32_t* types, int B, int64_t iteration,
                                 int64_t steps_between_decay, double decay, double beta1, double beta2, void* stream) {
    if (!state || !types || B < 1 || steps_between_decay < 1 || !(decay >= 0.)) return DCN_E_INVALID;
    if (!dcn::adam_hyperparameters_valid(beta1, beta2, 0., 0.)) return DCN_E_INVALID;
    hipLaunchKernelGGL(train_advance_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, state, types, B, iteration,
                       steps_between_decay, decay, beta1, beta2);
    return dcn::check_launch();
}

extern "C" int dcn_adam_step_guarded(int n, void* const* param, const void* const* grad, void* const* exp_avg,
                                     void* const* exp_avg_sq, const int64_t* numel, double eps, double weight_decay,
                                     double beta1, double beta2, const struct dcn_train_state* state, void* stream) {
    if (n < 0 || (n > 0 && (!param || !grad || !exp_avg || !exp_avg_sq || !numel)) || !state) return DCN_E_INVALID;
    if (!dcn::adam_hyperparameters_valid(beta1, beta2, eps, weight_decay)) return DCN_E_INVALID;
    hipStream_t st = (hipStream_t)stream;
    const dcn::AdamScalars s = dcn::adam_scalars(beta1, beta2, eps, weight_decay);
    return dcn::adam_for_each_table(n, param, grad, exp_avg, exp_avg_sq, numel, s, [&](const dcn::AdamTable& t, unsigned blocks) {
        hipLaunchKernelGGL(adam_step_guarded_kernel, dim3(blocks), dim3(256), 0, st, t, state);
    });
}

extern "C" int dcn_guarded_copy(int n, void* const* dst, const void* const* src, const int64_t* bytes,
                                const struct dcn_train_state* state, int when_active, void* stream) {
    if (n < 0 || (n > 0 && (!dst || !src || !bytes))) return DCN_E_INVALID;
    for (int i = 0; i < n; ++i) {              // every entry is checked before anything is launched
        if (bytes[i] < 0 || bytes[i] % 4 != 0) return DCN_E_INVALID;
        if (bytes[i] > 0x7fffffff) return DCN_E_UNSUPPORTED;
        if (bytes[i] > 0 && (!dst[i] || !src[i] || (((uintptr_t)dst[i] | (uintptr_t)src[i]) & 3))) return DCN_E_INVALID;
    }
    hipStream_t st = (hipStream_t)stream;
    for (int base = 0; base < n; base += kCopyBatch) {
        CopyTable t;
        t.when_active = state ? (when_active != 0) : -1;
        int m = 0;
        for (int i = base; i < n && i < base + kCopyBatch; ++i) {
            if (bytes[i] == 0) continue;
            t.dst[m] = (uint32_t*)dst[i];
            t.src[m] = (const uint32_t*)src[i];
            t.words[m] = (int)(bytes[i] / 4);
            ++m;
        }
        if (m == 0) continue;
        hipLaunchKernelGGL(guarded_copy_kernel, dim3((unsigned)m), dim3(256), 0, st, t, state);
        if (int rc = dcn::check_launch()) return rc;
    }
    return DCN_OK;
}

extern "C" int dcn_train_log(double* history, int64_t row, int64_t iteration, const struct dcn_train_state* state,
                             const float* loss, const float* terms, const int32_t* types, int B, void* stream) {
    if (!history || !state || !loss || !terms || !types || B < 1 || row < 0) return DCN_E_INVALID;
    hipLaunchKernelGGL(train_log_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, history, row, iteration, state, loss, terms,
                       types, B);
    return dcn::check_launch();
}
