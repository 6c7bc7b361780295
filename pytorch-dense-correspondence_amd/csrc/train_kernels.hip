// The bookkeeping of the reference's training loop (dense_correspondence/training/training.py:290-456) decided on the device,
// so that a training fed from a frame store never waits for the host (include/dcn_hip.h section 13):
//   train_advance_kernel        1 work-item   reads B types, writes the 48-byte state: is the iteration empty (:304-306), the
//                                             learning-rate decay that runs after that `continue` (:544-558), Adam's step count
//                                             and bias corrections
//   adam_step_guarded_kernel    HBM-bound     dcn_adam_step's pass (28 bytes per element) + one uniform 4-byte load of
//                                             state->active per workgroup; an inactive workgroup touches nothing
//   guarded_copy_kernel         < 100 KB      the batch-norm buffers of a skipped iteration put back (108 small buffers)
//   train_log_kernel            1 workgroup   one 128-byte row of the history: reads 5 B floats and B types
// and, for G data-parallel ranks that have gathered their types and their log rows in rank order (section 13e, 13f), the same
// rules over the G B pairs of the global batch, so that every rank takes the same decision and writes the same row:
//   train_advance_ranks_kernel  1 work-item   reads G B types; the state transition above and this rank's share n_rank / N
//   train_log_ranks_kernel      1 workgroup   reads G (1 + 5 B) floats and G B types
#include "adam_update.h"

namespace {

typedef struct dcn_train_state TrainState;

// the state transition of one iteration (13a), by the one work-item that owns the state
__device__ __forceinline__ void advance_state(TrainState* __restrict__ state, int active, int64_t iteration,
                                              int64_t steps_between_decay, double decay, double beta1, double beta2) {
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

// pairs that are not empty among n types
__device__ __forceinline__ int count_non_empty(const int32_t* __restrict__ types, int n) {
    int count = 0;
    for (int p = 0; p < n; ++p) count += (types[p] != -1);
    return count;
}

__global__ void __launch_bounds__(64)
train_advance_kernel(TrainState* __restrict__ state, const int32_t* __restrict__ types, int B, int64_t iteration,
                     int64_t steps_between_decay, double decay, double beta1, double beta2) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    advance_state(state, count_non_empty(types, B) > 0, iteration, steps_between_decay, decay, beta1, beta2);
}

__global__ void __launch_bounds__(64)
train_advance_ranks_kernel(TrainState* __restrict__ state, const int32_t* __restrict__ types_all, int G, int B, int rank,
                           float* __restrict__ weight_out, int64_t iteration, int64_t steps_between_decay, double decay,
                           double beta1, double beta2) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    int64_t total = 0;
    int mine = 0;
    for (int r = 0; r < G; ++r) {
        const int n = count_non_empty(types_all + (size_t)r * B, B);
        total += n;
        if (r == rank) mine = n;
    }
    advance_state(state, total > 0, iteration, steps_between_decay, decay, beta1, beta2);
    weight_out[0] = total > 0 ? (float)((double)mine / (double)total) : 0.0f;      // rounded once
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

// One history row (13d) by work-items 0 .. 5 of a workgroup, over G groups of B pairs in (group, pair) order: the terms of pair
// (r, p) are the five floats at terms + r * group_stride + 5 p, its type is types[r * B + p]; column 4 is the caller's.
__device__ __forceinline__ void log_row(double* __restrict__ out, int k, int64_t iteration, const TrainState* __restrict__ state,
                                        const float* __restrict__ terms, size_t group_stride, const int32_t* __restrict__ types,
                                        int G, int B, double loss) {
    if (k < 5) {                               // term k: pairs in order, in double
        double sum = 0.0;
        int count = 0;
        for (int r = 0; r < G; ++r) {
            for (int p = 0; p < B; ++p) {
                if (composed_terms(types[(size_t)r * B + p]) >> k & 1u) {
                    sum += (double)terms[r * group_stride + (size_t)p * 5 + k];
                    ++count;
                }
            }
        }
        out[5 + 2 * k] = count ? sum / (double)count : 0.0;
        out[6 + 2 * k] = (double)count;
    } else if (k == 5) {
        int valid = 0, first = -1;
        for (int p = 0; p < G * B; ++p) {
            const int ty = types[p];
            if (ty >= 0 && ty < DCN_LOSS_NUM_TYPES) ++valid;
            if (first < 0 && ty != -1) first = ty;
        }
        out[0] = (double)iteration;
        out[1] = (double)state->active;
        out[2] = state->lr;
        out[3] = (double)valid;
        out[4] = loss;
        out[15] = (double)first;
    }
}

__global__ void __launch_bounds__(64)
train_log_kernel(double* __restrict__ history, int64_t row, int64_t iteration, const TrainState* __restrict__ state,
                 const float* __restrict__ loss, const float* __restrict__ terms, const int32_t* __restrict__ types, int B) {
    const int k = (int)threadIdx.x;
    log_row(history + row * DCN_TRAIN_LOG_COLUMNS, k, iteration, state, terms, 0, types, 1, B, k == 5 ? (double)loss[0] : 0.0);
}

// gathered float [G][1 + 5 B]: every rank's weighted loss, then its terms
__global__ void __launch_bounds__(64)
train_log_ranks_kernel(double* __restrict__ history, int64_t row, int64_t iteration, const TrainState* __restrict__ state,
                       const float* __restrict__ gathered, const int32_t* __restrict__ types_all, int G, int B) {
    const int k = (int)threadIdx.x;
    const size_t stride = 1 + (size_t)5 * B;
    double loss = 0.0;
    if (k == 5)
        for (int r = 0; r < G; ++r) loss += (double)gathered[r * stride];           // in rank order
    log_row(history + row * DCN_TRAIN_LOG_COLUMNS, k, iteration, state, gathered + 1, stride, types_all, G, B, loss);
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

extern "C" int dcn_train_advance_ranks(struct dcn_train_state* state, const int32_t* types_all, int G, int B, int rank,
                                       float* weight_out, int64_t iteration, int64_t steps_between_decay, double decay,
                                       double beta1, double beta2, void* stream) {
    if (!state || !types_all || !weight_out || G < 1 || B < 1 || rank < 0 || rank >= G) return DCN_E_INVALID;
    if ((int64_t)G * B > 0x7fffffff || steps_between_decay < 1 || !(decay >= 0.)) return DCN_E_INVALID;
    if (!dcn::adam_hyperparameters_valid(beta1, beta2, 0., 0.)) return DCN_E_INVALID;
    hipLaunchKernelGGL(train_advance_ranks_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, state, types_all, G, B, rank,
                       weight_out, iteration, steps_between_decay, decay, beta1, beta2);
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

extern "C" int dcn_train_log_ranks(double* history, int64_t row, int64_t iteration, const struct dcn_train_state* state,
                                   const float* gathered, const int32_t* types_all, int G, int B, void* stream) {
    if (!history || !state || !gathered || !types_all || G < 1 || B < 1 || row < 0) return DCN_E_INVALID;
    if ((int64_t)G * B > 0x7fffffff) return DCN_E_INVALID;
    hipLaunchKernelGGL(train_log_ranks_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, history, row, iteration, state,
                       gathered, types_all, G, B);
    return dcn::check_launch();
}
