// Adam update of the training step (reference: `optimizer.step()` at dense_correspondence/training/training.py:346 on the
// torch.optim.Adam built at training.py:133-145: lr 1e-4, weight_decay 1e-4, default betas / eps).
// HBM-bound streaming kernel: per element 4 reads (p, g, m, v) + 3 writes = 28 bytes, one pass, all tensors of the model
// in ceil(n / 80) launches (the tensor table travels in the kernel arguments; stock torch needs ~10 passes over 85 MB).
#include "adam_update.h"

namespace {

__global__ void __launch_bounds__(256)
adam_step_kernel(dcn::AdamTable t) {
    dcn::adam_update_chunk(t, t.s);
}

}  // namespace

extern "C" int dcn_adam_step(int n, void* const* param, const void* const* grad, void* const* exp_avg,
                             void* const* exp_avg_sq, const int64_t* numel, double lr, double beta1, double beta2,
                             double eps, double weight_decay, int64_t step, void* stream) {
    if (n < 0 || (n > 0 && (!param || !grad || !exp_avg || !exp_avg_sq || !numel))) return DCN_E_INVALID;
    if (step < 1 || !dcn::adam_hyperparameters_valid(beta1, beta2, eps, weight_decay) || !(lr >= 0.)) return DCN_E_INVALID;
    hipStream_t st = (hipStream_t)stream;
    dcn::AdamScalars s = dcn::adam_scalars(beta1, beta2, eps, weight_decay);
    dcn::adam_bias_corrections(lr, beta1, beta2, step, &s.step_size, &s.bc2_sqrt);
    return dcn::adam_for_each_table(n, param, grad, exp_avg, exp_avg_sq, numel, s, [&](const dcn::AdamTable& t, unsigned blocks) {
        hipLaunchKernelGGL(adam_step_kernel, dim3(blocks), dim3(256), 0, st, t);
    });
}
