/*
 * dcn_hip.h -- C ABI of libdcn_hip.so: the MI355X (gfx950) implementation of the dense-correspondence
 * training hot path of RobotLocomotion/pytorch-dense-correspondence.
 *
 * The reference has no native code and no FFI of its own: its hot path is Python that calls into
 * torch.  The entry points below are what a binding for that path replaces;
 * each cites the reference interface it stands in for (paths relative to the reference root).  The
 * host-side mirror of the reference's Python API that calls them through ctypes lives in
 * pytorch-dense-correspondence_amd/ (see INTEGRATION.md for the binding a maintainer would add).
 *
 * Conventions
 *   - plain C: pointers + sizes, no torch / C++ types.  All tensor pointers are DEVICE pointers owned
 *     by the caller (the PyTorch caching allocator in practice); the library allocates no device
 *     memory.  Pointer *arrays* (params / grads) are HOST arrays of device pointers.
 *   - every call is asynchronous on the caller's stream (`hipStream_t` passed as void*) and performs no host
 *     synchronisation.  The only process-wide state is the table of DCN_* environment overrides (read once, see
 *     dcn_reload_env).  A dcn_plan carries per-plan state (a side stream, events, profiling slots, the conv mode):
 *     use ONE plan per stream -- two streams driving the same plan concurrently would race; one process per GPU.
 *   - return value: 0 on success, negative DCN_E_* otherwise (never throws across the ABI).  The
 *     Python wrapper raises RuntimeError / ValueError like the reference does
 *     (dense_correspondence/network/dense_correspondence_network.py:381).
 *   - layouts: activations are NHWC fp32 (logical [N,C,H,W] in torch.channels_last memory), so the
 *     reference's own `view(N, D, W*H).permute(0, 2, 1)` (network.py:317-318) of the descriptor map is a
 *     contiguous [N, H*W, D] tensor.  Convolution weights are [Cout][kh][kw][Cin] (logical OIHW in
 *     channels_last memory).  Pixel indices are int64 `u + W*v`
 *     (dense_correspondence/dataset/spartan_dataset_masked.py:1256-1264).
 */
#ifndef DCN_HIP_H
#define DCN_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DCN_OK 0
#define DCN_E_INVALID (-1)     /* bad argument (shape, null pointer, unsupported architecture name) */
#define DCN_E_LAUNCH (-2)      /* a kernel launch failed (hipGetLastError != hipSuccess) */
#define DCN_E_UNSUPPORTED (-3) /* valid request the library does not implement */

/* Build identification: "dcn_hip <version> gfx950" for the shipped library, "... hostemu" for the
 * test-only host emulation build (tests/hostemu). */
const char* dcn_version(void);

/* The DCN_* environment overrides -- the full list with their meaning is the header comment of csrc/dcn_tuning.h:
 * DCN_CONV_MODE, DCN_BACKWARD_OVERLAP, DCN_GEMM_TILE_M, DCN_STEM8, DCN_GEMM_SK, DCN_GEMM_SK_MIN_GAIN,
 * DCN_GEMM_UNI, DCN_GEMM_SK_FIXUP, DCN_BN_BWD_FUSED, DCN_DEFER_RESIDUAL_ADD, DCN_WGRAD_TILE, DCN_WGRAD_DEEP, DCN_WGRAD_ROLES,
 * DCN_WGRAD_SPLITS, DCN_GEMM_HL, DCN_HL_MIN_K, DCN_GEMM_HL_ROWS, DCN_WGRAD_HL, DCN_HL_PRODUCERS, DCN_HL_ONLY_MID, DCN_STEM_POOL_FUSED, DCN_BN_REVERSE, DCN_BN_NT, DCN_BN_REDUCE_WIDE, DCN_WSPLIT_OVERLAP,
 * DCN_BN_BWD_LEAN (0: the batch-norm backward kernels never run their <= 48-VGPR instances beside the side stream's weight-gradient
 * GEMMs), DCN_BN_BWD_LEAN_MASK (which of them do: 1 reduce, 2 finalize, 4 blocked apply), DCN_BN_BWD_LEAN_DEPTH (rows in flight per
 * work-item of that blocked apply instance: 1, 2 or 3) -- are read ONCE, at the first call that needs them -- never on the
 * launch path.  dcn_reload_env re-reads them (tests / tuning scripts that change a variable in-process); not to be called
 * while another thread is inside the library. */
void dcn_reload_env(void);

/* The ONE exception to "the library allocates no device memory": a 64 KB buffer of arrival words per (device, stream) that
 * ever ran a K-split launch of the small-tile gather-GEMM (csrc/conv_hlx_kernels.hip; never while the stream is being
 * captured).  This call frees them all; the caller has synchronised those streams.  The Python binding registers it atexit. */
void dcn_release_pooled_buffers(void);

/* =====================================================================================================
 * 1. Pixelwise contrastive loss  (kernel K9)
 *
 * Replaces, fused into one pass over all pair lists of all image pairs of a step:
 *   PixelwiseContrastiveLoss.match_loss                  dense_correspondence/loss_functions/pixelwise_contrastive_loss.py:132-167
 *   PixelwiseContrastiveLoss.non_match_descriptor_loss   ...pixelwise_contrastive_loss.py:171-213
 *   PixelwiseContrastiveLoss.non_match_loss_descriptor_only / _with_l2_pixel_norm / l2_pixel_loss
 *                                                        ...pixelwise_contrastive_loss.py:215-352
 *   loss_composer.get_within_scene_loss / get_different_object_loss / get_same_object_across_scene_loss
 *                                                        dense_correspondence/loss_functions/loss_composer.py:70-212
 *   and their autograd (index_select backward == index_add_ into a zeroed [1,HW,D] buffer).
 *
 * Pair lists are ragged: for image pair p (0 <= p < num_pairs) and list type t the pairs are
 * idx_a[offsets[4p+t] .. offsets[4p+t+1]) / idx_b[...] with t = DCN_LIST_*.  An empty list (the
 * reference's `[-1]` sentinel, dense_correspondence_dataset_masked.py:209-223) has equal offsets.
 * num_pairs == 1 is exactly one reference iteration; for num_pairs > 1 every pair keeps its own
 * hard-negative normaliser and `loss = mean_p loss_p` (SURVEY.md section 8a note B).
 * ===================================================================================================== */

enum { DCN_LIST_MATCH = 0, DCN_LIST_MASKED = 1, DCN_LIST_BACKGROUND = 2, DCN_LIST_BLIND = 3, DCN_NUM_LISTS = 4 };

/* How the per-list sums are composed into `loss` (loss_composer.py). */
enum {
    DCN_COMPOSE_WITHIN_SCENE = 0,     /* loss_composer.py:70-143  (also MULTI_OBJECT / SYNTHETIC_MULTI_OBJECT) */
    DCN_COMPOSE_DIFFERENT_OBJECT = 1, /* loss_composer.py:168-191 blind list only, margin M_background */
    DCN_COMPOSE_ACROSS_SCENE = 2,     /* loss_composer.py:193-212 blind list only, inverted hinge, margin M_masked */
    DCN_COMPOSE_RAW_SUMS = 3          /* loss = match_weight * S_match + non_match_weight * (S_masked + S_background + S_blind):
                                         the un-normalised sums the PixelwiseContrastiveLoss building blocks return
                                         (pixelwise_contrastive_loss.py:271-304) */
};

typedef struct dcn_loss_config {
    float margin[DCN_NUM_LISTS];       /* hinge margin per list type (match entry unused) */
    int32_t invert[DCN_NUM_LISTS];     /* 0: max(0, M - d)^2;  1: max(0, d - M)^2 (pcl.py:205-208);  2: max(0, M - d^2), the legacy
                                          hinge on the squared distance of get_loss_original (pcl.py:399-404) */
    int32_t pixel_weight[DCN_NUM_LISTS]; /* 1: weight each term by min(|uv(gt) - uv(b)|, M_pixel)/M_pixel (pcl.py:307-334);
                                            the list must hold (len/len_match) consecutive entries per match */
    float m_pixel;
    int32_t image_width;
    float match_loss_weight;
    float non_match_loss_weight;
    int32_t scale_by_hard_negatives;   /* training.yaml:59 (or scale_by_hard_negatives_DIFFERENT_OBJECT for mode 1) */
    int32_t compose;                   /* DCN_COMPOSE_* */
} dcn_loss_config;

/* Bytes of scratch `dcn_contrastive_loss_forward` needs for `num_pairs` image pairs whose longest list
 * has `max_list_len` entries. */
size_t dcn_loss_workspace_bytes(int num_pairs, int64_t max_list_len);

/*
 * Forward.  desc_a / desc_b: [num_pairs, HW, D] contiguous fp32.
 *   terms      [num_pairs][5] : (loss_p, match_loss, masked_scaled, background_scaled, blind_scaled)  -- the 5-tuple
 *                               loss_composer.get_loss returns (loss_composer.py:143)
 *   sums       [num_pairs][4] : raw per-list sums  (match: sum ||a-b||^2; others: sum l_j [*w_j])
 *   hard_neg   [num_pairs][4] : int32 #{j : l_j != 0} per list (pcl.py:210-211); match entry = list length
 *   loss       [1]            : mean_p loss_p
 *   per_term   nullable [offsets[4*num_pairs]] : every pair's own term (match: ||a-b||^2, others l_j) --
 *                               the vector PixelwiseContrastiveLoss.non_match_descriptor_loss returns
 *   status     [1] int32      : set to 1 if any index was outside [0, HW) (such pairs are skipped)
 */
int dcn_contrastive_loss_forward(const float* desc_a, const float* desc_b, int num_pairs, int64_t hw, int d,
                                 const int64_t* idx_a, const int64_t* idx_b, const int64_t* offsets_host,
                                 const int64_t* offsets_dev, const dcn_loss_config* cfg, float* terms, float* sums,
                                 int32_t* hard_neg, float* loss, float* per_term, int32_t* status, void* workspace,
                                 void* stream);

/*
 * Backward of `loss` w.r.t. desc_a / desc_b.  grad_loss: device scalar (the upstream gradient).
 * grad_a / grad_b [num_pairs, HW, D] are zero-filled by this call and then accumulated into (duplicate
 * indices are legal and accumulate, correspondence_finder.py:326-328).  `sums` / `hard_neg` are the
 * forward outputs (read on device; no host round trip for the hard-negative count, unlike
 * pcl.py:210-211's nonzero()/len()).
 * pair_grad (nullable, [offsets[4*num_pairs]]): when given, the call instead back-propagates the
 * per-pair vector `per_term` of the forward: d/d desc of sum_j pair_grad[j] * per_term[j]  (the autograd of the
 * vector PixelwiseContrastiveLoss.non_match_descriptor_loss returns); grad_loss / sums / hard_neg are ignored.
 */
int dcn_contrastive_loss_backward(const float* desc_a, const float* desc_b, int num_pairs, int64_t hw, int d,
                                  const int64_t* idx_a, const int64_t* idx_b, const int64_t* offsets_host,
                                  const int64_t* offsets_dev, const dcn_loss_config* cfg, const float* sums,
                                  const int32_t* hard_neg, const float* grad_loss, const float* pair_grad,
                                  float* grad_a, float* grad_b, void* stream);

/* The same forward / backward pair with the backward's gathers traded for coalesced streams (round 4): the forward also
 * writes, per pixel pair, the difference vector a - b and the factor s with  d loss / d a = coef(list, image pair) * s * (a - b)
 * into pair_records (dcn_loss_saved_floats(total pairs, d) floats: [total][d] differences, then [total] factors); the backward
 * reads those records -- no descriptor is gathered a second time -- and scatter-adds the same values, bit for bit, as
 * dcn_contrastive_loss_backward.  prefilled != 0: the caller has already zero-filled grad_a / grad_b (dcn_fill_bytes on another
 * stream, overlapped with the forward kernels); the call then only accumulates. */
size_t dcn_loss_saved_floats(int64_t total_pairs, int d);
int dcn_contrastive_loss_forward_save(const float* desc_a, const float* desc_b, int num_pairs, int64_t hw, int d,
                                      const int64_t* idx_a, const int64_t* idx_b, const int64_t* offsets_host,
                                      const int64_t* offsets_dev, const dcn_loss_config* cfg, float* terms, float* sums,
                                      int32_t* hard_neg, float* loss, float* per_term, int32_t* status, void* workspace,
                                      float* pair_records, void* stream);
int dcn_contrastive_loss_backward_saved(int num_pairs, int64_t hw, int d, const int64_t* idx_a, const int64_t* idx_b,
                                        const int64_t* offsets_host, const int64_t* offsets_dev, const dcn_loss_config* cfg,
                                        const int32_t* hard_neg, const float* grad_loss, const float* pair_records,
                                        int prefilled, float* grad_a, float* grad_b, void* stream);

/* The same backward pass with BIT-REPRODUCIBLE gradient maps: every contribution is accumulated as 64-bit fixed point under a
 * per-image-pair power-of-two scale with integer atomics (order-independent), then converted once.  `workspace`:
 * dcn_loss_exact_workspace_bytes(num_pairs, hw, d) bytes (two int64 maps the size of the gradient maps x 2 + a word per pair).
 * grad_a / grad_b are written in full.  DCN_E_UNSUPPORTED when an image pair has >= 2^22 pixel pairs (use the float path).
 * Replaces the index_add_ backward of pixelwise_contrastive_loss.py:154-165,192-210 like the call above. */
size_t dcn_loss_exact_workspace_bytes(int num_pairs, int64_t hw, int d);
int dcn_contrastive_loss_backward_saved_exact(int num_pairs, int64_t hw, int d, const int64_t* idx_a, const int64_t* idx_b,
                                              const int64_t* offsets_host, const int64_t* offsets_dev,
                                              const dcn_loss_config* cfg, const int32_t* hard_neg, const float* grad_loss,
                                              const float* pair_records, void* workspace, float* grad_a, float* grad_b,
                                              void* stream);
/* Stream-ordered fill of n bytes (n % 4 == 0) with a byte value, as a kernel (an ordinary node under hipGraph capture). */
int dcn_fill_bytes(void* p, int byte_value, size_t n, void* stream);

/* -----------------------------------------------------------------------------------------------------
 * 1b. The same loss for a batch built on the device (section 9, dcn_concat_samples): nothing is known on the host but BOUNDS.
 *   offsets_dev [4 * num_pairs + 1] int64 and types_dev [num_pairs] int32 are read on the device only.  types_dev[p] is pair
 *   p's data type in SpartanDatasetDataType numbering (0 SINGLE_OBJECT_WITHIN_SCENE, 1 SINGLE_OBJECT_ACROSS_SCENE,
 *   2 DIFFERENT_OBJECT, 3 MULTI_OBJECT, 4 SYNTHETIC_MULTI_OBJECT) and selects cfgs[types_dev[p]] -- margins, hinge modes,
 *   pixel weights, hard-negative scaling and composition -- for that pair; -1 leaves the pair out (the reference's
 *   return_empty_data sample, which its training loop skips, training.py:304-306).
 *   Host bounds: no list is longer than max_list_len, no pair has more than max_pair_len entries in its four lists, and
 *   idx_a / idx_b hold `capacity` entries (entries past offsets[4 * num_pairs] are never read).  The launches are shaped by
 *   max_list_len, the records by capacity: pair_records holds dcn_loss_saved_floats(capacity, d) floats (NULL: none kept).
 *   workspace: dcn_loss_workspace_bytes(num_pairs, max_list_len) bytes.  num_pairs <= 16383.
 *     loss      [1]  = (sum of loss_p over the pairs kept) / max(num_valid, 1); the backward scales by the same 1 / num_valid
 *     num_valid [1] int32: the pairs kept
 *     terms / sums / hard_neg as section 1; a pair left out has zero rows there and in both gradient maps, whatever its
 *       offsets say
 *     status    [1] int32: DCN_LOSS_BAD_* bits, written (not accumulated) by the last kernel of the forward call
 *   A batch of one type without a pair left out gives the bits of dcn_contrastive_loss_forward_save / _backward_saved_exact
 *   with that type's configuration (same partial layout, same summation orders).
 *   dcn_contrastive_loss_mixed_backward_saved_exact: DCN_E_UNSUPPORTED when max_pair_len >= 2^22 (use the float path). */
#define DCN_LOSS_NUM_TYPES 5
#define DCN_LOSS_BAD_INDEX 1        /* status: an index outside [0, HW) (that pixel pair is skipped), as section 1 */
#define DCN_LOSS_BAD_TYPE 2         /* status: a type outside {-1, 0 .. 4} (the pair is left out) */
#define DCN_LOSS_BAD_BOUNDS 4       /* status: a list longer than max_list_len, a pair with more than max_pair_len entries,
                                       offsets that decrease, or offsets[4 * num_pairs] > capacity (the pairs concerned are
                                       left out; nothing is read outside idx_a / idx_b [0, capacity)) */
#define DCN_LOSS_BAD_PIXEL_LAYOUT 8 /* status: pixel-distance weighting for a pair whose non-match count is not a whole
                                       multiple of its match count (pixelwise_contrastive_loss.py:321-325) */
int dcn_contrastive_loss_mixed_forward(const float* desc_a, const float* desc_b, int num_pairs, int64_t hw, int d,
                                       const int64_t* idx_a, const int64_t* idx_b, const int64_t* offsets_dev,
                                       const int32_t* types_dev, const dcn_loss_config* cfgs, int64_t max_list_len,
                                       int64_t max_pair_len, int64_t capacity, float* terms, float* sums, int32_t* hard_neg,
                                       float* loss, int32_t* num_valid, int32_t* status, void* workspace, float* pair_records,
                                       void* stream);
int dcn_contrastive_loss_mixed_backward_saved(int num_pairs, int64_t hw, int d, const int64_t* idx_a, const int64_t* idx_b,
                                              const int64_t* offsets_dev, const int32_t* types_dev, const dcn_loss_config* cfgs,
                                              int64_t max_list_len, int64_t max_pair_len, int64_t capacity,
                                              const int32_t* hard_neg, const int32_t* num_valid, const float* grad_loss,
                                              const float* pair_records, int prefilled, float* grad_a, float* grad_b,
                                              void* stream);
int dcn_contrastive_loss_mixed_backward_saved_exact(int num_pairs, int64_t hw, int d, const int64_t* idx_a, const int64_t* idx_b,
                                                    const int64_t* offsets_dev, const int32_t* types_dev,
                                                    const dcn_loss_config* cfgs, int64_t max_list_len, int64_t max_pair_len,
                                                    int64_t capacity, const int32_t* hard_neg, const int32_t* num_valid,
                                                    const float* grad_loss, const float* pair_records, void* workspace,
                                                    float* grad_a, float* grad_b, void* stream);

/* Triplet variant (pixelwise_contrastive_loss.py:104-129, loss_composer.py:145-166):
 *   loss = 1/n * sum_i sum_k max(0, (a_k - m_k)^2 - (a_k - q_k)^2 + alpha),   a = A[non_a[i]], m = B[match_b[i / (n / n_match)]],
 *   q = B[non_b[i]]  -- hinge per descriptor component, exactly as the reference computes it.  n % n_match == 0.
 * desc_a / desc_b: [hw, d] of ONE image pair.  backward ACCUMULATES into grad_a / grad_b (zero-fill them first). */
size_t dcn_triplet_loss_workspace_bytes(int64_t n);
int dcn_triplet_loss_forward(const float* desc_a, const float* desc_b, int64_t hw, int d, const int64_t* non_a,
                             const int64_t* match_b, const int64_t* non_b, int64_t n, int64_t n_match, float alpha,
                             float* loss, int32_t* status, void* workspace, void* stream);
int dcn_triplet_loss_backward(const float* desc_a, const float* desc_b, int64_t hw, int d, const int64_t* non_a,
                              const int64_t* match_b, const int64_t* non_b, int64_t n, int64_t n_match, float alpha,
                              const float* grad_loss, float* grad_a, float* grad_b, void* stream);

/* =====================================================================================================
 * 2. Dilated-ResNet FCN backbone  (kernels K1-K8, K10)
 *
 * Replaces `self.fcn(img_tensor)` in DenseCorrespondenceNetwork.forward
 * (dense_correspondence/network/dense_correspondence_network.py:239-263) and its autograd, for
 * fcn = resnet_dilated.Resnet{18,34,50,101}_8s(num_classes=D) (network.py:373-375; the module itself is
 * third-party, see oracle/resnet_dilated_oracle.py).
 *
 * A plan fixes (architecture, N, H, W, D).  Parameters are passed as a host array of device pointers in
 * the order dcn_plan_param_name enumerates them, which is the reference checkpoint's state_dict order
 * (`conv1.weight, bn1.weight, bn1.bias, layer1.0.conv1.weight, ... fc.weight, fc.bias`); BN running
 * statistics as a second array (`bn1.running_mean, bn1.running_var, layer1.0.bn1.running_mean, ...`).
 * ===================================================================================================== */

typedef struct dcn_plan dcn_plan;

/* arch: "Resnet18_8s" | "Resnet34_8s" | "Resnet50_8s" | "Resnet101_8s".  base_width = 64 for the real
 * networks (smaller widths, multiples of 4, exist for tests). */
int dcn_plan_create(const char* arch, int base_width, int n, int h, int w, int d, dcn_plan** out);
/* `groups` (1 or 2) independent batches of n / groups images stacked along N: ONE launch sequence computes what
 * `groups` consecutive forward calls of the reference compute (training.py:329-333 forwards img_a and img_b through the
 * same weights) -- batch-norm statistics, their backward and the running-statistics updates are per group, in order.
 * Larger launches fill the 256 CUs better at small batch.  DCN_E_UNSUPPORTED if a group's rows are not tile-aligned. */
int dcn_plan_create_grouped(const char* arch, int base_width, int n, int groups, int h, int w, int d, dcn_plan** out);
void dcn_plan_destroy(dcn_plan* plan);
/* A training-mode forward call leaves a small host-side record keyed by its `saved` pointer (what the matching backward call
 * must agree with).  dcn_plan_forget_saved drops it when the caller releases that arena without (or after) differentiating
 * it -- returns how many records were dropped; dcn_plan_num_forward_records counts the records a plan holds. */
int dcn_plan_forget_saved(dcn_plan* plan, const void* saved);
int dcn_plan_num_forward_records(const dcn_plan* plan);

/* How the plan's convolutions multiply.  Both modes take and return fp32 tensors and accumulate in fp32.
 *   DCN_CONV_FP32  : fp32 MFMA (v_mfma_f32_32x32x2_f32), 157 TFLOP/s peak.
 *   DCN_CONV_F16X3 : split-fp16 -- every operand element x is split on the fly into fp16 hi + lo with
 *                    s*x = hi + lo (s a power of two: 64 for weights, chosen from the tensor's abs-max for
 *                    gradients AND activations -- every tensor that feeds a convolution carries a device scalar
 *                    with (a bound of) its abs-max, written by the kernel that produced it) and
 *                    hi*hi + hi*lo + lo*hi runs on the fp16 MFMA pipe.  ~22 mantissa bits per operand:
 *                    indistinguishable from fp32 on this network, ~2x faster.  Operand range: any finite
 *                    fp32 tensor (the pre-scale brings its abs-max to <= 4096); |weight| < 1023.
 * Default: DCN_CONV_F16X3, or the environment variable DCN_CONV_MODE = "fp32" | "f16x3" at plan creation.
 * The saved / workspace arenas are sized for either mode, so the mode may be switched between steps (not between a
 * forward and its backward). */
#define DCN_CONV_FP32 0
#define DCN_CONV_F16X3 1
int dcn_plan_set_conv_mode(dcn_plan* plan, int mode);
int dcn_plan_conv_mode(const dcn_plan* plan);

int dcn_plan_num_params(const dcn_plan* plan);
int dcn_plan_num_bn(const dcn_plan* plan);
/* name (without the "resnet34_8s." prefix) and logical OIHW / [C] shape of parameter i; ndim is 4 or 1. */
int dcn_plan_param_info(const dcn_plan* plan, int i, char* name, int name_cap, int64_t shape[4], int* ndim);
/* name prefix ("layer1.0.bn1") and channel count of batch-norm j. */
int dcn_plan_bn_info(const dcn_plan* plan, int j, char* name, int name_cap, int64_t* channels);

/* number of batch norms of the last dcn_backbone_backward call whose backward reduction ran in the epilogue of the dgrad
 * that produced their upstream gradient (split-fp16 mode; DCN_BN_BWD_FUSED=0 disables) */
int dcn_plan_fused_bn_backward(const dcn_plan* plan);

/* Inside the `saved` buffer of a forward call, at byte offset dcn_plan_activation_absmax_offset: one float per
 * activation tensor that feeds a convolution (dcn_plan_num_activation_slots of them; slot 0 = the input image) with its
 * abs-max as the split-fp16 kernels used it (all zero in fp32 mode), followed by one int32 STATUS word: bit 0 = some
 * convolution input was not finite (inf / NaN) in that call.  Read it after the call (device memory; no sync is forced). */
int dcn_plan_num_activation_slots(const dcn_plan* plan);
size_t dcn_plan_activation_absmax_offset(const dcn_plan* plan);

/* Gradient buckets for data-parallel training: the parameters split into
 * dcn_plan_num_grad_buckets contiguous ranges of the state-dict order -- bucket k = parameters
 * [first_param(k), first_param(k - 1)), bucket 0 ending at the last parameter -- numbered in the order the backward pass
 * completes them (k = 0: fc + layer4, 62 % of Resnet34_8s; 1: layer3; 2: the rest).  dcn_backbone_backward records an
 * event per bucket on its stream once every launch that writes one of the bucket's gradients has been enqueued;
 * dcn_plan_stream_wait_grad_bucket makes `stream` wait for that event, so that a communication stream can all-reduce
 * bucket k (RCCL) while the caller's stream is still computing buckets k + 1, ...  Call it after
 * dcn_backbone_backward has returned; DCN_E_UNSUPPORTED before the plan's first backward pass. */
int dcn_plan_num_grad_buckets(const dcn_plan* plan);
int dcn_plan_grad_bucket_first_param(const dcn_plan* plan, int k);
int dcn_plan_stream_wait_grad_bucket(dcn_plan* plan, int k, void* stream);

size_t dcn_plan_saved_bytes(const dcn_plan* plan);     /* activations kept from forward to backward */
size_t dcn_plan_workspace_bytes(const dcn_plan* plan); /* scratch shared by forward and backward */
double dcn_plan_forward_flops(const dcn_plan* plan);   /* algorithmic conv FLOPs of one forward (2*MAC) */

/*
 * Forward.  image: [N,3,H,W] fp32 NCHW (what the reference's DataLoader yields, training.py:311-312).
 * descriptors: [N,H,W,D] fp32 (== logical [N,D,H,W] channels_last).
 * training != 0: batch statistics over the N images of this call + running-stat update with `momentum`
 * (nn.BatchNorm2d semantics); training == 0: running statistics.  normalize != 0 applies
 * network.py:256-259 (per-pixel L2 normalisation over D).
 * saved (dcn_plan_saved_bytes) and workspace (dcn_plan_workspace_bytes) are always required.
 */
int dcn_backbone_forward(dcn_plan* plan, const float* image, const float* const* params,
                         float* const* bn_running, float momentum, float eps, int training, int normalize,
                         float* descriptors, void* saved, void* workspace, void* stream);

/* The same call for a grouped plan (dcn_plan_create_grouped, groups == 2) whose two image batches are separate tensors:
 * images [0, N/2) are read from image_a, [N/2, N) from image_b ([N/2,3,H,W] each) -- forward(img_a), forward(img_b) of
 * training.py:329-333 as one launch sequence without a concatenated copy of the batches. */
int dcn_backbone_forward_pair(dcn_plan* plan, const float* image_a, const float* image_b, const float* const* params,
                              float* const* bn_running, float momentum, float eps, int training, int normalize,
                              float* descriptors, void* saved, void* workspace, void* stream);

/*
 * Launch-level timing of the two matrix-core kernels (for bench.py's roofline): between begin and end every
 * conv_gemm_kernel (forward + dgrad; category 0) and conv_wgrad_kernel (category 1) launch made through this
 * plan is bracketed by hipEventRecord on the caller's stream.  `end` synchronises on the recorded events and
 * returns, per category, the summed kernel milliseconds, the number of launches and the algorithmic FLOPs
 * (2 * MACs of the convolution being computed, padding not counted).
 */
int dcn_plan_profile_begin(dcn_plan* plan);
int dcn_plan_profile_end(dcn_plan* plan, double ms[2], int64_t launches[2], double flops[2]);
/* The same with a third category: [2] = the part of category 0 that ran on the pre-split (hl32) LDS-DMA kernel
 * (conv_hl_kernels.hip; an operand split pass that had to run in front of a launch is inside its bracket). */
int dcn_plan_profile_end3(dcn_plan* plan, double ms[3], int64_t launches[3], double flops[3]);
/* EVERY launch the engine makes between begin and end, by category (bench.py: `roofline_elementwise`, `kernel_ms_sum`):
 * work[c] = algorithmic FLOPs for the three matrix-core categories, algorithmic HBM bytes (4 B x elements read and
 * written, the operands a pass needs once) for the streaming ones, 0 where neither is meaningful.  Category
 * DCN_PROF_GEMM_HL is a subset of DCN_PROF_GEMM (as in dcn_plan_profile_end3); the others are disjoint, so the launches
 * of a step are  sum over c != DCN_PROF_GEMM_HL.  Arrays of DCN_PROF_NCAT entries. */
enum {
    DCN_PROF_GEMM = 0,           /* gather-GEMM convolutions, forward + dgrad (all kernels) */
    DCN_PROF_WGRAD = 1,          /* weight-gradient GEMMs (their slab-reduce launch included) */
    DCN_PROF_GEMM_HL = 2,        /* the part of DCN_PROF_GEMM on the pre-split (hl32) kernel */
    DCN_PROF_BN_APPLY = 3,       /* batch-norm apply (+ residual, ReLU, mask, hl32 image): one streaming pass */
    DCN_PROF_BN_BWD_REDUCE = 4,  /* batch-norm backward reduction pass */
    DCN_PROF_BN_BWD_APPLY = 5,   /* batch-norm backward apply pass (+ the gradient's operand images) */
    DCN_PROF_BN_FINALIZE = 6,    /* the two per-channel finalize kernels (latency-bound) */
    DCN_PROF_RESAMPLE = 7,       /* max pool, bilinear upsample (forward and backward), NCHW -> NHWC4 of the input */
    DCN_PROF_OTHER = 8,          /* fills, weight splits, stand-alone operand splits, status / bias-gradient kernels */
    DCN_PROF_NCAT = 9
};
int dcn_plan_profile_end_all(dcn_plan* plan, double ms[DCN_PROF_NCAT], int64_t launches[DCN_PROF_NCAT],
                             double work[DCN_PROF_NCAT]);

/* Backward.  grad_descriptors: [N,H,W,D]; grads[i] receives dL/d params[i] (overwritten, same layout as
 * params[i]).  `saved` is the buffer the matching forward filled; `normalize` must be the forward's flag. */
int dcn_backbone_backward(dcn_plan* plan, const float* grad_descriptors, const float* const* params,
                          const void* saved, void* workspace, float* const* grads, int normalize, void* stream);
/* Grouped plan, the two batches' descriptor gradients as separate [N/2,H,W,D] tensors (the two outputs of a
 * dcn_backbone_forward_pair call receive their gradients separately).  Both backward entry points return DCN_E_INVALID when
 * `saved` was not filled by a training-mode forward call of this plan in the plan's current arithmetic, or when the tuning
 * switches (dcn_reload_env) changed since in a way that would make the pass read a tensor that call did not write. */
int dcn_backbone_backward_pair(dcn_plan* plan, const float* grad_a, const float* grad_b, const float* const* params,
                               const void* saved, void* workspace, float* const* grads, int normalize, void* stream);

/* =====================================================================================================
 * 3. Individual kernels, exported for unit tests and micro-benchmarks (same conventions).
 * ===================================================================================================== */

typedef struct dcn_conv_desc {
    int32_t n, hin, win, cin;   /* input  [n, hin, win, cin] NHWC, cin % 4 == 0 */
    int32_t hout, wout, cout;   /* output [n, hout, wout, cout], leading dimension ldc >= cout */
    int32_t kh, kw, stride, pad, dil;
    int32_t ldc;
    int32_t group_rows;         /* 0, or: output rows (pixels) per batch-norm group -- the forward kernel then picks an M
                                   tile that divides it, so that no row of bn_partial mixes two groups (% 64 == 0 required) */
} dcn_conv_desc;

/* out = conv(in, w) [+ bias];  w: [cout][kh][kw][cin].  If bn_partial != NULL also writes per-M-tile
 * partial sums for batch-norm statistics: bn_partial[tile][3][cout] (sum, sum of squares, max |x|); the number of
 * tiles is returned by dcn_conv_num_mtiles. */
/* workspace (nullable): dcn_conv_gemm_workspace(c, dgrad) bytes; enables the stream-K work split used when the layer
 * has too few output tiles to load all 256 CUs evenly (small batch). */
int dcn_conv_forward(const dcn_conv_desc* c, const float* in, const float* w, const float* bias, float* out,
                     float* bn_partial, void* workspace, void* stream);
size_t dcn_conv_gemm_workspace(const dcn_conv_desc* c, int dgrad);
int dcn_conv_num_mtiles(const dcn_conv_desc* c);
/* din = conv_transpose(dout, w) [+ add];  wt: [cin][kh][kw][cout] (see dcn_transpose_weight). */
int dcn_conv_dgrad(const dcn_conv_desc* c, const float* dout, const float* wt, const float* add, float* din,
                   void* workspace, void* stream);
/* dw[cout][kh][kw][cin] = sum_m dout[m][cout] * in[pix(m,tap)][cin]; slabs: scratch of dcn_conv_wgrad_workspace bytes */
int dcn_conv_wgrad(const dcn_conv_desc* c, const float* in, const float* dout, float* dw, void* slabs, void* stream);
size_t dcn_conv_wgrad_workspace(const dcn_conv_desc* c);
/* wt[c][tap][0..ldn) = (w[0..cout)[tap][c], zeros);  ldn >= cout is the row pitch of dout in dcn_conv_dgrad */
int dcn_transpose_weight(const float* w, float* wt, int cout, int taps, int cin, int ldn, void* stream);

/* ---- split-fp16 ("f16x3") variants: same tensors and results to ~fp32 accuracy, products on the fp16 matrix pipe
 * (see csrc/conv_f16_kernels.hip).  Weights are pre-split with dcn_split_rows_f16 into two fp16 arrays of
 * rows x dcn_f16_kpad(K) (hi, lo), scaled by the power of two `w_scale`. */
int dcn_f16_kpad(int k);
int dcn_split_rows_f16(const float* w, void* hi, void* lo, int64_t rows, int k, float scale, void* stream);
int dcn_conv_num_mtiles_f16(const dcn_conv_desc* c);
size_t dcn_conv_gemm_workspace_f16(const dcn_conv_desc* c, int dgrad);
/* in_absmax: device scalar >= max|in| (picks the power-of-two pre-scale of the activation tensor) or NULL for scale 1 */
int dcn_conv_forward_f16(const dcn_conv_desc* c, const float* in, const float* in_absmax, const void* w_hi, const void* w_lo,
                         float w_scale, const float* bias, float* out, float* bn_partial, void* workspace, void* stream);
/* dout_absmax: device scalar >= max|dout| (picks the power-of-two pre-scale of the gradient tensor) or NULL */
int dcn_conv_dgrad_f16(const dcn_conv_desc* c, const float* dout, const void* wt_hi, const void* wt_lo, float w_scale,
                       const float* dout_absmax, const float* add, float* din, void* workspace, void* stream);
/* dcn_conv_dgrad_f16 whose result din is the upstream gradient of a train-mode batch norm (the one that produced this
 * convolution's input, training.py:345 through the backbone's BasicBlock): the batch norm's backward REDUCTION runs in the
 * GEMM epilogue.  din receives the gradient masked by relu_mask (the bytes dcn_bn_forward wrote for that batch norm's
 * output; NULL: no ReLU) and bn_partial[dcn_conv_dgrad_bn_num_mtiles_f16(c)][cin][4] the per-tile sums that
 * dcn_bn_backward_from_partial consumes.  bn_x: the batch norm's input [n, hin, win, cin]; bn_stats: its statistics
 * [4][cin] (per group when c->group_rows is set: M tiles then never straddle a group). */
int dcn_conv_dgrad_bn_num_mtiles_f16(const dcn_conv_desc* c);
int dcn_conv_dgrad_bn_f16(const dcn_conv_desc* c, const float* dout, const void* wt_hi, const void* wt_lo, float w_scale,
                          const float* dout_absmax, const float* add, float* din, const float* bn_x,
                          const unsigned char* relu_mask, const float* bn_stats, float* bn_partial, void* workspace,
                          void* stream);

/* dcn_split_weights_scaled_f16 (forward images; row_scale nullable) with a range check: bit 1 of the device word *status (not
 * cleared by the call) is raised when some |scale * row_scale * w| leaves fp16's range or is NaN -- with the engine's fixed
 * weight scale 64 that is |w| >= 1023.  The backbone engine passes the status word behind its activation abs-max slots
 * (dcn_plan_activation_absmax_offset). */
int dcn_split_weights_checked_f16(int n, const float* const* w, const float* const* row_scale, void* const* hi, void* const* lo,
                                  const int* cout, const int* taps, const int* cin, float scale, int* status, void* stream);

/* ---- pre-split ("hl32") operand path of the wide layers (csrc/conv_hl_kernels.hip): the forward convolution and dgrad of
 * every stride-1 convolution with >= 256 destination channels and source channels % 32 == 0 (layers 3-4 of the backbone behind
 * network.py:255 / training.py:345).  Operands are "hl32" tensors -- per 32-channel chunk one 128-byte line
 * [hi x32 | lo x32] fp16, the byte size of the fp32 tensor -- so that the GEMM loop is LDS-DMA + MFMA only (256 x 256 tiles,
 * two wavefront groups one phase apart; round 5: 160 x 256 / 160 x 128 tiles with a K split for the launches the big tiles do
 * not fill the chip with -- B = 1, training.yaml:14 -- from 128 destination channels on: csrc/conv_hlx_kernels.hip).  Results equal dcn_conv_forward_f16 / dcn_conv_dgrad_f16 (same products, other
 * summation order).  dcn_conv_hl_eligible: 1 when the descriptor qualifies (forward: dgrad = 0). */
int dcn_conv_hl_eligible(const dcn_conv_desc* c, int dgrad);
int dcn_conv_num_mtiles_hl(const dcn_conv_desc* c);
/* rows per tile of the launch (256, or 192 / 320 where that fills the 256 CUs better; DCN_GEMM_HL_ROWS forces one) */
int dcn_conv_tile_rows_hl(const dcn_conv_desc* c, int dgrad);
size_t dcn_conv_gemm_workspace_hl(const dcn_conv_desc* c, int dgrad);
/* the tile the launch of this convolution takes under the tuning of the moment: info[0..5] = rows (256 / 192 / 320: the big
 * tiles; 160: the small-tile kernel of csrc/conv_hlx_kernels.hip -- round 5: the reference's batch_size 1,
 * training.yaml:14, and its two separate forward calls, training.py:329-333), columns, K groups inside the workgroup,
 * workgroups per tile along K, M tiles, N tiles.  Returns 0, or DCN_E_UNSUPPORTED when no tile height fits. */
int dcn_conv_hl_shape_info(const dcn_conv_desc* c, int dgrad, int* info6);
/* fp32 [rows][channels] (channels % 32 == 0) -> hl32, scaled by the power of two chosen from *absmax (NULL: 1) */
int dcn_split_act_hl32(const float* src, const float* absmax, void* dst, int64_t rows, int channels, void* stream);
/* n weight tensors w[i] = [cout][taps][cin] -> out[i] = hl32 [cout][taps*cin/32][hi|lo], or (transposed) the dgrad image
 * [cin][taps*ldn/32][hi|lo]; all arrays are HOST arrays */
int dcn_split_weights_hl32(int n, const float* const* w, void* const* out, const int* cout, const int* taps, const int* cin,
                           const int* ldn, int transposed, float scale, void* stream);
int dcn_conv_forward_hl(const dcn_conv_desc* c, const void* in_hl, const float* in_absmax, const void* w_hl, float w_scale,
                        const float* bias, float* out, float* bn_partial, void* workspace, void* stream);
int dcn_conv_dgrad_hl(const dcn_conv_desc* c, const void* dout_hl, const void* wt_hl, float w_scale, const float* dout_absmax,
                      const float* add, float* din, void* workspace, void* stream);

/* Weight gradient on hl32 operands (csrc/wgrad_hl_kernels.hip; the wgrad of training.py:345 for the same wide layers): x_hl /
 * dout_hl are the hl32 images of the convolution's input and of the output gradient (scaled by the powers of two chosen from
 * *x_absmax / *dout_absmax).  256 x 256 tiles, pixel-major tiles by LDS-DMA, k-major fragments by transposing LDS reads.
 * Same result as dcn_conv_wgrad_f16 (same products, other summation order); bit-reproducible.
 * Round 5: the narrow 3 x 3 layers (64 / 128 input channels, stride 1, dilation 1: ResNet layers 1 and 2) take a second kernel behind
 * the same entry points -- 64 output channels x nine taps x all input channels per workgroup, three row windows of x per
 * 32-pixel stage (conv_wgrad_hlr_kernel).  dcn_conv_wgrad_hl_kind: which kernel dcn_conv_wgrad_hl launches for c now --
 * 0 none (unsupported), 1 the 256 x 256 tile kernel, 2 the row-window kernel. */
int dcn_conv_wgrad_hl_eligible(const dcn_conv_desc* c);
int dcn_conv_wgrad_hl_kind(const dcn_conv_desc* c);
size_t dcn_conv_wgrad_workspace_hl(const dcn_conv_desc* c);
int dcn_conv_wgrad_hl(const dcn_conv_desc* c, const void* x_hl, const float* x_absmax, const void* dout_hl,
                      const float* dout_absmax, float* dw, void* slabs, void* stream);

/* The backbone's stem (7x7 / stride 2 / pad 3 on 3 + 1 zero input channels; K1 of SURVEY.md section 8a) as a uniform-tap
 * convolution: a filter ROW is one 32-K chunk (8 pixels x 4 channels = 128 contiguous bytes of the NHWC4 image, the 8th
 * pixel with zero weights), so the gather is the wide layers' per-row buffer load instead of a per-element tap decode.
 * w4: [cout][7][7][4] fp32; hi / lo receive [cout][7][8][4] fp16.  Same result as dcn_conv_forward_f16. */
int dcn_split_stem_weights_f16(const float* w4, void* hi, void* lo, int cout, float scale, void* stream);
int dcn_conv_stem_forward_f16(const dcn_conv_desc* c, const float* in, const float* in_absmax, const void* w_hi, const void* w_lo,
                              float w_scale, float* out, float* bn_partial, void* stream);

/* All weight tensors of a network in one launch: w[i] = [cout[i]][taps[i]][cin[i]] (device), hi[i] / lo[i] (device) receive
 * the forward image [cout][kpad(taps*cin)] or, transposed != 0, the dgrad image [cin][kpad(taps*ldn[i])] of
 * dcn_transpose_weight + dcn_split_rows_f16.  The seven arrays themselves are HOST arrays of length n. */
int dcn_split_weights_f16(int n, const float* const* w, void* const* hi, void* const* lo, const int* cout, const int* taps,
                          const int* cin, const int* ldn, int transposed, float scale, void* stream);

/* as above with optional per-output-channel factors (forward images only): row_scale[i] = NULL or device vector [cout[i]] */
int dcn_split_weights_scaled_f16(int n, const float* const* w, const float* const* row_scale, void* const* hi,
                                 void* const* lo, const int* cout, const int* taps, const int* cin, const int* ldn,
                                 int transposed, float scale, void* stream);
/* inference: out = [relu](conv(in, w) + bias [+ add]) in one pass (eval-mode batch norm folded into w and bias);
 * out_absmax (nullable): device scalar raised to max|out| -- the in_absmax of the convolution that reads `out` next */
int dcn_conv_forward_fused_f16(const dcn_conv_desc* c, const float* in, const float* in_absmax, const void* w_hi,
                               const void* w_lo, float w_scale, const float* bias, const float* add, int relu, float* out,
                               float* out_absmax, void* workspace, void* stream);

/* wgrad consumes PRE-SPLIT operands (every element takes part in many tiles, so the fp32 -> fp16 hi/lo split is done
 * once per tensor).  Both split tensors have the byte size of their fp32 source:
 *   activations  xs[pixel][c/4][hi x4 | lo x4]                       dcn_split_act_f16 (n elements, n % 4 == 0)
 *   out-gradient dq[m/4][4 sub-planes][ldc/4][2 channels x 4 pixels], scaled by the power of two chosen from *absmax
 *                (dcn_split_grad_blocked_f16; dcn_grad_blocked_bytes(M, ldc) bytes).  dout_absmax = the same scalar. */
int dcn_split_act_f16(const float* src, void* xs, int64_t n, void* stream);
size_t dcn_grad_blocked_bytes(int m, int ld);
int dcn_split_grad_blocked_f16(const float* dy, int m, int ld, const float* absmax, void* dq, void* stream);
/* xs_is_fp32 != 0: `xs` is the fp32 activation tensor itself, split on the fly (cheaper than a split pass when every
 * element is only used by a few tiles, e.g. 1x1 convolutions); x_absmax (nullable, fp32 operand only): device scalar
 * >= max|xs| for its power-of-two pre-scale */
int dcn_conv_wgrad_f16(const dcn_conv_desc* c, const void* xs, int xs_is_fp32, const float* x_absmax, const void* dq,
                       const float* dout_absmax, float* dw, void* slabs, void* stream);
size_t dcn_conv_wgrad_workspace_f16(const dcn_conv_desc* c);

/* Train-mode batch norm (+ residual) (+ ReLU) of a convolution output x [rows][c] (kernel K7; nn.BatchNorm2d as the
 * backbone uses it): statistics from the per-M-tile partial sums the convolution's epilogue wrote (bn_partial
 * [mtiles][3][c], dcn_conv_forward), running statistics updated with `momentum` (unbiased variance); training == 0: the
 * running statistics are used instead.  y = [relu](x * scale + shift [+ res]); relu_mask (nullable): one byte per
 * float4 of y, bit j = y[4 i + j] > 0.  stats [4][c] receives scale, shift, mean, invstd (read by dcn_bn_backward). */
int dcn_bn_forward(const float* x, const float* bn_partial, int mtiles, int c, int64_t rows, const float* gamma,
                   const float* beta, float* running_mean, float* running_var, float momentum, float eps, int training,
                   const float* res, int relu, float* y, unsigned char* relu_mask, float* stats, void* stream);
/* dx, dgamma, dbeta of the above given dy (masked by relu_mask when given); g_out (nullable) receives the masked dy
 * (the residual branch's gradient).  workspace: dcn_bn_backward_workspace(rows, c) bytes. */
size_t dcn_bn_backward_workspace(int64_t rows, int c);
int dcn_bn_backward(const float* dy, const unsigned char* relu_mask, const float* x, const float* stats, const float* gamma,
                    int c, int64_t rows, float* dgamma, float* dbeta, float* dx, float* g_out, void* workspace,
                    void* stream);
/* dcn_bn_backward with the reduction already done by dcn_conv_dgrad_bn_f16 (dy masked, bn_partial [mtiles][c][4]);
 * workspace: 3 * c floats */
int dcn_bn_backward_from_partial(const float* dy, const float* bn_partial, int mtiles, const float* x, const float* stats,
                                 const float* gamma, int c, int64_t rows, float* dgamma, float* dbeta, float* dx,
                                 void* workspace, void* stream);
/* dcn_bn_backward with every optional input and output of the engine's batch-norm backward step (tests of its kernel variants):
 * the upstream gradient is dy (+ dy2), masked by relu_mask (bytes of dcn_bn_forward) or else by relu_out > 0 or not at all;
 * groups (1 | 2) batches stacked along the rows, stats [groups][4][c]; absmax (optional): one float, raised to a bound of
 * max |dx|; dq (optional, with absmax): dx as the pixel-blocked split-fp16 image, 4 * c * round_up(rows, 4) bytes; hl_dx
 * (optional, with absmax, c % 32 == 0): dx as the hl32 image, 4 * c * rows bytes -- dx itself may then be null unless keep_dx.
 * With two groups and dq / hl_dx, rows / groups must be a multiple of 4.  workspace: dcn_bn_backward_full_workspace bytes;
 * its last groups * 3 * c floats receive the coefficients k1, k2, k3 of the apply pass, [groups][3][c]. */
size_t dcn_bn_backward_full_workspace(int64_t rows, int c, int groups);
int dcn_bn_backward_full(const float* dy, const float* dy2, const float* relu_out, const unsigned char* relu_mask,
                         const float* x, const float* stats, const float* gamma, int c, int64_t rows, int groups,
                         float* dgamma, float* dbeta, float* dx, float* g_out, float* absmax, void* dq, void* hl_dx,
                         int keep_dx, void* workspace, void* stream);
/* 3x3 / stride 2 / pad 1 max pool (kernel K2) of in [n,hin,win,c] -> out [n,(hin+1)/2,(win+1)/2,c]; argmax (nullable in
 * forward): one byte per output element (window position 0..8); backward gathers with it (deterministic). */
int dcn_maxpool_forward(const float* in, int n, int hin, int win, int c, float* out, unsigned char* argmax, void* stream);
int dcn_maxpool_backward(const float* gout, const unsigned char* argmax, int n, int hin, int win, int c, float* gin,
                         void* stream);

/* bilinear xS upsample, align_corners=True (F.upsample_bilinear): low [n,hl,wl,ldl] -> out [n,h,w,d] */
int dcn_upsample_forward(const float* low, int n, int hl, int wl, int ldl, int d, int h, int w, int normalize,
                         float* out, void* stream);
/* glow [n,hl,wl,ldl] (pad channels zeroed); tmp: scratch of dcn_upsample_backward_tmp_bytes(n, hl, w, d) bytes */
int dcn_upsample_backward(const float* gout, int n, int hl, int wl, int ldl, int d, int h, int w, float* glow,
                          float* tmp, void* stream);
size_t dcn_upsample_backward_tmp_bytes(int n, int hl, int w, int d);

/* The same kernels with every optional input and output the engine launches them with (unit tests of the variants no entry point
 * above reaches); each is the engine's own launcher behind an argument check.
 * dcn_maxpool_forward_full: bn_stats (nullable, [groups][4][c] as dcn_bn_forward writes them, groups 1 | 2, n % groups == 0): `in` is
 *   a convolution output and y = relu(in * scale + shift) is applied on the way into the window maximum, per group of n / groups
 *   images; relu_mask (nullable, with bn_stats only) receives the one-byte-per-float4 sign mask of y, n * hin * win * c / 4 bytes.
 * dcn_maxpool_backward_full: gout2 (nullable): the gradient of the pooled tensor is gout + gout2. */
int dcn_maxpool_forward_full(const float* in, const float* bn_stats, int groups, int n, int hin, int win, int c, float* out,
                             unsigned char* argmax, unsigned char* relu_mask, void* stream);
int dcn_maxpool_backward_full(const float* gout, const float* gout2, const unsigned char* argmax, int n, int hin, int win, int c,
                              float* gin, void* stream);
/* backward of the L2 normalisation fused into dcn_upsample_forward(normalize = 1): gv [n,h,w,d] = gradient w.r.t. the
 * interpolated map v (re-interpolated from low) given gout = gradient w.r.t. v / ||v|| */
int dcn_normalize_backward(const float* low, int n, int hl, int wl, int ldl, int d, int h, int w, const float* gout, float* gv,
                           void* stream);
/* dcn_upsample_backward with gout_b (nullable, n even): the gradient of images [n / 2, n) as a tensor of its own, and absmax
 * (nullable): one float, raised to max |glow| */
int dcn_upsample_backward_full(const float* gout, const float* gout_b, int n, int hl, int wl, int ldl, int d, int h, int w,
                               float* glow, float* tmp, float* absmax, void* stream);
/* img [n,3,hw] (NCHW) -> out [n,hw,4] = (R, G, B, 0); absmax (nullable): one float, raised to max |img|, to +inf when img holds a NaN */
int dcn_image_to_nhwc4(const float* img, int n, int hw, float* out, float* absmax, void* stream);
/* [rows][3] -> [rows][4] with a zero fourth lane, and back; [rows][d] -> [rows][ld] (ld >= d) with zero pad columns */
int dcn_pad_c3_to_c4(const float* src, float* dst, int64_t rows, void* stream);
int dcn_unpad_c4_to_c3(const float* src, float* dst, int64_t rows, void* stream);
int dcn_pad_rows(const float* src, float* dst, int64_t rows, int d, int ld, void* stream);
/* out[j] = sum over the rows of m[rows][ld] of column j, j < d <= ld (the fc.bias gradient; fp64 accumulation, fixed order) */
int dcn_column_sums(const float* m, int64_t rows, int ld, int d, float* out, void* stream);

/* =====================================================================================================
 * 4. Best-match search over a descriptor image (evaluation / heat-map side)
 *
 * Replaces DenseCorrespondenceNetwork.find_best_match / find_best_match_for_descriptor
 * (dense_correspondence/network/dense_correspondence_network.py:488-550: numpy
 * `sqrt(sum(square(res_b - d), axis=2))` + argmin, once per query) for Q queries in one pass.
 *   res        [HW][D] fp32 descriptor image (the [H,W,D] tensor forward_single_image_tensor returns)
 *   queries    [Q][D]
 *   mask       nullable [HW] uint8: only pixels with mask != 0 are candidates
 *   best_idx   [Q] int64 flat index u + W*v of the first minimum (np.argmin order); -1 if the mask is empty
 *   best_dist  [Q] the distance at best_idx
 *   norm_diffs nullable [Q][HW]: the full distance images
 *   workspace  dcn_find_best_match_workspace(Q) bytes
 * ===================================================================================================== */
/* Match statistics of evaluation.py:1046-1100 for q query matches in ONE pass over the descriptor image res [hw][d]
 * (row length w):  queries[i] = res_a[uv_a_i], gt_idx[i] = flat index of the ground-truth match in image b.
 *   best_idx / best_dist  [2][q]: argmin / min of d over the image, and of d + (1 - mask) * 1e6 (mask NULL: same as the image)
 *   count                 [2][q]: pixels with d < ||queries[i] - res[gt_idx[i]]|| (image / masked)
 *   dist_sum              [2][q]: sum of the pixel distances of those pixels to the ground-truth pixel: each fp32 distance
 *                                 rounded to 2^-20 pixel and summed as an integer, so the sum does not depend on the order of
 *                                 the adds (the same bits from run to run); returned as float((double)sum / 2^20)
 *   gt_dist               [q]:    that ground-truth descriptor distance
 *   workspace             dcn_match_statistics_workspace(q) bytes: best keys [2][q] uint64 | distance sums [2][q] uint64 */
size_t dcn_match_statistics_workspace(int q);
int dcn_match_statistics(const float* res, int64_t hw, int w, int d, const float* queries, const int64_t* gt_idx, int q,
                         const unsigned char* mask, int64_t* best_idx, float* best_dist, int32_t* count, float* dist_sum,
                         float* gt_dist, void* workspace, void* stream);

int dcn_find_best_match(const float* res, int64_t hw, int d, const float* queries, int q, const unsigned char* mask,
                        int64_t* best_idx, float* best_dist, float* norm_diffs, void* workspace, void* stream);
size_t dcn_find_best_match_workspace(int q);

/* =====================================================================================================
 * 5. Pair generation on the device -- replaces, for device-resident depth images,
 *    dense_correspondence/correspondence_tools/correspondence_finder.py
 *      batch_find_pixel_correspondences (:409-619, from the point where the candidate pixels are chosen, :486)
 *      create_non_correspondences       (:276-405, sampling part; its perturbation step is inert in the reference)
 *    Depth images: [h][w] uint16 millimetres.  K, K_inv: row-major 3x3 fp32; pose_a, pose_b_inv: row-major 4x4 fp32
 *    camera-to-world of image a and world-to-camera of image b (HOST pointers: they travel as kernel arguments).
 *    Outputs keep candidate order; *out_count (device scalar) matches were written to the front of the out_* arrays.
 * ===================================================================================================== */
size_t dcn_find_correspondences_workspace(int64_t n);
int dcn_find_correspondences(const uint16_t* depth_a, const uint16_t* depth_b, int h, int w, const float* K,
                             const float* K_inv, const float* pose_a, const float* pose_b_inv, const int64_t* cand_u,
                             const int64_t* cand_v, int64_t n, int64_t* out_ua, int64_t* out_va, float* out_ub,
                             float* out_vb, int64_t* out_count, void* workspace, void* stream);
/* list[0 .. *count) = flat indices of the non-zero mask pixels, increasing (torch.nonzero order) */
size_t dcn_mask_nonzero_workspace(int64_t hw);
int dcn_mask_nonzero(const float* mask, int64_t hw, int64_t* list, int64_t* count, void* workspace, void* stream);
/* list == NULL: (u, v) = (floor(rand[i] * w), floor(rand[n + i] * h))            (pytorch_rand_select_pixel, :29-34)
 * otherwise   : p = list[floor(rand[i] * *count)], (u, v) = (p % w, p / w)       (:319-324).  u, v: float [n]. */
int dcn_sample_pixels(const float* rand, int64_t n, int w, int h, const int64_t* list, const int64_t* count, float* u,
                      float* v, void* stream);

/* =====================================================================================================
 * 6. Optimizer step -- replaces `optimizer.step()` (dense_correspondence/training/training.py:346) of the
 *    torch.optim.Adam built at training.py:133-145 (lr 1e-4, weight_decay 1e-4 from training.yaml:3,6; default betas,
 *    eps; no amsgrad): one pass over n dense fp32 tensors, ceil(n / 80) launches.
 *      g' = g + weight_decay * p;  m = m + (1 - beta1)(g' - m);  v = beta2 v + (1 - beta2) g'^2
 *      p  = p - lr / (1 - beta1^step) * m / (sqrt(v) / sqrt(1 - beta2^step) + eps)
 *    param / grad / exp_avg / exp_avg_sq: HOST arrays of n device pointers (element i of each addresses numel[i] floats in
 *    the same memory order); they travel as kernel arguments.  step >= 1 is the count INCLUDING this update.
 * ===================================================================================================== */
int dcn_adam_step(int n, void* const* param, const void* const* grad, void* const* exp_avg, void* const* exp_avg_sq,
                  const int64_t* numel, double lr, double beta1, double beta2, double eps, double weight_decay,
                  int64_t step, void* stream);

/* =====================================================================================================
 * 7. Training-image augmentation -- replaces, for device-resident images, the data augmentation of every within-scene
 *    sample (dense_correspondence/dataset/spartan_dataset_masked.py:667-680) and the ToTensor + Normalize after it
 *    (:297-304), i.e. dense_correspondence/correspondence_tools/correspondence_augmentation.py
 *      random_domain_randomize_background / domain_randomize_background / get_random_image (:86-215)
 *      random_image_and_indices_mutation / flip_vertical / flip_horizontal (:19-83)
 *    Images: uint8 [h][w][3]; masks: uint8 [h][w] with values 0 / 1 (other values follow the reference's uint8 formula
 *    rgb*m + (1-m)*bg, which is outside the contract).  One record of DCN_AUG_PARAM_WORDS int32 per image:
 *      [0] flags (DCN_AUG_*)   [1..3] rgb1 (solid colour / gradient start, 0..255)   [4..6] rgb2 (gradient end)
 *      [7] 0   [8..9] 64-bit noise seed (low word, high word)   [10..15] 0
 *    Randomization (when DCN_AUG_RANDOMIZE) runs on the unrotated image: the gradient position and the noise index of an
 *    output pixel are those of its source pixel.  Gradient: uint8(rgb2*p + rgb1*(1.0-p)) in float64, p = linspace(0, 1, n)
 *    along rows (DCN_AUG_VERTICAL) or columns.  Noise (DCN_AUG_NOISE): bg + d mod 256 with d = n1 - n2 mod 256, n1, n2
 *    uniform on 0..49, read from `noise` ([images][h][w][3]) or, when noise == NULL, from a counter-based hash of
 *    (seed, image, source pixel, channel).
 * ===================================================================================================== */
#define DCN_AUG_PARAM_WORDS 16
#define DCN_AUG_FLIP_V 1
#define DCN_AUG_FLIP_H 2
#define DCN_AUG_RANDOMIZE 4
#define DCN_AUG_GRADIENT 8
#define DCN_AUG_VERTICAL 16
#define DCN_AUG_NOISE 32
#define DCN_UV_INT64 0
#define DCN_UV_FLOAT32 1
/* n image pairs (rgb_b == mask_b == NULL: n images of side a only) in ONE launch.  params: device [sides * n] records, side
 * a's first; noise: device [sides * n][h][w][3] or NULL; mean, std: HOST float [3].  Outputs (each may be NULL):
 *   net_*      float [n][3][h][w] = (float(x) / 255 - mean_c) / std_c, IEEE division (torch ToTensor + Normalize)
 *   rgb_out_*  uint8 [n][h][w][3] the augmented image          mask_out_*  float [n][h][w] the (rotated) mask as 0.0 / 1.0 */
int dcn_augment_images(int n, int h, int w, const uint8_t* rgb_a, const uint8_t* rgb_b, const uint8_t* mask_a,
                       const uint8_t* mask_b, const int32_t* params, const uint8_t* noise, const float* mean,
                       const float* std, float* net_a, float* net_b, uint8_t* rgb_out_a, uint8_t* rgb_out_b,
                       float* mask_out_a, float* mask_out_b, void* stream);
/* out[p][y][x] = in[p][flip_v ? h-1-y : y][flip_h ? w-1-x : x] for `planes` planes of pixels of 1 .. 64 bytes; out != in */
int dcn_flip_planes(const void* in, void* out, int64_t planes, int h, int w, int bytes_per_pixel, int flip_v, int flip_h,
                    void* stream);
/* u -> (w-1) - u (DCN_AUG_FLIP_H), v -> (h-1) - v (DCN_AUG_FLIP_V) in the list's type (DCN_UV_*), out may equal in.
 * offsets: device int64 [n_images + 1] (entries [offsets[b], offsets[b+1]) belong to image b; others are copied) or NULL
 * (n_images == 1); the flags come from params[b * DCN_AUG_PARAM_WORDS] (device records) or, params == NULL, `flags`. */
int dcn_flip_uv(int uv_dtype, const void* u_in, const void* v_in, void* u_out, void* v_out, int64_t count, int n_images,
                const int64_t* offsets, const int32_t* params, int flags, int h, int w, void* stream);

/* =====================================================================================================
 * 8. Synthetic multi-object samples -- replaces, for device-resident images, the merge step of the SYNTHETIC_MULTI_OBJECT
 *    sample (dense_correspondence/dataset/spartan_dataset_masked.py:890-960) and the ToTensor + Normalize after it, i.e.
 *    dense_correspondence/correspondence_tools/correspondence_augmentation.py
 *      merge_images_with_occlusions (:217-297), prune_matches_if_occluded (:300-335), merge_matches (:337-345)
 *    Images: uint8 [n][h][w][3]; masks: uint8 [n][h][w] with values 0 / 1 (other values follow the reference's uint8
 *    formulas, outside the contract).  Object a's and object b's images of frame 1 and frame 2.  One foreground record per
 *    (sample, frame): foreground [n][2] int32, DCN_MERGE_FG_A or DCN_MERGE_FG_B (the reference: random.random() < 0.5 puts
 *    object b in front).
 * ===================================================================================================== */
#define DCN_MERGE_FG_A 0
#define DCN_MERGE_FG_B 1
#define DCN_MERGE_DROP_EMPTY 1      /* dcn_merge_prune flag: a sample whose a or b list ends up empty loses all its entries */
#define DCN_MERGE_BAD_INDEX 1       /* status bit: an entry's (u, v) was outside the image (the entry is dropped) */
#define DCN_MERGE_BAD_OFFSETS 2     /* status bit: offsets_a / offsets_b not increasing within [0, count] (every sample empty) */
/* n samples x `frames` (1 or 2; frame-2 pointers NULL for 1) in ONE launch.  Frame f of sample s: the foreground object's
 * image over the other's, fg*m + bg*(1-m) per channel in uint8 arithmetic, and the merged mask clip(mask_a + mask_b, 0, 1)
 * of their uint8 sum.  mean, std: HOST float [3].  Outputs (each may be NULL):
 *   net_f   float [n][3][h][w] = (float(x) / 255 - mean_c) / std_c of the merged image, IEEE division (as dcn_augment_images)
 *   mask_f  float [n][h][w] the merged mask as 0.0 / 1.0          rgb_f  uint8 [n][h][w][3] the merged image */
int dcn_merge_images(int n, int frames, int h, int w, const int32_t* foreground, const uint8_t* rgb_a1, const uint8_t* rgb_b1,
                     const uint8_t* rgb_a2, const uint8_t* rgb_b2, const uint8_t* mask_a1, const uint8_t* mask_b1,
                     const uint8_t* mask_a2, const uint8_t* mask_b2, const float* mean, const float* std, float* net_1,
                     float* net_2, float* mask_1, float* mask_2, uint8_t* rgb_1, uint8_t* rgb_2, void* stream);
/* Occlusion prune and concatenation over n samples, two launches, no host synchronisation.  Object a's match list of sample
 * s is entries [offsets_a[s], offsets_a[s+1]) of u_a1 / v_a1 (its pixels in frame 1) and u_a2 / v_a2 (frame 2), int64;
 * object b's likewise (offsets_* may be NULL when count_* == 0).  Entry i of object a is kept unless, in frame 1 or frame 2,
 * foreground puts b in front and mask_b<f>[s][v_a<f>[i]][u_a<f>[i]] != 0 (the reference prunes frame 1's background pair by
 * its first list, then frame 2's swapped pair); the same with a and b exchanged.  A NULL mask occludes nothing, and the
 * entries' (u, v) of a frame are range-checked exactly when the other object's mask of that frame is given: an entry outside
 * [0, w) x [0, h) sets DCN_MERGE_BAD_INDEX in *status and is dropped, never read out of bounds.  Outputs, capacity
 * count_a + count_b each: u_1, v_1, u_2, v_2 = for every sample in order, a's kept entries then b's (merge_matches(uv_a1,
 * uv_b1) / (uv_a2, uv_b2)); entries [offsets[n], count_a + count_b) are -1.  offsets: int64 [n + 1], sample s at
 * [offsets[s], offsets[s+1]); empty: uint8 [n], 1 when a's or b's kept list is empty (with DCN_MERGE_DROP_EMPTY such a
 * sample also contributes no entry, as the reference returns an empty sample); status: int32 [1], DCN_MERGE_BAD_* bits
 * (written, not accumulated).  workspace: device, dcn_merge_prune_workspace(n, count_a, count_b) bytes. */
size_t dcn_merge_prune_workspace(int n, int64_t count_a, int64_t count_b);
int dcn_merge_prune(int n, int h, int w, const int32_t* foreground, const uint8_t* mask_a1, const uint8_t* mask_b1,
                    const uint8_t* mask_a2, const uint8_t* mask_b2, const int64_t* u_a1, const int64_t* v_a1,
                    const int64_t* u_a2, const int64_t* v_a2, const int64_t* offsets_a, int64_t count_a, const int64_t* u_b1,
                    const int64_t* v_b1, const int64_t* u_b2, const int64_t* v_b2, const int64_t* offsets_b, int64_t count_b,
                    int flags, int64_t* u_1, int64_t* v_1, int64_t* u_2, int64_t* v_2, int64_t* offsets, uint8_t* empty,
                    int32_t* status, void* workspace, void* stream);

/* =====================================================================================================
 * 9. Training samples -- replaces, for device-resident frames, the sample recipe of the reference's loader
 *    (dense_correspondence/dataset/spartan_dataset_masked.py): get_within_scene_data (:577-839, SINGLE_OBJECT_WITHIN_SCENE
 *    and MULTI_OBJECT), get_across_scene_data (:1056-1141, SINGLE_OBJECT_ACROSS_SCENE and DIFFERENT_OBJECT), and the
 *    non-match / blind-set steps of any match lists (complete_samples, e.g. after dcn_merge_prune).
 *    n pairs of [h][w] frames: depth uint16 millimetres, masks uint8 with values 0 / 1 (the blind set is computed as
 *    (mask != 0) != matched and 1 - mask b as mask == 0: other values are outside the contract), one 180-degree rotation
 *    record per image, aug_params [2n][DCN_AUG_PARAM_WORDS] (section 7; a's records first; only the flip bits are read;
 *    NULL: no rotation).  cams: device float [n][DCN_SAMPLE_CAM_FLOATS] = K (3x3), K^-1, pose a (4x4 camera-to-world),
 *    pose b^-1 (world-to-camera), row-major, fp32.  Outputs, all on the device, no host synchronisation:
 *      idx_a, idx_b  int64 [capacity], 16-byte aligned: for every pair p in order its lists t = 0 match, 1 masked, 2 background, 3 blind at
 *                    [offsets[4p+t], offsets[4p+t+1]) as flattened pixels v * w + u; entries [offsets[4n], capacity) are -1
 *      offsets int64 [4n + 1]; empty uint8 [n]; type int32 [n] = data_type, or -1 for an empty pair (its lists are empty,
 *      as return_empty_data); status int32 [1], DCN_SAMPLE_BAD_* bits (written, not accumulated).
 *    Within-scene recipe per pair: A = attempts candidates, drawn from mask a's pixels (list[floor(r * count)], flag
 *    DCN_SAMPLE_ONLY_OFF_MASK; an empty mask a gives an empty pair) or uniformly ((floor(r0 * w), floor(r1 * h))); the
 *    reprojection / occlusion test of dcn_find_correspondences; the M survivors in candidate order, rotated by the pair's
 *    records (b's float coordinates as (w-1) - u, then truncated like `.long()`).  M == 0: empty pair.  Then, on the
 *    rotated masks: masked = match a repeated k_masked times in a row, b from mask b's pixels (uniform over the image if mask
 *    b is empty); background likewise with k_background from 1 - mask b (DCN_SAMPLE_MASK_INV) or uniform; blind = the
 *    pixels where (mask a != 0) != matched, in order, b from mask b's pixels -- empty when there are none or mask b is empty.
 *    Across-scene recipe: num_samples pixels of mask a's and of mask b's list (unrotated), each then rotated by its image's
 *    record, into the blind slot; the other lists are empty; the pair is empty when either mask is.
 *    Random numbers: seeds != NULL: seeds [n] int64 per pair; uniform k of site s is a counter-based hash of
 *    (seed, s, k) on torch.rand's grid (multiples of 2^-24).  seeds == NULL (replay): rand float32 holds the caller's values,
 *    site s of pair p at rand[rand_offsets[s * (n + 1) + p] ...  rand_offsets[s * (n + 1) + p + 1]) -- the reference's own
 *    torch.rand streams.  Sites (DCN_SAMPLE_SITE_*) and the values each reads: CAND A (from mask a) or 2A (uniform: all u
 *    values, then all v values, as torch.rand(2, A)); MASKED k_masked * M, or 2 k_masked * M when uniform; BACKGROUND
 *    likewise with k_background; BLIND nb (the blind set's size); ACROSS_A, ACROSS_B num_samples each.  A stream shorter
 *    than its site needs reads 0 there and raises DCN_SAMPLE_BAD_DRAWS.
 * ===================================================================================================== */
#define DCN_SAMPLE_CAM_FLOATS 50
#define DCN_SAMPLE_SITES 6
#define DCN_SAMPLE_SITE_CAND 0
#define DCN_SAMPLE_SITE_MASKED 1
#define DCN_SAMPLE_SITE_BACKGROUND 2
#define DCN_SAMPLE_SITE_BLIND 3
#define DCN_SAMPLE_SITE_ACROSS_A 4
#define DCN_SAMPLE_SITE_ACROSS_B 5
#define DCN_SAMPLE_ONLY_OFF_MASK 1  /* flag: candidates from mask a's pixels (sample_matches_only_off_mask) */
#define DCN_SAMPLE_MASK_INV 2       /* flag: background non-matches from 1 - mask b (use_image_b_mask_inv) */
#define DCN_SAMPLE_BAD_INDEX 1      /* status: a complete_samples entry outside the image (kept, as pixel 0) */
#define DCN_SAMPLE_BAD_DRAWS 2      /* status: a replay stream shorter than its site needs */
#define DCN_SAMPLE_BAD_OFFSETS 4    /* status: complete_samples offsets not increasing within [0, count] (pair empty) */
/* device workspace bytes: within-scene (attempts, attempts); complete_samples (0, count); across-scene (0, 0) */
size_t dcn_sample_workspace(int n, int h, int w, int64_t attempts, int64_t match_slots);
/* capacity = n * (attempts * (1 + k_masked + k_background) + h * w); 1 <= n <= 1024 */
int dcn_within_scene_samples(int n, int h, int w, const uint16_t* depth_a, const uint16_t* depth_b, const uint8_t* mask_a,
                             const uint8_t* mask_b, const float* cams, int64_t attempts, int k_masked, int k_background,
                             int flags, const int32_t* aug_params, const int64_t* seeds, const float* rand,
                             const int64_t* rand_offsets, int data_type, int64_t* idx_a, int64_t* idx_b, int64_t capacity,
                             int64_t* offsets, uint8_t* empty, int32_t* type, int32_t* status, void* workspace, void* stream);
/* Matches found elsewhere: pair p's are entries [list_offsets[p], list_offsets[p+1]) of u_a / v_a (int64) and u_b / v_b
 * (DCN_UV_INT64 or DCN_UV_FLOAT32, truncated like `.long()`), pixels of the frames BEFORE the aug_params rotation (NULL
 * aug_params: the lists and masks are final).  A pair without matches is empty.  Flags: DCN_SAMPLE_MASK_INV only.
 * capacity = count * (1 + k_masked + k_background) + n * h * w */
int dcn_complete_samples(int n, int h, int w, const int64_t* u_a, const int64_t* v_a, const void* u_b, const void* v_b,
                         int uv_b_dtype, const int64_t* list_offsets, int64_t count, const uint8_t* mask_a,
                         const uint8_t* mask_b, int k_masked, int k_background, int flags, const int32_t* aug_params,
                         const int64_t* seeds, const float* rand, const int64_t* rand_offsets, int data_type, int64_t* idx_a,
                         int64_t* idx_b, int64_t capacity, int64_t* offsets, uint8_t* empty, int32_t* type, int32_t* status,
                         void* workspace, void* stream);
/* capacity = n * num_samples */
int dcn_across_scene_samples(int n, int h, int w, const uint8_t* mask_a, const uint8_t* mask_b, int64_t num_samples,
                             const int32_t* aug_params, const int64_t* seeds, const float* rand, const int64_t* rand_offsets,
                             int data_type, int64_t* idx_a, int64_t* idx_b, int64_t capacity, int64_t* offsets, uint8_t* empty,
                             int32_t* type, int32_t* status, void* workspace, void* stream);

/* Joins the outputs of `groups` (<= DCN_CONCAT_MAX_GROUPS) calls above -- e.g. one per data type -- into one batch of
 * sum n[g] <= 1024 pairs, in the order given: host arrays [groups] of the group sizes n, of the DEVICE pointers idx_a, idx_b,
 * offsets ([4 n[g] + 1]), status_in (the array or single entries may be NULL) and of the groups' capacities.  Outputs as
 * above: idx_a_out / idx_b_out int64 [capacity], 16-byte aligned, pair p's list t at [offsets_out[4p+t], offsets_out[4p+t+1]),
 * -1 from offsets_out[4 * sum n] on (capacity >= the sum of the groups' capacities always holds them); offsets_out
 * [4 * sum n + 1]; status [1] = the groups' words OR-ed, | DCN_SAMPLE_BAD_OFFSETS for a group whose offsets do not increase
 * from 0 within its capacity (its pairs keep their slots with empty lists) or when the joined lists exceed `capacity`.  Two
 * launches, no host synchronisation.  type / empty and the images are per-pair arrays: the caller concatenates them. */
#define DCN_CONCAT_MAX_GROUPS 8
int dcn_concat_samples(int groups, const int* n, const int64_t* const* idx_a, const int64_t* const* idx_b,
                       const int64_t* const* offsets, const int64_t* capacity_in, const int32_t* const* status_in,
                       int64_t* idx_a_out, int64_t* idx_b_out, int64_t capacity, int64_t* offsets_out, int32_t* status,
                       void* stream);

/* =====================================================================================================
 * 9a. SYNTHETIC_MULTI_OBJECT training samples -- replaces, for device-resident frames, the whole of
 *     get_synthetic_multi_object_within_scene_data (dense_correspondence/dataset/spartan_dataset_masked.py:890-1053): two
 *     within-scene match searches (object a: frames a1 -> a2, object b: b1 -> b2), the occlusion prune and concatenation of
 *     section 8, the non-matches of section 9 on the merged frame-2 mask, and the merged images.  One chain on the caller's
 *     stream, no host synchronisation; the per-object non-matches of a composition of the section 9 entries are never built.
 *     n samples (1 <= n <= 1024) of [h][w] frames in the slot order of dcn_gather_frames(k = 4) -- a1, a2, b1, b2:
 *       depth uint16 [4][n][h][w] millimetres; mask uint8 [4][n][h][w], 0 / 1; rgb uint8 [4][n][h][w][3], or NULL: no images
 *       are written (net_* / mask_* must then be NULL); cams float [2][n][DCN_SAMPLE_CAM_FLOATS], row 0 for a1 -> a2, row 1
 *       for b1 -> b2; foreground int32 [n][2], the records of section 8; empty_in uint8 [n] or NULL: a sample marked here
 *       (its frames could not be chosen) reads no random number and comes out empty; mean, std: HOST float [3] (with rgb).
 *     Recipe per sample: (:906-927) the match search of dcn_within_scene_samples for object a and for object b on the
 *     unaugmented frames -- `attempts` candidates each, from mask a1 / b1 (DCN_SAMPLE_ONLY_OFF_MASK) or uniform, survivors in
 *     candidate order, frame-2 coordinates truncated like `.long()`; this type has no rotation and no background
 *     randomization.  (:929-955) the rule of dcn_merge_prune with DCN_MERGE_DROP_EMPTY: an entry of the object behind is
 *     dropped when its frame-1 or its frame-2 pixel lies inside the front object's mask of that frame; a's kept entries, then
 *     b's.  The sample is empty (type -1, no entries) when a's or b's search finds nothing or a's or b's list is pruned to
 *     nothing.  (:957-1000) on the merged frame-2 mask clip(mask a2 + mask b2, 0, 1): k_masked non-matches per match from its
 *     pixels (uniform over the image when it is empty), k_background from its inverse (DCN_SAMPLE_MASK_INV) or uniform, in
 *     the layout and with the `pick` rule of dcn_complete_samples.  The blind list is EMPTY (:1053 returns empty tensors).
 *     Images (rgb != NULL): net_1, net_2, mask_1, mask_2 exactly as dcn_merge_images writes them (each may be NULL).
 *     Outputs as in section 9: idx_a / idx_b int64 [capacity] (16-byte aligned, -1 from offsets[4n] on), offsets [4n + 1],
 *     empty [n], type [n] = DCN_SYNTHETIC_DATA_TYPE or -1, status [1] = DCN_SAMPLE_BAD_* bits (written, not accumulated).
 *       capacity = n * 2 * attempts * (1 + k_masked + k_background)
 *     Random numbers: seeds [n] (the hash of (seed, site, k) of section 9) or, seeds == NULL, the replay streams rand /
 *     rand_offsets[s * (n + 1) + p] over THIS entry's DCN_SYNTHETIC_SITES sites: CAND_A and CAND_B read A values (from the
 *     mask) or 2A (uniform: all u, then all v); MASKED k_masked * M or 2 k_masked * M when uniform (M = the merged match count);
 *     BACKGROUND likewise.  A stream shorter than its site needs reads 0 there and raises DCN_SAMPLE_BAD_DRAWS -- except
 *     CAND_B of a sample whose object a search found nothing: the reference never searches b's scene then, so the stream may
 *     be absent.  workspace: device, dcn_synthetic_workspace(n, h, w, attempts) bytes (0: sizes outside the contract).
 * ===================================================================================================== */
#define DCN_SYNTHETIC_DATA_TYPE 4
#define DCN_SYNTHETIC_SITES 4
#define DCN_SYNTHETIC_SITE_CAND_A 0
#define DCN_SYNTHETIC_SITE_CAND_B 1
#define DCN_SYNTHETIC_SITE_MASKED 2
#define DCN_SYNTHETIC_SITE_BACKGROUND 3
size_t dcn_synthetic_workspace(int n, int h, int w, int64_t attempts);
int dcn_synthetic_samples(int n, int h, int w, const uint16_t* depth, const uint8_t* mask, const uint8_t* rgb,
                          const float* cams, int64_t attempts, int k_masked, int k_background, int flags,
                          const int32_t* foreground, const uint8_t* empty_in, const int64_t* seeds, const float* rand,
                          const int64_t* rand_offsets, const float* mean, const float* std, float* net_1, float* net_2,
                          float* mask_1, float* mask_2, int64_t* idx_a, int64_t* idx_b, int64_t capacity, int64_t* offsets,
                          uint8_t* empty, int32_t* type, int32_t* status, void* workspace, void* stream);

/* =====================================================================================================
 * 10. Frame store -- replaces, for frames kept in device memory, the frame choice of the reference's loader
 *     (dense_correspondence/dataset/spartan_dataset_masked.py: the five type wrappers :543-575, :860-905 and the helpers
 *     get_random_image_index :408-420, get_random_single_object_scene_name :442-451, get_different_scene_for_object
 *     :453-474, get_two_different_object_ids :476-494, get_random_multi_object_scene_name :496-502;
 *     dense_correspondence_dataset_masked.py get_img_idx_with_different_pose :260-287) and the decode / stack / upload of
 *     the chosen frames.
 *     Store tables (struct dcn_frame_store, all DEVICE pointers, passed to the entry points as a HOST pointer to the struct):
 *       rgb uint8 [F][h][w][3]; depth uint16 [F][h][w] millimetres; mask uint8 [F][h][w] (0 / 1)
 *       scene_first_frame int32 [S + 1]: scene s owns frames [scene_first_frame[s], scene_first_frame[s+1]) (>= 1 each),
 *                  in the order of the reference's pose_data keys (a position drawn by random.choice IS the frame's offset)
 *       scene_object int32 [S]: the scene's object, or -1 for a multi-object scene
 *       object_scene_offsets int32 [O + 1], object_scenes int32 [...]: object o's scene list, in the reference's order
 *       multi_scenes int32 [M]: the multi-object scenes, in the reference's order
 *       scene_cams float [S][18]: K (3x3) then K^-1, row-major, fp32 of the float64 K and of its float64 inverse
 *       poses double [F][16]: camera-to-world, row-major
 *     No entry point needs a workspace.
 * ===================================================================================================== */
struct dcn_frame_store {
    int64_t num_frames;
    int32_t num_scenes, num_objects, num_multi, h, w;
    const uint8_t* rgb;
    const uint16_t* depth;
    const uint8_t* mask;
    const int32_t* scene_first_frame;
    const int32_t* scene_object;
    const int32_t* object_scene_offsets;
    const int32_t* object_scenes;
    const int32_t* multi_scenes;
    const float* scene_cams;
    const double* poses;
};
#define DCN_FRAME_CAM_FLOATS 18
#define DCN_FRAME_SLOTS 4           /* frames [n][4]: a, b (a1, a2, b1, b2 for SYNTHETIC_MULTI_OBJECT; -1 past 2 otherwise) */
/* Replay words, per pair: draws int32 [n][DCN_FRAME_DRAW_HEADER + 2 * num_attempts], each the POSITION that the reference's
 * random.choice / np.random.choice returned in its list (get_random_image_index: the second of its two random.choice calls) */
#define DCN_FRAME_DRAW_OBJECT_A 0   /* random.choice over the objects; np.random.choice(..., 2)[0] (DIFFERENT_OBJECT, SYNTHETIC) */
#define DCN_FRAME_DRAW_OBJECT_B 1   /* np.random.choice(..., 2)[1] over the objects (DIFFERENT_OBJECT, SYNTHETIC) */
#define DCN_FRAME_DRAW_SCENE_A 2    /* random.choice over object a's scenes (MULTI_OBJECT: over the multi-object scenes) */
#define DCN_FRAME_DRAW_SCENE_B 3    /* random.choice over object b's scenes; SINGLE_OBJECT_ACROSS_SCENE: np.random.choice[0] */
#define DCN_FRAME_DRAW_SCENE_B2 4   /* SINGLE_OBJECT_ACROSS_SCENE: np.random.choice(..., 2)[1] over the object's scenes */
#define DCN_FRAME_DRAW_FRAME_A 5    /* image a (a1) in scene a */
#define DCN_FRAME_DRAW_FRAME_B 6    /* image b in scene b (across types); image b1 (SYNTHETIC) */
#define DCN_FRAME_DRAW_HEADER 8     /* then num_attempts words: image b (a2) candidates in scene a; then num_attempts: b2's */
#define DCN_FRAME_BAD_INDEX 1       /* status: a table entry or a frame index out of range (that frame reads as zeros) */
#define DCN_FRAME_BAD_DRAWS 2       /* status: a replay position outside its list, or np.random.choice's two positions equal */
#define DCN_FRAME_NO_CANDIDATES 4   /* status: the type has no eligible object or scene (no multi-object scene, an object with
                                     * one scene for SINGLE_OBJECT_ACROSS_SCENE, fewer than two objects); the pair is empty */
/* One launch for n pairs of one data_type (SpartanDatasetDataType numbering, as section 9: 0 SINGLE_OBJECT_WITHIN_SCENE,
 * 1 SINGLE_OBJECT_ACROSS_SCENE, 2 DIFFERENT_OBJECT, 3 MULTI_OBJECT, 4 SYNTHETIC_MULTI_OBJECT), one wavefront per pair.
 * Image b of a within-scene choice is get_img_idx_with_different_pose(scene, pose a, threshold, angle_threshold,
 * num_attempts): the first of num_attempts uniform frames of the scene whose translation is more than `threshold` from pose
 * a's (float64, sqrt of the sum of squares) or whose angle 2 acos(clamp((tr(R_a^T R_b) - 1) / 2, -1, 1)) -- the reference's
 * 2 arccos(2 <q_a, q_b>^2 - 1), in radians -- exceeds angle_threshold (never, when angle_threshold >= 2 pi).  No such frame:
 * the pair is empty and its missing frame b is frame a (a2 := a1, b2 := b1 for SYNTHETIC).  Random numbers: seeds != NULL: seeds
 * [n] int64, word k of pair p is a counter-based hash of (seed, k) mapped onto the list's length (np.random.choice's two
 * distinct positions: the second over the other n - 1); seeds == NULL: draws (replay, layout above).
 * Outputs: frames int32 [n][DCN_FRAME_SLOTS] global frame indices; empty uint8 [n]; scenes int32 [n][2] (scene of a / a1,
 * of b / b1); objects int32 [n][2] (-1: multi-object); status int32 [1], DCN_FRAME_* bits (written, not accumulated).
 * 1 <= n <= 65536, 1 <= num_attempts <= 4096. */
int dcn_select_frames(int n, int data_type, const struct dcn_frame_store* store, int num_attempts, double threshold,
                      double angle_threshold, const int64_t* seeds, const int32_t* draws, int32_t* frames, uint8_t* empty,
                      int32_t* scenes, int32_t* objects, int32_t* status, void* stream);
/* One launch: copies slot k (0 <= k < frames_per_pair, 2 or 4) of every pair, frame frames[p][k], to rgb [k][n][h][w][3],
 * depth [k][n][h][w], mask [k][n][h][w] (any of the three may be NULL), 16-byte loads and stores where the planes allow.
 * An empty pair (empty may be NULL) gets zero depth in all its slots, so no match survives the reprojection test of section 9.
 * cams (may be NULL): float [frames_per_pair / 2][n][DCN_SAMPLE_CAM_FLOATS], row j of pair p for slots (2j, 2j+1): the
 * scene_cams row of slot 2j's scene, pose of slot 2j as fp32, and the rigid inverse of slot 2j+1's pose computed in float64
 * (R^T; -(R^T t) summed left to right, no contraction) then rounded to fp32 -- the rows of section 9's cams.  A frame index
 * outside [0, num_frames) ORs DCN_FRAME_BAD_INDEX into *status (accumulated: the selection's word) and reads as zeros. */
int dcn_gather_frames(int n, int frames_per_pair, const struct dcn_frame_store* store, const int32_t* frames,
                      const uint8_t* empty, uint8_t* rgb, uint16_t* depth, uint8_t* mask, float* cams, int32_t* status,
                      void* stream);

/* =====================================================================================================
 * 11. Evaluation on frame-store image pairs -- replaces, for device-resident frames and descriptor images, what
 *     DenseCorrespondenceEvaluation.evaluate_network (dense_correspondence/evaluation/evaluation.py:475-527) runs per image
 *     pair: the match search and subsample of single_same_scene_image_pair_quantitative_analysis (:908-921) and
 *     compute_descriptor_match_statistics (:1045-1175) for every chosen match, for ALL pairs in one call each.
 *
 * 11a. Matches: per pair batch_find_pixel_correspondences(depth_a, pose_a, depth_b, pose_b, img_a_mask=mask_a): `attempts`
 *     candidates from mask a's pixels and the reprojection test, exactly the first stages of dcn_within_scene_samples
 *     (section 9: same device functions, cams, seeds / rand / rand_offsets replay of site DCN_SAMPLE_SITE_CAND; the other
 *     sites' offsets are not read), kept as (u_a, v_a) int64 and the FLOAT projection (u_b, v_b).  Then the subsample
 *     random.sample(range(total), min(num_matches, total)) (:919-921) as a device stage: pair p contributes
 *     k_p = min(num_matches, total_p) rows, row j is survivor match_order[p][j] (replay: int32 [n][num_matches], -1 padded,
 *     the reference's match_list; a position outside [0, total_p) reads 0 and raises DCN_SAMPLE_BAD_DRAWS), or, with
 *     match_order == NULL, the survivor of rank j when the total_p survivors are ordered by a hash of (order_seeds[p],
 *     survivor) -- a uniform random order, its first k_p entries.
 *     Outputs: rows [offsets[p], offsets[p+1]) of u_a, v_a (int64), u_b, v_b (float), each [n * min(num_matches, attempts)],
 *     -1 / 0 from offsets[n] on; offsets int64 [n + 1]; totals int32 [n]; status int32 [1] (DCN_SAMPLE_* bits, written).
 *     A pair with no survivor (or an empty mask a) has no rows.  1 <= n <= 1024, 1 <= attempts <= 4096.
 *
 * 11b. Statistics: P pairs of [h][w] images; res_a, res_b float [P][hw][d] descriptor images; mask_b uint8 [P][hw] (non-zero:
 *     on the object); depth_a, depth_b uint16 [P][hw] millimetres; cams [P][DCN_SAMPLE_CAM_FLOATS] (section 9's rows);
 *     the query rows of pair p at [offsets[p], offsets[p+1]) of u_a, v_a (int64), u_b, v_b (float, as 11a returns them);
 *     offsets int64 [P + 1] on the device.  max_rows: the rows' capacity (every output's row dimension); max_pair_rows: a
 *     bound on one pair's rows (a longer list is cut there and raises DCN_EVAL_BAD_OFFSETS).  offsets must increase from >= 0
 *     to <= max_rows over all pairs: one violation anywhere raises DCN_EVAL_BAD_OFFSETS and every pair is then empty.
 *     Ground-truth pixel: clip_pixel_to_image_size_and_round (:604-607), min(int(round(x)), size - 1) with Python 2's round
 *     (half away from zero), and not below 0.
 *     Stage A, one launch over (pixel tile, pair): dcn_match_statistics' scheme (section 4) with the query descriptors
 *     res_a[p][v_a * w + u_a] gathered by the kernel, and the count of mask b's non-zero pixels.  Stage B, one work-item per
 *     row, writes
 *       columns double [DCN_EVAL_COLUMNS][max_rows] (DCN_EVAL_COL_*: the DCNEvaluationPandaTemplate columns, :37-63)
 *       is_valid uint8 [2][max_rows] (is_valid, is_valid_masked); pred_uv int32 [4][max_rows] (u, v of the best match over the
 *       image; u, v over the mask); closer int32 [2][max_rows] (pixels closer than the ground truth: image, masked);
 *       row_pair int32 [max_rows]; mask_pixels int32 [P]; status int32 [1] (DCN_EVAL_* bits, written).
 *     Rows from offsets[P] on: NaN columns, zero flags / counts, -1 in pred_uv and row_pair.
 *     Depth / 3D columns (:1102-1135, :1148-1164) in float64: depth / 1000.0, valid when 0 < d < 10; position = pose *
 *     (z * K^-1 * (u, v, 1)) with K^-1 the float64 inverse of the row's fp32 K, pose a the row's fp32 pose a, and pose b the
 *     float64 rigid inverse (R^T, -(R^T t)) of the row's fp32 pose b^-1; norm_diff_ground_truth_3d is NaN unless the ground
 *     truth's depth in b is valid, norm_diff_pred_3d[_masked] NaN unless that and the predicted pixel's depth are valid.
 *     fraction_..._masked of a pair whose mask b is empty is NaN (the reference divides by zero there).  The false positives'
 *     pixel distances are summed as integers of 2^-20 pixel, so the averages do not depend on the order of the atomics.
 *     No host synchronisation.  1 <= P <= 65535, 1 <= d <= 64, h * w < 2^31.
 * ===================================================================================================== */
#define DCN_EVAL_COLUMNS 13
#define DCN_EVAL_COL_NORM_DIFF_DESCRIPTOR_GROUND_TRUTH 0
#define DCN_EVAL_COL_NORM_DIFF_DESCRIPTOR 1
#define DCN_EVAL_COL_NORM_DIFF_DESCRIPTOR_MASKED 2
#define DCN_EVAL_COL_NORM_DIFF_GROUND_TRUTH_3D 3
#define DCN_EVAL_COL_NORM_DIFF_PRED_3D 4
#define DCN_EVAL_COL_NORM_DIFF_PRED_3D_MASKED 5
#define DCN_EVAL_COL_PIXEL_MATCH_ERROR_L2 6
#define DCN_EVAL_COL_PIXEL_MATCH_ERROR_L2_MASKED 7
#define DCN_EVAL_COL_PIXEL_MATCH_ERROR_L1 8
#define DCN_EVAL_COL_FRACTION_CLOSER 9
#define DCN_EVAL_COL_FRACTION_CLOSER_MASKED 10
#define DCN_EVAL_COL_AVERAGE_L2_FALSE_POSITIVES 11
#define DCN_EVAL_COL_AVERAGE_L2_FALSE_POSITIVES_MASKED 12
#define DCN_EVAL_BAD_INDEX 1        /* status: a query pixel outside the image, or a ground truth that is NaN / negative (read as 0) */
#define DCN_EVAL_BAD_OFFSETS 2      /* status: offsets not increasing within [0, max_rows] (every pair empty), or a pair above max_pair_rows */
#define DCN_EVAL_BAD_DRAWS 4        /* dcn_hip.evaluate only: the match search's DCN_SAMPLE_BAD_DRAWS (a bad replay stream or match_order) */
#define DCN_EVAL_BAD_FRAME 8        /* dcn_hip.evaluate only: the gather's DCN_FRAME_BAD_INDEX */
size_t dcn_eval_matches_workspace(int n, int h, int w, int64_t attempts);
int dcn_eval_matches(int n, int h, int w, const uint16_t* depth_a, const uint16_t* depth_b, const uint8_t* mask_a,
                     const float* cams, int64_t attempts, const int64_t* seeds, const float* rand, const int64_t* rand_offsets,
                     int num_matches, const int32_t* match_order, const int64_t* order_seeds, int64_t* u_a, int64_t* v_a,
                     float* u_b, float* v_b, int64_t* offsets, int32_t* totals, int32_t* status, void* workspace, void* stream);
size_t dcn_match_statistics_pairs_workspace(int64_t max_rows);
int dcn_match_statistics_pairs(int p, int h, int w, int d, const float* res_a, const float* res_b, const uint8_t* mask_b,
                               const uint16_t* depth_a, const uint16_t* depth_b, const float* cams, const int64_t* u_a,
                               const int64_t* v_a, const float* u_b, const float* v_b, const int64_t* offsets, int64_t max_rows,
                               int max_pair_rows, double* columns, uint8_t* is_valid, int32_t* pred_uv, int32_t* closer,
                               int32_t* row_pair, int32_t* mask_pixels, int32_t* status, void* workspace, void* stream);

/* -----------------------------------------------------------------------------------------------------
 * 11c. Across-object evaluation -- replaces, for device-resident masks and descriptor images, what
 *     single_across_object_image_pair_quantitative_analysis (evaluation.py:784-859) runs per image pair of two DIFFERENT
 *     objects: random_sample_from_masked_image(mask_a, q) (correspondence_finder.py:68-90) and, per sampled pixel,
 *     compute_descriptor_match_statistics_no_ground_truth (:977-1003), i.e. find_best_match over the whole of image b
 *     (dense_correspondence_network.py:488-550, no mask), for ALL pairs in one call each.  P pairs of [h][w] images.
 *
 *     Queries: mask_a uint8 [P][hw], res_a float [P][hw][d].  n_p = mask a's non-zero pixels.  Pair p gets q rows when
 *     n_p >= q, and none otherwise: n_p == 0 is the reference's empty list, 0 < n_p < q raises
 *     DCN_ACROSS_TOO_FEW_MASK_PIXELS (random.sample raises "Sample larger than population" there).  Row j of the pair is the
 *     non-zero pixel number r_j in row-major order (numpy's nonzero() order), with r_j = sample_order[p][j] (replay: int32
 *     [P][q], the reference's rand_inds; a rank outside [0, n_p) reads 0, and it or a rank repeated within the pair raises
 *     DCN_EVAL_BAD_DRAWS), or, with sample_order == NULL, the rank in place j when the n_p ranks are ordered by a hash of
 *     (order_seeds[p], rank), ties by rank -- a uniform random order, its first q entries (the order of 11a).
 *     Outputs: rows [offsets[p], offsets[p+1]) of u_a, v_a (int64) and queries (float [.][d], res_a at the pixel), each with
 *     P * q rows, -1 / 0 from offsets[P] on; offsets int64 [P + 1]; mask_pixels int32 [P]; status int32 [1] (written).
 *     1 <= P <= 1024, 1 <= q <= 1024, 1 <= d <= 64, h * w < 2^31.
 *
 *     Search: for every row of pair p the first minimum, in flat v * w + u order, of the fp32 distance
 *     sqrt(sum_c (res_b[p][pixel][c] - queries[row][c])^2) (summed with fma in channel order, as section 4) over ALL pixels of
 *     res_b float [P][hw][d]; queries float [max_rows][d]; offsets int64 [P + 1] on the device, checked as in 11b
 *     (DCN_EVAL_BAD_OFFSETS; max_pair_rows <= 1024 rows per pair).  res_b is read ONCE whatever the number of rows.
 *       norm_diff float [max_rows] (norm_diff_descriptor_best_match); best_uv int32 [2][max_rows] (u, v); row_pair int32
 *       [max_rows]; status int32 [1] (written).  Rows from offsets[P] on: NaN, -1, -1.
 *     Partial minima are combined as 64-bit integers (distance bits, pixel): bit-identical from run to run.  A NaN distance
 *     never wins.  No host synchronisation in either.
 * ----------------------------------------------------------------------------------------------------- */
#define DCN_ACROSS_TOO_FEW_MASK_PIXELS 16   /* status: a mask a with fewer non-zero pixels than samples asked (the pair has no rows) */
size_t dcn_across_object_queries_workspace(int p, int h, int w);
int dcn_across_object_queries(int p, int h, int w, int d, const uint8_t* mask_a, const float* res_a, int q,
                              const int32_t* sample_order, const int64_t* order_seeds, int64_t* u_a, int64_t* v_a,
                              float* queries, int64_t* offsets, int32_t* mask_pixels, int32_t* status, void* workspace,
                              void* stream);
size_t dcn_best_match_pairs_workspace(int64_t max_rows);
int dcn_best_match_pairs(int p, int h, int w, int d, const float* res_b, const float* queries, const int64_t* offsets,
                         int64_t max_rows, int max_pair_rows, float* norm_diff, int32_t* best_uv, int32_t* row_pair,
                         int32_t* status, void* workspace, void* stream);

/* -----------------------------------------------------------------------------------------------------
 * 11d. Cross-scene evaluation -- replaces, for a frame store and device-resident descriptor images, what
 *     single_cross_scene_image_pair_quantitative_analysis (evaluation.py:610-781) runs per human-labelled match: the
 *     reprojection of the labelled pixel into other views of its scene (batch_find_pixel_correspondences(..., uv_a=<one
 *     pixel>), :721, :756) and compute_descriptor_match_statistics (:1045-1175) of every resulting row.
 *
 *     Reprojection: v requests over the store itself (section 10's tables; nothing is gathered), requests int32 [v][4] =
 *     (src frame, u, v, dst frame).  kcam float [18]: K then K^-1, row-major fp32 (section 10's scene_cams layout) -- given
 *     explicitly because the reference passes no K to this search, which therefore runs with get_default_K_matrix() whatever
 *     the scene's K is.  Arithmetic: section 9's reprojection test (fp32, the reference's evaluation order, the 3 mm occlusion
 *     margin, an exactly-zero coordinate pruned) with pose src as fp32 and pose dst^-1 as section 10's camera rows carry it
 *     (float64 R^T and -(R^T t) summed left to right, then fp32): a request gets the answer 11a gives that candidate.
 *       found uint8 [v]; u2, v2 float [v] (the projection, as the reference's search returns it; 0 when image src has no depth
 *       there); uv int32 [2][v] (clip_pixel_to_image_size_and_round of the projection; -1 when not found); status int32 [1]
 *       (written): DCN_EVAL_BAD_FRAME for a frame index or a pixel outside the store -- that request is not found and
 *       nothing is read out of range.  One work-item per request.  v >= 1.
 *
 *     Statistics: 11b for GROUPS of rows that search one image.  Group g searches res_b[g] (float [G][hw][d]) with mask_b[g]
 *     (uint8 [G][hw]) and depth_b[g] (uint16 [G][hw]); its rows are [offsets[g], offsets[g+1]) (offsets int64 [G + 1] on the
 *     device, checked as in 11b; max_group_rows bounds one group's rows, which may exceed the kernel's query tile).  Every row
 *     carries its own query descriptor queries[r][d], query pixel u_a, v_a (int64), the depth there depth_q[r] (uint16
 *     millimetres), ground truth u_b, v_b (float, rounded and clipped as in 11b), camera row cams[r][DCN_SAMPLE_CAM_FLOATS]
 *     and keep[r] (uint8).  A row with keep == 0 costs no search, none of its other inputs is looked at, and it comes out like
 *     a row past offsets[G].  Outputs and arithmetic are 11b's (the same device functions): columns, is_valid, pred_uv, closer,
 *     row_pair (the row's GROUP, or -1), mask_pixels int32 [G], status int32 [1] (written).  64-bit integer atomics only:
 *     bit-identical from run to run.  No host synchronisation.  1 <= G <= 65535, 1 <= d <= 64, h * w < 2^31.
 *
 *     dcn_match_statistics_groups_wide: the same call for groups of MANY rows (the keypoint table, single_image_pair_cross_
 *     scene_keypoints_quantitative_analysis :1433-1552: an image is searched by (labelled images - 1) * keypoints rows).  The
 *     search is transposed: a work-item holds one row, a workgroup up to 256 rows of one group and a strip of strip_pixels
 *     pixels (0: chosen so that the grid fills the device), which pass by all rows through LDS; no cross-lane reduction.  The
 *     per-(pixel, row) arithmetic is the grouped call's and every accumulation is an integer one, so every output is the
 *     grouped call's BIT FOR BIT, whatever strip_pixels is.  Same workspace.  strip_pixels >= 0, max_group_rows <= 65535 * 256.
 * ----------------------------------------------------------------------------------------------------- */
int dcn_reproject_pixels(int v, const struct dcn_frame_store* store, const float* kcam, const int32_t* requests,
                         uint8_t* found, float* u2, float* v2, int32_t* uv, int32_t* status, void* stream);
size_t dcn_match_statistics_groups_workspace(int64_t max_rows);
int dcn_match_statistics_groups(int g, int h, int w, int d, const float* res_b, const uint8_t* mask_b, const uint16_t* depth_b,
                                const float* queries, const int64_t* u_a, const int64_t* v_a, const uint16_t* depth_q,
                                const float* u_b, const float* v_b, const float* cams, const uint8_t* keep,
                                const int64_t* offsets, int64_t max_rows, int max_group_rows, double* columns,
                                uint8_t* is_valid, int32_t* pred_uv, int32_t* closer, int32_t* row_pair, int32_t* mask_pixels,
                                int32_t* status, void* workspace, void* stream);
int dcn_match_statistics_groups_wide(int g, int h, int w, int d, const float* res_b, const uint8_t* mask_b,
                                     const uint16_t* depth_b, const float* queries, const int64_t* u_a, const int64_t* v_a,
                                     const uint16_t* depth_q, const float* u_b, const float* v_b, const float* cams,
                                     const uint8_t* keep, const int64_t* offsets, int64_t max_rows, int max_group_rows,
                                     int64_t strip_pixels, double* columns, uint8_t* is_valid, int32_t* pred_uv, int32_t* closer,
                                     int32_t* row_pair, int32_t* mask_pixels, int32_t* status, void* workspace, void* stream);

/* =====================================================================================================
 * 12. Descriptor statistics of a dataset -- replaces, for device-resident descriptor images, the per-image half and the
 *     running update of DenseCorrespondenceEvaluation.compute_descriptor_statistics_on_dataset
 *     (dense_correspondence/evaluation/evaluation.py:2157-2304), whose result descriptor_statistics.yaml colours descriptor
 *     images (DenseCorrespondenceNetwork.descriptor_image_stats).
 *
 * 12a. Per image (compute_descriptor_statistics, :2177-2219): res float [n][hw][d] descriptor images (channel last, as
 *     forward_image_tensors returns them); mask uint8 [n][hw] (non-zero: on the object).  ONE read of res and of mask gives
 *       per_image float [n][2][3][d]: (entire image, mask) x (min, max, mean) per channel; mask_pixels int32 [n].
 *     Sums are accumulated in float64 and divided by the float64 count; the mean is rounded to fp32 once.  Workgroups per
 *     image grow with h * w; their partials are folded in a fixed order by a second launch (no floating-point atomics): the
 *     result is the same bit for bit from run to run.  NaN as in torch: a NaN anywhere in a channel makes that channel's min,
 *     max and mean NaN -- for the mask rows only a NaN under the mask.  An image whose mask is empty has mask_pixels 0 and NaN
 *     in its mask rows (the reference returns None, None there, :2203-2204).
 *     1 <= n <= 65535, 1 <= d <= 64, h * w < 2^31.  workspace: dcn_descriptor_statistics_workspace(n, h, w, d) bytes.
 *
 * 12b. Over the images (update_stats and the final scaling, :2237-2292): per_image [n][2][3][d] and mask_pixels [n] as 12a
 *     writes them.  An image with mask_pixels == 0 is skipped for BOTH sets (:2280-2282); min and max over the images used
 *     (torch.min / torch.max: NaN if either is); mean: the fp32 sum of the used images' fp32 means, added in image order, times
 *     (float)(1.0 / num_images) -- num_images, not the number used: the reference's divisor (:2290).
 *       stats float [2][3][d]; used int32 [1].  No image used: stats is NaN.
 *     One workgroup.  n >= 1, num_images >= 1, 1 <= d <= 64.
 *     No host synchronisation in either.
 * ===================================================================================================== */
size_t dcn_descriptor_statistics_workspace(int n, int h, int w, int d);
int dcn_descriptor_statistics(int n, int h, int w, int d, const float* res, const uint8_t* mask, float* per_image,
                              int32_t* mask_pixels, void* workspace, void* stream);
int dcn_descriptor_statistics_combine(int n, int d, const float* per_image, const int32_t* mask_pixels, int num_images,
                                      float* stats, int32_t* used, void* stream);

/* =====================================================================================================
 * 13. Training from a frame store with no host read -- the bookkeeping of DenseCorrespondenceTraining.run()
 *     (dense_correspondence/training/training.py:290-456) around the step, decided on the device: whether the iteration
 *     counts (the `continue` on an empty sample, :304-306), the learning-rate schedule (adjust_learning_rate, :544-558, which
 *     runs AFTER that `continue`), the optimizer step, the batch-norm buffers of a skipped iteration, and the log
 *     (update_plots, :353-413).  All entries are asynchronous on `stream` and read nothing back.
 *
 * 13a. dcn_train_advance: one launch of one work-item, BEFORE the forward pass.  types int32 [B] (SampleBatch.type: -1 for
 *     an empty pair).  active = any(types[p] != -1); if active: when iteration % steps_between_decay == 0, lr *= decay (a
 *     double multiply: the bits of Python's); t += 1; step_size = (float)(lr / (1 - beta1^t)); bc2_sqrt =
 *     (float)sqrt(1 - beta2^t) -- the operations of dcn_adam_step's host code in the same order (double, beta^t by repeated
 *     squaring, rounded once), bit for bit its floats; num_active += 1.  If not: num_skipped += 1, nothing else changes.
 *     B >= 1, steps_between_decay >= 1, decay >= 0, betas in [0, 1).
 * 13b. dcn_adam_step_guarded: dcn_adam_step's launches (tables of 80 tensors, 4096 elements per workgroup, 16-byte path
 *     when the four pointers allow it) with step_size and bc2_sqrt read from the state; a workgroup that finds
 *     state->active == 0 returns before it touches a tensor.  28 bytes per element plus one uniform load per workgroup.
 * 13c. dcn_guarded_copy: n buffers dst[i] <- src[i] of bytes[i] bytes (dst, src, bytes: HOST arrays; 4-byte aligned pointers,
 *     bytes[i] % 4 == 0, bytes[i] < 2^31), performed when state->active == when_active; state == NULL copies
 *     unconditionally.  One workgroup per buffer, tables of 128 buffers per launch.
 * 13d. dcn_train_log: row `row` of history (float64 [rows][DCN_TRAIN_LOG_COLUMNS]):
 *       0 iteration, 1 active, 2 lr, 3 num_valid (pairs of a type in 0 .. 4), 4 loss (the float at `loss`),
 *       5 + 2k, 6 + 2k for term k of terms float [B][5] (loss, match, masked, background, blind): the mean of terms[p][k]
 *       over the pairs p whose TYPE composes term k, added in pair order in double, and the number of those pairs (mean 0
 *       where there is none).  Types 0, 3 and 4 (within scene, multi object, synthetic multi object) compose every term;
 *       types 1 and 2 (across scene, different object) the loss and the blind term (loss_composer.py:26-64, :168-212: the
 *       others are zero_loss()); type -1 none.
 *       15 the type of the first pair that is not empty (-1 when all are).
 *     One launch of one workgroup.  B >= 1, row >= 0 (the caller keeps it below the rows allocated).
 *
 *     Data parallel: G ranks of B pairs each; the global batch is the G B pairs in (rank, pair) order.  Every rank gathers
 *     all ranks' types (and, for the log, all ranks' rows) in rank order and runs the two entries below on them, so that every
 *     rank takes the same decision and writes the same row without a host read.
 * 13e. dcn_train_advance_ranks: 13a's state transition over the G B types of types_all int32 [G][B] (active = N > 0 with
 *     n_r = #{p : types_all[r][p] != -1}, N = sum of n_r; the same code as 13a: bit for bit its floats), and
 *     weight_out[0] = N > 0 ? (float)((double)n_rank / (double)N) : 0.0f -- this rank's share of the non-empty pairs, the
 *     factor of its loss with which the SUM of the ranks' gradients is the gradient of the mean over all non-empty pairs.
 *     One launch of one work-item.  G >= 1, B >= 1, G B < 2^31, 0 <= rank < G, the rest as 13a.
 * 13f. dcn_train_log_ranks: 13d's row over the global batch.  gathered float [G][1 + 5 B]: rank r's weighted loss
 *     (loss_r * w_r), then its terms [B][5].  Columns 0 - 3 and 5 - 15 are 13d's over the G B terms and types in (rank, pair)
 *     order (the same code); column 4 is the sum of the G weighted losses, added in rank order in double.
 *     One launch of one workgroup.  G >= 1, B >= 1, G B < 2^31, row >= 0.
 * ===================================================================================================== */
struct dcn_train_state {
    int32_t active;         /* this iteration counts (set by dcn_train_advance) */
    int32_t reserved;
    int64_t t;              /* Adam step count: the active iterations so far */
    double lr;
    float step_size;        /* lr / (1 - beta1^t) */
    float bc2_sqrt;         /* sqrt(1 - beta2^t) */
    int64_t num_active;
    int64_t num_skipped;
};
#define DCN_TRAIN_LOG_COLUMNS 16
int dcn_train_advance(struct dcn_train_state* state, const int32_t* types, int B, int64_t iteration,
                      int64_t steps_between_decay, double decay, double beta1, double beta2, void* stream);
int dcn_adam_step_guarded(int n, void* const* param, const void* const* grad, void* const* exp_avg, void* const* exp_avg_sq,
                          const int64_t* numel, double eps, double weight_decay, double beta1, double beta2,
                          const struct dcn_train_state* state, void* stream);
int dcn_guarded_copy(int n, void* const* dst, const void* const* src, const int64_t* bytes,
                     const struct dcn_train_state* state, int when_active, void* stream);
int dcn_train_log(double* history, int64_t row, int64_t iteration, const struct dcn_train_state* state, const float* loss,
                  const float* terms, const int32_t* types, int B, void* stream);
int dcn_train_advance_ranks(struct dcn_train_state* state, const int32_t* types_all /* [G][B] */, int G, int B, int rank,
                            float* weight_out /* [1] */, int64_t iteration, int64_t steps_between_decay, double decay,
                            double beta1, double beta2, void* stream);
int dcn_train_log_ranks(double* history, int64_t row, int64_t iteration, const struct dcn_train_state* state,
                        const float* gathered /* [G][1 + 5 B] */, const int32_t* types_all /* [G][B] */, int G, int B,
                        void* stream);

/* =====================================================================================================
 * 14. Evaluation curves -- what the reference does with a column of an evaluation table:
 *     DenseCorrespondenceEvaluationPlotter.make_cdf_plot and compute_area_above_curve
 *     (dense_correspondence/evaluation/evaluation.py:2658-2674, :2844-2863): the empirical CDF of the column over num_bins
 *     bins (scipy.stats.cumfreq with defaultreallimits=None) and the area above it, the number stats.yaml keeps as
 *     norm_diff_3d_area_above_curve (:2953-2975).
 *
 *     values float64 [c][ld]: curve k reads values[k * ld + r], r < rows <= ld.  Row r belongs to the table iff row_pair ==
 *     NULL or row_pair[r] >= 0 (the tables of sections 9 to 11 mark rows past the end, and cross-scene rows without a result,
 *     with -1 and NaN); a row that does not belong is neither counted nor counted as dropped.  drop_nan uint8 [c]: non-zero
 *     drops and counts the NaNs of rows that belong (dropna()); zero makes a NaN an error of that curve (DCN_CURVE_NAN).
 *
 *     In float64, every operation rounded on its own (no fma): n = values kept, mn, mx their minimum and maximum;
 *     s = (mx - mn) / (2. * (num_bins - 1.)); lowerlimit = mn - s; upper = mx + s; the histogram's range is (lowerlimit,
 *     upper), widened to (lowerlimit - 0.5, upper + 0.5) when the two are equal (lowerlimit is reported unwidened, binsize
 *     comes from the widened edges); edge[i] = i * step + first with step = (last - first) / num_bins, edge[num_bins] = last
 *     (np.linspace); binsize = edge[1] - edge[0]; a value is in bin i with edge[i] <= x < edge[i + 1], the last bin closed on
 *     the right -- found as numpy does, by division and a correction by one against the edges.
 *       cumcount int64 [c][num_bins]   running sum of the bin counts
 *       cdf float64 [c][num_bins]      cumcount[i] * (1.0 / n)
 *       summary float64 [c][DCN_CURVE_SUMMARY_DOUBLES]:
 *                                      0 n, 1 NaNs dropped, 2 mn, 3 mx, 4 lowerlimit, 5 binsize,
 *                                      6 area_above_curve = binsize * sum_i (1 - cdf[i]), 7 the curve's flag bits
 *       status int32 [1]               the OR of all curves' flag bits (written, not accumulated)
 *     The sum of the area runs in one fixed order (a butterfly over each 64 bins, the groups of 64 in order) and the counts are
 *     integer atomics in LDS: the outputs are the same bit for bit from run to run.  A flagged curve has cumcount 0 and NaN in
 *     cdf, lowerlimit, binsize and area_above_curve (mn and mx NaN too unless the flag is DCN_CURVE_NONFINITE); the other
 *     curves of the launch are not affected.  DCN_CURVE_NONFINITE also covers finite values whose range is not representable
 *     (mx - mn overflows, or +-0.5 does not widen it).  A bin holds fewer than 2^31 values.
 *     One workgroup per curve (rows in a strided loop: no bound on rows), one launch for all curves after a 4-byte fill of
 *     status, no workspace, no host synchronisation.  1 <= c <= 64, 2 <= num_bins <= 4096, 0 <= rows <= ld; rows == 0 is legal
 *     (every curve DCN_CURVE_EMPTY) and then values may be NULL.
 * ===================================================================================================== */
#define DCN_CURVE_SUMMARY_DOUBLES 8
#define DCN_CURVE_EMPTY 1       /* no value left: the reference divides by len(data) == 0 */
#define DCN_CURVE_NAN 2         /* a NaN met with drop_nan off: numpy refuses the range */
#define DCN_CURVE_NONFINITE 4   /* +-inf among the values: numpy refuses the range */
int dcn_eval_curves(int c, int64_t rows, int64_t ld, const double* values /* [c][ld] */,
                    const int32_t* row_pair /* [rows] or NULL */, const uint8_t* drop_nan /* [c] */,
                    int num_bins, int64_t* cumcount /* [c][num_bins] */, double* cdf /* [c][num_bins] */,
                    double* summary /* [c][8] */, int32_t* status /* [1], OR of all curves */, void* stream);

/* =====================================================================================================
 * 15. Qualitative evaluation -- descriptor pictures and distance heat maps: the arithmetic of
 *     plot_descriptor_colormaps (dense_correspondence/evaluation/evaluation.py:530-601) with the three normalisations of
 *     dense_correspondence/evaluation/plotting.py:5-87, and of compute_gaussian_kernel_heatmap_from_norm_diffs
 *     (dense_correspondence_manipulation/utils/visualization.py:27-31).  Nothing OpenCV draws.
 *     res_a, res_b float [p][h * w][d] (res_b may be NULL: one image per "pair"), mask_a, mask_b uint8 [p][h * w] or NULL
 *     (non-zero counts as 1).  1 <= p <= 1024, 1 <= d <= 64, h * w < 2^31.  No floating-point atomics: bit-identical from run
 *     to run.  No host synchronisation.
 *
 * 15a. dcn_descriptor_ranges: every image read once.
 *       image_ranges float [2][p][4][d]   per image (a's, then b's) and channel: min, max over the image; min, max over the
 *                                         products x * m that are non-zero by numpy's test (-0.0 and 0.0 are left out, NaN
 *                                         takes part: a zero under the mask is skipped, a non-finite value OUTSIDE the mask is
 *                                         inf * 0 = NaN) -- plotting.py:59-75.  A NaN among the values makes the min and the max
 *                                         NaN (np.min / np.max); without masks, or with no such product, rows 2 and 3 are NaN.
 *       pair_ranges float [p][4][d]       the two images' rows combined by Python's min(a, b) / max(a, b), "b if b < a else a"
 *                                         (:43-44, :77-78): a NaN in image a stays, a NaN in image b alone is dropped.
 *       scalar_ranges float [2][p][2]     res.min(), res.max() over all channels of an image
 *       status int32 [p]                  DCN_PICTURE_EMPTY_RANGE: a channel of an image of the pair has no non-zero product
 *                                         (the reference raises ValueError from np.min of an empty array)
 *     Two launches: partials of at most 256 workgroups per image, then one workgroup per pair that folds them in a fixed order.
 * 15b. dcn_descriptor_normalize: one launch that writes up to two families of outputs (say the unmasked and the masked row of
 *     the reference's figure), each by its mode:
 *       DCN_NORM_PAIR          (x - both_min) / (both_max - both_min) in fp32, pair_ranges rows 0, 1        (:28-50)
 *       DCN_NORM_MASKED_PAIR   the same with rows 2, 3, then * m, in fp32                                   (:52-87)
 *       DCN_NORM_STATS         v = clip((double)x, min, max); (v - min) / ((max - min) + 1e-10) in float64 with stats
 *                              double [2][d] (min, then max), the output float64                            (:5-26)
 *       DCN_NORM_STATS_MASKED  the same on the fp32 product x * m, the result times m     (evaluation.py:585-598)
 *       DCN_NORM_SCALAR        (x - res_min) / ((res_max - res_min) + 1e-10f) in fp32 with scalar_ranges    (:5-26, stats None)
 *     every operation rounded on its own.  normed [2][p][h * w][d] (float, double for the STATS modes) and / or picture: the
 *     bytes matplotlib's imshow shows for the float image, uint8(255 * clip(v, 0, 1)) truncated with the product in the
 *     precision of v; a NaN gives 0 (matplotlib's own byte for it is not pinned).  A picture shows picture_channels = 3 image
 *     channels channel[0..2] as [h * w][3] or picture_channels = 1 channel as [h * w]; the picture of (side, pair) starts at
 *     picture + side * side_stride + pair * pair_stride bytes, on any byte boundary: whole aligned dwords are stored, at most
 *     3 + 3 bytes per picture singly.  Two families with pictures show the same channels.
 * 15c. dcn_heat_maps: rows grouped by pair through offsets int64 [p + 1] exactly as dcn_best_match_pairs (section 11c).
 *     out uint8 [max_rows][h * w]: uint8(exp(-dist / variance) * 255) with dist the fp32 distance of section 4 (fma in
 *     channel order, sqrtf), the quotient and the product in fp32, the exponential computed in float64 from the fp32 quotient
 *     and rounded to fp32 once, truncated; a NaN distance gives 0.  With colour_table uint8 [256][3]: out uint8
 *     [max_rows][h * w][3] = colour_table[that byte].  An image is read once whatever the number of rows.  Rows from
 *     offsets[p] on are left UNTOUCHED.  status int32 [1] (DCN_EVAL_BAD_OFFSETS); workspace: DCN_HEAT_WORKSPACE_BYTES.  variance > 0.
 *     The formula is evaluated exactly once per level: a one-workgroup launch finds, by bisection over the float bit patterns,
 *     the 255 squared distances at which the byte steps (every operation of the formula is monotone), and the pixel loop
 *     compares against them -- the same bytes, without a float64 exponential per pixel.
 * ===================================================================================================== */
#define DCN_PICTURE_EMPTY_RANGE 1
#define DCN_HEAT_WORKSPACE_BYTES 2048
#define DCN_NORM_NONE 0
#define DCN_NORM_PAIR 1
#define DCN_NORM_MASKED_PAIR 2
#define DCN_NORM_STATS 3
#define DCN_NORM_STATS_MASKED 4
#define DCN_NORM_SCALAR 5
struct dcn_picture_family {
    int32_t mode;               /* DCN_NORM_* */
    int32_t picture_channels;   /* 1 or 3 (read when picture != NULL) */
    int32_t channel[3];
    int32_t reserved;
    const double* stats;        /* [2][d] for the STATS modes */
    void* normed;               /* or NULL */
    void* picture;              /* or NULL */
    int64_t side_stride, pair_stride;
};
size_t dcn_descriptor_ranges_workspace(int p, int h, int w, int d);
int dcn_descriptor_ranges(int p, int h, int w, int d, const float* res_a, const float* res_b, const uint8_t* mask_a,
                          const uint8_t* mask_b, float* image_ranges, float* pair_ranges, float* scalar_ranges,
                          int32_t* status, void* workspace, void* stream);
int dcn_descriptor_normalize(int p, int h, int w, int d, const float* res_a, const float* res_b, const uint8_t* mask_a,
                             const uint8_t* mask_b, const float* pair_ranges, const float* scalar_ranges,
                             const struct dcn_picture_family* families /* [2] */, void* stream);
int dcn_heat_maps(int p, int h, int w, int d, const float* res_b, const float* queries, const int64_t* offsets,
                  int64_t max_rows, float variance, const uint8_t* colour_table, uint8_t* out, int32_t* status,
                  void* workspace, void* stream);

/* =====================================================================================================
 * 16. Rendering depth images and foreground masks from scene meshes -- the output of the reference's data collection
 *     (modules/dense_correspondence_manipulation/change_detection/change_detection.py: ChangeDetection.run and
 *     render_depth_images draw the fused mesh from every logged camera pose through director / VTK / OpenGL windows) as a
 *     z-buffer rasteriser.  The mask rules are the reference's; the rasteriser has no reference text and is DEFINED here:
 *     every step is an integer operation or one correctly rounded float64 operation (no fma), so the image is the same bit
 *     for bit from run to run and equal to a numpy statement of these rules (tests/render_common.py).
 *
 * 16a. dcn_render_depth.  vertices float [v][3] in the world frame, triangles int32 [t][3] (an index outside [0, v) draws
 *     nothing), camera_to_world float [f][16] row-major, the pose convention of sections 5 and 10 (camera frame: x right, y
 *     down, z forward), the pinhole (fx, fy, cx, cy), h x w pixels (1 .. 16384 each), 0 < z_near < 65.536 (metres).
 *       (a) world-to-camera is the rigid inverse of the pose in float64: rows (R^T | -R^T t) with
 *           (R^T t)_i = (p[i] * p[3] + p[4 + i] * p[7]) + p[8 + i] * p[11], p the pose's entries widened to float64
 *       (b) a vertex in the camera frame: ((a0 * x + a1 * y) + a2 * z) + a3 per row
 *       (c) a triangle with a vertex that is NOT at z >= z_near (behind the camera, too close, NaN) is dropped whole and
 *           counted in status[frame][0].  Nothing is clipped: OpenGL would clip such a triangle against its near plane and
 *           draw the rest.
 *       (d) u = (fx * x) / z + cx, v = (fy * y) / z + cy, snapped to 1/256 pixel: X = rint(u * 256), ties to even.  A
 *           triangle with a snapped coordinate outside +-2^30 (2^22 pixels; NaN, infinity) is dropped whole and counted in
 *           status[frame][1].
 *       (e) pixel (px, py) is covered when its centre (256 px + 128, 256 py + 128) is inside by the three int64 edge
 *           functions E(a -> b, c) = (bx - ax) * (cy - ay) - (by - ay) * (cx - ax): E0 of v1 -> v2, E1 of v2 -> v0, E2 of
 *           v0 -> v1.  A triangle with E0 + E1 + E2 < 0 has v1 and v2 exchanged first (both windings draw); one with
 *           E0 + E1 + E2 == 0 is skipped.  Top-left rule: a centre with E == 0 belongs to the triangle when the edge a -> b has
 *           by < ay (a left edge) or by == ay and bx > ax (a top edge).
 *       (f) z = (E0 + E1 + E2) / ((E0 / z0 + E1 / z1) + E2 / z2) in float64, the integers converted to float64 first (ties to
 *           even), z_i the camera-frame depth of v_i; when z0 == z1 == z2 (a triangle facing the camera) z is that value,
 *           so that such a plane shows its own millimetres and not, after two roundings, one less.  (The quotient form is
 *           used, and not 1 / (...) * (E0 + E1 + E2): it has one rounding fewer and is exact at power-of-two depths.)
 *       (g) mm = trunc(z * 1000), as vtkImageShiftScale fills an unsigned short with scale 1000.  A fragment with mm == 0 or
 *           mm >= 65536 leaves the pixel as it is (alone on its pixel: 0).
 *       (h) the pixel keeps the minimum mm over the triangles that cover it (an unsigned atomicMin: no order dependence).
 *       depth uint16 [f][h][w] millimetres, 0: no surface.  status int32 [f][2]: triangles dropped by (c) and by (d).
 *     A triangle is walked by one work-item unless its bounding box, clipped to the image, holds more than large_threshold
 *     pixels (< 0: the default, 1024); those are drawn tile by tile by whole workgroups.  The image does not depend on it.
 *     Several frames per launch (as many as 64 MiB of per-frame triangle lists hold, at most 64); fills are kernels; no host
 *     synchronisation.  v >= 0, 0 <= t < 2^31 (t == 0: all zeros), f >= 1.
 * 16b. dcn_render_masks on n pixels (any number of images): with depth_b, computeForegroundMask's preparation and
 *     computeForegroundMaskFromDepthImagePair (:219-272, :314-329): int32, zeros read as INT32_MAX,
 *     mask = (b - f) > threshold, depth_change = mask * f; with depth_b == NULL computeForegroundMaskUsingCropStrategy
 *     (:274-312): mask = f > 0, depth_change = f.  mask uint8 0 / 1, visible (or NULL) = mask * 255 (the "visible" mask of
 *     ChangeDetection.run), depth_change (or NULL) uint16.  threshold >= 0.  Pointers as an allocator returns them (8-byte
 *     aligned): whole dwords are stored, the last n % 4 pixels singly.
 * ===================================================================================================== */
size_t dcn_render_depth_workspace(int v, int64_t t, int f, int h, int w);
int dcn_render_depth(int v, int64_t t, int f, int h, int w, const float* vertices, const int32_t* triangles,
                     const float* camera_to_world, double fx, double fy, double cx, double cy, double z_near,
                     int large_threshold, uint16_t* depth, int32_t* status, void* workspace, void* stream);
int dcn_render_masks(int64_t n, const uint16_t* depth_f, const uint16_t* depth_b, int threshold, uint8_t* mask,
                     uint8_t* visible, uint16_t* depth_change, void* stream);

/* =====================================================================================================
 * 17. From logged sensor depth images and camera poses to the scene's meshes: TSDF fusion, surface extraction and the box
 *     crop -- what the reference's data processing gets from its collaborators (spartan's extract_and_fuse_single_scene.py
 *     runs a CUDA tsdf-fusion binary and marching cubes, doc/data_processing_single_scene.md:42-57; director's cropToBox makes
 *     the foreground mesh, fusion_reconstruction.py:246-258, 316-332).  Neither has reference text in the checkout, so the
 *     arithmetic is DEFINED here in the style of section 16: every step is an integer operation or one correctly rounded
 *     float64 operation (no fma); results are the same bit for bit from run to run and equal to a numpy statement of these
 *     rules (tests/fusion_common.py).  Pose convention, rigid inverse and camera-frame point: rules 16(a) and 16(b).
 *
 * 17a. dcn_tsdf_integrate.  The volume: nx, ny, nz voxels (1 .. 1024 each, x fastest: voxel (i, j, k) at (k * ny + j) * nx + i),
 *     origin double [3] (a HOST pointer) and voxel_size s > 0 in metres, trunc_margin mu > 0.  Its state: sum int32 [n] and
 *     weight int32 [n], zero for an empty volume (the caller fills them, e.g. with dcn_fill_bytes); status int32 [1], ADDED to.
 *     depth uint16 [f][h][w] millimetres (h, w in 1 .. 16384), camera_to_world float [f][16], the pinhole (fx, fy, cx, cy),
 *     pixel_offset o, 0 <= max_depth_mm <= 65535.  Per voxel, for the frames in the order given:
 *       1. world centre: origin_x + s * i (one product, one sum), likewise y and z
 *       2. the camera-frame point (x, y, z) by 16(a), 16(b)
 *       3. the frame is skipped unless z > 0 (NaN skips)
 *       4. u = (fx * x) / z + cx, v = (fy * y) / z + cy as 16(d) orders them; px = floor(u + o), py = floor(v + o); skipped
 *          unless 0 <= px < w and 0 <= py < h (NaN and infinity skip)
 *       5. o = 0.5 reads integer pixel coordinates as pixel CENTRES -- the sensor's convention and tsdf-fusion's roundf.
 *          o = 0 is for images made by dcn_render_depth, whose pixel px has its centre at px + 0.5 (rule 16(e)): there the
 *          pixel that holds the projection is floor(u).
 *       6. mm = depth[py][px]; skipped when mm == 0 or mm > max_depth_mm
 *       7. d = mm / 1000.0, diff = d - z; skipped unless diff > -mu
 *       8. t = min(1.0, diff / mu), q = (int) rint(t * 32768.0), ties to even
 *       9. a voxel whose weight is >= 65535 takes no further frame: the frame is counted in status[0] instead (so
 *          |sum| < 2^31)
 *      10. otherwise sum += q, weight += 1
 *     The sums are integers: the result does not depend on how the frames are split over launches (frames_per_launch, 1 .. 64,
 *     < 0: the default 32) or over calls -- calls accumulate.  Frames are walked in order, which settles rule 9.  The signed
 *     distance of a voxel is sum / weight / 32768 * mu.  One work-item per voxel; no host synchronisation.
 * 17b. dcn_tsdf_extract: the zero level of sum / weight by MARCHING TETRAHEDRA on the Kuhn split (not marching cubes: some
 *     twice the triangles, no ambiguous cases, watertight).  A voxel is inside when sum < 0, outside otherwise.
 *       Cube (i, j, k) has its corners c = bx + 2 by + 4 bz at (i + bx, j + by, k + bz); it is valid when all eight have
 *       weight >= min_weight (>= 1).  A valid cube is split into six tetrahedra, one per permutation (a, b, c) of the axes in
 *       lexicographic order (x < y < z): vertices corner 0, e_a, e_a + e_b, corner 7 in this order.  Every tetrahedron edge
 *       runs from its lower voxel A in one of 7 directions x, y, z, xy, xz, yz, xyz (ids 0 .. 6).
 *       Vertices: an edge from A to B carries one vertex when its ends are on different sides and a valid cube has both ends
 *       among its corners.  fa = (double) sumA / (double) weightA, fb likewise, t = fa / (fa - fb); grid coordinate
 *       (double) iA + t on each axis the direction moves along, (double) iA on the others; world = origin + s * g (a product,
 *       then a sum), rounded once to float.  Vertex ids ascend by (voxel index, direction id).
 *       Triangles, per tetrahedron by its inside vertices in vertex order, e(p, q) the vertex of the edge between p and q:
 *       one inside p, outside q1 q2 q3: (e(p,q1), e(p,q2), e(p,q3)); two inside p1 p2, outside q1 q2: the quad e(p1,q1),
 *       e(p1,q2), e(p2,q2), e(p2,q1) as triangles (0, 1, 2) and (0, 2, 3); three inside p1 p2 p3, outside q: (e(p1,q),
 *       e(p2,q), e(p3,q)).  The last two vertices of a triangle are exchanged where needed so that its normal points to the
 *       outside (decided on the unit cube with every t = 1/2; the level set in a tetrahedron is planar, so it holds for every
 *       t).  Triangles ascend by (cube index, tetrahedron id, triangle 0 / 1).
 *     vertices float [max_vertices][3], triangles int32 [max_triangles][3] (unused rows -1), counts int32 [2]: the TRUE numbers
 *     of vertices and triangles (capped at INT32_MAX) even where they exceed the capacities.  Rows beyond a capacity are not
 *     written; a triangle that names an unwritten vertex is a row of -1 (dcn_render_depth draws nothing for it).  The order
 *     comes from exclusive scans over per-voxel counts (reduce per workgroup, one workgroup over the totals, apply).
 * 17c. dcn_mesh_crop: director_utils.py cropToBox / cropToLineSegment (:151-178).  segments double [3][7] (a HOST pointer),
 *     per axis of the box frame what those lines compute in numpy float64: point1 [3], axis' [3], length'.  A point's scalar is
 *     ((d0 * a0 + d1 * a1) + d2 * a2), d = p - point1, a = axis' -- director's labelPointDistanceAlongAxis, which is not in
 *     the checkout: the dot product, stated here.  A triangle survives an axis when all three of its points have the scalar
 *     in [0, length'], bounds included (thresholdCells on a point array: vtkThreshold's all-scalars rule), and the crop when
 *     it survives the three axes.  A row naming an index outside [0, v) does not survive.  Surviving triangles keep their
 *     order; the vertices they use keep theirs and are renumbered (VTK's point order after vtkThreshold is not reproduced).
 *     Capacities, counts and -1 rows as in 17b.  0 <= t < 2^31.
 * ===================================================================================================== */
int dcn_tsdf_integrate(int nx, int ny, int nz, const double* origin, double voxel_size, double trunc_margin, int f, int h, int w,
                       const uint16_t* depth, const float* camera_to_world, double fx, double fy, double cx, double cy,
                       double pixel_offset, int max_depth_mm, int frames_per_launch, int32_t* sum, int32_t* weight,
                       int32_t* status, void* stream);
size_t dcn_tsdf_extract_workspace(int nx, int ny, int nz);
int dcn_tsdf_extract(int nx, int ny, int nz, const double* origin, double voxel_size, const int32_t* sum, const int32_t* weight,
                     int min_weight, int max_vertices, int max_triangles, float* vertices, int32_t* triangles, int32_t* counts,
                     void* workspace, void* stream);
size_t dcn_mesh_crop_workspace(int v, int64_t t);
int dcn_mesh_crop(int v, int64_t t, const float* vertices, const int32_t* triangles, const double* segments, int max_vertices,
                  int max_triangles, float* out_vertices, int32_t* out_triangles, int32_t* counts, void* workspace, void* stream);

/* =====================================================================================================
 * 18. Painting mesh vertices from their views: colour fusion (what spartan's tsdf-fusion writes into fusion_mesh.ply as a colour
 *     per vertex) and the descriptor-coloured mesh (mesh_descriptor_color_app.py: DescriptorMeshColor.color_mesh_using_descriptors;
 *     MeshColorizer in change_detection/mesh_processing.py) as ONE operation.  Both classes live in mesh_processing.mesh_render,
 *     which is not in the checkout, so as in sections 16 and 17 the arithmetic is DEFINED here: every step is an integer operation
 *     or one correctly rounded float64 operation (no fma); results are the same bit for bit from run to run and equal to a numpy
 *     statement of these rules (tests/paint_common.py).  Pose convention, rigid inverse and camera-frame point: rules 16(a) and
 *     16(b); the projection: rule 17a.4 (one text in the library for all three, used by sections 17 and 18).
 *
 * 18a. dcn_mesh_paint accumulates f views into per-vertex state; calls accumulate.  vertices float [v][3] in the world frame;
 *     valid_vertices: a device int32 [1] or NULL -- rows at or beyond it (a negative value: every row) take nothing, which is how
 *     an untrimmed mesh of section 17 passes counts[0:1] without a read-back.  images [f][h][w][c] of image_type DCN_PAINT_UINT8
 *     (the store's RGB layout) or DCN_PAINT_FLOAT (the evaluation's descriptor layout), 1 <= c <= 32; depth uint16 [f][h][w]
 *     millimetres; mask uint8 [f][h][w] or NULL; camera_to_world float [f][16]; the pinhole (fx, fy, cx, cy); pixel_offset o;
 *     margin_mm >= 0.  The state, zero when empty (the caller fills it, e.g. with dcn_fill_bytes): count int32 [v], sum double
 *     [v][c], sumsq double [v][c].  Per vertex, for the frames in the order given:
 *       1. the camera-frame point (x, y, z) by 16(a), 16(b), the vertex widened to float64
 *       2. the frame is skipped unless z > 0 (NaN skips)
 *       3. u, v as 16(d) orders them, px = floor(u + o), py = floor(v + o) (rule 17a.4); skipped unless 0 <= px < w and
 *          0 <= py < h (NaN and infinity skip).  o = 0 for images on dcn_render_depth's grid, 0.5 for the sensor's (rule 17a.5)
 *       4. mm = depth[py][px]; skipped when mm == 0
 *       5. e = z * 1000.0 - (double) mm (a product, then a difference); skipped unless -margin_mm <= e <= margin_mm.  Two-sided:
 *          a vertex behind the surface the view shows is occluded, and one in front of it, projected past a silhouette, would be
 *          painted with the background
 *       6. skipped when a mask is given and mask[py][px] == 0
 *       7. count += 1; per channel in order x = (double) images[py][px][channel], sum += x, sumsq += x * x (a product, then a
 *          sum).  A NaN descriptor propagates.
 *     A vertex owns its state and walks its frames in order (no atomics): the state after all frames does not depend on how they
 *     were split over launches (frames_per_launch, 1 .. 64, < 0: the default 64) or over calls.  One work-item per vertex; no
 *     host synchronisation.  v >= 0, f >= 1, h, w in 1 .. 16384.
 * 18b. dcn_mesh_paint_finish: mean float [v][c], variance float [v] and, where colours is not NULL, colours uint8 [v][3].  For a
 *     vertex with n = count >= min_views (>= 1): mean_c = sum_c / n; var_c = sumsq_c / n - mean_c * mean_c in float64 on the
 *     unrounded mean (a quotient, a product, a difference), a negative result counts as 0; variance = (((0 + var_0) + var_1) +
 *     ...) in channel order; each output is rounded to float once.  For any other vertex mean is 0 and variance NaN (the tables'
 *     NaN convention).  The square root is not taken here.  Colours: for e = 0, 1, 2 with ch = channel_e (in [0, c)) and
 *     lo, hi device double [c]: t = (mean_ch - lo_ch) / (hi_ch - lo_ch) on the float64 mean, clipped to [0, 1],
 *     byte = rint(t * 255), ties to even; a NaN t, or hi_ch == lo_ch, gives 0; a vertex with count < min_views gets
 *     (unseen_red, unseen_green, unseen_blue), each in 0 .. 255.  With uint8 views, lo = 0 and hi = 255 give the rounded mean
 *     colour.
 * ===================================================================================================== */
#define DCN_PAINT_UINT8 0
#define DCN_PAINT_FLOAT 1
int dcn_mesh_paint(int v, const float* vertices, const int32_t* valid_vertices, int f, int h, int w, int c, int image_type,
                   const void* images, const uint16_t* depth, const uint8_t* mask, const float* camera_to_world, double fx,
                   double fy, double cx, double cy, double pixel_offset, double margin_mm, int frames_per_launch, int32_t* count,
                   double* sum, double* sumsq, void* stream);
int dcn_mesh_paint_finish(int v, int c, const int32_t* count, const double* sum, const double* sumsq, int min_views, float* mean,
                          float* variance, int channel0, int channel1, int channel2, const double* lo, const double* hi,
                          int unseen_red, int unseen_green, int unseen_blue, uint8_t* colours, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DCN_HIP_H */
