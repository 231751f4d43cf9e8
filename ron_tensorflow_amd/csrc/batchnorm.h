// Batch normalisation on the chain's halo tensors (batchnorm.hip -> conv_chain.hip): the kernels, plan and launch order of
// ron_batchnorm_train_nhwc / ron_batchnorm_backward_nhwc with the tensors read and written in place - storage-type (bf16 / fp16)
// views of a workspace instead of dense fp32.  Row r of the operator's [M][c] walk is pixel r of the map in N, H, W order, so the
// statistics and the gradient sums add the same values in the same order and have the operator's bytes.
#pragma once
#include "conv_mfma.h"

namespace ron {

// the descriptor's checks (`what` starts every message) and the bytes of scratch the two calls below need (256-byte aligned)
int bn_view_plan(const char* what, const ron_bn_desc* d, int64_t* scratch_bytes);

// x, y: views of d's shape (any halo, any channel slice), y written in its interior only.  mean and var [c] are written (the
// backward reads them); mean_copy / var_copy, when not null, get the same values; moving_* as in ron_batchnorm_train_nhwc.
int bn_view_forward(const ron_bn_desc* d, const TensorView& x, const TensorView& y, const float* gamma, const float* beta, float* mean,
                    float* var, float* mean_copy, float* var_copy, float* moving_mean, float* moving_var, char* scratch, hipStream_t s);

// dy: the gradient of y as a view; dx (null: not computed) a view written in its interior only; dgamma / dbeta may be null
int bn_view_backward(const ron_bn_desc* d, const TensorView& x, const TensorView& y, const TensorView& dy, const float* gamma,
                     const float* mean, const float* var, const TensorView* dx, float* dgamma, float* dbeta, char* scratch, hipStream_t s);

}  // namespace ron
