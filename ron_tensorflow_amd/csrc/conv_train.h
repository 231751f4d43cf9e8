// The interface between the training convolution's translation units - conv_forward_train.hip (ron_conv2d_forward_nhwc),
// conv_backward.hip (ron_conv2d_backward_nhwc and its two relatives), conv_wgrad.hip (the weight-gradient kernel) - and to the
// network-level chain (conv_chain.hip): the host plans of ONE convolution, forward and backward, and the launch steps behind them.
// The entry points and the chain call the same functions, so there is one copy of the plan and of every step: the same views,
// by-shape tile and split, Npad and channel padding whether a layer runs on its own or in the chain.  Only the places differ: every
// off_* is a byte offset from the `ws` pointer a step is given, and the caller may set them afresh behind the plan (the chain points
// them into its own workspace).
#pragma once
#include <algorithm>

#include "conv_mfma.h"

namespace ron {

constexpr int kWgStep = 32;      // pixels per K step of the weight gradient: its packed operands are zero up to the next multiple

// the offset of the next piece of a workspace that holds *total bytes so far; pieces are 256-byte aligned
inline int64_t carve(int64_t* total, int64_t bytes) {
  const int64_t o = *total;
  *total += align_up(bytes, 256);
  return o;
}

// ron_conv2d_forward_nhwc: the descriptor's checks, the ConvLaunch of setup_conv (conv_launch_geometry), the carving of the operator's own workspace
struct ForwardPlan {
  int kind = 0;                 // kFwd* of conv_forward_train.hip (0: a plain stride-1 SAME convolution)
  int pad = 0, K = 0;
  int bias_live = 0, bias_total = 0;
  bool c64 = false;             // the launch also gets the resident-weight images (ConvLaunch::wgt_c64), as setup_conv provides them
  int64_t x_bytes = 0, w_bytes = 0, c64_bytes = 0, out_bytes = 0, sk_bytes = 0;
  int64_t off_x = 0, off_w = 0, off_c64 = 0, off_bias = 0, off_out = 0, off_sk = 0, total = 0;
  ConvLaunch conv;              // pointers unset
};

// What the backward operators decide on the host behind their own descriptor checks (offsets and sizes in bytes).  The operator fills
// rows, sum_cols, conv and wg and carves its own operand buffers; finish_plan does the rest.
struct BackwardCore {
  int64_t rows = 0;         // rows of the packed operands: the pixels rounded up to the K step
  int sum_cols = 0;         // columns of the tensor the bias gradient sums
  int chunks = 0;
  int64_t chunk_rows = 0;
  int64_t off_w = 0, off_bias = 0, off_dx = 0, off_sk = 0, off_slab = 0, off_part = 0, total = 0;
  int64_t w_bytes = 0, dx_bytes = 0, sk_bytes = 0, slab_bytes = 0;
  ConvLaunch conv;          // the data gradient (pointers unset)
  WgradLaunch wg;           // the weight gradient (pointers unset)
};

// ron_conv2d_backward_nhwc
struct BackwardPlan : BackwardCore {
  int pad = 0, cop = 0, npad = 0, taps = 0;
  int64_t pixels = 0, guard = 0;                // halo pixels; guard pixels of x on each side
  int64_t off_dz = 0, off_x = 0;
};

int train_plan_forward(const ron_conv_desc* d, ForwardPlan* P);
int train_plan_backward(const ron_conv_desc* d, BackwardPlan* P);
// the launch of a forward plan over `ws` (every off_* applied)
ConvLaunch train_forward_launch(const ForwardPlan& P, char* ws);
// dense fp32 [n,h,w,csrc] -> `rows` + 2 `guard` pixels of cdst channels of `dtype` in the halo geometry of `pad`, every pixel of the
// buffer written (conv_bwd_pack_halo_kernel): zero where mask <= 0 (mask may be null), in channels >= csrc, halos, guards and tail.
// sstep > 0: src and mask are the coarser [n,hs,ws,csrc], scattered to pixels (soff + sstep * sy, soff + sstep * sx) of the h x w map
int train_pack_halo(int dtype, const float* src, const float* mask, void* out, int64_t rows, int n, int h, int w, int pad, int csrc,
                    int cdst, int64_t guard, hipStream_t s, int hs = 0, int ws = 0, int sstep = 0, int soff = 0);
// the forward's packs of w and bias (device fp32) to ws + P.off_w / off_c64 / off_bias
int train_forward_pack_w(const ron_conv_desc* d, const ForwardPlan& P, const ConvLaunch& c, const float* w, const float* bias, char* ws,
                         hipStream_t s);
// the data gradient's pack of w (taps flipped, cin / cout swapped) to ws + P.off_w
int train_backward_pack_w(const ron_conv_desc* d, const BackwardPlan& P, const float* w, char* ws, hipStream_t s);
// the data gradient: zero bias at ws + P.off_bias, the forward launch over dz into ws + P.off_dx; *out is the halo tensor it wrote
int train_data_grad(const BackwardCore& P, void* dzbuf, char* ws, hipStream_t s, TensorView* out);
// the weight gradient of halo tensors (xbase: halo pixel 0 of x, guard pixels in front); slabs at ws + P.off_slab
int train_weight_grad(const BackwardCore& P, void* xbase, void* dzbase, float* dw, char* ws, hipStream_t s);
// both passes of the bias gradient: column sums of dz, partials at ws + P.off_part
int train_bias_grad(int dtype, const BackwardPlan& P, const void* dzbuf, char* ws, int cout, float* dbias, hipStream_t s);

}  // namespace ron
