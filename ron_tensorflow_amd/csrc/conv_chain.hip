// ron_conv_chain_forward / ron_conv_chain_backward: a sequence of stride-1 SAME convolutions and 2x2 stride-2 max-pools (the VGG
// body: conv1_2 .. fc7) run forward in one call and backward in one call, with the activations and gradients kept as storage-type
// (bf16 / fp16) halo tensors in the caller's workspace between the layers and between the two calls.  fp32 appears only where data
// enters or leaves: x, y, the taps, dx, the weights, biases and their gradients.
//
// Every convolution layer runs the launches ron_conv2d_forward_nhwc and ron_conv2d_backward_nhwc give it on its own: the plans come
// from the same functions (conv_train.h), only the base pointers differ.  What those entry points do at their fp32 boundary - pack x,
// unpack y, pack dy under the ReLU mask, unpack dx - changes no value (they are storage-type values carried in fp32), so the chain's
// results have the same bytes as the operators chained through fp32.  What replaces the boundary here:
//
//   activation j lives in the geometry its CONSUMER reads: the halo of the consumer's padding, and, for the consumer's weight
//   gradient, guard pixels in front and behind and a zero tail up to 32 pixels (WgradLaunch, conv_mfma.h).  A convolution writes its
//   output with halo 1 (ConvLaunch::out of the by-shape plan).  Where the consumer's halo is 1 - the 3x3 body, and a pool - the
//   producer writes the consumer's buffer itself and chain_zero_kernel writes the halo, guards and tail around it; otherwise the
//   producer writes a staging tensor and chain_join_kernel copies it into the consumer's geometry (a re-halo).
//
//   backward, layer i:  dz_i = round((float(g) + dtap) * (y_i > 0))  chain_join_kernel: g is the gradient the next layer left (halo
//   1: the data gradient's output geometry, and the pool backward's), y_i the stored activation, dz_i in the geometry of layer i's
//   own padding with channels padded to 64, zero halo and tail.  One kernel is the ReLU backward, the branch join and the re-halo.
//   Then the data gradient (a forward launch), the weight gradient on (activation i, dz_i) and the column sums of dz_i, as in
//   ron_conv2d_backward_nhwc.  chain_pool_bwd_kernel routes g to the first maximum of each window on views.
//
// All three kernels are bandwidth kernels: 16 bytes per access along the channel axis, plain vector stores, every output element
// written exactly once, no atomics; the only sum (g + dtap) has two terms.
//
// ron_head_chain_forward / ron_head_chain_backward are the same planner and runner with two more layer kinds (include/ron_hip.h):
//
//   RON_CHAIN_BN        the kernels of batchnorm.hip on views (batchnorm.h): x is activation i, y activation i + 1 written straight
//   into its consumer's geometry (chain_zero_kernel around it where a convolution reads it), dy the gradient buffer of activation
//   i + 1, dx the gradient buffer of activation i (halo 1, like a data gradient: the join in front re-halos and masks it as it does
//   any gradient).  mean and var stay in the workspace, [c] floats each behind the scratch region.
//   RON_CHAIN_CONV_PAIR two convolutions (3x3 | 1x1) with their own plans.  Forward: both write channel slices of one tensor
//   (TensorView::coff / cstride).  The input activation exists twice, in the 3x3's geometry and - a re-halo copy - in the 1x1's,
//   because a weight gradient reads whole halo tensors.  Backward: one join per branch cuts its channel slice of the gradient into
//   the branch's own dz geometry; the two data gradients go to the gradient buffer and to a third one, and whoever reads the gradient
//   of that activation adds them in fp32 (chain_join_kernel's second gradient; chain_add_unpack_kernel for a dx that leaves unrounded).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <string>

#include "batchnorm.h"
#include "conv_mfma.h"
#include "conv_train.h"
#include "storage_device.h"      // the roundings, pack8 / unpack8, the halo walk, the pool's first maximum

namespace ron {
namespace {

// ---- the join: out(buffer of `rows` pixels, halo pixel 0 at pixel `guard`) = round((float(g) + float(g2) + add1 + add2) * (mask > 0)) ----
// g, g2 and mask are halo tensors of the map (their own halo and pixel stride), add1 / add2 dense fp32 [N,H,W,dcs] (dcs 0: Csrc);
// each may be null, and each pointer may stand at the first channel of a slice of a wider tensor.  g2 is the second data gradient
// behind a two-branch layer; it never meets add1 or add2 (head chain: no pair behind a tap), so no sum has more than two terms.
// Interior pixels get the value in channels < Csrc; every other element of the buffer - pad channels, halos, guards, tail - zero.
// With g alone it is a copy into another halo geometry.
RON_KERNEL_ARGS_BEGIN
struct JoinArgs {
  const unsigned short* g;
  const float* add1;
  const float* add2;
  const unsigned short* mask;
  unsigned short* out;
  long long rows, guard;
  int N, H, W, pad, Csrc, Cdst;
  int gpad, gcs, mpad, mcs;
};
RON_KERNEL_ARGS_END(JoinArgs)
// the join around a two-branch layer: the second gradient, and the pixel stride of a dense addend whose channels are a slice
RON_KERNEL_ARGS_BEGIN
struct PairJoinArgs {
  JoinArgs j;
  const unsigned short* g2;
  int g2pad, g2cs, dcs;
  int fill_ = 0;
};
RON_KERNEL_ARGS_END(PairJoinArgs)

struct JoinExtra {
  const unsigned short* g2;
  int g2pad, g2cs, dcs;
};
__device__ __forceinline__ const JoinArgs& join_base(const JoinArgs& a) { return a; }
__device__ __forceinline__ const JoinArgs& join_base(const PairJoinArgs& a) { return a.j; }
__device__ __forceinline__ JoinExtra join_extra(const JoinArgs&) { return JoinExtra{nullptr, 0, 0, 0}; }
__device__ __forceinline__ JoinExtra join_extra(const PairJoinArgs& a) { return JoinExtra{a.g2, a.g2pad, a.g2cs, a.dcs}; }

// (ARGS is deduced: JoinArgs - the convolution chain's launches, unchanged - or PairJoinArgs)
template <bool BF16, class ARGS>
__global__ __launch_bounds__(256) void chain_join_kernel(ARGS args) {
  const JoinArgs& a = join_base(args);
  const JoinExtra x2 = join_extra(args);
  // (every buffer of the chain is below 2 GiB, plan_chain: the 16-byte pieces and the pixels fit 32-bit arithmetic)
  const unsigned vecs = a.Cdst / 8;
  const unsigned total = (unsigned)a.rows * vecs;
  const bool vec_ok = a.Csrc % 8 == 0;
  const bool copy = a.add1 == nullptr && a.add2 == nullptr && a.mask == nullptr && x2.g2 == nullptr;
  const int dcs = x2.dcs > 0 ? x2.dcs : a.Csrc;
  for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    const unsigned b = i / vecs;
    const int c0 = (int)(i - b * vecs) * 8;
    uint4 o = {0u, 0u, 0u, 0u};
    HaloPixel p = {false, 0u, 0, 0};
    if (c0 < a.Csrc) p = halo_pixel(b, a.guard, a.N, a.H, a.W, a.pad);
    if (p.inside) {
      const long long img = p.img;
      const int y = p.y, x = p.x;
      const long long dense = (((long long)img * a.H + y) * a.W + x) * dcs + c0;
      const long long g2o = x2.g2 != nullptr ? halo_off(img, y, x, a.H, a.W, x2.g2pad, x2.g2cs) + c0 : 0;
      const long long go = a.g != nullptr ? halo_off(img, y, x, a.H, a.W, a.gpad, a.gcs) + c0 : 0;
      const long long mo = a.mask != nullptr ? halo_off(img, y, x, a.H, a.W, a.mpad, a.mcs) + c0 : 0;
      if (vec_ok && copy) {
        o = *reinterpret_cast<const uint4*>(a.g + go);
      } else {
        float f[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if (vec_ok) {
          float t[8];
          if (a.g != nullptr) unpack8<BF16>(*reinterpret_cast<const uint4*>(a.g + go), f);
          if (x2.g2 != nullptr) {
            unpack8<BF16>(*reinterpret_cast<const uint4*>(x2.g2 + g2o), t);
#pragma unroll
            for (int e = 0; e < 8; ++e) f[e] += t[e];
          }
          if (a.add1 != nullptr) {
            load8(a.add1 + dense, t);
#pragma unroll
            for (int e = 0; e < 8; ++e) f[e] = a.g != nullptr ? f[e] + t[e] : t[e];
          }
          if (a.add2 != nullptr) {
            load8(a.add2 + dense, t);
#pragma unroll
            for (int e = 0; e < 8; ++e) f[e] += t[e];
          }
          if (a.mask != nullptr) {
            unpack8<BF16>(*reinterpret_cast<const uint4*>(a.mask + mo), t);
            keep_positive(f, t);
          }
        } else {
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            if (c0 + e < a.Csrc) {
              float t = a.g != nullptr ? bits_to_f<BF16>(a.g[go + e]) : 0.f;
              if (x2.g2 != nullptr) t += bits_to_f<BF16>(x2.g2[g2o + e]);
              if (a.add1 != nullptr) t = a.g != nullptr ? t + a.add1[dense + e] : a.add1[dense + e];
              if (a.add2 != nullptr) t += a.add2[dense + e];
              f[e] = (a.mask == nullptr || bits_to_f<BF16>(a.mask[mo + e]) > 0.f) ? t : 0.f;
            }
          }
        }
        o = pack8<BF16>(f);
      }
    }
    *reinterpret_cast<uint4*>(a.out + (long long)i * 8) = o;
  }
}

// ---- dx of a chain that starts with a two-branch layer: out (dense fp32 [N,H,W,C]) = float(a) + float(b), unrounded ----------------------
RON_KERNEL_ARGS_BEGIN
struct AddUnpackArgs {
  const unsigned short* a;
  const unsigned short* b;
  float* out;
  long long total;          // pixels x groups of 8 channels
  int H, W, C, apad, bpad;
  int fill_ = 0;
};
RON_KERNEL_ARGS_END(AddUnpackArgs)

template <bool BF16>
__global__ __launch_bounds__(256) void chain_add_unpack_kernel(AddUnpackArgs p) {
  const int groups = p.C / 8;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < p.total; i += (long long)gridDim.x * blockDim.x) {
    const int c0 = (int)(i % groups) * 8;
    const long long pix = i / groups;
    const int x = (int)(pix % p.W), y = (int)((pix / p.W) % p.H);
    const long long img = pix / ((long long)p.W * p.H);
    float fa[8], fb[8];
    unpack8<BF16>(*reinterpret_cast<const uint4*>(p.a + halo_off(img, y, x, p.H, p.W, p.apad, p.C) + c0), fa);
    unpack8<BF16>(*reinterpret_cast<const uint4*>(p.b + halo_off(img, y, x, p.H, p.W, p.bpad, p.C) + c0), fb);
    float* o = p.out + pix * p.C + c0;
    *reinterpret_cast<float4*>(o) = make_float4(fa[0] + fb[0], fa[1] + fb[1], fa[2] + fb[2], fa[3] + fb[3]);
    *reinterpret_cast<float4*>(o + 4) = make_float4(fa[4] + fb[4], fa[5] + fb[5], fa[6] + fb[6], fa[7] + fb[7]);
  }
}

// ---- zero everything of a buffer that is not an interior pixel: halos, guards, tail (the producer wrote the interior) ---------------------
RON_KERNEL_ARGS_BEGIN
struct ZeroArgs {
  unsigned short* out;
  long long rows, guard;      // pixels of the buffer; halo pixel 0 is pixel `guard`
  int N, H, W, pad, C;
  int fill_ = 0;
};
RON_KERNEL_ARGS_END(ZeroArgs)

__global__ __launch_bounds__(256) void chain_zero_kernel(ZeroArgs a) {
  const unsigned vecs = a.C / 8;
  const unsigned total = (unsigned)a.rows * vecs;
  const uint4 zero4 = {0u, 0u, 0u, 0u};
  for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    if (!halo_pixel(i / vecs, a.guard, a.N, a.H, a.W, a.pad).inside) *reinterpret_cast<uint4*>(a.out + (long long)i * 8) = zero4;
  }
}

// ---- pool backward on views: dx(window position) = g(window) at the FIRST maximum of the stored x, 0 at the others -------------------------
// The rule is first_max_2x2 (storage_device.h), the one of ron_maxpool2x2_backward_nhwc; positions an odd map does not have are neither read nor written.  One lane = one window x 8 channels: four 16-byte
// loads of x, one of g, four 16-byte stores; every interior element of dx is written exactly once, its halo is left alone.
RON_KERNEL_ARGS_BEGIN
struct PoolBwdViewArgs {
  const unsigned short* x;
  const unsigned short* g;
  unsigned short* dx;
  long long total;          // windows x groups of 8 channels
  int H, W, OH, OW, C;
  int xpad, gpad, dpad;
};
RON_KERNEL_ARGS_END(PoolBwdViewArgs)

template <bool BF16>
__global__ __launch_bounds__(256) void chain_pool_bwd_kernel(PoolBwdViewArgs a) {
  const int groups = a.C / 8;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < a.total; i += (long long)gridDim.x * blockDim.x) {
    const int c0 = (int)(i % groups) * 8;
    const long long win = i / groups;
    const int ox = (int)(win % a.OW);
    const int oy = (int)((win / a.OW) % a.OH);
    const long long img = win / ((long long)a.OW * a.OH);
    const bool has_c = 2 * ox + 1 < a.W, has_r = 2 * oy + 1 < a.H;
    const long long x00 = halo_off(img, 2 * oy, 2 * ox, a.H, a.W, a.xpad, a.C) + c0;
    const long long xrow = (long long)(a.W + a.xpad) * a.C;
    const long long d00 = halo_off(img, 2 * oy, 2 * ox, a.H, a.W, a.dpad, a.C) + c0;
    const long long drow = (long long)(a.W + a.dpad) * a.C;
    const uint4 v00 = *reinterpret_cast<const uint4*>(a.x + x00);
    uint4 v01 = v00, v10 = v00, v11 = v00;
    if (has_c) v01 = *reinterpret_cast<const uint4*>(a.x + x00 + a.C);
    if (has_r) v10 = *reinterpret_cast<const uint4*>(a.x + x00 + xrow);
    if (has_r && has_c) v11 = *reinterpret_cast<const uint4*>(a.x + x00 + xrow + a.C);
    const uint4 gv = *reinterpret_cast<const uint4*>(a.g + halo_off(img, oy, ox, a.OH, a.OW, a.gpad, a.C) + c0);
    float f00[8], f01[8], f10[8], f11[8];
    unpack8<BF16>(v00, f00); unpack8<BF16>(v01, f01); unpack8<BF16>(v10, f10); unpack8<BF16>(v11, f11);
    const unsigned ug[4] = {gv.x, gv.y, gv.z, gv.w};
    unsigned o[4][4] = {{0u, 0u, 0u, 0u}, {0u, 0u, 0u, 0u}, {0u, 0u, 0u, 0u}, {0u, 0u, 0u, 0u}};
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int wd = e >> 1, sh = 16 * (e & 1);
      const int at = first_max_2x2(f00[e], f01[e], f10[e], f11[e], has_c, has_r);
      const unsigned grad = ((ug[wd] >> sh) & 0xFFFFu) << sh;
#pragma unroll
      for (int p = 0; p < 4; ++p) o[p][wd] |= at == p ? grad : 0u;
    }
    *reinterpret_cast<uint4*>(a.dx + d00) = make_uint4(o[0][0], o[0][1], o[0][2], o[0][3]);
    if (has_c) *reinterpret_cast<uint4*>(a.dx + d00 + a.C) = make_uint4(o[1][0], o[1][1], o[1][2], o[1][3]);
    if (has_r) *reinterpret_cast<uint4*>(a.dx + d00 + drow) = make_uint4(o[2][0], o[2][1], o[2][2], o[2][3]);
    if (has_r && has_c) *reinterpret_cast<uint4*>(a.dx + d00 + drow + a.C) = make_uint4(o[3][0], o[3][1], o[3][2], o[3][3]);
  }
}

// ---- plan_chain ---------------------------------------------------------------------------------------------------------------------------
// One planner and one runner for ron_conv_chain_* and ron_head_chain_*: the former are descriptors without BN and pair layers, copied
// into the latter's form; `Who` carries the names their messages use.
struct Who {
  const char* what;         // "conv chain" / "head chain"
  const char* sizer;
  bool head;                // batch normalisation and pair layers are accepted
};
const Who kConvChain = {"conv chain", "ron_conv_chain_workspace_bytes", false};
const Who kHeadChain = {"head chain", "ron_head_chain_workspace_bytes", true};

// Activation j (0: the chain's input, j: the output of layer j - 1) in the geometry of its consumer, layer j.  The buffer is
// [guard][rows][guard] pixels of c channels; the view starts `guard` pixels in.  A pair consumes it twice: the 3x3 branch this
// buffer, the 1x1 branch a copy in ITS geometry (the *2 members; rows2 == 0: none), because WgradLaunch reads whole halo tensors.
struct ChainAct {
  int h = 0, w = 0, c = 0, pad = 0;
  int64_t guard = 0, pixels = 0, rows = 0, off = 0;
  int pad2 = 0;
  int64_t guard2 = 0, pixels2 = 0, rows2 = 0, off2 = 0;
  bool zero_fill = false;       // a convolution reads it: halos, guards and tail must be zero
  int64_t bytes() const { return (rows + 2 * guard) * c * 2; }
  int64_t bytes2() const { return (rows2 + 2 * guard2) * c * 2; }
  int64_t view_off() const { return off + guard * c * 2; }
  int64_t view_off2() const { return off2 + guard2 * c * 2; }
};

// one convolution of a layer: the only one of a RON_CHAIN_CONV layer, one of the two of a pair
struct ChainConv {
  ron_conv_desc d;
  ForwardPlan fp;
  BackwardPlan bp;
  int coff = 0;                 // its first channel in the layer's output
};

struct ChainLayer {
  int kind = RON_CHAIN_CONV;
  int nconv = 0;                // 0 (pool, BN), 1 (convolution), 2 (pair: the 3x3 branch, then the 1x1)
  ChainConv conv[2];
  int cout = 0;                 // channels of the layer's output
  bool direct = false;          // the forward writes activation i + 1 itself (else: the staging tensor, then a re-halo copy)
  int64_t off_stage = 0, stage_bytes = 0;
  ron_bn_desc bn;               // BN layers
  int64_t off_bn = 0, bn_bytes = 0, off_stats = 0;      // the kernels' scratch; mean [c] then var [c], kept for the backward
};

struct ChainPlan {
  int L = 0, dtype = 0, n = 0;
  ChainAct act[RON_CHAIN_MAX_LAYERS + 1];
  ChainLayer layer[RON_CHAIN_MAX_LAYERS];
  int64_t off_g[2] = {0, 0}, g_bytes = 0;       // the gradient of activation j is in buffer j & 1, halo 1
  int64_t off_g2 = 0;                           // behind a pair: the 1x1 branch's data gradient (the 3x3's is in buffer j & 1)
  int64_t off_scratch = 0, scratch_bytes = 0;
  int64_t total = 0;
};

bool is_conv(int kind) { return kind == RON_CHAIN_CONV || kind == RON_CHAIN_CONV_PAIR; }

int check_chain_desc(const Who& who, const ron_head_chain_desc* d) {
  const char* what = who.what;
  RON_REQUIRE(d != nullptr, "%s: NULL descriptor", what);
  RON_REQUIRE(d->num_layers >= 1 && d->num_layers <= RON_CHAIN_MAX_LAYERS, "%s: num_layers %d: 1 .. %d", what, d->num_layers, RON_CHAIN_MAX_LAYERS);
  RON_REQUIRE(d->dtype == RON_DTYPE_BF16 || d->dtype == RON_DTYPE_F16, "%s: dtype %d: bf16 or fp16 only (fp32 and f16x3 have no backward)", what, d->dtype);
  RON_REQUIRE(d->n >= 1 && d->h >= 1 && d->w >= 1, "%s: empty tensor (n %d, h %d, w %d)", what, d->n, d->h, d->w);
  const bool head = who.head;
  // (a convolution's own plan asks for a multiple of 64; a head chain may start with a batch normalisation or a pool: 16-byte pieces)
  const int cin_unit = head && d->layers[0].kind != RON_CHAIN_CONV && d->layers[0].kind != RON_CHAIN_CONV_PAIR ? 8 : 64;
  RON_REQUIRE(d->cin >= cin_unit && d->cin % cin_unit == 0, "%s: cin %d must be a multiple of %d (the 3-channel stem is out of scope)", what, d->cin,
              cin_unit);
  for (int i = 0; i < d->num_layers; ++i) {
    const ron_head_chain_layer& l = d->layers[i];
    RON_REQUIRE(l.kind == RON_CHAIN_CONV || l.kind == RON_CHAIN_POOL2 || (head && (l.kind == RON_CHAIN_BN || l.kind == RON_CHAIN_CONV_PAIR)),
                "%s: layer %d: unknown kind %d", what, i, l.kind);
    RON_REQUIRE(l.tap == 0 || l.tap == 1, "%s: layer %d: tap %d: 0 or 1", what, i, l.tap);
    if (l.kind == RON_CHAIN_POOL2) {
      RON_REQUIRE(l.tap == 0, "%s: layer %d: a pool cannot be tapped (tap the convolution in front of it and pool the tap)", what, i);
      continue;
    }
    if (l.kind == RON_CHAIN_BN) {
      RON_REQUIRE(l.tap == 0, "%s: layer %d: a tap on a batch normalisation layer is not built", what, i);
      RON_REQUIRE(l.relu == 0 || l.relu == 1, "%s: layer %d: relu is 0 or 1", what, i);
      continue;       // eps, decay, the channels and M: plan_bn, with the layer's shape
    }
    RON_REQUIRE((l.relu == 0 || l.relu == 1) && (l.has_bias == 0 || l.has_bias == 1), "%s: layer %d: relu and has_bias are 0 or 1", what, i);
    if (l.kind == RON_CHAIN_CONV_PAIR) {
      RON_REQUIRE(l.tap == 0, "%s: layer %d: a tap on a two-branch convolution is not built", what, i);
      RON_REQUIRE(i == 0 || d->layers[i - 1].tap == 0,
                  "%s: layer %d: a two-branch convolution directly behind a tapped layer (its gradient would be a sum of three terms in no fixed order)", what, i);
      RON_REQUIRE(l.cout >= 64 && l.cout % 64 == 0, "%s: layer %d: cout %d of the 3x3 branch must be a multiple of 64", what, i, l.cout);
      RON_REQUIRE(l.cout2 >= 64 && l.cout2 % 64 == 0, "%s: layer %d: cout2 %d of the 1x1 branch must be a multiple of 64", what, i, l.cout2);
      continue;
    }
    RON_REQUIRE(l.k == 1 || l.k == 3 || (l.k == 7 && l.dilation == 1), "%s: layer %d: filter %d x %d at dilation %d: 1 x 1, 3 x 3, or 7 x 7 at dilation 1 only",
                what, i, l.k, l.k, l.dilation);
    RON_REQUIRE(l.dilation >= 1 && l.dilation <= kConvMaxDilation, "%s: layer %d: dilation %d: 1 .. %d", what, i, l.dilation, kConvMaxDilation);
    RON_REQUIRE(l.cout >= 1, "%s: layer %d: cout %d", what, i, l.cout);
    RON_REQUIRE(i == d->num_layers - 1 || l.cout % 64 == 0, "%s: layer %d: cout %d must be a multiple of 64 on a layer that feeds another one", what, i, l.cout);
  }
  return RON_OK;
}

int plan_one_conv(const ron_head_chain_desc* d, int h, int w, int cin, int k, int dilation, int cout, int relu, ChainConv* v) {
  ron_conv_desc& cd = v->d;
  cd = ron_conv_desc();
  cd.n = d->n; cd.h = h; cd.w = w; cd.cin = cin; cd.cout = cout;
  cd.kh = cd.kw = k; cd.stride = 1; cd.dilation = dilation; cd.relu = relu;
  cd.dtype = d->dtype; cd.tile_cfg = -1; cd.splitk = -1;
  if (int rc = train_plan_forward(&cd, &v->fp)) return rc;
  return train_plan_backward(&cd, &v->bp);
}

int plan_chain(const Who& who, const ron_head_chain_desc* d, ChainPlan* P) {
  if (int rc = check_chain_desc(who, d)) return rc;
  const char* what = who.what;
  const int L = d->num_layers;
  const int64_t lim = (int64_t)1 << 31;
  P->L = L; P->dtype = d->dtype; P->n = d->n;
  int h = d->h, w = d->w, c = d->cin;
  int64_t fwd_scratch = 0, bwd_scratch = 0;
  bool any_pair = false;
  for (int j = 0; j <= L; ++j) {
    ChainAct& a = P->act[j];
    a.h = h; a.w = w; a.c = c;
    const int kind = j < L ? d->layers[j].kind : -1;
    if (j < L) P->layer[j].kind = kind;
    if (is_conv(kind)) {
      const ron_head_chain_layer& l = d->layers[j];
      ChainLayer& y = P->layer[j];
      const bool pair = kind == RON_CHAIN_CONV_PAIR;
      y.nconv = pair ? 2 : 1;
      if (int rc = plan_one_conv(d, h, w, c, pair ? 3 : l.k, pair ? 1 : l.dilation, l.cout, l.relu, &y.conv[0])) return rc;
      const BackwardPlan& bp = y.conv[0].bp;
      a.pad = bp.pad;
      a.guard = align_up(bp.guard, 2);        // (an even number of pixels: the view stays 256-byte aligned)
      a.pixels = bp.pixels;
      a.rows = bp.rows;
      a.zero_fill = true;
      y.cout = l.cout;
      if (pair) {
        any_pair = true;
        if (int rc = plan_one_conv(d, h, w, c, 1, 1, l.cout2, l.relu, &y.conv[1])) return rc;
        const BackwardPlan& b2 = y.conv[1].bp;
        y.conv[1].coff = l.cout;
        a.pad2 = b2.pad;
        a.guard2 = align_up(b2.guard, 2);
        a.pixels2 = b2.pixels;
        a.rows2 = b2.rows;
        y.cout = l.cout + l.cout2;
      }
      c = y.cout;
    } else {
      // a pool and a batch normalisation read interiors only; the chain's output has the halo a convolution writes with
      a.pad = 1;
      a.pixels = TensorView::halo_pixels(d->n, h, w, 1);
      a.rows = a.pixels;
      if (kind == RON_CHAIN_POOL2) { h = (h + 1) / 2; w = (w + 1) / 2; }
      if (kind == RON_CHAIN_BN) {
        const ron_head_chain_layer& l = d->layers[j];
        ChainLayer& y = P->layer[j];
        y.bn = ron_bn_desc();
        y.bn.n = d->n; y.bn.h = h; y.bn.w = w; y.bn.c = c; y.bn.dtype = d->dtype; y.bn.relu = l.relu; y.bn.eps = l.eps; y.bn.decay = l.decay;
        char name[64];
        snprintf(name, sizeof name, "%s: layer %d (batch norm)", what, j);
        if (int rc = bn_view_plan(name, &y.bn, &y.bn_bytes)) return rc;
        y.cout = c;
      }
    }
    RON_REQUIRE(a.bytes() < lim && a.bytes2() < lim, "%s: activation %d (%d x %d x %d x %d) would reach 2 GiB", what, j, d->n, a.h, a.w, a.c);
    a.off = carve(&P->total, a.bytes());
    if (a.rows2 > 0) a.off2 = carve(&P->total, a.bytes2());
    P->g_bytes = std::max(P->g_bytes, TensorView::halo_pixels(d->n, a.h, a.w, 1) * (int64_t)a.c * 2);
  }
  RON_REQUIRE(P->g_bytes < lim, "%s: a gradient tensor would reach 2 GiB", what);
  for (int i = 0; i < L; ++i) {
    ChainLayer& y = P->layer[i];
    if (y.kind == RON_CHAIN_BN) {
      y.off_bn = 0;
      fwd_scratch = std::max(fwd_scratch, y.bn_bytes);
      bwd_scratch = std::max(bwd_scratch, y.bn_bytes);
    }
    if (y.nconv == 0) continue;
    const bool last = i == L - 1;
    y.direct = !last && P->act[i + 1].pad == 1;
    // a pair's branches write channel slices of one tensor: the staging tensor holds both
    y.stage_bytes = y.direct || last ? 0 : TensorView::halo_pixels(d->n, P->act[i].h, P->act[i].w, 1) * (int64_t)y.cout * 2;
    // the layer's share of the scratch region, re-carved from offset 0: the forward's packs, split-K slabs and staging tensor ...
    int64_t t = 0;
    auto take = [&t](int64_t bytes) { const int64_t o = t; t += align_up(bytes, 256); return o; };
    for (int b = 0; b < y.nconv; ++b) {
      ForwardPlan& fp = y.conv[b].fp;
      fp.off_w = take(fp.w_bytes);
      fp.off_c64 = take(fp.c64_bytes);
      fp.off_bias = take((int64_t)fp.bias_total * 4);
      fp.off_sk = take(fp.sk_bytes);
      if (b == 0) y.off_stage = take(y.stage_bytes);
    }
    fwd_scratch = std::max(fwd_scratch, t);
    // ... and the backward's: dz, the flipped weights, the zero bias, split-K slabs, pixel-slice slabs, column-sum partials
    t = 0;
    for (int b = 0; b < y.nconv; ++b) {
      BackwardPlan& bp = y.conv[b].bp;
      bp.off_dz = take(bp.rows * bp.cop * 2);
      bp.off_w = take(bp.w_bytes);
      bp.off_bias = take((int64_t)bp.conv.Npad * 4);
      bp.off_sk = take(bp.sk_bytes);
      bp.off_slab = take(bp.slab_bytes);
      bp.off_part = take((int64_t)bp.chunks * bp.sum_cols * 4);
    }
    bwd_scratch = std::max(bwd_scratch, t);
  }
  P->off_g[0] = carve(&P->total, P->g_bytes);
  P->off_g[1] = carve(&P->total, P->g_bytes);
  P->scratch_bytes = std::max(fwd_scratch, bwd_scratch);
  P->off_scratch = carve(&P->total, P->scratch_bytes);
  if (any_pair) P->off_g2 = carve(&P->total, P->g_bytes);
  // every layer offset becomes an offset from the workspace's base
  for (int i = 0; i < L; ++i) {
    ChainLayer& y = P->layer[i];
    const int64_t s = P->off_scratch;
    if (y.kind == RON_CHAIN_BN) {
      y.off_bn += s;
      y.off_stats = carve(&P->total, (int64_t)2 * y.bn.c * 4);
    }
    if (y.nconv == 0) continue;
    y.off_stage += s;
    for (int b = 0; b < y.nconv; ++b) {
      ForwardPlan& fp = y.conv[b].fp;
      BackwardPlan& bp = y.conv[b].bp;
      fp.off_w += s; fp.off_c64 += s; fp.off_bias += s; fp.off_sk += s;
      fp.off_x = b == 0 ? P->act[i].view_off() : P->act[i].view_off2();
      fp.off_out = i == L - 1 || y.direct ? P->act[i + 1].view_off() : y.off_stage;
      bp.off_dz += s; bp.off_w += s; bp.off_bias += s; bp.off_sk += s; bp.off_slab += s; bp.off_part += s;
      bp.off_x = fp.off_x;
      bp.off_dx = b == 0 ? P->off_g[i & 1] : P->off_g2;
    }
  }
  return RON_OK;
}

TensorView act_view(const ChainPlan& P, int j, char* ws) {
  const ChainAct& a = P.act[j];
  TensorView v;
  v.base = ws + a.view_off();
  v.N = P.n; v.H = a.h; v.W = a.w; v.C = a.c; v.cstride = a.c; v.coff = 0; v.pad = a.pad;
  v.bytes = a.pixels * a.c * 2;
  return v;
}

// the gradient of activation j: halo 1, in buffer j & 1 (second: the 1x1 branch's share behind a pair)
TensorView grad_view(const ChainPlan& P, int j, char* ws, bool second = false) {
  const ChainAct& a = P.act[j];
  TensorView v;
  v.base = ws + (second ? P.off_g2 : P.off_g[j & 1]);
  v.N = P.n; v.H = a.h; v.W = a.w; v.C = a.c; v.cstride = a.c; v.coff = 0; v.pad = 1;
  v.bytes = TensorView::halo_pixels(P.n, a.h, a.w, 1) * a.c * 2;
  return v;
}

template <class ARGS>
int launch_join_as(int dtype, int grid, const ARGS& a, hipStream_t s) {
  if (dtype == RON_DTYPE_BF16) RON_LAUNCH(chain_join_kernel<true>, dim3(grid), dim3(256), 0, s, a);
  else RON_LAUNCH(chain_join_kernel<false>, dim3(grid), dim3(256), 0, s, a);
  RON_HIP_CHECK(ron::launch_error());
  return RON_OK;
}

// without a second gradient and a slice's stride it is the convolution chain's launch, argument for argument
int launch_join(int dtype, const PairJoinArgs& a, hipStream_t s) {
  const int grid = grid_for(a.j.rows * (a.j.Cdst / 8));
  return a.g2 == nullptr && a.dcs == 0 ? launch_join_as(dtype, grid, a.j, s) : launch_join_as(dtype, grid, a, s);
}

int launch_zero(const ChainPlan& P, int j, char* ws, hipStream_t s) {
  const ChainAct& t = P.act[j];
  ZeroArgs a = ZeroArgs();
  a.out = reinterpret_cast<unsigned short*>(ws + t.off);
  a.rows = t.rows + 2 * t.guard; a.guard = t.guard;
  a.N = P.n; a.H = t.h; a.W = t.w; a.pad = t.pad; a.C = t.c;
  RON_LAUNCH(chain_zero_kernel, dim3(grid_for(a.rows * (a.C / 8))), dim3(256), 0, s, a);
  RON_HIP_CHECK(ron::launch_error());
  return RON_OK;
}

// `src` (a halo tensor of activation j's map) -> activation j's buffer in its consumer's geometry, every pixel of the buffer written;
// second: the copy a pair's 1x1 branch reads
int launch_rehalo(const ChainPlan& P, int j, const TensorView& src, bool second, char* ws, hipStream_t s) {
  const ChainAct& t = P.act[j];
  PairJoinArgs args = PairJoinArgs();
  JoinArgs& a = args.j;
  a.g = static_cast<const unsigned short*>(src.base); a.gpad = src.pad; a.gcs = src.cstride;
  a.out = reinterpret_cast<unsigned short*>(ws + (second ? t.off2 : t.off));
  a.guard = second ? t.guard2 : t.guard;
  a.rows = (second ? t.rows2 : t.rows) + 2 * a.guard;
  a.N = P.n; a.H = t.h; a.W = t.w; a.pad = second ? t.pad2 : t.pad; a.Csrc = t.c; a.Cdst = t.c;
  return launch_join(P.dtype, args, s);
}

int launch_pool_bwd(int dtype, const TensorView& x, const TensorView& g, const TensorView& dx, hipStream_t s) {
  PoolBwdViewArgs a = PoolBwdViewArgs();
  a.x = static_cast<const unsigned short*>(x.base); a.g = static_cast<const unsigned short*>(g.base);
  a.dx = static_cast<unsigned short*>(dx.base);
  a.H = x.H; a.W = x.W; a.OH = g.H; a.OW = g.W; a.C = x.C;
  a.xpad = x.pad; a.gpad = g.pad; a.dpad = dx.pad;
  a.total = (long long)x.N * a.OH * a.OW * (a.C / 8);
  const int grid = grid_for(a.total);
  if (dtype == RON_DTYPE_BF16) RON_LAUNCH(chain_pool_bwd_kernel<true>, dim3(grid), dim3(256), 0, s, a);
  else RON_LAUNCH(chain_pool_bwd_kernel<false>, dim3(grid), dim3(256), 0, s, a);
  RON_HIP_CHECK(ron::launch_error());
  return RON_OK;
}

int launch_add_unpack(int dtype, const TensorView& a, const TensorView& b, float* out, hipStream_t s) {
  AddUnpackArgs p = AddUnpackArgs();
  p.a = static_cast<const unsigned short*>(a.base); p.b = static_cast<const unsigned short*>(b.base); p.out = out;
  p.H = a.H; p.W = a.W; p.C = a.C; p.apad = a.pad; p.bpad = b.pad;
  p.total = (long long)a.N * a.H * a.W * (a.C / 8);
  const int grid = grid_for(p.total);
  if (dtype == RON_DTYPE_BF16) RON_LAUNCH(chain_add_unpack_kernel<true>, dim3(grid), dim3(256), 0, s, p);
  else RON_LAUNCH(chain_add_unpack_kernel<false>, dim3(grid), dim3(256), 0, s, p);
  RON_HIP_CHECK(ron::launch_error());
  return RON_OK;
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
bool aligned4(const void* p) { return ((uintptr_t)p & 3) == 0; }

// what launch_conv would refuse is refused before anything is enqueued
int describe(ConvLaunch c, char* ws) {
  if (c.bias == nullptr) c.bias = reinterpret_cast<const float*>(ws);
  int o[4];
  return conv_describe(c, o);
}

// the forward launch of one convolution of layer i: a pair's branch writes its channel slice of the layer's output
ConvLaunch forward_launch(const ChainLayer& y, int b, char* ws) {
  ConvLaunch c = train_forward_launch(y.conv[b].fp, ws);
  if (y.nconv == 2) {
    c.out.cstride = y.cout; c.out.coff = y.conv[b].coff;
    c.out.bytes = c.out.pixels() * y.cout * 2;
  }
  return c;
}

ConvLaunch data_grad_launch(const BackwardPlan& bp, char* ws) {
  ConvLaunch c = bp.conv;
  c.in.base = ws + bp.off_dz; c.out.base = ws + bp.off_dx;
  c.wgt = ws + bp.off_w; c.bias = reinterpret_cast<const float*>(ws + bp.off_bias);
  if (bp.sk_bytes > 0) { c.scratch = ws + bp.off_sk; c.scratch_bytes = bp.sk_bytes; }
  return c;
}

int chain_shape(const Who& who, const ron_head_chain_desc* d, int layer, int64_t nhwc[4]) {
  // (the whole plan, not the descriptor's checks alone: a shape is given for what the sizer and the calls accept)
  ChainPlan P;
  if (int rc = plan_chain(who, d, &P)) return rc;
  RON_REQUIRE(layer >= 0 && layer < d->num_layers, "%s: layer %d of %d", who.what, layer, d->num_layers);
  RON_REQUIRE(nhwc != nullptr, "%s: NULL shape", who.what);
  int h = d->h, w = d->w, c = d->cin;
  for (int i = 0; i <= layer; ++i) {
    const ron_head_chain_layer& l = d->layers[i];
    if (l.kind == RON_CHAIN_CONV) c = l.cout;
    else if (l.kind == RON_CHAIN_CONV_PAIR) c = l.cout + l.cout2;
    else if (l.kind == RON_CHAIN_POOL2) { h = (h + 1) / 2; w = (w + 1) / 2; }
  }
  nhwc[0] = d->n; nhwc[1] = h; nhwc[2] = w; nhwc[3] = c;
  return RON_OK;
}

int chain_forward(const Who& who, const ron_head_chain_desc* d, const float* x, const ron_head_chain_ptrs* p, float* y, void* workspace,
                  int64_t workspace_bytes, void* stream) {
  ChainPlan P;
  if (int rc = plan_chain(who, d, &P)) return rc;
  const char* what = who.what;
  const int L = P.L;
  RON_REQUIRE(x != nullptr && y != nullptr && p != nullptr, "%s forward: x, y or the layers' pointers are NULL", what);
  RON_REQUIRE(aligned16(x) && aligned16(y), "%s forward: x and y must be 16-byte aligned", what);
  for (int i = 0; i < L; ++i) {
    const ron_head_chain_layer& l = d->layers[i];
    const ron_head_chain_ptrs& q = p[i];
    if (l.kind == RON_CHAIN_BN) {
      RON_REQUIRE(q.gamma != nullptr && q.beta != nullptr, "%s forward: layer %d: gamma or beta is NULL", what, i);
      RON_REQUIRE((q.moving_mean == nullptr) == (q.moving_var == nullptr),
                  "%s forward: layer %d: moving_mean and moving_var come together (both, or both NULL)", what, i);
      RON_REQUIRE(aligned16(q.gamma) && aligned16(q.beta) && aligned16(q.moving_mean) && aligned16(q.moving_var) && aligned16(q.mean) && aligned16(q.var),
                  "%s forward: layer %d: gamma, beta, the moving statistics, mean and var must be 16-byte aligned", what, i);
      continue;
    }
    if (!is_conv(l.kind)) continue;
    RON_REQUIRE(q.w != nullptr, "%s forward: w[%d] is NULL", what, i);
    RON_REQUIRE(!l.has_bias || q.bias != nullptr, "%s forward: layer %d has a bias and bias[%d] is NULL", what, i, i);
    RON_REQUIRE(aligned4(q.w) && (!l.has_bias || aligned4(q.bias)), "%s forward: w[%d] and bias[%d] must be 4-byte aligned", what, i, i);
    if (l.kind == RON_CHAIN_CONV_PAIR) {
      RON_REQUIRE(q.w2 != nullptr && (!l.has_bias || q.bias2 != nullptr), "%s forward: layer %d: w2 (or bias2 of a layer with biases) is NULL", what, i);
      RON_REQUIRE(aligned4(q.w2) && (!l.has_bias || aligned4(q.bias2)), "%s forward: layer %d: w2 and bias2 must be 4-byte aligned", what, i);
    }
    RON_REQUIRE(!l.tap || q.tap != nullptr, "%s forward: layer %d is tapped and taps[%d] is NULL", what, i, i);
    RON_REQUIRE(!l.tap || aligned16(q.tap), "%s forward: taps[%d] must be 16-byte aligned", what, i);
  }
  if (int rc = check_workspace((std::string(what) + " forward").c_str(), who.sizer, workspace, workspace_bytes, P.total)) return rc;
  char* ws = static_cast<char*>(workspace);
  for (int i = 0; i < L; ++i)
    for (int b = 0; b < P.layer[i].nconv; ++b)
      if (int rc = describe(forward_launch(P.layer[i], b, ws), ws)) return rc;

  hipStream_t s = (hipStream_t)stream;
  int rc;
  const ChainAct& a0 = P.act[0];
  if ((rc = train_pack_halo(P.dtype, x, nullptr, ws + a0.off, a0.rows, P.n, a0.h, a0.w, a0.pad, a0.c, a0.c, a0.guard, s))) return rc;
  if (a0.rows2 > 0 && (rc = train_pack_halo(P.dtype, x, nullptr, ws + a0.off2, a0.rows2, P.n, a0.h, a0.w, a0.pad2, a0.c, a0.c, a0.guard2, s))) return rc;
  for (int i = 0; i < L; ++i) {
    const ron_head_chain_layer& l = d->layers[i];
    const ron_head_chain_ptrs& q = p[i];
    const ChainLayer& y0 = P.layer[i];
    const bool last = i == L - 1;
    TensorView out;
    bool wrote_next = true;       // the interior of activation i + 1 is in its buffer, nothing around it
    if (y0.nconv > 0) {
      for (int b = 0; b < y0.nconv; ++b) {
        const ConvLaunch c = forward_launch(y0, b, ws);
        const float* wb = b == 0 ? q.w : q.w2;
        const float* bb = !l.has_bias ? nullptr : b == 0 ? q.bias : q.bias2;
        if ((rc = train_forward_pack_w(&y0.conv[b].d, y0.conv[b].fp, c, wb, bb, ws, s))) return rc;
        if ((rc = launch_conv(c, s))) return rc;
        if (b == 0) out = c.out;
      }
      if (y0.nconv == 2) { out.C = y0.cout; out.coff = 0; }      // both slices: the layer's output
      if (l.tap && (rc = launch_unpack(out, P.dtype, 0, q.tap, s))) return rc;
      if (!last && !y0.direct) {
        // the consumer reads another halo: copy into its geometry, which writes every pixel of its buffer
        if ((rc = launch_rehalo(P, i + 1, out, false, ws, s))) return rc;
        wrote_next = false;
      }
    } else if (l.kind == RON_CHAIN_BN) {
      out = act_view(P, i + 1, ws);
      float* stats = reinterpret_cast<float*>(ws + y0.off_stats);
      if ((rc = bn_view_forward(&y0.bn, act_view(P, i, ws), out, q.gamma, q.beta, stats, stats + y0.bn.c, q.mean, q.var, q.moving_mean, q.moving_var,
                                ws + y0.off_bn, s)))
        return rc;
    } else {
      out = act_view(P, i + 1, ws);
      if ((rc = launch_maxpool2x2(act_view(P, i, ws), out, P.dtype, s))) return rc;
    }
    if (last) {
      if ((rc = launch_unpack(out, P.dtype, 0, y, s))) return rc;
    } else {
      if (wrote_next && P.act[i + 1].zero_fill && (rc = launch_zero(P, i + 1, ws, s))) return rc;
      // a pair reads the activation a second time, in its 1x1 branch's geometry
      if (P.act[i + 1].rows2 > 0 && (rc = launch_rehalo(P, i + 1, act_view(P, i + 1, ws), true, ws, s))) return rc;
    }
  }
  return RON_OK;
}

int chain_backward(const Who& who, const ron_head_chain_desc* d, const float* dy, const ron_head_chain_ptrs* p, float* dx, void* workspace,
                   int64_t workspace_bytes, void* stream) {
  ChainPlan P;
  if (int rc = plan_chain(who, d, &P)) return rc;
  const char* what = who.what;
  const int L = P.L;
  RON_REQUIRE(dy != nullptr && p != nullptr, "%s backward: dy or the layers' pointers are NULL", what);
  RON_REQUIRE(aligned16(dy) && aligned16(dx), "%s backward: dy and dx must be 16-byte aligned", what);
  for (int i = 0; i < L; ++i) {
    const ron_head_chain_layer& l = d->layers[i];
    const ron_head_chain_ptrs& q = p[i];
    if (l.kind == RON_CHAIN_BN) {
      RON_REQUIRE(q.gamma != nullptr, "%s backward: layer %d: gamma is NULL", what, i);
      RON_REQUIRE(aligned16(q.gamma) && aligned16(q.dgamma) && aligned16(q.dbeta), "%s backward: layer %d: gamma, dgamma and dbeta must be 16-byte aligned", what, i);
      continue;
    }
    if (!is_conv(l.kind)) continue;
    RON_REQUIRE(q.w != nullptr, "%s backward: w[%d] is NULL", what, i);
    RON_REQUIRE(aligned4(q.w), "%s backward: w[%d] must be 4-byte aligned", what, i);
    RON_REQUIRE(!l.tap || aligned16(q.dtap), "%s backward: dtaps[%d] must be 16-byte aligned", what, i);
    RON_REQUIRE(aligned4(q.dw), "%s backward: dw[%d] must be 4-byte aligned", what, i);
    RON_REQUIRE(aligned4(q.dbias), "%s backward: dbias[%d] must be 4-byte aligned", what, i);
    if (l.kind == RON_CHAIN_CONV_PAIR) {
      RON_REQUIRE(q.w2 != nullptr, "%s backward: layer %d: w2 is NULL", what, i);
      RON_REQUIRE(aligned4(q.w2) && aligned4(q.dw2) && aligned4(q.dbias2), "%s backward: layer %d: w2, dw2 and dbias2 must be 4-byte aligned", what, i);
    }
  }
  if (int rc = check_workspace((std::string(what) + " backward").c_str(), who.sizer, workspace, workspace_bytes, P.total)) return rc;
  char* ws = static_cast<char*>(workspace);
  // need[j]: somebody wants the gradient of activation j - the caller (dx), or a layer in front of it (a parameter gradient or its dx)
  bool need[RON_CHAIN_MAX_LAYERS + 1];
  need[0] = dx != nullptr;
  for (int i = 0; i < L; ++i) {
    const ron_head_chain_ptrs& q = p[i];
    const int kind = d->layers[i].kind;
    bool wants = false;
    if (is_conv(kind)) wants = q.dw != nullptr || q.dbias != nullptr;
    if (kind == RON_CHAIN_CONV_PAIR) wants = wants || q.dw2 != nullptr || q.dbias2 != nullptr;
    if (kind == RON_CHAIN_BN) wants = q.dgamma != nullptr || q.dbeta != nullptr;
    need[i + 1] = need[i] || wants;
  }
  for (int i = 0; i < L; ++i)
    for (int b = 0; b < P.layer[i].nconv && need[i]; ++b)
      if (int rc = describe(data_grad_launch(P.layer[i].conv[b].bp, ws), ws)) return rc;

  hipStream_t s = (hipStream_t)stream;
  int rc;
  for (int i = L - 1; i >= 0; --i) {
    if (!need[i + 1]) break;        // nothing in front of here is wanted either
    const ron_head_chain_layer& l = d->layers[i];
    const ron_head_chain_ptrs& q = p[i];
    const ChainLayer& y0 = P.layer[i];
    const bool last = i == L - 1;
    const bool two = !last && P.layer[i + 1].nconv == 2;      // the gradient of activation i + 1 is the sum of a pair's two data gradients
    if (y0.nconv == 0) {
      if (l.kind == RON_CHAIN_POOL2 && !need[i]) break;
      TensorView g = grad_view(P, i + 1, ws);
      if (last) {
        // the chain's own dy enters through the pack (rounded to the storage type, as the operators round it)
        if ((rc = train_pack_halo(P.dtype, dy, nullptr, g.base, g.pixels(), P.n, g.H, g.W, 1, g.C, g.C, 0, s))) return rc;
      } else if (two) {
        // round(float(a) + float(b)), in place: every lane reads the element it writes
        const TensorView g2 = grad_view(P, i + 1, ws, true);
        PairJoinArgs args = PairJoinArgs();
        JoinArgs& a = args.j;
        a.g = static_cast<const unsigned short*>(g.base); a.gpad = g.pad; a.gcs = g.cstride;
        args.g2 = static_cast<const unsigned short*>(g2.base); args.g2pad = g2.pad; args.g2cs = g2.cstride;
        a.out = static_cast<unsigned short*>(g.base);
        a.rows = g.pixels(); a.guard = 0;
        a.N = P.n; a.H = g.H; a.W = g.W; a.pad = 1; a.Csrc = g.C; a.Cdst = g.C;
        if ((rc = launch_join(P.dtype, args, s))) return rc;
      }
      if (l.kind == RON_CHAIN_POOL2) {
        if ((rc = launch_pool_bwd(P.dtype, act_view(P, i, ws), g, grad_view(P, i, ws), s))) return rc;
      } else {
        const float* stats = reinterpret_cast<const float*>(ws + y0.off_stats);
        const TensorView gx = grad_view(P, i, ws);
        if ((rc = bn_view_backward(&y0.bn, act_view(P, i, ws), act_view(P, i + 1, ws), g, q.gamma, stats, stats + y0.bn.c, need[i] ? &gx : nullptr,
                                   q.dgamma, q.dbeta, ws + y0.off_bn, s)))
          return rc;
      }
      continue;
    }
    for (int b = 0; b < y0.nconv; ++b) {
      const ChainConv& v = y0.conv[b];
      const BackwardPlan& bp = v.bp;
      char* dzbuf = ws + bp.off_dz;
      PairJoinArgs args = PairJoinArgs();
      JoinArgs& a = args.j;
      if (last) {
        a.add1 = dy + v.coff;
        if (y0.nconv == 2) args.dcs = y0.cout;
        if (l.tap && q.dtap != nullptr) a.add2 = q.dtap;
      } else {
        const TensorView g = grad_view(P, i + 1, ws);
        a.g = static_cast<const unsigned short*>(g.base) + v.coff; a.gpad = g.pad; a.gcs = g.cstride;
        if (two) {
          const TensorView g2 = grad_view(P, i + 1, ws, true);
          args.g2 = static_cast<const unsigned short*>(g2.base) + v.coff; args.g2pad = g2.pad; args.g2cs = g2.cstride;
        }
        if (l.tap && q.dtap != nullptr) a.add1 = q.dtap;
      }
      if (l.relu) {
        const TensorView m = act_view(P, i + 1, ws);
        a.mask = static_cast<const unsigned short*>(m.base) + v.coff; a.mpad = m.pad; a.mcs = m.cstride;
      }
      a.out = reinterpret_cast<unsigned short*>(dzbuf);
      a.rows = bp.rows; a.guard = 0;
      a.N = P.n; a.H = v.d.h; a.W = v.d.w; a.pad = bp.pad; a.Csrc = v.d.cout; a.Cdst = bp.cop;
      if ((rc = launch_join(P.dtype, args, s))) return rc;
      const float* wb = b == 0 ? q.w : q.w2;
      float* dwb = b == 0 ? q.dw : q.dw2;
      float* dbb = b == 0 ? q.dbias : q.dbias2;
      if (need[i]) {
        if ((rc = train_backward_pack_w(&v.d, bp, wb, ws, s))) return rc;
        TensorView out;
        if ((rc = train_data_grad(bp, dzbuf, ws, s, &out))) return rc;
      }
      if (dwb != nullptr && (rc = train_weight_grad(bp, ws + bp.off_x, dzbuf, dwb, ws, s))) return rc;
      if (dbb != nullptr && (rc = train_bias_grad(P.dtype, bp, dzbuf, ws, v.d.cout, dbb, s))) return rc;
    }
  }
  if (dx != nullptr) {
    // a pair as the first layer: dx = float(dx of the 3x3) + float(dx of the 1x1), unrounded
    if (P.layer[0].nconv == 2) rc = launch_add_unpack(P.dtype, grad_view(P, 0, ws), grad_view(P, 0, ws, true), dx, s);
    else rc = launch_unpack(grad_view(P, 0, ws), P.dtype, 0, dx, s);
    if (rc) return rc;
  }
  return RON_OK;
}

// what the convolution chain's entry points ask before they read num_layers entries of the caller's arrays
int check_layer_count(const ron_chain_desc* d) {
  RON_REQUIRE(d != nullptr, "conv chain: NULL descriptor");
  RON_REQUIRE(d->num_layers >= 1 && d->num_layers <= RON_CHAIN_MAX_LAYERS, "conv chain: num_layers %d: 1 .. %d", d->num_layers, RON_CHAIN_MAX_LAYERS);
  return RON_OK;
}

// ron_chain_desc and its parallel arrays in the head chain's form (the layers a refused num_layers leaves out are never read)
void widen(const ron_chain_desc* d, ron_head_chain_desc* o) {
  *o = ron_head_chain_desc();
  o->n = d->n; o->h = d->h; o->w = d->w; o->cin = d->cin; o->dtype = d->dtype; o->num_layers = d->num_layers;
  for (int i = 0; i < std::min(std::max(d->num_layers, 0), RON_CHAIN_MAX_LAYERS); ++i) {
    const ron_chain_layer& l = d->layers[i];
    ron_head_chain_layer& t = o->layers[i];
    t.kind = l.kind; t.k = l.k; t.dilation = l.dilation; t.cout = l.cout; t.relu = l.relu; t.has_bias = l.has_bias; t.tap = l.tap;
  }
}

}  // namespace
}  // namespace ron

extern "C" int ron_conv_chain_shape(const ron_chain_desc* d, int layer, int64_t nhwc[4]) {
  using namespace ron;
  RON_REQUIRE(d != nullptr, "conv chain: NULL descriptor");
  ron_head_chain_desc hd;
  widen(d, &hd);
  return chain_shape(kConvChain, &hd, layer, nhwc);
}

extern "C" int64_t ron_conv_chain_workspace_bytes(const ron_chain_desc* d) {
  using namespace ron;
  RON_REQUIRE(d != nullptr, "conv chain: NULL descriptor");
  ron_head_chain_desc hd;
  widen(d, &hd);
  ChainPlan P;
  if (plan_chain(kConvChain, &hd, &P) != RON_OK) return -1;
  return P.total;
}

extern "C" int ron_conv_chain_forward(const ron_chain_desc* d, const float* x, const float* const* w, const float* const* bias,
                                      float* const* taps, float* y, void* workspace, int64_t workspace_bytes, void* stream) {
  using namespace ron;
  if (int rc = check_layer_count(d)) return rc;
  RON_REQUIRE(w != nullptr, "conv chain forward: x, y or w is NULL");
  ron_head_chain_desc hd;
  widen(d, &hd);
  {
    ChainPlan P;        // the descriptor is refused before any entry of the caller's arrays is read
    if (int rc = plan_chain(kConvChain, &hd, &P)) return rc;
  }
  ron_head_chain_ptrs p[RON_CHAIN_MAX_LAYERS];
  for (int i = 0; i < RON_CHAIN_MAX_LAYERS; ++i) {
    p[i] = ron_head_chain_ptrs();
    if (i >= d->num_layers) continue;
    p[i].w = w[i];
    if (bias != nullptr) p[i].bias = bias[i];
    if (taps != nullptr) p[i].tap = taps[i];
  }
  return chain_forward(kConvChain, &hd, x, p, y, workspace, workspace_bytes, stream);
}

extern "C" int ron_conv_chain_backward(const ron_chain_desc* d, const float* dy, const float* const* dtaps, const float* const* w,
                                       float* dx, float* const* dw, float* const* dbias, void* workspace, int64_t workspace_bytes,
                                       void* stream) {
  using namespace ron;
  if (int rc = check_layer_count(d)) return rc;
  RON_REQUIRE(w != nullptr, "conv chain backward: dy or w is NULL");
  ron_head_chain_desc hd;
  widen(d, &hd);
  {
    ChainPlan P;        // the descriptor is refused before any entry of the caller's arrays is read
    if (int rc = plan_chain(kConvChain, &hd, &P)) return rc;
  }
  ron_head_chain_ptrs p[RON_CHAIN_MAX_LAYERS];
  for (int i = 0; i < RON_CHAIN_MAX_LAYERS; ++i) {
    p[i] = ron_head_chain_ptrs();
    if (i >= d->num_layers) continue;
    p[i].w = w[i];
    if (dtaps != nullptr) p[i].dtap = dtaps[i];
    if (dw != nullptr) p[i].dw = dw[i];
    if (dbias != nullptr) p[i].dbias = dbias[i];
  }
  return chain_backward(kConvChain, &hd, dy, p, dx, workspace, workspace_bytes, stream);
}

extern "C" int ron_head_chain_shape(const ron_head_chain_desc* d, int layer, int64_t nhwc[4]) {
  return ron::chain_shape(ron::kHeadChain, d, layer, nhwc);
}

extern "C" int64_t ron_head_chain_workspace_bytes(const ron_head_chain_desc* d) {
  ron::ChainPlan P;
  if (ron::plan_chain(ron::kHeadChain, d, &P) != RON_OK) return -1;
  return P.total;
}

extern "C" int ron_head_chain_forward(const ron_head_chain_desc* d, const float* x, const ron_head_chain_ptrs* p, float* y, void* workspace,
                                      int64_t workspace_bytes, void* stream) {
  return ron::chain_forward(ron::kHeadChain, d, x, p, y, workspace, workspace_bytes, stream);
}

extern "C" int ron_head_chain_backward(const ron_head_chain_desc* d, const float* dy, const ron_head_chain_ptrs* p, float* dx, void* workspace,
                                       int64_t workspace_bytes, void* stream) {
  return ron::chain_backward(ron::kHeadChain, d, dy, p, dx, workspace, workspace_bytes, stream);
}
