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
#include <hip/hip_runtime.h>

#include <algorithm>

#include "conv_mfma.h"
#include "conv_train.h"
#include "storage_device.h"      // the roundings, pack8 / unpack8, the halo walk, the pool's first maximum

namespace ron {
namespace {

// ---- the join: out(buffer of `rows` pixels, halo pixel 0 at pixel `guard`) = round((float(g) + add1 + add2) * (mask > 0)) ----------------
// g and mask are halo tensors of the map (their own halo and pixel stride), add1 / add2 dense fp32 [N,H,W,Csrc]; each may be null.
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

template <bool BF16>
__global__ __launch_bounds__(256) void chain_join_kernel(JoinArgs a) {
  // (every buffer of the chain is below 2 GiB, plan_chain: the 16-byte pieces and the pixels fit 32-bit arithmetic)
  const unsigned vecs = a.Cdst / 8;
  const unsigned total = (unsigned)a.rows * vecs;
  const bool vec_ok = a.Csrc % 8 == 0;
  const bool copy = a.add1 == nullptr && a.add2 == nullptr && a.mask == nullptr;
  for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    const unsigned b = i / vecs;
    const int c0 = (int)(i - b * vecs) * 8;
    uint4 o = {0u, 0u, 0u, 0u};
    HaloPixel p = {false, 0u, 0, 0};
    if (c0 < a.Csrc) p = halo_pixel(b, a.guard, a.N, a.H, a.W, a.pad);
    if (p.inside) {
      const long long img = p.img;
      const int y = p.y, x = p.x;
      const long long dense = (((long long)img * a.H + y) * a.W + x) * a.Csrc + c0;
      const long long go = a.g != nullptr ? halo_off(img, y, x, a.H, a.W, a.gpad, a.gcs) + c0 : 0;
      const long long mo = a.mask != nullptr ? halo_off(img, y, x, a.H, a.W, a.mpad, a.mcs) + c0 : 0;
      if (vec_ok && copy) {
        o = *reinterpret_cast<const uint4*>(a.g + go);
      } else {
        float f[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if (vec_ok) {
          float t[8];
          if (a.g != nullptr) unpack8<BF16>(*reinterpret_cast<const uint4*>(a.g + go), f);
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
// Activation j (0: the chain's input, j: the output of layer j - 1) in the geometry of its consumer, layer j.  The buffer is
// [guard][rows][guard] pixels of c channels; the view starts `guard` pixels in.
struct ChainAct {
  int h = 0, w = 0, c = 0, pad = 0;
  int64_t guard = 0, pixels = 0, rows = 0, off = 0;
  bool zero_fill = false;       // a convolution reads it: halos, guards and tail must be zero
  int64_t bytes() const { return (rows + 2 * guard) * c * 2; }
  int64_t view_off() const { return off + guard * c * 2; }
};

struct ChainLayer {
  ron_conv_desc d;              // convolution layers only
  ForwardPlan fp;
  BackwardPlan bp;
  bool direct = false;          // the forward writes activation i + 1 itself (else: the staging tensor, then a re-halo copy)
  int64_t off_stage = 0;
};

struct ChainPlan {
  int L = 0, dtype = 0, n = 0;
  ChainAct act[RON_CHAIN_MAX_LAYERS + 1];
  ChainLayer layer[RON_CHAIN_MAX_LAYERS];
  int64_t off_g[2] = {0, 0}, g_bytes = 0;       // the gradient of activation j is in buffer j & 1, halo 1
  int64_t off_scratch = 0, scratch_bytes = 0;
  int64_t total = 0;
};

int check_chain_desc(const ron_chain_desc* d) {
  RON_REQUIRE(d != nullptr, "conv chain: NULL descriptor");
  RON_REQUIRE(d->num_layers >= 1 && d->num_layers <= RON_CHAIN_MAX_LAYERS, "conv chain: num_layers %d: 1 .. %d", d->num_layers, RON_CHAIN_MAX_LAYERS);
  RON_REQUIRE(d->dtype == RON_DTYPE_BF16 || d->dtype == RON_DTYPE_F16, "conv chain: dtype %d: bf16 or fp16 only (fp32 and f16x3 have no backward)", d->dtype);
  RON_REQUIRE(d->n >= 1 && d->h >= 1 && d->w >= 1, "conv chain: empty tensor (n %d, h %d, w %d)", d->n, d->h, d->w);
  RON_REQUIRE(d->cin >= 64 && d->cin % 64 == 0, "conv chain: cin %d must be a multiple of 64 (the 3-channel stem is out of scope)", d->cin);
  for (int i = 0; i < d->num_layers; ++i) {
    const ron_chain_layer& l = d->layers[i];
    RON_REQUIRE(l.kind == RON_CHAIN_CONV || l.kind == RON_CHAIN_POOL2, "conv chain: layer %d: unknown kind %d", i, l.kind);
    RON_REQUIRE(l.tap == 0 || l.tap == 1, "conv chain: layer %d: tap %d: 0 or 1", i, l.tap);
    if (l.kind == RON_CHAIN_POOL2) {
      RON_REQUIRE(l.tap == 0, "conv chain: layer %d: a pool cannot be tapped (tap the convolution in front of it and pool the tap)", i);
      continue;
    }
    RON_REQUIRE(l.k == 1 || l.k == 3 || (l.k == 7 && l.dilation == 1), "conv chain: layer %d: filter %d x %d at dilation %d: 1 x 1, 3 x 3, or 7 x 7 at dilation 1 only",
                i, l.k, l.k, l.dilation);
    RON_REQUIRE(l.dilation >= 1 && l.dilation <= kConvMaxDilation, "conv chain: layer %d: dilation %d: 1 .. %d", i, l.dilation, kConvMaxDilation);
    RON_REQUIRE((l.relu == 0 || l.relu == 1) && (l.has_bias == 0 || l.has_bias == 1), "conv chain: layer %d: relu and has_bias are 0 or 1", i);
    RON_REQUIRE(l.cout >= 1, "conv chain: layer %d: cout %d", i, l.cout);
    RON_REQUIRE(i == d->num_layers - 1 || l.cout % 64 == 0, "conv chain: layer %d: cout %d must be a multiple of 64 on a layer that feeds another one", i, l.cout);
  }
  return RON_OK;
}

int plan_chain(const ron_chain_desc* d, ChainPlan* P) {
  if (int rc = check_chain_desc(d)) return rc;
  const int L = d->num_layers;
  const int64_t lim = (int64_t)1 << 31;
  P->L = L; P->dtype = d->dtype; P->n = d->n;
  int h = d->h, w = d->w, c = d->cin;
  int64_t fwd_scratch = 0, bwd_scratch = 0;
  for (int j = 0; j <= L; ++j) {
    ChainAct& a = P->act[j];
    a.h = h; a.w = w; a.c = c;
    const bool conv_reads = j < L && d->layers[j].kind == RON_CHAIN_CONV;
    if (conv_reads) {
      const ron_chain_layer& l = d->layers[j];
      ChainLayer& y = P->layer[j];
      ron_conv_desc& cd = y.d;
      cd = ron_conv_desc();
      cd.n = d->n; cd.h = h; cd.w = w; cd.cin = c; cd.cout = l.cout;
      cd.kh = cd.kw = l.k; cd.stride = 1; cd.dilation = l.dilation; cd.relu = l.relu;
      cd.dtype = d->dtype; cd.tile_cfg = -1; cd.splitk = -1;
      if (int rc = train_plan_forward(&cd, &y.fp)) return rc;
      if (int rc = train_plan_backward(&cd, &y.bp)) return rc;
      a.pad = y.bp.pad;
      a.guard = align_up(y.bp.guard, 2);        // (an even number of pixels: the view stays 256-byte aligned)
      a.pixels = y.bp.pixels;
      a.rows = y.bp.rows;
      a.zero_fill = true;
      c = l.cout;
    } else {
      // a pool reads interiors only; the chain's output has the halo a convolution writes with
      a.pad = 1;
      a.pixels = TensorView::halo_pixels(d->n, h, w, 1);
      a.rows = a.pixels;
      if (j < L) { h = (h + 1) / 2; w = (w + 1) / 2; }
    }
    RON_REQUIRE(a.bytes() < lim, "conv chain: activation %d (%d x %d x %d x %d) would reach 2 GiB", j, d->n, a.h, a.w, a.c);
    a.off = carve(&P->total, a.bytes());
    P->g_bytes = std::max(P->g_bytes, TensorView::halo_pixels(d->n, a.h, a.w, 1) * (int64_t)a.c * 2);
  }
  RON_REQUIRE(P->g_bytes < lim, "conv chain: a gradient tensor would reach 2 GiB");
  for (int i = 0; i < L; ++i) {
    if (d->layers[i].kind != RON_CHAIN_CONV) continue;
    ChainLayer& y = P->layer[i];
    const bool last = i == L - 1;
    y.direct = !last && P->act[i + 1].pad == 1;
    // the layer's share of the scratch region, re-carved from offset 0: the forward's packs, split-K slabs and staging tensor ...
    int64_t t = 0;
    auto take = [&t](int64_t bytes) { const int64_t o = t; t += align_up(bytes, 256); return o; };
    y.fp.off_w = take(y.fp.w_bytes);
    y.fp.off_c64 = take(y.fp.c64_bytes);
    y.fp.off_bias = take((int64_t)y.fp.bias_total * 4);
    y.fp.off_sk = take(y.fp.sk_bytes);
    y.off_stage = take(y.direct || last ? 0 : y.fp.out_bytes);
    fwd_scratch = std::max(fwd_scratch, t);
    // ... and the backward's: dz, the flipped weights, the zero bias, split-K slabs, pixel-slice slabs, column-sum partials
    t = 0;
    y.bp.off_dz = take(y.bp.rows * y.bp.cop * 2);
    y.bp.off_w = take(y.bp.w_bytes);
    y.bp.off_bias = take((int64_t)y.bp.conv.Npad * 4);
    y.bp.off_sk = take(y.bp.sk_bytes);
    y.bp.off_slab = take(y.bp.slab_bytes);
    y.bp.off_part = take((int64_t)y.bp.chunks * y.bp.sum_cols * 4);
    bwd_scratch = std::max(bwd_scratch, t);
  }
  P->off_g[0] = carve(&P->total, P->g_bytes);
  P->off_g[1] = carve(&P->total, P->g_bytes);
  P->scratch_bytes = std::max(fwd_scratch, bwd_scratch);
  P->off_scratch = carve(&P->total, P->scratch_bytes);
  // every layer offset becomes an offset from the workspace's base
  for (int i = 0; i < L; ++i) {
    if (d->layers[i].kind != RON_CHAIN_CONV) continue;
    ChainLayer& y = P->layer[i];
    const int64_t s = P->off_scratch;
    y.fp.off_w += s; y.fp.off_c64 += s; y.fp.off_bias += s; y.fp.off_sk += s; y.off_stage += s;
    y.fp.off_x = P->act[i].view_off();
    y.fp.off_out = i == L - 1 || y.direct ? P->act[i + 1].view_off() : y.off_stage;
    y.bp.off_dz += s; y.bp.off_w += s; y.bp.off_bias += s; y.bp.off_sk += s; y.bp.off_slab += s; y.bp.off_part += s;
    y.bp.off_x = P->act[i].view_off();
    y.bp.off_dx = P->off_g[i & 1];
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

// the gradient of activation j: halo 1, in buffer j & 1
TensorView grad_view(const ChainPlan& P, int j, char* ws) {
  const ChainAct& a = P.act[j];
  TensorView v;
  v.base = ws + P.off_g[j & 1];
  v.N = P.n; v.H = a.h; v.W = a.w; v.C = a.c; v.cstride = a.c; v.coff = 0; v.pad = 1;
  v.bytes = TensorView::halo_pixels(P.n, a.h, a.w, 1) * a.c * 2;
  return v;
}

int launch_join(int dtype, const JoinArgs& a, hipStream_t s) {
  const int grid = grid_for(a.rows * (a.Cdst / 8));
  if (dtype == RON_DTYPE_BF16) RON_LAUNCH(chain_join_kernel<true>, dim3(grid), dim3(256), 0, s, a);
  else RON_LAUNCH(chain_join_kernel<false>, dim3(grid), dim3(256), 0, s, a);
  RON_HIP_CHECK(ron::launch_error());
  return RON_OK;
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

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// what launch_conv would refuse is refused before anything is enqueued
int describe(ConvLaunch c, char* ws) {
  if (c.bias == nullptr) c.bias = reinterpret_cast<const float*>(ws);
  int o[4];
  return conv_describe(c, o);
}

ConvLaunch data_grad_launch(const BackwardPlan& bp, char* ws) {
  ConvLaunch c = bp.conv;
  c.in.base = ws + bp.off_dz; c.out.base = ws + bp.off_dx;
  c.wgt = ws + bp.off_w; c.bias = reinterpret_cast<const float*>(ws + bp.off_bias);
  if (bp.sk_bytes > 0) { c.scratch = ws + bp.off_sk; c.scratch_bytes = bp.sk_bytes; }
  return c;
}

}  // namespace
}  // namespace ron

extern "C" int ron_conv_chain_shape(const ron_chain_desc* d, int layer, int64_t nhwc[4]) {
  using namespace ron;
  if (int rc = check_chain_desc(d)) return rc;
  RON_REQUIRE(layer >= 0 && layer < d->num_layers, "conv chain: layer %d of %d", layer, d->num_layers);
  RON_REQUIRE(nhwc != nullptr, "conv chain: NULL shape");
  int h = d->h, w = d->w, c = d->cin;
  for (int i = 0; i <= layer; ++i) {
    if (d->layers[i].kind == RON_CHAIN_CONV) c = d->layers[i].cout;
    else { h = (h + 1) / 2; w = (w + 1) / 2; }
  }
  nhwc[0] = d->n; nhwc[1] = h; nhwc[2] = w; nhwc[3] = c;
  return RON_OK;
}

extern "C" int64_t ron_conv_chain_workspace_bytes(const ron_chain_desc* d) {
  ron::ChainPlan P;
  if (ron::plan_chain(d, &P) != RON_OK) return -1;
  return P.total;
}

extern "C" int ron_conv_chain_forward(const ron_chain_desc* d, const float* x, const float* const* w, const float* const* bias,
                                      float* const* taps, float* y, void* workspace, int64_t workspace_bytes, void* stream) {
  using namespace ron;
  ChainPlan P;
  if (int rc = plan_chain(d, &P)) return rc;
  const int L = P.L;
  RON_REQUIRE(x != nullptr && y != nullptr && w != nullptr, "conv chain forward: x, y or w is NULL");
  RON_REQUIRE(aligned16(x) && aligned16(y), "conv chain forward: x and y must be 16-byte aligned");
  for (int i = 0; i < L; ++i) {
    const ron_chain_layer& l = d->layers[i];
    if (l.kind != RON_CHAIN_CONV) continue;
    RON_REQUIRE(w[i] != nullptr, "conv chain forward: w[%d] is NULL", i);
    RON_REQUIRE(!l.has_bias || (bias != nullptr && bias[i] != nullptr), "conv chain forward: layer %d has a bias and bias[%d] is NULL", i, i);
    RON_REQUIRE((((uintptr_t)w[i] | (uintptr_t)(l.has_bias ? bias[i] : nullptr)) & 3) == 0, "conv chain forward: w[%d] and bias[%d] must be 4-byte aligned", i, i);
    RON_REQUIRE(!l.tap || (taps != nullptr && taps[i] != nullptr), "conv chain forward: layer %d is tapped and taps[%d] is NULL", i, i);
    RON_REQUIRE(!l.tap || aligned16(taps[i]), "conv chain forward: taps[%d] must be 16-byte aligned", i);
  }
  if (int rc = check_workspace("conv chain forward", "ron_conv_chain_workspace_bytes", workspace, workspace_bytes, P.total)) return rc;
  char* ws = static_cast<char*>(workspace);
  for (int i = 0; i < L; ++i)
    if (d->layers[i].kind == RON_CHAIN_CONV)
      if (int rc = describe(train_forward_launch(P.layer[i].fp, ws), ws)) return rc;

  hipStream_t s = (hipStream_t)stream;
  int rc;
  const ChainAct& a0 = P.act[0];
  if ((rc = train_pack_halo(P.dtype, x, nullptr, ws + a0.off, a0.rows, P.n, a0.h, a0.w, a0.pad, a0.c, a0.c, a0.guard, s))) return rc;
  for (int i = 0; i < L; ++i) {
    const ron_chain_layer& l = d->layers[i];
    const bool last = i == L - 1;
    TensorView out;
    bool wrote_next = true;       // the interior of activation i + 1 is in its buffer, nothing around it
    if (l.kind == RON_CHAIN_CONV) {
      const ChainLayer& y0 = P.layer[i];
      const ConvLaunch c = train_forward_launch(y0.fp, ws);
      if ((rc = train_forward_pack_w(&y0.d, y0.fp, c, w[i], l.has_bias ? bias[i] : nullptr, ws, s))) return rc;
      if ((rc = launch_conv(c, s))) return rc;
      out = c.out;
      if (l.tap && (rc = launch_unpack(out, P.dtype, 0, taps[i], s))) return rc;
      if (!last && !y0.direct) {
        // the consumer reads another halo: copy into its geometry, which writes every pixel of its buffer
        const ChainAct& t = P.act[i + 1];
        JoinArgs a = JoinArgs();
        a.g = static_cast<const unsigned short*>(out.base); a.gpad = out.pad; a.gcs = out.cstride;
        a.out = reinterpret_cast<unsigned short*>(ws + t.off);
        a.rows = t.rows + 2 * t.guard; a.guard = t.guard;
        a.N = P.n; a.H = t.h; a.W = t.w; a.pad = t.pad; a.Csrc = t.c; a.Cdst = t.c;
        if ((rc = launch_join(P.dtype, a, s))) return rc;
        wrote_next = false;
      }
    } else {
      out = act_view(P, i + 1, ws);
      if ((rc = launch_maxpool2x2(act_view(P, i, ws), out, P.dtype, s))) return rc;
    }
    if (last) {
      if ((rc = launch_unpack(out, P.dtype, 0, y, s))) return rc;
    } else if (wrote_next && P.act[i + 1].zero_fill) {
      if ((rc = launch_zero(P, i + 1, ws, s))) return rc;
    }
  }
  return RON_OK;
}

extern "C" int ron_conv_chain_backward(const ron_chain_desc* d, const float* dy, const float* const* dtaps, const float* const* w,
                                       float* dx, float* const* dw, float* const* dbias, void* workspace, int64_t workspace_bytes,
                                       void* stream) {
  using namespace ron;
  ChainPlan P;
  if (int rc = plan_chain(d, &P)) return rc;
  const int L = P.L;
  RON_REQUIRE(dy != nullptr && w != nullptr, "conv chain backward: dy or w is NULL");
  RON_REQUIRE(aligned16(dy) && aligned16(dx), "conv chain backward: dy and dx must be 16-byte aligned");
  for (int i = 0; i < L; ++i) {
    const ron_chain_layer& l = d->layers[i];
    if (l.kind != RON_CHAIN_CONV) continue;
    RON_REQUIRE(w[i] != nullptr, "conv chain backward: w[%d] is NULL", i);
    RON_REQUIRE(((uintptr_t)w[i] & 3) == 0, "conv chain backward: w[%d] must be 4-byte aligned", i);
    RON_REQUIRE(!l.tap || dtaps == nullptr || aligned16(dtaps[i]), "conv chain backward: dtaps[%d] must be 16-byte aligned", i);
    RON_REQUIRE(dw == nullptr || ((uintptr_t)dw[i] & 3) == 0, "conv chain backward: dw[%d] must be 4-byte aligned", i);
    RON_REQUIRE(dbias == nullptr || ((uintptr_t)dbias[i] & 3) == 0, "conv chain backward: dbias[%d] must be 4-byte aligned", i);
  }
  if (int rc = check_workspace("conv chain backward", "ron_conv_chain_workspace_bytes", workspace, workspace_bytes, P.total)) return rc;
  char* ws = static_cast<char*>(workspace);
  // need[j]: somebody wants the gradient of activation j - the caller (dx), or a convolution in front of it (its dw, dbias or dx)
  bool need[RON_CHAIN_MAX_LAYERS + 1];
  need[0] = dx != nullptr;
  for (int i = 0; i < L; ++i) {
    const bool conv = d->layers[i].kind == RON_CHAIN_CONV;
    need[i + 1] = need[i] || (conv && ((dw != nullptr && dw[i] != nullptr) || (dbias != nullptr && dbias[i] != nullptr)));
  }
  for (int i = 0; i < L; ++i)
    if (d->layers[i].kind == RON_CHAIN_CONV && need[i])
      if (int rc = describe(data_grad_launch(P.layer[i].bp, ws), ws)) return rc;

  hipStream_t s = (hipStream_t)stream;
  int rc;
  for (int i = L - 1; i >= 0; --i) {
    if (!need[i + 1]) break;        // nothing in front of here is wanted either
    const ron_chain_layer& l = d->layers[i];
    const bool last = i == L - 1;
    if (l.kind == RON_CHAIN_POOL2) {
      if (!need[i]) break;
      TensorView g = grad_view(P, i + 1, ws);
      // the chain's own dy enters through the pack (rounded to the storage type, as ron_maxpool2x2_backward_nhwc rounds it)
      if (last && (rc = train_pack_halo(P.dtype, dy, nullptr, g.base, g.pixels(), P.n, g.H, g.W, 1, g.C, g.C, 0, s))) return rc;
      if ((rc = launch_pool_bwd(P.dtype, act_view(P, i, ws), g, grad_view(P, i, ws), s))) return rc;
      continue;
    }
    const ChainLayer& y0 = P.layer[i];
    const BackwardPlan& bp = y0.bp;
    char* dzbuf = ws + bp.off_dz;
    JoinArgs a = JoinArgs();
    if (last) {
      a.add1 = dy;
      if (l.tap && dtaps != nullptr) a.add2 = dtaps[i];
    } else {
      const TensorView g = grad_view(P, i + 1, ws);
      a.g = static_cast<const unsigned short*>(g.base); a.gpad = g.pad; a.gcs = g.cstride;
      if (l.tap && dtaps != nullptr) a.add1 = dtaps[i];
    }
    if (l.relu) {
      const TensorView m = act_view(P, i + 1, ws);
      a.mask = static_cast<const unsigned short*>(m.base); a.mpad = m.pad; a.mcs = m.cstride;
    }
    a.out = reinterpret_cast<unsigned short*>(dzbuf);
    a.rows = bp.rows; a.guard = 0;
    a.N = P.n; a.H = y0.d.h; a.W = y0.d.w; a.pad = bp.pad; a.Csrc = y0.d.cout; a.Cdst = bp.cop;
    if ((rc = launch_join(P.dtype, a, s))) return rc;
    if (need[i]) {
      if ((rc = train_backward_pack_w(&y0.d, bp, w[i], ws, s))) return rc;
      TensorView out;
      if ((rc = train_data_grad(bp, dzbuf, ws, s, &out))) return rc;
    }
    if (dw != nullptr && dw[i] != nullptr && (rc = train_weight_grad(bp, ws + bp.off_x, dzbuf, dw[i], ws, s))) return rc;
    if (dbias != nullptr && dbias[i] != nullptr && (rc = train_bias_grad(P.dtype, bp, dzbuf, ws, y0.d.cout, dbias[i], s))) return rc;
  }
  if (dx != nullptr && (rc = launch_unpack(grad_view(P, 0, ws), P.dtype, 0, dx, s))) return rc;
  return RON_OK;
}
