// Backward of the stride-1 SAME convolution (ron_conv2d_backward_nhwc): data, weight and bias gradients.  The padded 3x3 convolutions
// of the SSD extra blocks (ron_conv2d_padded_backward_nhwc) reuse it behind a scattering pack of dz, the 2x2 stride-2 convolution and
// transposed convolution (ron_conv2d_k2s2_backward_nhwc) reuse its kernels on space-to-depth views: the last two sections of this file.
//
//   dz    = round(dy * (y > 0))                              pack_halo_kernel (ReLU mask fused), a halo tensor of the storage type
//   dx    = round(conv_SAME(dz, flipped / swapped weights))  launch_conv on dz (the forward's kernels), weights packed ON THE DEVICE
//   dw[t] = X_t^T . dZ  per tap                              launch_conv_wgrad (conv_wgrad.hip): a GEMM of its own, K = the pixel axis
//   dbias = column sums of dz                                colsum kernels, two passes, fixed order
//
//
// The plan and the steps of ron_conv2d_backward_nhwc are the functions of conv_train.h: the entry points here and the network-level
// chain (conv_chain.hip) call the same ones.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "conv_mfma.h"
#include "conv_train.h"
#include "storage_device.h"      // the roundings to the storage type and back, pack8 / unpack8, the halo walk

namespace ron {
namespace {

// ---- pack: dense fp32 [N,H,W,Csrc] -> halo tensor of the storage type, EVERY pixel of the buffer written ---------------------------
// The buffer holds `rows` pixels of Cdst channels; pixel `guard` is halo pixel 0 of the view.  Interior pixels get the rounded
// value (zero where mask <= 0, and in channels >= Csrc), everything else - halos, guards, the tail - zero.
RON_KERNEL_ARGS_BEGIN
struct PackArgs {
  const float* src;
  const float* mask;        // null: no mask
  unsigned short* out;
  long long rows, guard;
  int N, H, W, pad, Csrc, Cdst;
  // SCATTER only (ron_conv2d_padded_backward_nhwc): src and mask are [N,Hs,Ws,Csrc] and source pixel (sy, sx) lands on pixel
  // (soff + sstep * sy, soff + sstep * sx) of the H x W map; every other pixel of the map is zero
  int Hs, Ws, sstep, soff;
};
RON_KERNEL_ARGS_END(PackArgs)

template <bool BF16, bool SCATTER = false>
__global__ void conv_bwd_pack_halo_kernel(PackArgs a) {
  // (every buffer of the entry point is below 2 GiB, plan_backward: the 16-byte pieces and the pixels fit 32-bit arithmetic)
  const unsigned vecs = a.Cdst / 8;
  const unsigned total = (unsigned)a.rows * vecs;
  const bool vec_ok = a.Csrc % 4 == 0;
  for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    const unsigned b = i / vecs;
    const int v = (int)(i - b * vecs);
    float f[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    const HaloPixel p = halo_pixel(b, a.guard, a.N, a.H, a.W, a.pad);
    const unsigned img = p.img;
    bool inside = p.inside;
    int sy = p.y, sx = p.x, sh = a.H, sw = a.W;
    if (SCATTER && inside) {
      sy -= a.soff; sx -= a.soff;
      inside = sy >= 0 && sx >= 0 && sy % a.sstep == 0 && sx % a.sstep == 0;
      sy /= a.sstep; sx /= a.sstep; sh = a.Hs; sw = a.Ws;
      inside = inside && sy < sh && sx < sw;
    }
    if (inside) {
      const long long s0 = (((long long)img * sh + sy) * sw + sx) * a.Csrc + v * 8;
      if (vec_ok && v * 8 + 8 <= a.Csrc) {
        load8(a.src + s0, f);
        if (a.mask != nullptr) {
          float m[8];
          load8(a.mask + s0, m);
          keep_positive(f, m);
        }
      } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          if (v * 8 + e < a.Csrc) {
            const float val = a.src[s0 + e];
            f[e] = (a.mask == nullptr || a.mask[s0 + e] > 0.f) ? val : 0.f;
          }
        }
      }
    }
    *reinterpret_cast<uint4*>(a.out + (long long)i * 8) = pack8<BF16>(f);
  }
}

// ---- weights for the data gradient: fp32 HWIO on the device -> the blocked rows of pack.h, taps flipped, cin / cout swapped ----------
// rows[n = ci][k = t * CoP + co] = round(w[kh-1-ky, kw-1-kx, ci, co])  (zero for co >= cout and n >= cin), stored as
// [Npad / 64][K / 64][64 rows][64 elements]: hwio_to_rows + cast_rows + block_rows of the transposed filter.
RON_KERNEL_ARGS_BEGIN
struct WpackArgs {
  const float* w;
  unsigned short* out;
  int taps, cin, cout, cop, npad;
  int fill_ = 0;
};
RON_KERNEL_ARGS_END(WpackArgs)

template <bool BF16>
__global__ void conv_bwd_pack_weights_kernel(WpackArgs a) {
  const int K = a.taps * a.cop, steps = K / 64;
  const long long total = (long long)a.npad * (K / 8);
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    // i counts 16-byte pieces of the blocked image: [n / 64][kt][n % 64][piece of 8]
    const int piece = (int)(i & 7);
    const int nl = (int)((i >> 3) & 63);
    const long long blk = i >> 9;
    const int kt = (int)(blk % steps), nb = (int)(blk / steps);
    const int n = nb * 64 + nl, k = kt * 64 + piece * 8;
    const int t = k / a.cop, co = k - t * a.cop;
    const int ts = a.taps - 1 - t;                 // flipped tap (ky, kx both reversed = the flat tap index reversed)
    unsigned short h[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      float v = 0.f;
      if (n < a.cin && co + e < a.cout) v = a.w[((long long)ts * a.cin + n) * a.cout + co + e];
      h[e] = round_bits<BF16>(v);
    }
    *reinterpret_cast<uint4*>(a.out + i * 8) = pack8_bits(h);
  }
}

// ---- bias gradient: column sums of the packed dz, two passes in a fixed order ----------------------------------------------------------
// pass 1: block (chunk, 64-channel group): 32 row lanes x 8 vectors of 8 channels; a row lane adds rows r, r + 32, ... of its chunk,
// then 64 threads add the 32 lane sums in lane order.  pass 2: one wave per channel adds the chunk sums, lanes strided, then a fixed tree.
template <bool BF16>
__global__ __launch_bounds__(256) void conv_bwd_colsum_kernel(const unsigned short* dz, long long rows, int cop, long long chunk_rows, float* partial) {
  __shared__ float sums[32][64];
  const int tid = threadIdx.x, v = tid & 7, rl = tid >> 3;
  const int c0 = blockIdx.y * 64;
  const long long r0 = (long long)blockIdx.x * chunk_rows, r1 = r0 + chunk_rows < rows ? r0 + chunk_rows : rows;
  float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (long long r = r0 + rl; r < r1; r += 32) {
    float f[8];
    unpack8<BF16>(*reinterpret_cast<const uint4*>(dz + r * cop + c0 + v * 8), f);
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] += f[e];
  }
#pragma unroll
  for (int e = 0; e < 8; ++e) sums[rl][v * 8 + e] = acc[e];
  __syncthreads();
  if (tid < 64) {
    float s = 0.f;
    for (int l = 0; l < 32; ++l) s += sums[l][tid];
    partial[(long long)blockIdx.x * cop + c0 + tid] = s;
  }
}

// one wave per channel: lane l adds chunks l, l + 64, ... in that order, then the 64 lane sums are added in a fixed tree
__global__ __launch_bounds__(64) void conv_bwd_colsum_final_kernel(const float* partial, int chunks, int cop, float* dbias) {
  const int c = blockIdx.x, lane = threadIdx.x;
  float s = 0.f;
  for (int k = lane; k < chunks; k += 64) s += partial[(long long)k * cop + c];
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) s += __shfl_xor(s, d, 64);
  if (lane == 0) dbias[c] = s;
}

// ---- what the backward entry points share: the tail of the plan, the checks of a call, the launch steps --------------------------------
// (BackwardCore, what the operators decide on the host behind their own descriptor checks: conv_train.h)

int finish_plan(BackwardCore* P) {
  P->conv.out.bytes = P->dx_bytes;
  P->conv.wgt_bytes = P->w_bytes;
  P->sk_bytes = conv_scratch_bytes(P->conv);
  P->slab_bytes = conv_wgrad_scratch_bytes(P->wg);
  if (P->slab_bytes < 0) return RON_ERR_INVALID;
  // bias gradient: at most 512 chunks of >= 32 rows
  P->chunk_rows = std::max<int64_t>(32, (P->rows + 511) / 512);
  P->chunks = (int)((P->rows + P->chunk_rows - 1) / P->chunk_rows);
  P->off_w = carve(&P->total, P->w_bytes);
  P->off_bias = carve(&P->total, (int64_t)P->conv.Npad * 4);
  P->off_dx = carve(&P->total, P->dx_bytes);
  P->off_sk = carve(&P->total, P->sk_bytes);
  P->off_slab = carve(&P->total, P->slab_bytes);
  P->off_part = carve(&P->total, (int64_t)P->chunks * P->sum_cols * 4);
  return RON_OK;
}

// the checks of a call behind its plan; `what` starts every message, `sizer` is the entry that gives the workspace's size
int check_backward_call(const char* what, const char* sizer, const ron_conv_desc* d, const BackwardCore& P, const float* x,
                        const float* w, const float* y, const float* dy, const float* dx, const float* dw, void* workspace,
                        int64_t workspace_bytes) {
  RON_REQUIRE(dy != nullptr, "%s: dy is NULL", what);
  RON_REQUIRE(!d->relu || y != nullptr, "%s: relu is set and y is NULL (the mask is y > 0)", what);
  RON_REQUIRE(dx == nullptr || w != nullptr, "%s: dx needs w", what);
  RON_REQUIRE(dw == nullptr || x != nullptr, "%s: dw needs x", what);
  if (int rc = check_workspace(what, sizer, workspace, workspace_bytes, P.total)) return rc;
  RON_REQUIRE((((uintptr_t)x | (uintptr_t)y | (uintptr_t)dy) & 15) == 0, "%s: x, y and dy must be 16-byte aligned (they are read 16 bytes at a time)", what);
  if (dx != nullptr) {
    // what launch_conv would refuse is refused here, before anything is enqueued
    ConvLaunch c = P.conv;
    c.in.base = workspace; c.out.base = workspace; c.wgt = workspace; c.bias = static_cast<const float*>(workspace);
    if (P.sk_bytes > 0) { c.scratch = workspace; c.scratch_bytes = P.sk_bytes; }
    int o[4];
    if (int rc = conv_describe(c, o)) return rc;
  }
  return RON_OK;
}

// dense fp32 [n,h,w,csrc] -> `rows` + 2 `guard` pixels of cdst channels in the halo geometry of `pad` (0: a dense tensor).  sstep > 0:
// the same buffer from a COARSER source, dense fp32 [n,hs,ws,csrc] scattered to pixels (soff + sstep * sy, soff + sstep * sx) of the
// h x w map (the caller guarantees that they all exist), zero at every other pixel
template <bool BF16>
int launch_pack_halo(const float* src, const float* mask, void* out, int64_t rows, int n, int h, int w, int pad, int csrc, int cdst,
                     int64_t guard, hipStream_t s, int hs, int ws, int sstep, int soff) {
  PackArgs a = PackArgs();
  a.src = src; a.mask = mask; a.out = static_cast<unsigned short*>(out);
  a.rows = rows + 2 * guard; a.guard = guard;
  a.N = n; a.H = h; a.W = w; a.pad = pad; a.Csrc = csrc; a.Cdst = cdst;
  a.Hs = sstep ? hs : h; a.Ws = sstep ? ws : w; a.sstep = sstep ? sstep : 1; a.soff = soff;
  if (sstep) RON_LAUNCH((conv_bwd_pack_halo_kernel<BF16, true>), dim3(grid_for(a.rows * (cdst / 8))), dim3(256), 0, s, a);
  else RON_LAUNCH(conv_bwd_pack_halo_kernel<BF16>, dim3(grid_for(a.rows * (cdst / 8))), dim3(256), 0, s, a);
  RON_HIP_CHECK(ron::launch_error());
  return RON_OK;
}

// pass 1 of the bias gradient: the chunks' column sums of dz; returns them ([chunks][sum_cols]) for the operator's second pass
template <bool BF16>
int launch_colsum(const BackwardCore& P, const void* dzbuf, char* ws, hipStream_t s, const float** part) {
  *part = reinterpret_cast<const float*>(ws + P.off_part);
  RON_LAUNCH(conv_bwd_colsum_kernel<BF16>, dim3(P.chunks, P.sum_cols / 64), dim3(256), 0, s, static_cast<const unsigned short*>(dzbuf),
             (long long)P.rows, P.sum_cols, (long long)P.chunk_rows, reinterpret_cast<float*>(ws + P.off_part));
  RON_HIP_CHECK(ron::launch_error());
  return RON_OK;
}

// the data gradient's weights: w (device fp32 HWIO, `taps` x cin x cout) -> the blocked rows at `out` (w_bytes of them)
template <bool BF16>
int backward_pack_w(const float* w, void* out, int taps, int cin, int cout, int cop, int npad, int64_t w_bytes, hipStream_t s) {
  WpackArgs wa = WpackArgs();
  wa.w = w; wa.out = static_cast<unsigned short*>(out);
  wa.taps = taps; wa.cin = cin; wa.cout = cout; wa.cop = cop; wa.npad = npad;
  RON_LAUNCH(conv_bwd_pack_weights_kernel<BF16>, dim3(grid_for(w_bytes / 16)), dim3(256), 0, s, wa);
  RON_HIP_CHECK(ron::launch_error());
  return RON_OK;
}

}  // namespace

// ---- ron_conv2d_backward_nhwc: its plan and its steps are the functions of conv_train.h ------------------------------------------------
// Everything the entry point decides on the host: the descriptor's checks and the carving of the workspace (BackwardPlan, conv_train.h).
int train_plan_backward(const ron_conv_desc* d, BackwardPlan* P) {
  if (int rc0 = check_conv_desc(d)) return rc0;       // sizes, filter, stride, dilation inside the envelope of the forward; flags 0 or 1
  RON_REQUIRE(d->dtype == RON_DTYPE_BF16 || d->dtype == RON_DTYPE_F16, "conv backward: dtype %d: bf16 or fp16 only (fp32 and f16x3 have no backward)", d->dtype);
  RON_REQUIRE(d->transpose == 0 && d->pool == 0 && d->center_from == 0 && d->in_cstride == 0 && d->in_coff == 0 && d->tile_cfg == -1,
              "conv backward: a plain convolution (transpose, pool, center_from, in_cstride, in_coff = 0, tile_cfg = -1)");
  RON_REQUIRE(d->stride == 1, "conv backward: stride %d: stride-1 SAME convolutions only", d->stride);
  // 7 x 7 is fc6 of the `full` variant (dilation 1 there; nothing runs a dilated one, so none is accepted untested); 5 x 5 has no user
  RON_REQUIRE(d->kh == d->kw && (d->kh == 1 || d->kh == 3 || (d->kh == 7 && d->dilation == 1)),
              "conv backward: filter %d x %d at dilation %d: 1 x 1, 3 x 3, or 7 x 7 at dilation 1 only", d->kh, d->kw, d->dilation);
  RON_REQUIRE(d->dilation >= 1 && d->dilation <= kConvMaxDilation, "conv backward: dilation %d: 1 .. %d (the data gradient is a forward launch)",
              d->dilation, kConvMaxDilation);
  RON_REQUIRE(d->n > 0 && d->h > 0 && d->w > 0 && d->cout >= 1, "conv backward: empty tensor");
  RON_REQUIRE(d->cin > 0 && d->cin % 64 == 0, "conv backward: cin %d must be a multiple of 64 (the 3-channel stem is out of scope)", d->cin);
  RON_REQUIRE(d->splitk == -1 || d->splitk >= 1, "conv backward: pixel split %d (-1 = by shape, 1 = off, S = forced)", d->splitk);
  const int esz = 2;
  P->pad = (d->kh - 1) * d->dilation / 2;
  P->cop = (int)align_up(d->cout, 64);
  P->sum_cols = P->cop;
  P->taps = d->kh * d->kw;
  P->npad = (int)align_up(d->cin, conv_n_tile(d->cin));
  P->pixels = TensorView::halo_pixels(d->n, d->h, d->w, P->pad);
  P->rows = align_up(P->pixels, kWgStep);
  P->guard = (int64_t)P->pad * (d->w + P->pad) + P->pad;
  const int64_t dz_bytes = P->rows * P->cop * esz;
  const int64_t x_bytes = (P->rows + 2 * P->guard) * d->cin * esz;
  P->w_bytes = (int64_t)P->npad * P->taps * P->cop * esz;
  P->dx_bytes = TensorView::halo_pixels(d->n, d->h, d->w, 1) * d->cin * esz;
  const int64_t lim = (int64_t)1 << 31;
  RON_REQUIRE(dz_bytes < lim && x_bytes < lim && P->w_bytes < lim && P->dx_bytes < lim, "conv backward: a packed tensor would reach 2 GiB");
  // the data gradient as a forward launch over dz
  ConvLaunch& c = P->conv;
  c.dtype = d->dtype;
  c.in.N = d->n; c.in.H = d->h; c.in.W = d->w; c.in.C = P->cop; c.in.cstride = P->cop; c.in.pad = P->pad;
  c.in.bytes = P->pixels * P->cop * esz;
  c.out.N = d->n; c.out.H = d->h; c.out.W = d->w; c.out.C = d->cin; c.out.cstride = d->cin; c.out.pad = 1;
  c.Cout = d->cin; c.Npad = P->npad;
  c.kh = d->kh; c.kw = d->kw; c.stride = 1; c.dil = d->dilation; c.cpad = P->pad;
  c.relu = 0; c.Ho = d->h; c.Wo = d->w;
  c.splitk = -1;
  // the weight gradient
  WgradLaunch& g = P->wg;
  g.dtype = d->dtype;
  g.x = c.in; g.x.C = d->cin; g.x.cstride = d->cin; g.x.bytes = P->pixels * d->cin * esz;
  g.dz = c.in;
  g.kh = d->kh; g.kw = d->kw; g.dil = d->dilation; g.Cout = d->cout; g.guard = P->guard; g.splitk = d->splitk;
  P->off_dz = carve(&P->total, dz_bytes);
  P->off_x = carve(&P->total, x_bytes);
  return finish_plan(P);
}

int train_pack_halo(int dtype, const float* src, const float* mask, void* out, int64_t rows, int n, int h, int w, int pad, int csrc,
                    int cdst, int64_t guard, hipStream_t s, int hs, int ws, int sstep, int soff) {
  return dtype == RON_DTYPE_BF16 ? launch_pack_halo<true>(src, mask, out, rows, n, h, w, pad, csrc, cdst, guard, s, hs, ws, sstep, soff)
                                 : launch_pack_halo<false>(src, mask, out, rows, n, h, w, pad, csrc, cdst, guard, s, hs, ws, sstep, soff);
}

int train_backward_pack_w(const ron_conv_desc* d, const BackwardPlan& P, const float* w, char* ws, hipStream_t s) {
  return d->dtype == RON_DTYPE_BF16 ? backward_pack_w<true>(w, ws + P.off_w, P.taps, d->cin, d->cout, P.cop, P.npad, P.w_bytes, s)
                                    : backward_pack_w<false>(w, ws + P.off_w, P.taps, d->cin, d->cout, P.cop, P.npad, P.w_bytes, s);
}

// the data gradient behind the weights' pack: zero bias, the forward launch over dz; *out is the halo tensor it wrote
int train_data_grad(const BackwardCore& P, void* dzbuf, char* ws, hipStream_t s, TensorView* out) {
  RON_HIP_CHECK(dev_memset_async(ws + P.off_bias, 0, (size_t)P.conv.Npad * 4, s));
  ConvLaunch c = P.conv;
  c.in.base = dzbuf; c.out.base = ws + P.off_dx;
  c.wgt = ws + P.off_w; c.bias = reinterpret_cast<const float*>(ws + P.off_bias);
  if (P.sk_bytes > 0) { c.scratch = ws + P.off_sk; c.scratch_bytes = P.sk_bytes; }
  *out = c.out;
  return launch_conv(c, s);
}

// the weight gradient of the packed operands
int train_weight_grad(const BackwardCore& P, void* xbase, void* dzbase, float* dw, char* ws, hipStream_t s) {
  WgradLaunch g = P.wg;
  g.x.base = xbase;
  g.dz.base = dzbase;
  g.dw = dw;
  if (P.slab_bytes > 0) { g.scratch = ws + P.off_slab; g.scratch_bytes = P.slab_bytes; }
  return launch_conv_wgrad(g, s);
}

int train_bias_grad(int dtype, const BackwardPlan& P, const void* dzbuf, char* ws, int cout, float* dbias, hipStream_t s) {
  const float* part;
  if (int rc = dtype == RON_DTYPE_BF16 ? launch_colsum<true>(P, dzbuf, ws, s, &part) : launch_colsum<false>(P, dzbuf, ws, s, &part)) return rc;
  RON_LAUNCH(conv_bwd_colsum_final_kernel, dim3(cout), dim3(64), 0, s, part, P.chunks, P.cop, dbias);
  RON_HIP_CHECK(ron::launch_error());
  return RON_OK;
}

namespace {

// sstep = 0: y and dy are [n,h,w,cout] (ron_conv2d_backward_nhwc); else they are [n,hs,ws,cout] and dz is their scatter to pixels
// (soff + sstep * oy, soff + sstep * ox) of a zero h x w map (ron_conv2d_padded_backward_nhwc) - everything behind the pack is the same
int run_backward(const ron_conv_desc* d, const BackwardPlan& P, const float* x, const float* w, const float* y, const float* dy,
                 float* dx, float* dw, float* dbias, char* ws, hipStream_t s, int hs = 0, int wsrc = 0, int sstep = 0, int soff = 0) {
  int rc;
  void* dzbuf = ws + P.off_dz;
  if ((rc = train_pack_halo(d->dtype, dy, d->relu ? y : nullptr, dzbuf, P.rows, d->n, d->h, d->w, P.pad, d->cout, P.cop, 0, s, hs, wsrc, sstep, soff)))
    return rc;
  if (dx != nullptr) {
    TensorView out;
    if ((rc = train_backward_pack_w(d, P, w, ws, s))) return rc;
    if ((rc = train_data_grad(P, dzbuf, ws, s, &out))) return rc;
    if ((rc = launch_unpack(out, d->dtype, 0, dx, s))) return rc;
  }
  if (dw != nullptr) {
    char* xbuf = ws + P.off_x;
    if ((rc = train_pack_halo(d->dtype, x, nullptr, xbuf, P.rows, d->n, d->h, d->w, P.pad, d->cin, d->cin, P.guard, s))) return rc;
    if ((rc = train_weight_grad(P, xbuf + P.guard * d->cin * 2, dzbuf, dw, ws, s))) return rc;
  }
  if (dbias != nullptr && (rc = train_bias_grad(d->dtype, P, dzbuf, ws, d->cout, dbias, s))) return rc;
  return RON_OK;
}

}  // namespace
}  // namespace ron

extern "C" int64_t ron_conv2d_backward_workspace_bytes(const ron_conv_desc* d) {
  ron::BackwardPlan P;
  if (ron::train_plan_backward(d, &P) != RON_OK) return -1;
  return P.total;
}

extern "C" int ron_conv2d_backward_nhwc(const ron_conv_desc* d, const float* x, const float* w, const float* y, const float* dy,
                                        float* dx, float* dw, float* dbias, void* workspace, int64_t workspace_bytes, void* stream) {
  using namespace ron;
  BackwardPlan P;
  if (int rc = train_plan_backward(d, &P)) return rc;
  if (int rc = check_backward_call("conv backward", "ron_conv2d_backward_workspace_bytes", d, P, x, w, y, dy, dx, dw, workspace,
                                   workspace_bytes))
    return rc;
  hipStream_t s = (hipStream_t)stream;
  char* ws = static_cast<char*>(workspace);
  return run_backward(d, P, x, w, y, dy, dx, dw, dbias, ws, s);
}

// ---- ron_conv2d_padded_backward_nhwc: the 3x3 convolutions of the SSD extra blocks ----------------------------------------------------
// pad2d(cpad) + 3x3 VALID at stride s is the stride-1 SAME convolution sampled at (o + s oy, o + s ox), o = 1 - cpad.  So its
// backward is the stride-1 SAME backward of dz scattered to those pixels of a zero map of the input's size: dx, dw and dbias are the
// same sums with zero terms added.  The only new device code is the scatter in the pack (conv_bwd_pack_halo_kernel<.., true>); the
// plan, the data gradient, the weight gradient and the column sums run unchanged on the full-resolution geometry.  At stride 2 that
// is four times the MFMA work of a strided gather, on maps of 32 x 32 and smaller.
namespace ron {
namespace {

struct PaddedPlan : BackwardPlan {
  int ho = 0, wo = 0, soff = 0;
};

int plan_padded(const ron_conv_desc* d, int cpad, PaddedPlan* P) {
  RON_REQUIRE(d != nullptr, "conv padded backward: NULL descriptor");
  if (int rc0 = check_conv_desc(d)) return rc0;
  RON_REQUIRE(d->kh == 3 && d->kw == 3 && d->dilation == 1, "conv padded backward: filter %d x %d, dilation %d: 3 x 3, dilation 1 only (the 4 x 4 of block12 is ron_conv2d_k2s2_backward_nhwc on its inner taps)",
              d->kh, d->kw, d->dilation);
  RON_REQUIRE((d->stride == 2 && cpad == 1) || (d->stride == 1 && cpad == 0),
              "conv padded backward: stride %d with padding %d: (2, 1) = pad2d(1) + stride-2 VALID or (1, 0) = plain VALID only", d->stride, cpad);
  RON_REQUIRE(cpad == 1 || (d->h >= 3 && d->w >= 3), "conv padded backward: map %d x %d: a VALID 3 x 3 convolution needs h, w >= 3", d->h, d->w);
  ron_conv_desc full = *d;          // the stride-1 SAME convolution on the same map
  full.stride = 1;
  if (int rc = train_plan_backward(&full, P)) return rc;
  P->ho = (d->h + 2 * cpad - 3) / d->stride + 1;
  P->wo = (d->w + 2 * cpad - 3) / d->stride + 1;
  P->soff = 1 - cpad;
  return RON_OK;
}

}  // namespace
}  // namespace ron

extern "C" int64_t ron_conv2d_padded_backward_workspace_bytes(const ron_conv_desc* d, int cpad) {
  ron::PaddedPlan P;
  if (ron::plan_padded(d, cpad, &P) != RON_OK) return -1;
  return P.total;
}

extern "C" int ron_conv2d_padded_backward_nhwc(const ron_conv_desc* d, int cpad, const float* x, const float* w, const float* y, const float* dy,
                                               float* dx, float* dw, float* dbias, void* workspace, int64_t workspace_bytes, void* stream) {
  using namespace ron;
  PaddedPlan P;
  if (int rc = plan_padded(d, cpad, &P)) return rc;
  if (int rc = check_backward_call("conv padded backward", "ron_conv2d_padded_backward_workspace_bytes", d, P, x, w, y, dy, dx, dw, workspace,
                                   workspace_bytes))
    return rc;
  hipStream_t s = (hipStream_t)stream;
  char* ws = static_cast<char*>(workspace);
  return run_backward(d, P, x, w, y, dy, dx, dw, dbias, ws, s, P.ho, P.wo, d->stride, P.soff);
}

// ---- ron_conv2d_k2s2_backward_nhwc: the 2x2 stride-2 convolution and the 2x2 stride-2 transposed convolution ----------------------------
// Kernel == stride: every input pixel meets every output pixel through exactly one tap, so with s2d = space-to-depth
// ([n,2H,2W,C] -> [n,H,W,(ky,kx,C)]) and d2s its inverse both operators are 1x1 convolutions on the coarse H x W grid:
//
//   convolution (x [n,2H,2W,cin], w [2,2,cin,cout], dz [n,H,W,cout])
//     dw.reshape(4 cin, cout) = s2d(xs)^T dz          launch_conv_wgrad, kh = 1: x := s2d(xs), dz := dz
//     dx = d2s(dz @ ws.reshape(4 cin, cout)^T)        launch_conv, 1x1, 4 cin outputs; the depth-to-space happens in the unpack
//     dbias = column sums of dz
//   transposed (x [n,H,W,cin], w [2,2,cout,cin], dz [n,2H,2W,cout]), Dz = s2d(dz) [n,H,W,4 cout]
//     dw.reshape(4 cout, cin) = Dz^T xs               launch_conv_wgrad with the operands' roles swapped: x := Dz, dz := xs
//     dx = Dz @ ws.reshape(4 cout, cin)               launch_conv, 1x1, K = 4 cout
//     dbias[co] = the four taps' column sums of Dz, added in tap order
//
// No new MFMA kernel.  New here: the pack that gathers space-to-depth while it masks, rounds and packs (no fp32 shuffle pass), the
// weights pack for [4 cout] x [cin] (the transposed layout is already K-major per output row: no flip, no swap), the depth-to-space
// unpack and the tap fold of the bias gradient.  The coarse grid has no halo (pad 0, no guard pixels): the only zeros the weight
// gradient relies on are the rows from n H W up to the next multiple of 32, which both packs write.
namespace ron {
namespace {

// dense fp32 [N,2H,2W,C] -> [rows][4 C] of the storage type: row = coarse pixel, column (ky * 2 + kx) * C + c; rows >= N H W zero
RON_KERNEL_ARGS_BEGIN
struct S2dArgs {
  const float* src;
  const float* mask;        // null: no mask
  unsigned short* out;
  long long rows;
  int N, H, W, C;           // the COARSE grid; C % 8 == 0
};
RON_KERNEL_ARGS_END(S2dArgs)

template <bool BF16>
__global__ void k2s2_pack_s2d_kernel(S2dArgs a) {
  // (every packed tensor is below 2 GiB, plan_k2s2: the 16-byte pieces and the pixels fit 32-bit arithmetic)
  const unsigned vecs = a.C / 2;                    // 4 C / 8
  const unsigned total = (unsigned)a.rows * vecs;
  const unsigned pixels = (unsigned)a.N * a.H * a.W;
  for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    const unsigned b = i / vecs;
    const int k = (int)(i - b * vecs) * 8;
    float f[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (b < pixels) {
      const int t = k / a.C, c = k - t * a.C;
      const unsigned r = b / a.W;
      const int col = (int)(b - r * a.W);
      const unsigned img = r / a.H;
      const int row = (int)(r - img * a.H);
      const long long s0 = (((long long)img * 2 * a.H + 2 * row + (t >> 1)) * 2 * a.W + 2 * col + (t & 1)) * a.C + c;
      load8(a.src + s0, f);
      if (a.mask != nullptr) {
        float m[8];
        load8(a.mask + s0, m);
        keep_positive(f, m);
      }
    }
    *reinterpret_cast<uint4*>(a.out + (long long)i * 8) = pack8<BF16>(f);
  }
}

// weights of the transposed convolution for its data gradient: fp32 [2,2,cout,cin] = [K = 4 cout][cin] on the device -> the blocked rows
// of pack.h, rows[n = ci][k] = round(w[k, ci]) (zero for n >= cin): [Npad / 64][K / 64][64 rows][64 elements]
template <bool BF16>
__global__ void k2s2_pack_weights_kn_kernel(const float* w, unsigned short* out, int K, int cin, int npad) {
  const int steps = K / 64;
  const long long total = (long long)npad * (K / 8);
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int piece = (int)(i & 7);
    const int nl = (int)((i >> 3) & 63);
    const long long blk = i >> 9;
    const int kt = (int)(blk % steps), nb = (int)(blk / steps);
    const int n = nb * 64 + nl, k = kt * 64 + piece * 8;
    unsigned short h[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) h[e] = round_bits<BF16>(n < cin ? w[(long long)(k + e) * cin + n] : 0.f);
    *reinterpret_cast<uint4*>(out + i * 8) = pack8_bits(h);
  }
}

// dx of the convolution: the 1x1 launch's output, a halo tensor [N,H,W,4 C] (pad 1) of the storage type -> dense fp32 [N,2H,2W,C]
RON_KERNEL_ARGS_BEGIN
struct D2sArgs {
  const unsigned short* in;
  float* dx;
  int N, H, W, C;           // the coarse grid; C = cin
  int vec_store;            // dx is 16-byte aligned
  int fill_ = 0;
};
RON_KERNEL_ARGS_END(D2sArgs)

template <bool BF16>
__global__ void k2s2_unpack_d2s_kernel(D2sArgs a) {
  const int groups = a.C / 8;
  const long long total = (long long)a.N * 2 * a.H * 2 * a.W * groups;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int g = (int)(i % groups);
    const long long pix = i / groups;
    const int ox = (int)(pix % (2 * a.W));
    const int oy = (int)((pix / (2 * a.W)) % (2 * a.H));
    const long long img = pix / ((long long)4 * a.W * a.H);
    const long long q = halo_off(img, oy >> 1, ox >> 1, a.H, a.W, 1, 4 * a.C);
    float f[8];
    unpack8<BF16>(*reinterpret_cast<const uint4*>(a.in + q + ((oy & 1) * 2 + (ox & 1)) * a.C + g * 8), f);
    float* o = a.dx + i * 8;
    if (a.vec_store) {
      *reinterpret_cast<float4*>(o) = make_float4(f[0], f[1], f[2], f[3]);
      *reinterpret_cast<float4*>(o + 4) = make_float4(f[4], f[5], f[6], f[7]);
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) o[e] = f[e];
    }
  }
}

// bias gradient of the transposed convolution: per channel the four taps' column sums of Dz, each summed like
// conv_bwd_colsum_final_kernel does (lanes strided over the chunks, a fixed tree), then added in tap order
__global__ __launch_bounds__(64) void k2s2_colsum_fold_kernel(const float* partial, int chunks, int cols, int cout, float* dbias) {
  const int c = blockIdx.x, lane = threadIdx.x;
  float total = 0.f;
  for (int t = 0; t < 4; ++t) {
    float s = 0.f;
    for (int k = lane; k < chunks; k += 64) s += partial[(long long)k * cols + t * cout + c];
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) s += __shfl_xor(s, d, 64);
    total = t == 0 ? s : total + s;
  }
  if (lane == 0) dbias[c] = total;
}

struct K2Plan : BackwardCore {
  int H = 0, W = 0;             // the coarse grid
  int ca = 0, cz = 0;           // channels of the two packed operands: A (s2d gathered) and Z (dense)
  int npad = 0, nout = 0;       // rows of the packed weights; outputs of the data-gradient launch
  int kconv = 0;                // K of the data-gradient launch = channels of its input
  int64_t pixels = 0;
  int64_t off_a = 0, off_z = 0;
};

int plan_k2s2(const ron_conv_desc* d, K2Plan* P) {
  if (int rc0 = check_conv_desc(d)) return rc0;       // flags 0 or 1, sizes >= 1
  RON_REQUIRE(d->dtype == RON_DTYPE_BF16 || d->dtype == RON_DTYPE_F16, "conv k2s2 backward: dtype %d: bf16 or fp16 only (fp32 and f16x3 have no backward)", d->dtype);
  RON_REQUIRE(d->pool == 0 && d->center_from == 0 && d->in_cstride == 0 && d->in_coff == 0 && d->tile_cfg == -1,
              "conv k2s2 backward: a plain operator (pool, center_from, in_cstride, in_coff = 0, tile_cfg = -1)");
  RON_REQUIRE(d->kh == 2 && d->kw == 2 && d->stride == 2, "conv k2s2 backward: filter %d x %d, stride %d: 2 x 2 stride 2 only", d->kh, d->kw, d->stride);
  RON_REQUIRE(d->dilation == 1, "conv k2s2 backward: dilation %d: 1 only", d->dilation);
  RON_REQUIRE(d->n > 0 && d->h > 0 && d->w > 0 && d->cout >= 1, "conv k2s2 backward: empty tensor");
  RON_REQUIRE(d->cin > 0 && d->cin % 64 == 0, "conv k2s2 backward: cin %d must be a multiple of 64", d->cin);
  RON_REQUIRE(d->splitk == -1 || d->splitk >= 1, "conv k2s2 backward: pixel split %d (-1 = by shape, 1 = off, S = forced)", d->splitk);
  const bool tr = d->transpose != 0;
  if (tr) RON_REQUIRE(d->cout % 64 == 0, "conv k2s2 backward: transposed: cout %d must be a multiple of 64", d->cout);
  else RON_REQUIRE(d->h % 2 == 0 && d->w % 2 == 0, "conv k2s2 backward: map %d x %d: the strided convolution needs even sides", d->h, d->w);
  const int esz = 2;
  const int64_t lim = (int64_t)1 << 31;
  P->H = tr ? d->h : d->h / 2;
  P->W = tr ? d->w : d->w / 2;
  RON_REQUIRE((int64_t)d->n * P->H * P->W + kWgStep < lim, "conv k2s2 backward: too many pixels");
  const int cop = (int)align_up(d->cout, 64);
  P->ca = tr ? 4 * d->cout : 4 * d->cin;
  P->cz = tr ? d->cin : cop;
  P->kconv = tr ? P->ca : P->cz;
  P->nout = tr ? d->cin : 4 * d->cin;
  P->npad = (int)align_up(P->nout, conv_n_tile(P->nout));
  P->sum_cols = tr ? P->ca : P->cz;
  P->pixels = (int64_t)d->n * P->H * P->W;
  P->rows = align_up(P->pixels, kWgStep);
  const int64_t a_bytes = P->rows * P->ca * esz, z_bytes = P->rows * P->cz * esz;
  P->w_bytes = (int64_t)P->npad * P->kconv * esz;
  P->dx_bytes = TensorView::halo_pixels(d->n, P->H, P->W, 1) * P->nout * esz;
  RON_REQUIRE(a_bytes < lim && z_bytes < lim && P->w_bytes < lim && P->dx_bytes < lim, "conv k2s2 backward: a packed tensor would reach 2 GiB");
  // the data gradient: a 1x1 forward launch on the coarse grid
  ConvLaunch& c = P->conv;
  c.dtype = d->dtype;
  c.in.N = d->n; c.in.H = P->H; c.in.W = P->W; c.in.C = P->kconv; c.in.cstride = P->kconv; c.in.pad = 0;
  c.in.bytes = P->pixels * P->kconv * esz;
  c.out.N = d->n; c.out.H = P->H; c.out.W = P->W; c.out.C = P->nout; c.out.cstride = P->nout; c.out.pad = 1;
  c.Cout = P->nout; c.Npad = P->npad;
  c.kh = 1; c.kw = 1; c.stride = 1; c.dil = 1; c.cpad = 0;
  c.relu = 0; c.Ho = P->H; c.Wo = P->W;
  c.splitk = -1;
  // the weight gradient: x := A, dz := Z
  WgradLaunch& g = P->wg;
  g.dtype = d->dtype;
  g.x = c.in; g.x.C = P->ca; g.x.cstride = P->ca; g.x.bytes = P->pixels * P->ca * esz;
  g.dz = c.in; g.dz.C = P->cz; g.dz.cstride = P->cz; g.dz.bytes = P->pixels * P->cz * esz;
  g.kh = 1; g.kw = 1; g.dil = 1; g.Cout = tr ? d->cin : d->cout; g.guard = 0; g.splitk = d->splitk;
  P->off_a = carve(&P->total, a_bytes);
  P->off_z = carve(&P->total, z_bytes);
  return finish_plan(P);
}

template <bool BF16>
int k2s2_pack_s2d(const float* src, const float* mask, void* out, const K2Plan& P, int n, int c, hipStream_t s) {
  S2dArgs a = S2dArgs();
  a.src = src; a.mask = mask; a.out = static_cast<unsigned short*>(out);
  a.rows = P.rows; a.N = n; a.H = P.H; a.W = P.W; a.C = c;
  RON_LAUNCH(k2s2_pack_s2d_kernel<BF16>, dim3(grid_for(a.rows * (c / 2))), dim3(256), 0, s, a);
  RON_HIP_CHECK(ron::launch_error());
  return RON_OK;
}

template <bool BF16>
int run_k2s2(const ron_conv_desc* d, const K2Plan& P, const float* x, const float* w, const float* y, const float* dy,
             float* dx, float* dw, float* dbias, char* ws, hipStream_t s) {
  int rc;
  const bool tr = d->transpose != 0;
  const float* mask = d->relu ? y : nullptr;
  void* abuf = ws + P.off_a;
  void* zbuf = ws + P.off_z;
  // dz: the dense operand of the convolution, the gathered one of the transposed convolution
  void* dzbuf = tr ? abuf : zbuf;
  if (tr) rc = k2s2_pack_s2d<BF16>(dy, mask, abuf, P, d->n, d->cout, s);
  else rc = train_pack_halo(d->dtype, dy, mask, zbuf, P.rows, d->n, P.H, P.W, 0, d->cout, P.cz, 0, s);
  if (rc) return rc;
  if (dx != nullptr) {
    unsigned short* wout = reinterpret_cast<unsigned short*>(ws + P.off_w);
    if (tr) {
      RON_LAUNCH(k2s2_pack_weights_kn_kernel<BF16>, dim3(grid_for(P.w_bytes / 16)), dim3(256), 0, s, w, wout, P.kconv, d->cin, P.npad);
      RON_HIP_CHECK(ron::launch_error());
    } else if ((rc = backward_pack_w<BF16>(w, wout, 1, 4 * d->cin, d->cout, P.cz, P.npad, P.w_bytes, s))) {
      return rc;      // (HWIO [2,2,cin,cout] = [4 cin][cout]: the rows of the launch as they stand, a single tap)
    }
    TensorView out;
    if ((rc = train_data_grad(P, dzbuf, ws, s, &out))) return rc;
    if (tr) {
      if ((rc = launch_unpack(out, d->dtype, 0, dx, s))) return rc;
    } else {
      D2sArgs u = D2sArgs();
      u.in = reinterpret_cast<const unsigned short*>(ws + P.off_dx); u.dx = dx;
      u.N = d->n; u.H = P.H; u.W = P.W; u.C = d->cin; u.vec_store = ((uintptr_t)dx & 15) == 0;
      RON_LAUNCH(k2s2_unpack_d2s_kernel<BF16>, dim3(grid_for((long long)d->n * d->h * d->w * (d->cin / 8))), dim3(256), 0, s, u);
      RON_HIP_CHECK(ron::launch_error());
    }
  }
  if (dw != nullptr) {
    if (tr) rc = train_pack_halo(d->dtype, x, nullptr, zbuf, P.rows, d->n, P.H, P.W, 0, d->cin, d->cin, 0, s);
    else rc = k2s2_pack_s2d<BF16>(x, nullptr, abuf, P, d->n, d->cin, s);
    if (rc) return rc;
    if ((rc = train_weight_grad(P, abuf, zbuf, dw, ws, s))) return rc;
  }
  if (dbias != nullptr) {
    const float* part;
    if ((rc = launch_colsum<BF16>(P, dzbuf, ws, s, &part))) return rc;
    if (tr) RON_LAUNCH(k2s2_colsum_fold_kernel, dim3(d->cout), dim3(64), 0, s, part, P.chunks, P.sum_cols, d->cout, dbias);
    else RON_LAUNCH(conv_bwd_colsum_final_kernel, dim3(d->cout), dim3(64), 0, s, part, P.chunks, P.sum_cols, dbias);
    RON_HIP_CHECK(ron::launch_error());
  }
  return RON_OK;
}

}  // namespace
}  // namespace ron

extern "C" int64_t ron_conv2d_k2s2_backward_workspace_bytes(const ron_conv_desc* d) {
  ron::K2Plan P;
  if (ron::plan_k2s2(d, &P) != RON_OK) return -1;
  return P.total;
}

extern "C" int ron_conv2d_k2s2_backward_nhwc(const ron_conv_desc* d, const float* x, const float* w, const float* y, const float* dy,
                                             float* dx, float* dw, float* dbias, void* workspace, int64_t workspace_bytes, void* stream) {
  using namespace ron;
  K2Plan P;
  if (int rc = plan_k2s2(d, &P)) return rc;
  if (int rc = check_backward_call("conv k2s2 backward", "ron_conv2d_k2s2_backward_workspace_bytes", d, P, x, w, y, dy, dx, dw,
                                   workspace, workspace_bytes))
    return rc;
  hipStream_t s = (hipStream_t)stream;
  char* ws = static_cast<char*>(workspace);
  return d->dtype == RON_DTYPE_BF16 ? run_k2s2<true>(d, P, x, w, y, dy, dx, dw, dbias, ws, s)
                                    : run_k2s2<false>(d, P, x, w, y, dy, dx, dw, dbias, ws, s);
}
