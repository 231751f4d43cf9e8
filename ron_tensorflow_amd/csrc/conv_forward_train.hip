// ron_conv2d_forward_nhwc: the forward that the entry points of conv_backward.hip differentiate, fed from DEVICE weights.
// ron_conv2d_nhwc (ops.cpp) is the same launch behind a host pack: it reads w and bias on the host, allocates its operands and
// synchronises.  Here everything that pack does happens on the stream: x goes through the halo pack of the backward (every pixel of the
// buffer written, so nothing is assumed about the workspace), w through conv_fwd_pack_weights_kernel below, the bias through a pad
// kernel, then launch_conv with the by-shape plan and launch_unpack.  The packed operands are byte for byte what setup_conv uploads
// (hwio_to_rows + cast_rows + block_rows, pack_conv_c64_weights, stem_pack_weights), the ConvLaunch is field for field the one it
// builds: for the same inputs y has the same bytes.  Nothing is cached between calls: the optimizer changes w every step.
//
// The weight pack.  HWIO flattened is [K = taps * cin][cout] with cout fastest; the kernels read rows[n = co][k], k fastest, in
// 64 x 64 blocks of 8 KB ([Npad / 64][K / 64][64][64], pack.h block_rows): a blocked 2-D transpose.  One workgroup moves one block through
// LDS.  In: a lane loads 16 bytes (four co) of two adjacent k rows, 8 lanes side by side (128 contiguous bytes per row), rounds and
// writes four dwords {k even | k odd << 16} into tile[co][k / 2].  Out: a lane reads four dwords of one co row and stores 16 bytes, the
// 256 lanes of a pass covering 4 KB of contiguous memory.  Rows are 33 dwords apart: with the 32-bank rule of ds_write_b32 / ds_read_b32
// (lane groups of 32) a write group touches banks 4 ql + (p & 3) + const - ql 0..7, four consecutive p - and a read group
// r + 4 j + const - four consecutive r, j 0..7: all distinct, no conflict in either direction (computed from the bank rule; no
// conflict counter was collected).  cout that is no multiple of 4, or a w that is not 16-byte aligned, takes 4-byte loads behind the
// same staging.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "conv_mfma.h"
#include "conv_train.h"
#include "storage_device.h"      // the roundings to the storage type, pack8

namespace ron {
namespace {

RON_KERNEL_ARGS_BEGIN
struct FwdWpackArgs {
  const float* w;
  unsigned short* out;
  int K, cout, npad;        // K = taps * cin, a multiple of 64
  int vec;                  // cout % 4 == 0 and w 16-byte aligned: 16-byte loads
};
RON_KERNEL_ARGS_END(FwdWpackArgs)

constexpr int kFwdTileStride = 33;      // dwords between the co rows of the staged block

template <bool BF16>
__global__ __launch_bounds__(256) void conv_fwd_pack_weights_kernel(FwdWpackArgs a) {
  __shared__ unsigned tile[64 * kFwdTileStride];
  const int tid = threadIdx.x;
  const int nbs = a.npad / 64, steps = a.K / 64;
  const long long blocks = (long long)nbs * steps;
  for (long long b = blockIdx.x; b < blocks; b += gridDim.x) {
    // column blocks fastest: neighbouring workgroups read neighbouring 256-byte pieces of the same k rows
    const int nb = (int)(b % nbs);
    const int kt = (int)(b / nbs);
#pragma unroll
    for (int it = 0; it < 2; ++it) {
      const int i = tid + 256 * it;
      const int p = (i >> 3) & 31, q = (i >> 8) * 8 + (i & 7);      // k pair, co quad of the block
      const int co = nb * 64 + 4 * q;
      const float* r0 = a.w + ((long long)kt * 64 + 2 * p) * a.cout + co;
      const float* r1 = r0 + a.cout;
      float lo[4] = {0.f, 0.f, 0.f, 0.f}, hi[4] = {0.f, 0.f, 0.f, 0.f};
      if (a.vec) {
        if (co < a.cout) {      // (cout % 4 == 0: the whole quad is inside)
          const float4 l = *reinterpret_cast<const float4*>(r0), h = *reinterpret_cast<const float4*>(r1);
          lo[0] = l.x; lo[1] = l.y; lo[2] = l.z; lo[3] = l.w; hi[0] = h.x; hi[1] = h.y; hi[2] = h.z; hi[3] = h.w;
        }
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (co + e < a.cout) { lo[e] = r0[e]; hi[e] = r1[e]; }
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) tile[(4 * q + e) * kFwdTileStride + p] = round_bits<BF16>(lo[e]) | ((unsigned)round_bits<BF16>(hi[e]) << 16);
    }
    __syncthreads();
    unsigned short* blk = a.out + ((long long)nb * steps + kt) * 4096;
#pragma unroll
    for (int it = 0; it < 2; ++it) {
      const int i = tid + 256 * it;
      const int j = i & 7, r = i >> 3;
      const unsigned* t = tile + r * kFwdTileStride + 4 * j;
      uint4 o;
      o.x = t[0]; o.y = t[1]; o.z = t[2]; o.w = t[3];
      *reinterpret_cast<uint4*>(blk + r * 64 + j * 8) = o;
    }
    __syncthreads();
  }
}

// the transposed convolution's weights [2,2,cout,cin] = rows[n = t * cout + co][k = ci] as they stand: a cast and the blocking
template <bool BF16>
__global__ void conv_fwd_pack_rows_kernel(const float* w, unsigned short* out, int K, int npad, int vec) {
  const int steps = K / 64;
  const long long total = (long long)npad * (K / 8);
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int piece = (int)(i & 7);
    const int nl = (int)((i >> 3) & 63);
    const long long blk = i >> 9;
    const int kt = (int)(blk % steps), nb = (int)(blk / steps);
    const float* src = w + ((long long)nb * 64 + nl) * K + kt * 64 + piece * 8;
    float f[8];
    if (vec) {
      load8(src, f);
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) f[e] = src[e];
    }
    *reinterpret_cast<uint4*>(out + i * 8) = pack8<BF16>(f);
  }
}

// The small images, one element per lane (a few KB each).  `what`:
//   0  the stem's im2col rows [64][64]: rows[n][k] = w[k][n] for k < 27, else 0 (one K step: blocked = plain)
//   1  the stem kernel's fragments (stem.hip, stem_pack_weights): fragment (t, s), lane (r, h), element j = w[k = 16 s + 8 h + j][2 r + t]
//   2  the resident-weight kernel's LDS images (conv_c64.hip, pack_conv_c64_weights) of a 3x3 filter over 64 channels
template <bool BF16>
__global__ void conv_fwd_pack_small_kernel(const float* w, unsigned short* out, int what, int cout, int total) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    float v = 0.f;
    if (what == 0) {
      const int n = i >> 6, k = i & 63;
      if (k < 27 && n < cout) v = w[k * cout + n];
    } else if (what == 1) {
      const int j = i & 7, lane = (i >> 3) & 63, ts = i >> 9;
      const int k = 16 * (ts & 1) + 8 * (lane >> 5) + j, ch = 2 * (lane & 31) + (ts >> 1);
      if (k < 27) v = w[k * 64 + ch];
    } else {
      const int e = i & 7, slot = (i >> 3) & 7, row = (i >> 6) & 63, rest = i >> 12;
      const int tap = rest % 9, hf = rest / 9;
      const int cin = (slot ^ (((row >> 1) & 3) << 1)) * 8 + e, ch = 64 * hf + 4 * (row % 16) + row / 16;
      v = w[((long long)tap * 64 + cin) * cout + ch];
    }
    out[i] = round_bits<BF16>(v);
  }
}

// bias [cout] (or none) -> [total] floats: `live` values bias[i % cout], then zeros (the transposed form repeats it per tap)
__global__ void conv_fwd_pad_bias_kernel(const float* bias, float* out, int cout, int live, int total) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x)
    out[i] = (bias != nullptr && i < live) ? bias[i % cout] : 0.f;
}

enum { kFwdPlain = 0, kFwdStrided, kFwdTransposed, kFwdStem, kFwdStemIm2col };

static_assert(kFwdPlain == 0, "ForwardPlan::kind defaults to the plain convolution");

TensorView dense_view(int n, int h, int w, int c, int pad) {
  TensorView v;
  v.N = n; v.H = h; v.W = w; v.C = c; v.cstride = c; v.coff = 0; v.pad = pad;
  v.bytes = TensorView::halo_pixels(n, h, w, pad) * c * 2;
  return v;
}

// w and bias -> what the launch reads
template <bool BF16>
int forward_pack_w(const ron_conv_desc* d, const ForwardPlan& P, const ConvLaunch& c, const float* w, const float* bias, char* ws, hipStream_t s) {
  unsigned short* wout = reinterpret_cast<unsigned short*>(ws + P.off_w);
  const int w_vec16 = ((uintptr_t)w & 15) == 0;
  if (P.kind == kFwdStem || P.kind == kFwdStemIm2col) {
    const int total = (int)(P.w_bytes / 2);
    RON_LAUNCH(conv_fwd_pack_small_kernel<BF16>, dim3(grid_for(total)), dim3(256), 0, s, w, wout, P.kind == kFwdStem ? 1 : 0, d->cout, total);
  } else if (P.kind == kFwdTransposed) {
    RON_LAUNCH(conv_fwd_pack_rows_kernel<BF16>, dim3(grid_for(P.w_bytes / 16)), dim3(256), 0, s, w, wout, P.K, c.Npad, w_vec16);
  } else {
    FwdWpackArgs a = FwdWpackArgs();
    a.w = w; a.out = wout; a.K = P.K; a.cout = d->cout; a.npad = c.Npad;
    a.vec = w_vec16 && d->cout % 4 == 0;
    const long long blocks = (long long)(c.Npad / 64) * (P.K / 64);
    RON_LAUNCH(conv_fwd_pack_weights_kernel<BF16>, dim3((unsigned)std::min<long long>(blocks, 1 << 20)), dim3(256), 0, s, a);
  }
  RON_HIP_CHECK(ron::launch_error());
  if (P.c64) {
    const int total = (int)(P.c64_bytes / 2);
    RON_LAUNCH(conv_fwd_pack_small_kernel<BF16>, dim3(grid_for(total)), dim3(256), 0, s, w, reinterpret_cast<unsigned short*>(ws + P.off_c64), 2, d->cout, total);
    RON_HIP_CHECK(ron::launch_error());
  }
  RON_LAUNCH(conv_fwd_pad_bias_kernel, dim3(grid_for(P.bias_total)), dim3(256), 0, s, bias, reinterpret_cast<float*>(ws + P.off_bias), d->cout, P.bias_live,
             P.bias_total);
  RON_HIP_CHECK(ron::launch_error());
  return RON_OK;
}

}  // namespace

// ---- conv_train.h: the plan and the steps of the forward ----------------------------------------------------------------------------
// Everything the entry point decides on the host: the descriptor's checks, the ConvLaunch of setup_conv (conv_launch_geometry gives
// both their geometry), the carving of the workspace
int train_plan_forward(const ron_conv_desc* d, ForwardPlan* P) {
  if (int rc0 = check_conv_desc(d)) return rc0;       // sizes, filter, stride, dilation inside the envelope; flags 0 or 1
  RON_REQUIRE(d->dtype == RON_DTYPE_BF16 || d->dtype == RON_DTYPE_F16, "conv forward: dtype %d: bf16 or fp16 only (fp32 and f16x3 run through ron_conv2d_nhwc)", d->dtype);
  RON_REQUIRE(d->pool == 0 && d->center_from == 0 && d->in_cstride == 0 && d->in_coff == 0 && d->tile_cfg == -1 && d->splitk == -1,
              "conv forward: a plain operator planned by shape (pool, center_from, in_cstride, in_coff = 0, tile_cfg = -1, splitk = -1)");
  RON_REQUIRE(d->kh == d->kw, "conv forward: filter %d x %d: square filters only", d->kh, d->kw);
  const bool k2s2 = d->kh == 2 && d->stride == 2 && d->dilation == 1;
  if (d->transpose) {
    RON_REQUIRE(k2s2, "conv forward: transposed: filter %d x %d, stride %d, dilation %d: 2 x 2 stride 2 only", d->kh, d->kw, d->stride, d->dilation);
    RON_REQUIRE(d->cin % 64 == 0, "conv forward: cin %d must be a multiple of 64", d->cin);
    RON_REQUIRE(d->cout % 128 == 0, "conv forward: transposed: cout %d must be a multiple of 128", d->cout);
    P->kind = kFwdTransposed;
    P->K = d->cin;
  } else if (d->stride != 1) {
    RON_REQUIRE(k2s2, "conv forward: stride %d with a %d x %d filter at dilation %d: the only strided convolution is 2 x 2 at stride 2", d->stride, d->kh,
                d->kw, d->dilation);
    RON_REQUIRE(d->h % 2 == 0 && d->w % 2 == 0, "conv forward: map %d x %d: the strided convolution needs even sides", d->h, d->w);
    RON_REQUIRE(d->cin % 64 == 0, "conv forward: cin %d must be a multiple of 64", d->cin);
    P->kind = kFwdStrided;
    P->K = 4 * d->cin;
  } else if (d->cin == 3) {
    RON_REQUIRE(d->kh == 3 && d->dilation == 1 && d->cout == 64, "conv forward: a 3-channel input: the 3 x 3, 3 -> 64 stem at dilation 1 only (%d x %d, cout %d, dilation %d)",
                d->kh, d->kw, d->cout, d->dilation);
    // the routes of ron_conv2d_nhwc: with the ReLU the stem kernel, without it (the kernel has it built in) im2col + one GEMM step
    P->kind = d->relu ? kFwdStem : kFwdStemIm2col;
    P->K = 64;
  } else {
    RON_REQUIRE(d->kh == 1 || d->kh == 3 || (d->kh == 7 && d->dilation == 1),
                "conv forward: filter %d x %d at dilation %d: 1 x 1, 3 x 3, or 7 x 7 at dilation 1 only", d->kh, d->kw, d->dilation);
    RON_REQUIRE(d->cin % 64 == 0, "conv forward: cin %d must be a multiple of 64 (or the 3-channel stem)", d->cin);
    P->K = d->kh * d->kw * d->cin;
  }
  int ho, wo;
  ConvLaunch& c = P->conv;
  conv_launch_geometry(d, &c, &ho, &wo);
  P->pad = c.cpad;
  c.cfg = -1; c.splitk = -1;
  const bool stem = P->kind == kFwdStem || P->kind == kFwdStemIm2col;
  c.in = dense_view(d->n, d->h, d->w, stem ? 64 : d->cin, P->pad);
  c.out = dense_view(d->n, ho, wo, d->cout, 1);
  const int64_t lim = (int64_t)1 << 31;
  P->x_bytes = P->kind == kFwdStem ? 0 : c.in.bytes;       // the stem kernel reads the fp32 image itself
  P->w_bytes = P->kind == kFwdStem ? 4 * 64 * 8 * 2 : (int64_t)c.Npad * P->K * 2;
  P->out_bytes = c.out.bytes;
  RON_REQUIRE(P->x_bytes < lim && P->w_bytes < lim && P->out_bytes < lim, "conv forward: a packed tensor would reach 2 GiB");
  c.wgt_bytes = P->w_bytes;
  P->c64 = conv_c64_wants_images(d->dtype, d->kh, d->kw, d->cin, d->cout, c.Npad);      // (a plain convolution: the others have no 3 x 3)
  if (P->c64) P->c64_bytes = (int64_t)(c.Npad / 64) * 9 * 64 * 64 * 2;
  P->bias_total = P->kind == kFwdStem ? 64 : c.Npad;
  P->bias_live = P->kind == kFwdTransposed ? c.Npad : d->cout;
  if (P->kind != kFwdStem) {
    static const char present = 0;      // conv_c64_applicable asks whether the images exist, not where
    ConvLaunch probe = c;
    if (P->c64) probe.wgt_c64 = &present;
    P->sk_bytes = conv_scratch_bytes(probe);
  }
  P->off_x = carve(&P->total, P->x_bytes);
  P->off_w = carve(&P->total, P->w_bytes);
  P->off_c64 = carve(&P->total, P->c64_bytes);
  P->off_bias = carve(&P->total, (int64_t)P->bias_total * 4);
  P->off_out = carve(&P->total, P->out_bytes);
  P->off_sk = carve(&P->total, P->sk_bytes);
  return RON_OK;
}

// the launch of a plan over a workspace
ConvLaunch train_forward_launch(const ForwardPlan& P, char* ws) {
  ConvLaunch c = P.conv;
  c.in.base = ws + P.off_x; c.out.base = ws + P.off_out;
  c.wgt = ws + P.off_w; c.bias = reinterpret_cast<const float*>(ws + P.off_bias);
  if (P.c64) c.wgt_c64 = ws + P.off_c64;
  if (P.sk_bytes > 0) { c.scratch = ws + P.off_sk; c.scratch_bytes = P.sk_bytes; }
  return c;
}

int train_forward_pack_w(const ron_conv_desc* d, const ForwardPlan& P, const ConvLaunch& c, const float* w, const float* bias, char* ws,
                         hipStream_t s) {
  return d->dtype == RON_DTYPE_BF16 ? forward_pack_w<true>(d, P, c, w, bias, ws, s) : forward_pack_w<false>(d, P, c, w, bias, ws, s);
}

namespace {

// the steps of `parts` (RON_FWD_PART_*) in order: x -> the launch's input tensor (the stem kernel reads the fp32 image itself), w and
// bias -> what the launch reads, the launch of ron_conv2d_nhwc on the packed operands, the delivery of y
int run_forward(const ron_conv_desc* d, const ForwardPlan& P, const float* x, const float* w, const float* bias, float* y, char* ws, hipStream_t s,
                int parts) {
  int rc;
  const ConvLaunch c = train_forward_launch(P, ws);
  if ((parts & RON_FWD_PART_X) && P.kind != kFwdStem) {
    if (P.kind == kFwdStemIm2col) rc = launch_im2col_c3(x, d->n, d->h, d->w, d->dtype, c.in.base, 64, s);
    else rc = train_pack_halo(d->dtype, x, nullptr, c.in.base, c.in.pixels(), d->n, d->h, d->w, P.pad, d->cin, d->cin, 0, s);
    if (rc) return rc;
  }
  if ((parts & RON_FWD_PART_W) && (rc = train_forward_pack_w(d, P, c, w, bias, ws, s))) return rc;
  if (parts & RON_FWD_PART_LAUNCH) {
    rc = P.kind == kFwdStem ? launch_stem_conv(x, d->n, d->h, d->w, d->dtype, c.wgt, c.bias, c.out, s) : launch_conv(c, s);
    if (rc) return rc;
  }
  return (parts & RON_FWD_PART_UNPACK) ? launch_unpack(c.out, d->dtype, 0, y, s) : RON_OK;
}

}  // namespace
}  // namespace ron

extern "C" int64_t ron_conv2d_forward_workspace_bytes(const ron_conv_desc* d) {
  ron::ForwardPlan P;
  if (ron::train_plan_forward(d, &P) != RON_OK) return -1;
  return P.total;
}

extern "C" int ron_conv2d_forward_parts_nhwc(const ron_conv_desc* d, const float* x, const float* w, const float* bias, float* y, void* workspace,
                                             int64_t workspace_bytes, int parts, void* stream) {
  using namespace ron;
  RON_REQUIRE(parts >= 1 && parts <= RON_FWD_PART_ALL, "conv forward: parts %d: a non-empty set of RON_FWD_PART_*", parts);
  ForwardPlan P;
  if (int rc = train_plan_forward(d, &P)) return rc;
  RON_REQUIRE(x != nullptr && w != nullptr && y != nullptr, "conv forward: x, w or y is NULL");
  if (int rc = check_workspace("conv forward", "ron_conv2d_forward_workspace_bytes", workspace, workspace_bytes, P.total)) return rc;
  const bool stem = P.kind == kFwdStem || P.kind == kFwdStemIm2col;
  RON_REQUIRE(((uintptr_t)x & (stem ? 3 : 15)) == 0 && ((uintptr_t)y & 15) == 0,
              "conv forward: x and y must be 16-byte aligned (x of the 3-channel stem: 4-byte)");
  RON_REQUIRE((((uintptr_t)w | (uintptr_t)bias) & 3) == 0, "conv forward: w and bias must be 4-byte aligned");
  char* ws = static_cast<char*>(workspace);
  if (P.kind != kFwdStem) {
    // what launch_conv would refuse is refused here, before anything is enqueued
    int o[4];
    if (int rc = conv_describe(train_forward_launch(P, ws), o)) return rc;
  }
  hipStream_t s = (hipStream_t)stream;
  return run_forward(d, P, x, w, bias, y, ws, s, parts);
}

extern "C" int ron_conv2d_forward_nhwc(const ron_conv_desc* d, const float* x, const float* w, const float* bias, float* y, void* workspace,
                                       int64_t workspace_bytes, void* stream) {
  return ron_conv2d_forward_parts_nhwc(d, x, w, bias, y, workspace, workspace_bytes, RON_FWD_PART_ALL, stream);
}
