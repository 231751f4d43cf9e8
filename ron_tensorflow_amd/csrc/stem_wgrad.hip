// Backward of the 3-channel stem convolution conv1_1 (ron_conv2d_stem_backward_nhwc): weight and bias gradients, one fused pass.
//
//   dz = round(dy * (y > 0)),  xs = round(x)
//   dw[k][co] = sum over pixels of xs[pixel + tap(k)][c(k)] * dz[pixel][co],  k = (ky * 3 + kx) * 3 + c  (HWIO [3,3,3,64] = [27][64])
//   dbias[co] = sum over pixels of dz[pixel][co]
//
// A GEMM of M = 27 (padded to 32) x N = 64 with K = n h w pixels: 13 GFLOP at batch 32 against 1.7 GB of dy and y, so the layer is
// bound by reading those two tensors once.  K = 27 rows of x per pixel are too thin for conv_wgrad_tile_kernel (128 x 128 tiles over
// packed halo tensors: it would write and re-read a packed dz); like the forward (stem_conv_kernel) the stem gets a kernel of its own.
//
// Pixels are walked in DENSE order, p = (img * h + row) * w + col: no halo geometry and nothing packed to memory.  One workgroup =
// four waves owns every S-th of the 32-pixel K steps (workgroup s: steps s, s + S, ...), so that at any time the S workgroups read
// one contiguous stretch of dy and y (contiguous slices of steps, 2 S streams far apart: 504 against 483 us at batch 32, measured
// together with the unrolled loop of the reduce kernel).  Per step:
//   * dy (and y) 16 bytes per lane, two pixel rows per lane; masked, rounded (round_pair, storage_device.h), written as a [32 pixels][64 channels] image of the
//     storage type; the rounded values are added to the lane's four dbias partials (fixed order: the lane's rows, step by step);
//   * the x operand [32 pixels][32 k] is gathered 4 k per lane with a bounds test PER PIXEL (a step may straddle rows and images):
//     taps outside the image, k >= 27 and pixels behind the last one are staged as zeros, as the forward's patch staging does;
//   * 2 x 4 blocks of v_mfma_f32_16x16x32: wave v owns output channels 16 v .. 16 v + 15 and both k blocks.  Both operands have the
//     pixels (K) along the image rows, so they are read with ds_read_b64_tr_b16 as in conv_wgrad_tile_kernel: EXEC all ones (256
//     lanes, every branch around the reads is workgroup-uniform), overhang staged as zeros.
// The next step's global loads are issued before the MFMAs of the current one and staged into the other buffer behind them: one
// barrier per step.
//
// LDS images.  A transposed read serves, per 32-lane half, 8 pixel rows {8g + 4h + q: g in a pair, q = 0..3} x 32 bytes; the 64-dword
// bank row holds exactly those 256 bytes when the eight 32-byte pieces fall into eight different 32-byte bank slots:
//   dz   128-byte rows:  off(row, blk) = 128 row + 32 (blk ^ ((row >> 1 & 1) | (row >> 3 & 1) << 1)),  blk = 16-channel block 0..3
//   x     64-byte rows:  off(row, blk) =  64 row + 32 (blk ^ (row >> 3 & 1)),                          blk = k block 0..1
// (worked out from the bank rule, slot = (off / 32) mod 8; no LDS bank-conflict counter was collected).
//
// Slices.  Workgroup s of the S pixel slices writes slab s = [27][64] dw partials + [64] dbias partials with plain stores;
// stem_wgrad_reduce_kernel adds the slabs: 16 strided partial sums per element (slices g, g + 16, ... in that order), then those in order g = 0..15.  No float
// atomics: the same inputs and the same split give the same bytes.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "conv_mfma.h"
#include "storage_device.h"      // round_pair, bits_to_f, the MFMA and its transposed operand read (shared with conv_wgrad.hip)

namespace ron {
namespace {

constexpr int kStep = 32;                           // pixels per K step
constexpr int kCout = 64, kRows = 27;               // dw as a matrix: [27][64]
constexpr int kDwElems = kRows * kCout;             // 1728
constexpr int kSlabElems = kDwElems + kCout;        // one slice's partial sums: dw, then dbias
constexpr int kZImage = kStep * kCout * 2;          // 4096 bytes
constexpr int kXImage = kStep * 32 * 2;             // 2048 bytes
constexpr int kStage = kZImage + kXImage;           // one buffer; two of them: 12 KB
constexpr int kReduceGroups = 16;
// the kernel holds pixel indices, rounded up to the step, in 32-bit signed integers
constexpr int64_t kMaxPixels = RON_STEM_BACKWARD_MAX_PIXELS;
static_assert(kMaxPixels + kStep - 1 <= 0x7FFFFFFFLL, "a pixel index of the last step must fit an int");

__device__ __forceinline__ int z_off(int row, int blk) { return 128 * row + 32 * (blk ^ (((row >> 1) & 1) | (((row >> 3) & 1) << 1))); }
__device__ __forceinline__ int x_off(int row, int blk) { return 64 * row + 32 * (blk ^ ((row >> 3) & 1)); }

RON_KERNEL_ARGS_BEGIN
struct StemWgradArgs {
  const float* x;           // [pixels][3]; not read when want_dw == 0
  const float* y;           // [pixels][64], or null: no mask
  const float* dy;          // [pixels][64]
  float* slabs;             // [slices][kSlabElems]
  int H, W, pixels;
  int steps, slices;        // K steps in all; workgroup s owns steps s, s + slices, ... (slices <= steps: no empty slice)
  int want_dw;
};
RON_KERNEL_ARGS_END(StemWgradArgs)

template <bool BF16>
__global__ __launch_bounds__(256) void stem_wgrad_kernel(StemWgradArgs a) {
  __shared__ __attribute__((aligned(16))) char smem[2 * kStage];      // [buffer][dz image | x image]; the dbias fold reuses it
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int slice = blockIdx.x;
  const int n_steps = (a.steps - slice + a.slices - 1) / a.slices;      // steps slice, slice + slices, ...: >= 1, slices <= steps
  const bool want_dw = a.want_dw != 0, masked = a.y != nullptr;         // workgroup-uniform

  // dz staging: lane -> channels 4 zq .. 4 zq + 3 of pixel rows zrow and zrow + 16
  const int zrow = tid >> 4, zq = tid & 15;
  const int zst0 = z_off(zrow, zq >> 2) + 8 * (zq & 3), zst1 = z_off(zrow + 16, zq >> 2) + 8 * (zq & 3);
  // x staging: lane -> k = 4 xq .. 4 xq + 3 of pixel row xrow; k = (ky * 3 + kx) * 3 + c
  const int xrow = tid >> 3, xq = tid & 7;
  const int xst = x_off(xrow, xq >> 2) + 8 * (xq & 3);
  int kdy[4], kdx[4], koff[4];
  bool kreal[4];                                   // k < 27: the five padding rows of the operand are zeros
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int k = 4 * xq + e;
    const int tap = k / 3;
    kreal[e] = k < kRows;
    kdy[e] = tap / 3 - 1;
    kdx[e] = tap % 3 - 1;
    koff[e] = k - 3 * tap;
  }

  // transposed reads: lane 16 g + 4 q + p supplies pixel row 8 g + 4 h + q, bytes 8 p .. 8 p + 7 of the 32-byte block (h = 0, 1)
  const int g = lane >> 4, q = (lane >> 2) & 3, p = lane & 3;
  int aoff[2][2], boff[2];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int row = 8 * g + 4 * h + q;
    boff[h] = z_off(row, wave) + 8 * p;
    aoff[0][h] = x_off(row, 0) + 8 * p;
    aoff[1][h] = x_off(row, 1) + 8 * p;
  }

  v4f32 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
  float bsum[4] = {0.f, 0.f, 0.f, 0.f};
  const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
  float4 d0 = zero4, d1 = zero4, m0 = zero4, m1 = zero4;
  float xv[4] = {0.f, 0.f, 0.f, 0.f};

  // k = -1 fetches and stages step 0; step k's MFMAs run between the fetch and the staging of step k + 1
  for (int k = -1; k < n_steps; ++k) {                 // every branch here is workgroup-uniform: EXEC stays all ones at the reads
    const bool more = k + 1 < n_steps;
    if (more) {
      const int p0 = (slice + (k + 1) * a.slices) * kStep;        // < pixels, and p0 + 31 fits an int (kMaxPixels)
      const int pz0 = p0 + zrow, pz1 = pz0 + 16;
      d0 = pz0 < a.pixels ? *reinterpret_cast<const float4*>(a.dy + (long long)pz0 * kCout + 4 * zq) : zero4;
      d1 = pz1 < a.pixels ? *reinterpret_cast<const float4*>(a.dy + (long long)pz1 * kCout + 4 * zq) : zero4;
      if (masked) {
        m0 = pz0 < a.pixels ? *reinterpret_cast<const float4*>(a.y + (long long)pz0 * kCout + 4 * zq) : zero4;
        m1 = pz1 < a.pixels ? *reinterpret_cast<const float4*>(a.y + (long long)pz1 * kCout + 4 * zq) : zero4;
      }
      if (want_dw) {
        const int px = p0 + xrow;
        const unsigned r = (unsigned)px / (unsigned)a.W;
        const int col = px - (int)r * a.W;
        const int row = (int)(r % (unsigned)a.H);
        const bool live = px < a.pixels;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const bool ok = live && kreal[e] && (unsigned)(row + kdy[e]) < (unsigned)a.H && (unsigned)(col + kdx[e]) < (unsigned)a.W;
          // (the pixel a tap lands on is a pixel of the same image: its index is inside [0, pixels))
          xv[e] = ok ? a.x[((long long)px + (long long)kdy[e] * a.W + kdx[e]) * 3 + koff[e]] : 0.f;
        }
      }
    }
    if (k >= 0 && want_dw) {
      const char* zi = smem + (k & 1) * kStage;
      const char* xi = zi + kZImage;
      const v8i16 B = wgrad_operand(zi, boff[0], boff[1]);
      const v8i16 A0 = wgrad_operand(xi, aoff[0][0], aoff[0][1]);
      const v8i16 A1 = wgrad_operand(xi, aoff[1][0], aoff[1][1]);
      acc0 = wgrad_mfma<BF16>(A0, B, acc0);
      acc1 = wgrad_mfma<BF16>(A1, B, acc1);
    }
    if (more) {
      char* zi = smem + ((k + 1) & 1) * kStage;
      char* xi = zi + kZImage;
      const float f0[4] = {d0.x, d0.y, d0.z, d0.w}, f1[4] = {d1.x, d1.y, d1.z, d1.w};
      const float y0[4] = {m0.x, m0.y, m0.z, m0.w}, y1[4] = {m1.x, m1.y, m1.z, m1.w};
      float z0[4], z1[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        z0[e] = !masked || y0[e] > 0.f ? f0[e] : 0.f;
        z1[e] = !masked || y1[e] > 0.f ? f1[e] : 0.f;
      }
      const uint2 b0 = make_uint2(round_pair<BF16>(z0[0], z0[1]), round_pair<BF16>(z0[2], z0[3]));
      const uint2 b1 = make_uint2(round_pair<BF16>(z1[0], z1[1]), round_pair<BF16>(z1[2], z1[3]));
      const unsigned u0[2] = {b0.x, b0.y}, u1[2] = {b1.x, b1.y};
#pragma unroll
      for (int e = 0; e < 4; ++e) bsum[e] += bits_to_f<BF16>((unsigned short)(u0[e >> 1] >> (16 * (e & 1))));
#pragma unroll
      for (int e = 0; e < 4; ++e) bsum[e] += bits_to_f<BF16>((unsigned short)(u1[e >> 1] >> (16 * (e & 1))));
      if (want_dw) {
        *reinterpret_cast<uint2*>(zi + zst0) = b0;
        *reinterpret_cast<uint2*>(zi + zst1) = b1;
        *reinterpret_cast<uint2*>(xi + xst) = make_uint2(round_pair<BF16>(xv[0], xv[1]), round_pair<BF16>(xv[2], xv[3]));
      }
    }
    __syncthreads();
  }

  float* slab = a.slabs + (long long)slice * kSlabElems;
  if (want_dw) {
    // accumulator of k block i, register r of lane l: k = 16 i + 4 (l / 16) + r, cout = 16 wave + l % 16
    const int n = 16 * wave + (lane & 15);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int k0 = 4 * g + r, k1 = 16 + 4 * g + r;
      slab[k0 * kCout + n] = acc0[r];
      if (k1 < kRows) slab[k1 * kCout + n] = acc1[r];
    }
  }
  // dbias: the 16 row lanes of a channel, added in row order (the loop's last barrier is behind every read of the images)
  float* fold = reinterpret_cast<float*>(smem);          // [16][64]
#pragma unroll
  for (int e = 0; e < 4; ++e) fold[zrow * kCout + 4 * zq + e] = bsum[e];
  __syncthreads();
  if (tid < kCout) {
    float s = fold[tid];
    for (int l = 1; l < 16; ++l) s += fold[l * kCout + tid];
    slab[kDwElems + tid] = s;
  }
}

// out = the slabs' sum: wave g of a block adds slices g, g + 16, ... of its 64 elements in that order, then the groups are added in order
__global__ __launch_bounds__(64 * kReduceGroups) void stem_wgrad_reduce_kernel(const float* slabs, int slices, float* dw, float* dbias) {
  __shared__ float part[kReduceGroups][64];
  const int l = threadIdx.x & 63, grp = threadIdx.x >> 6;
  const int e = blockIdx.x * 64 + l;                       // kDwElems is a multiple of 64: a block is all dw or all dbias
  float* dst = e < kDwElems ? dw : dbias;
  if (dst == nullptr) return;                              // block-uniform
  float s = 0.f;
#pragma unroll 8
  for (int k = grp; k < slices; k += kReduceGroups) s += slabs[(long long)k * kSlabElems + e];
  part[grp][l] = s;
  __syncthreads();
  if (grp == 0) {
    const int groups = slices < kReduceGroups ? slices : kReduceGroups;
    float t = part[0][l];
    for (int k = 1; k < groups; ++k) t += part[k][l];
    dst[e < kDwElems ? e : e - kDwElems] = t;
  }
}

// ---- planner ---------------------------------------------------------------------------------------------------------------------------
struct StemPlan {
  int pixels = 0, steps = 0, slices = 0;
  int64_t total = 0;        // bytes of workspace: the slabs
};

int plan_stem_backward(const ron_conv_desc* d, StemPlan* P) {
  if (int rc0 = check_conv_desc(d)) return rc0;       // sizes >= 1, flags 0 or 1, the envelope of the forward
  RON_REQUIRE(d->dtype == RON_DTYPE_BF16 || d->dtype == RON_DTYPE_F16, "conv stem backward: dtype %d: bf16 or fp16 only (fp32 and f16x3 have no backward)", d->dtype);
  RON_REQUIRE(d->transpose == 0 && d->pool == 0 && d->center_from == 0 && d->in_cstride == 0 && d->in_coff == 0 && d->tile_cfg == -1,
              "conv stem backward: a plain convolution (transpose, pool, center_from, in_cstride, in_coff = 0, tile_cfg = -1)");
  RON_REQUIRE(d->stride == 1, "conv stem backward: stride %d: 1 only", d->stride);
  RON_REQUIRE(d->kh == 3 && d->kw == 3, "conv stem backward: filter %d x %d: 3 x 3 only", d->kh, d->kw);
  RON_REQUIRE(d->dilation == 1, "conv stem backward: dilation %d: 1 only", d->dilation);
  RON_REQUIRE(d->cin == 3 && d->cout == kCout, "conv stem backward: cin %d, cout %d: the 3 -> 64 channel stem only (every other convolution: ron_conv2d_backward_nhwc)",
              d->cin, d->cout);
  RON_REQUIRE(d->splitk == -1 || d->splitk >= 1, "conv stem backward: pixel split %d (-1 = by shape, 1 = off, S = forced)", d->splitk);
  const int64_t rows = (int64_t)d->n * d->h;          // < 2^62
  RON_REQUIRE(rows <= kMaxPixels && rows * d->w <= kMaxPixels, "conv stem backward: too many pixels: %d x %d x %d, at most %lld (RON_STEM_BACKWARD_MAX_PIXELS)",
              d->n, d->h, d->w, (long long)kMaxPixels);
  P->pixels = (int)(rows * d->w);
  P->steps = (int)(((int64_t)P->pixels + kStep - 1) / kStep);
  // by shape: four workgroups for each of the 256 CUs (12 KB of LDS each), slices of >= 8 steps
  int want = d->splitk;
  if (want < 0) want = std::min(1024, std::max(1, P->steps / 8));
  want = std::min(want, P->steps);                    // no empty slice: workgroup s starts at step s
  // a forced split is capped where the slabs would reach 2 GiB
  P->slices = (int)std::min<int64_t>(want, (((int64_t)1 << 31) - 1) / (kSlabElems * 4));
  P->total = align_up((int64_t)P->slices * kSlabElems * 4, 256);
  return RON_OK;
}

template <bool BF16>
int run_stem_backward(const ron_conv_desc* d, const StemPlan& P, const float* x, const float* y, const float* dy, float* dw, float* dbias,
                      void* workspace, hipStream_t s) {
  StemWgradArgs a = StemWgradArgs();
  a.x = x; a.y = d->relu ? y : nullptr; a.dy = dy;
  a.slabs = static_cast<float*>(workspace);
  a.H = d->h; a.W = d->w; a.pixels = P.pixels;
  a.steps = P.steps; a.slices = P.slices;
  a.want_dw = dw != nullptr;
  RON_LAUNCH(stem_wgrad_kernel<BF16>, dim3(P.slices), dim3(256), 0, s, a);
  RON_HIP_CHECK(ron::launch_error());
  RON_LAUNCH(stem_wgrad_reduce_kernel, dim3(kSlabElems / 64), dim3(64 * kReduceGroups), 0, s, static_cast<const float*>(workspace), P.slices, dw, dbias);
  RON_HIP_CHECK(ron::launch_error());
  return RON_OK;
}

}  // namespace
}  // namespace ron

extern "C" int64_t ron_conv2d_stem_backward_workspace_bytes(const ron_conv_desc* d) {
  ron::StemPlan P;
  if (ron::plan_stem_backward(d, &P) != RON_OK) return -1;
  return P.total;
}

extern "C" int ron_conv2d_stem_backward_nhwc(const ron_conv_desc* d, const float* x, const float* y, const float* dy, float* dw,
                                             float* dbias, void* workspace, int64_t workspace_bytes, void* stream) {
  using namespace ron;
  StemPlan P;
  if (int rc = plan_stem_backward(d, &P)) return rc;
  const char* what = "conv stem backward";
  RON_REQUIRE(dy != nullptr, "%s: dy is NULL", what);
  RON_REQUIRE(!d->relu || y != nullptr, "%s: relu is set and y is NULL (the mask is y > 0)", what);
  RON_REQUIRE(dw == nullptr || x != nullptr, "%s: dw needs x", what);
  if (int rc = check_workspace(what, "ron_conv2d_stem_backward_workspace_bytes", workspace, workspace_bytes, P.total)) return rc;
  RON_REQUIRE((((uintptr_t)y | (uintptr_t)dy) & 15) == 0, "%s: y and dy must be 16-byte aligned (they are read 16 bytes at a time)", what);
  RON_REQUIRE(((uintptr_t)x & 3) == 0, "%s: x must be 4-byte aligned", what);
  if (dw == nullptr && dbias == nullptr) return RON_OK;
  hipStream_t s = (hipStream_t)stream;
  return d->dtype == RON_DTYPE_BF16 ? run_stem_backward<true>(d, P, x, y, dy, dw, dbias, workspace, s)
                                    : run_stem_backward<false>(d, P, x, y, dy, dw, dbias, workspace, s);
}
