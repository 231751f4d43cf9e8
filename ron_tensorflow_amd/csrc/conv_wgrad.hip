// The weight gradient of a stride-1 SAME convolution (launch_conv_wgrad, conv_mfma.h): dw[t] = X_t^T . dZ per tap, a GEMM whose K is
// the pixel axis.  The backward operators that call it, with their packs, data gradient and bias gradient, are conv_backward.hip.
//
// x and dz live in the SAME halo geometry (TensorView: shared halos, pad = (k - 1) * dilation / 2) and dz's
// halo is zero, so K is simply the flat halo-pixel index q: dz row q meets x row q + (ky * dil - pad) * Wp + (kx * dil - pad), the
// addressing of the forward's row gather.  A product whose dz pixel is a halo pixel is 0 * (a finite x value), one whose x pixel left
// the map reads a zero halo pixel: no 2-D index math and no bounds test in the loop.  The price is that EVERY row the loop can touch
// holds finite data: x carries `guard` = pad * Wp + pad zero pixels in front of pixel 0 and behind the last one, and both tensors
// are zero up to the next multiple of 32 pixels (the K step, kWgStep of conv_train.h).  ron_conv2d_backward_nhwc writes all of that
// itself.
//
// One workgroup = four waves = one 128 (cin) x 128 (cout) tile of one tap over one slice of the pixel range; each wave owns 64 x 64
// of it as 4 x 4 v_mfma_f32_16x16x32 accumulators (64 fp32 registers per lane).  An axis of exactly 64 channels gets a 64-wide tile
// (2 blocks per wave along it) instead of multiplying zeros in half of a 128-wide one.  Per K step of 32 pixels both operands are staged
// as [32 pixels][128 channels] images: plain 16-byte global loads -> registers -> ds_write_b128, double buffered, one barrier per step
// (no LDS-DMA, no counted vmcnt: nothing for tools/check_dma_counts.py here).  Both MFMA operands want K (pixels) along the lane's
// registers while the images have channels along the row, so both are read with ds_read_b64_tr_b16: per 16 channels two reads per
// lane group g, pixel rows 8g .. 8g+3 and 8g+4 .. 8g+7.  The images use the XOR swizzle of 256-byte rows that is documented as
// conflict free for these reads on a full 128-channel image (not measured here: no LDS bank-conflict counter was collected):  off(row, ch) = 256 * row + 16 * (ch ^ (((row & 3) << 2) | ((row >> 2) & 3))),  ch = the 16-byte chunk of the row.
// The transposed read needs EXEC all ones: the workgroup is 256 lanes, every branch around the reads is workgroup-uniform, and
// channel tiles that overhang the tensor are staged as zeros (pad, do not mask).
//
// Pixel slices: when tiles x taps leave CUs idle the pixel range is split over S workgroups per tile (conv1_2: 64 x 64 channels,
// 3.3 M pixels -> 9 tiles, S > 100).  Slices write fp32 slabs with plain stores, conv_wgrad_reduce_kernel adds them in slice order:
// no float atomics, the same bits on every run.  The taps of one (slice, tile) are adjacent workgroup ids: the nine read the same
// pixel rows, shifted, while those are in L2.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "conv_mfma.h"
#include "conv_train.h"
#include "storage_device.h"      // the MFMA and its transposed operand read (shared with stem_wgrad.hip)

namespace ron {
namespace {

constexpr int kWgTile = 128;       // channels per tile side
constexpr int kWgImage = kWgStep * kWgTile * 2;     // bytes of one staged operand image
constexpr int kWgLds = 4 * kWgImage;                // two operands, double buffered: 32 KB, inside the default limit

// byte offset of 16-byte chunk `ch` (0..15) of pixel row `row` (0..31) in a staged image
__device__ __forceinline__ int image_off(int row, int ch) { return 256 * row + 16 * (ch ^ (((row & 3) << 2) | ((row >> 2) & 3))); }

// ---- the weight-gradient tile ----------------------------------------------------------------------------------------------------------
RON_KERNEL_ARGS_BEGIN
struct WgradArgs {
  const char* x;            // halo pixel 0 of x (guard pixels in front)
  const char* dz;           // halo pixel 0 of dz
  float* out;               // dw [taps][cin][cout], or the slabs [slices][taps][cin][cout]
  long long slab_elems;     // taps * cin * cout
  int cin, cop, cout;
  int Wp, pad, dil, kw, taps;
  int tiles_m, tiles_n;
  int steps, steps_per;     // K steps in all / per slice (no empty slice)
};
RON_KERNEL_ARGS_END(WgradArgs)

// WBM, WBN: 16-channel MFMA blocks per wave along cin / cout (4 or 2): the workgroup's tile is 32 WBM x 32 WBN channels.  The 64-wide
// forms are for tensors of 64 channels (conv1_2; heads of <= 64 outputs), where a 128-wide tile would multiply zeros half the time.
// They keep the 256-byte image rows and their swizzle and fill half of each row: whether the transposed reads stay conflict free on
// the half-filled image has not been measured.  The epilogue stores 4 bytes per lane, 16 lanes side by side (64-byte segments at
// stride cout): not measured either; it runs once per workgroup behind the whole K loop.
template <bool BF16, int WBM, int WBN>
__global__ __launch_bounds__(256) void conv_wgrad_tile_kernel(WgradArgs a) {
  constexpr int TM = 32 * WBM, TN = 32 * WBN;
  constexpr int XCH = TM / 8, ZCH = TN / 8;            // 16-byte chunks per image row
  constexpr int XN = XCH * kWgStep / 256, ZN = ZCH * kWgStep / 256;      // chunks a lane stages per step (2 or 1)
  extern __shared__ __attribute__((aligned(16))) char smem[];      // [buffer][x image | dz image]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave >> 1, wn = wave & 1;
  unsigned id = blockIdx.x;
  const int tap = id % a.taps; id /= a.taps;
  const int tn = id % a.tiles_n; id /= a.tiles_n;
  const int tm = id % a.tiles_m;
  const int slice = id / a.tiles_m;
  const int m0 = tm * TM, n0 = tn * TN;
  const int ky = tap / a.kw, kx = tap - ky * a.kw;
  const long long tap_off = (long long)(ky * a.dil - a.pad) * a.Wp + (kx * a.dil - a.pad);

  // staging: lane -> 16-byte chunk xch of pixel row xrow (and, 128-wide, of row xrow + 16) of the x image; the same for dz
  const int xrow = tid / XCH, xch = tid % XCH, zrow = tid / ZCH, zch = tid % ZCH;
  const bool xv = m0 + xch * 8 < a.cin, zv = n0 + zch * 8 < a.cop;        // a tile that overhangs the channels stages zeros
  const int s_begin = slice * a.steps_per;
  const int n_steps = (a.steps - s_begin < a.steps_per ? a.steps - s_begin : a.steps_per);
  const long long q0 = (long long)s_begin * kWgStep;
  const long long x_row_bytes = (long long)a.cin * 2, z_row_bytes = (long long)a.cop * 2;
  const char* xp = a.x + (q0 + xrow + tap_off) * x_row_bytes + (long long)(m0 + xch * 8) * 2;
  const char* zp = a.dz + (q0 + zrow) * z_row_bytes + (long long)(n0 + zch * 8) * 2;
  const int xst = image_off(xrow, xch), zst = image_off(zrow, zch);        // (row + 16: the same swizzle, 4096 bytes on)
  const uint4 zero4 = {0u, 0u, 0u, 0u};
  // (plain variables, not arrays: indexed through the lambdas' references they ended up in scratch memory, the loads waited for at once)
  uint4 rx0 = zero4, rx1 = zero4, rz0 = zero4, rz1 = zero4;
  auto fetch = [&]() {
    rx0 = xv ? *reinterpret_cast<const uint4*>(xp) : zero4;
    if constexpr (XN == 2) rx1 = xv ? *reinterpret_cast<const uint4*>(xp + 16 * x_row_bytes) : zero4;
    rz0 = zv ? *reinterpret_cast<const uint4*>(zp) : zero4;
    if constexpr (ZN == 2) rz1 = zv ? *reinterpret_cast<const uint4*>(zp + 16 * z_row_bytes) : zero4;
    xp += kWgStep * x_row_bytes;
    zp += kWgStep * z_row_bytes;
  };
  auto stage = [&](int buf) {
    char* xi = smem + buf * 2 * kWgImage;
    char* zi = xi + kWgImage;
    *reinterpret_cast<uint4*>(xi + xst) = rx0;
    if constexpr (XN == 2) *reinterpret_cast<uint4*>(xi + xst + 4096) = rx1;
    *reinterpret_cast<uint4*>(zi + zst) = rz0;
    if constexpr (ZN == 2) *reinterpret_cast<uint4*>(zi + zst + 4096) = rz1;
  };

  // transposed reads: lane 16g + 4q + p supplies row 8g + 4h + q, channels 16 * blk + 4p .. + 3 (h = 0, 1)
  const int g = lane >> 4, q = (lane >> 2) & 3, p = lane & 3;
  int aoff[WBM][2], boff[WBN][2];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int row = 8 * g + 4 * h + q;
#pragma unroll
    for (int i = 0; i < WBM; ++i) aoff[i][h] = image_off(row, 2 * (wm * WBM + i) + (p >> 1)) + 8 * (p & 1);
#pragma unroll
    for (int j = 0; j < WBN; ++j) boff[j][h] = image_off(row, 2 * (wn * WBN + j) + (p >> 1)) + 8 * (p & 1);
  }

  v4f32 acc[WBM][WBN];
#pragma unroll
  for (int i = 0; i < WBM; ++i)
#pragma unroll
    for (int j = 0; j < WBN; ++j) acc[i][j] = v4f32{0.f, 0.f, 0.f, 0.f};

  fetch();
  stage(0);
  __syncthreads();
  for (int k = 0; k < n_steps; ++k) {                 // every branch here is workgroup-uniform: EXEC stays all ones at the reads
    const bool more = k + 1 < n_steps;
    if (more) fetch();
    const char* xi = smem + (k & 1) * 2 * kWgImage;
    const char* zi = xi + kWgImage;
    v8i16 A[WBM], B[WBN];
#pragma unroll
    for (int i = 0; i < WBM; ++i) A[i] = wgrad_operand(xi, aoff[i][0], aoff[i][1]);
#pragma unroll
    for (int j = 0; j < WBN; ++j) B[j] = wgrad_operand(zi, boff[j][0], boff[j][1]);
#pragma unroll
    for (int i = 0; i < WBM; ++i)
#pragma unroll
      for (int j = 0; j < WBN; ++j) acc[i][j] = wgrad_mfma<BF16>(A[i], B[j], acc[i][j]);
    if (more) stage((k + 1) & 1);
    __syncthreads();
  }

  // accumulator (i, j), register r of lane l: cin = 16 i + 4 (l / 16) + r, cout = 16 j + l % 16 of the wave's blocks
  float* out = a.out + (long long)slice * a.slab_elems + (long long)tap * a.cin * a.cout;
#pragma unroll
  for (int i = 0; i < WBM; ++i)
#pragma unroll
    for (int j = 0; j < WBN; ++j) {
      const int n = n0 + (wn * WBN + j) * 16 + (lane & 15);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int m = m0 + (wm * WBM + i) * 16 + 4 * g + r;
        if (m < a.cin && n < a.cout) out[(long long)m * a.cout + n] = acc[i][j][r];
      }
    }
}

// dw = slab 0 + slab 1 + ... in slice order
__global__ void conv_wgrad_reduce_kernel(const float* slabs, int slices, long long elems, float* dw) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < elems; i += (long long)gridDim.x * blockDim.x) {
    float s = slabs[i];
    for (int k = 1; k < slices; ++k) s += slabs[(long long)k * elems + i];
    dw[i] = s;
  }
}

// ---- planner ---------------------------------------------------------------------------------------------------------------------------
struct WgradPlan {
  int tm, tn;               // tile sides (128 or 64 channels)
  int taps, tiles_m, tiles_n, steps, steps_per, slices;
  int64_t slab_elems;
};

int plan_wgrad(const WgradLaunch& c, WgradPlan* p) {
  RON_REQUIRE(dtype_is_half(c.dtype), "conv wgrad: bf16 / f16 only (dtype %d)", c.dtype);
  RON_REQUIRE(c.kh >= 1 && c.kh == c.kw && (c.kh & 1) && c.dil >= 1, "conv wgrad: square odd filters (%d x %d, dilation %d)", c.kh, c.kw, c.dil);
  const int pad = (c.kh - 1) * c.dil / 2;
  RON_REQUIRE(c.x.N == c.dz.N && c.x.H == c.dz.H && c.x.W == c.dz.W && c.x.pad == pad && c.dz.pad == pad && c.x.N > 0 && c.x.H > 0 && c.x.W > 0,
              "conv wgrad: x and dz must share one halo geometry with pad %d", pad);
  RON_REQUIRE(c.x.coff == 0 && c.dz.coff == 0 && c.x.cstride == c.x.C && c.dz.cstride == c.dz.C && c.x.C % 64 == 0 && c.x.C > 0 &&
              c.dz.C % 64 == 0 && c.Cout >= 1 && c.Cout <= c.dz.C, "conv wgrad: whole tensors with channels padded to 64 (cin %d, dz %d, cout %d)",
              c.x.C, c.dz.C, c.Cout);
  RON_REQUIRE(c.guard >= (int64_t)pad * c.x.Wp() + pad, "conv wgrad: x needs %lld guard pixels, has %lld", (long long)pad * c.x.Wp() + pad, (long long)c.guard);
  const int64_t pixels = c.x.pixels();
  RON_REQUIRE(pixels + kWgStep < ((int64_t)1 << 31), "conv wgrad: too many pixels");
  p->taps = c.kh * c.kw;
  p->tm = c.x.C == 64 ? 64 : kWgTile;
  p->tn = c.dz.C == 64 ? 64 : kWgTile;
  p->tiles_m = (c.x.C + p->tm - 1) / p->tm;
  p->tiles_n = (c.dz.C + p->tn - 1) / p->tn;
  p->steps = (int)((pixels + kWgStep - 1) / kWgStep);
  p->slab_elems = (int64_t)p->taps * c.x.C * c.Cout;
  // by shape: about four workgroups per CU (256 CUs; 32 KB of LDS each), slices of >= 8 steps
  const int64_t base = (int64_t)p->taps * p->tiles_m * p->tiles_n;
  int want = c.splitk;
  if (want < 0) want = (int)std::min<int64_t>(std::max<int64_t>(1, 1024 / base), std::max(1, p->steps / 8));
  RON_REQUIRE(want >= 1, "conv wgrad: pixel split %d", c.splitk);
  want = std::min(want, p->steps);
  // a forced split is capped where the slabs would reach 2 GiB (the sum kernel walks them serially per element)
  want = (int)std::min<int64_t>(want, std::max<int64_t>(1, (((int64_t)1 << 31) - 1) / (p->slab_elems * 4)));
  p->steps_per = (p->steps + want - 1) / want;
  p->slices = (p->steps + p->steps_per - 1) / p->steps_per;       // no empty slice
  RON_REQUIRE(base * p->slices < ((int64_t)1 << 31), "conv wgrad: grid too large");
  return RON_OK;
}

template <bool BF16, int WBM, int WBN>
int launch_wgrad_t(const WgradLaunch& c, const WgradPlan& p, hipStream_t s) {
  WgradArgs a = WgradArgs();
  a.x = static_cast<const char*>(c.x.base); a.dz = static_cast<const char*>(c.dz.base);
  a.out = p.slices > 1 ? static_cast<float*>(c.scratch) : c.dw;
  a.slab_elems = p.slab_elems;
  a.cin = c.x.C; a.cop = c.dz.C; a.cout = c.Cout;
  a.Wp = c.x.Wp(); a.pad = c.x.pad; a.dil = c.dil; a.kw = c.kw; a.taps = p.taps;
  a.tiles_m = p.tiles_m; a.tiles_n = p.tiles_n; a.steps = p.steps; a.steps_per = p.steps_per;
  const unsigned grid = (unsigned)((int64_t)p.taps * p.tiles_m * p.tiles_n * p.slices);
  RON_LAUNCH((conv_wgrad_tile_kernel<BF16, WBM, WBN>), dim3(grid), dim3(256), kWgLds, s, a);
  RON_HIP_CHECK(ron::launch_error());
  if (p.slices > 1) {
    RON_LAUNCH(conv_wgrad_reduce_kernel, dim3(grid_for(p.slab_elems)), dim3(256), 0, s, static_cast<const float*>(c.scratch), p.slices, (long long)p.slab_elems, c.dw);
    RON_HIP_CHECK(ron::launch_error());
  }
  return RON_OK;
}

template <bool BF16>
int launch_wgrad_dtype(const WgradLaunch& c, const WgradPlan& p, hipStream_t s) {
  if (p.tm == 64) return p.tn == 64 ? launch_wgrad_t<BF16, 2, 2>(c, p, s) : launch_wgrad_t<BF16, 2, 4>(c, p, s);
  return p.tn == 64 ? launch_wgrad_t<BF16, 4, 2>(c, p, s) : launch_wgrad_t<BF16, 4, 4>(c, p, s);
}

}  // namespace

int conv_wgrad_slices(const WgradLaunch& c) {
  WgradPlan p;
  return plan_wgrad(c, &p) == RON_OK ? p.slices : -1;
}

int64_t conv_wgrad_scratch_bytes(const WgradLaunch& c) {
  WgradPlan p;
  if (plan_wgrad(c, &p) != RON_OK) return -1;
  return p.slices > 1 ? (int64_t)p.slices * p.slab_elems * 4 : 0;
}

int launch_conv_wgrad(const WgradLaunch& c, hipStream_t stream) {
  WgradPlan p;
  int rc = plan_wgrad(c, &p);
  if (rc != RON_OK) return rc;
  RON_REQUIRE(c.x.base != nullptr && c.dz.base != nullptr && c.dw != nullptr, "conv wgrad: NULL tensor");
  RON_REQUIRE(p.slices == 1 || (c.scratch != nullptr && c.scratch_bytes >= (int64_t)p.slices * p.slab_elems * 4),
              "conv wgrad: %d pixel slices need %lld bytes of scratch", p.slices, (long long)p.slices * p.slab_elems * 4);
  return c.dtype == RON_DTYPE_BF16 ? launch_wgrad_dtype<true>(c, p, stream) : launch_wgrad_dtype<false>(c, p, stream);
}

}  // namespace ron
