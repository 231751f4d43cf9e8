// Backward of the two SSD-only elementwise operators: the 3x3 stride-1 SAME max-pool (pool5 of SSD: ron_maxpool3x3s1_backward_nhwc)
// and the L2 normalisation with a learned scale (block4 of SSD: ron_l2norm_backward_nhwc).  Semantics: include/ron_hip.h.
//
// ---- the pool ------------------------------------------------------------------------------------------------------------------------
// The windows overlap, so op_backward.hip's "one store per window" does not carry over; a scatter would need atomics or a cleared
// buffer.  This is a GATHER: one lane = one input position x 4 channels.  It loads the 5x5 neighbourhood of xs = round(x) (what any
// of the up to nine windows that contain the position can see), decides for each of those windows whether the position is the
// window's first maximum, adds round(dy) of the windows that select it in row-major order of (oy, ox), rounds the sum once and
// stores dx once.  "First maximum" without walking each window: position p is selected iff every in-bounds position in front of it
// (row-major) is LESS than xs[p] and every one behind it is LESS OR EQUAL - the running-maximum rule (start at the first position, take
// over on > only) solved for p.  The positions of a window row in front of / behind p's own row enter through that row's maximum over
// the window's columns, which the three windows of a window column share: 15 row maxima, then two row tests and two in-row tests per
// window.  The row maxima are taken on the unrounded values and rounded once (rounding is monotone).  Padding is excluded (never
// read, never a zero).  -0.0 == +0.0 under < and <=, so the two are a tie.  NaN: outside the contract.  34 16-byte loads per lane,
// 25 of x and 9 of dy, neighbouring lanes' overlap served from L1 / L2; one 16-byte store.  Measured: the kernel is
// bound by its instruction count (about 3000 per wave), not by memory.
//
// ---- the L2 normalisation ------------------------------------------------------------------------------------------------------------
// One wave per pixel like the forward (elementwise.hip, l2norm_kernel): lane l owns channels 4 l + 256 k .. + 3, k < IT.  x and dy are
// read once, 16 bytes per lane, and stay in registers through the two butterflies (ss, then t); dx is written once.  The dgamma partial
// sums of the wave's channels stay in registers over the pixels the wave walks (pixel = wave, wave + waves, ...) and are written as
// row `wave` of a [waves][c] fp32 table in the workspace; l2norm_dgamma_kernel adds the rows: eight contiguous runs of rows, each in
// row order, then the eight runs in run order.  waves = min(n h w, kL2MaxWaves) is a function of the shape alone, so every sum's order
// is: no atomics, the same bytes on every call and on every device.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "conv_mfma.h"
#include "storage_device.h"      // round_storage

namespace ron {
namespace {

// n h w c elements of 4 bytes inside 2^62 bytes (the kernels index with 64-bit integers)
bool elems_fit(int n, int h, int w, int c, int64_t* pixels) {
  int64_t p, e;
  if (__builtin_mul_overflow((int64_t)n, (int64_t)h, &p) || __builtin_mul_overflow(p, (int64_t)w, &p)) return false;
  if (__builtin_mul_overflow(p, (int64_t)c, &e) || e >= ((int64_t)1 << 60)) return false;
  *pixels = p;
  return true;
}

RON_KERNEL_ARGS_BEGIN
struct Pool3Args {
  const float* x;
  const float* dy;
  float* dx;
  long long total;          // positions x groups of 4 channels
  int h, w, c;
  int fill_ = 0;
};
RON_KERNEL_ARGS_END(Pool3Args)

template <bool BF16>
__global__ __launch_bounds__(256) void maxpool3x3s1_backward_kernel(Pool3Args a) {
  const int groups = a.c / 4;
  for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < a.total; idx += (long long)gridDim.x * blockDim.x) {
    const long long pix = idx / groups;
    const int j = (int)(pix % a.w);
    const int i = (int)((pix / a.w) % a.h);
    const long long at = idx * 4;                    // element (image, i, j, 4 (idx % groups))
    const long long rowstep = (long long)a.w * a.c;
    // the 5x5 neighbourhood, index 2 = the position itself; rv / cv: the row / column exists
    bool rv[5], cv[5];
#pragma unroll
    for (int k = 0; k < 5; ++k) { rv[k] = i + k - 2 >= 0 && i + k - 2 < a.h; cv[k] = j + k - 2 >= 0 && j + k - 2 < a.w; }
    float nb[5][5][4];
#pragma unroll
    for (int r = 0; r < 5; ++r)
#pragma unroll
      for (int q = 0; q < 5; ++q) {
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (rv[r] && cv[q]) v = *reinterpret_cast<const float4*>(a.x + at + (r - 2) * rowstep + (long long)(q - 2) * a.c);
        nb[r][q][0] = v.x; nb[r][q][1] = v.y; nb[r][q][2] = v.z; nb[r][q][3] = v.w;
      }
    // Rounding is monotone, so round(max(a, b)) == max(round(a), round(b)): the row maxima are taken on the raw values and rounded
    // once each (60 roundings per lane instead of 400); only the position's own row is compared value by value and rounded as it is.
    float own[5][4];
#pragma unroll
    for (int q = 0; q < 5; ++q)
#pragma unroll
      for (int e = 0; e < 4; ++e) own[q][e] = round_storage<BF16>(nb[2][q][e]);
    // cm[r][k]: the maximum of row r over the in-bounds columns of the windows at ox = j - 1 + k (columns k .. k + 2; k + 1 exists
    // whenever the window does)
    float cm[5][3][4];
#pragma unroll
    for (int r = 0; r < 5; ++r)
#pragma unroll
      for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          float m = nb[r][k + 1][e];
          if (cv[k]) m = fmaxf(m, nb[r][k][e]);
          if (cv[k + 2]) m = fmaxf(m, nb[r][k + 2][e]);
          cm[r][k][e] = round_storage<BF16>(m);
        }
    float sum[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int m = 0; m < 3; ++m)                       // window row oy = i - 1 + m: rows m .. m + 2 of the neighbourhood
#pragma unroll
      for (int k = 0; k < 3; ++k) {                   // window column ox = j - 1 + k
        if (!(rv[m + 1] && cv[k + 1])) continue;      // no such window
        const float4 gv = *reinterpret_cast<const float4*>(a.dy + at + (m - 1) * rowstep + (long long)(k - 1) * a.c);
        const float gy[4] = {gv.x, gv.y, gv.z, gv.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float me = own[2][e];
          bool sel = true;
#pragma unroll
          for (int r = m; r < m + 3; ++r) {
            if (r < 2) sel = sel && (!rv[r] || cm[r][k][e] < me);
            if (r > 2) sel = sel && (!rv[r] || cm[r][k][e] <= me);
          }
#pragma unroll
          for (int q = k; q < k + 3; ++q) {
            if (q < 2) sel = sel && (!cv[q] || own[q][e] < me);
            if (q > 2) sel = sel && (!cv[q] || own[q][e] <= me);
          }
          sum[e] += sel ? round_storage<BF16>(gy[e]) : 0.f;
        }
      }
    *reinterpret_cast<float4*>(a.dx + at) = make_float4(round_storage<BF16>(sum[0]), round_storage<BF16>(sum[1]), round_storage<BF16>(sum[2]), round_storage<BF16>(sum[3]));
  }
}

// ---- L2 normalisation ------------------------------------------------------------------------------------------------------------------
constexpr int kL2MaxWaves = 2048;       // rows of the dgamma table at most: eight waves per CU of a 256-CU device, 4 MB of table at c = 512
constexpr int kL2MaxC = 2048;           // channels: IT <= 8 passes of 256 per wave, everything in registers
constexpr int kL2Runs = 8;              // contiguous runs of table rows the second kernel adds side by side

RON_KERNEL_ARGS_BEGIN
struct L2Args {
  const float* x;
  const float* gamma;
  const float* dy;
  float* dx;                // null: not computed
  float* table;             // [waves][c]; null: dgamma not computed
  long long pixels;
  int c, waves;
};
RON_KERNEL_ARGS_END(L2Args)

template <bool BF16, int IT>
__global__ __launch_bounds__(256) void l2norm_backward_kernel(L2Args a) {
  const int lane = threadIdx.x & 63;
  const int wave = (int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6);
  if (wave >= a.waves) return;                        // (wave-uniform: the butterflies below run with all 64 lanes)
  float gm[IT][4], acc[IT][4];
#pragma unroll
  for (int k = 0; k < IT; ++k) {
    const int c0 = lane * 4 + k * 256;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (c0 < a.c) v = *reinterpret_cast<const float4*>(a.gamma + c0);
    gm[k][0] = v.x; gm[k][1] = v.y; gm[k][2] = v.z; gm[k][3] = v.w;
#pragma unroll
    for (int e = 0; e < 4; ++e) acc[k][e] = 0.f;
  }
  for (long long pix = wave; pix < a.pixels; pix += a.waves) {
    const long long base = pix * a.c;
    float xs[IT][4], dz[IT][4];
    float ss = 0.f;
#pragma unroll
    for (int k = 0; k < IT; ++k) {
      const int c0 = lane * 4 + k * 256;
      float4 vx = make_float4(0.f, 0.f, 0.f, 0.f), vd = vx;
      if (c0 < a.c) {
        vx = *reinterpret_cast<const float4*>(a.x + base + c0);
        vd = *reinterpret_cast<const float4*>(a.dy + base + c0);
      }
      xs[k][0] = round_storage<BF16>(vx.x); xs[k][1] = round_storage<BF16>(vx.y); xs[k][2] = round_storage<BF16>(vx.z); xs[k][3] = round_storage<BF16>(vx.w);
      dz[k][0] = round_storage<BF16>(vd.x); dz[k][1] = round_storage<BF16>(vd.y); dz[k][2] = round_storage<BF16>(vd.z); dz[k][3] = round_storage<BF16>(vd.w);
#pragma unroll
      for (int e = 0; e < 4; ++e) ss += xs[k][e] * xs[k][e];
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) ss += __shfl_xor(ss, d, 64);
    const float inv = 1.f / sqrtf(fmaxf(ss, 1e-12f));
    float t = 0.f;
#pragma unroll
    for (int k = 0; k < IT; ++k)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        xs[k][e] = xs[k][e] * inv;                    // u
        t += (dz[k][e] * gm[k][e]) * xs[k][e];
        acc[k][e] += dz[k][e] * xs[k][e];
      }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) t += __shfl_xor(t, d, 64);
    if (a.dx != nullptr) {
      const bool live = ss >= 1e-12f;                 // below: TF's maximum hands the gradient to the constant, none to ss
#pragma unroll
      for (int k = 0; k < IT; ++k) {
        const int c0 = lane * 4 + k * 256;
        if (c0 >= a.c) continue;
        float o[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float g = dz[k][e] * gm[k][e];
          o[e] = round_storage<BF16>(live ? inv * (g - xs[k][e] * t) : inv * g);
        }
        *reinterpret_cast<float4*>(a.dx + base + c0) = make_float4(o[0], o[1], o[2], o[3]);
      }
    }
  }
  if (a.table != nullptr) {
#pragma unroll
    for (int k = 0; k < IT; ++k) {
      const int c0 = lane * 4 + k * 256;
      if (c0 < a.c) *reinterpret_cast<float4*>(a.table + (long long)wave * a.c + c0) = make_float4(acc[k][0], acc[k][1], acc[k][2], acc[k][3]);
    }
  }
}

// dgamma[ch] = the table's column ch: run r adds rows r * per .. min(rows, (r + 1) * per) - 1 in row order starting from 0.f, then
// the runs are added in run order.  Block = 32 channels x 8 runs.
__global__ __launch_bounds__(256) void l2norm_dgamma_kernel(const float* table, int rows, int c, float* dgamma) {
  __shared__ float part[kL2Runs][32];
  const int cl = threadIdx.x & 31, run = threadIdx.x >> 5;
  const int ch = blockIdx.x * 32 + cl;
  const int per = (rows + kL2Runs - 1) / kL2Runs;
  const int r0 = run * per, r1 = min(rows, r0 + per);
  float s = 0.f;
  if (ch < c) {
    // sixteen loads in flight, added in row order: the loop is bound by the latency of its loads, not by their number
    int r = r0;
    for (; r + 16 <= r1; r += 16) {
      float v[16];
#pragma unroll
      for (int k = 0; k < 16; ++k) v[k] = table[(long long)(r + k) * c + ch];
#pragma unroll
      for (int k = 0; k < 16; ++k) s += v[k];
    }
    for (; r < r1; ++r) s += table[(long long)r * c + ch];
  }
  part[run][cl] = s;
  __syncthreads();
  if (run == 0 && ch < c) {
    float d = part[0][cl];
#pragma unroll
    for (int r = 1; r < kL2Runs; ++r) d += part[r][cl];
    dgamma[ch] = d;
  }
}

int l2_waves(int64_t pixels) { return (int)std::min<int64_t>(pixels, kL2MaxWaves); }

int check_l2_shape(int n, int h, int w, int c, int dtype, int64_t* pixels) {
  RON_REQUIRE(dtype == RON_DTYPE_BF16 || dtype == RON_DTYPE_F16, "l2norm backward: dtype %d: bf16 or fp16 only", dtype);
  RON_REQUIRE(n >= 1 && h >= 1 && w >= 1, "l2norm backward: empty tensor (n %d, h %d, w %d)", n, h, w);
  RON_REQUIRE(c >= 8 && c % 8 == 0, "l2norm backward: c %d must be a multiple of 8", c);
  RON_REQUIRE(c <= kL2MaxC, "l2norm backward: c %d: at most %d channels (a wave keeps a pixel in registers)", c, kL2MaxC);
  RON_REQUIRE(elems_fit(n, h, w, c, pixels), "l2norm backward: tensor of %d x %d x %d x %d elements is beyond 64-bit indexing", n, h, w, c);
  return RON_OK;
}

template <bool BF16>
void launch_l2_backward(const L2Args& a, hipStream_t s) {
  const int grid = (a.waves + 3) / 4;
  const int it = (a.c + 255) / 256;
  if (it <= 1) RON_LAUNCH((l2norm_backward_kernel<BF16, 1>), dim3(grid), dim3(256), 0, s, a);
  else if (it <= 2) RON_LAUNCH((l2norm_backward_kernel<BF16, 2>), dim3(grid), dim3(256), 0, s, a);
  else if (it <= 4) RON_LAUNCH((l2norm_backward_kernel<BF16, 4>), dim3(grid), dim3(256), 0, s, a);
  else RON_LAUNCH((l2norm_backward_kernel<BF16, 8>), dim3(grid), dim3(256), 0, s, a);
}

}  // namespace
}  // namespace ron

extern "C" int ron_maxpool3x3s1_backward_nhwc(const float* x, const float* dy, int n, int h, int w, int c, int dtype, float* dx, void* stream) {
  using namespace ron;
  RON_REQUIRE(dtype == RON_DTYPE_BF16 || dtype == RON_DTYPE_F16, "maxpool3x3 backward: dtype %d: bf16 or fp16 only", dtype);
  RON_REQUIRE(n >= 1 && h >= 1 && w >= 1, "maxpool3x3 backward: empty tensor (n %d, h %d, w %d)", n, h, w);
  RON_REQUIRE(c >= 8 && c % 8 == 0, "maxpool3x3 backward: c %d must be a multiple of 8", c);
  int64_t pixels = 0;
  RON_REQUIRE(elems_fit(n, h, w, c, &pixels), "maxpool3x3 backward: tensor of %d x %d x %d x %d elements is beyond 64-bit indexing", n, h, w, c);
  RON_REQUIRE(x != nullptr && dy != nullptr && dx != nullptr, "maxpool3x3 backward: NULL tensor");
  RON_REQUIRE((((uintptr_t)x | (uintptr_t)dy | (uintptr_t)dx) & 15) == 0, "maxpool3x3 backward: x, dy and dx must be 16-byte aligned (16 bytes per access)");
  Pool3Args a = Pool3Args();
  a.x = x; a.dy = dy; a.dx = dx;
  a.h = h; a.w = w; a.c = c;
  a.total = pixels * (c / 4);
  const int grid = grid_for(a.total);
  hipStream_t s = (hipStream_t)stream;
  if (dtype == RON_DTYPE_BF16) RON_LAUNCH(maxpool3x3s1_backward_kernel<true>, dim3(grid), dim3(256), 0, s, a);
  else RON_LAUNCH(maxpool3x3s1_backward_kernel<false>, dim3(grid), dim3(256), 0, s, a);
  RON_HIP_CHECK(ron::launch_error());
  return RON_OK;
}

extern "C" int64_t ron_l2norm_backward_workspace_bytes(int n, int h, int w, int c, int dtype) {
  int64_t pixels = 0;
  if (ron::check_l2_shape(n, h, w, c, dtype, &pixels) != RON_OK) return -1;
  return ron::align_up((int64_t)ron::l2_waves(pixels) * c * 4, 256);
}

extern "C" int ron_l2norm_backward_nhwc(const float* x, const float* gamma, const float* dy, int n, int h, int w, int c, int dtype,
                                        float* dx, float* dgamma, void* workspace, int64_t workspace_bytes, void* stream) {
  using namespace ron;
  int64_t pixels = 0;
  if (int rc = check_l2_shape(n, h, w, c, dtype, &pixels)) return rc;
  const int waves = l2_waves(pixels);
  const int64_t need = align_up((int64_t)waves * c * 4, 256);
  RON_REQUIRE(x != nullptr && gamma != nullptr && dy != nullptr, "l2norm backward: NULL tensor (x, gamma and dy are always read)");
  RON_REQUIRE((((uintptr_t)x | (uintptr_t)gamma | (uintptr_t)dy | (uintptr_t)dx | (uintptr_t)dgamma) & 15) == 0,
              "l2norm backward: x, gamma, dy, dx and dgamma must be 16-byte aligned (16 bytes per access)");
  if (int rc = check_workspace("l2norm backward", "ron_l2norm_backward_workspace_bytes", workspace, workspace_bytes, need)) return rc;
  if (dx == nullptr && dgamma == nullptr) return RON_OK;
  L2Args a = L2Args();
  a.x = x; a.gamma = gamma; a.dy = dy; a.dx = dx;
  a.table = dgamma != nullptr ? static_cast<float*>(workspace) : nullptr;
  a.pixels = pixels; a.c = c; a.waves = waves;
  hipStream_t s = (hipStream_t)stream;
  if (dtype == RON_DTYPE_BF16) launch_l2_backward<true>(a, s);
  else launch_l2_backward<false>(a, s);
  RON_HIP_CHECK(ron::launch_error());
  if (dgamma != nullptr) {
    RON_LAUNCH(l2norm_dgamma_kernel, dim3((c + 31) / 32), dim3(256), 0, s, static_cast<const float*>(workspace), waves, c, dgamma);
    RON_HIP_CHECK(ron::launch_error());
  }
  return RON_OK;
}
