// Backward of the 2x2 stride-2 SAME max-pool (ron_maxpool2x2_backward_nhwc): pool1 .. pool5 of the VGG body.
//
//   xs = round(x) to the storage type: what ron_maxpool2x2_nhwc pools
//   dx[n,i,j,ch] = round(dy[n,i/2,j/2,ch]) where (i, j) is the FIRST position of its window, in the order (0,0) (0,1) (1,0) (1,1),
//                  whose xs equals the window's maximum; 0 everywhere else
//
// "First maximum" (first_max_2x2, storage_device.h) is TensorFlow's MaxPoolGrad on CPU and GPU (and torch-CPU's max_pool2d backward).  The running maximum starts at
// position (0,0) and a later position takes over only when it is GREATER (>), on the rounded values: two inputs that differ in fp32
// and agree after rounding are a tie, and so are -0.0 and +0.0.  On an odd map the last window holds one row and / or one column:
// positions that do not exist are neither read nor written.  A window that holds a NaN is outside the contract (the forward's fmaxf
// drops NaNs).
//
// Bandwidth bound: one lane = one window x 4 channels = four 16-byte loads of x, one of dy, four 16-byte stores of dx; consecutive
// lanes walk the channels, then the windows, so a wave reads and writes whole rows of pixels.  Every element of dx is written exactly
// once by a plain store: no atomics, no cleared buffer, the same bytes on every call.  64-bit indices, a capped grid with a stride.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "conv_mfma.h"
#include "storage_device.h"      // round_storage, first_max_2x2

namespace ron {
namespace {

RON_KERNEL_ARGS_BEGIN
struct PoolBwdArgs {
  const float* x;
  const float* dy;
  float* dx;
  long long total;          // windows x groups of 4 channels
  int h, w, oh, ow, c;
  int fill_ = 0;
};
RON_KERNEL_ARGS_END(PoolBwdArgs)

template <bool BF16>
__global__ __launch_bounds__(256) void maxpool2x2_backward_kernel(PoolBwdArgs a) {
  const int groups = a.c / 4;
  const long long row = (long long)a.w * a.c;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < a.total; i += (long long)gridDim.x * blockDim.x) {
    const int g = (int)(i % groups);
    const long long win = i / groups;
    const int ox = (int)(win % a.ow);
    const int oy = (int)((win / a.ow) % a.oh);
    const long long img = win / ((long long)a.ow * a.oh);
    const bool has_c = 2 * ox + 1 < a.w, has_r = 2 * oy + 1 < a.h;
    const long long p00 = ((img * a.h + 2 * oy) * a.w + 2 * ox) * a.c + g * 4;
    const float4 v00 = *reinterpret_cast<const float4*>(a.x + p00);
    float4 v01 = v00, v10 = v00, v11 = v00;
    if (has_c) v01 = *reinterpret_cast<const float4*>(a.x + p00 + a.c);
    if (has_r) v10 = *reinterpret_cast<const float4*>(a.x + p00 + row);
    if (has_r && has_c) v11 = *reinterpret_cast<const float4*>(a.x + p00 + row + a.c);
    const float4 gv = *reinterpret_cast<const float4*>(a.dy + i * 4);          // dy [windows][c]: element win * c + 4 g
    const float x00[4] = {v00.x, v00.y, v00.z, v00.w}, x01[4] = {v01.x, v01.y, v01.z, v01.w};
    const float x10[4] = {v10.x, v10.y, v10.z, v10.w}, x11[4] = {v11.x, v11.y, v11.z, v11.w};
    const float gy[4] = {gv.x, gv.y, gv.z, gv.w};
    float o[4][4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int at = first_max_2x2(round_storage<BF16>(x00[e]), round_storage<BF16>(x01[e]), round_storage<BF16>(x10[e]),
                                   round_storage<BF16>(x11[e]), has_c, has_r);
      const float grad = round_storage<BF16>(gy[e]);
#pragma unroll
      for (int p = 0; p < 4; ++p) o[p][e] = at == p ? grad : 0.f;
    }
    *reinterpret_cast<float4*>(a.dx + p00) = make_float4(o[0][0], o[0][1], o[0][2], o[0][3]);
    if (has_c) *reinterpret_cast<float4*>(a.dx + p00 + a.c) = make_float4(o[1][0], o[1][1], o[1][2], o[1][3]);
    if (has_r) *reinterpret_cast<float4*>(a.dx + p00 + row) = make_float4(o[2][0], o[2][1], o[2][2], o[2][3]);
    if (has_r && has_c) *reinterpret_cast<float4*>(a.dx + p00 + row + a.c) = make_float4(o[3][0], o[3][1], o[3][2], o[3][3]);
  }
}

}  // namespace
}  // namespace ron

extern "C" int ron_maxpool2x2_backward_nhwc(const float* x, const float* dy, int n, int h, int w, int c, int dtype, float* dx, void* stream) {
  using namespace ron;
  RON_REQUIRE(dtype == RON_DTYPE_BF16 || dtype == RON_DTYPE_F16, "maxpool backward: dtype %d: bf16 or fp16 only", dtype);
  RON_REQUIRE(n >= 1 && h >= 1 && w >= 1, "maxpool backward: empty tensor (n %d, h %d, w %d)", n, h, w);
  RON_REQUIRE(c >= 8 && c % 8 == 0, "maxpool backward: c %d must be a multiple of 8", c);
  RON_REQUIRE(x != nullptr && dy != nullptr && dx != nullptr, "maxpool backward: NULL tensor");
  RON_REQUIRE((((uintptr_t)x | (uintptr_t)dy | (uintptr_t)dx) & 15) == 0, "maxpool backward: x, dy and dx must be 16-byte aligned (16 bytes per access)");
  PoolBwdArgs a = PoolBwdArgs();
  a.x = x; a.dy = dy; a.dx = dx;
  a.h = h; a.w = w; a.oh = (h + 1) / 2; a.ow = (w + 1) / 2; a.c = c;
  a.total = (long long)n * a.oh * a.ow * (c / 4);
  const int grid = grid_for(a.total);
  hipStream_t s = (hipStream_t)stream;
  if (dtype == RON_DTYPE_BF16) RON_LAUNCH(maxpool2x2_backward_kernel<true>, dim3(grid), dim3(256), 0, s, a);
  else RON_LAUNCH(maxpool2x2_backward_kernel<false>, dim3(grid), dim3(256), 0, s, a);
  RON_HIP_CHECK(ron::launch_error());
  return RON_OK;
}
