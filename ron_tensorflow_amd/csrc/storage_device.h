// Device helpers of the training kernels (conv_backward.hip, conv_forward_train.hip, conv_chain.hip, conv_wgrad.hip, stem_wgrad.hip,
// op_backward.hip, ssd_backward.hip, batchnorm.hip): ONE definition of how a value becomes a storage-type (bf16 / fp16) value, of how
// eight of them travel as 16 bytes, of how a halo tensor is walked and of the pool's first maximum - plus the weight gradients' MFMA.
//
// The rounding contract.  Every operator carries storage-type values in fp32 at its boundary, and the chain (conv_chain.hip) promises
// the bytes of the operators chained through fp32: that holds because every path below gives the same value for every finite input.
//   * Finite values round to nearest, ties to even, on the dropped mantissa bits; what lies beyond the largest finite storage value
//     by half an ulp or more becomes +-inf; +-0 keep their sign; nothing is flushed: fp32 subnormals round to bf16 subnormals by the
//     same rule (to +-0 in fp16), fp32 normals below the fp16 normal range to fp16 subnormals.
//   * NaN is where the paths differ, and no operator's contract covers one: round_bits sets the quiet bit and drops the low payload
//     (bf16; fp16: the hardware conversion), round_storage returns the fp32 NaN as it came, round_pair does what v_cvt_pk_bf16_f32 does.
//   * round_pair is the hardware conversion, used by stem_wgrad_kernel alone: the integer rounding costs six instructions a value, and
//     that kernel's vector work per byte is what bounds it.  Everything else here uses the integer form for bf16.
//   * The forward boundary (elementwise.hip, Cvt / IO<T>: pack_kernel, the pools, ...) reaches the same values through HIP's
//     __float2bfloat16 and the _Float16 cast; its view_off is halo_off on a view that carries Hp and Wp.
// tests/test_gpu_storage_rounding.py sends one tensor of ties, limits, zeros and subnormals down each path.  The file is compiled
// with and without -ffp-contract=off (Makefile): nothing in it is a floating-point multiply-add.
#pragma once
#include <hip/hip_runtime.h>

namespace ron {

typedef short v4i16 __attribute__((ext_vector_type(4)));
typedef short v8i16 __attribute__((ext_vector_type(8)));
typedef __bf16 v8bf16 __attribute__((ext_vector_type(8)));
typedef _Float16 v8f16 __attribute__((ext_vector_type(8)));
typedef float v4f32 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) v4i16 lds_v4i16;

// ---- fp32 -> storage bits -> fp32 ----------------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned short round_bf16_bits(float f) {
  const unsigned u = __float_as_uint(f);
  if ((u & 0x7FFFFFFFu) > 0x7F800000u) return (unsigned short)((u >> 16) | 0x0040u);      // keep NaN a NaN
  return (unsigned short)((u + 0x7FFFu + ((u >> 16) & 1u)) >> 16);
}
__device__ __forceinline__ unsigned short round_f16_bits(float f) {
  const _Float16 h = (_Float16)f;
  return __builtin_bit_cast(unsigned short, h);
}
template <bool BF16> __device__ __forceinline__ unsigned short round_bits(float f) { return BF16 ? round_bf16_bits(f) : round_f16_bits(f); }
template <bool BF16> __device__ __forceinline__ float bits_to_f(unsigned short b) {
  if (BF16) return __uint_as_float((unsigned)b << 16);
  return (float)__builtin_bit_cast(_Float16, b);
}

// fp32 -> the storage-type value, carried in fp32 (the operators whose tensors stay fp32: pool, L2 norm, batch norm)
__device__ __forceinline__ float round_bf16_f(float f) {
  const unsigned u = __float_as_uint(f);
  if ((u & 0x7FFFFFFFu) > 0x7F800000u) return f;
  return __uint_as_float((u + 0x7FFFu + ((u >> 16) & 1u)) & 0xFFFF0000u);
}
template <bool BF16> __device__ __forceinline__ float round_storage(float f) { return BF16 ? round_bf16_f(f) : (float)(_Float16)f; }

// two values rounded and packed, bf16 through the hardware conversion (v_cvt_pk_bf16_f32): see the contract above
template <bool BF16> __device__ __forceinline__ unsigned round_pair(float lo, float hi) {
  if (BF16) {
    typedef __bf16 v2bf16 __attribute__((ext_vector_type(2)));
    typedef float v2f32 __attribute__((ext_vector_type(2)));
    return __builtin_bit_cast(unsigned, __builtin_convertvector(v2f32{lo, hi}, v2bf16));
  }
  return round_f16_bits(lo) | ((unsigned)round_f16_bits(hi) << 16);
}

// ---- eight adjacent channels: two float4 of fp32, one uint4 of storage bits ----------------------------------------------------------
__device__ __forceinline__ void load8(const float* p, float (&f)[8]) {
  const float4 lo = *reinterpret_cast<const float4*>(p), hi = *reinterpret_cast<const float4*>(p + 4);
  f[0] = lo.x; f[1] = lo.y; f[2] = lo.z; f[3] = lo.w; f[4] = hi.x; f[5] = hi.y; f[6] = hi.z; f[7] = hi.w;
}
// f where m > 0, else 0: the ReLU mask of a backward
__device__ __forceinline__ void keep_positive(float (&f)[8], const float (&m)[8]) {
#pragma unroll
  for (int e = 0; e < 8; ++e) f[e] = m[e] > 0.f ? f[e] : 0.f;
}
__device__ __forceinline__ uint4 pack8_bits(const unsigned short (&h)[8]) {
  uint4 o;
  o.x = h[0] | ((unsigned)h[1] << 16); o.y = h[2] | ((unsigned)h[3] << 16);
  o.z = h[4] | ((unsigned)h[5] << 16); o.w = h[6] | ((unsigned)h[7] << 16);
  return o;
}
template <bool BF16> __device__ __forceinline__ uint4 pack8(const float (&f)[8]) {
  uint4 o;
  o.x = round_bits<BF16>(f[0]) | ((unsigned)round_bits<BF16>(f[1]) << 16);
  o.y = round_bits<BF16>(f[2]) | ((unsigned)round_bits<BF16>(f[3]) << 16);
  o.z = round_bits<BF16>(f[4]) | ((unsigned)round_bits<BF16>(f[5]) << 16);
  o.w = round_bits<BF16>(f[6]) | ((unsigned)round_bits<BF16>(f[7]) << 16);
  return o;
}
template <bool BF16> __device__ __forceinline__ void unpack8(uint4 v, float (&f)[8]) {
  const unsigned u[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    f[2 * e] = bits_to_f<BF16>((unsigned short)(u[e] & 0xFFFFu));
    f[2 * e + 1] = bits_to_f<BF16>((unsigned short)(u[e] >> 16));
  }
}

// ---- halo tensors (TensorView, conv_mfma.h) ---------------------------------------------------------------------------------------------
// element offset of channel 0 of pixel (img, y, x) of an H x W map with halo `pad` and `cs` elements per pixel
__device__ __forceinline__ long long halo_off(long long img, int y, int x, int H, int W, int pad, int cs) {
  return ((img * (H + pad) + y + pad) * (W + pad) + x + pad) * cs;
}
// Pixel b of a buffer whose pixel `guard` is halo pixel 0 of N such maps: is it an interior pixel of one of them, and which; not
// inside are the guards, the halos and whatever lies behind the last map (then img, y and x hold nothing of use).
struct HaloPixel {
  bool inside;
  unsigned img;
  int y, x;
};
__device__ __forceinline__ HaloPixel halo_pixel(unsigned b, long long guard, int N, int H, int W, int pad) {
  HaloPixel p = {false, 0u, 0, 0};
  if (b >= (unsigned)guard) {
    const unsigned Wp = W + pad, Hp = H + pad;
    const unsigned q = b - (unsigned)guard;
    const unsigned r = q / Wp;
    const int col = (int)(q - r * Wp);
    p.img = r / Hp;
    const int row = (int)(r - p.img * Hp);
    p.inside = col >= pad && row >= pad && p.img < (unsigned)N;
    p.y = row - pad; p.x = col - pad;
  }
  return p;
}

// The FIRST maximum of a 2x2 window in the order (0,0) (0,1) (1,0) (1,1) = 0 .. 3: a later position takes over only when it is
// GREATER (TensorFlow's MaxPoolGrad, op_backward.hip).  has_c / has_r: the window has a second column / row (odd maps).
__device__ __forceinline__ int first_max_2x2(float v00, float v01, float v10, float v11, bool has_c, bool has_r) {
  float best = v00;
  int at = 0;
  if (has_c && v01 > best) { best = v01; at = 1; }
  if (has_r && v10 > best) { best = v10; at = 2; }
  if (has_r && has_c && v11 > best) at = 3;
  return at;
}

// ---- the weight gradients' MFMA (conv_wgrad.hip, stem_wgrad.hip) ---------------------------------------------------------------------
template <bool BF16>
__device__ __forceinline__ v4f32 wgrad_mfma(v8i16 a, v8i16 b, v4f32 c) {
  if (BF16) return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(v8bf16, a), __builtin_bit_cast(v8bf16, b), c, 0, 0, 0);
  return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(v8f16, a), __builtin_bit_cast(v8f16, b), c, 0, 0, 0);
}

// the 8 K values (pixel rows 8g .. 8g+7) x 16 channels operand of one lane group, from the image at `img`: two transposed reads
__device__ __forceinline__ v8i16 wgrad_operand(const char* img, int off_lo, int off_hi) {
  const v4i16 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4i16*)(img + off_lo));
  const v4i16 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4i16*)(img + off_hi));
  return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
}

}  // namespace ron
