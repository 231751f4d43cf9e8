// Device helpers the weight-gradient kernels and the training packs share (conv_wgrad.hip, stem_wgrad.hip, conv_backward.hip,
// conv_forward_train.hip): the roundings to the storage type, the v_mfma_f32_16x16x32 wrapper and the transposed LDS read that feeds it.
#pragma once
#include <hip/hip_runtime.h>

namespace ron {
namespace wgrad {

typedef short v4i16 __attribute__((ext_vector_type(4)));
typedef short v8i16 __attribute__((ext_vector_type(8)));
typedef __bf16 v8bf16 __attribute__((ext_vector_type(8)));
typedef _Float16 v8f16 __attribute__((ext_vector_type(8)));
typedef float v4f32 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) v4i16 lds_v4i16;

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

}  // namespace wgrad
}  // namespace ron
