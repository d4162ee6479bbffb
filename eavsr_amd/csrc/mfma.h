// Device-side vector types, the exact bf16 split and the 32x32x16 MFMA wrappers shared by the matrix-pipe kernels (gfx950 only).
#pragma once
#include "common.h"

#ifdef __HIPCC__

typedef const __attribute__((address_space(1))) void* gptr_t;
typedef __attribute__((address_space(3))) void* lptr_t;
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 h16x8 __attribute__((ext_vector_type(8)));

// exact three-way split of two fp32 values into packed bf16 pairs (low half = first value)
__device__ __forceinline__ void eavsr_split2(float a, float b, unsigned& hi, unsigned& mid, unsigned& lo) {
  const unsigned ua = __float_as_uint(a), ub = __float_as_uint(b);
  const float ra = a - __uint_as_float(ua & 0xFFFF0000u), rb = b - __uint_as_float(ub & 0xFFFF0000u);
  const unsigned uma = __float_as_uint(ra), umb = __float_as_uint(rb);
  const float la = ra - __uint_as_float(uma & 0xFFFF0000u), lb = rb - __uint_as_float(umb & 0xFFFF0000u);
  // v_perm_b32: bytes 2,3 of the first value into the low half, bytes 2,3 of the second into the high half
  hi = __builtin_amdgcn_perm(ub, ua, 0x07060302u);
  mid = __builtin_amdgcn_perm(umb, uma, 0x07060302u);
  lo = __builtin_amdgcn_perm(__float_as_uint(lb), __float_as_uint(la), 0x07060302u);
}

// two fp32 values rounded to nearest even into one packed bf16 pair (low half = first value): v_cvt_pk_bf16_f32, what
// torch.Tensor.to(torch.bfloat16) computes (no truncation)
__device__ __forceinline__ unsigned eavsr_rne2(float a, float b) {
  typedef __bf16 b2_ __attribute__((ext_vector_type(2)));
  return __builtin_bit_cast(unsigned, __builtin_convertvector(f32x2{a, b}, b2_));
}

// v_mfma_f32_32x32x16_{bf16,f16}: operands as the four dwords a lane holds (eight 16-bit values of K)
__device__ __forceinline__ f32x16 eavsr_mfma_bf16(const u32x4& a, const u32x4& b, const f32x16& c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}
__device__ __forceinline__ f32x16 eavsr_mfma_f16(const u32x4& a, const u32x4& b, const f32x16& c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(h16x8, a), __builtin_bit_cast(h16x8, b), c, 0, 0, 0);
}
template <bool BF16>
__device__ __forceinline__ f32x16 eavsr_mfma16(const u32x4& a, const u32x4& b, const f32x16& c) {
  if (BF16) return eavsr_mfma_bf16(a, b, c);
  else return eavsr_mfma_f16(a, b, c);
}
// the same on operands that the kernel keeps as f32x4 (what its ds_read_b128 returns)
template <bool BF16>
__device__ __forceinline__ f32x16 eavsr_mfma16(const f32x4& a, const f32x4& b, const f32x16& c) {
  return eavsr_mfma16<BF16>(__builtin_bit_cast(u32x4, a), __builtin_bit_cast(u32x4, b), c);
}

#endif  // __HIPCC__
