// fp32 <-> fp16 / bf16, one element: the rounding of the 16-bit feature cache (cache16.hip) and of the range census of the 16-bit
// backbone (range16.hip) -- one definition, so that "counted as rounded" means the bits the pack kernels write.
//
// round16 -- to nearest even.  fp16: the hardware convert (v_cvt_f16_f32 under the default mode: overflow to +-inf from 65520 on,
//            subnormals produced, NaN quieted).  bf16: in integer arithmetic, (u + 0x7FFF + ((u >> 16) & 1)) >> 16, a NaN written as
//            0x7FC0 as torch writes it.  +-0 keep their sign.
// widen16 -- exact (fp16: v_cvt_f32_f16, subnormals included; bf16: the 16 bits moved up).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace round16_ns {

template <int BF16>
__device__ __forceinline__ uint32_t round16(float x) {
  if (BF16) {
    const uint32_t u = __float_as_uint(x);
    if ((u & 0x7FFFFFFFu) > 0x7F800000u) return 0x7FC0u;      // NaN: torch's
    return (u + 0x7FFFu + ((u >> 16) & 1u)) >> 16;             // nearest even; the carry out of the mantissa is the overflow to inf
  }
  const _Float16 h = (_Float16)x;
  return (uint32_t)__builtin_bit_cast(uint16_t, h);
}

template <int BF16>
__device__ __forceinline__ float widen16(uint32_t b) {
  if (BF16) return __uint_as_float(b << 16);
  return (float)__builtin_bit_cast(_Float16, (uint16_t)b);
}

}  // namespace round16_ns
