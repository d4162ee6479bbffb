// The census of the 16-bit feature cache (addendum): what rounding fp32 features to fp16 / bf16 did, counted inside the
// launch that rounds them (`pack16_census_kernel`, cache16.hip).  Every count is a function of an element's fp32 bits u and its
// 16-bit result o alone, so the reference is one numpy line each (tests/census_ref.py):
//
//   slot 0  max_abs    max of a = u & 0x7FFFFFFF over the finite elements (a < 0x7F800000), kept as the integer: the order of the
//                      non-negative floats is the order of their bits
//   slot 1  nonfinite  a >= 0x7F800000: inf or NaN going in
//   slot 2  overflow   finite in, +-inf out: (o & 0x7FFF) == 0x7C00 (fp16) / 0x7F80 (bf16)
//   slot 3  flushed    finite and non-zero in, +-0 out
//   slot 4  subnormal  out: a zero exponent field and a non-zero mantissa, 0 < (o & 0x7FFF) < 0x0400 (fp16) / 0x0080 (bf16)
//
// A lane keeps the five values in registers over all its items and all passes of the grid stride (`Tally`); `commit` then combines
// the 64 lanes of a wave by cross-lane moves, the four waves of the workgroup through 4 x 5 words of LDS, and lane 0 adds the
// workgroup's values to the record with at most one atomicMax / atomicAdd per slot, skipping a slot whose value is 0 -- with
// nothing non-finite, overflowed or flushed that is two operations per workgroup.  Integer max and integer add do not depend on
// order: two launches give the same record, and launches may add into one record.  The number of elements is the caller's.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace census16 {

constexpr int kSlots = 5;
constexpr int kWaves = 4;      // of 64 lanes: cache16.hip's workgroup of 256

struct Tally {
  unsigned long long v[kSlots];

  __device__ __forceinline__ void clear() {
#pragma unroll
    for (int k = 0; k < kSlots; ++k) v[k] = 0;
  }

  // one element: its fp32 bits and its 16-bit result
  template <int BF16>
  __device__ __forceinline__ void count(uint32_t u, uint32_t o) {
    const uint32_t a = u & 0x7FFFFFFFu, r = o & 0x7FFFu;
    const bool finite = a < 0x7F800000u;
    if (finite && a > v[0]) v[0] = a;
    v[1] += finite ? 0u : 1u;
    v[2] += (finite && r == (BF16 ? 0x7F80u : 0x7C00u)) ? 1u : 0u;
    v[3] += (finite && a != 0u && r == 0u) ? 1u : 0u;
    v[4] += (r != 0u && r < (BF16 ? 0x0080u : 0x0400u)) ? 1u : 0u;
  }

  // every lane of the workgroup calls this once, outside divergent control flow
  __device__ __forceinline__ void commit(unsigned long long* record) {
    __shared__ unsigned long long part[kWaves][kSlots];
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
      const unsigned long long m = __shfl_down(v[0], d, 64);
      v[0] = m > v[0] ? m : v[0];
#pragma unroll
      for (int k = 1; k < kSlots; ++k) v[k] += __shfl_down(v[k], d, 64);
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
#pragma unroll
      for (int k = 0; k < kSlots; ++k) part[wave][k] = v[k];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      unsigned long long t[kSlots];
#pragma unroll
      for (int k = 0; k < kSlots; ++k) t[k] = part[0][k];
#pragma unroll
      for (int w = 1; w < kWaves; ++w) {
        t[0] = part[w][0] > t[0] ? part[w][0] : t[0];
#pragma unroll
        for (int k = 1; k < kSlots; ++k) t[k] += part[w][k];
      }
      if (t[0]) atomicMax(record, t[0]);
#pragma unroll
      for (int k = 1; k < kSlots; ++k)
        if (t[k]) atomicAdd(record + k, t[k]);
    }
  }
};

}  // namespace census16
