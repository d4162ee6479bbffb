// Device-side one-liners of the pixel kernels (ingest, batching, metrics, resize, blend, 16-bit cache).
#pragma once
#include "common.h"

#ifdef __HIPCC__

// an 8-bit sample as a float in [0, 1]
__device__ __forceinline__ float unit(uint32_t v) { return (float)v / 255.0f; }

// a float sample on the 8-bit grid of the metrics: scaled, clamped to [0, 255], rounded half to even
__device__ __forceinline__ float quantise(float v, float scale) { return rintf(fminf(fmaxf(v * scale, 0.f), 255.f)); }

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : v; }

// 16, 8 or 4: what p is aligned to
__device__ __forceinline__ int align_of(const void* p) {
  const uintptr_t a = (uintptr_t)p;
  return (a & 15) == 0 ? 16 : ((a & 7) == 0 ? 8 : 4);
}

// 4 consecutive floats at p: `align` is 16, 8 or 4, what p is aligned to (uniform over the wave: a property of the row)
__device__ __forceinline__ float4 load_quad(const float* p, int align) {
  if (align == 16) return *reinterpret_cast<const float4*>(p);
  if (align == 8) {
    const float2 a = *reinterpret_cast<const float2*>(p), b = *reinterpret_cast<const float2*>(p + 2);
    return make_float4(a.x, a.y, b.x, b.y);
  }
  return make_float4(p[0], p[1], p[2], p[3]);
}

__device__ __forceinline__ void store_quad(float* p, int align, float4 v) {
  if (align == 16) {
    *reinterpret_cast<float4*>(p) = v;
  } else if (align == 8) {
    *reinterpret_cast<float2*>(p) = make_float2(v.x, v.y);
    *reinterpret_cast<float2*>(p + 2) = make_float2(v.z, v.w);
  } else {
    p[0] = v.x, p[1] = v.y, p[2] = v.z, p[3] = v.w;
  }
}

#endif  // __HIPCC__
