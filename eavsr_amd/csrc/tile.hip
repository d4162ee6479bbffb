// Spatial tiling: frames of any resolution as overlapped tiles.  A tile's frames are read by the windowed ingest of
// ingest_pad.hip (eavsr_ingest_window); this file holds the blend.
//
// tile_blend -- one SR tile into the accumulator of the frame:
//   acc[n, f, c, Y0 + y, X0 + x] += (wy[y] * wx[x]) * sr[n, f, c, y, x]
//   three separately rounded fp32 operations in that order (the product is kept from being contracted into the sum: a fused
//   multiply-add would round once where the definition rounds twice).  acc is contiguous (N, F, C, SH, SW); sr has element strides
//   on n, f, c and rows and unit stride along x.  A wave per row, wy[y] read once per row, a lane per 4 samples: 16-byte accesses where the row's
//   address is 16-byte aligned, 8-byte ones where it is 8-byte aligned (x2 network, odd window start), single words otherwise --
//   decided per row and per operand, uniform over the wave.  Tiles are blended one after another on one stream: plain stores.
#include "common.h"

#include <stdint.h>

namespace {

constexpr int kLanes = 64;      // threadIdx.x: along the row
constexpr int kRows = 4;        // threadIdx.y: one wave per row

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

__device__ __forceinline__ int align_of(const void* p) {
  const uintptr_t a = (uintptr_t)p;
  return (a & 15) == 0 ? 16 : ((a & 7) == 0 ? 8 : 4);
}

// a (+)= (wy * wx) * v: two products and a sum, each rounded on its own.  The library is built with -ffp-contract=fast, under which
// the backend fuses a product into the sum that follows it whatever the source says (the pragma below clears the per-operation
// permission, the global one remains; __fmul_rn / __fadd_rn are plain operators in this toolchain and fuse as well): the empty
// asm makes the rounded product a value the compiler has to materialise before it adds.
__device__ __forceinline__ float blend(float a, float wy, float wx, float v) {
#pragma clang fp contract(off)
  const float w = wy * wx;
  float p = w * v;
  asm volatile("" : "+v"(p));
  return a + p;
}

struct Blend {
  uint32_t F, C;            // frames per clip, channels (blockIdx.z = n F + f, blockIdx.y = c)
  uint32_t SH, SW;          // the accumulator's frames
  uint32_t th, tw;          // the tile
  uint32_t Y0, X0;          // where it goes
  int64_t sn, sf, sc, sy;   // the tile's strides, in elements
};

__global__ __launch_bounds__(kLanes* kRows) void tile_blend_kernel(float* __restrict__ acc, const float* __restrict__ sr,
                                                                   const float* __restrict__ wy, const float* __restrict__ wx, Blend g) {
  const uint32_t n = blockIdx.z / g.F, f = blockIdx.z - n * g.F;      // once per workgroup, on the scalar unit
  const size_t plane = (size_t)blockIdx.z * g.C + blockIdx.y;
  float* dst = acc + (plane * g.SH + g.Y0) * g.SW + g.X0;
  const float* src = sr + (int64_t)n * g.sn + (int64_t)f * g.sf + (int64_t)blockIdx.y * g.sc;
  const uint32_t quads = g.tw / 4;
  const int wx_align = align_of(wx);
  for (size_t y = (size_t)blockIdx.x * kRows + threadIdx.y; y < g.th; y += (size_t)gridDim.x * kRows) {
    float* arow = dst + y * g.SW;
    const float* srow = src + (int64_t)y * g.sy;
    const float wyv = wy[y];
    const int a_align = align_of(arow), s_align = align_of(srow);
    for (uint32_t xv = threadIdx.x; xv < quads; xv += kLanes) {
      const uint32_t x = 4 * xv;
      const float4 a = load_quad(arow + x, a_align), v = load_quad(srow + x, s_align), w = load_quad(wx + x, wx_align);
      store_quad(arow + x, a_align,
                 make_float4(blend(a.x, wyv, w.x, v.x), blend(a.y, wyv, w.y, v.y), blend(a.z, wyv, w.z, v.z), blend(a.w, wyv, w.w, v.w)));
    }
    const uint32_t x = 4 * quads + threadIdx.x;      // the 0 .. 3 samples past the last quad
    if (x < g.tw) arow[x] = blend(arow[x], wyv, wx[x], srow[x]);
  }
}

}  // namespace

extern "C" int eavsr_tile_blend_f32(float* acc, const float* sr, const float* wy, const float* wx, int32_t N, int32_t F, int32_t C, int32_t SH,
                                    int32_t SW, int32_t th, int32_t tw, int32_t Y0, int32_t X0, int64_t sn, int64_t sf, int64_t sc, int64_t sy,
                                    void* stream) {
  EAVSR_REQUIRE(acc && sr && wy && wx, -1, "tile_blend: NULL pointer");
  EAVSR_REQUIRE(N >= 0 && F >= 0 && C >= 1 && C <= 65535 && SH >= 1 && SW >= 1 && (int64_t)N * F <= 65535, -2,
                "tile_blend: bad dims N=%d F=%d C=%d SH=%d SW=%d (N F and C: at most 65535)", N, F, C, SH, SW);
  EAVSR_REQUIRE(th >= 1 && tw >= 1 && Y0 >= 0 && X0 >= 0 && th <= SH - Y0 && tw <= SW - X0, -2,
                "tile_blend: the tile [%d, %d + %d) x [%d, %d + %d) does not lie inside frames of %d x %d", Y0, Y0, th, X0, X0, tw, SH, SW);
  EAVSR_REQUIRE(sn >= 0 && sf >= 0 && sc >= 0 && sy >= tw, -2, "tile_blend: strides n=%lld f=%lld c=%lld row=%lld (in elements; rows >= %d)",
                (long long)sn, (long long)sf, (long long)sc, (long long)sy, tw);
  EAVSR_REQUIRE(((((uintptr_t)acc) | ((uintptr_t)sr) | ((uintptr_t)wy) | ((uintptr_t)wx)) & 3) == 0, -2,
                "tile_blend: pointers must be 4-byte aligned");
  if (N == 0 || F == 0) return 0;
  const Blend g{(uint32_t)F, (uint32_t)C, (uint32_t)SH, (uint32_t)SW, (uint32_t)th, (uint32_t)tw, (uint32_t)Y0, (uint32_t)X0, sn, sf, sc, sy};
  const dim3 grid(eavsr::row_blocks(th, kRows, (size_t)N * F * C), C, N * F);
  hipLaunchKernelGGL(tile_blend_kernel, grid, dim3(kLanes, kRows), 0, eavsr::as_stream(stream), acc, sr, wy, wx, g);
  return eavsr::launch_status("tile_blend");
}
