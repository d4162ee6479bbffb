// Spatial tiling: frames of any resolution as overlapped tiles.  Two streaming kernels.
//
// ingest_window -- ingest_pad.hip reading a WINDOW [y0, y0 + wh) x [x0, x0 + ww) of frames of h x w, addressed with the frame's pitch:
//   out[f, c, y, x] = conv(src[f, c, y0 + r(y, wh), x0 + r(x, ww)]),  0 <= y < H, 0 <= x < W,  H >= wh, W >= ww
//   r: ingest_pad.hip's reflect / edge index, relative to the window (a padded axis repeats the WINDOW's samples, never the frame's
//   samples outside it); conv: a byte is float(v) / 255.0f as an IEEE division, an fp32 sample is copied as a 32-bit word.
//   Same structure: a workgroup is 4 waves, a wave per output row, a lane per 4 samples, 16-byte stores where W % 4 == 0; a quad left
//   of the window's last column is read with one 32-bit load where ITS address is 4-byte aligned (an fp32 quad: one 16-byte load
//   where it is 16-byte aligned), per-sample loads otherwise -- x0 and a pitch that is no multiple of 4 make that the common case.
//   blockIdx.y = channel, blockIdx.z = frame; row loops in size_t.
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

enum { kU8Planes = 0, kU8Interleaved = 1, kF32Planes = 2 };

__device__ __forceinline__ float unit(uint32_t v) { return (float)v / 255.0f; }

// source index of output index i (i >= 0) on an axis of s samples: inside [0, s)
__device__ __forceinline__ uint32_t src_index(uint32_t i, uint32_t s, int edge) {
  if (i < s) return i;
  if (edge || s == 1) return s - 1;
  const uint32_t period = 2u * (s - 1u);      // s <= 2^31 - 1: no wrap
  const uint32_t m = i % period;
  return m < s ? m : period - m;
}

__device__ __forceinline__ uint32_t load_word(const uint8_t* p) {
  if ((((uintptr_t)p) & 3) == 0) return *reinterpret_cast<const uint32_t*>(p);
  return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}

struct Window {
  uint32_t h, w;        // the frames
  uint32_t y0, x0;      // the window's first row / column
  uint32_t wh, ww;      // its size
  uint32_t H, W;        // the output
};

// planes: T = uint8_t (-> v / 255) or uint32_t (an fp32 sample's bits, copied); VEC: W % 4 == 0, a lane owns 4 samples
template <typename T, bool VEC>
__global__ __launch_bounds__(kLanes* kRows) void ingest_window_planes_kernel(const T* __restrict__ in, float* __restrict__ out, Window g,
                                                                             int edge) {
  const size_t plane = (size_t)blockIdx.z * gridDim.y + blockIdx.y;
  const T* src = in + plane * g.h * g.w + g.x0;      // column x0 of the frame's row 0
  float* dst = out + plane * g.H * g.W;
  const uint32_t cols = VEC ? g.W / 4 : g.W;
  for (size_t y = (size_t)blockIdx.x * kRows + threadIdx.y; y < g.H; y += (size_t)gridDim.x * kRows) {
    const T* row = src + (size_t)(g.y0 + src_index((uint32_t)y, g.wh, edge)) * g.w;
    float* orow = dst + y * g.W;
    for (uint32_t xv = threadIdx.x; xv < cols; xv += kLanes) {
      if constexpr (!VEC) {
        const T v = row[src_index(xv, g.ww, edge)];
        if constexpr (sizeof(T) == 1) orow[xv] = unit(v);
        else reinterpret_cast<uint32_t*>(orow)[xv] = v;
      } else {
        const uint32_t xq = 4 * xv;
        const bool straight = xq + 4 <= g.ww;
        const T* p = row + xq;
        if constexpr (sizeof(T) == 1) {
          uint32_t word;
          if (straight) {
            word = load_word(p);
          } else {
            word = 0;
            for (int j = 0; j < 4; ++j) word |= (uint32_t)row[src_index(xq + j, g.ww, edge)] << (8 * j);
          }
          reinterpret_cast<float4*>(orow)[xv] =
              make_float4(unit(word & 255u), unit((word >> 8) & 255u), unit((word >> 16) & 255u), unit(word >> 24));
        } else {
          uint4 q;
          if (straight && (((uintptr_t)p) & 15) == 0) {
            q = *reinterpret_cast<const uint4*>(p);
          } else if (straight) {
            q = make_uint4(p[0], p[1], p[2], p[3]);
          } else {
            q = make_uint4(row[src_index(xq, g.ww, edge)], row[src_index(xq + 1, g.ww, edge)], row[src_index(xq + 2, g.ww, edge)],
                           row[src_index(xq + 3, g.ww, edge)]);
          }
          reinterpret_cast<uint4*>(orow)[xv] = q;
        }
      }
    }
  }
}

// interleaved: in (F, h, w, 3) -> out (F, 3, H, W); blockIdx.z = frame; a lane owns 4 pixels (VEC) or one, and all three planes
template <bool VEC>
__global__ __launch_bounds__(kLanes* kRows) void ingest_window_interleaved_kernel(const uint8_t* __restrict__ in, float* __restrict__ out,
                                                                                  Window g, int edge) {
  const size_t f = blockIdx.z;
  const size_t HW = (size_t)g.H * g.W;
  const uint8_t* src = in + f * g.h * g.w * 3 + (size_t)g.x0 * 3;
  float* dst = out + f * HW * 3;
  const uint32_t cols = VEC ? g.W / 4 : g.W;
  for (size_t y = (size_t)blockIdx.x * kRows + threadIdx.y; y < g.H; y += (size_t)gridDim.x * kRows) {
    const uint8_t* row = src + (size_t)(g.y0 + src_index((uint32_t)y, g.wh, edge)) * g.w * 3;
    float* orow = dst + y * g.W;
    for (uint32_t xv = threadIdx.x; xv < cols; xv += kLanes) {
      if constexpr (!VEC) {
        const uint8_t* px = row + (size_t)src_index(xv, g.ww, edge) * 3;
        for (int c = 0; c < 3; ++c) orow[c * HW + xv] = unit(px[c]);
      } else {
        const uint32_t xq = 4 * xv;
        uint32_t a, b, c;      // bytes r0 g0 b0 r1 | g1 b1 r2 g2 | b2 r3 g3 b3
        if (xq + 4 <= g.ww) {
          const uint8_t* p = row + (size_t)xq * 3;      // p, p + 4, p + 8 are aligned together
          a = load_word(p), b = load_word(p + 4), c = load_word(p + 8);
        } else {
          const uint8_t* p0 = row + (size_t)src_index(xq, g.ww, edge) * 3;
          const uint8_t* p1 = row + (size_t)src_index(xq + 1, g.ww, edge) * 3;
          const uint8_t* p2 = row + (size_t)src_index(xq + 2, g.ww, edge) * 3;
          const uint8_t* p3 = row + (size_t)src_index(xq + 3, g.ww, edge) * 3;
          a = (uint32_t)p0[0] | ((uint32_t)p0[1] << 8) | ((uint32_t)p0[2] << 16) | ((uint32_t)p1[0] << 24);
          b = (uint32_t)p1[1] | ((uint32_t)p1[2] << 8) | ((uint32_t)p2[0] << 16) | ((uint32_t)p2[1] << 24);
          c = (uint32_t)p2[2] | ((uint32_t)p3[0] << 8) | ((uint32_t)p3[1] << 16) | ((uint32_t)p3[2] << 24);
        }
        reinterpret_cast<float4*>(orow)[xv] = make_float4(unit(a & 255u), unit(a >> 24), unit((b >> 16) & 255u), unit((c >> 8) & 255u));
        reinterpret_cast<float4*>(orow + HW)[xv] =
            make_float4(unit((a >> 8) & 255u), unit(b & 255u), unit(b >> 24), unit((c >> 16) & 255u));
        reinterpret_cast<float4*>(orow + 2 * HW)[xv] =
            make_float4(unit((a >> 16) & 255u), unit((b >> 8) & 255u), unit(c & 255u), unit(c >> 24));
      }
    }
  }
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

// row groups per plane, capped as ingest_pad.hip caps its grid: about 2048 workgroups in all, the rest is the grid-stride loop
unsigned row_blocks(int32_t H, size_t planes) {
  const size_t want = ((size_t)H + kRows - 1) / kRows;
  const size_t cap = planes >= 2048 ? 1 : 2048 / planes;
  return (unsigned)(want < cap ? want : cap);
}

}  // namespace

extern "C" int eavsr_ingest_window(const void* in, float* out, int32_t F, int32_t C, int32_t h, int32_t w, int32_t y0, int32_t x0,
                                   int32_t wh, int32_t ww, int32_t H, int32_t W, int32_t kind, int32_t mode, void* stream) {
  EAVSR_REQUIRE(in && out, -1, "ingest_window: NULL pointer");
  EAVSR_REQUIRE(F >= 0 && F <= 65535 && C >= 1 && C <= 65535 && h >= 1 && w >= 1, -2, "ingest_window: bad dims F=%d C=%d h=%d w=%d", F, C, h,
                w);
  EAVSR_REQUIRE(y0 >= 0 && x0 >= 0 && wh >= 1 && ww >= 1 && wh <= h - y0 && ww <= w - x0, -2,
                "ingest_window: the window [%d, %d + %d) x [%d, %d + %d) does not lie inside frames of %d x %d", y0, y0, wh, x0, x0, ww, h, w);
  EAVSR_REQUIRE(H >= wh && W >= ww, -2, "ingest_window: the output %d x %d is smaller than the window %d x %d (padding only)", H, W, wh, ww);
  EAVSR_REQUIRE(kind == kU8Planes || kind == kU8Interleaved || kind == kF32Planes, -2,
                "ingest_window: kind %d (0 = uint8 planes (F, C, h, w), 1 = uint8 interleaved (F, h, w, 3), 2 = fp32 planes)", kind);
  EAVSR_REQUIRE(mode == 0 || mode == 1, -2, "ingest_window: mode %d (0 = reflect, 1 = edge)", mode);
  EAVSR_REQUIRE(kind != kU8Interleaved || C == 3, -2, "ingest_window: an interleaved source has 3 channels, got C=%d", C);
  EAVSR_REQUIRE((((uintptr_t)out) & 15) == 0, -2, "ingest_window: out must be 16-byte aligned");
  EAVSR_REQUIRE(kind != kF32Planes || (((uintptr_t)in) & 3) == 0, -2, "ingest_window: an fp32 source must be 4-byte aligned");
  if (F == 0) return 0;
  hipStream_t st = eavsr::as_stream(stream);
  const dim3 block(kLanes, kRows);
  const Window g{(uint32_t)h, (uint32_t)w, (uint32_t)y0, (uint32_t)x0, (uint32_t)wh, (uint32_t)ww, (uint32_t)H, (uint32_t)W};
  const bool vec = W % 4 == 0;
  if (kind == kU8Interleaved) {
    const dim3 grid(row_blocks(H, (size_t)F), 1, F);
    const uint8_t* src = static_cast<const uint8_t*>(in);
    if (vec) hipLaunchKernelGGL(ingest_window_interleaved_kernel<true>, grid, block, 0, st, src, out, g, mode);
    else hipLaunchKernelGGL(ingest_window_interleaved_kernel<false>, grid, block, 0, st, src, out, g, mode);
  } else {
    const dim3 grid(row_blocks(H, (size_t)F * C), C, F);
    if (kind == kU8Planes) {
      const uint8_t* src = static_cast<const uint8_t*>(in);
      if (vec) hipLaunchKernelGGL((ingest_window_planes_kernel<uint8_t, true>), grid, block, 0, st, src, out, g, mode);
      else hipLaunchKernelGGL((ingest_window_planes_kernel<uint8_t, false>), grid, block, 0, st, src, out, g, mode);
    } else {
      const uint32_t* src = static_cast<const uint32_t*>(in);
      if (vec) hipLaunchKernelGGL((ingest_window_planes_kernel<uint32_t, true>), grid, block, 0, st, src, out, g, mode);
      else hipLaunchKernelGGL((ingest_window_planes_kernel<uint32_t, false>), grid, block, 0, st, src, out, g, mode);
    }
  }
  return eavsr::launch_status("ingest_window");
}

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
  const dim3 grid(row_blocks(th, (size_t)N * F * C), C, N * F);
  hipLaunchKernelGGL(tile_blend_kernel, grid, dim3(kLanes, kRows), 0, eavsr::as_stream(stream), acc, sr, wy, wx, g);
  return eavsr::launch_status("tile_blend");
}
