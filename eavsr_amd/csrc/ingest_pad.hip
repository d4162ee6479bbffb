// Padded and windowed ingest: frames of any size, or a window of them, -> fp32 planes of the size the network takes, in
// one launch.  One kernel family: the window [y0, y0 + wh) x [x0, x0 + ww) of frames of h x w, addressed with the frame's pitch;
// eavsr_ingest_pad is eavsr_ingest_window with the whole frame as its window (y0 = x0 = 0, wh = h, ww = w).
//   out[f, c, y, x] = conv(src[f, c, y0 + r(y, wh), x0 + r(x, ww)]),  0 <= y < H, 0 <= x < W,  H >= wh, W >= ww: padding at the bottom
//   and right only, and a padded axis repeats the WINDOW's samples, never the frame's samples outside it.
//   reflect: r(i, s) = (m < s ? m : 2 (s - 1) - m) with m = i mod 2 (s - 1), 0 for s = 1 -- numpy's np.pad(mode="reflect") for every
//            pad width, pads several times the size included;   edge: r(i, s) = min(i, s - 1).
//   conv: a byte becomes float(v) / 255.0f as an IEEE division (ingest.hip says why not a multiplication); an fp32 sample is copied
//         bit for bit (as a 32-bit word: no float instruction touches it).
// Sources: uint8 planes (F, C, h, w), uint8 interleaved (F, h, w, 3), fp32 planes (F, C, h, w); any base byte alignment for bytes.
//
// Pure streaming, as ingest.hip.  A workgroup is 4 waves, each wave one output row: lane l owns samples 4 l .. 4 l + 3 of it (and
// 4 (l + 64) .., a loop), one 16-byte store where W % 4 == 0 -- what the model asks for; any other W takes one sample (interleaved:
// one pixel) per lane with scalar stores.  A reflected ROW is another source row and costs nothing; a quad is "straight" while it
// lies left of the window's last column (4 xv + 4 <= ww): then a byte source is read with one 32-bit load where ITS address is
// 4-byte aligned (three for the 12 bytes of an interleaved quad), an fp32 source with one 16-byte load where it is 16-byte aligned,
// per-sample loads otherwise -- under a window, x0 and a pitch that is no multiple of 4 make that the common case.  The quads right
// of that -- the reflected columns, a few percent of a frame -- are per-sample loads.
// blockIdx.y = channel (planes), blockIdx.z = frame: no division anywhere; the row loop is a grid-stride loop in size_t.
#include "pixel.h"

#include <stdint.h>

namespace {

constexpr int kLanes = 64;      // threadIdx.x: along the row
constexpr int kRows = 4;        // threadIdx.y: one wave per row

enum { kU8Planes = 0, kU8Interleaved = 1, kF32Planes = 2 };

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
__global__ __launch_bounds__(kLanes* kRows) void ingest_planes_kernel(const T* __restrict__ in, float* __restrict__ out, Window g, int edge) {
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
__global__ __launch_bounds__(kLanes* kRows) void ingest_interleaved_kernel(const uint8_t* __restrict__ in, float* __restrict__ out, Window g,
                                                                           int edge) {
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

// What both entry points refuse, under the caller's name `who`, then the one launch.  The entry points have checked the window
// against the frames and the output against the window: g's fields are what they were given, each >= 0.
int launch_ingest(const void* in, float* out, int32_t F, int32_t C, const Window& g, int32_t kind, int32_t mode, void* stream,
                  const char* who) {
  EAVSR_REQUIRE(in && out, -1, "%s: NULL pointer", who);
  EAVSR_REQUIRE(F >= 0 && F <= 65535 && C >= 1 && C <= 65535, -2, "%s: bad dims F=%d C=%d (at most 65535 each)", who, F, C);
  EAVSR_REQUIRE(kind == kU8Planes || kind == kU8Interleaved || kind == kF32Planes, -2,
                "%s: kind %d (0 = uint8 planes (F, C, h, w), 1 = uint8 interleaved (F, h, w, 3), 2 = fp32 planes)", who, kind);
  EAVSR_REQUIRE(mode == 0 || mode == 1, -2, "%s: mode %d (0 = reflect, 1 = edge)", who, mode);
  EAVSR_REQUIRE(kind != kU8Interleaved || C == 3, -2, "%s: an interleaved source has 3 channels, got C=%d", who, C);
  EAVSR_REQUIRE((((uintptr_t)out) & 15) == 0, -2, "%s: out must be 16-byte aligned", who);
  EAVSR_REQUIRE(kind != kF32Planes || (((uintptr_t)in) & 3) == 0, -2, "%s: an fp32 source must be 4-byte aligned", who);
  if (F == 0) return 0;
  hipStream_t st = eavsr::as_stream(stream);
  const dim3 block(kLanes, kRows);
  const bool vec = g.W % 4 == 0;
  if (kind == kU8Interleaved) {
    const dim3 grid(eavsr::row_blocks(g.H, kRows, (size_t)F), 1, F);
    const uint8_t* src = static_cast<const uint8_t*>(in);
    if (vec) hipLaunchKernelGGL(ingest_interleaved_kernel<true>, grid, block, 0, st, src, out, g, mode);
    else hipLaunchKernelGGL(ingest_interleaved_kernel<false>, grid, block, 0, st, src, out, g, mode);
  } else {
    const dim3 grid(eavsr::row_blocks(g.H, kRows, (size_t)F * C), C, F);
    if (kind == kU8Planes) {
      const uint8_t* src = static_cast<const uint8_t*>(in);
      if (vec) hipLaunchKernelGGL((ingest_planes_kernel<uint8_t, true>), grid, block, 0, st, src, out, g, mode);
      else hipLaunchKernelGGL((ingest_planes_kernel<uint8_t, false>), grid, block, 0, st, src, out, g, mode);
    } else {
      const uint32_t* src = static_cast<const uint32_t*>(in);
      if (vec) hipLaunchKernelGGL((ingest_planes_kernel<uint32_t, true>), grid, block, 0, st, src, out, g, mode);
      else hipLaunchKernelGGL((ingest_planes_kernel<uint32_t, false>), grid, block, 0, st, src, out, g, mode);
    }
  }
  return eavsr::launch_status(who);
}

}  // namespace

extern "C" int eavsr_ingest_pad(const void* in, float* out, int32_t F, int32_t C, int32_t h, int32_t w, int32_t H, int32_t W, int32_t kind,
                                int32_t mode, void* stream) {
  EAVSR_REQUIRE(h >= 1 && w >= 1, -2, "ingest_pad: bad dims h=%d w=%d", h, w);
  EAVSR_REQUIRE(H >= h && W >= w, -2, "ingest_pad: the output %d x %d is smaller than the source %d x %d (padding only)", H, W, h, w);
  const Window g{(uint32_t)h, (uint32_t)w, 0u, 0u, (uint32_t)h, (uint32_t)w, (uint32_t)H, (uint32_t)W};
  return launch_ingest(in, out, F, C, g, kind, mode, stream, "ingest_pad");
}

extern "C" int eavsr_ingest_window(const void* in, float* out, int32_t F, int32_t C, int32_t h, int32_t w, int32_t y0, int32_t x0,
                                   int32_t wh, int32_t ww, int32_t H, int32_t W, int32_t kind, int32_t mode, void* stream) {
  EAVSR_REQUIRE(h >= 1 && w >= 1, -2, "ingest_window: bad dims h=%d w=%d", h, w);
  EAVSR_REQUIRE(y0 >= 0 && x0 >= 0 && wh >= 1 && ww >= 1 && wh <= h - y0 && ww <= w - x0, -2,
                "ingest_window: the window [%d, %d + %d) x [%d, %d + %d) does not lie inside frames of %d x %d", y0, y0, wh, x0, x0, ww, h, w);
  EAVSR_REQUIRE(H >= wh && W >= ww, -2, "ingest_window: the output %d x %d is smaller than the window %d x %d (padding only)", H, W, wh, ww);
  const Window g{(uint32_t)h, (uint32_t)w, (uint32_t)y0, (uint32_t)x0, (uint32_t)wh, (uint32_t)ww, (uint32_t)H, (uint32_t)W};
  return launch_ingest(in, out, F, C, g, kind, mode, stream, "ingest_window");
}
