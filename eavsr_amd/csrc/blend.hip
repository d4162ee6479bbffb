// The output side of spatial tiling and of self-ensemble inference: SR tiles, under any of the eight flips
// and transposes of the frame, into the accumulator of the frame -- and the flips and transposes themselves on the way into the
// network.  (A tile's frames are read by the windowed ingest of ingest_pad.hip, eavsr_ingest_window.)  Mode k: bit 0 hflip, bit 1
// vflip, bit 2 transpose, applied in that order on the last two axes (the `flags` of batch.hip):
//   g_k(x)[i, j]   = x[vflip ? H-1-r : r, hflip ? W-1-q : q],  (r, q) = (j, i) if transposed (the result is W x H), else (i, j)
//   inv_k(z)[y, x] = z[R, Q],  (R, Q) = (x', y') if transposed, else (y', x'),  y' = vflip ? th-1-y : y,  x' = hflip ? tw-1-x : x
//
// dihedral -- out = g_k(in) for fp32 (F, C, H, W) planes, a bit copy.
// blend    -- acc[n, f, c, Y0 + y, X0 + x] += (wy[y] * wx[x]) * inv_k(sr)[n, f, c, y, x]
//   three separately rounded fp32 operations in that order (see blend() below).  acc is contiguous (N, F, C, SH, SW); sr has element
//   strides on n, f, c and rows and unit stride along its rows.  Calls are made one after another on one stream: plain stores.
//   eavsr_tile_blend_f32 is mode 0, eavsr_blend_dihedral_f32 any mode.
//
// Modes without the transpose: a wave per destination row, wy[y] read once per row, a lane per 4 samples: 16-byte accesses where the
// row's address is 16-byte aligned, 8-byte ones where it is 8-byte aligned (x2 network, odd window start), single words otherwise --
// decided per row and per operand, uniform over the wave.  A mirrored row is read as mirrored quads with their components reversed;
// whether it is mirrored is a template parameter of the blend (it sits inside the quad loop: mode 0 is the kernel with the flips
// compiled out), the row flip one address select per row.  Modes with the transpose: a workgroup owns a 64 x 64 tile of the
// SOURCE, reads its rows along their unit stride into LDS with a row pitch of 65 dwords, and writes (blends) destination rows along
// THEIR unit stride from LDS columns; with the odd pitch lane l of a row write hits bank (65 r + l) mod 64 and lane l of a column read
// bank (65 l + c) mod 64: distinct per lane.  The flips move the tile's destination coordinates.  Tiles have tails on both axes.
#include "pixel.h"

#include <stdint.h>

namespace {

constexpr int kLanes = 64;      // threadIdx.x: along the row
constexpr int kRows = 4;        // threadIdx.y: one wave per row
constexpr int kTile = 64;       // the transposing kernels' square tile
constexpr int kPitch = 65;      // its row pitch in LDS, dwords: odd

// the quad of a row of `w` samples that a mirrored row shows at x = 4 xv .. 4 xv + 3: samples w - 4 - x .. w - 1 - x, reversed.
// `tail` = row + (w & 3), where the row's last whole quad counted from its END starts; all quads lie 16 bytes apart from it.
__device__ __forceinline__ float4 load_mirrored(const float* tail, uint32_t quads, uint32_t xv, int align) {
  const float4 v = load_quad(tail + 4 * (size_t)(quads - 1 - xv), align);
  return make_float4(v.w, v.z, v.y, v.x);
}

// a (+)= (wy * wx) * v: two products and a sum, each rounded on its own (a fused multiply-add would round once where the definition
// rounds twice).  The library is built with -ffp-contract=fast, under which the backend fuses a product into the sum that follows
// it whatever the source says (the pragma below clears the per-operation permission, the global one remains; __fmul_rn / __fadd_rn
// are plain operators in this toolchain and fuse as well): the empty asm makes the rounded product a value the compiler has to
// materialise before it adds.
__device__ __forceinline__ float blend(float a, float wy, float wx, float v) {
#pragma clang fp contract(off)
  const float w = wy * wx;
  float p = w * v;
  asm volatile("" : "+v"(p));
  return a + p;
}

// -- dihedral, modes 0 .. 3: blockIdx.z = f, blockIdx.y = c, rows by grid stride ------------------------------------------------------
__global__ __launch_bounds__(kLanes* kRows) void dihedral_rows_kernel(const float* __restrict__ in, float* __restrict__ out, uint32_t C,
                                                                      uint32_t H, uint32_t W, uint32_t hflip, uint32_t vflip) {
  const size_t plane = (size_t)blockIdx.z * C + blockIdx.y;
  const float* src = in + plane * H * W;
  float* dst = out + plane * H * W;
  const uint32_t quads = W / 4;
  for (size_t y = (size_t)blockIdx.x * kRows + threadIdx.y; y < H; y += (size_t)gridDim.x * kRows) {
    const float* srow = src + (vflip ? H - 1 - y : y) * W;
    float* drow = dst + y * W;
    const int d_align = align_of(drow);
    const uint32_t xt = 4 * quads + threadIdx.x;      // the 0 .. 3 samples past the last quad
    if (hflip) {
      const float* tail = srow + (W & 3);
      const int s_align = align_of(tail);
      for (uint32_t xv = threadIdx.x; xv < quads; xv += kLanes) store_quad(drow + 4 * xv, d_align, load_mirrored(tail, quads, xv, s_align));
      if (xt < W) drow[xt] = srow[W - 1 - xt];
    } else {
      const int s_align = align_of(srow);
      for (uint32_t xv = threadIdx.x; xv < quads; xv += kLanes) store_quad(drow + 4 * xv, d_align, load_quad(srow + 4 * xv, s_align));
      if (xt < W) drow[xt] = srow[xt];
    }
  }
}

// -- dihedral, modes 4 .. 7: blockIdx.x = the source tile (row-major over ntx columns of tiles) ------------------------------------------
// source sample (r, q) goes to out[hflip ? W-1-q : q][vflip ? H-1-r : r]; out is W x H
__global__ __launch_bounds__(kLanes* kRows) void dihedral_transpose_kernel(const float* __restrict__ in, float* __restrict__ out, uint32_t C,
                                                                           uint32_t H, uint32_t W, uint32_t ntx, uint32_t hflip,
                                                                           uint32_t vflip) {
  __shared__ float tile[kTile * kPitch];
  const size_t plane = (size_t)blockIdx.z * C + blockIdx.y;
  const float* src = in + plane * H * W;
  float* dst = out + plane * H * W;
  const uint32_t ty = blockIdx.x / ntx, tx = blockIdx.x - ty * ntx;
  const uint32_t r0 = ty * kTile, q0 = tx * kTile;
  const uint32_t rows = min((uint32_t)kTile, H - r0), cols = min((uint32_t)kTile, W - q0);
  const uint32_t l = threadIdx.x;
  if (l < cols)
    for (uint32_t rr = threadIdx.y; rr < rows; rr += kRows) tile[rr * kPitch + l] = src[(size_t)(r0 + rr) * W + q0 + l];
  __syncthreads();
  if (l < rows) {
    const size_t j = vflip ? H - 1 - (r0 + l) : r0 + l;
    for (uint32_t cc = threadIdx.y; cc < cols; cc += kRows) {
      const size_t i = hflip ? W - 1 - (q0 + cc) : q0 + cc;
      dst[i * H + j] = tile[l * kPitch + cc];
    }
  }
}

struct Blend {
  uint32_t F, C;            // frames per clip, channels (blockIdx.z = n F + f, blockIdx.y = c)
  uint32_t SH, SW;          // the accumulator's frames
  uint32_t th, tw;          // the tile, as the accumulator sees it
  uint32_t Y0, X0;          // where it goes
  uint32_t hflip, vflip;    // (the rows kernel takes hflip as its template parameter)
  uint32_t ntx;             // transposed modes: columns of source tiles
  int64_t sn, sf, sc, sy;   // the source's strides, in elements
};

// -- blend, modes 0 .. 3 ----------------------------------------------------------------------------------------------------------------
template <bool HFLIP>
__global__ __launch_bounds__(kLanes* kRows) void blend_rows_kernel(float* __restrict__ acc, const float* __restrict__ sr,
                                                                   const float* __restrict__ wy, const float* __restrict__ wx, Blend g) {
  const uint32_t n = blockIdx.z / g.F, f = blockIdx.z - n * g.F;      // once per workgroup, on the scalar unit
  const size_t plane = (size_t)blockIdx.z * g.C + blockIdx.y;
  float* dst = acc + (plane * g.SH + g.Y0) * g.SW + g.X0;
  const float* src = sr + (int64_t)n * g.sn + (int64_t)f * g.sf + (int64_t)blockIdx.y * g.sc;
  const uint32_t quads = g.tw / 4;
  const int wx_align = align_of(wx);
  for (size_t y = (size_t)blockIdx.x * kRows + threadIdx.y; y < g.th; y += (size_t)gridDim.x * kRows) {
    float* arow = dst + y * g.SW;
    const float* srow = src + (int64_t)(g.vflip ? g.th - 1 - y : y) * g.sy;
    const float* from = HFLIP ? srow + (g.tw & 3) : srow;      // where the row's quads are counted from: load_mirrored's `tail`
    const float wyv = wy[y];
    const int a_align = align_of(arow), s_align = align_of(from);
    for (uint32_t xv = threadIdx.x; xv < quads; xv += kLanes) {
      const uint32_t x = 4 * xv;
      const float4 a = load_quad(arow + x, a_align), w = load_quad(wx + x, wx_align);
      const float4 v = HFLIP ? load_mirrored(from, quads, xv, s_align) : load_quad(from + x, s_align);
      store_quad(arow + x, a_align,
                 make_float4(blend(a.x, wyv, w.x, v.x), blend(a.y, wyv, w.y, v.y), blend(a.z, wyv, w.z, v.z), blend(a.w, wyv, w.w, v.w)));
    }
    const uint32_t x = 4 * quads + threadIdx.x;      // the 0 .. 3 samples past the last quad
    if (x < g.tw) arow[x] = blend(arow[x], wyv, wx[x], srow[HFLIP ? g.tw - 1 - x : x]);
  }
}

// -- blend, modes 4 .. 7: the source is (tw, th); its sample (R, Q) goes to acc row vflip ? th-1-Q : Q, column hflip ? tw-1-R : R ------------
__global__ __launch_bounds__(kLanes* kRows) void blend_transpose_kernel(float* __restrict__ acc, const float* __restrict__ sr,
                                                                        const float* __restrict__ wy, const float* __restrict__ wx, Blend g) {
  __shared__ float tile[kTile * kPitch];
  const uint32_t n = blockIdx.z / g.F, f = blockIdx.z - n * g.F;
  const size_t plane = (size_t)blockIdx.z * g.C + blockIdx.y;
  float* dst = acc + (plane * g.SH + g.Y0) * g.SW + g.X0;
  const float* src = sr + (int64_t)n * g.sn + (int64_t)f * g.sf + (int64_t)blockIdx.y * g.sc;
  const uint32_t ty = blockIdx.x / g.ntx, tx = blockIdx.x - ty * g.ntx;
  const uint32_t r0 = ty * kTile, q0 = tx * kTile;      // source rows run over tw, source columns over th
  const uint32_t rows = min((uint32_t)kTile, g.tw - r0), cols = min((uint32_t)kTile, g.th - q0);
  const uint32_t l = threadIdx.x;
  if (l < cols)
    for (uint32_t rr = threadIdx.y; rr < rows; rr += kRows) tile[rr * kPitch + l] = src[(int64_t)(r0 + rr) * g.sy + q0 + l];
  __syncthreads();
  if (l < rows) {
    const uint32_t x = g.hflip ? g.tw - 1 - (r0 + l) : r0 + l;
    const float wxv = wx[x];
    for (uint32_t cc = threadIdx.y; cc < cols; cc += kRows) {
      const uint32_t y = g.vflip ? g.th - 1 - (q0 + cc) : q0 + cc;
      float* a = dst + (size_t)y * g.SW + x;
      *a = blend(*a, wy[y], wxv, tile[l * kPitch + cc]);
    }
  }
}

// tiles of a rows x cols source, or 0 where they do not fit grid.x
inline int64_t tile_count(int32_t rows, int32_t cols) {
  return (int64_t)eavsr::cdiv(rows, kTile) * eavsr::cdiv(cols, kTile);
}

// both blend entry points: the checks, under the caller's name, and the one launch of mode k (0 .. 7)
int blend_launch(const char* who, int32_t k, float* acc, const float* sr, const float* wy, const float* wx, int32_t N, int32_t F, int32_t C,
                 int32_t SH, int32_t SW, int32_t th, int32_t tw, int32_t Y0, int32_t X0, int64_t sn, int64_t sf, int64_t sc, int64_t sy,
                 void* stream) {
  EAVSR_REQUIRE(acc && sr && wy && wx, -1, "%s: NULL pointer", who);
  EAVSR_REQUIRE(N >= 0 && F >= 0 && C >= 1 && C <= 65535 && SH >= 1 && SW >= 1 && (int64_t)N * F <= 65535, -2,
                "%s: bad dims N=%d F=%d C=%d SH=%d SW=%d (N F and C: at most 65535)", who, N, F, C, SH, SW);
  EAVSR_REQUIRE(th >= 1 && tw >= 1 && Y0 >= 0 && X0 >= 0 && th <= SH - Y0 && tw <= SW - X0, -2,
                "%s: the tile [%d, %d + %d) x [%d, %d + %d) does not lie inside frames of %d x %d", who, Y0, Y0, th, X0, X0, tw, SH, SW);
  const int32_t row = (k & 4) ? th : tw;      // samples in a row of the source
  EAVSR_REQUIRE(sn >= 0 && sf >= 0 && sc >= 0 && sy >= row, -2, "%s: strides n=%lld f=%lld c=%lld row=%lld (in elements; rows >= %d)", who,
                (long long)sn, (long long)sf, (long long)sc, (long long)sy, row);
  EAVSR_REQUIRE(((((uintptr_t)acc) | ((uintptr_t)sr) | ((uintptr_t)wy) | ((uintptr_t)wx)) & 3) == 0, -2,
                "%s: pointers must be 4-byte aligned", who);
  EAVSR_REQUIRE(k == 0 || tile_count(tw, th) <= 2147483647LL, -2, "%s: a %d x %d tile is more LDS tiles than a grid holds", who, th, tw);
  if (N == 0 || F == 0) return 0;
  const Blend g{(uint32_t)F, (uint32_t)C, (uint32_t)SH, (uint32_t)SW, (uint32_t)th, (uint32_t)tw, (uint32_t)Y0, (uint32_t)X0,
                (uint32_t)(k & 1), (uint32_t)((k >> 1) & 1), (uint32_t)eavsr::cdiv(th, kTile), sn, sf, sc, sy};
  if (k & 4) {
    const dim3 grid((unsigned)tile_count(tw, th), C, N * F);
    hipLaunchKernelGGL(blend_transpose_kernel, grid, dim3(kLanes, kRows), 0, eavsr::as_stream(stream), acc, sr, wy, wx, g);
  } else {
    const dim3 grid(eavsr::row_blocks(th, kRows, (size_t)N * F * C), C, N * F);
    hipLaunchKernelGGL(g.hflip ? blend_rows_kernel<true> : blend_rows_kernel<false>, grid, dim3(kLanes, kRows), 0,
                       eavsr::as_stream(stream), acc, sr, wy, wx, g);
  }
  return eavsr::launch_status(who);
}

}  // namespace

extern "C" int eavsr_dihedral_f32(const float* in, float* out, int32_t F, int32_t C, int32_t H, int32_t W, int32_t k, void* stream) {
  EAVSR_REQUIRE(in && out, -1, "dihedral: NULL pointer");
  EAVSR_REQUIRE(F >= 0 && F <= 65535 && C >= 1 && C <= 65535 && H >= 1 && W >= 1, -2,
                "dihedral: bad dims F=%d C=%d H=%d W=%d (F and C: at most 65535)", F, C, H, W);
  EAVSR_REQUIRE(k >= 0 && k <= 7, -2, "dihedral: mode %d: 0 .. 7 (bit 0 hflip, bit 1 vflip, bit 2 transpose)", k);
  EAVSR_REQUIRE(((((uintptr_t)in) | ((uintptr_t)out)) & 3) == 0, -2, "dihedral: pointers must be 4-byte aligned");
  EAVSR_REQUIRE(tile_count(H, W) <= 2147483647LL, -2, "dihedral: %d x %d frames are more tiles than a grid holds", H, W);
  if (F == 0) return 0;
  const uint32_t hflip = k & 1, vflip = (k >> 1) & 1;
  if (k & 4) {
    const dim3 grid((unsigned)tile_count(H, W), C, F);
    hipLaunchKernelGGL(dihedral_transpose_kernel, grid, dim3(kLanes, kRows), 0, eavsr::as_stream(stream), in, out, (uint32_t)C, (uint32_t)H,
                       (uint32_t)W, (uint32_t)eavsr::cdiv(W, kTile), hflip, vflip);
  } else {
    const dim3 grid(eavsr::row_blocks(H, kRows, (size_t)F * C), C, F);
    hipLaunchKernelGGL(dihedral_rows_kernel, grid, dim3(kLanes, kRows), 0, eavsr::as_stream(stream), in, out, (uint32_t)C, (uint32_t)H,
                       (uint32_t)W, hflip, vflip);
  }
  return eavsr::launch_status("dihedral");
}

extern "C" int eavsr_tile_blend_f32(float* acc, const float* sr, const float* wy, const float* wx, int32_t N, int32_t F, int32_t C, int32_t SH,
                                    int32_t SW, int32_t th, int32_t tw, int32_t Y0, int32_t X0, int64_t sn, int64_t sf, int64_t sc, int64_t sy,
                                    void* stream) {
  return blend_launch("tile_blend", 0, acc, sr, wy, wx, N, F, C, SH, SW, th, tw, Y0, X0, sn, sf, sc, sy, stream);
}

extern "C" int eavsr_blend_dihedral_f32(float* acc, const float* sr, const float* wy, const float* wx, int32_t N, int32_t F, int32_t C,
                                        int32_t SH, int32_t SW, int32_t th, int32_t tw, int32_t Y0, int32_t X0, int32_t k, int64_t sn,
                                        int64_t sf, int64_t sc, int64_t sy, void* stream) {
  EAVSR_REQUIRE(k >= 0 && k <= 7, -2, "blend_dihedral: mode %d: 0 .. 7 (bit 0 hflip, bit 1 vflip, bit 2 transpose)", k);
  return blend_launch(k == 0 ? "tile_blend" : "blend_dihedral", k, acc, sr, wy, wx, N, F, C, SH, SW, th, tw, Y0, X0, sn, sf, sc, sy, stream);
}
