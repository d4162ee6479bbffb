// Antialiased bicubic resize of fp32 frames to any size: MATLAB's `imresize` as eavsr_amd/resize.py builds its tables,
// rows first, then columns.  The file is built with -ffp-contract=off (build.py PER_FILE_FLAGS): every product and every sum below is
// rounded to fp32 on its own, taps in increasing order, and a tap whose weight is zero is skipped -- never multiplied -- so numpy
// restates the result bit for bit (tests/resize_ref.py) and a non-finite sample reaches only the outputs whose non-zero taps read it.
//
// Two launches, no atomics, no per-plane loop on the host:
//   resize_v_kernel  the vertical pass streams: a lane owns four adjacent x of one output row of one plane and loops over that row's
//                    taps, whose indices and weights are wave-uniform (scalar loads).  The quads are laid out from the first
//                    16-byte boundary of the plane: a source row whose offset keeps that phase is read as float4, any other row and
//                    the head / tail quads of a row as scalars.  The intermediate row is stored shifted by the same phase, so every
//                    full quad is one aligned float4 store.
//   resize_h_kernel  the horizontal pass: a workgroup takes a piece of `cols` output columns, stages their taps once in LDS (index
//                    and weight transposed to [tap][column], indices relative to the piece's first input column) and then walks
//                    over output rows, one wave per row: the wave stages the span of the intermediate row the piece reads
//                    (at most kLdsRow floats) and each lane gathers its taps from it.
#include "common.h"

#include <limits.h>

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxTaps = 64;
constexpr int kLdsRow = 2048;        // floats of an intermediate row one wave stages: the input span of a piece of output columns
constexpr int kLdsTable = 3072;      // (index, weight) pairs a workgroup stages: columns of a piece x taps
constexpr int kMaxCols = 256;        // output columns of a piece: four per lane
constexpr int kSpanMargin = 4;       // floats kept free when the piece is sized from W / ow (the tables are rounded on the host)

// elements between the last 16-byte boundary and the plane's first sample: the phase every quad of the plane is shifted by
__device__ __forceinline__ int plane_phase(const float* plane) { return (int)(((uintptr_t)plane >> 2) & 3); }

__device__ __forceinline__ const float* plane_of(const float* src, int64_t p, int C, int64_t sN, int64_t sC) {
  return src + (p / C) * sN + (p % C) * sC;
}

__global__ __launch_bounds__(kThreads) void resize_v_kernel(const float* __restrict__ src, int64_t sN, int64_t sC, int64_t sH, int C, int H,
                                                            int W, const int32_t* __restrict__ idx, const float* __restrict__ wgt, int K,
                                                            int oh, int64_t rows, float* __restrict__ t, int Wt) {
  const int q = blockIdx.x * kThreads + threadIdx.x;
  for (int64_t r = blockIdx.y; r < rows; r += gridDim.y) {
    const int64_t p = r / oh;
    const int o = (int)(r - p * oh);
    const float* plane = plane_of(src, p, C, sN, sC);
    const int x0 = 4 * q - plane_phase(plane);      // quad 0 holds the head: the samples before the first boundary
    if (x0 >= W) continue;
    const bool full = x0 >= 0 && x0 + 3 < W;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
    for (int k = 0; k < K; ++k) {
      const float w = wgt[o * K + k];
      if (w != 0.f) {
        const int y = min(max(idx[o * K + k], 0), H - 1);
        const int64_t off = (int64_t)y * sH;
        const float* row = plane + off;
        float v0, v1, v2, v3;
        if (full && (off & 3) == 0) {
          const f32x4 v = *reinterpret_cast<const f32x4*>(row + x0);
          v0 = v[0], v1 = v[1], v2 = v[2], v3 = v[3];
        } else {
          v0 = (x0 >= 0) ? row[x0] : 0.f;      // (x0 < W holds)
          v1 = (x0 + 1 >= 0 && x0 + 1 < W) ? row[x0 + 1] : 0.f;
          v2 = (x0 + 2 >= 0 && x0 + 2 < W) ? row[x0 + 2] : 0.f;
          v3 = (x0 + 3 < W) ? row[x0 + 3] : 0.f;      // (x0 + 3 >= 0 holds: x0 >= -3)
        }
        a0 = a0 + w * v0;
        a1 = a1 + w * v1;
        a2 = a2 + w * v2;
        a3 = a3 + w * v3;
      }
    }
    float* trow = t + r * Wt + 4 * (int64_t)q;      // sample x sits at x + phase: quad q at 4 q
    if (full) {
      f32x4 v;
      v[0] = a0, v[1] = a1, v[2] = a2, v[3] = a3;
      *reinterpret_cast<f32x4*>(trow) = v;
    } else {
      if (x0 >= 0) trow[0] = a0;
      if (x0 + 1 >= 0 && x0 + 1 < W) trow[1] = a1;
      if (x0 + 2 >= 0 && x0 + 2 < W) trow[2] = a2;
      if (x0 + 3 < W) trow[3] = a3;
    }
  }
}

__global__ __launch_bounds__(kThreads) void resize_h_kernel(const float* __restrict__ t, int Wt, int W, const float* __restrict__ src,
                                                            int64_t sN, int64_t sC, int C, int oh, const int32_t* __restrict__ idx,
                                                            const float* __restrict__ wgt, int K, int ow, int cols, int64_t rows,
                                                            float* __restrict__ out) {
  extern __shared__ __align__(16) float lds[];
  int* tab_i = reinterpret_cast<int*>(lds);             // [K][cols]
  float* tab_w = lds + K * cols;                        // [K][cols]
  float* stage = lds + 2 * K * cols;                    // [kWaves][kLdsRow]
  int* red = reinterpret_cast<int*>(stage + kWaves * kLdsRow);      // [2][kWaves]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int p0 = blockIdx.x * cols;
  const int nc = min(cols, ow - p0);
  int lo = INT_MAX, hi = 0;
  for (int e = tid; e < K * nc; e += kThreads) {
    const int j = e / K, k = e - j * K;
    const int i = min(max(idx[(int64_t)p0 * K + e], 0), W - 1);
    tab_i[k * cols + j] = i;
    tab_w[k * cols + j] = wgt[(int64_t)p0 * K + e];
    lo = min(lo, i);
    hi = max(hi, i);
  }
  for (int off = 32; off > 0; off >>= 1) {
    lo = min(lo, __shfl_xor(lo, off));
    hi = max(hi, __shfl_xor(hi, off));
  }
  if (lane == 0) red[wave] = lo, red[kWaves + wave] = hi;
  __syncthreads();
  lo = min(min(red[0], red[1]), min(red[2], red[3]));
  hi = max(max(red[kWaves], red[kWaves + 1]), max(red[kWaves + 2], red[kWaves + 3]));
  const int span = min(hi - lo + 1, kLdsRow);      // (the entry point sizes `cols` so that the span fits: never cut)
  for (int e = tid; e < K * nc; e += kThreads) {
    const int j = e / K, k = e - j * K;
    tab_i[k * cols + j] = min(tab_i[k * cols + j] - lo, kLdsRow - 1);
  }
  __syncthreads();
  float* st = stage + wave * kLdsRow;
  for (int64_t base = (int64_t)blockIdx.y * kWaves; base < rows; base += (int64_t)gridDim.y * kWaves) {
    const int64_t r = base + wave;
    const bool valid = r < rows;
    if (valid) {
      const float* trow = t + r * Wt + plane_phase(plane_of(src, r / oh, C, sN, sC)) + lo;
      for (int i = lane; i < span; i += 64) st[i] = trow[i];
    }
    __syncthreads();
    if (valid) {
      float* orow = out + r * ow + p0;
      for (int j = lane; j < nc; j += 64) {
        float a = 0.f;
        for (int k = 0; k < K; ++k) {
          const float w = tab_w[k * cols + j];
          if (w != 0.f) a = a + w * st[tab_i[k * cols + j]];
        }
        orow[j] = a;
      }
    }
    __syncthreads();
  }
}

}  // namespace

extern "C" int eavsr_resize_aa_f32(const float* src, int64_t stride_n, int64_t stride_c, int64_t stride_h, int32_t N, int32_t C, int32_t H,
                                   int32_t W, const int32_t* row_idx, const float* row_w, int32_t row_taps, const int32_t* col_idx,
                                   const float* col_w, int32_t col_taps, float* tmp, float* out, int32_t oh, int32_t ow, void* stream) {
  EAVSR_REQUIRE(src && row_idx && row_w && col_idx && col_w && tmp && out, -1, "resize_aa: NULL pointer");
  EAVSR_REQUIRE(N >= 1 && C >= 1 && H >= 1 && W >= 1 && oh >= 1 && ow >= 1, -2, "resize_aa: %d x %d planes of %d x %d -> %d x %d", N, C, H, W,
                oh, ow);
  EAVSR_REQUIRE(H <= (1 << 24) && W <= (1 << 24) && oh <= (1 << 24) && ow <= (1 << 24), -2, "resize_aa: a side above 2^24 (%d x %d -> %d x %d)", H,
                W, oh, ow);
  EAVSR_REQUIRE(row_taps >= 1 && row_taps <= kMaxTaps && col_taps >= 1 && col_taps <= kMaxTaps, -2, "resize_aa: %d / %d taps outside 1..%d",
                row_taps, col_taps, kMaxTaps);
  EAVSR_REQUIRE(stride_n >= 0 && stride_c >= 0 && stride_h >= 0, -2, "resize_aa: negative stride");
  EAVSR_REQUIRE((((uintptr_t)src | (uintptr_t)out | (uintptr_t)row_w | (uintptr_t)col_w | (uintptr_t)row_idx | (uintptr_t)col_idx) & 3) == 0 &&
                    ((uintptr_t)tmp & 15) == 0,
                -2, "resize_aa: pointers must be 4-byte aligned, tmp 16-byte aligned");
  const int64_t rows = (int64_t)N * C * oh;
  const int Wt = (W + 6) & ~3;      // a row of tmp: W samples behind a phase of at most 3, in whole quads
  // a piece of `cols` output columns: its taps fit the table, and the input span it reads -- at most (cols - 1) W / ow + taps + 1
  // samples: consecutive outputs sit W / ow apart, reflection only folds the range -- fits the staged row
  int cols = min(kMaxCols, kLdsTable / col_taps);
  const int64_t room = kLdsRow - kSpanMargin - col_taps - 1;
  const int64_t by_span = room * ow / W + 1;
  if (by_span < cols) cols = (int)by_span;
  EAVSR_REQUIRE(cols >= 1, -2, "resize_aa: %d taps along a row of %d -> %d samples leave no room for a piece", col_taps, W, ow);
  const int quads = (W + 3 + 3) / 4;      // with the largest phase
  const dim3 gv(eavsr::cdiv(quads, kThreads), (unsigned)(rows < 65535 ? rows : 65535));
  hipLaunchKernelGGL(resize_v_kernel, gv, dim3(kThreads), 0, eavsr::as_stream(stream), src, stride_n, stride_c, stride_h, (int)C, (int)H, (int)W,
                     row_idx, row_w, (int)row_taps, (int)oh, rows, tmp, Wt);
  if (int rc = eavsr::launch_status("resize_aa (rows)")) return rc;
  const int pieces = eavsr::cdiv(ow, cols);
  const int64_t groups = (rows + kWaves - 1) / kWaves;
  int64_t gy = 4096 / pieces;
  gy = gy < 1 ? 1 : gy;
  gy = gy < groups ? gy : groups;
  gy = gy < 65535 ? gy : 65535;
  const size_t lds = ((size_t)2 * col_taps * cols + (size_t)kWaves * kLdsRow + 2 * kWaves) * 4;
  hipLaunchKernelGGL(resize_h_kernel, dim3(pieces, (unsigned)gy), dim3(kThreads), lds, eavsr::as_stream(stream), tmp, Wt, (int)W, src, stride_n,
                     stride_c, (int)C, (int)oh, col_idx, col_w, (int)col_taps, (int)ow, cols, rows, out);
  return eavsr::launch_status("resize_aa (columns)");
}
