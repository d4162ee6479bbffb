// NIQE, the report's no-reference column (Mittal et al., SPL 2013): the two device passes of the metric, in float64.
//
// niqe_moments: one workgroup per p x p block of the cropped luma plane.  For the plane I (cropped to whole blocks; the 7-tap window
// g of DESIGN 7m, applied separably, along W first, taps in ascending order, every product and sum rounded on its own):
//   mu = correlate(I, g), edge replicated at the CROPPED plane's border;  sigma = sqrt(|correlate(I I, g) - mu mu|)
//   M = (I - mu) / (sigma + 1)
//   the five maps v0 = M, v1 = M roll(M, (0, 1)), v2 = M roll(M, (1, 0)), v3 = M roll(M, (1, 1)), v4 = M roll(M, (1, -1)), the roll
//   circular inside the block; per map (n_neg, n_pos, sum of v^2 over v < 0, sum of v^2 over v > 0, sum of |v|): 25 numbers a block
// This file is built WITHOUT floating-point contraction (eavsr_amd/build.py PER_FILE_FLAGS): numpy restates mu, sigma and M bit for
// bit (tests/niqe_ref.py), so the counts -- the signs of M and of its products -- are equal, not close.
//
// LDS of a workgroup: the block with its 3-sample halo (fp32 where the source is the 8-bit frame: luma is an integer; fp64 for an
// fp64 plane), M (p x p fp64), and the horizontal pass of ONE strip of 16 output rows (22 rows of two fp64 sums): the whole
// block's horizontal pass would not fit beside the block and M (96 x 96: 41.6 + 73.7 + 33.8 KB of 160).  An fp64 plane with p = 96
// does not fit (83.2 KB of block): p <= 80 there; the metric reads its fp64 plane in blocks of 48.
// Threads walk a row's samples in order, so every LDS access of a wavefront is a run of consecutive 4- or 8-byte words: no bank
// conflict beyond the row change inside a wavefront.  The sums: a lane adds its samples in index order, the wavefront by a fixed
// butterfly, thread k < 25 the four wavefronts in order.  No atomics: two calls agree bit for bit.
//
// niqe_half: the antialiased resize of the fp64 plane from host-built (index, weight) tables (eavsr_amd/niqe.py resize_tables),
// rows (along H) first, then columns, each one fp64 accumulation in tap order: a workgroup computes the row pass of 8 output rows
// over the columns its 32 output columns read into LDS, then the column pass from LDS.
#include "pixel.h"

#include <math.h>

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kHalo = 3, kTaps = 7;
constexpr int kStrip = 16;                 // output rows per strip of the separable window
constexpr int kMaps = 5, kPerMap = 5;      // 25 numbers per block
constexpr int kMaxLds = 160 * 1024;
constexpr int kHY = 8, kHX = 32;           // niqe_half: output samples per workgroup

struct Window {
  double g[kTaps];
};

// BT.601 studio-range luma of an 8-bit pixel in integers: 16 + round_half_even((65481 R + 128553 G + 24966 B) / 255000)
__device__ __forceinline__ int luma601(int r, int g, int b) {
  const int n = 65481 * r + 128553 * g + 24966 * b;      // <= 55 845 000
  int q = n / 255000;
  const int rem2 = 2 * (n - q * 255000);
  if (rem2 > 255000 || (rem2 == 255000 && (q & 1))) ++q;
  return 16 + q;
}

__device__ __forceinline__ float load_sample(const float* frame, size_t at, size_t hw, int C, float scale) {
  if (C == 1) return quantise(frame[at], scale);
  return (float)luma601((int)quantise(frame[at], scale), (int)quantise(frame[hw + at], scale), (int)quantise(frame[2 * hw + at], scale));
}

__device__ __forceinline__ double load_sample(const double* frame, size_t at, size_t, int, float) { return frame[at]; }

template <typename Src, typename Tile>
__global__ __launch_bounds__(kThreads) void niqe_moments_kernel(const Src* __restrict__ src, float scale, int C, int H, int W, int y0, int x0,
                                                                int p, Window win, double* __restrict__ luma_out, double* __restrict__ out) {
  extern __shared__ __align__(16) unsigned char niqe_lds[];
  const int tp = p + 2 * kHalo;
  double* M = reinterpret_cast<double*>(niqe_lds);      // [p][p]
  double* h1 = M + p * p;                               // [kStrip + 6][p]: the window along W of I
  double* h2 = h1 + (kStrip + 2 * kHalo) * p;           // ... and of I I
  double* red = h2 + (kStrip + 2 * kHalo) * p;          // [kWaves][25]
  Tile* tile = reinterpret_cast<Tile*>(red + kWaves * kMaps * kPerMap);      // [tp][tp]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int bx = blockIdx.x, by = blockIdx.y, n = blockIdx.z;
  const int ch = gridDim.y * p, cw = gridDim.x * p;      // the cropped plane
  const size_t hw = (size_t)H * W;
  const Src* frame = src + (size_t)n * C * hw;

  // the block and its halo, replicated at the cropped plane's border; the block's own samples also go out as the fp64 luma plane
  for (int i = tid; i < tp * tp; i += kThreads) {
    const int ty = i / tp, tx = i - ty * tp;
    const int cy = by * p + ty - kHalo, cx = bx * p + tx - kHalo;
    const int gy = min(max(cy, 0), ch - 1), gx = min(max(cx, 0), cw - 1);
    const Tile v = load_sample(frame, (size_t)(y0 + gy) * W + (x0 + gx), hw, C, scale);
    tile[i] = v;
    if (luma_out && ty >= kHalo && ty < kHalo + p && tx >= kHalo && tx < kHalo + p) luma_out[((size_t)n * ch + cy) * cw + cx] = (double)v;
  }
  __syncthreads();

  for (int s0 = 0; s0 < p; s0 += kStrip) {
    const int rows = min(kStrip, p - s0);
    for (int i = tid; i < (rows + 2 * kHalo) * p; i += kThreads) {      // along W: tile rows s0 .. s0 + rows + 6
      const int r = i / p, x = i - r * p;
      const Tile* row = tile + (s0 + r) * tp + x;
      double a = 0.0, b = 0.0;
#pragma unroll
      for (int k = 0; k < kTaps; ++k) {
        const double v = (double)row[k];
        a += win.g[k] * v;
        b += win.g[k] * (v * v);
      }
      h1[i] = a;
      h2[i] = b;
    }
    __syncthreads();
    for (int i = tid; i < rows * p; i += kThreads) {      // along H, then M
      const int r = i / p, x = i - r * p;
      double mu = 0.0, e2 = 0.0;
#pragma unroll
      for (int k = 0; k < kTaps; ++k) {
        mu += win.g[k] * h1[(r + k) * p + x];
        e2 += win.g[k] * h2[(r + k) * p + x];
      }
      const double sigma = sqrt(fabs(e2 - mu * mu));
      const double v = (double)tile[(s0 + r + kHalo) * tp + x + kHalo];
      M[(s0 + r) * p + x] = (v - mu) / (sigma + 1.0);
    }
    __syncthreads();
  }

  double s_neg[kMaps], s_pos[kMaps], s_abs[kMaps];
  int n_neg[kMaps], n_pos[kMaps];
#pragma unroll
  for (int j = 0; j < kMaps; ++j) {
    s_neg[j] = s_pos[j] = s_abs[j] = 0.0;
    n_neg[j] = n_pos[j] = 0;
  }
  for (int i = tid; i < p * p; i += kThreads) {
    const int y = i / p, x = i - y * p;
    const int ym = y ? y - 1 : p - 1, xm = x ? x - 1 : p - 1, xp = x + 1 < p ? x + 1 : 0;      // np.roll: circular inside the block
    const double m = M[i];
    const double v[kMaps] = {m, m * M[y * p + xm], m * M[ym * p + x], m * M[ym * p + xm], m * M[ym * p + xp]};
#pragma unroll
    for (int j = 0; j < kMaps; ++j) {
      const double q = v[j] * v[j];
      if (v[j] < 0.0) {
        n_neg[j] += 1;
        s_neg[j] += q;
      } else if (v[j] > 0.0) {
        n_pos[j] += 1;
        s_pos[j] += q;
      }
      s_abs[j] += fabs(v[j]);
    }
  }
#pragma unroll
  for (int j = 0; j < kMaps; ++j) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      s_neg[j] += __shfl_xor(s_neg[j], off);
      s_pos[j] += __shfl_xor(s_pos[j], off);
      s_abs[j] += __shfl_xor(s_abs[j], off);
      n_neg[j] += __shfl_xor(n_neg[j], off);
      n_pos[j] += __shfl_xor(n_pos[j], off);
    }
    if (lane == 0) {
      double* r = red + (wave * kMaps + j) * kPerMap;
      r[0] = (double)n_neg[j];
      r[1] = (double)n_pos[j];
      r[2] = s_neg[j];
      r[3] = s_pos[j];
      r[4] = s_abs[j];
    }
  }
  __syncthreads();
  if (tid < kMaps * kPerMap) {
    constexpr int kRec = kMaps * kPerMap;
    out[(((size_t)n * gridDim.y + by) * gridDim.x + bx) * kRec + tid] = ((red[tid] + red[kRec + tid]) + red[2 * kRec + tid]) + red[3 * kRec + tid];
  }
}

__global__ __launch_bounds__(kThreads) void niqe_half_kernel(const double* __restrict__ in, int H, int W, const int32_t* __restrict__ row_idx,
                                                             const double* __restrict__ row_w, int Kr, const int32_t* __restrict__ col_idx,
                                                             const double* __restrict__ col_w, int Kc, const int32_t* __restrict__ col_lo,
                                                             int span, int h, int w, double* __restrict__ out) {
  extern __shared__ __align__(16) double half_rows[];      // [kHY][span]: the row pass over the columns this tile reads
  const int tid = threadIdx.x;
  const int ox0 = blockIdx.x * kHX, oy0 = blockIdx.y * kHY;
  const double* plane = in + (size_t)blockIdx.z * H * W;
  const int lo = min(max(col_lo[blockIdx.x], 0), W - 1);
  for (int i = tid; i < kHY * span; i += kThreads) {
    const int r = i / span, j = i - r * span;
    const int oy = oy0 + r, c = min(lo + j, W - 1);
    double a = 0.0;
    if (oy < h) {
      for (int k = 0; k < Kr; ++k) {
        const int y = min(max(row_idx[oy * Kr + k], 0), H - 1);
        a += row_w[oy * Kr + k] * plane[(size_t)y * W + c];
      }
    }
    half_rows[i] = a;
  }
  __syncthreads();
  for (int i = tid; i < kHY * kHX; i += kThreads) {
    const int r = i / kHX, oy = oy0 + r, ox = ox0 + (i - r * kHX);
    if (oy >= h || ox >= w) continue;
    double a = 0.0;
    for (int k = 0; k < Kc; ++k) {
      const int j = min(max(col_idx[ox * Kc + k] - lo, 0), span - 1);
      a += col_w[ox * Kc + k] * half_rows[r * span + j];
    }
    out[((size_t)blockIdx.z * h + oy) * w + ox] = a;
  }
}

size_t moments_lds(int p, size_t sample) {
  return ((size_t)p * p + 2 * (size_t)(kStrip + 2 * kHalo) * p + kWaves * kMaps * kPerMap) * 8 + (size_t)(p + 2 * kHalo) * (p + 2 * kHalo) * sample;
}

}  // namespace

extern "C" int eavsr_niqe_moments(const void* src, int32_t src_f64, float scale, int32_t N, int32_t C, int32_t H, int32_t W, int32_t y0,
                                  int32_t x0, int32_t block, int32_t blocks_h, int32_t blocks_w, const double* window, double* luma_out,
                                  double* moments, void* stream) {
  EAVSR_REQUIRE(src && window && moments, -1, "niqe_moments: NULL pointer");
  EAVSR_REQUIRE(N >= 1 && N <= 65535 && H >= 1 && W >= 1, -2, "niqe_moments: N=%d frames of %d x %d (N 1..65535)", N, H, W);
  EAVSR_REQUIRE(src_f64 ? C == 1 : (C == 1 || C == 3), -2, "niqe_moments: C=%d planes (fp32 frames: 1 or 3; an fp64 plane: 1)", C);
  EAVSR_REQUIRE(block >= 8 && block <= 96, -2, "niqe_moments: block %d outside 8..96", block);
  EAVSR_REQUIRE(blocks_h >= 1 && blocks_w >= 1 && blocks_h <= 65535, -2, "niqe_moments: %d x %d blocks", blocks_h, blocks_w);
  EAVSR_REQUIRE(y0 >= 0 && x0 >= 0 && (int64_t)y0 + (int64_t)blocks_h * block <= H && (int64_t)x0 + (int64_t)blocks_w * block <= W, -2,
                "niqe_moments: %d x %d blocks of %d from (%d, %d) leave the %d x %d frame", blocks_h, blocks_w, block, y0, x0, H, W);
  EAVSR_REQUIRE((((uintptr_t)src | (uintptr_t)luma_out | (uintptr_t)moments) & 7) == 0, -2, "niqe_moments: pointers must be 8-byte aligned");
  const size_t lds = moments_lds(block, src_f64 ? 8 : 4);
  EAVSR_REQUIRE(lds <= (size_t)kMaxLds, -2, "niqe_moments: block %d of an fp%d source needs %zu bytes of LDS, at most %d (fp64 plane: block <= 80)",
                block, src_f64 ? 64 : 32, lds, kMaxLds);
  Window win;
  for (int k = 0; k < kTaps; ++k) win.g[k] = window[k];
  const dim3 grid(blocks_w, blocks_h, N);
  if (src_f64) {
    if (int rc = eavsr::raise_lds<&niqe_moments_kernel<double, double>>(kMaxLds, "niqe_moments")) return rc;
    hipLaunchKernelGGL((niqe_moments_kernel<double, double>), grid, dim3(kThreads), lds, eavsr::as_stream(stream), (const double*)src, scale,
                       C, H, W, y0, x0, block, win, luma_out, moments);
  } else {
    if (int rc = eavsr::raise_lds<&niqe_moments_kernel<float, float>>(kMaxLds, "niqe_moments")) return rc;
    hipLaunchKernelGGL((niqe_moments_kernel<float, float>), grid, dim3(kThreads), lds, eavsr::as_stream(stream), (const float*)src, scale, C,
                       H, W, y0, x0, block, win, luma_out, moments);
  }
  return eavsr::launch_status("niqe_moments");
}

extern "C" int eavsr_niqe_half_f64(const double* in, double* out, const int32_t* row_idx, const double* row_w, int32_t row_taps,
                                   const int32_t* col_idx, const double* col_w, int32_t col_taps, const int32_t* col_lo, int32_t span,
                                   int32_t N, int32_t H, int32_t W, int32_t h, int32_t w, void* stream) {
  EAVSR_REQUIRE(in && out && row_idx && row_w && col_idx && col_w && col_lo, -1, "niqe_half: NULL pointer");
  EAVSR_REQUIRE(N >= 1 && N <= 65535 && H >= 1 && W >= 1 && h >= 1 && w >= 1, -2, "niqe_half: N=%d planes %d x %d -> %d x %d", N, H, W, h, w);
  EAVSR_REQUIRE(row_taps >= 1 && row_taps <= 64 && col_taps >= 1 && col_taps <= 64, -2, "niqe_half: %d / %d taps outside 1..64", row_taps,
                col_taps);
  EAVSR_REQUIRE(span >= 1 && (size_t)span * kHY * 8 <= (size_t)kMaxLds, -2, "niqe_half: a tile of %d output columns reads %d columns, at most %d",
                kHX, span, kMaxLds / (kHY * 8));
  EAVSR_REQUIRE(eavsr::cdiv(h, kHY) <= 65535, -2, "niqe_half: %d output rows, at most %d", h, 65535 * kHY);
  EAVSR_REQUIRE((((uintptr_t)in | (uintptr_t)out | (uintptr_t)row_w | (uintptr_t)col_w) & 7) == 0, -2, "niqe_half: fp64 pointers must be 8-byte aligned");
  if (int rc = eavsr::raise_lds<&niqe_half_kernel>(kMaxLds, "niqe_half")) return rc;
  const dim3 grid(eavsr::cdiv(w, kHX), eavsr::cdiv(h, kHY), N);
  hipLaunchKernelGGL(niqe_half_kernel, grid, dim3(kThreads), (size_t)span * kHY * 8, eavsr::as_stream(stream), in, H, W, row_idx, row_w,
                     (int)row_taps, col_idx, col_w, (int)col_taps, col_lo, (int)span, h, w, out);
  return eavsr::launch_status("niqe_half");
}
