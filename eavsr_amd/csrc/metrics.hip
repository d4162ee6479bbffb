// Per-frame PSNR / SSIM of the evaluation report (psnr_total.py:39-44, :88-143) in one fused pass, and the 8-bit interleaved frame
// that goes into the PNG (test_basic.py:85-92).
//
// Both images are quantised in registers, q = rint(clamp(v * scale, 0, 255)) (round half to even: `torch.clamp(v * 255, 0,
// 255).round()` of get_current_visuals); no quantised float copy goes to memory.  Per frame the pass produces
//   sse      = sum (q_sr - q_hr)^2 over the whole frame, an exact integer (64-bit), and
//   ssim_sum = sum of the SSIM map over the C (H - 10)(W - 10) valid positions: skimage's structural_similarity(win_size=11,
//              data_range=255, gaussian_weights=True) -- an 11-tap gaussian (sigma 1.5, normalised), applied separably to the five
//              moments x, y, x^2, y^2, xy, sample covariance (121 / 120), C1 = (0.01 * 255)^2, C2 = (0.03 * 255)^2.
// The moments and the map are fp64: filt(x^2) - filt(x)^2 cancels at magnitude 65 025, and in fp32 that costs the 4th decimal the
// report prints.  With fp64 moments the summation order is immaterial (<= 1e-12 on the map's mean).
//
// A 256-thread workgroup owns a 64 x 32 tile of valid outputs of one frame and walks the frame's C planes.  Per plane it stages the
// tile plus the 10-sample apron (74 x 42 quantised samples of both images) in LDS once, then per moment runs the horizontal pass
// into an fp64 LDS plane (42 x 64) and the vertical pass into registers (8 outputs per lane); the SSIM map of the lane's outputs is
// summed in the lane, then over the wavefront (wave-64 shuffles) and the four wavefronts.  The squared error and the 8-bit frame
// come from the staged samples the tile OWNS (the 64 x 32 samples at its origin; the last tile of a row / column also owns the
// apron), so every sample is counted and written once.  ONE (ssim, sse) pair per workgroup is written with ordinary stores; a second
// kernel sums a frame's pairs in a fixed order.  No atomics: two calls on the same input are bitwise equal.
#include "pixel.h"

#include <math.h>

namespace {

constexpr int kWin = 11;                  // window taps
constexpr int kApron = kWin - 1;          // 10
constexpr int kTW = 64, kTH = 32;         // valid outputs per tile
constexpr int kSW = kTW + kApron;         // 74 staged columns
constexpr int kSH = kTH + kApron;         // 42 staged rows
constexpr int kThreads = 256;
constexpr int kRowsPerLane = kTH / (kThreads / kTW);      // 8 output rows per lane in the vertical pass

struct Taps {
  double g[kWin];
};

struct Partial {      // one per workgroup; 16 bytes
  double ssim;
  int64_t sse;
};

// value of moment M (x, y, x^2, y^2, xy) at one sample; the quantised samples are integers <= 255: exact
template <int M>
__device__ __forceinline__ double moment_of(float x, float y) {
  return M == 0 ? (double)x : M == 1 ? (double)y : M == 2 ? (double)(x * x) : M == 3 ? (double)(y * y) : (double)(x * y);
}

// horizontal pass of moment M over the 42 staged rows into hbuf, then the vertical pass into acc[0..7] (rows rb * 8 + k of column col)
template <int M>
__device__ __forceinline__ void moment_pass(const float (*xs)[kSW], const float (*ys)[kSW], double (*hbuf)[kTW], const Taps& taps,
                                            int col, int rb, double* acc) {
  __syncthreads();      // the previous moment's vertical pass has read hbuf (and, for M == 0, the staging has written xs / ys)
  for (int r = rb; r < kSH; r += kThreads / kTW) {
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < kWin; ++k) s = fma(taps.g[k], moment_of<M>(xs[r][col + k], ys[r][col + k]), s);
    hbuf[r][col] = s;
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < kRowsPerLane; ++k) acc[k] = 0.0;
#pragma unroll
  for (int r = 0; r < kRowsPerLane + kApron; ++r) {
    const double v = hbuf[rb * kRowsPerLane + r][col];
#pragma unroll
    for (int k = 0; k < kRowsPerLane; ++k)
      if (r - k >= 0 && r - k < kWin) acc[k] = fma(taps.g[r - k], v, acc[k]);
  }
}

__global__ __launch_bounds__(kThreads) void frame_metrics_kernel(const float* __restrict__ sr, const float* __restrict__ hr, float scale,
                                                                 int C, int H, int W, Taps taps, Partial* __restrict__ partials,
                                                                 uint8_t* __restrict__ rgb8) {
  __shared__ float xs[kSH][kSW], ys[kSH][kSW];
  __shared__ double hbuf[kSH][kTW];
  __shared__ uint8_t q8[kSH * kSW * 3];
  __shared__ double red_ssim[kThreads / 64];
  __shared__ unsigned long long red_sse[kThreads / 64];

  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int tx = blockIdx.x, ty = blockIdx.y, f = blockIdx.z;
  const int x0 = tx * kTW, y0 = ty * kTH;
  // samples this tile owns (for the squared error and the 8-bit frame): its 64 x 32 origin block; the last tile of a row / column
  // owns what is left, which its staged region covers: W - x0 <= 64 + 10
  const int own_w = tx == (int)gridDim.x - 1 ? W - x0 : kTW;
  const int own_h = ty == (int)gridDim.y - 1 ? H - y0 : kTH;
  const int col = t & (kTW - 1), rb = t / kTW;
  const int vw = W - kApron, vh = H - kApron;      // valid outputs of the frame

  unsigned int sse = 0;      // <= 13 staged samples per lane and plane, <= 39 over 3 planes: 39 * 65025 < 2^32
  double ssim = 0.0;
  for (int c = 0; c < C; ++c) {
    const size_t plane = ((size_t)f * C + c) * (size_t)H * W;
    // (no barrier: the previous plane's last read of xs / ys is before the barrier inside its fifth moment pass)
    for (int i = t; i < kSH * kSW; i += kThreads) {
      const int r = i / kSW, cc = i - r * kSW;
      const int gy = y0 + r, gx = x0 + cc;
      float qx = 0.f, qy = 0.f;
      if (gy < H && gx < W) {
        const size_t at = plane + (size_t)gy * W + gx;
        qx = quantise(sr[at], scale);
        qy = quantise(hr[at], scale);
      }
      xs[r][cc] = qx;
      ys[r][cc] = qy;
      if (r < own_h && cc < own_w) {
        const int d = (int)qx - (int)qy;
        sse += (unsigned int)(d * d);
        if (rgb8) q8[i * C + c] = (uint8_t)(int)qx;
      }
    }
    double m[5][kRowsPerLane];
    moment_pass<0>(xs, ys, hbuf, taps, col, rb, m[0]);
    moment_pass<1>(xs, ys, hbuf, taps, col, rb, m[1]);
    moment_pass<2>(xs, ys, hbuf, taps, col, rb, m[2]);
    moment_pass<3>(xs, ys, hbuf, taps, col, rb, m[3]);
    moment_pass<4>(xs, ys, hbuf, taps, col, rb, m[4]);
    const double cov_norm = 121.0 / 120.0, c1 = (0.01 * 255.0) * (0.01 * 255.0), c2 = (0.03 * 255.0) * (0.03 * 255.0);
#pragma unroll
    for (int k = 0; k < kRowsPerLane; ++k) {
      const double ux = m[0][k], uy = m[1][k];
      const double vx = cov_norm * (m[2][k] - ux * ux), vy = cov_norm * (m[3][k] - uy * uy), vxy = cov_norm * (m[4][k] - ux * uy);
      const double s = ((2.0 * ux * uy + c1) * (2.0 * vxy + c2)) / ((ux * ux + uy * uy + c1) * (vx + vy + c2));
      if (x0 + col < vw && y0 + rb * kRowsPerLane + k < vh) ssim += s;
    }
  }

  // wavefront, then workgroup
  unsigned long long sse64 = sse;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    ssim += __shfl_xor(ssim, off);
    sse64 += __shfl_xor(sse64, off);
  }
  if (lane == 0) {
    red_ssim[wave] = ssim;
    red_sse[wave] = sse64;
  }
  __syncthreads();      // also: every plane's q8 bytes are in place
  if (t == 0) {
    Partial p;
    p.ssim = ((red_ssim[0] + red_ssim[1]) + red_ssim[2]) + red_ssim[3];
    p.sse = (int64_t)(red_sse[0] + red_sse[1] + red_sse[2] + red_sse[3]);
    partials[((size_t)f * gridDim.y + ty) * gridDim.x + tx] = p;
  }
  if (rgb8) {
    // the owned block as HWC bytes: own_w * C consecutive bytes per row
    const int nb = own_w * C;
    uint8_t* out = rgb8 + ((size_t)f * H + y0) * (size_t)W * C + (size_t)x0 * C;
    for (int r = wave; r < own_h; r += kThreads / 64)
      for (int b = lane; b < nb; b += 64) out[(size_t)r * W * C + b] = q8[r * kSW * C + b];
  }
}

// a frame's partial pairs summed in a fixed order: lane t takes partials t, t + 256, ... in turn, then a fixed tree over the lanes
__global__ __launch_bounds__(kThreads) void frame_metrics_sum_kernel(const Partial* __restrict__ partials, int count,
                                                                     long long* __restrict__ sse_out, double* __restrict__ ssim_out) {
  __shared__ double s_ssim[kThreads];
  __shared__ long long s_sse[kThreads];
  const int t = threadIdx.x, f = blockIdx.x;
  const Partial* p = partials + (size_t)f * count;
  double a = 0.0;
  long long e = 0;
  for (int i = t; i < count; i += kThreads) {
    a += p[i].ssim;
    e += p[i].sse;
  }
  s_ssim[t] = a;
  s_sse[t] = e;
  __syncthreads();
  for (int half = kThreads / 2; half > 0; half >>= 1) {
    if (t < half) {
      s_ssim[t] += s_ssim[t + half];
      s_sse[t] += s_sse[t + half];
    }
    __syncthreads();
  }
  if (t == 0) {
    ssim_out[f] = s_ssim[0];
    sse_out[f] = s_sse[0];
  }
}

// the quantise + interleave alone: one lane per pixel, C coalesced plane reads, C bytes out
__global__ __launch_bounds__(kThreads) void rgb8_kernel(const float* __restrict__ sr, float scale, int C, size_t hw,
                                                        uint8_t* __restrict__ rgb8) {
  const size_t f = blockIdx.y;
  for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i < hw; i += (size_t)gridDim.x * kThreads)
    for (int c = 0; c < C; ++c) rgb8[(f * hw + i) * C + c] = (uint8_t)(int)quantise(sr[(f * C + c) * hw + i], scale);
}

Taps gaussian_taps() {
  Taps t;
  double sum = 0.0;
  for (int i = 0; i < kWin; ++i) {
    const double d = (double)(i - kWin / 2) / 1.5;
    t.g[i] = exp(-0.5 * d * d);
    sum += t.g[i];
  }
  for (int i = 0; i < kWin; ++i) t.g[i] /= sum;
  return t;
}

bool shape_ok(const char* what, int32_t F, int32_t C, int32_t H, int32_t W, bool window) {
  if (F < 0 || F > 65535) {
    eavsr::set_error("%s: F=%d frames outside 0..65535", what, F);
    return false;
  }
  if (C != 1 && C != 3) {
    eavsr::set_error("%s: C=%d planes, must be 1 or 3", what, C);
    return false;
  }
  if (window ? (H < kWin || W < kWin) : (H < 1 || W < 1)) {
    eavsr::set_error("%s: frame %d x %d smaller than the %d-tap window", what, H, W, window ? kWin : 1);
    return false;
  }
  if (eavsr::cdiv(H, kTH) > 65535) {
    eavsr::set_error("%s: H=%d too large", what, H);
    return false;
  }
  return true;
}

}  // namespace

extern "C" int32_t eavsr_frame_metrics_partials(int32_t F, int32_t C, int32_t H, int32_t W) {
  if (!shape_ok("frame_metrics_partials", F, C, H, W, true)) return -2;
  return eavsr::cdiv(W - kApron, kTW) * eavsr::cdiv(H - kApron, kTH);
}

extern "C" int eavsr_frame_metrics_f32(const float* sr, const float* hr, float scale, int32_t F, int32_t C, int32_t H, int32_t W,
                                       void* workspace, int64_t* sse_out, double* ssim_sum_out, uint8_t* rgb8, void* stream) {
  EAVSR_REQUIRE(sr && hr && workspace && sse_out && ssim_sum_out, -1, "frame_metrics: NULL pointer");
  if (!shape_ok("frame_metrics", F, C, H, W, true)) return -2;
  if (F == 0) return 0;
  static_assert(sizeof(Partial) == 16, "the workspace is 16 bytes per partial");
  const dim3 grid(eavsr::cdiv(W - kApron, kTW), eavsr::cdiv(H - kApron, kTH), F);
  hipLaunchKernelGGL(frame_metrics_kernel, grid, dim3(kThreads), 0, eavsr::as_stream(stream), sr, hr, scale, C, H, W, gaussian_taps(),
                     (Partial*)workspace, rgb8);
  int rc = eavsr::launch_status("frame_metrics");
  if (rc) return rc;
  hipLaunchKernelGGL(frame_metrics_sum_kernel, dim3(F), dim3(kThreads), 0, eavsr::as_stream(stream), (const Partial*)workspace,
                     (int)(grid.x * grid.y), (long long*)sse_out, ssim_sum_out);
  return eavsr::launch_status("frame_metrics_sum");
}

extern "C" int eavsr_rgb8_f32(const float* sr, float scale, int32_t F, int32_t C, int32_t H, int32_t W, uint8_t* rgb8, void* stream) {
  EAVSR_REQUIRE(sr && rgb8, -1, "rgb8: NULL pointer");
  if (!shape_ok("rgb8", F, C, H, W, false)) return -2;
  if (F == 0) return 0;
  const size_t hw = (size_t)H * W;
  size_t bx = (hw + kThreads - 1) / kThreads;
  if (bx > 1024) bx = 1024;
  hipLaunchKernelGGL(rgb8_kernel, dim3((unsigned)bx, F), dim3(kThreads), 0, eavsr::as_stream(stream), sr, scale, C, hw, rgb8);
  return eavsr::launch_status("rgb8");
}
