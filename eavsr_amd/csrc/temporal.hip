// Temporal consistency of the evaluation report: per pair of consecutive frames (t, t + 1) the warping error after
// Lai et al. (ECCV 2018; occlusion test after Ruder et al. 2016) and the flow distance tOF after Chu et al. (TOG 2020), in one
// fused pass.  The definition is this project's own, fixed operation by operation so that numpy restates it exactly
// (tests/temporal_ref.py); for pair t and pixel (x, y), every fp32 operation rounded on its own:
//   u = fw[t,0,y,x], v = fw[t,1,y,x];  sx = float(x) + u, sy = float(y) + v
//   inside = 0 <= sx <= W - 1 and 0 <= sy <= H - 1                                       (false for NaN)
//   x0 = floor(sx), ax = sx - x0, x1 = min(x0 + 1, W - 1)   (y likewise)
//   bil(P) = (1 - ay) ((1 - ax) P[y0,x0] + ax P[y0,x1]) + ay ((1 - ax) P[y1,x0] + ax P[y1,x1])
//   bu = bil(bw[t,0]), bv = bil(bw[t,1]);  m_f = u u + v v, m_b = bu bu + bv bv, m_fb = (u + bu)^2 + (v + bv)^2
//   g = the squared forward differences of fw[t] to the right and below (0 at the last column / row)
//   valid = inside and m_fb <= 0.01 (m_f + m_b) + 0.5 and g <= 0.01 m_f + 0.002              (any NaN: not valid)
//   valid:  count += 1;  per plane c: d = q(seq[t,c,y,x]) - bil(q(seq[t+1,c])), err += (double)d (double)d
//   flow_b: eu = flow_b[t,0,y,x] - u, ev = flow_b[t,1,y,x] - v, epe += sqrt((double)eu eu + (double)ev ev)     (every pixel)
// with q(p) = rint(clamp(p scale, 0, 255)), the quantisation of metrics.hip.  This file is built WITHOUT floating-point contraction
// (eavsr_amd/build.py PER_FILE_FLAGS): a fused multiply-add would round once where the definition rounds twice.
//
// A 256-thread workgroup owns a 64 x 16 pixel tile of one pair: wave w takes rows w, w + 4, w + 8, w + 12 of the tile, a lane a
// column, so every row a wave reads is one contiguous run and the gather's taps (the four of bw and of each plane of frame t + 1,
// the right and lower neighbour of fw) stay inside a few neighbouring rows.  A lane sums its pixels in row order, the wave sums its
// lanes by a fixed butterfly, lane 0 of wave 0 the four waves in order: ONE (err, epe, count) record per workgroup, written with
// ordinary stores; a second kernel sums a pair's records in a fixed order.  No atomics: two calls on the same input are bitwise equal.
#include "pixel.h"

#include <math.h>

namespace {

constexpr int kTW = 64, kTH = 16;      // pixels per tile
constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;

struct Partial {      // one per workgroup; 24 bytes
  double err;
  double epe;
  int64_t count;
};

struct Taps {      // the four samples of a bilinear read and their weights
  size_t o00, o01, o10, o11;
  float ax, ay, bx, by;      // bx = 1 - ax, by = 1 - ay
};

__device__ __forceinline__ float mix(const Taps& k, float p00, float p01, float p10, float p11) {
  const float top = k.bx * p00 + k.ax * p01;
  const float bot = k.bx * p10 + k.ax * p11;
  return k.by * top + k.ay * bot;
}

__global__ __launch_bounds__(kThreads) void temporal_metrics_kernel(const float* __restrict__ seq, const float* __restrict__ fw,
                                                                    const float* __restrict__ bw, const float* __restrict__ flow_b,
                                                                    float scale, int C, int H, int W, Partial* __restrict__ partials) {
  __shared__ double red_err[kWaves], red_epe[kWaves];
  __shared__ long long red_count[kWaves];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int t = blockIdx.z;
  const int x = blockIdx.x * kTW + lane;
  const size_t hw = (size_t)H * W;
  const float* fu = fw + (size_t)t * 2 * hw;
  const float* fv = fu + hw;
  const float* bu_p = bw + (size_t)t * 2 * hw;
  const float* bv_p = bu_p + hw;
  const float* cur = seq + (size_t)t * C * hw;
  const float* nxt = cur + (size_t)C * hw;

  double err = 0.0, epe = 0.0;
  long long count = 0;
  if (x < W) {
    const int xr = min(x + 1, W - 1);
    for (int k = 0; k < kTH / kWaves; ++k) {
      const int y = blockIdx.y * kTH + wave + k * kWaves;
      if (y >= H) break;
      const int yd = min(y + 1, H - 1);
      const size_t at = (size_t)y * W + x;
      const float u = fu[at], v = fv[at];
      if (flow_b) {
        const float eu = flow_b[(size_t)t * 2 * hw + at] - u, ev = flow_b[(size_t)t * 2 * hw + hw + at] - v;
        epe += sqrt((double)eu * (double)eu + (double)ev * (double)ev);
      }
      const float sx = (float)x + u, sy = (float)y + v;
      if (!(sx >= 0.f && sx <= (float)(W - 1) && sy >= 0.f && sy <= (float)(H - 1))) continue;      // NaN: not inside
      const float fx0 = floorf(sx), fy0 = floorf(sy);
      const int x0 = (int)fx0, y0 = (int)fy0;      // 0 .. W - 1, 0 .. H - 1
      const int x1 = min(x0 + 1, W - 1), y1 = min(y0 + 1, H - 1);
      Taps tp;
      tp.ax = sx - fx0;
      tp.ay = sy - fy0;
      tp.bx = 1.f - tp.ax;
      tp.by = 1.f - tp.ay;
      tp.o00 = (size_t)y0 * W + x0;
      tp.o01 = (size_t)y0 * W + x1;
      tp.o10 = (size_t)y1 * W + x0;
      tp.o11 = (size_t)y1 * W + x1;
      const float bu = mix(tp, bu_p[tp.o00], bu_p[tp.o01], bu_p[tp.o10], bu_p[tp.o11]);
      const float bv = mix(tp, bv_p[tp.o00], bv_p[tp.o01], bv_p[tp.o10], bv_p[tp.o11]);
      const float m_f = u * u + v * v, m_b = bu * bu + bv * bv;
      const float du = u + bu, dv = v + bv;
      const float m_fb = du * du + dv * dv;
      const size_t right = (size_t)y * W + xr, below = (size_t)yd * W + x;
      const float gxu = fu[right] - u, gxv = fv[right] - v, gyu = fu[below] - u, gyv = fv[below] - v;
      const float g = (gxu * gxu + gxv * gxv) + (gyu * gyu + gyv * gyv);
      if (!(m_fb <= 0.01f * (m_f + m_b) + 0.5f && g <= 0.01f * m_f + 0.002f)) continue;      // any NaN: not valid
      count += 1;
      for (int c = 0; c < C; ++c) {
        const float* n = nxt + (size_t)c * hw;
        const float warped = mix(tp, quantise(n[tp.o00], scale), quantise(n[tp.o01], scale), quantise(n[tp.o10], scale),
                                 quantise(n[tp.o11], scale));
        const float d = quantise(cur[(size_t)c * hw + at], scale) - warped;
        err += (double)d * (double)d;
      }
    }
  }

  // wavefront (a fixed butterfly: every lane ends with the same bits), then the four wavefronts in order
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    err += __shfl_xor(err, off);
    epe += __shfl_xor(epe, off);
    count += __shfl_xor(count, off);
  }
  if (lane == 0) {
    red_err[wave] = err;
    red_epe[wave] = epe;
    red_count[wave] = count;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    Partial p;
    p.err = ((red_err[0] + red_err[1]) + red_err[2]) + red_err[3];
    p.epe = ((red_epe[0] + red_epe[1]) + red_epe[2]) + red_epe[3];
    p.count = (int64_t)(red_count[0] + red_count[1] + red_count[2] + red_count[3]);
    partials[((size_t)t * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = p;
  }
}

// a pair's records summed in a fixed order: lane i takes records i, i + 256, ... in turn, then a fixed tree over the lanes
__global__ __launch_bounds__(kThreads) void temporal_metrics_sum_kernel(const Partial* __restrict__ partials, int count,
                                                                        double* __restrict__ err_out, long long* __restrict__ count_out,
                                                                        double* __restrict__ epe_out) {
  __shared__ double s_err[kThreads], s_epe[kThreads];
  __shared__ long long s_count[kThreads];
  const int i0 = threadIdx.x, t = blockIdx.x;
  const Partial* p = partials + (size_t)t * count;
  double e = 0.0, d = 0.0;
  long long n = 0;
  for (int i = i0; i < count; i += kThreads) {
    e += p[i].err;
    d += p[i].epe;
    n += p[i].count;
  }
  s_err[i0] = e;
  s_epe[i0] = d;
  s_count[i0] = n;
  __syncthreads();
  for (int half = kThreads / 2; half > 0; half >>= 1) {
    if (i0 < half) {
      s_err[i0] += s_err[i0 + half];
      s_epe[i0] += s_epe[i0 + half];
      s_count[i0] += s_count[i0 + half];
    }
    __syncthreads();
  }
  if (i0 == 0) {
    err_out[t] = s_err[0];
    count_out[t] = s_count[0];
    if (epe_out) epe_out[t] = s_epe[0];
  }
}

bool shape_ok(const char* what, int32_t F, int32_t C, int32_t H, int32_t W) {
  if (F < 2 || F > 65536) {
    eavsr::set_error("%s: F=%d frames outside 2..65536 (a pair needs two)", what, F);
    return false;
  }
  if (C != 1 && C != 3) {
    eavsr::set_error("%s: C=%d planes, must be 1 or 3", what, C);
    return false;
  }
  if (H < 1 || W < 1) {
    eavsr::set_error("%s: frame %d x %d, at least 1 x 1", what, H, W);
    return false;
  }
  if (H > (1 << 24) || W > (1 << 24)) {      // float(x), float(y) and W - 1, H - 1 must be exact in fp32
    eavsr::set_error("%s: frame %d x %d, a side above 2^24", what, H, W);
    return false;
  }
  if (eavsr::cdiv(H, kTH) > 65535 || (int64_t)eavsr::cdiv(H, kTH) * eavsr::cdiv(W, kTW) > INT32_MAX) {
    eavsr::set_error("%s: frame %d x %d too large", what, H, W);
    return false;
  }
  return true;
}

}  // namespace

extern "C" int32_t eavsr_temporal_metrics_partials(int32_t F, int32_t C, int32_t H, int32_t W) {
  if (!shape_ok("temporal_metrics_partials", F, C, H, W)) return -2;
  return eavsr::cdiv(W, kTW) * eavsr::cdiv(H, kTH);
}

extern "C" int eavsr_temporal_metrics_f32(const float* seq, const float* fw, const float* bw, const float* flow_b, float scale, int32_t F,
                                          int32_t C, int32_t H, int32_t W, void* workspace, double* err_out, int64_t* count_out,
                                          double* epe_out, void* stream) {
  EAVSR_REQUIRE(seq && fw && bw && workspace && err_out && count_out, -1, "temporal_metrics: NULL pointer");
  EAVSR_REQUIRE((flow_b == nullptr) == (epe_out == nullptr), -1, "temporal_metrics: flow_b and epe_out go together");
  if (!shape_ok("temporal_metrics", F, C, H, W)) return -2;
  EAVSR_REQUIRE((((uintptr_t)workspace | (uintptr_t)err_out | (uintptr_t)count_out | (uintptr_t)epe_out) & 7) == 0, -2,
                "temporal_metrics: workspace and outputs must be 8-byte aligned");
  static_assert(sizeof(Partial) == 24, "the workspace is 24 bytes per record");
  const dim3 grid(eavsr::cdiv(W, kTW), eavsr::cdiv(H, kTH), F - 1);
  hipLaunchKernelGGL(temporal_metrics_kernel, grid, dim3(kThreads), 0, eavsr::as_stream(stream), seq, fw, bw, flow_b, scale, C, H, W,
                     (Partial*)workspace);
  int rc = eavsr::launch_status("temporal_metrics");
  if (rc) return rc;
  hipLaunchKernelGGL(temporal_metrics_sum_kernel, dim3(F - 1), dim3(kThreads), 0, eavsr::as_stream(stream), (const Partial*)workspace,
                     (int)(grid.x * grid.y), err_out, (long long*)count_out, epe_out);
  return eavsr::launch_status("temporal_metrics_sum");
}
