// PWC-Net (models/pwc_net.py) for the late-training validity mask (models/eavsrp_model.py:85-97, models/base_model.py:294-354):
// the strided / dilated 3x3 convolutions of Extractor, Decoder and Refiner on the fp32 MFMA pipe, the two transposed 4x4 / stride-2
// convolutions of a decoder level, the 81-channel cost volume (pwc/correlation/correlation.py:35-103) and the normalised-grid
// backwarp with its thresholded ones channel.  Every tensor is fp32 NCHW with an explicit batch stride, so that the decoder's
// dense concatenations are channel slices of one buffer per level (no torch.cat).
#include "common.h"

namespace {

// ---------------------------------------------------------------------------------------------------------------------------
// 3x3 convolution, stride 1 | 2, dilation d with padding d: implicit GEMM, M = output channels, N = output pixels (all samples
// flattened, so a 1 x 1 level still fills a tile), K = 9 taps x cin.  A 256-thread workgroup owns a (32 CO_T) x (32 PX_T) output
// tile; its four waves split cin four ways (K split: the level-2 convolutions have ~450 tiles of 64 x 64 on 1024 SIMDs) and sum
// their accumulators through LDS.  Every wave issues CO_T + PX_T operand loads per CO_T x PX_T v_mfma_f32_32x32x2_f32.
// Packed weight: [9][ci_pad][co_pad], ci_pad = cin rounded up to even, co_pad = cout rounded up to 32 CO_T, zeros in the padding.
// ---------------------------------------------------------------------------------------------------------------------------
constexpr int kSplit = 4;

__host__ __device__ inline int conv_co_t(int cout) { return cout > 32 ? 2 : 1; }
__host__ __device__ inline int conv_ci_pad(int cin) { return (cin + 1) & ~1; }
__host__ __device__ inline int conv_co_pad(int cout) {
  const int t = 32 * conv_co_t(cout);
  return (cout + t - 1) / t * t;
}

__global__ void pwc_pack_conv3x3_kernel(const float* __restrict__ w, float* __restrict__ packed, int cout, int cin, int ci_pad,
                                        int co_pad) {
  const long total = 9L * ci_pad * co_pad;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int co = (int)(i % co_pad);
    const int ci = (int)((i / co_pad) % ci_pad);
    const int tap = (int)(i / ((long)co_pad * ci_pad));
    packed[i] = (co < cout && ci < cin) ? w[((long)co * cin + ci) * 9 + tap] : 0.f;
  }
}

template <int CO_T, int PX_T>
__global__ __launch_bounds__(256) void pwc_conv3x3_kernel(const float* __restrict__ x, long xs_n, int cin, int h, int w,
                                                          const float* __restrict__ wp, int ci_pad, int co_pad,
                                                          const float* __restrict__ bias, float* __restrict__ out, long os_n,
                                                          int cout, int ho, int wo, int stride, int dil, int npix, float act_s) {
  constexpr int NT = CO_T * PX_T;
  __shared__ float red[kSplit][NT * 16][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int ptiles = (npix + 32 * PX_T - 1) / (32 * PX_T);
  const int p0 = (blockIdx.x % ptiles) * 32 * PX_T;
  const int c0 = (blockIdx.x / ptiles) * 32 * CO_T;
  const int hwo = ho * wo, hwi = h * w;
  const int kl = lane >> 5, col = lane & 31;

  long pbase[PX_T];
  int iy0[PX_T], ix0[PX_T];
#pragma unroll
  for (int j = 0; j < PX_T; ++j) {
    const int p = p0 + j * 32 + col;
    const bool pv = p < npix;
    const int pp = pv ? p : 0;
    const int nn = pp / hwo, r = pp - nn * hwo;
    const int oy = r / wo, ox = r - oy * wo;
    pbase[j] = (long)nn * xs_n;
    // pixels past npix never pass the bounds test below
    iy0[j] = pv ? oy * stride - dil : -(1 << 28);
    ix0[j] = ox * stride - dil;
  }

  const int cq = ((cin + 2 * kSplit - 1) / (2 * kSplit)) * 2;
  const int ci_lo = wave * cq, ci_hi = min(cin, ci_lo + cq);

  f32x16 acc[CO_T][PX_T];
#pragma unroll
  for (int i = 0; i < CO_T; ++i)
#pragma unroll
    for (int j = 0; j < PX_T; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  for (int tap = 0; tap < 9; ++tap) {
    const int ky = tap / 3, kx = tap - ky * 3;
    long off[PX_T];
    bool ok[PX_T];
#pragma unroll
    for (int j = 0; j < PX_T; ++j) {
      const int iy = iy0[j] + ky * dil, ix = ix0[j] + kx * dil;
      ok[j] = iy >= 0 && iy < h && ix >= 0 && ix < w;
      off[j] = ok[j] ? pbase[j] + (long)iy * w + ix : 0;
    }
    const float* wt = wp + (long)tap * ci_pad * co_pad + c0 + col;
    // the small levels (a few hundred pixels, one or two workgroups) are a chain of 9 x cin / 8 load -> MFMA steps per wave,
    // bound by the load latency; unrolling by 8 instead of 2 measured the same (9.1 ms per get_backwarp)
#pragma unroll 8
    for (int ci = ci_lo; ci < ci_hi; ci += 2) {
      const int c = ci + kl;
      const bool cok = c < ci_hi;
      float a[CO_T], b[PX_T];
#pragma unroll
      for (int i = 0; i < CO_T; ++i) a[i] = wt[(long)c * co_pad + i * 32];
#pragma unroll
      for (int j = 0; j < PX_T; ++j) b[j] = (ok[j] && cok) ? x[off[j] + (long)c * hwi] : 0.f;
#pragma unroll
      for (int i = 0; i < CO_T; ++i)
#pragma unroll
        for (int j = 0; j < PX_T; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i], b[j], acc[i][j], 0, 0, 0);
    }
  }

#pragma unroll
  for (int i = 0; i < CO_T; ++i)
#pragma unroll
    for (int j = 0; j < PX_T; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) red[wave][(i * PX_T + j) * 16 + r][lane] = acc[i][j][r];
  __syncthreads();

  // wave q stores tiles q, q + 4, ...: the sum of the four K quarters, + bias, activation
  for (int t = wave; t < NT; t += kSplit) {
    const int i = t / PX_T, j = t - i * PX_T;
    const int p = p0 + j * 32 + col;
    if (p >= npix) continue;
    const int nn = p / hwo, r = p - nn * hwo;
    float* o = out + (long)nn * os_n + r;
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const int co = c0 + i * 32 + (q & 3) + 8 * (q >> 2) + 4 * kl;
      if (co >= cout) continue;
      float v = red[0][t * 16 + q][lane] + red[1][t * 16 + q][lane] + red[2][t * 16 + q][lane] + red[3][t * 16 + q][lane];
      v += bias ? bias[co] : 0.f;
      o[(long)co * hwo] = eavsr_act(v, act_s);
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------------
// ConvTranspose2d(cin -> 2, kernel 4, stride 2, padding 1): output pixel (oy, ox) = (2 qy + py, 2 qx + px) gathers the 2 x 2 input
// pixels iy = (oy + 1 - ky) / 2 over the two ky of parity (oy + 1) % 2 (likewise x).  blockIdx.y is the output parity phase, so
// each workgroup reads one uniform set of four taps per input channel (weight (cin, 2, 4, 4) as nn.ConvTranspose2d stores it).
// ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void pwc_deconv4x4s2_kernel(const float* __restrict__ x, long xs_n, int cin, int h, int w,
                                                              const float* __restrict__ wt, const float* __restrict__ bias,
                                                              float* __restrict__ out, long os_n, int n) {
  const int py = blockIdx.y >> 1, px = blockIdx.y & 1;
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= n * h * w) return;
  const int nn = idx / (h * w), r = idx - nn * h * w;
  const int qy = r / w, qx = r - qy * w;
  const int oy = 2 * qy + py, ox = 2 * qx + px;
  // the two taps per axis: k = 1 - p + 2 t (t = 0, 1), input coordinate (o + 1 - k) / 2
  int ky[2], kx[2], iy[2], ix[2];
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    ky[t] = 1 - py + 2 * t;
    kx[t] = 1 - px + 2 * t;
    iy[t] = (oy + 1 - ky[t]) / 2;
    ix[t] = (ox + 1 - kx[t]) / 2;
  }
  long off[4];
  bool ok[4];
  int kk[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int a = t >> 1, b = t & 1;
    ok[t] = iy[a] >= 0 && iy[a] < h && ix[b] >= 0 && ix[b] < w;
    off[t] = ok[t] ? (long)iy[a] * w + ix[b] : 0;
    kk[t] = ky[a] * 4 + kx[b];
  }
  const float* xp = x + (long)nn * xs_n;
  const long hw = (long)h * w;
  float s0 = 0.f, s1 = 0.f;
  for (int ci = 0; ci < cin; ++ci) {
    const float* wc = wt + (long)ci * 32;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const float v = ok[t] ? xp[ci * hw + off[t]] : 0.f;
      s0 = fmaf(v, wc[kk[t]], s0);
      s1 = fmaf(v, wc[16 + kk[t]], s1);
    }
  }
  const int wo = 2 * w;
  float* o = out + (long)nn * os_n + (long)oy * wo + ox;
  o[0] = s0 + (bias ? bias[0] : 0.f);
  o[(long)4 * hw] = s1 + (bias ? bias[1] : 0.f);
}

// ---------------------------------------------------------------------------------------------------------------------------
// cost volume: out[n, (dy+4)*9 + (dx+4), y, x] = lrelu_0.1((1/C) sum_c a[n,c,y,x] b[n,c,y+dy,x+dx]), zero outside the image.
// One thread per output element, consecutive threads along x: both operand reads coalesce.
// ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void pwc_correlation_kernel(const float* __restrict__ a, long as_n, const float* __restrict__ b,
                                                              long bs_n, float* __restrict__ out, long os_n, int n, int c, int h,
                                                              int w, float inv_c) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  const long hw = (long)h * w;
  if (idx >= (long)n * 81 * hw) return;
  const int x = (int)(idx % w);
  const int y = (int)((idx / w) % h);
  const int d = (int)((idx / hw) % 81);
  const int nn = (int)(idx / (81 * hw));
  const int y2 = y + d / 9 - 4, x2 = x + d % 9 - 4;
  float s = 0.f;
  if (y2 >= 0 && y2 < h && x2 >= 0 && x2 < w) {
    const float* pa = a + (long)nn * as_n + (long)y * w + x;
    const float* pb = b + (long)nn * bs_n + (long)y2 * w + x2;
    for (int ch = 0; ch < c; ++ch) s = fmaf(pa[ch * hw], pb[ch * hw], s);
    s *= inv_c;
  }
  out[(long)nn * os_n + (long)d * hw + (long)y * w + x] = s > 0.f ? s : 0.1f * s;
}

// ---------------------------------------------------------------------------------------------------------------------------
// backwarp: grid_sample(bilinear, zeros, align_corners=False) of x at linspace(-1 + 1/W, 1 - 1/W) + flow / ((W - 1) / 2), i.e. at
// pixel x + f W / (W - 1), computed in the grid's normalised form as torch does.  The flow is read at (y / fs, x / fs) (nearest
// upsampling by fs; 1 = same size) and multiplied by fmul.  The ones channel (the summed weights of the in-image corners) is
// thresholded: mask = ones > 0.999.  out = warped x mask; `mask` (nullable) receives the mask.
// ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void pwc_backwarp_kernel(const float* __restrict__ x, long xs_n, const float* __restrict__ flow,
                                                           long fs_n, float* __restrict__ out, long os_n, float* __restrict__ mask,
                                                           int n, int c, int h, int w, int fh, int fw, int fs, float fmul) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= n * h * w) return;
  const int nn = idx / (h * w), r = idx - nn * h * w;
  const int y = r / w, xx = r - y * w;
  const float* fp = flow + (long)nn * fs_n + (long)(y / fs) * fw + xx / fs;
  const float fx = fp[0] * fmul, fy = fp[(long)fh * fw] * fmul;
  const float gx = (-1.f + (float)(2 * xx + 1) / (float)w) + fx / (((float)w - 1.f) / 2.f);
  const float gy = (-1.f + (float)(2 * y + 1) / (float)h) + fy / (((float)h - 1.f) / 2.f);
  // clamped before the int conversion, as flow_warp does: every position outside [-4, size + 4] has all four corners outside the
  // image, as its clamped value has, and a NaN becomes -4 (fmaxf returns its other operand): mask 0 and out 0, not NaN x 0
  const float ix = fminf(fmaxf(((gx + 1.f) * (float)w - 1.f) / 2.f, -4.f), (float)w + 4.f);
  const float iy = fminf(fmaxf(((gy + 1.f) * (float)h - 1.f) / 2.f, -4.f), (float)h + 4.f);
  const float x0f = floorf(ix), y0f = floorf(iy);
  const int x0 = (int)x0f, y0 = (int)y0f, x1 = x0 + 1, y1 = y0 + 1;
  const float wnw = (x0f + 1.f - ix) * (y0f + 1.f - iy), wne = (ix - x0f) * (y0f + 1.f - iy);
  const float wsw = (x0f + 1.f - ix) * (iy - y0f), wse = (ix - x0f) * (iy - y0f);
  const bool vx0 = x0 >= 0 && x0 < w, vx1 = x1 >= 0 && x1 < w, vy0 = y0 >= 0 && y0 < h, vy1 = y1 >= 0 && y1 < h;
  const bool bnw = vx0 && vy0, bne = vx1 && vy0, bsw = vx0 && vy1, bse = vx1 && vy1;
  float ones = 0.f;
  if (bnw) ones += wnw;
  if (bne) ones += wne;
  if (bsw) ones += wsw;
  if (bse) ones += wse;
  const float m = ones > 0.999f ? 1.f : 0.f;
  if (mask) mask[idx] = m;
  const long hw = (long)h * w;
  const float* xp = x + (long)nn * xs_n;
  float* o = out + (long)nn * os_n + r;
  for (int ch = 0; ch < c; ++ch) {
    const float* pc = xp + ch * hw;
    float v = 0.f;
    if (bnw) v += pc[(long)y0 * w + x0] * wnw;
    if (bne) v += pc[(long)y0 * w + x1] * wne;
    if (bsw) v += pc[(long)y1 * w + x0] * wsw;
    if (bse) v += pc[(long)y1 * w + x1] * wse;
    o[ch * hw] = v * m;
  }
}

inline int blocks_of(long count) { return (int)((count + 255) / 256); }

}  // namespace

extern "C" int64_t eavsr_pwc_conv3x3_weight_elems(int32_t cout, int32_t cin) {
  if (cout <= 0 || cin <= 0) return -1;
  return 9L * conv_ci_pad(cin) * conv_co_pad(cout);
}

extern "C" int eavsr_pwc_pack_conv3x3_f32(const float* weight, float* packed, int32_t cout, int32_t cin, void* stream) {
  EAVSR_REQUIRE(weight && packed, -1, "pwc_pack_conv3x3: NULL pointer");
  EAVSR_REQUIRE(cout > 0 && cin > 0 && cout <= 1024 && cin <= 4096, -1, "pwc_pack_conv3x3: bad dims cout=%d cin=%d", cout, cin);
  const long total = 9L * conv_ci_pad(cin) * conv_co_pad(cout);
  hipLaunchKernelGGL(pwc_pack_conv3x3_kernel, dim3((unsigned)std::min<long>(blocks_of(total), 4096)), dim3(256), 0,
                     eavsr::as_stream(stream), weight, packed, cout, cin, conv_ci_pad(cin), conv_co_pad(cout));
  return eavsr::launch_status("pwc_pack_conv3x3");
}

extern "C" int eavsr_pwc_conv3x3_f32(const float* x, int64_t x_batch_stride, const float* weight_packed, const float* bias,
                                     float* out, int64_t out_batch_stride, int32_t n, int32_t cin, int32_t h, int32_t w,
                                     int32_t cout, int32_t stride, int32_t dilation, int32_t act, float slope, void* stream) {
  EAVSR_REQUIRE(x && weight_packed && out, -1, "pwc_conv3x3: NULL pointer");
  EAVSR_REQUIRE(n > 0 && cin > 0 && h > 0 && w > 0 && cout > 0 && cin <= 4096 && cout <= 1024, -1,
                "pwc_conv3x3: bad dims n=%d cin=%d h=%d w=%d cout=%d", n, cin, h, w, cout);
  EAVSR_REQUIRE(stride == 1 || stride == 2, -2, "pwc_conv3x3: stride %d (1 or 2)", stride);
  EAVSR_REQUIRE(dilation >= 1 && dilation <= 64, -2, "pwc_conv3x3: dilation %d", dilation);
  EAVSR_REQUIRE(act == EAVSR_ACT_NONE || act == EAVSR_ACT_LRELU, -2, "pwc_conv3x3: act %d (none or leaky ReLU)", act);
  EAVSR_REQUIRE(x_batch_stride >= (int64_t)cin * h * w, -1, "pwc_conv3x3: input batch stride %lld < cin*h*w",
                (long long)x_batch_stride);
  const int ho = (h - 1) / stride + 1, wo = (w - 1) / stride + 1;
  EAVSR_REQUIRE(out_batch_stride >= (int64_t)cout * ho * wo, -1, "pwc_conv3x3: output batch stride %lld < cout*ho*wo",
                (long long)out_batch_stride);
  const long npix_l = (long)n * ho * wo;
  EAVSR_REQUIRE(npix_l < (1L << 30), -1, "pwc_conv3x3: too many output pixels");
  const int npix = (int)npix_l;
  const float act_s = act == EAVSR_ACT_LRELU ? slope : 1.f;
  const int ci_pad = conv_ci_pad(cin), co_pad = conv_co_pad(cout);
  hipStream_t st = eavsr::as_stream(stream);
  if (conv_co_t(cout) == 2) {
    const int blocks = eavsr::cdiv(npix, 64) * (co_pad / 64);
    hipLaunchKernelGGL((pwc_conv3x3_kernel<2, 2>), dim3(blocks), dim3(256), 0, st, x, (long)x_batch_stride, cin, h, w,
                       weight_packed, ci_pad, co_pad, bias, out, (long)out_batch_stride, cout, ho, wo, stride, dilation, npix,
                       act_s);
  } else {
    const int blocks = eavsr::cdiv(npix, 128) * (co_pad / 32);
    hipLaunchKernelGGL((pwc_conv3x3_kernel<1, 4>), dim3(blocks), dim3(256), 0, st, x, (long)x_batch_stride, cin, h, w,
                       weight_packed, ci_pad, co_pad, bias, out, (long)out_batch_stride, cout, ho, wo, stride, dilation, npix,
                       act_s);
  }
  return eavsr::launch_status("pwc_conv3x3");
}

extern "C" int eavsr_pwc_deconv4x4s2_f32(const float* x, int64_t x_batch_stride, const float* weight, const float* bias,
                                         float* out, int64_t out_batch_stride, int32_t n, int32_t cin, int32_t h, int32_t w,
                                         void* stream) {
  EAVSR_REQUIRE(x && weight && out, -1, "pwc_deconv4x4s2: NULL pointer");
  EAVSR_REQUIRE(n > 0 && cin > 0 && h > 0 && w > 0 && (long)n * h * w < (1L << 30), -1, "pwc_deconv4x4s2: bad dims");
  EAVSR_REQUIRE(x_batch_stride >= (int64_t)cin * h * w, -1, "pwc_deconv4x4s2: input batch stride < cin*h*w");
  EAVSR_REQUIRE(out_batch_stride >= (int64_t)2 * 4 * h * w, -1, "pwc_deconv4x4s2: output batch stride < 2*(2h)*(2w)");
  hipLaunchKernelGGL(pwc_deconv4x4s2_kernel, dim3(blocks_of((long)n * h * w), 4), dim3(256), 0, eavsr::as_stream(stream), x,
                     (long)x_batch_stride, cin, h, w, weight, bias, out, (long)out_batch_stride, n);
  return eavsr::launch_status("pwc_deconv4x4s2");
}

extern "C" int eavsr_pwc_correlation_f32(const float* a, int64_t a_batch_stride, const float* b, int64_t b_batch_stride,
                                         float* out, int64_t out_batch_stride, int32_t n, int32_t c, int32_t h, int32_t w,
                                         void* stream) {
  EAVSR_REQUIRE(a && b && out, -1, "pwc_correlation: NULL pointer");
  EAVSR_REQUIRE(n > 0 && c > 0 && h > 0 && w > 0 && (long)n * 81 * h * w < (1L << 40), -1, "pwc_correlation: bad dims");
  EAVSR_REQUIRE(a_batch_stride >= (int64_t)c * h * w && b_batch_stride >= (int64_t)c * h * w, -1,
                "pwc_correlation: operand batch stride < c*h*w");
  EAVSR_REQUIRE(out_batch_stride >= (int64_t)81 * h * w, -1, "pwc_correlation: output batch stride < 81*h*w");
  const long total = (long)n * 81 * h * w;
  EAVSR_REQUIRE(total / 256 < (1L << 31), -1, "pwc_correlation: too large");
  hipLaunchKernelGGL(pwc_correlation_kernel, dim3(blocks_of(total)), dim3(256), 0, eavsr::as_stream(stream), a,
                     (long)a_batch_stride, b, (long)b_batch_stride, out, (long)out_batch_stride, n, c, h, w, 1.f / (float)c);
  return eavsr::launch_status("pwc_correlation");
}

extern "C" int eavsr_pwc_backwarp_f32(const float* x, int64_t x_batch_stride, const float* flow, int64_t flow_batch_stride,
                                      float* out, int64_t out_batch_stride, float* mask, int32_t n, int32_t c, int32_t h, int32_t w,
                                      int32_t flow_h, int32_t flow_w, float flow_mul, void* stream) {
  EAVSR_REQUIRE(x && flow && out, -1, "pwc_backwarp: NULL pointer");
  EAVSR_REQUIRE(n > 0 && c > 0 && h > 1 && w > 1 && flow_h > 0 && flow_w > 0 && (long)n * h * w < (1L << 30), -1,
                "pwc_backwarp: bad dims (h, w > 1)");
  const int fs = h / flow_h;
  EAVSR_REQUIRE(fs >= 1 && h == fs * flow_h && w == fs * flow_w, -2,
                "pwc_backwarp: image %dx%d is not the flow %dx%d upsampled by one integer factor", h, w, flow_h, flow_w);
  EAVSR_REQUIRE(x_batch_stride >= (int64_t)c * h * w && out_batch_stride >= (int64_t)c * h * w, -1,
                "pwc_backwarp: batch stride < c*h*w");
  EAVSR_REQUIRE(flow_batch_stride >= (int64_t)2 * flow_h * flow_w, -1, "pwc_backwarp: flow batch stride < 2*h*w");
  hipLaunchKernelGGL(pwc_backwarp_kernel, dim3(blocks_of((long)n * h * w)), dim3(256), 0, eavsr::as_stream(stream), x,
                     (long)x_batch_stride, flow, (long)flow_batch_stride, out, (long)out_batch_stride, mask, n, c, h, w, flow_h,
                     flow_w, fs, flow_mul);
  return eavsr::launch_status("pwc_backwarp");
}
