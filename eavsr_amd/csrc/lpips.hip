// LPIPS with the AlexNet backbone, the third column of the evaluation report (psnr_total.py:27-35, :116-138), as the published
// definition states it (lpips 0.1, LPIPS(net='alex'), eval mode, spatial=False, normalize=False) on the 8-bit images:
//   q = rint(clamp(v * scale, 0, 255)) (half to even), x = q / 127.5 - 1, (x - shift) / scale per channel (the scaling layer);
//   AlexNet `features`: conv 3->64 11x11 /4 pad 2, ReLU | maxpool 3/2, conv 64->192 5x5 pad 2, ReLU | maxpool 3/2, conv 192->384
//   3x3 pad 1, ReLU | conv 384->256 3x3, ReLU | conv 256->256 3x3, ReLU, tapped after every ReLU;
//   per tap and pixel f^ = f / (sqrt(sum_c f^2) + 1e-10), d = sum_c w_c (f^_sr - f^_hr)^2, the tap's mean of d; LPIPS = the five means
//   added.
// Every tensor is fp32 NCHW.  The SR and HR frames of an item go through the network as ONE batch of 2F images: image f < F is SR
// frame f, image F + f its HR frame.
//
// Convolutions: implicit GEMM on the fp32 matrix pipe (v_mfma_f32_32x32x2_f32, fp32 operands and accumulators: no operand is rounded),
// M = output channels, N = output pixels of all images flattened, K = taps x input channels.  A 256-thread workgroup owns a 64 x 64
// (channels x pixels) output tile; its four waves split K four ways and add their accumulators through LDS, then bias and ReLU.
// The first convolution reads the two fp32 frame sequences themselves and applies the front end in registers (no normalised image
// is stored); its four waves split the 121 taps (K = 363), the other layers split the input channels.
// Packed weight: [taps][ci_pad][cout], ci_pad = cin rounded up to 4, zeros in the padding; cout a multiple of 64.
//
// The tap pass stages a 16-pixel x C tile of both images' features in LDS while it sums the squares (one read of the features),
// then forms the weighted squared difference of the normalised features from LDS.  One fp64 partial per workgroup with ordinary
// stores; a second kernel adds a frame's partials in a fixed order in fp64: no atomics, two calls agree bit for bit.
#include "common.h"

namespace {

constexpr int kSplit = 4;         // waves per workgroup = K quarters
constexpr int kTile = 64;         // output channels and output pixels per workgroup
constexpr int kTapPx = 16;        // pixels per workgroup of the tap pass
constexpr int kTapGroups = 16;    // channel groups per pixel (256 threads)
constexpr int kTapMaxC = 448;     // 2 x 16 x 448 floats = 56 KiB of LDS beside 4 KiB of reduction buffers

inline int ci_pad_of(int cin) { return (cin + 3) & ~3; }

struct FrontEnd {      // the quantiser's scale and the scaling layer's two buffers (device pointers to three floats each)
  float scale;
  const float* shift;
  const float* divisor;
};

__global__ void lpips_pack_conv_kernel(const float* __restrict__ w, float* __restrict__ packed, int cout, int cin, int ci_pad,
                                       int taps) {
  const long total = (long)taps * ci_pad * cout;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int co = (int)(i % cout);
    const int ci = (int)((i / cout) % ci_pad);
    const int tap = (int)(i / ((long)cout * ci_pad));
    packed[i] = ci < cin ? w[((long)co * cin + ci) * taps + tap] : 0.f;
  }
}

// the front end of one sample: quantise, map to [-1, 1], scaling layer (shift, divisor: the sample's channel)
__device__ __forceinline__ float front_end(float v, float scale, float shift, float divisor) {
  const float q = rintf(fminf(fmaxf(v * scale, 0.f), 255.f));
  const float x = q / 127.5f - 1.f;
  return (x - shift) / divisor;
}

// FRONT: x = SR frames, x2 = HR frames (nhalf each, 3 channels), the front end applied at the load, the waves split the taps.
// Otherwise x holds all n images (x2 unused) and the waves split the input channels (cin a multiple of 32).
template <bool FRONT>
__global__ __launch_bounds__(256) void lpips_conv_kernel(const float* __restrict__ x, const float* __restrict__ x2, FrontEnd fe,
                                                         int nhalf, int cin, int h, int w, const float* __restrict__ wp, int ci_pad,
                                                         const float* __restrict__ bias, float* __restrict__ out, int cout, int ho,
                                                         int wo, int ks, int stride, int pad, int npix) {
  __shared__ float red[kSplit][64][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int ptiles = (npix + kTile - 1) / kTile;
  const int p0 = (blockIdx.x % ptiles) * kTile;
  const int c0 = (blockIdx.x / ptiles) * kTile;
  const int hwo = ho * wo;
  const long hwi = (long)h * w;
  const int kl = lane >> 5, col = lane & 31;

  const float* pbase[2];
  int iy0[2], ix0[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int p = p0 + j * 32 + col;
    const bool pv = p < npix;
    const int pp = pv ? p : 0;
    const int nn = pp / hwo, r = pp - nn * hwo;
    const int oy = r / wo, ox = r - oy * wo;
    if (FRONT)
      pbase[j] = nn < nhalf ? x + (long)nn * cin * hwi : x2 + (long)(nn - nhalf) * cin * hwi;
    else
      pbase[j] = x + (long)nn * cin * hwi;
    // pixels past npix never pass the bounds test below
    iy0[j] = pv ? oy * stride - pad : -(1 << 28);
    ix0[j] = ox * stride - pad;
  }

  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  const int taps = ks * ks;
  // One step = one tap and U pairs of input channels (U MFMA k-steps of 2).  FRONT: wave q takes taps q, q + 4, ... with all four
  // (padded) channels; otherwise every tap and the wave's quarter of the channels, 8 at a time.
  constexpr int U = FRONT ? 2 : 4;
  const int cq = cin / kSplit;
  const int ci_lo = FRONT ? 0 : wave * cq;
  const int chunks = FRONT ? 1 : cq / (2 * U);
  const int steps = FRONT ? (taps - wave + kSplit - 1) / kSplit : taps * chunks;
  // FRONT: lane half kl reads channels kl and 2 + kl (channel 3 is padding)
  float fe_shift[2] = {0.f, 0.f}, fe_div[2] = {1.f, 1.f};
  if (FRONT) {
    fe_shift[0] = fe.shift[kl];
    fe_div[0] = fe.divisor[kl];
    if (kl == 0) {
      fe_shift[1] = fe.shift[2];
      fe_div[1] = fe.divisor[2];
    }
  }
  // the operands of step (tap, chunk): a[u][i] the weights of channel pair u for channel tile i, b[u][j] the samples for pixel tile j
  auto load = [&](int tap, int chunk, float (&a)[U][2], float (&b)[U][2]) {
    const int ky = tap / ks, kx = tap - ky * ks;
    long off[2];
    bool ok[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int iy = iy0[j] + ky, ix = ix0[j] + kx;
      ok[j] = iy >= 0 && iy < h && ix >= 0 && ix < w;
      off[j] = ok[j] ? (long)iy * w + ix : 0;
    }
    const float* wt = wp + (long)tap * ci_pad * cout + c0 + col;
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int c = ci_lo + chunk * 2 * U + 2 * u + kl;      // < ci_pad
      const bool cok = c < cin;                              // false for the padding channel of FRONT only
#pragma unroll
      for (int i = 0; i < 2; ++i) a[u][i] = wt[(long)c * cout + i * 32];
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        float v = 0.f;      // the zero padding is applied to the scaling layer's output: a padded sample is 0, not front_end(0)
        if (ok[j] && cok) {
          v = pbase[j][off[j] + (long)c * hwi];
          if (FRONT) v = front_end(v, fe.scale, fe_shift[u], fe_div[u]);
        }
        b[u][j] = v;
      }
    }
  };
  float a[U][2], b[U][2];
  int tap = FRONT ? wave : 0, chunk = 0;
  if (steps > 0) load(tap, chunk, a, b);
  for (int s = 0; s < steps; ++s) {
    // the next step's operands are requested before this step's MFMAs are issued
    float an[U][2], bn[U][2];
    if (++chunk == chunks) {
      chunk = 0;
      tap += FRONT ? kSplit : 1;
    }
    if (s + 1 < steps) load(tap, chunk, an, bn);
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u][i], b[u][j], acc[i][j], 0, 0, 0);
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        a[u][i] = an[u][i];
        b[u][i] = bn[u][i];
      }
  }

#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) red[wave][(i * 2 + j) * 16 + r][lane] = acc[i][j][r];
  __syncthreads();

  // wave q stores 32 x 32 tile q: the sum of the four K quarters in a fixed order, + bias, ReLU
  {
    const int i = wave >> 1, j = wave & 1;
    const int p = p0 + j * 32 + col;
    if (p < npix) {
      const int nn = p / hwo, r = p - nn * hwo;
      float* o = out + (long)nn * cout * hwo + r;
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int co = c0 + i * 32 + (q & 3) + 8 * (q >> 2) + 4 * kl;      // < cout: cout is a multiple of 64
        const int row = wave * 16 + q;
        float v = ((red[0][row][lane] + red[1][row][lane]) + red[2][row][lane]) + red[3][row][lane];
        v += bias[co];
        o[(long)co * hwo] = eavsr_act(v, 0.f);
      }
    }
  }
}

// max over the 3 x 3 window at stride 2, no padding, floor: ho = (h - 3) / 2 + 1; every window lies inside the plane
__global__ __launch_bounds__(256) void lpips_maxpool_kernel(const float* __restrict__ x, float* __restrict__ out, long planes, int h,
                                                            int w, int ho, int wo) {
  const long total = planes * ho * wo;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int ox = (int)(i % wo);
    const int oy = (int)((i / wo) % ho);
    const long pl = i / ((long)wo * ho);
    const float* p = x + (pl * h + 2 * oy) * (long)w + 2 * ox;
    float m = p[0];
#pragma unroll
    for (int dy = 0; dy < 3; ++dy)
#pragma unroll
      for (int dx = 0; dx < 3; ++dx) {
        const float v = p[(long)dy * w + dx];
        m = (v > m || v != v) ? v : m;      // a NaN wins, as in F.max_pool2d
      }
    out[i] = m;
  }
}

// feat (2F, C, h, w); workgroup (tile, f) handles pixels tile * 16 .. + 15 of frame f: images f (SR) and F + f (HR)
__global__ __launch_bounds__(256) void lpips_tap_kernel(const float* __restrict__ feat, const float* __restrict__ lin, int F, int C,
                                                        int hw, double* __restrict__ partials) {
  extern __shared__ float smem[];      // a[C][16], b[C][16]
  __shared__ float s_sq[2][kTapGroups][kTapPx];
  __shared__ double s_red[256];
  float* sa = smem;
  float* sb = smem + (size_t)C * kTapPx;
  const int t = threadIdx.x, px = t & (kTapPx - 1), g = t / kTapPx;
  const int f = blockIdx.y;
  const int p = blockIdx.x * kTapPx + px;
  const bool pv = p < hw;
  const float* pa = feat + (size_t)f * C * hw + (pv ? p : 0);
  const float* pb = feat + (size_t)(F + f) * C * hw + (pv ? p : 0);

  float qa = 0.f, qb = 0.f;
  for (int c = g; c < C; c += kTapGroups) {
    const float a = pv ? pa[(size_t)c * hw] : 0.f;
    const float b = pv ? pb[(size_t)c * hw] : 0.f;
    sa[c * kTapPx + px] = a;
    sb[c * kTapPx + px] = b;
    qa = fmaf(a, a, qa);
    qb = fmaf(b, b, qb);
  }
  s_sq[0][g][px] = qa;
  s_sq[1][g][px] = qb;
  __syncthreads();
  float na = 0.f, nb = 0.f;
#pragma unroll
  for (int k = 0; k < kTapGroups; ++k) {      // every lane of a pixel adds the 16 group sums in the same order
    na += s_sq[0][k][px];
    nb += s_sq[1][k][px];
  }
  na = sqrtf(na) + 1e-10f;
  nb = sqrtf(nb) + 1e-10f;
  float d = 0.f;
  for (int c = g; c < C; c += kTapGroups) {      // the values this lane staged itself
    const float e = sa[c * kTapPx + px] / na - sb[c * kTapPx + px] / nb;
    d = fmaf(lin[c] * e, e, d);
  }
  s_red[t] = pv ? (double)d : 0.0;
  __syncthreads();
  for (int half = 128; half > 0; half >>= 1) {
    if (t < half) s_red[t] += s_red[t + half];
    __syncthreads();
  }
  if (t == 0) partials[(size_t)f * gridDim.x + blockIdx.x] = s_red[0];
}

// a frame's partials added in a fixed order (lane t takes t, t + 256, ..., then a fixed tree); out[f] (+)= sum / hw (the tap's mean)
__global__ __launch_bounds__(256) void lpips_tap_sum_kernel(const double* __restrict__ partials, int count, int hw,
                                                            int accumulate, double* __restrict__ out) {
  __shared__ double s[256];
  const int t = threadIdx.x, f = blockIdx.x;
  const double* p = partials + (size_t)f * count;
  double a = 0.0;
  for (int i = t; i < count; i += 256) a += p[i];
  s[t] = a;
  __syncthreads();
  for (int half = 128; half > 0; half >>= 1) {
    if (t < half) s[t] += s[t + half];
    __syncthreads();
  }
  if (t == 0) out[f] = (accumulate ? out[f] : 0.0) + s[0] / (double)hw;
}

bool conv_shape_ok(const char* what, int32_t n, int32_t cin, int32_t h, int32_t w, int32_t cout, int32_t ks, int ho, int wo) {
  if (n <= 0 || cin <= 0 || h <= 0 || w <= 0 || cout <= 0) {
    eavsr::set_error("%s: bad dims n=%d cin=%d h=%d w=%d cout=%d", what, n, cin, h, w, cout);
    return false;
  }
  if (cout % kTile || cout > 4096 || cin > 4096) {
    eavsr::set_error("%s: cout=%d must be a multiple of %d (cin, cout <= 4096)", what, cout, kTile);
    return false;
  }
  if (ks != 1 && ks != 3 && ks != 5 && ks != 7 && ks != 11) {
    eavsr::set_error("%s: kernel size %d (1, 3, 5, 7 or 11)", what, ks);
    return false;
  }
  if (ho < 1 || wo < 1) {
    eavsr::set_error("%s: image %d x %d leaves no output pixel", what, h, w);
    return false;
  }
  if ((long)n * ho * wo >= (1L << 30) || (long)h * w >= (1L << 30)) {
    eavsr::set_error("%s: too many pixels", what);
    return false;
  }
  return true;
}

}  // namespace

extern "C" int64_t eavsr_lpips_conv_weight_elems(int32_t cout, int32_t cin, int32_t ksize) {
  if (cout <= 0 || cin <= 0 || ksize <= 0 || ksize > 11 || cout > 4096 || cin > 4096) return -1;
  return (int64_t)ksize * ksize * ci_pad_of(cin) * cout;
}

extern "C" int eavsr_lpips_pack_conv_f32(const float* weight, float* packed, int32_t cout, int32_t cin, int32_t ksize, void* stream) {
  EAVSR_REQUIRE(weight && packed, -1, "lpips_pack_conv: NULL pointer");
  EAVSR_REQUIRE(eavsr_lpips_conv_weight_elems(cout, cin, ksize) > 0, -1, "lpips_pack_conv: bad dims cout=%d cin=%d ksize=%d", cout,
                cin, ksize);
  const long total = (long)ksize * ksize * ci_pad_of(cin) * cout;
  hipLaunchKernelGGL(lpips_pack_conv_kernel, dim3((unsigned)std::min<long>((total + 255) / 256, 4096)), dim3(256), 0,
                     eavsr::as_stream(stream), weight, packed, cout, cin, ci_pad_of(cin), ksize * ksize);
  return eavsr::launch_status("lpips_pack_conv");
}

extern "C" int eavsr_lpips_conv1_f32(const float* sr, const float* hr, float scale, const float* shift3, const float* scale3,
                                     const float* weight_packed, const float* bias, float* out, int32_t F, int32_t H, int32_t W,
                                     int32_t cout, void* stream) {
  // shapes first: an output without pixels has no storage, and its NULL pointer is not the caller's mistake
  EAVSR_REQUIRE(H >= 7 && W >= 7, -2, "lpips_conv1: frame %d x %d smaller than the 11 x 11 window less its padding", H, W);
  EAVSR_REQUIRE(sr && hr && shift3 && scale3 && weight_packed && bias && out, -1, "lpips_conv1: NULL pointer");
  EAVSR_REQUIRE(F > 0 && F <= (1 << 20), -1, "lpips_conv1: F=%d", F);
  const int ho = (H + 4 - 11) / 4 + 1, wo = (W + 4 - 11) / 4 + 1;
  if (!conv_shape_ok("lpips_conv1", 2 * F, 3, H, W, cout, 11, ho, wo)) return -2;
  const FrontEnd fe = {scale, shift3, scale3};
  const int npix = 2 * F * ho * wo;
  const int blocks = eavsr::cdiv(npix, kTile) * (cout / kTile);
  hipLaunchKernelGGL((lpips_conv_kernel<true>), dim3(blocks), dim3(256), 0, eavsr::as_stream(stream), sr, hr, fe, F, 3, H, W,
                     weight_packed, ci_pad_of(3), bias, out, cout, ho, wo, 11, 4, 2, npix);
  return eavsr::launch_status("lpips_conv1");
}

extern "C" int eavsr_lpips_conv_f32(const float* x, const float* weight_packed, const float* bias, float* out, int32_t n, int32_t cin,
                                    int32_t h, int32_t w, int32_t cout, int32_t ksize, void* stream) {
  EAVSR_REQUIRE(x && weight_packed && bias && out, -1, "lpips_conv: NULL pointer");
  if (!conv_shape_ok("lpips_conv", n, cin, h, w, cout, ksize, h, w)) return -2;
  EAVSR_REQUIRE(cin % (8 * kSplit) == 0, -2, "lpips_conv: cin=%d must be a multiple of %d", cin, 8 * kSplit);
  const int npix = n * h * w;
  const int blocks = eavsr::cdiv(npix, kTile) * (cout / kTile);
  const FrontEnd fe = {0.f, nullptr, nullptr};
  hipLaunchKernelGGL((lpips_conv_kernel<false>), dim3(blocks), dim3(256), 0, eavsr::as_stream(stream), x, (const float*)nullptr, fe,
                     0, cin, h, w, weight_packed, ci_pad_of(cin), bias, out, cout, h, w, ksize, 1, ksize / 2, npix);
  return eavsr::launch_status("lpips_conv");
}

extern "C" int eavsr_lpips_maxpool3s2_f32(const float* x, float* out, int64_t planes, int32_t h, int32_t w, void* stream) {
  EAVSR_REQUIRE(h >= 3 && w >= 3, -2, "lpips_maxpool3s2: plane %d x %d smaller than the 3 x 3 window", h, w);
  EAVSR_REQUIRE(x && out, -1, "lpips_maxpool3s2: NULL pointer");
  EAVSR_REQUIRE(planes > 0 && planes < (1L << 40), -1, "lpips_maxpool3s2: planes=%lld", (long long)planes);
  const int ho = (h - 3) / 2 + 1, wo = (w - 3) / 2 + 1;
  const long total = (long)planes * ho * wo;
  hipLaunchKernelGGL(lpips_maxpool_kernel, dim3((unsigned)std::min<long>((total + 255) / 256, 1 << 20)), dim3(256), 0,
                     eavsr::as_stream(stream), x, out, (long)planes, h, w, ho, wo);
  return eavsr::launch_status("lpips_maxpool3s2");
}

extern "C" int32_t eavsr_lpips_tap_partials(int32_t h, int32_t w) {
  if (h <= 0 || w <= 0 || (long)h * w >= (1L << 30)) {
    eavsr::set_error("lpips_tap_partials: bad dims %d x %d", h, w);
    return -2;
  }
  return eavsr::cdiv(h * w, kTapPx);
}

extern "C" int eavsr_lpips_tap_f32(const float* feat, const float* lin_weight, void* workspace, double* out, int32_t F, int32_t C,
                                   int32_t h, int32_t w, int32_t accumulate, void* stream) {
  EAVSR_REQUIRE(feat && lin_weight && workspace && out, -1, "lpips_tap: NULL pointer");
  EAVSR_REQUIRE(F >= 0 && F <= 65535, -2, "lpips_tap: F=%d frames outside 0..65535", F);
  EAVSR_REQUIRE(C > 0 && C <= kTapMaxC, -2, "lpips_tap: C=%d channels outside 1..%d", C, kTapMaxC);
  const int parts = eavsr_lpips_tap_partials(h, w);
  if (parts < 0) return -2;
  if (F == 0) return 0;
  const int hw = h * w;
  hipLaunchKernelGGL(lpips_tap_kernel, dim3(parts, F), dim3(256), (size_t)2 * C * kTapPx * sizeof(float), eavsr::as_stream(stream),
                     feat, lin_weight, F, C, hw, (double*)workspace);
  int rc = eavsr::launch_status("lpips_tap");
  if (rc) return rc;
  hipLaunchKernelGGL(lpips_tap_sum_kernel, dim3(F), dim3(256), 0, eavsr::as_stream(stream), (const double*)workspace, parts, hw,
                     accumulate, out);
  return eavsr::launch_status("lpips_tap_sum");
}
