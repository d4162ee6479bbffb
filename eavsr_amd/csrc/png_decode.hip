// The incoming PNG file on the device: the scanline UNfilter (eavsr_png_unfilter_u8).  The inflate stays on the host (one
// serial bit stream per file, C-speed zlib in threads: DESIGN 8); what it leaves -- F x H scanlines, a filter-type byte and W C filtered
// bytes each -- is turned into planar uint8 frames here.  Integer arithmetic, no atomics; two calls on equal input write equal bytes.
//
// Dependencies.  Byte i of row y needs byte i - C of its own row (a) and bytes i (b) and i - C (c) of row y - 1, reconstructed.  A lane
// that owns a row and lags the lane above it by ONE PIXEL therefore always finds its three neighbours finished: a skewed wavefront.
//
// Schedule.  One wave per frame (a workgroup of 64 lanes; frames are independent, nothing waits between workgroups).  The wave walks the
// frame in bands of 64 rows; lane l owns row 64 band + l and at step s reconstructs pixel x = s - l, so a band takes W + 63 steps.
//   * A pixel is one dword for every C (1, 3 or 4 bytes).  At the top of a step lane l takes lane l - 1's last pixel by ONE cross-lane
//     move (DPP wave_shr:1): that is pixel x of the row above.  What it took one step earlier is pixel x - 1 of the row above (c); its
//     own previous pixel is a.  Before a row starts all three are 0, which is PNG's rule for the neighbours outside the image.
//   * Lane 63's finished pixels are the next band's row above: it leaves them in a hand-over row of one dword per pixel, which lane 0 of
//     the next band reads at step s = x.  Lane 63 writes index s - 63 in the step in which lane 0 reads index s, so ONE row is enough: a
//     position is read before it is overwritten.  The row lives in LDS up to kLdsPixels pixels and in a scratch row in global memory
//     (stream-ordered allocation in the entry point) beyond.
//   * Input: a lane reads its own row front to back through a window of two ALIGNED dwords (v_alignbyte picks the pixel), so rows may
//     start at any byte; a dword that is not wholly inside `rows` is assembled from the bytes that are.
//   * Output: per plane the lane gathers bytes into the aligned dword they belong to and stores it whole; a row's unaligned head and
//     tail go out as bytes.  Dropped channels (alpha with Cout = 3) are reconstructed like the others and not stored.
// A filter type above 4 is treated as 0 (the host has rejected such a file; the kernel only promises not to fault).
#include "common.h"

#include <stdint.h>

namespace {

constexpr int kLanes = 64;
constexpr int kLdsPixels = 4096;      // hand-over row in LDS: 16 KiB; 3840-pixel frames fit

__device__ __forceinline__ uint32_t load_dword(uintptr_t p, uintptr_t lo, uintptr_t hi) {      // p 4-byte aligned; reads inside [lo, hi) only
  if (p >= lo && p + 4 <= hi) return *reinterpret_cast<const uint32_t*>(p);
  uint32_t v = 0;
  for (int j = 0; j < 4; ++j)
    if (p + j >= lo && p + j < hi) v |= (uint32_t) * reinterpret_cast<const uint8_t*>(p + j) << (8 * j);
  return v;
}

// PNG specification 9.2 / 9.4: the predictor of filter `ft` from a (left), b (above), c (above left), added mod 256
__device__ __forceinline__ uint32_t reconstruct(uint32_t ft, int x, int a, int b, int c) {
  const int pa = abs(b - c), pb = abs(a - c), pc = abs(a + b - 2 * c);
  const int paeth = (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);      // ties in the order a, b, c
  const int pred = ft == 1 ? a : ft == 2 ? b : ft == 3 ? ((a + b) >> 1) : ft == 4 ? paeth : 0;
  return (uint32_t)(x + pred) & 255u;
}

// lane l <- lane l - 1 (lane 0 keeps 0): DPP wave_shr:1, one VALU instruction
__device__ __forceinline__ uint32_t from_lane_above(uint32_t v) {
  return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x138, 0xf, 0xf, false);
}

template <int C, bool kLds>
__global__ __launch_bounds__(kLanes) void png_unfilter_kernel(const uint8_t* __restrict__ rows, uint8_t* __restrict__ out,
                                                              uint32_t* hand_global, int H, int W, int Cout) {
  __shared__ uint32_t hand_lds[kLds ? kLdsPixels : 1];
  const int f = blockIdx.x, lane = threadIdx.x;
  const size_t stride = (size_t)W * C + 1;
  const uintptr_t lo = reinterpret_cast<uintptr_t>(rows), hi = lo + (size_t)gridDim.x * (size_t)H * stride;
  uint32_t* hand = kLds ? hand_lds : hand_global + (size_t)f * (size_t)W;
  const size_t plane = (size_t)H * (size_t)W;

  for (int y0 = 0; y0 < H; y0 += kLanes) {
    const int y = y0 + lane;
    const bool active = y < H;
    const uint8_t* rp = rows + ((size_t)f * H + (active ? y : y0)) * stride;
    uint32_t ft = active ? rp[0] : 0;
    if (ft > 4) ft = 0;
    uintptr_t nx = reinterpret_cast<uintptr_t>(rp + 1);
    uint32_t o = (uint32_t)(nx & 3);
    nx &= ~(uintptr_t)3;
    uint32_t q0 = 0, q1 = 0;      // the window: aligned dwords nx - 8 and nx - 4 from here on
    if (active) q0 = load_dword(nx, lo, hi), q1 = load_dword(nx + 4, lo, hi);
    nx += 8;
    uint8_t* op = out + ((size_t)f * Cout * H + (active ? y : y0)) * (size_t)W;      // the row in plane 0
    const uint32_t al = (uint32_t)(reinterpret_cast<uintptr_t>(op) & 3), alp = (uint32_t)(plane & 3);
    uint32_t acc[C];
#pragma unroll
    for (int ch = 0; ch < C; ++ch) acc[ch] = 0;
    uint32_t mine = 0, upleft = 0;
    const int lanes = H - y0 < kLanes ? H - y0 : kLanes;
    const int steps = W + lanes - 1;
    for (int s = 0; s < steps; ++s) {
      const int x = s - lane;
      uint32_t up = from_lane_above(mine);      // pixel x of the row above
      if (lane == 0) up = (y0 > 0 && s < W) ? hand[s] : 0u;
      if (active && x >= 0 && x < W) {
        const uint32_t pix = __builtin_amdgcn_alignbyte(q1, q0, o);
        uint32_t r = 0;
#pragma unroll
        for (int j = 0; j < C; ++j)
          r |= reconstruct(ft, (pix >> (8 * j)) & 255u, (mine >> (8 * j)) & 255u, (up >> (8 * j)) & 255u, (upleft >> (8 * j)) & 255u) << (8 * j);
        mine = r;
        if (lane == kLanes - 1) hand[x] = r;
        o += C;
        if (o >= 4) {
          o -= 4, q0 = q1;
          q1 = load_dword(nx, lo, hi);
          nx += 4;
        }
#pragma unroll
        for (int ch = 0; ch < C; ++ch) {
          if (ch < Cout) {
            uint8_t* orow = op + (size_t)ch * plane;
            const uint32_t ph = (al + alp * ch + (uint32_t)x) & 3u;      // byte of its aligned dword
            acc[ch] |= ((r >> (8 * ch)) & 255u) << (8 * ph);
            if (ph == 3 || x == W - 1) {
              const int n = (int)ph < x ? (int)ph + 1 : x + 1;      // bytes gathered since the last store
              if (n == 4) {
                *reinterpret_cast<uint32_t*>(orow + (x - 3)) = acc[ch];
              } else {
                for (int k = 0; k < n; ++k) orow[x - k] = (uint8_t)(acc[ch] >> (8 * (ph - k)));
              }
              acc[ch] = 0;
            }
          }
        }
      }
      upleft = up;
    }
    __threadfence_block();      // the hand-over row is complete before the next band reads it
    __syncthreads();
  }
}

template <int C>
void launch(const uint8_t* rows, uint8_t* out, uint32_t* scratch, int F, int H, int W, int Cout, hipStream_t st) {
  if (scratch == nullptr)
    hipLaunchKernelGGL((png_unfilter_kernel<C, true>), dim3((unsigned)F), dim3(kLanes), 0, st, rows, out, scratch, H, W, Cout);
  else
    hipLaunchKernelGGL((png_unfilter_kernel<C, false>), dim3((unsigned)F), dim3(kLanes), 0, st, rows, out, scratch, H, W, Cout);
}

}  // namespace

extern "C" int eavsr_png_unfilter_u8(const uint8_t* rows, uint8_t* out, int32_t F, int32_t H, int32_t W, int32_t C, int32_t Cout,
                                     void* stream) {
  EAVSR_REQUIRE(rows && out, -1, "png_unfilter_u8: NULL pointer");
  EAVSR_REQUIRE(C == 1 || C == 3 || C == 4, -2, "png_unfilter_u8: C=%d: grey (1), RGB (3) or RGBA (4)", C);
  EAVSR_REQUIRE(Cout >= 1 && Cout <= C, -2, "png_unfilter_u8: Cout=%d: 1 .. C=%d planes", Cout, C);
  EAVSR_REQUIRE(F >= 0 && H >= 1 && W >= 1, -2, "png_unfilter_u8: bad dims F=%d H=%d W=%d", F, H, W);
  EAVSR_REQUIRE((int64_t)W * C <= 2147483646ll, -2, "png_unfilter_u8: rows of %lld bytes, at most 2^31 - 2", (long long)W * C);
  if (F == 0) return 0;
  hipStream_t st = eavsr::as_stream(stream);
  uint32_t* scratch = nullptr;
  if (W > kLdsPixels) {      // the hand-over row does not fit LDS: one dword per pixel and frame, allocated and freed in stream order
    const hipError_t e = hipMallocAsync(reinterpret_cast<void**>(&scratch), (size_t)F * (size_t)W * sizeof(uint32_t), st);
    EAVSR_REQUIRE(e == hipSuccess && scratch, -3, "png_unfilter_u8: %lld bytes of scratch for rows of %d pixels: %s",
                  (long long)F * W * 4, W, hipGetErrorString(e));
  }
  if (C == 1) launch<1>(rows, out, scratch, F, H, W, Cout, st);
  else if (C == 3) launch<3>(rows, out, scratch, F, H, W, Cout, st);
  else launch<4>(rows, out, scratch, F, H, W, Cout, st);
  const int rc = eavsr::launch_status("png_unfilter_u8");
  if (scratch) (void)hipFreeAsync(scratch, st);
  return rc;
}
