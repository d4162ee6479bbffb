// 8-bit ingest: uint8 frames -> fp32 planes in [0, 1], the device counterpart of the reference's `np.float32(img) / 255`
// (data/mvsr4x_dataset.py reads 8-bit images and divides on the host; four times the bytes then cross the link).
//
// Every sample is float(v) / 255.0f as an IEEE division (NOT a multiplication by the rounded reciprocal: 1 / 255 is not a binary
// fraction, and v * (1.0f / 255.0f) differs from v / 255.0f in the last bit for some byte values).  The build has no fast-math /
// reciprocal-math flag, so the compiler emits the correctly rounded sequence (v_div_scale / v_div_fmas / v_div_fixup).
//
// Pure streaming: 1 byte read, 4 bytes written per sample.  A lane owns 4 consecutive samples of one output plane: one 32-bit
// load where the source is 4-byte aligned (byte loads otherwise), one 16-byte store.
//   CHW source (F, C, h, w): the layout does not change, so the whole tensor is one flat run of samples.
//   HWC source (F, h, w, 3): a lane reads the 12 bytes of 4 pixels and stores one float4 into each of the three planes; needs
//     h * w % 4 == 0 for the planes to start 16-byte aligned, a scalar kernel covers the rest.
#include "pixel.h"

#include <stdint.h>

namespace {

constexpr int kThreads = 256;

__device__ __forceinline__ float4 unit4(uint32_t word) {
  return make_float4(unit(word & 255u), unit((word >> 8) & 255u), unit((word >> 16) & 255u), unit(word >> 24));
}

__device__ __forceinline__ uint32_t load4(const uint8_t* p, bool aligned) {
  if (aligned) return *reinterpret_cast<const uint32_t*>(p);
  return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}

// flat: out[i] = in[i] / 255 for i < total; quads = total / 4 float4 stores, the last total % 4 samples by the first lanes
__global__ __launch_bounds__(kThreads) void u8_to_f32_flat_kernel(const uint8_t* __restrict__ in, float* __restrict__ out, size_t total,
                                                                  bool aligned) {
  const size_t quads = total / 4;
  const size_t stride = (size_t)gridDim.x * kThreads;
  const size_t first = (size_t)blockIdx.x * kThreads + threadIdx.x;
  for (size_t q = first; q < quads; q += stride) reinterpret_cast<float4*>(out)[q] = unit4(load4(in + 4 * q, aligned));
  const size_t tail = 4 * quads + first;
  if (first < 4 && tail < total) out[tail] = unit(in[tail]);
}

// interleaved: in (F, hw, 3) -> out (F, 3, hw); hw % 4 == 0; blockIdx.y = frame
__global__ __launch_bounds__(kThreads) void u8_hwc_to_f32_kernel(const uint8_t* __restrict__ in, float* __restrict__ out, size_t hw,
                                                                 bool aligned) {
  const size_t f = blockIdx.y;
  const uint8_t* src = in + f * hw * 3;
  float* dst = out + f * hw * 3;
  const size_t quads = hw / 4;
  for (size_t q = (size_t)blockIdx.x * kThreads + threadIdx.x; q < quads; q += (size_t)gridDim.x * kThreads) {
    const uint32_t a = load4(src + 12 * q, aligned), b = load4(src + 12 * q + 4, aligned), c = load4(src + 12 * q + 8, aligned);
    // bytes r0 g0 b0 r1 | g1 b1 r2 g2 | b2 r3 g3 b3
    const float4 r = make_float4(unit(a & 255u), unit(a >> 24), unit((b >> 16) & 255u), unit((c >> 8) & 255u));
    const float4 g = make_float4(unit((a >> 8) & 255u), unit(b & 255u), unit(b >> 24), unit((c >> 16) & 255u));
    const float4 bl = make_float4(unit((a >> 16) & 255u), unit((b >> 8) & 255u), unit(c & 255u), unit(c >> 24));
    reinterpret_cast<float4*>(dst)[q] = r;
    reinterpret_cast<float4*>(dst + hw)[q] = g;
    reinterpret_cast<float4*>(dst + 2 * hw)[q] = bl;
  }
}

// interleaved, any hw: one lane per pixel, scalar stores
__global__ __launch_bounds__(kThreads) void u8_hwc_to_f32_scalar_kernel(const uint8_t* __restrict__ in, float* __restrict__ out, size_t hw) {
  const size_t f = blockIdx.y;
  const uint8_t* src = in + f * hw * 3;
  float* dst = out + f * hw * 3;
  for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i < hw; i += (size_t)gridDim.x * kThreads)
    for (int c = 0; c < 3; ++c) dst[c * hw + i] = unit(src[3 * i + c]);
}

unsigned blocks_for(size_t items) {
  size_t b = (items + kThreads - 1) / kThreads;
  // 256 CUs x 8 workgroups of 4 waves: enough in flight to cover HBM latency; the rest is the grid-stride loop
  return (unsigned)(b < 1 ? 1 : b > 2048 ? 2048 : b);
}

}  // namespace

extern "C" int eavsr_u8_to_f32(const uint8_t* in, float* out, int32_t F, int32_t C, int32_t H, int32_t W, int32_t hwc, void* stream) {
  EAVSR_REQUIRE(in && out, -1, "u8_to_f32: NULL pointer");
  EAVSR_REQUIRE(F >= 0 && F <= 65535 && C >= 1 && H >= 1 && W >= 1, -2, "u8_to_f32: bad dims F=%d C=%d H=%d W=%d", F, C, H, W);
  EAVSR_REQUIRE(hwc == 0 || hwc == 1, -2, "u8_to_f32: hwc %d (0 = planes (F, C, H, W), 1 = interleaved (F, H, W, 3))", hwc);
  EAVSR_REQUIRE(!hwc || C == 3, -2, "u8_to_f32: an interleaved source has 3 channels, got C=%d", C);
  EAVSR_REQUIRE((((uintptr_t)out) & 15) == 0, -2, "u8_to_f32: out must be 16-byte aligned");
  if (F == 0) return 0;
  hipStream_t st = eavsr::as_stream(stream);
  const bool aligned = (((uintptr_t)in) & 3) == 0;
  const size_t hw = (size_t)H * W;
  if (!hwc) {
    const size_t total = (size_t)F * C * hw;
    hipLaunchKernelGGL(u8_to_f32_flat_kernel, dim3(blocks_for(total / 4)), dim3(kThreads), 0, st, in, out, total, aligned);
  } else if (hw % 4 == 0) {
    hipLaunchKernelGGL(u8_hwc_to_f32_kernel, dim3(blocks_for(hw / 4), F), dim3(kThreads), 0, st, in, out, hw, aligned);
  } else {
    hipLaunchKernelGGL(u8_hwc_to_f32_scalar_kernel, dim3(blocks_for(hw), F), dim3(kThreads), 0, st, in, out, hw);
  }
  return eavsr::launch_status("u8_to_f32");
}
