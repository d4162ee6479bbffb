// Training batches from device-resident 8-bit frames: window selection, crop, hflip / vflip / transpose and the `/ 255` conversion of
// the reference's training item (data/realvsr_dataset.py:62-94 `_getitem_train` + `_crop_patch`, util/util.py:223-248
// `augment_basic`) for a whole batch, LR and HR together, as ONE launch.
//
//   lr_store (F, C, h, w) uint8, hr_store (F, C, s h, s w) uint8 (nullable), frames (n, t) int32, desc (n, 4) int32 =
//   (top, left, flags, 0) in LR pixels; flags bit 0 hflip, bit 1 vflip, bit 2 transpose, applied in the reference's order:
//     (r, q) = transposed ? (x, y) : (y, x);  out[c, y, x] = float(crop[c, vflip ? P-1-r : r, hflip ? P-1-q : q]) / 255.0f
//   -> lr_out (n, t, C, ph, pw), hr_out (n, t, C, s ph, s pw) fp32.  The division is the IEEE division of ingest.hip.
//
// `frames` and `desc` are read on the device (the launch is graph-capturable and replays with new indices), so the kernel cannot
// trust them: the frame index is clamped into [0, F), the origin into [0, h-ph] x [0, w-pw], and the transpose bit is dropped
// when ph != pw.  Whatever they hold, no byte outside the stores is read and none outside the outputs written.
//
// A workgroup owns one 32-row x 128-column OUTPUT tile of one (sample, frame, channel) plane, of LR or of HR, and branches
// uniformly on its sample's flags.  A lane owns 4 consecutive samples of one output row: one 16-byte store (scalar stores when
// the patch width is not a multiple of 4: rows then start unaligned).
//   not transposed: the 4 source bytes are one dword cut out of the two aligned dwords around them by a 64-bit shift (`left` is
//     arbitrary, so the source is generally unaligned: 2 loads instead of `load4`'s 4 byte loads); hflip reads the mirrored
//     dword and reverses its bytes, vflip mirrors the row index.
//   transposed: the tile's source bytes (128 source rows x 32 source columns, flips applied on the way in) are staged in LDS with
//     the same coalesced row reads, then read by columns.  LDS row stride 33 BYTES: the lane of output columns 4l..4l+3 reads
//     rows 4l+i at byte (4l + i) * 33 + y = 132 l + const, i.e. dword 33 l + const, bank (l + const) % 32 -- the 32 lanes of a
//     half (one output row) hit 32 distinct banks, 0 conflicts predicted.  (A dword-multiple stride S puts them on 4 l S/4 % 32:
//     at most 8 banks.)  The odd stride costs byte writes on the way in.
#include "pixel.h"

#include <stdint.h>

namespace {

constexpr int kThreads = 256;
constexpr int kTX = 128;           // output columns of a tile
constexpr int kTY = 32;            // output rows of a tile
constexpr int kStride = kTY + 1;   // bytes per LDS row of the transposed path

// bytes j = 0..3 of the result: crop[row][hflip ? pw-1-(c0+j) : c0+j], 0 where c0 + j >= pw.  `row` is the byte offset of the crop
// row's first FRAME column in the store, `left` the crop's first column, `total` the store's size (nothing is read at or past it).
__device__ __forceinline__ uint32_t load_quad(const uint8_t* __restrict__ store, size_t total, size_t row, int left, int c0, int pw,
                                              bool hflip) {
  if (c0 + 4 <= pw) {
    const size_t a = row + (size_t)(left + (hflip ? pw - 4 - c0 : c0));
    const size_t a4 = a & ~(size_t)3;      // the store's base is 4-byte aligned (checked by the entry point)
    uint32_t v;
    if (a4 + 8 <= total) {
      const uint32_t lo = *reinterpret_cast<const uint32_t*>(store + a4);
      const uint32_t hi = *reinterpret_cast<const uint32_t*>(store + a4 + 4);
      v = (uint32_t)((((uint64_t)hi << 32) | lo) >> (8 * (unsigned)(a & 3)));
    } else {                               // the last bytes of the store: a + 3 < total holds, a4 + 7 may not
      v = (uint32_t)store[a] | ((uint32_t)store[a + 1] << 8) | ((uint32_t)store[a + 2] << 16) | ((uint32_t)store[a + 3] << 24);
    }
    return hflip ? __builtin_bswap32(v) : v;
  }
  uint32_t v = 0;
  for (int j = 0; j < 4; ++j)
    if (c0 + j < pw) v |= (uint32_t)store[row + (size_t)(left + (hflip ? pw - 1 - (c0 + j) : c0 + j))] << (8 * j);
  return v;
}

// 4 samples (fewer at the end of a row: `rem` = samples left in the row) to o
__device__ __forceinline__ void store_quad(float* __restrict__ o, uint32_t v, bool vec, int rem) {
  if (vec) {
    *reinterpret_cast<float4*>(o) = make_float4(unit(v & 255u), unit((v >> 8) & 255u), unit((v >> 16) & 255u), unit(v >> 24));
  } else {
    for (int j = 0; j < 4; ++j)
      if (j < rem) o[j] = unit((v >> (8 * j)) & 255u);
  }
}

// grid: x = the plane's LR tiles followed by its HR tiles, y = (sample, frame, channel)
__global__ __launch_bounds__(kThreads) void gather_pairs_kernel(const uint8_t* __restrict__ lr_store, const uint8_t* __restrict__ hr_store,
                                                                const int32_t* __restrict__ frames, const int32_t* __restrict__ desc,
                                                                float* __restrict__ lr_out, float* __restrict__ hr_out, int F, int t, int C,
                                                                int h, int w, int s, int ph, int pw, int lr_tiles_x, int lr_tiles,
                                                                int hr_tiles_x) {
  __shared__ uint8_t tile[kTX * kStride];
  const int plane = blockIdx.y;
  const int c = plane % C, f = (plane / C) % t, smp = plane / (C * t);
  const bool hr = (int)blockIdx.x >= lr_tiles;
  const int sc = hr ? s : 1;
  const uint8_t* __restrict__ store = hr ? hr_store : lr_store;
  const int W = w * sc, H = h * sc, PH = ph * sc, PW = pw * sc;
  const int u = hr ? (int)blockIdx.x - lr_tiles : (int)blockIdx.x, tiles_x = hr ? hr_tiles_x : lr_tiles_x;
  const int X0 = (u % tiles_x) * kTX, Y0 = (u / tiles_x) * kTY;

  const int frame = clampi(frames[smp * t + f], 0, F - 1);
  const int top = clampi(desc[4 * smp], 0, h - ph) * sc, left = clampi(desc[4 * smp + 1], 0, w - pw) * sc;
  int flags = desc[4 * smp + 2];
  if (ph != pw) flags &= 3;      // a transposed patch has the output's shape only when it is square
  const bool hflip = flags & 1, vflip = flags & 2, transposed = flags & 4;

  const size_t total = (size_t)F * C * H * W;
  const size_t plane_off = ((size_t)frame * C + c) * H * W + (size_t)top * W;      // row 0 of the crop, frame column 0
  float* __restrict__ o = (hr ? hr_out : lr_out) + (size_t)plane * PH * PW;
  const bool vec = (PW & 3) == 0;

  if (!transposed) {
    for (int i = threadIdx.x; i < kTY * (kTX / 4); i += kThreads) {
      const int y = Y0 + i / (kTX / 4), x = X0 + 4 * (i % (kTX / 4));
      if (y >= PH || x >= PW) continue;
      const int r = vflip ? PH - 1 - y : y;
      store_quad(o + (size_t)y * PW + x, load_quad(store, total, plane_off + (size_t)r * W, left, x, PW, hflip), vec, PW - x);
    }
    return;
  }
  // transposed (PH == PW): LDS row xl = the source row of output column X0 + xl, LDS column yl = the source column of output row Y0 + yl
  for (int i = threadIdx.x; i < kTX * (kTY / 4); i += kThreads) {
    const int xl = i / (kTY / 4), yl = 4 * (i % (kTY / 4));
    const int x = X0 + xl, y = Y0 + yl;
    if (x >= PW || y >= PH) continue;
    const int r = vflip ? PH - 1 - x : x;
    const uint32_t v = load_quad(store, total, plane_off + (size_t)r * W, left, y, PW, hflip);
    uint8_t* d = tile + xl * kStride + yl;
    d[0] = (uint8_t)v, d[1] = (uint8_t)(v >> 8), d[2] = (uint8_t)(v >> 16), d[3] = (uint8_t)(v >> 24);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < kTY * (kTX / 4); i += kThreads) {      // a 32-lane half = one output row
    const int yl = i / (kTX / 4), xl = 4 * (i % (kTX / 4));
    const int y = Y0 + yl, x = X0 + xl;
    if (y >= PH || x >= PW) continue;
    const uint8_t* q = tile + xl * kStride + yl;      // rows past the patch were not staged; store_quad drops their samples
    const uint32_t v = (uint32_t)q[0] | ((uint32_t)q[kStride] << 8) | ((uint32_t)q[2 * kStride] << 16) | ((uint32_t)q[3 * kStride] << 24);
    store_quad(o + (size_t)y * PW + x, v, vec, PW - x);
  }
}

}  // namespace

extern "C" int eavsr_gather_pairs_u8(const uint8_t* lr_store, const uint8_t* hr_store, const int32_t* frames, const int32_t* desc,
                                     float* lr_out, float* hr_out, int32_t F, int32_t n, int32_t t, int32_t C, int32_t h, int32_t w,
                                     int32_t s, int32_t ph, int32_t pw, void* stream) {
  EAVSR_REQUIRE(lr_store && frames && desc && lr_out, -1, "gather_pairs_u8: NULL pointer");
  EAVSR_REQUIRE(!hr_store == !hr_out, -1, "gather_pairs_u8: hr_store and hr_out are given together or not at all");
  EAVSR_REQUIRE(F >= 1 && n >= 0 && t >= 1 && C >= 1 && h >= 1 && w >= 1 && s >= 1, -2,
                "gather_pairs_u8: bad dims F=%d n=%d t=%d C=%d h=%d w=%d s=%d", F, n, t, C, h, w, s);
  EAVSR_REQUIRE(ph >= 1 && pw >= 1 && ph <= h && pw <= w, -2, "gather_pairs_u8: patch %d x %d does not fit a %d x %d frame", ph, pw, h, w);
  EAVSR_REQUIRE((int64_t)s * h <= 32768 && (int64_t)s * w <= 32768, -2, "gather_pairs_u8: HR frame %lld x %lld is above 32768",
                (long long)s * h, (long long)s * w);
  EAVSR_REQUIRE((int64_t)n * t * C <= 65535, -2, "gather_pairs_u8: n t C = %lld planes, at most 65535 per launch", (long long)n * t * C);
  EAVSR_REQUIRE((((uintptr_t)lr_store) & 3) == 0 && (((uintptr_t)hr_store) & 3) == 0, -2, "gather_pairs_u8: stores must be 4-byte aligned");
  EAVSR_REQUIRE((((uintptr_t)lr_out) & 15) == 0 && (((uintptr_t)hr_out) & 15) == 0, -2, "gather_pairs_u8: outputs must be 16-byte aligned");
  if (n == 0) return 0;
  auto tiles = [](int len, int tile) { return (len + tile - 1) / tile; };
  const int lr_tiles_x = tiles(pw, kTX), lr_tiles = lr_tiles_x * tiles(ph, kTY);
  const int hr_tiles_x = tiles(s * pw, kTX), hr_tiles = hr_store ? hr_tiles_x * tiles(s * ph, kTY) : 0;
  hipLaunchKernelGGL(gather_pairs_kernel, dim3(lr_tiles + hr_tiles, n * t * C), dim3(kThreads), 0, eavsr::as_stream(stream), lr_store,
                     hr_store, frames, desc, lr_out, hr_out, F, t, C, h, w, s, ph, pw, lr_tiles_x, lr_tiles, hr_tiles_x);
  return eavsr::launch_status("gather_pairs_u8");
}
