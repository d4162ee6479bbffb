// LR frames from full-size frames on the device: OpenCV's `cv2.resize(img, (w, h), interpolation=cv2.INTER_CUBIC)` for 8-bit images
// as the reference's loaders call it on every "wide" frame (data/mvsr4x_dataset.py:192-201, data/realvsr_dataset.py:200), for F x C
// planes, as ONE launch.  Integer arithmetic throughout: the result is defined bit for bit.
//
//   in (F, C, H, W) uint8, out (F, C, h, w) uint8; per axis a table built on the HOST (eavsr_amd/dataset.py cubic_tables: the
//   float32 coefficient arithmetic must not be contracted into FMAs, so it is not done here): ofs int32[dst] = floor of the
//   source position, coef int16[dst][4] = the 4 taps in units of 1 / 2048 (their sum is 2047 or 2049 at some positions).
//     hor[y][dx] = sum_j xcoef[dx][j] * in[y][clamp(xofs[dx] - 1 + j, 0, W-1)]                    int32, exact
//     v          = sum_j ycoef[dy][j] * hor[clamp(yofs[dy] - 1 + j, 0, H-1)][dx]                  int32
//     out[dy][dx] = clamp((v + 2^21) >> 22, 0, 255)                                               arithmetic shift: ties round up
//
// The tables are DEVICE memory, so the kernel cannot trust them: every source index is clamped into the plane and then into the
// rectangle the workgroup staged, whose size is bounded by the host from H / h and W / w alone.  Whatever the tables hold, no
// byte outside `in` is read and none outside `out` written; with the tables of cubic_tables the second clamp never acts.
//
// A workgroup of 256 lanes owns a 16-row x 64-column OUTPUT tile of one plane.
//   1. stage: the tile's source rectangle, rows yofs[first] - 1 .. yofs[last] + 2, columns likewise (clamped), goes to LDS as the
//      ALIGNED dwords that cover each row (W is arbitrary, so a row starts at any phase p = address & 3; sample k of LDS row r is
//      byte r * stride + p_r + k).  Consecutive lanes load consecutive dwords.  A dword that begins before `in` or ends after
//      its last byte is assembled from the bytes inside instead.  ds_write_b32 to consecutive dwords: 32 lanes, 32 banks.
//   2. horizontal: one wave per staged row, lane = output column: 4 byte reads at p_r + xofs - 1 + j - x0.  Banks ((a / 4) % 32 per
//      32-lane half): neighbouring lanes are `ratio` bytes apart -- at x4 one dword per lane, 32 distinct banks; at x2 and x3
//      lanes share dwords or take neighbouring ones, no bank twice; at x8 lanes are 2 dwords apart and l, l + 16 meet: 2-way.
//      The int32 sum goes to hor[r][dx], row stride 64 dwords (ds_write_b32, consecutive banks); columns past the tile get 0.
//   3. vertical: lane (yl = lane / 16, q = lane % 16) owns outputs 4q .. 4q + 3 of output row yl: 4 ds_read_b128 of
//      hor[row_j][4q .. 4q + 3].  Banks ((a / 4) % 64 per group of 16 lanes; the groups are {0-3, 12-15, 20-27}, {4-11, 16-19,
//      28-31} and the same + 32): a group's lanes come from two output rows, i.e. from two hor rows, but cover quads {0-3,
//      12-15} of one and {4-11} of the other (or the complement); the row stride is exactly 64 dwords, so whichever rows they
//      are, the 16 lanes hit 64 distinct banks: 0 conflicts predicted.  One 4-byte store per lane when w % 4 == 0 (and `out` is
//      4-byte aligned), byte stores otherwise.
// Nothing but `in`, the tables and `out` touches HBM: 1 B per source sample + 1 B per output sample + the tables through L2.
//
// Addressing: the plane's base offset is size_t; offsets inside a plane are 32-bit (H W <= 2^31 - 1 is required).
// Planes and tiles share grid x: F C tiles <= 2^24 - 1 workgroups (x 256 lanes stays below 2^32 work-items).
#include "pixel.h"

#include <stdint.h>

namespace {

constexpr int kThreads = 256;
constexpr int kTX = 64;               // output columns of a tile = dwords of a hor row
constexpr int kTY = 16;               // output rows of a tile
constexpr int kMaxRatio = 8;
constexpr int kSlack = 7;             // source samples of a tile of T outputs: at most floor(ratio (T - 1)) + 7
constexpr int kMaxNX = kMaxRatio * (kTX - 1) + kSlack, kMaxNY = kMaxRatio * (kTY - 1) + kSlack;
constexpr int kMaxLds = kMaxNY * (((kMaxNX + 6) / 4) * 4 + kTX * 4);      // 98044 bytes at ratio 8 in both axes
constexpr long long kMaxBlocks = (1ll << 24) - 1;

struct Taps {
  int ofs;
  int k[4];
};

__device__ __forceinline__ Taps load_taps(const int32_t* __restrict__ ofs, const int16_t* __restrict__ coef, int d) {
  Taps t;
  t.ofs = ofs[d];
  const int2 c = *reinterpret_cast<const int2*>(coef + 4 * (size_t)d);      // 8-byte aligned (checked by the entry point)
  t.k[0] = (int16_t)(c.x & 0xffff), t.k[1] = c.x >> 16, t.k[2] = (int16_t)(c.y & 0xffff), t.k[3] = c.y >> 16;
  return t;
}

// first and count of the source samples a tile of outputs [d0, d0 + n) reads along one axis of `len` samples, at most `cap`
__device__ __forceinline__ void source_span(const int32_t* __restrict__ ofs, int d0, int n, int len, int cap, int& first, int& count) {
  first = clampi(ofs[d0] - 1, 0, len - 1);
  const int last = clampi(ofs[d0 + n - 1] + 2, 0, len - 1);
  count = clampi(last - first + 1, 1, cap);
}

__global__ __launch_bounds__(kThreads) void resize_cubic_u8_kernel(const uint8_t* __restrict__ in, uint8_t* __restrict__ out,
                                                                   const int32_t* __restrict__ xofs, const int16_t* __restrict__ xcoef,
                                                                   const int32_t* __restrict__ yofs, const int16_t* __restrict__ ycoef,
                                                                   size_t total, int H, int W, int h, int w, int tiles_x, int tiles,
                                                                   int nx_cap, int ny_cap, int vec) {
  extern __shared__ __align__(16) uint8_t lds[];
  const int plane = (int)(blockIdx.x / (unsigned)tiles), tile = (int)(blockIdx.x % (unsigned)tiles);
  const int X0 = (tile % tiles_x) * kTX, Y0 = (tile / tiles_x) * kTY;
  const int tx = min(kTX, w - X0), ty = min(kTY, h - Y0);
  int sx0, nx, sy0, ny;
  source_span(xofs, X0, tx, W, nx_cap, sx0, nx);
  source_span(yofs, Y0, ty, H, ny_cap, sy0, ny);

  const int dw_row = (nx_cap + 6) >> 2;                   // dwords of an LDS byte row: nx_cap samples at any phase 0..3
  int32_t* __restrict__ hor = reinterpret_cast<int32_t*>(lds);                        // [ny_cap][kTX], 16-byte aligned rows
  uint32_t* __restrict__ stage = reinterpret_cast<uint32_t*>(lds + (size_t)ny_cap * kTX * 4);      // [ny_cap][dw_row]
  const uint8_t* __restrict__ src = in + (size_t)plane * H * W;
  const uintptr_t lo = reinterpret_cast<uintptr_t>(in), hi = lo + total;
  const uintptr_t a00 = reinterpret_cast<uintptr_t>(src) + (unsigned)(sy0 * W + sx0);      // the rectangle's first sample

  // 1. stage the aligned dwords that cover samples [sx0, sx0 + nx) of rows [sy0, sy0 + ny)
  for (int i = threadIdx.x; i < ny * dw_row; i += kThreads) {
    const int r = i / dw_row, k = i - r * dw_row;
    const uintptr_t a = a00 + (unsigned)(r * W);
    const uintptr_t q = (a & ~(uintptr_t)3) + 4u * (unsigned)k;
    if (q >= a + (unsigned)nx) continue;                  // past the row's last needed sample
    uint32_t v;
    if (q >= lo && q + 4 <= hi) {
      v = *reinterpret_cast<const uint32_t*>(in + (q - lo));
    } else {                                              // the first / last bytes of `in`: only what lies inside
      v = 0;
      for (int j = 0; j < 4; ++j)
        if (q + j >= lo && q + j < hi) v |= (uint32_t)in[q + j - lo] << (8 * j);
    }
    stage[r * dw_row + k] = v;
  }
  __syncthreads();

  // 2. horizontal pass: lane = output column, wave = staged row
  {
    const int dx = threadIdx.x & (kTX - 1);
    const bool live = dx < tx;
    Taps t = {0, {0, 0, 0, 0}};
    int c[4] = {0, 0, 0, 0};
    if (live) {
      t = load_taps(xofs, xcoef, X0 + dx);
      for (int j = 0; j < 4; ++j) c[j] = clampi(clampi(t.ofs - 1 + j, 0, W - 1) - sx0, 0, nx - 1);
    }
    const uint8_t* __restrict__ bytes = reinterpret_cast<const uint8_t*>(stage);
    for (int r = threadIdx.x / kTX; r < ny; r += kThreads / kTX) {
      const uint8_t* row = bytes + (size_t)r * dw_row * 4 + ((a00 + (unsigned)(r * W)) & 3);
      int acc = 0;
      if (live) acc = t.k[0] * row[c[0]] + t.k[1] * row[c[1]] + t.k[2] * row[c[2]] + t.k[3] * row[c[3]];
      hor[r * kTX + dx] = acc;
    }
  }
  __syncthreads();

  // 3. vertical pass: 4 outputs per lane
  const int yl = threadIdx.x / (kTX / 4), xq = 4 * (threadIdx.x % (kTX / 4));
  if (yl >= ty || xq >= tx) return;
  const Taps t = load_taps(yofs, ycoef, Y0 + yl);
  int v[4] = {0, 0, 0, 0};
  for (int j = 0; j < 4; ++j) {
    const int r = clampi(clampi(t.ofs - 1 + j, 0, H - 1) - sy0, 0, ny - 1);
    const int4 q = *reinterpret_cast<const int4*>(hor + r * kTX + xq);
    v[0] += t.k[j] * q.x, v[1] += t.k[j] * q.y, v[2] += t.k[j] * q.z, v[3] += t.k[j] * q.w;
  }
  uint32_t px[4];
  for (int j = 0; j < 4; ++j) px[j] = (uint32_t)clampi((v[j] + (1 << 21)) >> 22, 0, 255);
  uint8_t* __restrict__ o = out + (size_t)plane * h * w + (unsigned)((Y0 + yl) * w + X0 + xq);
  if (vec) {                                              // w % 4 == 0: tx is a multiple of 4 and every row start is aligned
    *reinterpret_cast<uint32_t*>(o) = px[0] | (px[1] << 8) | (px[2] << 16) | (px[3] << 24);
  } else {
    for (int j = 0; j < 4; ++j)
      if (xq + j < tx) o[j] = (uint8_t)px[j];
  }
}

// the most source samples a tile of T outputs can need: floor(ratio (T - 1)) + kSlack, at most the axis
int span_cap(int src, int dst, int T) {
  const long long need = ((long long)src * (T - 1)) / dst + kSlack;
  return (int)(need < src ? need : src);
}

}  // namespace

extern "C" int eavsr_resize_cubic_u8(const uint8_t* in, uint8_t* out, const int32_t* xofs, const int16_t* xcoef, const int32_t* yofs,
                                     const int16_t* ycoef, int32_t F, int32_t C, int32_t H, int32_t W, int32_t h, int32_t w,
                                     void* stream) {
  EAVSR_REQUIRE(in && out && xofs && xcoef && yofs && ycoef, -1, "resize_cubic_u8: NULL pointer");
  EAVSR_REQUIRE(F >= 0 && C >= 1 && H >= 1 && W >= 1 && h >= 1 && w >= 1, -2, "resize_cubic_u8: bad dims F=%d C=%d H=%d W=%d h=%d w=%d", F,
                C, H, W, h, w);
  EAVSR_REQUIRE(h <= H && w <= W && (int64_t)H <= (int64_t)kMaxRatio * h && (int64_t)W <= (int64_t)kMaxRatio * w, -2,
                "resize_cubic_u8: %d x %d -> %d x %d: the ratio of each axis must be in [1, %d] (no upscaling; the table lengths are h and w)",
                H, W, h, w, kMaxRatio);
  EAVSR_REQUIRE((int64_t)H * W <= 2147483647ll, -2, "resize_cubic_u8: plane of %lld samples, at most 2^31 - 1 (32-bit offsets inside a plane)",
                (long long)H * W);
  EAVSR_REQUIRE((((uintptr_t)xofs | (uintptr_t)yofs) & 3) == 0 && (((uintptr_t)xcoef | (uintptr_t)ycoef) & 7) == 0, -2,
                "resize_cubic_u8: ofs tables must be 4-byte aligned, coef tables 8-byte aligned");
  const int tiles_x = eavsr::cdiv(w, kTX), tiles = tiles_x * eavsr::cdiv(h, kTY);
  const long long blocks = (long long)F * C * tiles;
  EAVSR_REQUIRE(blocks <= kMaxBlocks, -2,
                "resize_cubic_u8: F C = %lld planes x %d tiles = %lld workgroups, at most %lld per launch (grid x: 2^24 - 1 workgroups of 256)",
                (long long)F * C, tiles, blocks, kMaxBlocks);
  if (F == 0) return 0;
  const int nx_cap = span_cap(W, w, kTX), ny_cap = span_cap(H, h, kTY);
  const size_t lds_bytes = (size_t)ny_cap * (kTX * 4 + ((nx_cap + 6) / 4) * 4);

  if (int rc = eavsr::raise_lds<&resize_cubic_u8_kernel>(kMaxLds, "resize_cubic_u8")) return rc;
  const int vec = (w % 4 == 0) && (((uintptr_t)out) & 3) == 0;
  hipLaunchKernelGGL(resize_cubic_u8_kernel, dim3((unsigned)blocks), dim3(kThreads), lds_bytes, eavsr::as_stream(stream), in, out, xofs,
                     xcoef, yofs, ycoef, (size_t)F * C * H * W, H, W, h, w, tiles_x, tiles, nx_cap, ny_cap, vec);
  return eavsr::launch_status("resize_cubic_u8");
}
