// The outgoing PNG file on the device: scanline filters (eavsr_png_filter_u8) and a literal-only dynamic-Huffman deflate coder
// (eavsr_deflate_huffman_u8) that knows nothing of PNG.  Integer arithmetic throughout; no global atomics; two calls on equal input
// write equal bytes.
//
// Filter pass.  in (F, H, W, C) uint8 -> out (F, H, 1 + W C): byte 0 of a row is its filter type, chosen per row by libpng's default
// heuristic: of filters 0 - 4 the one whose filtered bytes, read as signed, have the smallest sum of absolute values; ties go to the
// lowest number.  Every filter reads ORIGINAL pixels only, so rows are independent: one workgroup per row, two passes over the row
// (sums, then the chosen filter); the second pass re-reads what the first left in L1 / L2.  Neighbours outside the image are 0.
//
// Entropy pass.  in (F, nbytes) is cut into stripes of stripe_bytes; one workgroup of 256 lanes codes one stripe:
//   1. histogram + Adler-32 partials, one pass of aligned dword loads (the stripe starts at any phase; the first / last dword is
//      assembled from the bytes inside the stripe).  Per-WAVE sub-histograms in LDS (ds_add_u32: the one place besides the bit packer
//      where an LDS atomic is used; integer sums, so the order does not show).  Adler: per lane sum d and sum ((n - i) mod 65521) d in
//      32 bits, the second folded every 32 dwords (128 terms < 2^24 each), then a wave / workgroup sum.
//   2. the 257 used symbols are ranked by (count, symbol) in parallel (one symbol per lane, 257 comparisons), then lane 0 runs the
//      serial part (csrc/deflate_tables.h): lengths limited to 15 bits, canonical codes, the block header into the LDS bit buffer.
//   3. sizes are now known: header + sum count x length + end-of-block, + the empty stored block that byte-aligns the stripe.  If
//      that is not smaller than the stored form, the stripe is written as stored blocks of at most 65535 bytes instead.
//   4. bit packing in tiles of 1024 bytes: a lane owns 4 consecutive bytes = at most 60 bits; an inclusive scan of the bit counts
//      (6 __shfl_up steps per wave, 4 wave totals through LDS) gives every lane its bit offset; the lane ORs its bits into the
//      tile's LDS buffer of 64-bit words (ds_or_b64, at most two per lane); the complete words then go to global memory with ONE
//      writer per word (64-bit stores, consecutive lanes consecutive words) and the incomplete last word is carried to the next tile.
//   Output goes to a per-stripe slot of the workspace (8-byte aligned, capacity from the shape alone); a scan kernel turns stripe
//   sizes into 64-bit offsets and folds the Adler pairs in stripe order (the adler32_combine identity), and a gather kernel leaves
//   every frame's stream contiguous: 78 01, the stripes, 03 00, Adler-32 big-endian.
#include "common.h"
#include "deflate_tables.h"

#include <stdint.h>

namespace {

namespace D = eavsr_deflate;

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr uint32_t kAdlerMod = 65521;
constexpr int kTileBytes = kThreads * 4;
constexpr int kBufWords = 256;                 // 64-bit words: a carry (< 64 bits) + 1024 codes of at most 15 bits = 241 words; header <= 58
constexpr int64_t kMaxBytes = 2147483647ll;    // per frame: 32-bit offsets inside a frame
constexpr int kMaxFrames = 65535;              // grid y
constexpr int kMaxStripes = 65535;             // per frame: the scan kernel folds the Adler pairs serially
static_assert(D::kMaxHeaderBits + 64 <= kBufWords * 64, "the header must fit the bit buffer");
static_assert(64 + kTileBytes * 15 <= kBufWords * 64, "a tile must fit the bit buffer");

// ------------------------------------------------------------------------------------------------------------------ filter pass
__device__ __forceinline__ uint32_t abs_s8(uint32_t v) {      // |v as a signed byte|, v in 0 .. 255
  return v < 128 ? v : 256 - v;
}

__device__ __forceinline__ void residuals(int x, int a, int b, int c, uint32_t r[5]) {
  const int p = a + b - c, pa = abs(p - a), pb = abs(p - b), pc = abs(p - c);
  const int paeth = (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
  r[0] = (uint32_t)x;
  r[1] = (uint32_t)(x - a) & 255u;
  r[2] = (uint32_t)(x - b) & 255u;
  r[3] = (uint32_t)(x - ((a + b) >> 1)) & 255u;
  r[4] = (uint32_t)(x - paeth) & 255u;
}

__global__ __launch_bounds__(kThreads) void png_filter_kernel(const uint8_t* __restrict__ in, uint8_t* __restrict__ out, int H, int R, int C) {
  __shared__ uint32_t part[kWaves][5];
  const int y = blockIdx.x, f = blockIdx.y;
  const uint8_t* __restrict__ cur = in + ((size_t)f * H + y) * (size_t)R;
  const uint8_t* __restrict__ prev = y > 0 ? cur - R : cur;      // read only where y > 0
  uint8_t* __restrict__ o = out + ((size_t)f * H + y) * ((size_t)R + 1);
  uint32_t sum[5] = {0, 0, 0, 0, 0};
  for (int i = threadIdx.x; i < R; i += kThreads) {
    const int x = cur[i], a = i >= C ? cur[i - C] : 0, b = y > 0 ? prev[i] : 0, c = (y > 0 && i >= C) ? prev[i - C] : 0;
    uint32_t r[5];
    residuals(x, a, b, c, r);
    for (int k = 0; k < 5; ++k) sum[k] += abs_s8(r[k]);      // <= 128 R < 2^32 (R <= 2^24 is required)
  }
  for (int k = 0; k < 5; ++k)
    for (int off = 32; off > 0; off >>= 1) sum[k] += __shfl_xor(sum[k], off);
  if ((threadIdx.x & 63) == 0)
    for (int k = 0; k < 5; ++k) part[threadIdx.x >> 6][k] = sum[k];
  __syncthreads();
  int ft = 0;
  uint32_t best = 0;
  for (int k = 0; k < 5; ++k) {
    uint32_t s = 0;
    for (int w = 0; w < kWaves; ++w) s += part[w][k];
    if (k == 0 || s < best) best = s, ft = k;      // strict: a tie keeps the lower filter number
  }
  if (threadIdx.x == 0) o[0] = (uint8_t)ft;
  for (int i = threadIdx.x; i < R; i += kThreads) {
    const int x = cur[i], a = i >= C ? cur[i - C] : 0, b = y > 0 ? prev[i] : 0, c = (y > 0 && i >= C) ? prev[i - C] : 0;
    uint32_t r[5];
    residuals(x, a, b, c, r);
    o[1 + i] = (uint8_t)(ft == 0 ? r[0] : ft == 1 ? r[1] : ft == 2 ? r[2] : ft == 3 ? r[3] : r[4]);
  }
}

// ----------------------------------------------------------------------------------------------------------------- entropy pass
struct Shape {
  int64_t nbytes, stripe;
  int stripes;           // per frame
  int64_t slot;          // bytes of a stripe's workspace slot: its capacity rounded up to 8
  int64_t frame_cap;     // bytes of a frame's slot in `out`
};

// stored form of n bytes: blocks of at most 65535 bytes, 5 bytes of header each
__host__ __device__ inline int64_t stored_size(int64_t n) { return n + 5 * ((n + 65534) / 65535); }
inline int64_t stripe_capacity(int64_t stripe) { return stored_size(stripe) + 9; }

bool make_shape(int64_t nbytes, int64_t stripe, Shape& s) {
  if (nbytes < 1 || nbytes > kMaxBytes || stripe < 1 || stripe > kMaxBytes) return false;
  const int64_t n = (nbytes + stripe - 1) / stripe;
  if (n > kMaxStripes) return false;
  s.nbytes = nbytes, s.stripe = stripe < nbytes ? stripe : nbytes, s.stripes = (int)n;
  s.slot = (stripe_capacity(s.stripe) + 7) & ~(int64_t)7;
  s.frame_cap = n * stripe_capacity(s.stripe) + 8;      // zlib header 2 + final block 2 + Adler-32 4
  return true;
}

// the 4 bytes of aligned dword k of a stripe that begins `mis` bytes into its first dword: stripe positions 4 k - mis .. + 3; `valid`
// has bit j set where byte j lies inside [0, n).  Only bytes of the stripe are read.
__device__ __forceinline__ uint32_t load4(const uint8_t* __restrict__ p, uint32_t n, uint32_t mis, uint32_t k, int64_t& pos0, uint32_t& valid) {
  pos0 = 4ll * k - mis;
  if (pos0 >= 0 && pos0 + 4 <= (int64_t)n) {
    valid = 15;
    return *reinterpret_cast<const uint32_t*>(p + pos0);
  }
  uint32_t v = 0;
  valid = 0;
  for (int j = 0; j < 4; ++j) {
    const int64_t q = pos0 + j;
    if (q >= 0 && q < (int64_t)n) v |= (uint32_t)p[q] << (8 * j), valid |= 1u << j;
  }
  return v;
}

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return v;
}

struct DeflateLds {
  uint32_t hist[kWaves][256];
  uint32_t freq[D::kLit];
  uint32_t tab[D::kLit];
  uint16_t sorted[D::kLit + 1];
  uint32_t w[2 * D::kLit];
  uint16_t par[2 * D::kLit];
  uint16_t rle[D::kSeq];
  uint8_t lens[D::kLit + 3];
  uint32_t red[2][kWaves];
  uint32_t wtot[kWaves];
  uint32_t hdr_bits;
  int dynamic;
  alignas(8) uint64_t buf[kBufWords];
};

__global__ __launch_bounds__(kThreads) void deflate_stripe_kernel(const uint8_t* __restrict__ in, uint8_t* __restrict__ slots,
                                                                   int64_t* __restrict__ stripe_size, uint2* __restrict__ adler,
                                                                   int64_t nbytes, int64_t stripe, int stripes, int64_t slot) {
  __shared__ DeflateLds L;
  const int s = blockIdx.x, f = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t first = (int64_t)s * stripe;
  const uint32_t n = (uint32_t)(nbytes - first < stripe ? nbytes - first : stripe);      // >= 1
  const uint8_t* __restrict__ p = in + (size_t)f * (size_t)nbytes + (size_t)first;
  const size_t sidx = (size_t)f * stripes + s;
  uint8_t* __restrict__ o = slots + sidx * (size_t)slot;      // 8-byte aligned
  const uint32_t mis = (uint32_t)(reinterpret_cast<uintptr_t>(p) & 3);
  const uint32_t ndw = (mis + n + 3) >> 2;

  for (int i = tid; i < kWaves * 256; i += kThreads) (&L.hist[0][0])[i] = 0;
  for (int i = tid; i < kBufWords; i += kThreads) L.buf[i] = 0;
  for (int i = tid; i < D::kLit + 3; i += kThreads) L.lens[i] = 0;
  __syncthreads();

  // 1. histogram and Adler partials
  uint32_t a1 = 0, a2 = 0, it = 0;
  for (uint32_t k = tid; k < ndw; k += kThreads, ++it) {
    int64_t pos0;
    uint32_t valid;
    const uint32_t v = load4(p, n, mis, k, pos0, valid);
    for (int j = 0; j < 4; ++j) {
      if (!(valid >> j & 1)) continue;
      const uint32_t d = (v >> (8 * j)) & 255u;
      atomicAdd(&L.hist[wave][d], 1u);
      a1 += d;                                                      // <= 4 x 255 per dword, <= 2^21 dwords per lane
      a2 += ((n - (uint32_t)(pos0 + j)) % kAdlerMod) * d;           // each term < 2^24
    }
    if ((it & 31) == 31) a2 %= kAdlerMod;                           // 128 terms between folds: < 2^31 + 2^16
  }
  a1 = wave_sum(a1 % kAdlerMod), a2 = wave_sum(a2 % kAdlerMod);     // 64 values < 2^16
  if (lane == 0) L.red[0][wave] = a1, L.red[1][wave] = a2;
  __syncthreads();
  for (int i = tid; i < D::kLit; i += kThreads)
    L.freq[i] = i < 256 ? L.hist[0][i] + L.hist[1][i] + L.hist[2][i] + L.hist[3][i] : 1u;      // end-of-block occurs once
  if (tid == 0) {
    uint32_t s1 = 0, s2 = 0;
    for (int w = 0; w < kWaves; ++w) s1 += L.red[0][w], s2 += L.red[1][w];
    adler[sidx] = make_uint2(s1 % kAdlerMod, s2 % kAdlerMod);
  }
  __syncthreads();

  // 2. rank the used symbols by (count, symbol); lane 0 builds lengths, codes and the header
  for (int i = tid; i < D::kLit; i += kThreads) {
    const uint32_t fi = L.freq[i];
    if (fi == 0) continue;
    int rank = 0;
    for (int u = 0; u < D::kLit; ++u) {
      const uint32_t fu = L.freq[u];
      rank += (fu != 0 && (fu < fi || (fu == fi && u < i))) ? 1 : 0;
    }
    L.sorted[rank] = (uint16_t)i;
  }
  __syncthreads();
  if (tid == 0) {
    int used = 0;
    for (int i = 0; i < D::kLit; ++i) used += L.freq[i] != 0;
    D::build_lengths(L.freq, L.sorted, used, 15, L.lens, L.w, L.par);
    D::canonical_codes(L.lens, D::kLit, L.tab);
    uint32_t pos = 0;
    D::write_header(L.lens, L.buf, pos, L.rle, L.w, L.par);
    uint64_t bits = pos;
    for (int i = 0; i < D::kLit; ++i) bits += (uint64_t)L.freq[i] * L.lens[i];
    const uint64_t dyn = (bits + 3 + 7) / 8 + 4;      // + `000`, pad to a byte, 00 00 FF FF
    const uint64_t stored = (uint64_t)stored_size(n);
    L.hdr_bits = pos;
    L.dynamic = dyn < stored;
    stripe_size[sidx] = (int64_t)(dyn < stored ? dyn : stored);
  }
  __syncthreads();

  // 3. the stored form: incompressible data
  if (!L.dynamic) {
    const uint32_t blocks = (n + 65534u) / 65535u;
    for (uint32_t b = tid; b < blocks; b += kThreads) {
      const uint32_t len = b + 1 < blocks ? 65535u : n - b * 65535u;
      uint8_t* h = o + (size_t)b * 65540u;
      h[0] = 0, h[1] = (uint8_t)(len & 255), h[2] = (uint8_t)(len >> 8), h[3] = (uint8_t)(~len & 255), h[4] = (uint8_t)((~len >> 8) & 255);
    }
    for (uint32_t i = tid; i < n; i += kThreads) o[(size_t)i + 5u * (i / 65535u + 1u)] = p[i];
    return;
  }

  // 4. bit packing, one tile of 1024 bytes at a time
  uint64_t* __restrict__ o64 = reinterpret_cast<uint64_t*>(o);
  uint32_t carry = L.hdr_bits, outw = 0;      // bits waiting in buf from bit 0 on; 64-bit words already written
  auto flush = [&](bool all) {                // workgroup-uniform; buf is complete on entry (after a barrier)
    const uint32_t nfull = all ? (carry + 63) >> 6 : carry >> 6;
    for (uint32_t i = tid; i < nfull; i += kThreads) o64[outw + i] = L.buf[i];
    const uint64_t last = (!all && nfull < kBufWords) ? L.buf[nfull] : 0;
    __syncthreads();
    for (uint32_t i = tid; i <= nfull && i < kBufWords; i += kThreads) L.buf[i] = i == 0 ? last : 0;
    outw += nfull, carry = all ? 0 : carry & 63;
    __syncthreads();
  };
  flush(false);
  const uint32_t tiles = (ndw + kThreads - 1) / kThreads;
  for (uint32_t t = 0; t < tiles; ++t) {
    const uint32_t k = t * kThreads + tid;
    uint64_t bits = 0;
    uint32_t nb = 0;
    if (k < ndw) {
      int64_t pos0;
      uint32_t valid;
      const uint32_t v = load4(p, n, mis, k, pos0, valid);
      for (int j = 0; j < 4; ++j) {
        if (!(valid >> j & 1)) continue;
        const uint32_t e = L.tab[(v >> (8 * j)) & 255u];
        bits |= (uint64_t)(e & 0xffffu) << nb;
        nb += e >> 16;
      }
    }
    uint32_t incl = nb;
    for (int off = 1; off < 64; off <<= 1) {
      const uint32_t up = __shfl_up(incl, off);
      if (lane >= off) incl += up;
    }
    if (lane == 63) L.wtot[wave] = incl;
    __syncthreads();
    uint32_t base = carry, total = carry;
    for (int w = 0; w < kWaves; ++w) {
      const uint32_t wt = L.wtot[w];
      base += w < wave ? wt : 0;
      total += wt;
    }
    const uint32_t pos = base + incl - nb, sh = pos & 63;
    if (nb) {
      atomicOr(reinterpret_cast<unsigned long long*>(&L.buf[pos >> 6]), (unsigned long long)(bits << sh));
      if (sh + nb > 64) atomicOr(reinterpret_cast<unsigned long long*>(&L.buf[(pos >> 6) + 1]), (unsigned long long)(bits >> (64 - sh)));
    }
    __syncthreads();
    carry = total;
    flush(false);
  }
  if (tid == 0) {      // end-of-block, the empty stored block `000` + pad + 00 00 FF FF
    uint32_t pos = carry;
    const uint32_t e = L.tab[256];
    D::put_bits(L.buf, pos, e & 0xffffu, (int)(e >> 16));
    pos = (pos + 3 + 7) & ~7u;
    D::put_bits(L.buf, pos, 0xFFFF0000u, 32);
    L.hdr_bits = pos;
  }
  __syncthreads();
  carry = L.hdr_bits;
  flush(true);
}

// per frame: exclusive scan of the stripe sizes (offsets inside the frame's stream, after the 2-byte zlib header), the frame's size,
// and the Adler-32 of the frame from the stripes' pairs in stripe order: a' = a + s1, b' = b + n a + s2 (mod 65521)
__global__ __launch_bounds__(kThreads) void deflate_scan_kernel(const int64_t* __restrict__ stripe_size, const uint2* __restrict__ adler,
                                                                 int64_t* __restrict__ stripe_off, int64_t* __restrict__ offsets,
                                                                 int64_t* __restrict__ sizes, uint32_t* __restrict__ frame_adler,
                                                                 int64_t nbytes, int64_t stripe, int stripes, int64_t frame_cap) {
  __shared__ int64_t part[kThreads];
  const int f = blockIdx.x, tid = threadIdx.x;
  const int per = (stripes + kThreads - 1) / kThreads, lo = min(tid * per, stripes), hi = min(lo + per, stripes);
  const int64_t* __restrict__ sz = stripe_size + (size_t)f * stripes;
  int64_t sum = 0;
  for (int i = lo; i < hi; ++i) sum += sz[i];
  part[tid] = sum;
  __syncthreads();
  int64_t run = 2;
  for (int i = 0; i < tid; ++i) run += part[i];
  for (int i = lo; i < hi; ++i) {
    stripe_off[(size_t)f * stripes + i] = run;
    run += sz[i];
  }
  if (tid == kThreads - 1) {
    offsets[f] = (int64_t)f * frame_cap;
    sizes[f] = run + 6;      // + 03 00 + Adler-32
    uint32_t a = 1, b = 0;
    for (int i = 0; i < stripes; ++i) {
      const int64_t first = (int64_t)i * stripe;
      const uint32_t n = (uint32_t)(nbytes - first < stripe ? nbytes - first : stripe);
      const uint2 pr = adler[(size_t)f * stripes + i];
      b = (uint32_t)(((uint64_t)b + (uint64_t)(n % kAdlerMod) * a + pr.y) % kAdlerMod);
      a = (a + pr.x) % kAdlerMod;
    }
    frame_adler[f] = (b << 16) | a;
  }
}

// a frame's stream, contiguous in its slot of `out`: 78 01 | stripes | 03 00 | Adler-32 big-endian
__global__ __launch_bounds__(kThreads) void deflate_gather_kernel(const uint8_t* __restrict__ slots, const int64_t* __restrict__ stripe_size,
                                                                   const int64_t* __restrict__ stripe_off, const uint32_t* __restrict__ frame_adler,
                                                                   uint8_t* __restrict__ out, int stripes, int64_t slot, int64_t frame_cap) {
  const int s = blockIdx.x, f = blockIdx.y, tid = threadIdx.x;
  const size_t sidx = (size_t)f * stripes + s;
  const int64_t n = stripe_size[sidx], off = stripe_off[sidx];
  uint8_t* __restrict__ dst = out + (size_t)f * (size_t)frame_cap;
  const uint8_t* __restrict__ src = slots + sidx * (size_t)slot;
  for (int64_t i = tid; i < n; i += kThreads) dst[off + i] = src[i];
  if (s == 0 && tid == 0) dst[0] = 0x78, dst[1] = 0x01;      // deflate, 32 KiB window, no dictionary, fastest: 0x7801 % 31 == 0
  if (s == stripes - 1 && tid == 0) {
    const uint32_t ad = frame_adler[f];
    uint8_t* t = dst + off + n;
    t[0] = 0x03, t[1] = 0x00;      // final block: fixed Huffman, end-of-block at once
    t[2] = (uint8_t)(ad >> 24), t[3] = (uint8_t)(ad >> 16), t[4] = (uint8_t)(ad >> 8), t[5] = (uint8_t)ad;
  }
}

// workspace: [stripe sizes int64][stripe offsets int64][Adler pairs 2 x uint32][frame Adler uint32, padded to 8][stripe slots]
int64_t table_bytes(int64_t F, const Shape& s) { return F * s.stripes * 24 + ((F * 4 + 7) & ~(int64_t)7); }

}  // namespace

extern "C" int64_t eavsr_png_capacity(int64_t nbytes, int64_t stripe_bytes) {
  Shape s;
  if (!make_shape(nbytes, stripe_bytes, s)) {
    eavsr::set_error("png_capacity: nbytes=%lld stripe_bytes=%lld: 1 .. 2^31 - 1 bytes per frame, stripes of 1 .. 2^31 - 1 bytes, at most %d stripes",
                     (long long)nbytes, (long long)stripe_bytes, kMaxStripes);
    return -2;
  }
  return s.frame_cap;
}

extern "C" int64_t eavsr_deflate_workspace_bytes(int32_t F, int64_t nbytes, int64_t stripe_bytes) {
  Shape s;
  if (F < 0 || F > kMaxFrames || !make_shape(nbytes, stripe_bytes, s)) {
    eavsr::set_error("deflate_workspace_bytes: F=%d nbytes=%lld stripe_bytes=%lld out of range", F, (long long)nbytes, (long long)stripe_bytes);
    return -2;
  }
  return table_bytes(F, s) + (int64_t)F * s.stripes * s.slot;
}

extern "C" int eavsr_png_filter_u8(const uint8_t* in, uint8_t* out, int32_t F, int32_t H, int32_t W, int32_t C, void* stream) {
  EAVSR_REQUIRE(in && out, -1, "png_filter_u8: NULL pointer");
  EAVSR_REQUIRE(C == 1 || C == 3, -2, "png_filter_u8: C=%d: grey (1) or RGB (3)", C);
  EAVSR_REQUIRE(F >= 0 && H >= 1 && W >= 1, -2, "png_filter_u8: bad dims F=%d H=%d W=%d", F, H, W);
  EAVSR_REQUIRE(F <= kMaxFrames, -2, "png_filter_u8: F=%d frames, at most %d per launch (grid y)", F, kMaxFrames);
  EAVSR_REQUIRE((int64_t)W * C <= (1 << 24), -2, "png_filter_u8: rows of %lld bytes, at most 2^24 (32-bit sums of the heuristic)", (long long)W * C);
  EAVSR_REQUIRE((int64_t)H * ((int64_t)W * C + 1) <= kMaxBytes, -2,
                "png_filter_u8: H (W C + 1) = %lld bytes per frame, at most 2^31 - 1", (long long)H * ((long long)W * C + 1));
  if (F == 0) return 0;
  hipLaunchKernelGGL(png_filter_kernel, dim3((unsigned)H, (unsigned)F), dim3(kThreads), 0, eavsr::as_stream(stream), in, out, H, W * C, C);
  return eavsr::launch_status("png_filter_u8");
}

extern "C" int eavsr_deflate_huffman_u8(const uint8_t* in, uint8_t* out, int64_t* offsets, int64_t* sizes, void* workspace, int32_t F,
                                        int64_t nbytes, int64_t stripe_bytes, void* stream) {
  EAVSR_REQUIRE(in && out && offsets && sizes && workspace, -1, "deflate_huffman_u8: NULL pointer");
  EAVSR_REQUIRE(F >= 0 && F <= kMaxFrames, -2, "deflate_huffman_u8: F=%d frames, 0 .. %d per launch (grid y)", F, kMaxFrames);
  Shape s;
  EAVSR_REQUIRE(make_shape(nbytes, stripe_bytes, s), -2,
                "deflate_huffman_u8: nbytes=%lld stripe_bytes=%lld: 1 .. 2^31 - 1 bytes per frame, stripes of 1 .. 2^31 - 1 bytes, at most %d stripes",
                (long long)nbytes, (long long)stripe_bytes, kMaxStripes);
  EAVSR_REQUIRE((((uintptr_t)workspace | (uintptr_t)offsets | (uintptr_t)sizes) & 7) == 0, -2,
                "deflate_huffman_u8: workspace, offsets and sizes must be 8-byte aligned");
  if (F == 0) return 0;
  const size_t ns = (size_t)F * s.stripes;
  uint8_t* ws = static_cast<uint8_t*>(workspace);
  int64_t* stripe_size = reinterpret_cast<int64_t*>(ws);
  int64_t* stripe_off = stripe_size + ns;
  uint2* adler = reinterpret_cast<uint2*>(stripe_off + ns);
  uint32_t* frame_adler = reinterpret_cast<uint32_t*>(adler + ns);
  uint8_t* slots = ws + table_bytes(F, s);
  hipStream_t st = eavsr::as_stream(stream);
  const dim3 grid((unsigned)s.stripes, (unsigned)F);
  hipLaunchKernelGGL(deflate_stripe_kernel, grid, dim3(kThreads), 0, st, in, slots, stripe_size, adler, s.nbytes, s.stripe, s.stripes, s.slot);
  int rc = eavsr::launch_status("deflate_huffman_u8 (stripes)");
  if (rc) return rc;
  hipLaunchKernelGGL(deflate_scan_kernel, dim3((unsigned)F), dim3(kThreads), 0, st, stripe_size, adler, stripe_off, offsets, sizes, frame_adler,
                     s.nbytes, s.stripe, s.stripes, s.frame_cap);
  rc = eavsr::launch_status("deflate_huffman_u8 (scan)");
  if (rc) return rc;
  hipLaunchKernelGGL(deflate_gather_kernel, grid, dim3(kThreads), 0, st, slots, stripe_size, stripe_off, frame_adler, out, s.stripes, s.slot,
                     s.frame_cap);
  return eavsr::launch_status("deflate_huffman_u8 (gather)");
}
