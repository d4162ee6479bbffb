// The 16-bit feature cache of the long-clip path: fp32 features are rounded to fp16 or bf16 when they enter the frame
// store (`framestore.py`) and widened when they leave it.  Two streaming kernels, each over a LIST of contiguous segments in one
// launch (everything a time step of `propagate` fetches is widened together); no compute kernel reads 16 bits.
//
// pack16   -- dst16[i] = round(src32[i]), to nearest even.  fp16: the hardware convert (v_cvt_f16_f32 under the default mode:
//             overflow to +-inf from 65520 on, subnormals produced, NaN quieted).  bf16: in integer arithmetic,
//             (u + 0x7FFF + ((u >> 16) & 1)) >> 16, a NaN written as 0x7FC0 as torch writes it.  +-0 keep their sign.
// unpack16 -- dst32[i] = src16[i], exact (fp16: v_cvt_f32_f16, subnormals included; bf16: the 16 bits moved up).
//
// A segment of n elements is cut by its 16-BIT side's address: `head` scalar elements up to the next 16-byte boundary there (0 .. 7),
// then vectors of 8 elements -- one 16-byte access on the 16-bit side, two on the fp32 side -- then a scalar tail (0 .. 7).  The fp32
// side of a vector is read / written by 16-, 8- or 4-byte accesses, by what its address past the head is aligned to (uniform over
// the segment, as blend.hip's rows).  An ITEM is one vector or one scalar element, one lane each; a workgroup of 256 lanes takes
// kUnroll x 256 consecutive items of one segment: vectors first, then head and tail elements.  Which segment a workgroup serves
// comes from the prefix sums of the segments' workgroup counts in the kernel arguments (pointers and extents by value, at most
// EAVSR_CACHE16_MAX_SEGMENTS; a longer list is split on the host).  Every extent is 64-bit.  The grid is capped at 2048 workgroups,
// the rest is a grid stride.  pack16 and unpack16: No LDS, no atomics.
//
// pack16_census -- pack16 (the same segment table, cut, accesses and 16-bit result: one body, `pack_passes`, with a compile-time
//             switch) that also counts what the rounding did into a record of five 64-bit words: the largest finite |x|, the
//             non-finite inputs, the overflows to +-inf, the flushes to +-0 and the subnormal results.  The definitions, the lane's
//             registers and the one reduction per workgroup (cross-lane moves, a few words of LDS, one update per non-zero slot) are
//             cache16_census.h's; with the switch off nothing of it is compiled and pack16 is the kernel it was.
#include "pixel.h"
#include "cache16_census.h"
#include "round16.h"

#include <stdint.h>

namespace {

constexpr int kMaxSeg = EAVSR_CACHE16_MAX_SEGMENTS;
constexpr int kThreads = 256;
constexpr int kUnroll = 4;                                 // items per lane and workgroup pass: 8 x 16-byte fp32 accesses in flight
constexpr int64_t kBlockItems = (int64_t)kThreads * kUnroll;
constexpr int kGridCap = 2048;                             // 256 CUs x 8 workgroups of 4 waves

struct Segments {
  const void* src[kMaxSeg];
  void* dst[kMaxSeg];
  int64_t n[kMaxSeg];               // elements
  int64_t first_block[kMaxSeg + 1]; // prefix sums of the segments' workgroup passes
  int32_t nseg;
};

// the cut of a segment whose 16-bit side starts at `p16`: [0, head) scalar, nvec vectors from head on, then n - head - 8 nvec scalar
struct Cut {
  int64_t head, nvec, items;
};

__host__ __device__ inline Cut cut_of(const void* p16, int64_t n) {
  int64_t head = (int64_t)((8 - (((uintptr_t)p16 >> 1) & 7)) & 7);
  if (head > n) head = n;
  const int64_t nvec = (n - head) >> 3;
  return Cut{head, nvec, n - 7 * nvec};      // nvec vectors + (n - 8 nvec) scalar elements
}

using round16_ns::round16;      // (round16.h: shared with the range census of the 16-bit backbone, range16.hip)
using round16_ns::widen16;

// where scalar item j (0 <= j < n - 8 nvec) of a segment lies: the head's elements, then the tail's
__device__ __forceinline__ int64_t scalar_index(int64_t j, const Cut& c) { return j < c.head ? j : j + 8 * c.nvec; }

// round16, and with CENSUS the element's entry in the lane's tally
template <int BF16, int CENSUS>
__device__ __forceinline__ uint32_t round_count(float x, census16::Tally& tally) {
  const uint32_t o = round16<BF16>(x);
  if (CENSUS) tally.count<BF16>(__float_as_uint(x), o);
  return o;
}

template <int BF16, int CENSUS>
__device__ __forceinline__ uint32_t round_pair(float lo, float hi, census16::Tally& tally) {
  return round_count<BF16, CENSUS>(lo, tally) | (round_count<BF16, CENSUS>(hi, tally) << 16);
}

// every pass of one workgroup: the body of both pack kernels (CENSUS 0: `tally` is never touched)
template <int BF16, int CENSUS>
__device__ __forceinline__ void pack_passes(const Segments& g, int64_t total_blocks, census16::Tally& tally) {
  for (int64_t blk = blockIdx.x; blk < total_blocks; blk += gridDim.x) {
    int s = 0;
    while (s + 1 < g.nseg && blk >= g.first_block[s + 1]) ++s;      // uniform: the segment of this pass
    const float* src = reinterpret_cast<const float*>(g.src[s]);
    uint16_t* dst = reinterpret_cast<uint16_t*>(g.dst[s]);
    const int64_t n = g.n[s];
    const Cut c = cut_of(dst, n);
    const int align = align_of(src + c.head);
    const int64_t base = (blk - g.first_block[s]) * kBlockItems + threadIdx.x;
    float4 a[kUnroll], b[kUnroll];
#pragma unroll
    for (int j = 0; j < kUnroll; ++j) {      // every load of the pass before its first store
      const int64_t i = base + (int64_t)j * kThreads;
      if (i < c.nvec) {
        const float* p = src + c.head + 8 * i;
        a[j] = load_quad(p, align);
        b[j] = load_quad(p + 4, align);
      }
    }
#pragma unroll
    for (int j = 0; j < kUnroll; ++j) {
      const int64_t i = base + (int64_t)j * kThreads;
      if (i < c.nvec) {
        uint4 v;
        v.x = round_pair<BF16, CENSUS>(a[j].x, a[j].y, tally);
        v.y = round_pair<BF16, CENSUS>(a[j].z, a[j].w, tally);
        v.z = round_pair<BF16, CENSUS>(b[j].x, b[j].y, tally);
        v.w = round_pair<BF16, CENSUS>(b[j].z, b[j].w, tally);
        *reinterpret_cast<uint4*>(dst + c.head + 8 * i) = v;      // 16-byte aligned: what the head is for
      } else if (i < c.items) {
        const int64_t e = scalar_index(i - c.nvec, c);
        dst[e] = (uint16_t)round_count<BF16, CENSUS>(src[e], tally);
      }
    }
  }
}

template <int BF16>
__global__ __launch_bounds__(kThreads) void pack16_kernel(Segments g, int64_t total_blocks) {
  census16::Tally unused;
  pack_passes<BF16, 0>(g, total_blocks, unused);
}

// pack16 + the census: `record` is five 64-bit words in device memory that the kernel adds into (the caller zeroes them)
template <int BF16>
__global__ __launch_bounds__(kThreads) void pack16_census_kernel(Segments g, int64_t total_blocks, unsigned long long* record) {
  static_assert(kThreads == 64 * census16::kWaves, "the census reduction is written for this workgroup");
  census16::Tally tally;
  tally.clear();
  pack_passes<BF16, 1>(g, total_blocks, tally);
  tally.commit(record);      // every lane, after the grid stride: a workgroup without a pass adds nothing
}

template <int BF16>
__global__ __launch_bounds__(kThreads) void unpack16_kernel(Segments g, int64_t total_blocks) {
  for (int64_t blk = blockIdx.x; blk < total_blocks; blk += gridDim.x) {
    int s = 0;
    while (s + 1 < g.nseg && blk >= g.first_block[s + 1]) ++s;
    const uint16_t* src = reinterpret_cast<const uint16_t*>(g.src[s]);
    float* dst = reinterpret_cast<float*>(g.dst[s]);
    const int64_t n = g.n[s];
    const Cut c = cut_of(src, n);
    const int align = align_of(dst + c.head);
    const int64_t base = (blk - g.first_block[s]) * kBlockItems + threadIdx.x;
    uint4 v[kUnroll];
#pragma unroll
    for (int j = 0; j < kUnroll; ++j) {
      const int64_t i = base + (int64_t)j * kThreads;
      if (i < c.nvec) v[j] = *reinterpret_cast<const uint4*>(src + c.head + 8 * i);
    }
#pragma unroll
    for (int j = 0; j < kUnroll; ++j) {
      const int64_t i = base + (int64_t)j * kThreads;
      if (i < c.nvec) {
        float* p = dst + c.head + 8 * i;
        store_quad(p, align, make_float4(widen16<BF16>(v[j].x & 0xFFFFu), widen16<BF16>(v[j].x >> 16), widen16<BF16>(v[j].y & 0xFFFFu),
                                         widen16<BF16>(v[j].y >> 16)));
        store_quad(p + 4, align, make_float4(widen16<BF16>(v[j].z & 0xFFFFu), widen16<BF16>(v[j].z >> 16), widen16<BF16>(v[j].w & 0xFFFFu),
                                             widen16<BF16>(v[j].w >> 16)));
      } else if (i < c.items) {
        const int64_t e = scalar_index(i - c.nvec, c);
        dst[e] = widen16<BF16>(src[e]);
      }
    }
  }
}

// the checked segment table of both entry points; `side16`: which list holds the 16-bit pointers (0: src, 1: dst)
int fill(const char* who, const void* const* src_list, void* const* dst_list, const int64_t* n_list, int32_t nseg, int32_t dtype, int side16,
         Segments& g, int64_t& total) {
  EAVSR_REQUIRE(nseg >= 0 && nseg <= kMaxSeg, -1, "%s: %d segments (0..%d)", who, nseg, kMaxSeg);
  EAVSR_REQUIRE(dtype == EAVSR_CACHE16_FP16 || dtype == EAVSR_CACHE16_BF16, -2, "%s: dtype %d (0: fp16, 1: bf16)", who, dtype);
  EAVSR_REQUIRE(nseg == 0 || (src_list && dst_list && n_list), -1, "%s: NULL list", who);
  total = 0;
  g.nseg = nseg;
  for (int s = 0; s < kMaxSeg; ++s) {
    g.first_block[s] = total;
    g.src[s] = nullptr, g.dst[s] = nullptr, g.n[s] = 0;
    if (s >= nseg) continue;
    const int64_t n = n_list[s];
    EAVSR_REQUIRE(n >= 0 && n < (int64_t(1) << 60), -2, "%s: segment %d has %lld elements", who, s, (long long)n);
    if (n == 0) continue;      // an empty segment: no pass, its pointers are never read
    const void* p16 = side16 ? (const void*)dst_list[s] : src_list[s];
    const void* p32 = side16 ? src_list[s] : (const void*)dst_list[s];
    EAVSR_REQUIRE(p16 && p32, -1, "%s: segment %d: NULL pointer", who, s);
    EAVSR_REQUIRE(((uintptr_t)p16 & 1) == 0 && ((uintptr_t)p32 & 3) == 0, -2,
                  "%s: segment %d: the 16-bit side must be 2-byte and the fp32 side 4-byte aligned", who, s);
    g.src[s] = src_list[s], g.dst[s] = dst_list[s], g.n[s] = n;
    total += (cut_of(p16, n).items + kBlockItems - 1) / kBlockItems;
  }
  g.first_block[kMaxSeg] = total;
  return 0;
}

}  // namespace

extern "C" int eavsr_pack16(const void* const* src_list, void* const* dst_list, const int64_t* n_list, int32_t nseg, int32_t dtype,
                            void* stream) {
  Segments g;
  int64_t total;
  if (int rc = fill("pack16", src_list, dst_list, n_list, nseg, dtype, 1, g, total)) return rc;
  if (total == 0) return 0;
  const dim3 grid((unsigned)(total < kGridCap ? total : kGridCap));
  if (dtype == EAVSR_CACHE16_BF16)
    hipLaunchKernelGGL(pack16_kernel<1>, grid, dim3(kThreads), 0, eavsr::as_stream(stream), g, total);
  else
    hipLaunchKernelGGL(pack16_kernel<0>, grid, dim3(kThreads), 0, eavsr::as_stream(stream), g, total);
  return eavsr::launch_status("pack16");
}

extern "C" int eavsr_pack16_census(const void* const* src_list, void* const* dst_list, const int64_t* n_list, int32_t nseg, int32_t dtype,
                                   uint64_t* census, void* stream) {
  EAVSR_REQUIRE(census != nullptr, -1, "pack16_census: NULL census");
  EAVSR_REQUIRE(((uintptr_t)census & 7) == 0, -2, "pack16_census: the census must be 8-byte aligned");
  Segments g;
  int64_t total;
  if (int rc = fill("pack16_census", src_list, dst_list, n_list, nseg, dtype, 1, g, total)) return rc;
  if (total == 0) return 0;
  const dim3 grid((unsigned)(total < kGridCap ? total : kGridCap));
  unsigned long long* record = reinterpret_cast<unsigned long long*>(census);
  if (dtype == EAVSR_CACHE16_BF16)
    hipLaunchKernelGGL(pack16_census_kernel<1>, grid, dim3(kThreads), 0, eavsr::as_stream(stream), g, total, record);
  else
    hipLaunchKernelGGL(pack16_census_kernel<0>, grid, dim3(kThreads), 0, eavsr::as_stream(stream), g, total, record);
  return eavsr::launch_status("pack16_census");
}

extern "C" int eavsr_unpack16(const void* const* src_list, void* const* dst_list, const int64_t* n_list, int32_t nseg, int32_t dtype,
                              void* stream) {
  Segments g;
  int64_t total;
  if (int rc = fill("unpack16", src_list, dst_list, n_list, nseg, dtype, 0, g, total)) return rc;
  if (total == 0) return 0;
  const dim3 grid((unsigned)(total < kGridCap ? total : kGridCap));
  if (dtype == EAVSR_CACHE16_BF16)
    hipLaunchKernelGGL(unpack16_kernel<1>, grid, dim3(kThreads), 0, eavsr::as_stream(stream), g, total);
  else
    hipLaunchKernelGGL(unpack16_kernel<0>, grid, dim3(kThreads), 0, eavsr::as_stream(stream), g, total);
  return eavsr::launch_status("unpack16");
}
