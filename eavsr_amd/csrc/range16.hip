// The range census of the 16-bit backbone modes (addendum): what the kernels of those modes round to fp16 / bf16, counted
// by a launch of its own into cache16_census.h's record of five 64-bit words -- `Tally` and `commit` as pack16_census uses them, the
// slot meanings unchanged.  One kernel, two flavours, each over a LIST of contiguous segments (as cache16.hip); nothing is written
// but the record.
//
// range16_words      -- the segments hold 16-bit words o that some kernel has already stored (NHWC activations, the IL8 layout).  An
//                       element's fp32 bits u are the exact widening of o: max_abs is the largest finite stored value, nonfinite
//                       counts the inf / NaN words, subnormal the subnormal words; overflow and flushed are 0 by construction (a
//                       finite u widens from a finite o; u != 0 exactly where o & 0x7FFF != 0).
// range16_as_rounded -- the segments hold fp32 values that a 16-bit route is about to round inside its own kernel.  o =
//                       round16(x), round16.h's, the function pack16 stores with: the record is pack16_census's on the same input.
//
// A segment of n elements is cut by its own address: `head` scalar elements up to the next 16-byte boundary (0 .. V - 1, V = 8
// words or 4 floats per 16 bytes), then 16-byte vectors, then a scalar tail (0 .. V - 1).  An ITEM is one vector or one scalar
// element, one lane each; a workgroup of 256 lanes takes kUnroll x 256 consecutive items of one segment (every load of a pass before
// its first count): vectors first, then head and tail elements.  The segment of a pass comes from the prefix sums of the segments'
// pass counts in the kernel arguments (pointers and extents by value, at most EAVSR_CACHE16_MAX_SEGMENTS; a longer list is split on
// the host).  Every extent is 64-bit.  The grid is capped at 2048 workgroups, the rest is a grid stride.  Integer max and add only:
// two launches give identical records.
//
// range16_stamp      -- one lane: *stamp = tick where the record holds a non-finite or an overflowed element and *stamp is still 0.
//                       Launched behind a count, it keeps WHEN a record that many launches share first left the range.
#include "common.h"
#include "cache16_census.h"
#include "round16.h"

#include <stdint.h>

namespace {

constexpr int kMaxSeg = EAVSR_CACHE16_MAX_SEGMENTS;
constexpr int kThreads = 256;
constexpr int kUnroll = 4;                                 // items per lane and workgroup pass: 4 x 16-byte loads in flight
constexpr int64_t kBlockItems = (int64_t)kThreads * kUnroll;
constexpr int kGridCap = 2048;                             // 256 CUs x 8 workgroups of 4 waves

struct Segments {
  const void* src[kMaxSeg];
  int64_t n[kMaxSeg];               // elements
  int64_t first_block[kMaxSeg + 1]; // prefix sums of the segments' workgroup passes
  int32_t nseg;
};

// the cut of a segment of n elements of ES bytes that starts at `p`: [0, head) scalar, nvec vectors of V = 16 / ES elements from
// head on, then n - head - V nvec scalar
struct Cut {
  int64_t head, nvec, items;
};

template <int ES>
__host__ __device__ inline Cut cut_of(const void* p, int64_t n) {
  constexpr int V = 16 / ES;
  int64_t head = (int64_t)((V - (((uintptr_t)p / ES) & (V - 1))) & (V - 1));
  if (head > n) head = n;
  const int64_t nvec = (n - head) / V;
  return Cut{head, nvec, n - (V - 1) * nvec};      // nvec vectors + (n - V nvec) scalar elements
}

// where scalar item j (0 <= j < n - V nvec) of a segment lies: the head's elements, then the tail's
template <int V>
__device__ __forceinline__ int64_t scalar_index(int64_t j, const Cut& c) { return j < c.head ? j : j + V * c.nvec; }

// one stored word: its fp32 bits are its exact widening
template <int BF16>
__device__ __forceinline__ void count_word(uint32_t o, census16::Tally& tally) {
  tally.count<BF16>(__float_as_uint(round16_ns::widen16<BF16>(o)), o);
}

// one fp32 value about to be rounded
template <int BF16>
__device__ __forceinline__ void count_value(uint32_t u, census16::Tally& tally) {
  tally.count<BF16>(u, round16_ns::round16<BF16>(__uint_as_float(u)));
}

// ROUNDED 0: segments of 16-bit words; 1: segments of fp32 values
template <int BF16, int ROUNDED>
__global__ __launch_bounds__(kThreads) void range16_kernel(Segments g, int64_t total_blocks, unsigned long long* record) {
  static_assert(kThreads == 64 * census16::kWaves, "the census reduction is written for this workgroup");
  constexpr int ES = ROUNDED ? 4 : 2, V = 16 / ES;
  census16::Tally tally;
  tally.clear();
  for (int64_t blk = blockIdx.x; blk < total_blocks; blk += gridDim.x) {
    int s = 0;
    while (s + 1 < g.nseg && blk >= g.first_block[s + 1]) ++s;      // uniform: the segment of this pass
    const int64_t n = g.n[s];
    const Cut c = cut_of<ES>(g.src[s], n);
    const int64_t base = (blk - g.first_block[s]) * kBlockItems + threadIdx.x;
    uint4 v[kUnroll];
    uint32_t e[kUnroll];
#pragma unroll
    for (int j = 0; j < kUnroll; ++j) {      // every load of the pass before its first count
      const int64_t i = base + (int64_t)j * kThreads;
      if (i < c.nvec) {
        if (ROUNDED)
          v[j] = *reinterpret_cast<const uint4*>(reinterpret_cast<const uint32_t*>(g.src[s]) + c.head + (int64_t)V * i);
        else
          v[j] = *reinterpret_cast<const uint4*>(reinterpret_cast<const uint16_t*>(g.src[s]) + c.head + (int64_t)V * i);
      } else if (i < c.items) {
        const int64_t k = scalar_index<V>(i - c.nvec, c);
        e[j] = ROUNDED ? reinterpret_cast<const uint32_t*>(g.src[s])[k] : (uint32_t)reinterpret_cast<const uint16_t*>(g.src[s])[k];
      }
    }
#pragma unroll
    for (int j = 0; j < kUnroll; ++j) {
      const int64_t i = base + (int64_t)j * kThreads;
      if (i < c.nvec) {
        const uint32_t q[4] = {v[j].x, v[j].y, v[j].z, v[j].w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          if (ROUNDED) {
            count_value<BF16>(q[k], tally);
          } else {
            count_word<BF16>(q[k] & 0xFFFFu, tally);
            count_word<BF16>(q[k] >> 16, tally);
          }
        }
      } else if (i < c.items) {
        if (ROUNDED)
          count_value<BF16>(e[j], tally);
        else
          count_word<BF16>(e[j], tally);
      }
    }
  }
  tally.commit(record);      // every lane, after the grid stride: a workgroup without a pass adds nothing
}

template <int ES>
int fill(const char* who, const void* const* src_list, const int64_t* n_list, int32_t nseg, int32_t dtype, const uint64_t* census,
         Segments& g, int64_t& total) {
  EAVSR_REQUIRE(census != nullptr, -1, "%s: NULL census", who);
  EAVSR_REQUIRE(((uintptr_t)census & 7) == 0, -2, "%s: the census must be 8-byte aligned", who);
  EAVSR_REQUIRE(nseg >= 0 && nseg <= kMaxSeg, -1, "%s: %d segments (0..%d)", who, nseg, kMaxSeg);
  EAVSR_REQUIRE(dtype == EAVSR_CACHE16_FP16 || dtype == EAVSR_CACHE16_BF16, -2, "%s: dtype %d (0: fp16, 1: bf16)", who, dtype);
  EAVSR_REQUIRE(nseg == 0 || (src_list && n_list), -1, "%s: NULL list", who);
  total = 0;
  g.nseg = nseg;
  for (int s = 0; s < kMaxSeg; ++s) {
    g.first_block[s] = total;
    g.src[s] = nullptr, g.n[s] = 0;
    if (s >= nseg) continue;
    const int64_t n = n_list[s];
    EAVSR_REQUIRE(n >= 0 && n < (int64_t(1) << 60), -2, "%s: segment %d has %lld elements", who, s, (long long)n);
    if (n == 0) continue;      // an empty segment: no pass, its pointer is never read
    EAVSR_REQUIRE(src_list[s] != nullptr, -1, "%s: segment %d: NULL pointer", who, s);
    EAVSR_REQUIRE(((uintptr_t)src_list[s] & (ES - 1)) == 0, -2, "%s: segment %d must be %d-byte aligned", who, s, ES);
    g.src[s] = src_list[s], g.n[s] = n;
    total += (cut_of<ES>(src_list[s], n).items + kBlockItems - 1) / kBlockItems;
  }
  g.first_block[kMaxSeg] = total;
  return 0;
}

// when a record first held a non-finite or an overflowed element: one lane, behind the launches that counted into it
__global__ void range16_stamp_kernel(const unsigned long long* record, unsigned long long* stamp, unsigned long long tick) {
  if (*stamp == 0 && (record[1] | record[2]) != 0) *stamp = tick;
}

}  // namespace

extern "C" int eavsr_range16_stamp(const uint64_t* census, uint64_t* stamp, uint64_t tick, void* stream) {
  EAVSR_REQUIRE(census != nullptr && stamp != nullptr, -1, "range16_stamp: NULL pointer");
  EAVSR_REQUIRE((((uintptr_t)census | (uintptr_t)stamp) & 7) == 0, -2, "range16_stamp: census and stamp must be 8-byte aligned");
  EAVSR_REQUIRE(tick != 0, -2, "range16_stamp: tick 0 means 'never'");
  hipLaunchKernelGGL(range16_stamp_kernel, dim3(1), dim3(1), 0, eavsr::as_stream(stream),
                     reinterpret_cast<const unsigned long long*>(census), reinterpret_cast<unsigned long long*>(stamp),
                     (unsigned long long)tick);
  return eavsr::launch_status("range16_stamp");
}

extern "C" int eavsr_range16_words(const void* const* src_list, const int64_t* n_list, int32_t nseg, int32_t dtype, uint64_t* census,
                                   void* stream) {
  Segments g;
  int64_t total;
  if (int rc = fill<2>("range16_words", src_list, n_list, nseg, dtype, census, g, total)) return rc;
  if (total == 0) return 0;
  const dim3 grid((unsigned)(total < kGridCap ? total : kGridCap));
  unsigned long long* record = reinterpret_cast<unsigned long long*>(census);
  if (dtype == EAVSR_CACHE16_BF16)
    hipLaunchKernelGGL((range16_kernel<1, 0>), grid, dim3(kThreads), 0, eavsr::as_stream(stream), g, total, record);
  else
    hipLaunchKernelGGL((range16_kernel<0, 0>), grid, dim3(kThreads), 0, eavsr::as_stream(stream), g, total, record);
  return eavsr::launch_status("range16_words");
}

extern "C" int eavsr_range16_as_rounded(const void* const* src_list, const int64_t* n_list, int32_t nseg, int32_t dtype,
                                        uint64_t* census, void* stream) {
  Segments g;
  int64_t total;
  if (int rc = fill<4>("range16_as_rounded", src_list, n_list, nseg, dtype, census, g, total)) return rc;
  if (total == 0) return 0;
  const dim3 grid((unsigned)(total < kGridCap ? total : kGridCap));
  unsigned long long* record = reinterpret_cast<unsigned long long*>(census);
  if (dtype == EAVSR_CACHE16_BF16)
    hipLaunchKernelGGL((range16_kernel<1, 1>), grid, dim3(kThreads), 0, eavsr::as_stream(stream), g, total, record);
  else
    hipLaunchKernelGGL((range16_kernel<0, 1>), grid, dim3(kThreads), 0, eavsr::as_stream(stream), g, total, record);
  return eavsr::launch_status("range16_as_rounded");
}
