// Scene-cut statistics on the 8-bit frames the device already holds (eavsr_frame_change_u8): per frame a 64-bin histogram
// of the luma, per pair of consecutive frames the sum of absolute luma differences.  All integers: exact, independent of the
// order of summation, so the integer atomics below leave two calls bit-identical.
//   Y = (77 R + 150 G + 29 B + 128) >> 8 for three channels, Y = v for one;  hist[f][Y >> 2];  sad[f] = sum |Y_f - Y_{f+1}|.
//
// One launch.  A workgroup of 256 lanes owns 4096 pixels -- lane l the 16 consecutive pixels from (256 block + l) 16 -- and walks a
// run of frames in order with the previous frame's 16 lumas packed in four registers: every byte of a run is read once.  So that
// a small frame still fills the chip, the F frames are cut into gridDim.y runs of `run` frames; a run that does not start at frame
// 0 reads the frame before it for its luma alone (one extra frame per run; at most ceil(F / 8) runs, so at most about 1 / 8 more
// bytes: the wrapper's bound.  The runs themselves may be shorter than 8 frames: F = 9 gives 5 + 4).
// Loads: three 16-byte loads per lane and frame (one per plane, or the 48 interleaved bytes of the 16 pixels); the next frame's are
// issued before this frame's arithmetic.  A lane's 16 bytes start wherever base + plane + pixel falls, so they are read through
// memcpy from a byte pointer, which the compiler turns into ONE global_load_dwordx4 at an arbitrary byte address.  That is a
// DEPENDENCY on the amdhsa unaligned-access mode: the compiler assumes it for this target and the driver sets it for every queue
// (the listing was checked: 3 or 9 dwordx4 loads per kernel, no byte loads outside the tail).  A target without the mode would get
// byte loads from the same source, correct and slower.  There is no scalar head; the last h w % 16 pixels are read byte by byte.
// Histogram: 32 copies of the 64 bins in LDS (copy = lane % 32, bin-major: a wave in a flat region spreads over 32 banks instead
// of serialising on one address), ds_add per pixel; after a barrier thread t sums and clears eight copies of bin t / 4, four lanes
// combine by shuffle and one adds into hist with a global atomic.  SAD: v_sad_u8 on the packed lumas, a wave reduction by
// shuffles, one 64-bit global atomic per wave and pair.  A wave's partial is at most 1024 x 255: 32 bits hold it; the global sum is
// 64 bits wide end to end.
#include "common.h"

#include <stdint.h>

namespace {

constexpr int kThreads = 256;
constexpr int kPix = 16;                   // pixels per lane
constexpr int kBlockPix = kThreads * kPix; // pixels per workgroup
constexpr int kBins = 64;
constexpr int kCopies = 32;

struct Raw {
  uint32_t w[12];      // planar: w[4 c + k] = pixels 4 k .. 4 k + 3 of plane c; interleaved: the 48 bytes in order
};

__device__ __forceinline__ void load16(const uint8_t* p, uint32_t* w) {
  uint4 v;
  __builtin_memcpy(&v, p, 16);      // any alignment; one dwordx4 load in the target's unaligned-access mode
  w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
}

// bytes [0, count) of p into the little-endian words w (zero on entry), count <= 4 WORDS
template <int WORDS>
__device__ __forceinline__ void load_bytes(const uint8_t* p, int count, uint32_t* w) {
#pragma unroll
  for (int i = 0; i < 4 * WORDS; ++i)      // constant register indices: nothing spills to scratch
    if (i < count) w[i >> 2] |= (uint32_t)p[i] << (8 * (i & 3));
}

// the lane's pixels p0 .. p0 + nvalid - 1 of one frame (frame: its first byte); pixels past nvalid read as 0
template <int C, bool HWC>
__device__ __forceinline__ Raw load_frame(const uint8_t* frame, size_t hw, size_t p0, int nvalid) {
  Raw r;
#pragma unroll
  for (int k = 0; k < 12; ++k) r.w[k] = 0;
  if (nvalid == kPix) {
    if (HWC) {
#pragma unroll
      for (int k = 0; k < 3; ++k) load16(frame + 3 * p0 + 16 * k, r.w + 4 * k);
    } else {
#pragma unroll
      for (int c = 0; c < C; ++c) load16(frame + c * hw + p0, r.w + 4 * c);
    }
  } else if (nvalid > 0) {
    if (HWC) {
      load_bytes<12>(frame + 3 * p0, 3 * nvalid, r.w);
    } else {
#pragma unroll
      for (int c = 0; c < C; ++c) load_bytes<4>(frame + c * hw + p0, nvalid, r.w + 4 * c);
    }
  }
  return r;
}

__device__ __forceinline__ uint32_t byte_of(const uint32_t* w, int i) { return (w[i >> 2] >> (8 * (i & 3))) & 255u; }

// the 16 lumas, four to a word
template <int C, bool HWC>
__device__ __forceinline__ void luma16(const Raw& r, uint32_t* y) {
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (C == 1) {
      y[k] = r.w[k];
    } else {
      uint32_t word = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int i = 4 * k + j;
        const uint32_t R = HWC ? byte_of(r.w, 3 * i) : byte_of(r.w, i);
        const uint32_t G = HWC ? byte_of(r.w, 3 * i + 1) : byte_of(r.w + 4, i);
        const uint32_t B = HWC ? byte_of(r.w, 3 * i + 2) : byte_of(r.w + 8, i);
        word |= ((77u * R + 150u * G + 29u * B + 128u) >> 8) << (8 * j);      // at most 255: 256 x 255 + 128 < 2^16
      }
      y[k] = word;
    }
  }
}

template <int C, bool HWC>
__global__ __launch_bounds__(kThreads) void frame_change_kernel(const uint8_t* __restrict__ in, int32_t* __restrict__ hist,
                                                                unsigned long long* __restrict__ sad, int F, size_t hw, int run) {
  __shared__ uint32_t bins[kBins * kCopies];
  const int tid = threadIdx.x;
  for (int i = tid; i < kBins * kCopies; i += kThreads) bins[i] = 0;
  __syncthreads();
  const size_t p0 = ((size_t)blockIdx.x * kThreads + tid) * kPix;
  const int nvalid = p0 >= hw ? 0 : (hw - p0 >= (size_t)kPix ? kPix : (int)(hw - p0));
  const size_t frame_bytes = (size_t)C * hw;
  const int f0 = blockIdx.y * run;
  const int f1 = f0 + run < F ? f0 + run : F;
  const int copy = tid & (kCopies - 1);

  uint32_t prev[4] = {0, 0, 0, 0};
  if (f0 > 0) luma16<C, HWC>(load_frame<C, HWC>(in + (size_t)(f0 - 1) * frame_bytes, hw, p0, nvalid), prev);
  Raw cur = load_frame<C, HWC>(in + (size_t)f0 * frame_bytes, hw, p0, nvalid);
  for (int f = f0; f < f1; ++f) {
    Raw nxt = cur;
    if (f + 1 < f1) nxt = load_frame<C, HWC>(in + (size_t)(f + 1) * frame_bytes, hw, p0, nvalid);
    uint32_t y[4];
    luma16<C, HWC>(cur, y);
    if (nvalid == kPix) {
#pragma unroll
      for (int i = 0; i < kPix; ++i) atomicAdd(&bins[(byte_of(y, i) >> 2) * kCopies + copy], 1u);
    } else {
#pragma unroll
      for (int i = 0; i < kPix; ++i)
        if (i < nvalid) atomicAdd(&bins[(byte_of(y, i) >> 2) * kCopies + copy], 1u);
    }
    if (f > 0) {
      uint32_t s = 0;      // pixels past nvalid are 0 in both frames
#pragma unroll
      for (int k = 0; k < 4; ++k) s = __builtin_amdgcn_sad_u8(y[k], prev[k], s);
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
      if ((tid & 63) == 0 && s != 0) atomicAdd(&sad[f - 1], (unsigned long long)s);
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) prev[k] = y[k];
    cur = nxt;
    __syncthreads();
    // thread t: copies 8 (t % 4) .. + 7 of bin t / 4, read and cleared by the one thread that owns them
    {
      uint32_t* mine = bins + (tid >> 2) * kCopies + 8 * (tid & 3);
      uint32_t n = 0;
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        n += mine[k];
        mine[k] = 0;
      }
      n += __shfl_xor(n, 1);
      n += __shfl_xor(n, 2);
      if ((tid & 3) == 0 && n != 0) atomicAdd(&hist[(size_t)f * kBins + (tid >> 2)], (int32_t)n);
    }
    __syncthreads();
  }
}

template <int C, bool HWC>
void launch(const uint8_t* in, int32_t* hist, int64_t* sad, int F, size_t hw, hipStream_t st) {
  const unsigned blocks = (unsigned)((hw + kBlockPix - 1) / kBlockPix);
  // enough workgroups to fill 256 CUs eight deep, but at most ceil(F / 8) runs: a run re-reads one frame
  int runs = (int)((2048 + blocks - 1) / blocks);
  const int most = (F + 7) / 8;
  if (runs > most) runs = most;
  if (runs < 1) runs = 1;
  const int run = (F + runs - 1) / runs;
  runs = (F + run - 1) / run;
  hipLaunchKernelGGL((frame_change_kernel<C, HWC>), dim3(blocks, (unsigned)runs), dim3(kThreads), 0, st, in, hist,
                     reinterpret_cast<unsigned long long*>(sad), F, hw, run);
}

}  // namespace

extern "C" int eavsr_frame_change_u8(const uint8_t* in, int32_t* hist, int64_t* sad, int32_t F, int32_t C, int32_t H, int32_t W, int32_t hwc,
                                     void* stream) {
  EAVSR_REQUIRE(in && hist && (sad || F <= 1), -1, "frame_change_u8: NULL pointer");
  EAVSR_REQUIRE(F >= 1 && H >= 1 && W >= 1, -2, "frame_change_u8: bad dims F=%d H=%d W=%d", F, H, W);
  EAVSR_REQUIRE(C == 1 || C == 3, -2, "frame_change_u8: C=%d: grey (1) or RGB (3)", C);
  EAVSR_REQUIRE(hwc == 0 || hwc == 1, -2, "frame_change_u8: hwc %d (0 = planes (F, C, H, W), 1 = interleaved (F, H, W, 3))", hwc);
  EAVSR_REQUIRE(!hwc || C == 3, -2, "frame_change_u8: an interleaved source has 3 channels, got C=%d", C);
  EAVSR_REQUIRE((int64_t)H * W < 2147483648ll, -2, "frame_change_u8: frames of %lld pixels, fewer than 2^31 (a bin is 32 bits)",
                (long long)H * W);
  EAVSR_REQUIRE((((uintptr_t)hist) & 3) == 0 && (((uintptr_t)sad) & 7) == 0, -2, "frame_change_u8: hist 4-byte, sad 8-byte aligned");
  hipStream_t st = eavsr::as_stream(stream);
  const size_t hw = (size_t)H * W;
  if (C == 1) launch<1, false>(in, hist, sad, F, hw, st);
  else if (hwc) launch<3, true>(in, hist, sad, F, hw, st);
  else launch<3, false>(in, hist, sad, F, hw, st);
  return eavsr::launch_status("frame_change_u8");
}
