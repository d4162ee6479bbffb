// Device-side global-memory access helpers: buffer-resource loads / stores / LDS-DMA and the uniform-base load (gfx950 only).
#pragma once
#include "mfma.h"

#ifdef __HIPCC__

// Every global access of a pipeline that uses these is a BUFFER instruction (dcnv2_il2.hip since round 5; the epilogue of the
// grouped F(4x4,3x3) kernel and the bf16 weight-gradient kernel since round 6): a 128-bit resource (base + extent, four scalar
// registers, rebuilt once per tile) + one per-lane 32-bit offset register that lives as long as the tile + one scalar offset
// computed where it is used (one s_mul_i32 / s_add_i32).  The round-4 form (global_load / global_store / global_load_lds
// with 64-bit addresses) cost 4 scalar + 1-2 vector instructions per access for address arithmetic, a branch + two
// compares + two selects per window request of a border tile (zero padding) and an exec-mask region per store; here the
// hardware's range check does both jobs: a lane whose offset register holds EAVSR_OOB reads zeros (also into LDS) and its
// store is dropped.  The loop is bound by instruction ISSUE (one instruction per ~4 cycles and SIMD over both resident
// waves, scalar and branch instructions included: DESIGN.md 4b-r5), so every instruction removed is time.
typedef __amdgpu_buffer_rsrc_t eavsr_rsrc;
constexpr unsigned EAVSR_OOB = 0x80000000u;      // beyond every extent the launchers accept (< 2^31 bytes per resource)
__device__ __forceinline__ eavsr_rsrc eavsr_make_rsrc(const void* base, unsigned bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, (int)bytes, 0x00020000);
}
// scalar offset = c * s where c is a compile-time constant: computed AT the use by one s_mul_i32 the optimizer cannot hoist
// (hoisted, the ~60 distinct products of a pair step become long-lived scalar registers, spill, and a spilled scalar costs
// VECTOR instructions: v_readlane / v_writelane)
__device__ __forceinline__ unsigned eavsr_smul(unsigned s, int c) {      // c: a constant once the caller is inlined / unrolled
  unsigned r;
  asm volatile("s_mul_i32 %0, %1, %2" : "=s"(r) : "s"(s), "i"(c));
  return r;
}
__device__ __forceinline__ float eavsr_buf_ld(eavsr_rsrc r, unsigned voff, unsigned soff) {
  return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, voff, soff, 0));
}
__device__ __forceinline__ f32x4 eavsr_buf_ld4(eavsr_rsrc r, unsigned voff, unsigned soff) {
  return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r, voff, soff, 0));
}
__device__ __forceinline__ void eavsr_buf_st(eavsr_rsrc r, unsigned voff, unsigned soff, float v) {
  __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), r, voff, soff, 0);
}
__device__ __forceinline__ void eavsr_buf_dma16(eavsr_rsrc r, unsigned voff, unsigned soff, char* lds_dst) {
  __builtin_amdgcn_raw_ptr_buffer_load_lds(r, (lptr_t)lds_dst, 16, voff, soff, 0, 0);
}
// A 128-bit store's offset goes through the VECTOR offset (one v_add per store), never through the scalar one.  A 128-bit buffer
// store reads its data registers over the cycles after it issues, and a vector instruction that rewrites them too early corrupts
// the store.  The compiler pads that hazard -- except for stores with a REGISTER scalar offset, which older parts exempt; gfx950
// does not honour the exemption: with `soffset` in a register the next channel's results landed in the previous channel's rows
// for the last lanes of each row segment, run-dependent (found by tools/dbg/rsc_diff.py against the round-5 library; one wait
// state).  With an immediate scalar offset the hazard recogniser does its job.
__device__ __forceinline__ void eavsr_buf_st4(eavsr_rsrc r, unsigned voff, unsigned off, f32x4 v) {
  __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), r, voff + off, 0, 0);
}

// load through a wave-uniform base + 32-bit BYTE offset: lowers to `global_load_dword v, v_off, s[base]`
// (an element index would have to be shifted in 64 bits, which forces per-lane 64-bit addresses)
__device__ __forceinline__ float eavsr_ld_b(const float* base, unsigned byte_off) {
  return *reinterpret_cast<const float*>(reinterpret_cast<const char*>(base) + byte_off);
}

#endif  // __HIPCC__
