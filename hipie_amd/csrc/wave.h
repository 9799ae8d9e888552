// wave.h -- the wave-level primitives the kernels share (gfx950, wave64), one definition each: LDS-DMA, s_waitcnt encodings, cross-half,
// three-way and lane maxima, the lane sum, the paired fp16 hi / lo split with its wait-state rules, 4-wide typed loads and stores.
// (mfma.h holds the MFMA / LDS-transpose lane layouts.)
#pragma once
#include "common.h"

namespace hipie {

// ---- LDS-DMA, 16 bytes per lane -----------------------------------------------------------------------------------------------------
// LDS[lds_dst + 16 * lane] <- *(sbase + voff).  Inline asm on purpose: the compiler tracks the builtin form as an LDS write and puts
// s_waitcnt vmcnt(0) in front of every later ds_read (a full L2 round trip per DMA, measured); here the completion is counted by
// hand -- vmcnt(0) (or vmcnt(n), see below) before the tile / stage barrier.  M0 carries the wave-uniform LDS byte address and is
// saved and restored around the load.
__device__ __forceinline__ void dma16(const char* sbase, unsigned int voff, unsigned int lds_dst) {
#if defined(__HIP_DEVICE_COMPILE__)
  unsigned int keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0"
               : "=&s"(keep) : "v"(voff), "s"(sbase), "s"(lds_dst) : "memory");
#endif
}

// The `off` address form: LDS[lds_dst + 16 * lane] <- *gsrc, every lane supplies a full 64-bit address (no scalar base).
__device__ __forceinline__ void dma16_off(const void* gsrc, unsigned int lds_dst) {
#if defined(__HIP_DEVICE_COMPILE__)
  unsigned int keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
               : "=&s"(keep) : "v"(gsrc), "s"(lds_dst) : "memory");
#endif
}

// The exec-masked form: as dma16 for the lanes of `mask` only (a tile's row-padding chunks are neither fetched nor written).  The lane
// mask is applied inside the statement -- s_and_saveexec / s_mov exec around the load, no branch -- and M0 is simply OVERWRITTEN, not
// restored (for kernels in which nothing else uses it): 5 scalar instructions per DMA where the compiler's own predication + an M0
// save / restore took 12.
__device__ __forceinline__ void dma16_masked(const char* sbase, unsigned int voff, unsigned int lds_dst, unsigned long long mask) {
#if defined(__HIP_DEVICE_COMPILE__)
  unsigned long long save;
  asm volatile("s_and_saveexec_b64 %0, %4\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\ts_mov_b64 exec, %0"
               : "=&s"(save) : "v"(voff), "s"(sbase), "s"(lds_dst), "s"(mask) : "memory", "m0");
#endif
}

// ---- s_waitcnt immediates (gfx9 encoding) for __builtin_amdgcn_s_waitcnt ---------------------------------------------------------------
constexpr int vmcnt(int n) { return 0x0F70 | (n & 15) | ((n >> 4) << 14); }   // s_waitcnt vmcnt(n) only
constexpr int lgkmcnt0 = 0xC07F;                                              // s_waitcnt lgkmcnt(0) only

// ---- maxima -------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float max3(float a, float b, float c) {
  float d;
  asm("v_max3_f32 %0, %1, %2, %3" : "=v"(d) : "v"(a), "v"(b), "v"(c));
  return d;
}

// max over the two 32-lane halves (lane l <-> l ^ 32) without LDS: v_permlane32_swap exchanges the upper half of its first
// operand with the lower half of its second
__device__ __forceinline__ float xhalf_max(float x) {
  typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
  const unsigned int u = __builtin_bit_cast(unsigned int, x);
  const u32x2 r = __builtin_amdgcn_permlane32_swap(u, u, false, false);
  return fmaxf(__builtin_bit_cast(float, (unsigned int)r[0]), __builtin_bit_cast(float, (unsigned int)r[1]));
}

// the maximum over the 64 lanes, in every lane: the xor butterfly
__device__ __forceinline__ float wave_max(float x) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x = fmaxf(x, __shfl_xor(x, o));
  return x;
}

// ---- sums -----------------------------------------------------------------------------------------------------------------------------
// the sum over the 64 lanes, in every lane: the xor butterfly, a fixed order of additions (the same bits from call to call)
__device__ __forceinline__ float wave_sum(float x) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o);
  return x;
}
__device__ __forceinline__ double wave_sum(double x) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o);
  return x;
}

// ---- paired fp16 hi / lo split ------------------------------------------------------------------------------------------------------
// two values -> one VGPR of fp16 hi halves and one of lo halves: hi = fp16(x) for the pair in one v_cvt_pk_f16_f32, lo = fp16(x - hi)
// from ONE v_fma_mix{lo,hi}_f16 each (the fp16 hi enters as an fp16 source operand of the fma, x - hi is exact, one rounding): the same
// bits as the C++ form `(f16)(x - (float)(f16)x)` (tools/split_form_check.py), which costs a v_cvt_f16_f32, a v_cvt_f32_f16 and a
// v_sub_f32 per VALUE on top of the two packs: 4 instead of 1.5 VALU per value, 80 of the ~230 VALU instructions a wave issues per
// 64-key tile of the global-attention instance of vit_attn_split.hip.  The asm operands are the register values themselves: nothing
// for the compiler to re-fold (see hl_split).  No clamp: a caller whose values may leave the fp16 range saturates them first.
// CONTRACT: the statements are inline asm, which hipcc's hazard recogniser does not look into -- a caller owes the two wait-state
// rules below, settle() behind the splits and exp_settle() in front of them.
__device__ __forceinline__ void hl_split2(const float a, const float b, unsigned int& H, unsigned int& L) {
#if defined(__HIP_DEVICE_COMPILE__) && !defined(HIPIE_NO_FMA_MIX)
  unsigned int h, l;
  asm("v_cvt_pk_f16_f32 %0, %1, %2" : "=v"(h) : "v"(a), "v"(b));
  asm("v_fma_mixlo_f16 %0, %1, -1.0, %2 op_sel_hi:[1,0,0]" : "=v"(l) : "v"(h), "v"(a));
  asm("v_fma_mixhi_f16 %0, %1, -1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "+v"(l) : "v"(h), "v"(b));
  H = h;
  L = l;
#else
  typedef _Float16 h2v __attribute__((ext_vector_type(2)));
  h2v h, l;
  h[0] = (f16_t)a; h[1] = (f16_t)b;
  l[0] = (f16_t)(a - (float)h[0]); l[1] = (f16_t)(b - (float)h[1]);
  H = __builtin_bit_cast(unsigned int, h);
  L = __builtin_bit_cast(unsigned int, l);
#endif
}

// Behind the splits: a VGPR written by the statements above and read by the NEXT instruction as an MFMA operand or by v_permlane*_swap
// is read too early (gfx950 needs 2 wait states there; round 5: the a22 error of the full-depth fixture went from 5e-5 to 1e-3 --
// isolated stale fragments -- until this was added).  One s_nop behind a block of splits, tied to every register the block wrote.
__device__ __forceinline__ void settle(unsigned int (&h)[4], unsigned int (&l)[4]) {
#if defined(__HIP_DEVICE_COMPILE__)
  asm volatile("s_nop 1" : "+v"(h[0]), "+v"(h[1]), "+v"(h[2]), "+v"(h[3]), "+v"(l[0]), "+v"(l[1]), "+v"(l[2]), "+v"(l[3]));
#endif
}

// In front of the splits: when the values come out of v_exp_f32 -- on gfx950 a transcendental result needs one wait state before a
// non-transcendental VALU instruction reads it.  hipcc inserts it for instructions it can see -- not for the asm statements of hl_split2.
// Where the scheduler happened to put something between the two nothing showed; in the 96-slot instance of vit_attn_split.hip with the
// 16-row tail it did not, and the splits read stale registers (garbage outputs, round 5).  One s_nop behind the block of exps, tied to
// all of them.
__device__ __forceinline__ void exp_settle(float (&pv)[8]) {
#if defined(__HIP_DEVICE_COMPILE__)
  asm volatile("s_nop 0" : "+v"(pv[0]), "+v"(pv[1]), "+v"(pv[2]), "+v"(pv[3]), "+v"(pv[4]), "+v"(pv[5]), "+v"(pv[6]), "+v"(pv[7]));
#endif
}

// ---- 4 consecutive elements of type T <-> 4 floats, one vector access ------------------------------------------------------------------
template <typename T> struct Vec4;
template <> struct Vec4<float> {
  static __device__ __forceinline__ void load(const float* p, float (&v)[4]) {
    const float4 r = *reinterpret_cast<const float4*>(p);
    v[0] = r.x; v[1] = r.y; v[2] = r.z; v[3] = r.w;
  }
  static __device__ __forceinline__ void store(float* p, const float (&v)[4]) {
    *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
  }
};
template <> struct Vec4<bf16_t> {
  static __device__ __forceinline__ void load(const bf16_t* p, float (&v)[4]) {
    const bf16x4 r = *reinterpret_cast<const bf16x4*>(p);
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = (float)r[i];
  }
  static __device__ __forceinline__ void store(bf16_t* p, const float (&v)[4]) {
    bf16x4 r;
#pragma unroll
    for (int i = 0; i < 4; ++i) r[i] = (bf16_t)v[i];
    *reinterpret_cast<bf16x4*>(p) = r;
  }
};
template <> struct Vec4<f16_t> {
  static __device__ __forceinline__ void load(const f16_t* p, float (&v)[4]) {
    const f16x4 r = *reinterpret_cast<const f16x4*>(p);
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = (float)r[i];
  }
  static __device__ __forceinline__ void store(f16_t* p, const float (&v)[4]) {
    f16x4 r;
#pragma unroll
    for (int i = 0; i < 4; ++i) r[i] = (f16_t)v[i];
    *reinterpret_cast<f16x4*>(p) = r;
  }
};

}  // namespace hipie
