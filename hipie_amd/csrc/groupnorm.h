// groupnorm.h -- what groupnorm.hip (forward) and groupnorm_bwd.hip (the training step's backward) share, one definition each: the group
// geometry, the 32-byte per-thread access and the chunking of an NCHW channel row.
#pragma once
#include "common.h"

namespace hipie {

constexpr int GN_CPG = 8;          // channels per group
constexpr int GN_MAXK = 512;       // partials per (image, group)

template <typename T> struct V8 {
  static __device__ __forceinline__ void ld(const T* p, float (&v)[8]) {
    typedef T t8 __attribute__((ext_vector_type(8)));
    const t8 r = *reinterpret_cast<const t8*>(p);
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = (float)r[i];
  }
  static __device__ __forceinline__ void st(T* p, const float (&v)[8]) {
    typedef T t8 __attribute__((ext_vector_type(8)));
    t8 r;
#pragma unroll
    for (int i = 0; i < 8; ++i) r[i] = (T)v[i];
    *reinterpret_cast<t8*>(p) = r;
  }
};

// NCHW: y = fmaf(v, sc, sh) for channel c -- the two statements of gn_apply_nchw_kernel (which keeps its own text: calling this from it
// reorders its loads, and its ISA is pinned), the same operations in the same order.  The backward recomputes the ReLU mask
// [fmaf(x, sc, sh) > 0] from them, the forward's `y > 0` bit for bit (tests/test_gpu_group_norm_bwd.py, the mask identity).
__device__ __forceinline__ void gn_scale_shift_nchw(float gamma_c, float beta_c, float prebias_c, float mean, float rstd, float& sc, float& sh) {
  sc = rstd * gamma_c;
  sh = beta_c + (prebias_c - mean) * sc;
}

// NCHW: a channel row of HW values (HW % 8 == 0) is cut into nchunk <= GN_MAXK / GN_CPG runs of `per` values (per % 8 == 0, the last one may
// be shorter); one workgroup per (chunk, image * channel), so the workgroups of a row walk contiguous memory.  The forward's partial sums
// and the backward's are both 2 floats per (image, channel, chunk).
static inline void gn_nchw_chunks(int HW, int& nchunk, int& per) {
  nchunk = HW / 8192;
  nchunk = nchunk < 1 ? 1 : (nchunk > GN_MAXK / GN_CPG ? GN_MAXK / GN_CPG : nchunk);
  per = (HW + nchunk - 1) / nchunk;
  per = (per + 7) / 8 * 8;
  nchunk = (HW + per - 1) / per;
}

}  // namespace hipie
