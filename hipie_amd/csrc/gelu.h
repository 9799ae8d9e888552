// gelu.h -- the exact-erf GELU of the library, shared by the GEMM epilogue (gemm_tile.h) and the activation kernels of the training step
// (act_bwd.hip): ONE formula, so that an activation recomputed in the backward has the bits of the one the forward produced.
#pragma once
#include "common.h"

namespace hipie {

// exact-erf GELU (nn.GELU() default, timm Mlp: hipie/backbone/vit.py:193-197), branch-free:  gelu(x) = x * Phi(x),
//   Phi(x) = 1 - h(|x|) for x >= 0,  h(|x|) for x < 0,   h(a) = P(t) * exp(-a^2 / 2),  t = 1 / (1 + p a)
// -- the erfc form of Abramowitz & Stegun 7.1.26 with one more term, the seven constants re-fitted for this code (minimax over [0, 6 sqrt 2]:
// |erf error| 9.2e-9 against 1.4e-7 for the handbook's five-term constants; tools/fit_gelu_erf.py).  Evaluated in fp32: max |error| 3.8e-7
// over |x| <= 12, relative error <= 2.4e-7 |x| -- the figures of 0.5 x (1 + erff(x / sqrt 2)) with a correctly rounded erff, and better for
// x < -4, where 1 + erf cancels.  16 VALU instructions, two of them transcendental, no branch: ocml's erff is two polynomial branches
// (both executed by a wavefront) around an exp -- the fc1 epilogue (160 values per lane and tile) was 0.145 ms per launch behind fc2's.
__device__ __forceinline__ float gm_gelu(float x) {
#ifdef HIPIE_GELU_ERFF
  return 0.5f * x * (1.f + erff(x * 0.70710678118654752440f));
#endif
  const float a = __builtin_fabsf(x);
  const float t = __builtin_amdgcn_rcpf(__builtin_fmaf(0.27601078152656555f, a, 1.f));
  float q = -0.113462433218956f;
  q = __builtin_fmaf(q, t, 0.4407985508441925f);
  q = __builtin_fmaf(q, t, -0.31384575366973877f);
  q = __builtin_fmaf(q, t, 0.32216209173202515f);
  q = __builtin_fmaf(q, t, 0.046716462820768356f);
  q = __builtin_fmaf(q, t, 0.11763110756874084f);
  const float e = __builtin_amdgcn_exp2f(-0.7213475108146667f * (a * a));
  const float h = (q * t) * e;
  return x * (x >= 0.f ? 1.f - h : h);
}

// d gelu / dx = Phi(x) + x phi(x),  phi(x) = exp(-x^2 / 2) / sqrt(2 pi): Phi from the SAME h(|x|) as gm_gelu and phi from the same exp2 --
// written out again operation for operation, so that next to gm_gelu(x) the compiler keeps one copy of t, P(t) and e (no second
// transcendental).  |x| beyond 38.6: e = 0, h = 0, the derivative is exactly 1 or 0 (x * 0: no inf is formed anywhere).
__device__ __forceinline__ float gm_gelu_grad(float x) {
#ifdef HIPIE_GELU_ERFF
  return __builtin_fmaf(x, 0.3989422804014327f * expf(-0.5f * (x * x)), 0.5f * (1.f + erff(x * 0.70710678118654752440f)));
#endif
  const float a = __builtin_fabsf(x);
  const float t = __builtin_amdgcn_rcpf(__builtin_fmaf(0.27601078152656555f, a, 1.f));
  float q = -0.113462433218956f;
  q = __builtin_fmaf(q, t, 0.4407985508441925f);
  q = __builtin_fmaf(q, t, -0.31384575366973877f);
  q = __builtin_fmaf(q, t, 0.32216209173202515f);
  q = __builtin_fmaf(q, t, 0.046716462820768356f);
  q = __builtin_fmaf(q, t, 0.11763110756874084f);
  const float e = __builtin_amdgcn_exp2f(-0.7213475108146667f * (a * a));
  const float h = (q * t) * e;
  return __builtin_fmaf(x, 0.3989422804014327f * e, x >= 0.f ? 1.f - h : h);
}

}  // namespace hipie
