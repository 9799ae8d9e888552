// common.h -- shared device/host helpers for libhipie_mi355 (gfx950 only; wave = 64).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/hipie_mi355.h"

namespace hipie {

typedef __bf16 bf16_t;
typedef _Float16 f16_t;

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef short i16x4 __attribute__((ext_vector_type(4)));
typedef short i16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));

// ---- error plumbing (host) -------------------------------------------------------------------------
extern thread_local char g_err[512];
int set_err(int code, const char* fmt, ...);
int check_launch(const char* what);

#define HIPIE_REQUIRE(cond, ...)                              \
  do {                                                        \
    if (!(cond)) return ::hipie::set_err(HIPIE_EINVAL, __VA_ARGS__); \
  } while (0)

// a check that has set the error itself (returns 0 or the code): pass the refusal on
#define HIPIE_TRY(call)                  \
  do {                                   \
    if (const int rc_ = (call)) return rc_; \
  } while (0)

// ---- dynamic-LDS limit (host) ----------------------------------------------------------------------
// A kernel that takes more dynamic LDS than the default 64 KiB needs hipFuncAttributeMaxDynamicSharedMemorySize raised, on every device
// it runs on.  One `static LdsLimit` per kernel at its launch site remembers what each device has been given and calls the runtime only
// when a launch needs more: the call is not a stream operation, so after a kernel's first launch it stays out of graph capture.
// `floor`: what needs no call at all (kernels whose LDS size varies pass the default limit).  A device index outside 0..63 is always set.
struct LdsLimit {
  size_t seen[64];                       // per device; zero-initialised (static storage)
  void raise(const void* kernel, size_t lds, size_t floor = 0) {
    if (lds <= floor) return;
    int dev = 0;
    (void)hipGetDevice(&dev);
    const bool known = dev >= 0 && dev < 64;
    if (known && lds <= seen[dev]) return;
    (void)hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (known) seen[dev] = lds;
  }
};

// ---- 16-bit <-> f32 ---------------------------------------------------------------------------------
template <typename T> struct elem;
template <> struct elem<float> {
  static __device__ __forceinline__ float to_f32(float x) { return x; }
  static __device__ __forceinline__ float from_f32(float x) { return x; }
};
template <> struct elem<bf16_t> {
  static __device__ __forceinline__ float to_f32(bf16_t x) { return (float)x; }
  static __device__ __forceinline__ bf16_t from_f32(float x) { return (bf16_t)x; }
};
template <> struct elem<f16_t> {
  static __device__ __forceinline__ float to_f32(f16_t x) { return (float)x; }
  static __device__ __forceinline__ f16_t from_f32(float x) { return (f16_t)x; }
};

// x -> (hi, lo) fp16 pair with hi = fp16(x), lo = fp16(x - hi)  (HIPIE_HL8).  The value is pinned in a register first: hipcc otherwise
// folds the multiply that PRODUCED x into a v_fma_mix*_f16 for one of its two uses (single rounding of the exact product) while the other
// use converts the fp32-rounded product -- near an fp16 tie the stored hi and the hi the remainder was taken from then differ by one ulp
// (measured: isolated 1-ulp(hi) errors in one output of 1e5).
// Values beyond the fp16 range saturate at +-65504 (an overflowing hi would be inf and its remainder x - inf a NaN).
__device__ __forceinline__ void hl_split(float x, f16_t& h, f16_t& l) {
  x = __builtin_fminf(__builtin_fmaxf(x, -65504.f), 65504.f);
#if defined(__HIP_DEVICE_COMPILE__)
  asm volatile("" : "+v"(x));
#endif
  h = (f16_t)x;
  l = (f16_t)(x - (float)h);
}

// ---- dtype code -> type (host) ------------------------------------------------------------------------
// f(T()) for the T of a HIPIE_F32 / HIPIE_F16 / HIPIE_BF16 code (a generic lambda reads it as decltype); another code is refused as "<what> <code>"
template <typename F>
static inline int with_dtype(int code, const char* what, F&& f) {
  switch (code) {
    case HIPIE_F32: return f(float());
    case HIPIE_F16: return f(f16_t());
    case HIPIE_BF16: return f(bf16_t());
    default: return set_err(HIPIE_EINVAL, "%s %d", what, code);
  }
}

static inline int ceil_div(int a, int b) { return (a + b - 1) / b; }

// A/B switches of the kernel studies (tile orders, wave counts, ablations: tools/bench_*.py).  The shipped library has ONE path per policy:
// the switches exist only in a study build (make EXTRA=-DHIPIE_STUDY_KNOBS), where they are read from the environment once per process.
#ifdef HIPIE_STUDY_KNOBS
static inline const char* study_env(const char* name) { return getenv(name); }
#else
static inline const char* study_env(const char*) { return nullptr; }
#endif

}  // namespace hipie
