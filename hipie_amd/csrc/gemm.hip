// gemm.hip -- the entry points of the GEMM family on the tile kernels of gemm_tile.h (the design is described there): hipie_gemm and its
// dispatch between the thin-K kernel (gemm_k256.hip), the 64 x 128 tile kernel and the 256-row tile kernel, the gather, batched and
// 3 x 3 convolution forms, and the producers of split operands (hipie_to_hl8, hipie_to_hl8_t).
#include "gemm_tile.h"

namespace hipie {

// fp32 / fp16 rows -> HL8 (optionally scaled): the generic producer of split operands (weights are split once on the host)
template <typename T>
__global__ __launch_bounds__(256) void to_hl8_kernel(const T* __restrict__ x, f16_t* __restrict__ out, long rows, int K, long ldx, long ldo,
                                                     float scale) {
  const long gid = (long)blockIdx.x * 256 + threadIdx.x;       // one group of 8 elements per thread
  const int gpr = K / 8;
  if (gid >= rows * gpr) return;
  const long r = gid / gpr;
  const int g = (int)(gid - r * gpr);
  const T* src = x + r * ldx + 8 * g;
  f16x8 h, l;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    f16_t hh, ll;
    hl_split((float)src[e] * scale, hh, ll);
    h[e] = hh;
    l[e] = ll;
  }
  f16_t* dst = out + r * ldo + 16 * g;
  *reinterpret_cast<f16x8*>(dst) = h;
  *reinterpret_cast<f16x8*>(dst + 8) = l;
}


// x (rows x C fp32, row stride ldx) -> out (C x 2 rows_p) HL8: the TRANSPOSE as a split operand, for products that contract over the rows
// (the weight gradients of the training step: dW = dy^T . x needs dy^T and x^T with the token dimension as K).  One pass instead of a
// strided transpose copy followed by hipie_to_hl8: a 128-row x 64-column tile goes through LDS; columns beyond `rows` (up to rows_p, a
// multiple of 8) are written as zeros.
constexpr int kTrRows = 128, kTrCols = 64;
__global__ __launch_bounds__(256) void to_hl8_t_kernel(const float* __restrict__ x, f16_t* __restrict__ out, long rows, int C, long ldx,
                                                       long ldo, long rows_p, float scale) {
  __shared__ float tile[kTrRows][kTrCols + 1];
  const long r0 = (long)blockIdx.x * kTrRows;
  const int c0 = blockIdx.y * kTrCols;
  const int tid = threadIdx.x;
  for (int k = tid; k < kTrRows * (kTrCols / 4); k += 256) {           // coalesced along the columns
    const int i = k / (kTrCols / 4), j = (k % (kTrCols / 4)) * 4;
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    if (r0 + i < rows) {
      const float* src = x + (r0 + i) * ldx + c0 + j;
      if (c0 + j + 3 < C && (((uintptr_t)src) & 15) == 0) {
        const float4 q = *reinterpret_cast<const float4*>(src);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
      } else {
        for (int e = 0; e < 4; ++e) v[e] = c0 + j + e < C ? src[e] : 0.f;
      }
    }
    for (int e = 0; e < 4; ++e) tile[i][j + e] = v[e];
  }
  __syncthreads();
  for (int u = tid; u < kTrCols * (kTrRows / 8); u += 256) {           // unit = (output row c, group of 8 source rows)
    const int g = u % (kTrRows / 8), c = u / (kTrRows / 8);      // lanes along the 16 row groups: 512 contiguous bytes of one output row
    const long m = r0 + 8 * g;
    if (c0 + c >= C || m >= rows_p) continue;
    f16x8 h, l;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      f16_t hh, ll;
      hl_split(tile[8 * g + e][c] * scale, hh, ll);
      h[e] = hh;
      l[e] = ll;
    }
    f16_t* dst = out + (long)(c0 + c) * ldo + 2 * m;
    *reinterpret_cast<f16x8*>(dst) = h;
    *reinterpret_cast<f16x8*>(dst + 8) = l;
  }
}

}  // namespace hipie

using namespace hipie;

namespace hipie {       // gemm_k256.hip
int launch_gemm_k256(const void* X, long ldx_b, int x_f32, const void* W, long ldw_b, const float* bias, float* out, long ldo, int M, int N,
                     hipStream_t st);
}

// The MFMA shape of the wide split instances: true = the 16x16x32 form (gemm_tile.h, MS = 16).  ONE rule for wide && split: in the same-process
// A/B on random operands (tools/bench_gemm_mfma.py, 7 rounds x 50 launches, 32768 rows; docs/measurements.md) the median of the 16x16x32
// instance is below the MINIMUM of the 32x32x16 one on every shape -- ms, 32 -> 16: qkv 0.792 -> 0.715, fc1 + GELU 1.071 -> 0.987, proj 0.271 ->
// 0.249, fc2 0.965 -> 0.877, proj / fc2 with fp32 output and residual 0.325 -> 0.279 / 1.007 -> 0.901, gathered qkv 0.787 -> 0.723 -- so no rule
// on K is needed.  HIPIE_GEMM_MFMA=16|32 (study builds) is read at EVERY launch, unlike the switches of gemm_impl, so that the tool can
// alternate the two instances inside one process.
static inline bool gemm_mfma16() {
  const char* e = study_env("HIPIE_GEMM_MFMA");
  return e ? atoi(e) == 16 : true;
}

static int gemm_impl(const void* A, int64_t lda, const void* W, int64_t ldw, const float* bias, const float* resid, int64_t ldr,
                     void* out, int64_t ldo, const int32_t* out_row, const int32_t* a_row, int64_t a_rows, int M, int N, int K, int in_fmt,
                     int out_fmt, int act, float alpha, float oscale, void* stream, const float* alpha_dev = nullptr) {
  HIPIE_REQUIRE(A && W && out, "gemm: null pointer");
  HIPIE_REQUIRE(in_fmt == HIPIE_F16 || in_fmt == HIPIE_HL8 || in_fmt == HIPIE_F32, "gemm: operand format %d (HIPIE_F16 | HIPIE_HL8 | HIPIE_F32)",
                in_fmt);
  HIPIE_REQUIRE(out_fmt == HIPIE_F32 || out_fmt == HIPIE_F16 || out_fmt == HIPIE_HL8, "gemm: output format %d", out_fmt);
  HIPIE_REQUIRE(act >= 0 && act <= 3, "gemm: activation %d (0 none, 1 gelu, 2 relu, 3 quick-gelu)", act);
  HIPIE_REQUIRE(M > 0 && N > 0 && K > 0 && N % 8 == 0, "gemm: M=%d N=%d K=%d (N must be a multiple of 8)", M, N, K);
  const bool a_f32 = in_fmt == HIPIE_F32;       // A rows are plain fp32 (lda in fp32 elements), split in the kernel; W is HL8
  const bool split = in_fmt == HIPIE_HL8 || a_f32;
  if (a_f32) lda *= 2;                          // from here on in fp16 units like the HL8 form: the same bytes per row
  const int kq = split ? 32 : 64;               // elements per 128-byte k tile
  HIPIE_REQUIRE(K % kq == 0, "gemm: K=%d must be a multiple of %d", K, kq);
  const int epr = split ? 2 * K : K;            // fp16 elements per operand row
  HIPIE_TRY(gm_check_operands("gemm", lda, ldw, epr, 320));
  HIPIE_TRY(gm_check_out("gemm", ldo, out_fmt, N));
  HIPIE_TRY(gm_check_resid("gemm", resid, ldr, N));
  HIPIE_TRY(gm_check_aligned("gemm", {A, W, out, bias, resid}));
  GemmParams p;
  gm_set_operands(p, A, lda, W, ldw, M, N, K, kq);
  p.bias = bias; p.resid = resid; p.ldr = ldr; p.out = (char*)out; p.ldo = ldo; p.out_row = out_row; p.a_row = a_row;
  p.out_fmt = out_fmt; p.act = act; p.alpha = alpha; p.oscale = oscale; p.alpha_dev = alpha_dev;
  hipStream_t st = (hipStream_t)stream;
  // K = 256 linears over many rows with a plain fp32 result: the thin-K kernel (gemm_k256.hip: X rows live in registers, the weight
  // streams through LDS in 32-feature chunks) where it is faster than the 256-column tiles -- N >= 384 (tools/bench_gemm_k256.py: -20 % at
  // N = 384, -7 % at 1024, -9 % at 2304; level at N = 256).  HIPIE_GEMM_K256=0: never, =1: every eligible shape (A/B timing)
  // (diagnostic switches are read from the environment ONCE per process, not per launch)
  static const int k256_mode = [] { const char* e = study_env("HIPIE_GEMM_K256"); return e ? atoi(e) : 2; }();
  const bool k256_on = k256_mode == 1 || (k256_mode == 2 && N >= 384);
  // the thin-K kernel addresses X rows with 32-bit offsets from the base of the whole matrix: M rows must stay below 4 GiB
  if (k256_on && split && K == 256 && out_fmt == HIPIE_F32 && act == 0 && resid == nullptr && out_row == nullptr && a_row == nullptr &&
      alpha == 1.f && oscale == 1.f && alpha_dev == nullptr && N % 32 == 0 && M >= 8192 && ldw * 2 == 1024 && (long)M * p.lda_b < (1L << 32))
    return launch_gemm_k256(A, p.lda_b, a_f32 ? 1 : 0, W, p.ldw_b, bias, (float*)out, ldo, M, N, st);
  const bool wide = (N % 320 == 0);
  // problems that fill less than 3/8 of the CUs with 256-row tiles go to the 64 x 128 tile kernel (HIPIE_GEMM_SMALL=0: never; A/B timing)
  static const int small_on = [] { const char* e = study_env("HIPIE_GEMM_SMALL"); return e ? atoi(e) : 1; }();
  static const long small_tiles = [] { const char* e = study_env("HIPIE_GEMM_SMALL_MAXTILES"); return e ? atol(e) : 96L; }();      // A/B runs: tools/bench_gemm_small.py big
  const bool small_ok = small_on && (long)((M + 255) / 256) * ((N + (wide ? 319 : 255)) / (wide ? 320 : 256)) < small_tiles;
#ifdef HIPIE_GEMM_VARIANTS
  { const char* e = study_env("HIPIE_GEMM_VARIANT"); const int v = e ? atoi(e) : 0;
    if (split && wide && v == 1) return launch_gemm<320, true, 1>(p, st);
    if (split && wide && v == 3) return launch_gemm<320, true, 3>(p, st); }
  { const char* e = study_env("HIPIE_GEMM_VARIANT"); if (e) p.variant = atoi(e); }
  p.prio_mode = gemm2_prio();
  if (split && gemm2_mode() == 4) {
    const bool w160 = (N % 160 == 0);
    if (a_f32) return w160 ? launch_gemm4<5, 2>(p, st) : launch_gemm4<4, 2>(p, st);
    return w160 ? launch_gemm4<5, 0>(p, st) : launch_gemm4<4, 0>(p, st);
  }
  if (split && gemm2_mode() == 2) {
    const bool w160 = (N % 160 == 0);
    if (a_f32) return w160 ? launch_gemm3<5, 2>(p, st) : launch_gemm3<4, 2>(p, st);
    return w160 ? launch_gemm3<5, 0>(p, st) : launch_gemm3<4, 0>(p, st);
  }
  if (split && gemm2_mode() == 1) {
    const bool w160 = (N % 160 == 0);
    if (a_f32) return w160 ? launch_gemm2<5, 2>(p, st) : launch_gemm2<4, 2>(p, st);
    return w160 ? launch_gemm2<5, 0>(p, st) : launch_gemm2<4, 0>(p, st);
  }
#endif
  if (split && small_ok && a_row == nullptr) return a_f32 ? launch_gemm_small<2>(p, st) : launch_gemm_small<0>(p, st);
  // wide split outputs (the four ViT linears, the gathered windowed qkv): the MFMA shape of the k loop, see gemm_mfma16
  if (split && wide && gemm_mfma16()) return a_f32 ? launch_gemm<320, true, 2, 16>(p, st) : launch_gemm<320, true, 0, 16>(p, st);
  if (a_f32) return wide ? launch_gemm<320, true, 2>(p, st) : launch_gemm<256, true, 2>(p, st);
  if (split) return wide ? launch_gemm<320, true>(p, st) : launch_gemm<256, true>(p, st);
  return wide ? launch_gemm<320, false>(p, st) : launch_gemm<256, false>(p, st);
}

extern "C" int hipie_gemm(const void* A, int64_t lda, const void* W, int64_t ldw, const float* bias, const float* resid, int64_t ldr,
                          void* out, int64_t ldo, const int32_t* out_row, int M, int N, int K, int in_fmt, int out_fmt, int act, float alpha,
                          float oscale, void* stream) {
  return gemm_impl(A, lda, W, ldw, bias, resid, ldr, out, ldo, out_row, nullptr, 0, M, N, K, in_fmt, out_fmt, act, alpha, oscale, stream);
}

// hipie_gemm + a device factor of alpha.  The thin-K kernel (gemm_k256.hip) has no alpha at all, so a call WITH the pointer never goes there
// (gemm_impl); every tile kernel reads it (gm_alpha_dev).  NULL: hipie_gemm, dispatch and bits.
extern "C" int hipie_gemm_scaled(const void* A, int64_t lda, const void* W, int64_t ldw, const float* bias, const float* resid, int64_t ldr,
                                 void* out, int64_t ldo, const int32_t* out_row, int M, int N, int K, int in_fmt, int out_fmt, int act, float alpha,
                                 float oscale, const float* alpha_dev, void* stream) {
  HIPIE_REQUIRE(((uintptr_t)alpha_dev % 4) == 0, "gemm_scaled: alpha_dev must be 4-byte aligned");
  return gemm_impl(A, lda, W, ldw, bias, resid, ldr, out, ldo, out_row, nullptr, 0, M, N, K, in_fmt, out_fmt, act, alpha, oscale, stream, alpha_dev);
}

extern "C" int hipie_gemm_gather(const void* A, int64_t lda, int64_t a_rows, const int32_t* a_row, const void* W, int64_t ldw, const float* bias,
                                 const float* resid, int64_t ldr, void* out, int64_t ldo, const int32_t* out_row, int M, int N, int K, int in_fmt,
                                 int out_fmt, int act, float alpha, float oscale, void* stream) {
  HIPIE_REQUIRE(a_row != nullptr && a_rows > 0, "gemm_gather: a_row map / operand row count missing");
  HIPIE_REQUIRE(in_fmt == HIPIE_HL8 || in_fmt == HIPIE_F32, "gemm_gather: split operands only (HIPIE_HL8 | HIPIE_F32 rows)");
  HIPIE_REQUIRE((long)a_rows * lda * (in_fmt == HIPIE_F32 ? 4 : 2) < (1L << 32), "gemm_gather: the gathered operand must stay below 4 GiB");
  return gemm_impl(A, lda, W, ldw, bias, resid, ldr, out, ldo, out_row, a_row, a_rows, M, N, K, in_fmt, out_fmt, act, alpha, oscale, stream);
}

extern "C" int hipie_gemm_batched(const void* A, int64_t lda, int64_t a_outer, int64_t a_inner, const void* W, int64_t ldw, int64_t w_outer,
                                  int64_t w_inner, void* out, int64_t ldo, int64_t o_outer, int64_t o_inner, int n_outer, int n_inner, int M,
                                  int N, int K, int out_fmt, float alpha, void* stream) {
  HIPIE_REQUIRE(A && W && out, "gemm_batched: null pointer");
  HIPIE_REQUIRE(out_fmt == HIPIE_F32 || out_fmt == HIPIE_HL8, "gemm_batched: output format %d (HIPIE_F32 | HIPIE_HL8)", out_fmt);
  HIPIE_REQUIRE(M > 0 && N > 0 && K > 0 && N % 8 == 0 && K % 32 == 0, "gemm_batched: M=%d N=%d K=%d (N %% 8, K %% 32)", M, N, K);
  HIPIE_TRY(gm_check_batch_shape("gemm_batched", n_outer, n_inner));
  HIPIE_TRY(gm_check_operands("gemm_batched", lda, ldw, 2 * K, 320));
  HIPIE_TRY(gm_check_out("gemm_batched", ldo, out_fmt, N));
  HIPIE_TRY(gm_check_batch_offsets("gemm_batched", a_outer, a_inner, w_outer, w_inner, o_outer, o_inner));
  HIPIE_TRY(gm_check_aligned("gemm_batched", {A, W, out}));
  GemmParams p;
  gm_set_operands(p, A, lda, W, ldw, M, N, K);
  gm_set_batch(p, n_inner, a_outer, a_inner, w_outer, w_inner, o_outer, o_inner, out_fmt == HIPIE_F32 ? 4 : 2);
  p.out = (char*)out; p.ldo = ldo; p.out_fmt = out_fmt; p.alpha = alpha;
  hipStream_t st = (hipStream_t)stream;
  const int batches = n_outer * n_inner;
#ifdef HIPIE_GEMM_VARIANTS
  if (gemm2_mode() == 1) return (N % 160 == 0) ? launch_gemm2<5, 0>(p, st, batches) : launch_gemm2<4, 0>(p, st, batches);
#endif
  return (N % 320 == 0) ? launch_gemm<320, true>(p, st, batches) : launch_gemm<256, true>(p, st, batches);
}

// the batched launch of the PLAIN fp16 instances hipie_gemm runs for HIPIE_F16 operands (one product, 64-element k tiles), fp32 output, with
// the device factor of hipie_gemm_scaled: the chunks of a split-K weight gradient of the half-precision training linears.  No new kernel
// instance: gemm_kernel<320 | 256, false> reads the batch offsets and alpha_dev as every instance does.
extern "C" int hipie_gemm_batched_f16(const void* A, int64_t lda, int64_t a_outer, int64_t a_inner, const void* W, int64_t ldw, int64_t w_outer,
                                      int64_t w_inner, void* out, int64_t ldo, int64_t o_outer, int64_t o_inner, int n_outer, int n_inner, int M,
                                      int N, int K, float alpha, const float* alpha_dev, void* stream) {
  HIPIE_REQUIRE(A && W && out, "gemm_batched_f16: null pointer");
  HIPIE_REQUIRE(M > 0 && N > 0 && K > 0 && N % 8 == 0 && K % 64 == 0, "gemm_batched_f16: M=%d N=%d K=%d (N %% 8, K %% 64)", M, N, K);
  HIPIE_TRY(gm_check_batch_shape("gemm_batched_f16", n_outer, n_inner));
  HIPIE_TRY(gm_check_operands("gemm_batched_f16", lda, ldw, K, 320));
  HIPIE_TRY(gm_check_out("gemm_batched_f16", ldo, HIPIE_F32, N));
  HIPIE_TRY(gm_check_batch_offsets("gemm_batched_f16", a_outer, a_inner, w_outer, w_inner, o_outer, o_inner));
  HIPIE_TRY(gm_check_aligned("gemm_batched_f16", {A, W, out}));
  HIPIE_REQUIRE(((uintptr_t)alpha_dev % 4) == 0, "gemm_batched_f16: alpha_dev must be 4-byte aligned");
  GemmParams p;
  gm_set_operands(p, A, lda, W, ldw, M, N, K, 64);
  gm_set_batch(p, n_inner, a_outer, a_inner, w_outer, w_inner, o_outer, o_inner, 4);
  p.out = (char*)out; p.ldo = ldo; p.out_fmt = HIPIE_F32; p.alpha = alpha; p.alpha_dev = alpha_dev;
  hipStream_t st = (hipStream_t)stream;
  const int batches = n_outer * n_inner;
  return (N % 320 == 0) ? launch_gemm<320, false>(p, st, batches) : launch_gemm<256, false>(p, st, batches);
}

extern "C" int hipie_gemm_batched_resid(const void* A, int64_t lda, int64_t a_outer, int64_t a_inner, const void* W, int64_t ldw, int64_t w_outer,
                                        int64_t w_inner, const float* bias, const float* resid, int64_t ldr, int64_t r_outer, int64_t r_inner,
                                        float* out, int64_t ldo, int64_t o_outer, int64_t o_inner, int n_outer, int n_inner, int M, int N, int K,
                                        float alpha, void* stream) {
  HIPIE_REQUIRE(A && W && out, "gemm_batched_resid: null pointer");
  HIPIE_REQUIRE(M > 0 && N > 0 && K > 0 && N % 8 == 0 && K % 32 == 0, "gemm_batched_resid: M=%d N=%d K=%d (N %% 8, K %% 32)", M, N, K);
  HIPIE_TRY(gm_check_batch_shape("gemm_batched_resid", n_outer, n_inner));
  HIPIE_TRY(gm_check_operands("gemm_batched_resid", lda, ldw, 2 * K, 320));
  HIPIE_TRY(gm_check_out("gemm_batched_resid", ldo, HIPIE_F32, N));
  HIPIE_REQUIRE(resid == nullptr || (ldr >= N && ldr % 4 == 0 && ((r_outer | r_inner) % 4) == 0), "gemm_batched_resid: residual strides %ld / %ld / %ld",
                (long)ldr, (long)r_outer, (long)r_inner);
  HIPIE_TRY(gm_check_batch_offsets("gemm_batched_resid", a_outer, a_inner, w_outer, w_inner, o_outer, o_inner));
  HIPIE_TRY(gm_check_aligned("gemm_batched_resid", {A, W, out, bias, resid}));
  GemmParams p;
  gm_set_operands(p, A, lda, W, ldw, M, N, K);
  gm_set_batch(p, n_inner, a_outer, a_inner, w_outer, w_inner, o_outer, o_inner, 4);
  p.out = (char*)out; p.ldo = ldo; p.alpha = alpha;
  p.bias = bias; p.resid = resid; p.ldr = ldr; p.r_bo = r_outer; p.r_bi = r_inner;
  return (N % 320 == 0) ? launch_gemm<320, true>(p, (hipStream_t)stream, n_outer * n_inner) : launch_gemm<256, true>(p, (hipStream_t)stream, n_outer * n_inner);
}

extern "C" int hipie_gemm_batched_softmax(const void* A, int64_t lda, int64_t a_outer, int64_t a_inner, const void* W, int64_t ldw, int64_t w_outer,
                                          int64_t w_inner, void* out, int64_t ldo, int64_t o_outer, int64_t o_inner, int n_outer, int n_inner,
                                          int M, int N, int K, const unsigned char* mask, int L, float clamp, float alpha, void* stream) {
  HIPIE_REQUIRE(A && W && out, "gemm_batched_softmax: null pointer");
  HIPIE_REQUIRE(M > 0 && N > 0 && N <= 256 && N % 8 == 0 && K > 0 && K % 32 == 0 && L > 0 && L <= N,
                "gemm_batched_softmax: M=%d N=%d K=%d L=%d (N <= 256: the row must fit one column tile)", M, N, K, L);
  HIPIE_TRY(gm_check_batch_shape("gemm_batched_softmax", n_outer, n_inner));
  HIPIE_TRY(gm_check_operands("gemm_batched_softmax", lda, ldw, 2 * K, 320));
  HIPIE_TRY(gm_check_out("gemm_batched_softmax", ldo, HIPIE_HL8, N));
  HIPIE_TRY(gm_check_batch_offsets("gemm_batched_softmax", a_outer, a_inner, w_outer, w_inner, o_outer, o_inner));
  HIPIE_TRY(gm_check_aligned("gemm_batched_softmax", {A, W, out}));
  GemmParams p;
  gm_set_operands(p, A, lda, W, ldw, M, N, K);
  gm_set_batch(p, n_inner, a_outer, a_inner, w_outer, w_inner, o_outer, o_inner, 2);
  p.out = (char*)out; p.ldo = ldo; p.out_fmt = HIPIE_HL8; p.alpha = alpha;
  p.softmax = 1; p.sm_L = L; p.sm_clamp = clamp; p.sm_mask = mask;
  return launch_gemm<256, true>(p, (hipStream_t)stream, n_outer * n_inner);
}

extern "C" int hipie_conv3x3_split(const void* x, int64_t ldx, const void* w, const float* bias, void* out, int64_t ldo, int64_t rows, int Wp,
                                   int C, int N, int in_fmt, int out_fmt, int act, void* stream) {
  HIPIE_REQUIRE(x && w && out, "conv3x3_split: null pointer");
  HIPIE_REQUIRE(in_fmt == HIPIE_HL8 || in_fmt == HIPIE_F32, "conv3x3_split: input format %d (HIPIE_HL8 | HIPIE_F32 rows)", in_fmt);
  HIPIE_REQUIRE(out_fmt == HIPIE_F32 || out_fmt == HIPIE_HL8, "conv3x3_split: output format %d (HIPIE_F32 | HIPIE_HL8)", out_fmt);
  HIPIE_REQUIRE(act >= 0 && act <= 2, "conv3x3_split: activation %d", act);
  HIPIE_REQUIRE(rows > 0 && rows < (1L << 31) && Wp >= 3 && C > 0 && C % 32 == 0 && N > 0 && N % 8 == 0, "conv3x3_split: rows=%ld Wp=%d C=%d N=%d",
                (long)rows, Wp, C, N);
  if (in_fmt == HIPIE_F32) ldx *= 2;                 // from here on in fp16 units (the same bytes per row as HL8)
  HIPIE_REQUIRE(ldx >= 2 * C && ldx % 8 == 0, "conv3x3_split: input row stride %ld", (long)ldx);
  HIPIE_REQUIRE((long)(256 + Wp + 2) * ldx * 2 < (1L << 31), "conv3x3_split: row stride too large");
  HIPIE_TRY(gm_check_out("conv3x3_split", ldo, out_fmt, N));
  HIPIE_TRY(gm_check_aligned("conv3x3_split", {x, w, out, bias}));
  GemmParams p;
  gm_set_operands(p, x, ldx, w, (long)2 * 9 * C, (int)rows, N, 9 * C);      // w rows are dense: 2 x 9 C fp16 elements
  p.bias = bias; p.out = (char*)out; p.ldo = ldo; p.out_fmt = out_fmt; p.act = act;
  p.conv_kpt = C / 32; p.conv_wp = Wp;
  hipStream_t st = (hipStream_t)stream;
  const bool wide = (N % 320 == 0);
  if (in_fmt == HIPIE_F32) return wide ? launch_gemm<320, true, 2>(p, st) : launch_gemm<256, true, 2>(p, st);
  return wide ? launch_gemm<320, true>(p, st) : launch_gemm<256, true>(p, st);
}

extern "C" int hipie_to_hl8(const void* x, int64_t ldx, void* out, int64_t ldo, int64_t rows, int K, int x_dtype, float scale, void* stream) {
  HIPIE_REQUIRE(x && out && rows > 0 && K > 0 && K % 8 == 0, "to_hl8: rows=%ld K=%d (K must be a multiple of 8)", (long)rows, K);
  HIPIE_REQUIRE(ldx >= K && ldo >= 2 * K && ldo % 8 == 0, "to_hl8: row strides %ld / %ld", (long)ldx, (long)ldo);
  const long n = rows * (K / 8);
  const dim3 grid((unsigned)((n + 255) / 256));
  hipStream_t st = (hipStream_t)stream;
  switch (x_dtype) {
    case HIPIE_F32: hipLaunchKernelGGL(to_hl8_kernel<float>, grid, dim3(256), 0, st, (const float*)x, (f16_t*)out, rows, K, ldx, ldo, scale); break;
    case HIPIE_F16: hipLaunchKernelGGL(to_hl8_kernel<f16_t>, grid, dim3(256), 0, st, (const f16_t*)x, (f16_t*)out, rows, K, ldx, ldo, scale); break;
    default: return set_err(HIPIE_EINVAL, "to_hl8: dtype %d", x_dtype);
  }
  return check_launch("to_hl8");
}

extern "C" int hipie_to_hl8_t(const void* x, int64_t ldx, void* out, int64_t ldo, int64_t rows, int C, int64_t rows_p, float scale, void* stream) {
  HIPIE_REQUIRE(x && out && rows > 0 && C > 0, "to_hl8_t: rows=%ld C=%d", (long)rows, C);
  HIPIE_REQUIRE(rows_p >= rows && rows_p % 8 == 0 && ldx >= C && ldo >= 2 * rows_p && ldo % 8 == 0, "to_hl8_t: rows_p=%ld (>= rows, multiple of 8), strides %ld / %ld",
                (long)rows_p, (long)ldx, (long)ldo);
  HIPIE_REQUIRE(((uintptr_t)out % 16) == 0, "to_hl8_t: output must be 16-byte aligned");
  const long tiles_r = (rows_p + kTrRows - 1) / kTrRows, tiles_c = (C + kTrCols - 1) / kTrCols;
  HIPIE_REQUIRE(tiles_c <= 65535, "to_hl8_t: C=%d too wide", C);
  hipLaunchKernelGGL(to_hl8_t_kernel, dim3((unsigned)tiles_r, (unsigned)tiles_c), dim3(256), 0, (hipStream_t)stream, (const float*)x, (f16_t*)out,
                     (long)rows, C, (long)ldx, (long)ldo, (long)rows_p, scale);
  return check_launch("to_hl8_t");
}
