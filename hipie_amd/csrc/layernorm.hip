// layernorm.hip -- fused residual-add + LayerNorm + cast (glue kernel, HBM-bound).
//
//   s = x + delta (delta optional);  res_out = s (optional, dtype of x);  norm_out = LN(s) * gamma + beta  (dtype Tn)
//
// Replaces the add -> LayerNorm -> cast chains around every ViT block (hipie/backbone/vit.py:212-230, eps 1e-6) and the
// post-norm residuals of the deformable encoder layers (deformable_transformer_dino.py:384-394), which in eager PyTorch
// are 2-3 separate elementwise passes over the (B, tokens, C) stream.  One wave owns one row: the row is read once (8-byte
// vector loads), statistics are fp32 wave reductions (two-pass: mean, then centred variance -- the same arithmetic as
// torch's layer_norm), and both outputs are written once.  Bytes per row: C * (|x| + |delta| + |res| + |norm|).
#include "common.h"
#include "row_norm.h"

namespace hipie {

// HIPIE_HL8 as an OUTPUT (or addend) type of these kernels.  An HL8 row of C values occupies 4 C bytes like an fp32 row, so the kernels'
// element indexing (row * C + c, 4-byte elements) lands on the right row; inside the row the 4 consecutive values of a lane (c % 8 is 0
// or 4) live at bytes 32 (c / 8) + 2 (c % 8) (hi) and + 16 (lo).  With p = base + 4 c that is p / p + 16 for c % 8 == 0 and p - 8 / p + 8 for
// c % 8 == 4 (bit 4 of p: the rows are 32-byte aligned because C % 8 == 0 and torch allocations are).
struct hl8_t { unsigned int u; };
template <> struct Vec4<hl8_t> {
  static __device__ __forceinline__ void load(const hl8_t* p, float (&v)[4]) {
    const char* q = reinterpret_cast<const char*>(p);
    const bool second = (reinterpret_cast<uintptr_t>(q) & 16) != 0;
    const f16x4 h = *reinterpret_cast<const f16x4*>(second ? q - 8 : q);
    const f16x4 l = *reinterpret_cast<const f16x4*>(second ? q + 8 : q + 16);
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = (float)h[i] + (float)l[i];
  }
  static __device__ __forceinline__ void store(hl8_t* p, const float (&v)[4]) {
    char* q = reinterpret_cast<char*>(p);
    const bool second = (reinterpret_cast<uintptr_t>(q) & 16) != 0;
    f16x4 h, l;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      f16_t hh, ll;
      hl_split(v[i], hh, ll);
      h[i] = hh;
      l[i] = ll;
    }
    *reinterpret_cast<f16x4*>(second ? q - 8 : q) = h;
    *reinterpret_cast<f16x4*>(second ? q + 8 : q + 16) = l;
  }
};

template <typename Tx, typename Td, typename Tn>
__global__ __launch_bounds__(256) void add_layernorm_kernel(const Tx* __restrict__ x, const Td* __restrict__ delta,
                                                            const float* __restrict__ gamma, const float* __restrict__ beta,
                                                            Tx* __restrict__ res_out, Tn* __restrict__ norm_out, long rows,
                                                            int C, float eps, const int32_t* __restrict__ delta_row,
                                                            const int32_t* __restrict__ out_src, const Tn* __restrict__ addend,
                                                            Tn* __restrict__ sum_out) {
  // row maps (both optional): the wave owns OUTPUT row `orow`; it normalises x row `row = out_src[orow]` (-1: the output row
  // is padding -> zeros, e.g. the pad tokens of window_partition) and adds delta row `delta_row[row]` (e.g. the window
  // layout the attention wrote) -- window partition / un-partition become index arithmetic of this pass
  const long orow = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (orow >= rows) return;
  const LnRow r(C);
  const long row = out_src ? (long)out_src[orow] : orow;
  if (row < 0) {
    const float z[4] = {0.f, 0.f, 0.f, 0.f};
    for (int i = 0; i <= r.nv; ++i)        // LnRow::on(i) for i <= nv, spelled out: with on(i) this cold loop is unrolled LN_MAXV times
      if ((i < r.nv)|| (r.lane < r.tail)) Vec4<Tn>::store(norm_out + orow * C + r.col(i), z);
    return;
  }
  const long drow = delta_row ? (long)delta_row[row] : row;
  float v[LN_MAXV][4];
  float sum = 0.f;
  const Tx* xr = x + row * C;
#pragma unroll
  for (int i = 0; i < LN_MAXV; ++i) {
    if (r.on(i)) {
      const int c = r.col(i);
      Vec4<Tx>::load(xr + c, v[i]);
      if (delta != nullptr) {
        float d[4];
        Vec4<Td>::load(delta + drow * C + c, d);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[i][e] += d[e];
      }
      if (res_out != nullptr) Vec4<Tx>::store(res_out + row * C + c, v[i]);
#pragma unroll
      for (int e = 0; e < 4; ++e) sum += v[i][e];
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) v[i][e] = 0.f;
    }
  }
  // ln_row_stats of row_norm.h, written out: through the helper this kernel measured 9 - 12 % slower at C = 256 (docs/measurements.md)
  sum = wave_sum(sum);
  const float mean = sum / (float)C;
  float sq = 0.f;
#pragma unroll
  for (int i = 0; i < LN_MAXV; ++i) {
    if (r.on(i)) {
#pragma unroll
      for (int e = 0; e < 4; ++e) { const float d = v[i][e] - mean; sq += d * d; }
    }
  }
  sq = wave_sum(sq);
  const float rstd = rsqrtf(sq / (float)C + eps);
#pragma unroll
  for (int i = 0; i < LN_MAXV; ++i) {
    if (r.on(i)) {
      const int c = r.col(i);
      float o[4];
      ln_affine(v[i], mean, rstd, gamma + c, beta + c, o);
      Vec4<Tn>::store(norm_out + orow * C + c, o);
      if (sum_out != nullptr) {               // the normalised row plus a second addend (e.g. the position embedding of the next query)
        float a[4];
        Vec4<Tn>::load(addend + orow * C + c, a);
#pragma unroll
        for (int e = 0; e < 4; ++e) a[e] += o[e];
        Vec4<Tn>::store(sum_out + orow * C + c, a);
      }
    }
  }
}

// one call of add_layernorm_kernel, as the three entry points fill it in: what all of them take, then the optional arguments (null = absent)
struct LnArgs {
  const void* x; const void* delta; const float* gamma; const float* beta; void* res_out; void* norm_out;
  long rows; int C; float eps;
  int x_dtype, delta_dtype, norm_dtype;
  hipStream_t stream;
  const int32_t* delta_row = nullptr; const int32_t* out_src = nullptr;       // row maps (see the kernel)
  const void* addend = nullptr; void* sum_out = nullptr;                      // second output: norm_out + addend
};

template <typename Tx, typename Td, typename Tn>
static int launch_ln(const LnArgs& a) {
  hipLaunchKernelGGL((add_layernorm_kernel<Tx, Td, Tn>), dim3((unsigned)((a.rows + 3) / 4)), dim3(256), 0, a.stream, (const Tx*)a.x,
                     (const Td*)a.delta, a.gamma, a.beta, (Tx*)a.res_out, (Tn*)a.norm_out, a.rows, a.C, a.eps, a.delta_row, a.out_src,
                     (const Tn*)a.addend, (Tn*)a.sum_out);
  return check_launch("add_layernorm");
}

static int add_layernorm(const LnArgs& a) {
  HIPIE_REQUIRE(a.x && a.gamma && a.beta && a.norm_out, "add_layernorm: null pointer");
  HIPIE_REQUIRE(a.rows >= 0 && a.C > 0 && a.C % 4 == 0 && a.C <= LN_MAXV * 256, "add_layernorm: C=%d must be a multiple of 4 and <= %d", a.C, LN_MAXV * 256);
  if (a.rows == 0) return HIPIE_OK;
  return with_dtype(a.x_dtype, "add_layernorm: bad x dtype", [&](auto tx) {
    return with_dtype(a.delta_dtype, "add_layernorm: bad delta dtype", [&](auto td) {
      using Tx = decltype(tx);
      using Td = decltype(td);
      if (a.norm_dtype == HIPIE_HL8) {
        if (a.C % 8 != 0 || (reinterpret_cast<uintptr_t>(a.norm_out) & 31) != 0) return set_err(HIPIE_EINVAL, "add_layernorm: HL8 output needs C %% 8 == 0 and a 32-byte aligned buffer");
        return launch_ln<Tx, Td, hl8_t>(a);
      }
      return with_dtype(a.norm_dtype, "add_layernorm: bad norm dtype", [&](auto tn) { return launch_ln<Tx, Td, decltype(tn)>(a); });
    });
  });
}


// Post-norm residual of the DINO decoder layers with an fp32 query stream and 16-bit GEMMs: the LayerNorm output leaves once in
// fp32 (the next residual) and, in the same pass, as the 16-bit operands of the GEMMs that follow: a plain copy (value / FFN /
// box-head input) and / or the copy with the positional query added (the query of the next attention).  Replaces the
// add -> cast chains between the launches of a decoder layer (deformable_transformer_dino.py:418-450).
template <typename Td, typename Ta>
__global__ __launch_bounds__(256) void add_layernorm_dec_kernel(const float* __restrict__ x, const Td* __restrict__ delta,
                                                                const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                float* __restrict__ norm_out, Ta* __restrict__ norm16,
                                                                const Ta* __restrict__ addend, Ta* __restrict__ sum16, long rows,
                                                                int C, float eps) {
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const LnRow r(C);
  float v[LN_MAXV][4];
  float sum = 0.f;
#pragma unroll
  for (int i = 0; i < LN_MAXV; ++i) {
    if (r.on(i)) {
      const long c = row * C + r.col(i);
      float d[4];
      Vec4<float>::load(x + c, v[i]);
      Vec4<Td>::load(delta + c, d);
#pragma unroll
      for (int e = 0; e < 4; ++e) { v[i][e] += d[e]; sum += v[i][e]; }
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) v[i][e] = 0.f;
    }
  }
  float mean, rstd;
  ln_row_stats(r, v, sum, C, eps, mean, rstd);
#pragma unroll
  for (int i = 0; i < LN_MAXV; ++i) {
    if (r.on(i)) {
      const int cc = r.col(i);
      const long c = row * C + cc;
      float o[4];
      ln_affine(v[i], mean, rstd, gamma + cc, beta + cc, o);
      Vec4<float>::store(norm_out + c, o);
      if (norm16 != nullptr) Vec4<Ta>::store(norm16 + c, o);
      if (sum16 != nullptr) {
        float a[4];
        Vec4<Ta>::load(addend + c, a);
#pragma unroll
        for (int e = 0; e < 4; ++e) a[e] += o[e];
        Vec4<Ta>::store(sum16 + c, a);
      }
    }
  }
}

template <typename Td, typename Ta>
static int launch_ln_dec(const float* x, const void* d, const float* g, const float* b, float* n, void* n16, const void* add,
                         void* s16, long rows, int C, float eps, hipStream_t st) {
  hipLaunchKernelGGL((add_layernorm_dec_kernel<Td, Ta>), dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st, x, (const Td*)d, g, b,
                     n, (Ta*)n16, (const Ta*)add, (Ta*)s16, rows, C, eps);
  return check_launch("add_layernorm_dec");
}

// out = (Ta)(a + b): the positional query added to the fp32 stream, rounded once to the GEMM operand type
template <typename Ta>
__global__ __launch_bounds__(256) void add_cast_kernel(const float* __restrict__ a, const Ta* __restrict__ b, Ta* __restrict__ out, long n4) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n4) return;
  float x[4], y[4];
  Vec4<float>::load(a + 4 * i, x);
  Vec4<Ta>::load(b + 4 * i, y);
#pragma unroll
  for (int e = 0; e < 4; ++e) x[e] += y[e];
  Vec4<Ta>::store(out + 4 * i, x);
}

}  // namespace hipie

extern "C" int hipie_add_layernorm(const void* x, const void* delta, const float* gamma, const float* beta, void* res_out,
                                   void* norm_out, int64_t rows, int C, float eps, int x_dtype, int delta_dtype,
                                   int norm_dtype, void* stream) {
  return hipie::add_layernorm({x, delta, gamma, beta, res_out, norm_out, rows, C, eps, x_dtype, delta_dtype, norm_dtype, (hipStream_t)stream});
}

extern "C" int hipie_add_layernorm_rows(const void* x, const void* delta, const float* gamma, const float* beta,
                                        void* res_out, void* norm_out, int64_t out_rows, int C, float eps, int x_dtype,
                                        int delta_dtype, int norm_dtype, const int32_t* delta_row, const int32_t* out_src,
                                        void* stream) {
  hipie::LnArgs a = {x, delta, gamma, beta, res_out, norm_out, out_rows, C, eps, x_dtype, delta_dtype, norm_dtype, (hipStream_t)stream};
  a.delta_row = delta_row;
  a.out_src = out_src;
  return hipie::add_layernorm(a);
}

extern "C" int hipie_add_layernorm_dec(const float* x, const void* delta, const float* gamma, const float* beta, float* norm_out,
                                       void* norm16_out, const void* addend, void* sum16_out, int64_t rows, int C, float eps,
                                       int delta_dtype, int aux_dtype, void* stream) {
  using namespace hipie;
  HIPIE_REQUIRE(x && delta && gamma && beta && norm_out, "add_layernorm_dec: null pointer");
  HIPIE_REQUIRE((sum16_out == nullptr) || (addend != nullptr), "add_layernorm_dec: sum16_out needs addend");
  HIPIE_REQUIRE(rows >= 0 && C > 0 && C % 4 == 0 && C <= LN_MAXV * 256, "add_layernorm_dec: C=%d must be a multiple of 4 and <= %d", C, LN_MAXV * 256);
  HIPIE_REQUIRE(aux_dtype == HIPIE_F16 || aux_dtype == HIPIE_BF16 || aux_dtype == HIPIE_HL8, "add_layernorm_dec: aux dtype must be f16, bf16 or HL8");
  HIPIE_REQUIRE(aux_dtype != HIPIE_HL8 || (C % 8 == 0 && (((uintptr_t)norm16_out | (uintptr_t)addend | (uintptr_t)sum16_out) & 31) == 0),
                "add_layernorm_dec: HL8 outputs need C %% 8 == 0 and 32-byte aligned buffers");
  if (rows == 0) return HIPIE_OK;
  hipStream_t st = (hipStream_t)stream;
  return with_dtype(delta_dtype, "add_layernorm_dec: bad delta dtype", [&](auto td) {
    auto launch = [&](auto ta) {
      return launch_ln_dec<decltype(td), decltype(ta)>(x, delta, gamma, beta, norm_out, norm16_out, addend, sum16_out, rows, C, eps, st);
    };
    return aux_dtype == HIPIE_F16 ? launch(f16_t()) : aux_dtype == HIPIE_HL8 ? launch(hl8_t()) : launch(bf16_t());
  });
}

extern "C" int hipie_add_cast(const float* a, const void* b, void* out, int64_t n, int dtype, void* stream) {
  using namespace hipie;
  HIPIE_REQUIRE(a && b && out, "add_cast: null pointer");
  HIPIE_REQUIRE(n >= 0 && n % 4 == 0, "add_cast: n must be a multiple of 4");
  HIPIE_REQUIRE(dtype == HIPIE_F16 || dtype == HIPIE_BF16 || dtype == HIPIE_HL8, "add_cast: dtype must be f16, bf16 or HL8");
  HIPIE_REQUIRE(dtype != HIPIE_HL8 || (n % 8 == 0 && (((uintptr_t)b | (uintptr_t)out) & 31) == 0), "add_cast: HL8 needs n %% 8 == 0 and 32-byte aligned buffers");
  if (n == 0) return HIPIE_OK;
  hipStream_t st = (hipStream_t)stream;
  const long n4 = n / 4;
  const unsigned grid = (unsigned)((n4 + 255) / 256);
  auto launch = [&](auto t) {
    using Ta = decltype(t);
    hipLaunchKernelGGL((add_cast_kernel<Ta>), dim3(grid), dim3(256), 0, st, a, (const Ta*)b, (Ta*)out, n4);
  };
  if (dtype == HIPIE_HL8) launch(hl8_t());
  else if (dtype == HIPIE_F16) launch(f16_t());
  else launch(bf16_t());
  return check_launch("add_cast");
}

extern "C" int hipie_add_layernorm_sum(const void* x, const void* delta, const float* gamma, const float* beta, void* res_out,
                                       void* norm_out, const void* addend, void* sum_out, int64_t rows, int C, float eps,
                                       int x_dtype, int delta_dtype, int norm_dtype, void* stream) {
  using namespace hipie;
  HIPIE_REQUIRE((addend == nullptr) == (sum_out == nullptr), "add_layernorm_sum: addend and sum_out go together");
  LnArgs a = {x, delta, gamma, beta, res_out, norm_out, rows, C, eps, x_dtype, delta_dtype, norm_dtype, (hipStream_t)stream};
  a.addend = addend;
  a.sum_out = sum_out;
  return add_layernorm(a);
}
