// attn_train.hip -- the GLOBAL instance of the fused training attention (attn_train_tile.h: the kernels, their dataflow and budget): 224
// operand columns, one 16-row tile per wave, 8 waves = 128 rows per workgroup, N a multiple of 128; and the fp32 -> fp16-pair conversion of
// the operands of both instances.
#include "attn_train_tile.h"

namespace hipie {

constexpr int AT_DQ = 224;          // columns of q' / k' (7 MFMA k-steps of 32)

#ifndef AT_WAVES
#define AT_WAVES 8                  // waves per workgroup: 16 queries (or keys) each
#endif
#ifndef AT_TR
#define AT_TR 32                    // rows of the tile that streams through LDS per step (64: 8.3 ms per block instead of 7.5)
#endif
using AtGlobal = AtCfg<AT_DQ, 1, AT_WAVES, AT_TR, false>;

// fp32 rows -> the two fp16 planes of the operands above, zero-padded to Cp columns and optionally scaled by a DEVICE scalar (dO's power of
// two): one pass instead of pad + clamp + two casts + a subtraction
__global__ __launch_bounds__(256) void to_f16_pair_kernel(const float* __restrict__ x, long ldx, f16_t* __restrict__ hi, f16_t* __restrict__ lo,
                                                          long rows, int C, int Cp, const float* __restrict__ scale) {
  const long gid = (long)blockIdx.x * 256 + threadIdx.x;
  const int cpr = Cp / 8;
  if (gid >= rows * cpr) return;
  const long r = gid / cpr;
  const int c0 = (int)(gid - r * cpr) * 8;
  const float sc = scale ? *scale : 1.f;
  const float* src = x + r * ldx + c0;
  at_frag h, l;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    f16_t hh, ll;
    hl_split(c0 + e < C ? src[e] * sc : 0.f, hh, ll);
    h[e] = hh;
    l[e] = ll;
  }
  *reinterpret_cast<at_frag*>(hi + r * Cp + c0) = h;
  *reinterpret_cast<at_frag*>(lo + r * Cp + c0) = l;
}

}  // namespace hipie

using namespace hipie;

static int at_global_check(const char* who, bool pointers, int BH, int N) {
  return at_check(who, pointers, BH, N, N % 128 == 0 && (long)BH * (N / 128) < (1L << 31), "N a multiple of 128");
}

extern "C" int hipie_attn_train_forward(const void* q_hi, const void* q_lo, const void* k_hi, const void* k_lo, const void* v_hi, const void* v_lo,
                                        void* out, void* lse, int BH, int N, void* stream) {
  HIPIE_TRY(at_global_check("attn_train_forward", q_hi && q_lo && k_hi && k_lo && v_hi && v_lo && out && lse, BH, N));
  AtArgs a{};
  a.q_hi = q_hi, a.q_lo = q_lo, a.k_hi = k_hi, a.k_lo = k_lo, a.v_hi = v_hi, a.v_lo = v_lo, a.out = out, a.lse_out = lse;
  at_forward<AtGlobal>((hipStream_t)stream, (unsigned)((N / AtGlobal::WG_ROWS) * BH), a, BH, N);
  return check_launch("attn_train_forward");
}

extern "C" int hipie_attn_train_backward(const void* q_hi, const void* q_lo, const void* k_hi, const void* k_lo, const void* v_hi, const void* v_lo,
                                         const void* do_hi, const void* do_lo, const void* lse, const void* delta, void* dq, void* dk, void* dv,
                                         int BH, int N, void* stream) {
  HIPIE_TRY(at_global_check("attn_train_backward", q_hi && q_lo && k_hi && k_lo && v_hi && v_lo && do_hi && do_lo && lse && delta && dq && dk && dv,
                            BH, N));
  const AtArgs a{q_hi, q_lo, k_hi, k_lo, v_hi, v_lo, do_hi, do_lo, lse, delta, nullptr, nullptr, dq, dk, dv};
  at_backward<AtGlobal>((hipStream_t)stream, (unsigned)((N / AtGlobal::WG_ROWS) * BH), a, BH, N);
  return check_launch("attn_train_backward");
}

extern "C" int hipie_to_f16_pair(const void* x, int64_t ldx, void* hi, void* lo, int64_t rows, int C, int Cp, const void* scale, void* stream) {
  HIPIE_REQUIRE(x && hi && lo && rows > 0 && C > 0 && Cp >= C && Cp % 8 == 0 && ldx >= C, "to_f16_pair: rows=%ld C=%d Cp=%d ldx=%ld", (long)rows, C, Cp, (long)ldx);
  HIPIE_REQUIRE(((uintptr_t)hi % 16) == 0 && ((uintptr_t)lo % 16) == 0, "to_f16_pair: planes must be 16-byte aligned");
  const long n = rows * (Cp / 8);
  hipLaunchKernelGGL(to_f16_pair_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const float*)x, (long)ldx, (f16_t*)hi,
                     (f16_t*)lo, (long)rows, C, Cp, (const float*)scale);
  return check_launch("to_f16_pair");
}
