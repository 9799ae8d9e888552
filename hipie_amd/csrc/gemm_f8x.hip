// gemm_f8x.hip -- hipie_gemm_f8x: the split GEMM with its two CROSS terms on block-scaled FP8 (the opt-in `fp8x` precision policy)
//
//     out = epilogue( W_hi . X_hi  +  q8(W_lo) . q8(X_hi)  +  q8(W_hi) . q8(X_lo) )            fp32 accumulation
//
// hipie_gemm forms an fp32-class product from three fp16 MFMAs (gemm_tile.h).  The two cross terms are 2^-11 of the main term, so their
// operands need ~5 bits: here they are e4m3 with one power-of-two (E8M0) scale per 32 k-elements (q8, hipie_amd/fp8x.py has the exact rule)
// and run on v_mfma_scale_f32_32x32x64_f8f6f4, which takes e4m3 at twice the fp16 rate.  Per (feature block, token tile) and 32-element k
// stage: two v_mfma_f32_32x32x16_f16 for W_hi . X_hi and ONE scaled MFMA for both cross terms, concatenated along its K = 64:
//     [ q8(W_lo) | q8(W_hi) ] . [ q8(X_hi) ; q8(X_lo) ]
// Operand lane map of the scaled MFMA (32 bytes of e4m3 per lane, found on the hardware: the contiguous reading, lane half h = k 32 h ..
// 32 h + 31, puts part of every product under the other block's scale): bytes 0-15 of BOTH lane halves form k block 0 and bytes 16-31
// k block 1, whose E8M0 scale comes from lane half 0 / 1 of the row (column).  So every lane carries 16 values of the W_lo / X_hi term in
// bytes 0-15 and 16 of the W_hi / X_lo term in bytes 16-31, the products pair by position, and lane half h supplies that row's (column's)
// scale of term h.  2 + 2 fp16-equivalents per stage instead of 6; nothing crosses a stage boundary.
//
// Operands (include/hipie_mi355.h):
//   X  ordinary HL8 rows (the GELU epilogue of fc1 writes them; no producer changes), quantised in the kernel, in registers: lane half h
//      already holds hi and lo of the 8-groups h and h + 2 of its token (the main term's fragments), so a block's amax is the lane's 16
//      values and one exchange with the partner lane (xor 32); then 8 packed conversions per part (f8x_amax16 / f8x_scale / f8x_cvt16, the
//      device functions hipie_to_f8x runs).
//   W  the f8x weight format: every 32-element k slice of a row is 128 bytes like an HL8 slice, hi fp16 [64 B] then 64 B of e4m3 in the lane
//      order above: [q8(lo) g0 g2 | q8(hi) g0 g2 | q8(lo) g1 g3 | q8(hi) g1 g3] (8 bytes per 8-group g), and a side tensor (N, K/32, 2) of
//      E8M0 scales [lo, hi].  Stage size, LDS-DMA and swizzle are gemm_kernel's.
// The tile (256 x 256, 8 waves, 2 LDS stages of 128-byte k32 rows, XCD tile order) and the epilogue (gm_epi_quads) are gemm_tile.h's.
#include "gemm_tile.h"

namespace hipie {

typedef int i32x8 __attribute__((ext_vector_type(8)));

// q8 of a 32-element block (hipie_amd/fp8x.py has the exact rule): e = the largest integer with amax * 2^e <= 448 (amax = 0: e = 0), clamped
// to [-127, 127]; code = RNE e4m3fn(v * 2^e); scale byte = 127 - e, i.e. the value is code * 2^(byte - 127).
// f8x_amax16: the 15-bit magnitude bits of 16 fp16 values (two per register): |fp16| compares as an unsigned integer, so packed u16 maxima.
__device__ __forceinline__ unsigned int f8x_amax16(const unsigned int (&v)[8]) {
  typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
  u16x2 m = __builtin_bit_cast(u16x2, v[0] & 0x7FFF7FFFu);
#pragma unroll
  for (int i = 1; i < 8; ++i) m = __builtin_elementwise_max(m, __builtin_bit_cast(u16x2, v[i] & 0x7FFF7FFFu));
  return m[0] > m[1] ? m[0] : m[1];
}

// block amax bits -> scale byte (returned) and the conversion's scale operand sc.  amax = 2^x * f with f in [0.5, 1): f <= 0.875 gives
// e = 9 - x, else 8 - x.  v_cvt_scalef32_pk_fp8_f16 DIVIDES by its scale operand (only the operand's exponent is used; pinned bit for bit by
// tests/test_gpu_fp8x.py): 2^-e, whose exponent field is the scale byte itself.
__device__ __forceinline__ unsigned int f8x_scale(const unsigned int amax_bits, float& sc) {
  const float amax = (float)__builtin_bit_cast(f16_t, (unsigned short)amax_bits);
  int e = 0;
  if (amax > 0.f) {
    const int x = __builtin_amdgcn_frexp_expf(amax);
    e = (__builtin_amdgcn_frexp_mantf(amax) <= 0.875f ? 9 : 8) - x;
    e = min(max(e, -127), 127);
  }
  const unsigned int sb = (unsigned int)(127 - e);
  sc = __builtin_bit_cast(float, sb << 23);                       // 2^-e (e <= 32 for fp16 input: a normal float)
  return sb;
}

// 16 fp16 values (two per register, low half first) -> 16 e4m3 codes, byte b = value b
__device__ __forceinline__ void f8x_cvt16(const unsigned int (&v)[8], const float sc, unsigned int (&q)[4]) {
  typedef short i16x2 __attribute__((ext_vector_type(2)));
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    i16x2 w = {0, 0};
    w = __builtin_amdgcn_cvt_scalef32_pk_fp8_f16(w, __builtin_bit_cast(gm_h2, v[2 * i]), sc, false);
    w = __builtin_amdgcn_cvt_scalef32_pk_fp8_f16(w, __builtin_bit_cast(gm_h2, v[2 * i + 1]), sc, true);
    q[i] = __builtin_bit_cast(unsigned int, w);
  }
}

struct F8xParams {
  GemmParams g;
  const unsigned char* wsc = nullptr;   // (N, K/32, 2) E8M0 scales of W's [lo, hi] e4m3 parts
};

template <int BN>
__global__ __launch_bounds__(512, 2) void gemm_f8x_kernel(const F8xParams fp) {
  const GemmParams& p = fp.g;
  constexpr int BM = 256;
  constexpr int ROWS = BM + BN;
  constexpr int STAGE = ROWS * 128;
  constexpr int NI = ROWS / 64;                // DMA instructions per wave and stage
  constexpr int NJ = BN / 64;                  // 32-feature blocks per wave
  typedef Mfma32<f16_t>::frag frag;
  typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
  typedef unsigned short u16x2_t __attribute__((ext_vector_type(2)));

  extern __shared__ __attribute__((aligned(128))) char smem[];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave & 3, wn = wave >> 2;
  const int li = lane & 31, hi = lane >> 5;

  // ---- block -> tile: gemm_kernel's XCD-aware order ----
  int tm, tn;
  {
    const int nblk = p.tiles_m * p.tiles_n;
    const int id = blockIdx.x, xcd = id & 7, j = id >> 3;
    const int q = nblk >> 3, r = nblk & 7;
    const int v = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + j;
    if (p.group_m > 1) {
      const int gsz = p.group_m * p.tiles_n;
      const int g = v / gsz, w = v - g * gsz;
      const int rows = min(p.group_m, p.tiles_m - g * p.group_m);
      tn = w / rows;
      tm = g * p.group_m + (w - tn * rows);
    } else {
      tm = v / p.tiles_n;
      tn = v - tm * p.tiles_n;
    }
  }
  const int m0 = tm * BM, n0 = tn * BN;

  // ---- DMA plan (gemm_kernel's): rows beyond M / N re-read the last row, their results are never stored ----
  unsigned int dvoff[NI];
  {
    const int rl = lane >> 3, cp = lane & 7;
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      const int r = 8 * (8 * i + wave) + rl;
      const int c = cp ^ ((r >> 1) & 7);
      if (r < BM) dvoff[i] = (unsigned int)((long)min(r, p.M - 1 - m0) * p.lda_b + 16 * c);
      else dvoff[i] = (unsigned int)((long)min(r - BM, p.N - 1 - n0) * p.ldw_b + 16 * c);
    }
  }
  const char* abase = p.A + (long)m0 * p.lda_b;
  const char* wbase = p.W + (long)n0 * p.ldw_b;
  const unsigned int lds0 = (unsigned int)reinterpret_cast<uintptr_t>((__attribute__((address_space(3))) char*)smem);
  auto dma = [&](const int i, const int kt, const int stage) {
    const bool isa = (8 * (8 * i + wave)) < BM;
    dma16((isa ? abase : wbase) + (long)kt * 128, dvoff[i],
             __builtin_amdgcn_readfirstlane(lds0 + (unsigned int)(stage * STAGE + 1024 * (8 * i + wave))));
  };

  // W scale bytes of this lane: feature row (n0 + wn BN/2 + 32 j + li), part hi (0: lo, 1: hi) of k block kt
  const int nkb = p.nkt;
  int wsc_off[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) wsc_off[j] = min(n0 + wn * (BN / 2) + j * 32 + li, p.N - 1) * nkb * 2 + hi;

  const int swz = (li >> 1) & 7;
  const char* xrow = smem + (wm * 64 + li) * 128;
  const char* wrow = smem + (BM + wn * (BN / 2) + li) * 128;
  auto coff = [&](const int c) -> int { return 16 * (c ^ swz); };

  f32x16 acc[NJ][2];
#pragma unroll
  for (int j = 0; j < NJ; ++j)
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[j][t][r] = 0.f;

  const int nkt = p.nkt;
#pragma unroll
  for (int i = 0; i < NI; ++i) dma(i, 0, 0);
  unsigned int wsc[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) wsc[j] = fp.wsc[wsc_off[j]];
  __builtin_amdgcn_s_waitcnt(vmcnt(0));
  __syncthreads();

  for (int kt = 0; kt < nkt; ++kt) {
    const int st = kt & 1;
    const bool more = kt + 1 < nkt;
    const char* xs = xrow + st * STAGE;
    const char* ws = wrow + st * STAGE;
    // next stage's W scales (they land with the stage's DMA, before the barrier)
    unsigned int wsn[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) wsn[j] = more ? (fp.wsc + 2 * (kt + 1))[wsc_off[j]] : 0u;

    // ---- X: the main term's hi fragments (k-step s, lane half h: 8-group 2 s + h) and the lo ones; q8 of the token's 32 hi / 32 lo values:
    //      the lane's 16 of each, the block amax with the partner lane half (one lane exchange), 8 + 8 packed conversions ----
    frag xh[2][2];
    i32x8 xq[2];
    unsigned int xsc[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      unsigned int vh[8], vl[8];
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        xh[s][t] = *reinterpret_cast<const frag*>(xs + t * 4096 + coff(2 * (2 * s + hi)));
        const u32x4 h4 = __builtin_bit_cast(u32x4, xh[s][t]);
        const u32x4 l4 = *reinterpret_cast<const u32x4*>(xs + t * 4096 + coff(2 * (2 * s + hi) + 1));
#pragma unroll
        for (int e = 0; e < 4; ++e) { vh[4 * s + e] = h4[e]; vl[4 * s + e] = l4[e]; }
      }
      const unsigned int ah = f8x_amax16(vh), al = f8x_amax16(vl);
      const unsigned int own = (ah << 16) | al;
      const unsigned int partner = (unsigned int)__shfl_xor((int)own, 32);
      const u16x2_t m2 = __builtin_elementwise_max(__builtin_bit_cast(u16x2_t, own), __builtin_bit_cast(u16x2_t, partner));    // (lo, hi)
      float sch, scl;
      const unsigned int sbh = f8x_scale(m2[1], sch), sbl = f8x_scale(m2[0], scl);
      unsigned int qh[4], ql[4];
      f8x_cvt16(vh, sch, qh);
      f8x_cvt16(vl, scl, ql);
      xq[t] = (i32x8){(int)qh[0], (int)qh[1], (int)qh[2], (int)qh[3], (int)ql[0], (int)ql[1], (int)ql[2], (int)ql[3]};
      xsc[t] = hi ? sbl : sbh;                                  // k block 0 = the X_hi term, block 1 = the X_lo term
    }

    // ---- W per feature block j: hi fp16 of k-step s at chunk 2 s + h; lane half h's e4m3 bytes at chunks 4 + 2 h (q8(lo) of 8-groups h, h + 2:
    //      k block 0) and 5 + 2 h (q8(hi) of the same groups: k block 1).
    //      Block j + 1's fragments are requested before block j's MFMAs ----
    frag wh[2][2];
    auto load_wh = [&](const int j) {
#pragma unroll
      for (int s = 0; s < 2; ++s) wh[j & 1][s] = *reinterpret_cast<const frag*>(ws + j * 4096 + coff(2 * s + hi));
    };
    load_wh(0);
    constexpr int DMA_BY = NJ < 3 ? NJ : 3;                      // blocks that carry the next stage's DMA instructions
    constexpr int PER = (NI + DMA_BY - 1) / DMA_BY;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const u32x4 a = *reinterpret_cast<const u32x4*>(ws + j * 4096 + coff(4 + 2 * hi));
      const u32x4 b = *reinterpret_cast<const u32x4*>(ws + j * 4096 + coff(5 + 2 * hi));
      if (j + 1 < NJ) load_wh(j + 1);
      const i32x8 wq = {(int)a[0], (int)a[1], (int)a[2], (int)a[3], (int)b[0], (int)b[1], (int)b[2], (int)b[3]};
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        acc[j][t] = Mfma32<f16_t>::mma(wh[j & 1][0], xh[0][t], acc[j][t]);
        acc[j][t] = Mfma32<f16_t>::mma(wh[j & 1][1], xh[1][t], acc[j][t]);
      }
#pragma unroll
      for (int t = 0; t < 2; ++t)
        acc[j][t] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(wq, xq[t], acc[j][t], 0, 0, 0, (int)wsc[j], 0, (int)xsc[t]);
      if (more) {
#pragma unroll
        for (int i = j * PER; i < (j + 1) * PER && i < NI; ++i) dma(i, kt + 1, st ^ 1);
      }
#if defined(__HIP_DEVICE_COMPILE__)
      __builtin_amdgcn_sched_barrier(0);       // one block's W fragments in flight at a time (hoisted together they spill)
#endif
    }
    __builtin_amdgcn_s_waitcnt(vmcnt(0));      // this wave's DMA writes of stage t+1 (and its scale loads) have landed
#pragma unroll
    for (int j = 0; j < NJ; ++j) wsc[j] = wsn[j];
    __syncthreads();                          // ... and everybody's; all reads of stage t are done
  }

  // ---- epilogue: gemm_kernel's (bias through LDS, residual quads one block ahead, gm_epi_quads) ----
  const bool has_res = p.resid != nullptr;
  float* sbias = reinterpret_cast<float*>(smem);
  if (tid < BN) sbias[tid] = (p.bias != nullptr && n0 + tid < p.N) ? p.bias[n0 + tid] : 0.f;
  __syncthreads();
  float4 rq[2][4];
  long orow[2];
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const int m = m0 + wm * 64 + t * 32 + li;
    orow[t] = (m < p.M) ? (p.out_row != nullptr ? (long)p.out_row[m] : (long)m) : -1;
  }
  auto load_res = [&](const int t, const int j, float4 (&dst)[4]) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int n = n0 + wn * (BN / 2) + j * 32 + 8 * g + 4 * hi;
      dst[g] = (has_res && orow[t] >= 0 && n < p.N) ? *reinterpret_cast<const float4*>(p.resid + orow[t] * p.ldr + n) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
  };
  load_res(0, 0, rq[0]);
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const long m = orow[t];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int blk = t * NJ + j;
      if (blk + 1 < 2 * NJ) load_res((blk + 1) / NJ, (blk + 1) % NJ, rq[(blk + 1) & 1]);
      const int nb = n0 + wn * (BN / 2) + j * 32;
      gm_epi_quads<0, 4>(acc[j][t], rq[blk & 1], sbias + (nb - n0), m, m >= 0, nb, hi, p, has_res);
    }
  }
}

template <int BN>
static int launch_gemm_f8x(F8xParams& fp, hipStream_t st) {
  constexpr size_t lds = (size_t)2 * (256 + BN) * 128;
  GemmParams& p = fp.g;
  p.tiles_m = (p.M + 255) / 256;
  p.tiles_n = (p.N + BN - 1) / BN;
  p.group_m = p.tiles_n > 4 ? 8 : 0;            // launch_gemm's tile order
  auto kern = gemm_f8x_kernel<BN>;
  static LdsLimit limit;
  limit.raise((const void*)kern, lds);
  hipLaunchKernelGGL(kern, dim3((unsigned)(p.tiles_m * p.tiles_n)), dim3(512), lds, st, fp);
  return check_launch("gemm_f8x");
}

// HL8 rows -> q8 of every 32-element block's hi and lo values: one thread per (row, block), the GEMM's amax / scale / conversion functions
__global__ __launch_bounds__(256) void to_f8x_kernel(const char* __restrict__ x, long ldx_b, unsigned char* __restrict__ out, long ldo_b,
                                                     unsigned char* __restrict__ sc, long rows, int nkb) {
  typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
  const long gid = (long)blockIdx.x * 256 + threadIdx.x;
  if (gid >= rows * nkb) return;
  const long r = gid / nkb;
  const int b = (int)(gid - r * nkb);
  const u32x4* src = reinterpret_cast<const u32x4*>(x + r * ldx_b + 128L * b);
  unsigned int vh[2][8], vl[2][8];            // [k 0..15 | k 16..31]
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    const u32x4 h4 = src[2 * g], l4 = src[2 * g + 1];
#pragma unroll
    for (int e = 0; e < 4; ++e) { vh[g >> 1][4 * (g & 1) + e] = h4[e]; vl[g >> 1][4 * (g & 1) + e] = l4[e]; }
  }
  const unsigned int ah = max(f8x_amax16(vh[0]), f8x_amax16(vh[1])), al = max(f8x_amax16(vl[0]), f8x_amax16(vl[1]));
  float sch, scl;
  const unsigned int sh = f8x_scale(ah, sch), sl = f8x_scale(al, scl);
  unsigned int qh[8], ql[8];
  f8x_cvt16(vh[0], sch, *reinterpret_cast<unsigned int(*)[4]>(qh));
  f8x_cvt16(vh[1], sch, *reinterpret_cast<unsigned int(*)[4]>(qh + 4));
  f8x_cvt16(vl[0], scl, *reinterpret_cast<unsigned int(*)[4]>(ql));
  f8x_cvt16(vl[1], scl, *reinterpret_cast<unsigned int(*)[4]>(ql + 4));
  u32x4* dst = reinterpret_cast<u32x4*>(out + r * ldo_b + 64L * b);
  dst[0] = (u32x4){qh[0], qh[1], qh[2], qh[3]};
  dst[1] = (u32x4){qh[4], qh[5], qh[6], qh[7]};
  dst[2] = (u32x4){ql[0], ql[1], ql[2], ql[3]};
  dst[3] = (u32x4){ql[4], ql[5], ql[6], ql[7]};
  *reinterpret_cast<unsigned short*>(sc + 2 * gid) = (unsigned short)(sh | (sl << 8));
}

}  // namespace hipie

using namespace hipie;

extern "C" int hipie_gemm_f8x(const void* A, int64_t lda, const void* W, int64_t ldw, const void* w_scale, const float* bias, const float* resid,
                              int64_t ldr, void* out, int64_t ldo, const int32_t* out_row, int M, int N, int K, int in_fmt, int out_fmt, int act,
                              float alpha, float oscale, void* stream) {
  HIPIE_REQUIRE(A && W && w_scale && out, "gemm_f8x: null pointer");
  HIPIE_REQUIRE(in_fmt == HIPIE_HL8, "gemm_f8x: operand format %d (HL8 activations only)", in_fmt);
  HIPIE_REQUIRE(out_fmt == HIPIE_F32 || out_fmt == HIPIE_F16 || out_fmt == HIPIE_HL8, "gemm_f8x: output format %d", out_fmt);
  HIPIE_REQUIRE(act >= 0 && act <= 3, "gemm_f8x: activation %d (0 none, 1 gelu, 2 relu, 3 quick-gelu)", act);
  HIPIE_REQUIRE(M > 0 && N > 0 && K > 0 && N % 8 == 0 && K % 32 == 0, "gemm_f8x: M=%d N=%d K=%d (N %% 8, K %% 32)", M, N, K);
  HIPIE_TRY(gm_check_operands("gemm_f8x", lda, ldw, 2 * K, 320));
  HIPIE_TRY(gm_check_out("gemm_f8x", ldo, out_fmt, N));
  HIPIE_TRY(gm_check_resid("gemm_f8x", resid, ldr, N));
  HIPIE_TRY(gm_check_aligned("gemm_f8x", {A, W, out, bias, resid}));
  F8xParams fp;
  GemmParams& p = fp.g;
  gm_set_operands(p, A, lda, W, ldw, M, N, K);
  p.bias = bias; p.resid = resid; p.ldr = ldr; p.out = (char*)out; p.ldo = ldo; p.out_row = out_row;
  p.out_fmt = out_fmt; p.act = act; p.alpha = alpha; p.oscale = oscale;
  fp.wsc = (const unsigned char*)w_scale;
  hipStream_t st = (hipStream_t)stream;
  // the 256-column tile for every N: the 320-column one needs ~40 registers more than the 256 a wave has at two waves per SIMD (X's q8 operands,
  // the e4m3 W fragment and the scale bytes stay live beside the 160 accumulators) and would spill
  return launch_gemm_f8x<256>(fp, st);
}

extern "C" int hipie_to_f8x(const void* x, int64_t ldx, void* out, int64_t ldo, void* scale, int64_t rows, int K, void* stream) {
  HIPIE_REQUIRE(x && out && scale, "to_f8x: null pointer");
  HIPIE_REQUIRE(rows > 0 && K > 0 && K % 32 == 0, "to_f8x: rows=%ld K=%d (K must be a multiple of 32)", (long)rows, K);
  HIPIE_REQUIRE(ldx >= 2 * K && ldx % 8 == 0 && ldo >= 2 * K && ldo % 16 == 0, "to_f8x: row strides %ld (fp16) / %ld (bytes)", (long)ldx, (long)ldo);
  HIPIE_REQUIRE(((uintptr_t)x % 16) == 0 && ((uintptr_t)out % 16) == 0 && ((uintptr_t)scale % 2) == 0, "to_f8x: x / out 16-byte, scale 2-byte aligned");
  const long n = rows * (K / 32);
  hipLaunchKernelGGL(to_f8x_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const char*)x, (long)ldx * 2,
                     (unsigned char*)out, (long)ldo, (unsigned char*)scale, (long)rows, K / 32);
  return check_launch("to_f8x");
}
