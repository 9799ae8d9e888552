// gemm_tile.h -- what gemm.hip, gemm_ln.hip and gemm_f8x.hip share: GemmParams, the tile kernels with their epilogue and launchers, and
// the host helpers that fill and check the parameters.  The kernels are the linears of the path (ViT qkv / proj / fc1 / fc2, BERT, encoder
// / decoder FFNs and projections) as one hand-written MFMA GEMM for gfx950:      out = epilogue( alpha * A (M x K) . W^T (N x K) + bias )
//
// Both operands are K-contiguous (torch.nn.Linear keeps W as (N, K)), so both MFMA fragments are 16-byte row pieces: no
// transposes anywhere.  Two operand formats:
//   HIPIE_F16   one fp16 per element                                                       1 MFMA per tile and k-step
//   HIPIE_HL8   SPLIT fp16: every group of 8 k-elements is stored as 8 fp16 "hi" then 8 fp16 "lo" with hi + lo == x to 2^-22
//               (32 bytes per group = the bytes of fp32).  The product is formed as  W_lo.X_hi + W_hi.X_lo + W_hi.X_hi  with
//               fp32 accumulation: every fp16 x fp16 product is exact in fp32, the dropped lo x lo term is 2^-22 relative, so
//               the result is fp32-class (the reference runs these linears in fp32, hipie/backbone/vit.py:67-83,212-230;
//               deformable_transformer_dino.py:378-394) at 3 MFMAs per k-step on the 16-bit matrix pipe -- gfx950's fp32 MFMA
//               runs at 1/16 of the fp16 rate.  A row's 32-element k slice is one 128-byte line.
//
// Design (MI355X_MICROARCH.md, cdna_hip_programming.md section 5):
//   * workgroup tile 256 (M) x BN (N), BN = 320 | 256, 8 waves as 4 (M) x 2 (N): a wave owns 64 tokens x BN/2 features =
//     2 x (BN/64) MFMA tiles of 32x32 (160 / 128 accumulator registers).  BN = 320 tiles N = 1280 / 3840 / 5120 of ViT-H
//     exactly and makes 512 / 1536 / 2048 workgroups at 32768 tokens = whole waves of the 256 CUs;
//   * the MFMA computes out^T = W . X^T (features are the 32 MFMA rows, tokens the 32 columns), so a lane owns ONE token and
//     4 consecutive features per accumulator quad: bias / activation / residual / split are per-lane vector work and the stores
//     are 16 bytes;
//   * k tile = 128 bytes per row in both formats (64 fp16 elements, or 32 split elements); operand tiles go L2 -> LDS by
//     LDS-DMA (global_load_lds_dwordx4: no staging registers, no ds_write), 2 LDS stages of (256 + BN) x 128 B, one barrier
//     per stage, the DMA instructions of stage t+1 spread between the MFMAs of stage t;
//   * LDS rows are 128 B, which would put a ds_read_b128 lane group on two 16-byte slots (8-way conflict); the 16-byte chunk c
//     of row r is therefore stored at chunk position c ^ ((r >> 1) & 7).  The DMA writes LDS lane-linearly, so the swizzle is
//     applied to the per-lane global SOURCE address; the reader applies the same XOR.  Conflict-free for every b128 lane group;
//   * block -> tile map: the blocks of one XCD (blockIdx % 8) walk a contiguous range of tiles -- N index fastest for up to 4 column
//     tiles, else in groups of 8 row panels with the row panel fastest (GemmParams::group_m) -- so the 32 workgroups resident on an
//     XCD share 8 A row panels and 4 W panels through that XCD's L2.
//   * MS = 16 (gemm_kernel's fourth parameter; BN = 320 split instances only): the same workgroup tile, waves, stages and DMA plan on
//     v_mfma_f32_16x16x32_f16 -- a k32 stage is ONE k-step, a wave owns 4 token tiles x 10 feature tiles of 16 x 16 (the same 160 accumulator
//     registers), lane (c = lane & 15, g = lane >> 4) reads k group g of row c.  The chip holds a higher clock on this shape in a power-
//     limited loop (MI355X_MICROARCH.md, DVFS give-back).  Its LDS image has its own swizzle (gm_swz16): the one above is 2-way for the
//     16 x 4 lane map.  gemm_impl chooses the shape (gemm.hip);
// Epilogue (runtime switches, once per tile): * alpha, + bias, exact-erf GELU | ReLU, + fp32 residual, then the output as
// fp32, fp16 or HL8 (optionally scaled) -- the HL8 form is directly the A operand of the next GEMM.
#pragma once
#include <stdlib.h>

#include <initializer_list>

#include "common.h"
#include "gelu.h"        // gm_gelu: the exact-erf GELU of the epilogue (shared with act_bwd.hip)
#include "mfma.h"
#include "wave.h"

namespace hipie {

// The kernel argument.  Every field defaults to its "off" value, so an entry point states only what is particular to it (gm_set_operands /
// gm_set_batch below fill the parts that recur).  The field ORDER is the layout the device code loads from: do not reorder or retype.
struct GemmParams {
  const char* A = nullptr; const char* W = nullptr; const float* bias = nullptr; const float* resid = nullptr; char* out = nullptr;
  const int32_t* out_row = nullptr;     // optional: row m of the product goes to output / residual row out_row[m] (< 0: dropped) -- window un-partition
  const int32_t* a_row = nullptr;       // optional: row m of the product READS operand row a_row[m] (gather; hipie_gemm_gather) -- the real tokens of a padded window layout
  long lda_b = 0, ldw_b = 0;            // row strides of A / W in BYTES
  long ldr = 0, ldo = 0;                // row strides of resid (fp32 elements) / out (elements of the output format: fp32 | fp16; HL8: fp16 elements)
  int M = 0, N = 0, K = 0;
  int nkt = 0;                          // 128-byte k tiles
  int tiles_m = 0, tiles_n = 0;         // set by the launchers, like group_m
  int group_m = 0;                      // block -> tile order: 0 / 1 = N fastest; g > 1 = groups of g M-panels, M fastest inside a group
  int out_fmt = HIPIE_F32, act = 0;
  float alpha = 1.f, oscale = 1.f;
  // batched form (hipie_gemm_batched): blockIdx.y = outer * nbi + inner; operand / output base offsets in BYTES per outer / inner index
  int nbi = 1;
  long a_bo = 0, a_bi = 0, w_bo = 0, w_bi = 0, o_bo = 0, o_bi = 0;
  // 3 x 3 convolution as an implicit GEMM on a zero-PADDED pixel grid (hipie_conv3x3_split): K = 9 taps x C channels, the A rows of k tile kt
  // come from the pixel row shifted by tap (dy, dx): byte offset ((dy - 1) * conv_wp + (dx - 1)) * lda_b + (kt % conv_kpt) * 128 -- the same
  // for every row, so only the scalar source base of the A tile changes.  conv_kpt = k tiles per tap (0: plain GEMM).
  int conv_kpt = 0, conv_wp = 0;
  // row softmax in the epilogue (hipie_gemm_batched_softmax: the logits GEMM of the image -> text fusion attention, N = text length <= 256
  // = ONE column tile): out = HL8 of softmax_j( clamp(acc) masked ) per row; sm_mask (n_outer, sm_L) uint8 or null, column j valid iff
  // j < sm_L && mask[outer][j].  0 = off.
  int softmax = 0, sm_L = 0;
  float sm_clamp = 0.f;
  const unsigned char* sm_mask = nullptr;
  const float* sm_bias = nullptr;            // softmax epilogue (VAR 8): per-column logit bias, (n_outer * n_inner, N) fp32, added before the clamp
  long r_bo = 0, r_bi = 0;                   // batched form: offsets of `resid` per outer / inner index in fp32 ELEMENTS (bias is shared)
  // residual add + LayerNorm in the epilogue (hipie_gemm_ln: N = 256 = ONE column tile, so a workgroup holds whole rows):
  // y = LN(alpha * acc + bias + resid) * ln_g + ln_b; out = y as fp32, out2 (optional) = y as HL8 rows (row stride ldo2 fp16 elements)
  const float* ln_g = nullptr; const float* ln_b = nullptr; float ln_eps = 0.f;
  char* out2 = nullptr; long ldo2 = 0;
  int variant = 0;            // timing experiments (HIPIE_GEMM_VARIANTS builds only)
  int prio_mode = 0;          // gemm2: 0 none, 1 blocks 256..511 at low priority (phase offset), 2 by dispatch-round parity
  // optional DEVICE factor of alpha (hipie_gemm_scaled: 1 / s of a gradient operand that was scaled by the power of two s, grad_pack.hip); a
  // kernel reads it once per block, in front of its k loop (gm_alpha_dev).  NULL = off: alpha is used as it stands, today's bits.
  const float* alpha_dev = nullptr;
};

// the epilogue's alpha of this block: the host's value, times the device factor when there is one
__device__ __forceinline__ void gm_alpha_dev(GemmParams& p) {
  if (p.alpha_dev != nullptr) p.alpha *= *p.alpha_dev;
}

__device__ __forceinline__ unsigned int gm_pack2(float a, float b) {
  typedef _Float16 h2 __attribute__((ext_vector_type(2)));
  h2 v;
  v[0] = (f16_t)a;
  v[1] = (f16_t)b;
  return __builtin_bit_cast(unsigned int, v);
}

__device__ __forceinline__ unsigned int gm_pack2h(f16_t a, f16_t b) {
  typedef _Float16 h2 __attribute__((ext_vector_type(2)));
  h2 v;
  v[0] = a;
  v[1] = b;
  return __builtin_bit_cast(unsigned int, v);
}


// ---- tile epilogue of one 32-feature x 32-token MFMA block (both kernels): lane = token, 16 accumulator values = 4 quads of 4
// consecutive features.  The activation / residual / scale switches are taken once per block (not per value: the per-value form cost
// ~1400 scalar branches per wave), and the HL8 split works on PAIRS: v_cvt_pk_f16_f32 for the hi and the lo halves.
typedef _Float16 gm_h2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void gm_split2(float x0, float x1, unsigned int& H, unsigned int& L) {
  x0 = __builtin_amdgcn_fmed3f(x0, -65504.f, 65504.f);
  x1 = __builtin_amdgcn_fmed3f(x1, -65504.f, 65504.f);
  hl_split2(x0, x1, H, L);
}

// quads [G0, G0 + NG) of the block; rq = the residual quads (zeros when there is no residual); sb = this block's 32 bias values in LDS
// x = the raw accumulator values of quads [G0, G0 + NG) of the block (G0 may be a runtime value: 0 | 2 for half blocks)
template <int NG>
__device__ __forceinline__ void gm_epi_vals(const float (&x)[NG][4], const int G0, const float4* rq, const float* sb, const long m, const bool mok,
                                            const int nb, const int hi, const GemmParams& p, const bool has_res) {
  typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
  typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
  const float alpha = p.alpha, osc = p.oscale;
  const int act = p.act, ofmt = p.out_fmt;
  float v[NG][4];
#pragma unroll
  for (int g = 0; g < NG; ++g) {
    const float4 b4 = *reinterpret_cast<const float4*>(sb + 8 * (G0 + g) + 4 * hi);
    v[g][0] = x[g][0] * alpha + b4.x;
    v[g][1] = x[g][1] * alpha + b4.y;
    v[g][2] = x[g][2] * alpha + b4.z;
    v[g][3] = x[g][3] * alpha + b4.w;
  }
  if (act == 1) {
#pragma unroll
    for (int g = 0; g < NG; ++g)
#pragma unroll
      for (int e = 0; e < 4; ++e) v[g][e] = gm_gelu(v[g][e]);
  } else if (act == 2) {
#pragma unroll
    for (int g = 0; g < NG; ++g)
#pragma unroll
      for (int e = 0; e < 4; ++e) v[g][e] = fmaxf(v[g][e], 0.f);
  } else if (act == 3) {                       // QuickGELU of the OpenAI CLIP weights: y * sigmoid(1.702 y) (open_clip's QuickGELU; hipie/open_vocab/clip.py towers)
#pragma unroll
    for (int g = 0; g < NG; ++g)
#pragma unroll
      for (int e = 0; e < 4; ++e) v[g][e] = v[g][e] / (1.f + expf(-1.702f * v[g][e]));
  }
  if (has_res) {
#pragma unroll
    for (int g = 0; g < NG; ++g) { v[g][0] += rq[g].x; v[g][1] += rq[g].y; v[g][2] += rq[g].z; v[g][3] += rq[g].w; }
  }
  if (osc != 1.f) {
#pragma unroll
    for (int g = 0; g < NG; ++g)
#pragma unroll
      for (int e = 0; e < 4; ++e) v[g][e] *= osc;
  }
  if (ofmt == HIPIE_F16) {
    // quads g and g + 1 of the two lane halves are exchanged so that the lower half stores features 8g .. 8g+7 and the upper
    // half 8(g+1) .. 8(g+1)+7 as ONE 16-byte piece each
#pragma unroll
    for (int g = 0; g < NG; g += 2) {
      const u32x2 s0 = __builtin_amdgcn_permlane32_swap(gm_pack2(v[g][0], v[g][1]), gm_pack2(v[g + 1][0], v[g + 1][1]), false, false);
      const u32x2 s1 = __builtin_amdgcn_permlane32_swap(gm_pack2(v[g][2], v[g][3]), gm_pack2(v[g + 1][2], v[g + 1][3]), false, false);
      const int n = nb + 8 * (G0 + g + hi);
      if (mok && n < p.N) *reinterpret_cast<u32x4*>(reinterpret_cast<f16_t*>(p.out) + m * p.ldo + n) = (u32x4){s0[0], s1[0], s0[1], s1[1]};
    }
  } else {
    // fp32 and HL8: the block's 32 features are a 128-byte span of the output row, of which this lane holds the four 16-byte
    // pieces at byte 32 g + 16 hi (fp32: features 8g+4hi ..+3; HL8: the lower lane half ends up with the 8 hi values of group g,
    // the upper half with its 8 lo values).  One store per piece: 32 rows x 32 bytes per instruction.
    u32x4 piece[NG];
    if (ofmt == HIPIE_F32) {
#pragma unroll
      for (int g = 0; g < NG; ++g)
        piece[g] = (u32x4){__builtin_bit_cast(unsigned int, v[g][0]), __builtin_bit_cast(unsigned int, v[g][1]),
                           __builtin_bit_cast(unsigned int, v[g][2]), __builtin_bit_cast(unsigned int, v[g][3])};
    } else {
#pragma unroll
      for (int g = 0; g < NG; ++g) {
        unsigned int H0, L0, H1, L1;
        gm_split2(v[g][0], v[g][1], H0, L0);
        gm_split2(v[g][2], v[g][3], H1, L1);
#if defined(__HIP_DEVICE_COMPILE__) && !defined(HIPIE_NO_FMA_MIX)
        // the split above is inline asm, which hipcc's hazard recogniser does not look into: v_permlane32_swap must not read a VGPR in the
        // two wait states behind the VALU instruction that wrote it (the rule of settle(), wave.h, for the four registers of this quad)
        asm volatile("s_nop 1" : "+v"(H0), "+v"(L0), "+v"(H1), "+v"(L1));
#endif
        const u32x2 s0 = __builtin_amdgcn_permlane32_swap(H0, L0, false, false);    // lower: (H0 own, H0 of upper); upper: (L0 of lower, L0 own)
        const u32x2 s1 = __builtin_amdgcn_permlane32_swap(H1, L1, false, false);
        piece[g] = (u32x4){s0[0], s1[0], s0[1], s1[1]};
      }
    }
    const long rowb = (m * p.ldo) * (ofmt == HIPIE_F32 ? 4 : 2) + (long)nb * 4 + 16 * hi;
#pragma unroll
    for (int g = 0; g < NG; ++g)
      if (mok && nb + 8 * (G0 + g) < p.N) *reinterpret_cast<u32x4*>(p.out + rowb + 32 * (G0 + g)) = piece[g];
  }
}

template <int G0, int NG>
__device__ __forceinline__ void gm_epi_quads(const f32x16& a, const float4* rq, const float* sb, const long m, const bool mok, const int nb,
                                             const int hi, const GemmParams& p, const bool has_res) {
  float x[NG][4];
#pragma unroll
  for (int g = 0; g < NG; ++g)
#pragma unroll
    for (int e = 0; e < 4; ++e) x[g][e] = a[4 * (G0 + g) + e];
  gm_epi_vals<NG>(x, G0, rq, sb, m, mok, nb, hi, p, has_res);
}

// ---- the 16x16x32 instances (MS = 16) ----
// LDS swizzle of their stage image: chunk k of row r sits at position k ^ gm_swz16(r).  A ds_read_b128 lane group is 4 + 4 + 8 lanes of three
// k groups (MI355X_MICROARCH.md, LDS table: {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31} and the same + 32), i.e. rows {0-3, 12-15} of one k
// group and rows 4-11 of the next, or the complement: the 16 (row parity, position) pairs of a group are distinct when rows 4-11 take the
// other half of the positions than rows 0-3 / 12-15 (bit 2) and the row pairs inside a half differ in bits 0-1.  Enumerated on the CPU for
// both chunks of a k group (tools/lds_swizzle_check.py).
__device__ __forceinline__ constexpr int gm_swz16(const int r) { return ((r >> 1) & 3) | (((((r & 15) + 4) >> 3) & 1) << 2); }

// tile epilogue of a PAIR of 16-feature x 16-token MFMA tiles (features nb .. nb + 31 of one token tile): lane (c, g) holds token c and
// features 16 i + 4 g .. + 3 of tile i.  The arithmetic of gm_epi_vals in the same order; rq = the residual values of the two quads
// (zeros when there is no residual); sb = the pair's 32 bias values in LDS.  The lane-half exchange of gm_epi_vals becomes
// v_permlane16_swap, which exchanges the ODD 16-lane rows of its first operand with the EVEN rows of its second (quarters 0 <-> 1, 2 <-> 3).
__device__ __forceinline__ void gm_epi_vals16(const float (&x)[2][4], const float4* rq, const float* sb, const long m, const bool mok, const int nb,
                                              const int g, const GemmParams& p, const bool has_res) {
  typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
  typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
  const float alpha = p.alpha, osc = p.oscale;
  const int act = p.act, ofmt = p.out_fmt;
  float v[2][4];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const float4 b4 = *reinterpret_cast<const float4*>(sb + 16 * i + 4 * g);
    v[i][0] = x[i][0] * alpha + b4.x;
    v[i][1] = x[i][1] * alpha + b4.y;
    v[i][2] = x[i][2] * alpha + b4.z;
    v[i][3] = x[i][3] * alpha + b4.w;
  }
  if (act == 1) {
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int e = 0; e < 4; ++e) v[i][e] = gm_gelu(v[i][e]);
  } else if (act == 2) {
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int e = 0; e < 4; ++e) v[i][e] = fmaxf(v[i][e], 0.f);
  } else if (act == 3) {
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int e = 0; e < 4; ++e) v[i][e] = v[i][e] / (1.f + expf(-1.702f * v[i][e]));
  }
  if (has_res) {
#pragma unroll
    for (int i = 0; i < 2; ++i) { v[i][0] += rq[i].x; v[i][1] += rq[i].y; v[i][2] += rq[i].z; v[i][3] += rq[i].w; }
  }
  if (osc != 1.f) {
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int e = 0; e < 4; ++e) v[i][e] *= osc;
  }
  if (ofmt == HIPIE_F16) {
    // the two tiles are exchanged between neighbouring quarters: quarter 0 ends up with features 0..7 of tile 0, quarter 1 with 0..7 of
    // tile 1, quarters 2 / 3 with 8..15 of tile 0 / 1 -- ONE 16-byte piece each
    const u32x2 s0 = __builtin_amdgcn_permlane16_swap(gm_pack2(v[0][0], v[0][1]), gm_pack2(v[1][0], v[1][1]), false, false);
    const u32x2 s1 = __builtin_amdgcn_permlane16_swap(gm_pack2(v[0][2], v[0][3]), gm_pack2(v[1][2], v[1][3]), false, false);
    const int n = nb + 16 * (g & 1) + 8 * (g >> 1);
    if (mok && n < p.N) *reinterpret_cast<u32x4*>(reinterpret_cast<f16_t*>(p.out) + m * p.ldo + n) = (u32x4){s0[0], s1[0], s0[1], s1[1]};
  } else {
    // fp32 and HL8: a tile's 16 features are a 64-byte span of the output row, of which this lane holds the 16-byte piece at byte 16 g
    // (fp32: features 4g ..+3; HL8: quarters 0 / 2 end up with the 8 hi values of a group, quarters 1 / 3 with its 8 lo values)
    u32x4 piece[2];
    if (ofmt == HIPIE_F32) {
#pragma unroll
      for (int i = 0; i < 2; ++i)
        piece[i] = (u32x4){__builtin_bit_cast(unsigned int, v[i][0]), __builtin_bit_cast(unsigned int, v[i][1]),
                           __builtin_bit_cast(unsigned int, v[i][2]), __builtin_bit_cast(unsigned int, v[i][3])};
    } else {
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        unsigned int H0, L0, H1, L1;
        gm_split2(v[i][0], v[i][1], H0, L0);
        gm_split2(v[i][2], v[i][3], H1, L1);
#if defined(__HIP_DEVICE_COMPILE__) && !defined(HIPIE_NO_FMA_MIX)
        // inline-asm split in front of a lane swap: the wait states of settle() (wave.h), as in gm_epi_vals
        asm volatile("s_nop 1" : "+v"(H0), "+v"(L0), "+v"(H1), "+v"(L1));
#endif
        const u32x2 s0 = __builtin_amdgcn_permlane16_swap(H0, L0, false, false);    // even quarter: (H0 own, H0 of the odd one); odd: (L0 of the even one, L0 own)
        const u32x2 s1 = __builtin_amdgcn_permlane16_swap(H1, L1, false, false);
        piece[i] = (u32x4){s0[0], s1[0], s0[1], s1[1]};
      }
    }
    const long rowb = (m * p.ldo) * (ofmt == HIPIE_F32 ? 4 : 2) + (long)nb * 4 + 16 * g;
#pragma unroll
    for (int i = 0; i < 2; ++i)
      if (mok && nb + 16 * i < p.N) *reinterpret_cast<u32x4*>(p.out + rowb + 64 * i) = piece[i];
  }
}

// k loop and epilogue of gemm_kernel<BN, true, VAR, 16> behind the common front (tile map, DMA plan): `dma` is the kernel's own issue lambda
template <int BN, bool AF32, typename Dma>
__device__ __forceinline__ void gm_body16(const GemmParams& p, char* smem, const Dma& dma, const int m0, const int n0, const int wm, const int wn,
                                          const int tid) {
  constexpr int BM = 256, ROWS = BM + BN, STAGE = ROWS * 128, NI = ROWS / 64;
  constexpr int NT = 4;                        // 16-token tiles per wave
  constexpr int NF = BN / 32;                  // 16-feature tiles per wave
  typedef Mfma16<f16_t>::frag frag;
  const int lane = tid & 63, c = lane & 15, g = lane >> 4;

  // ---- fragment addresses: row = tile base (multiple of 16) + c; chunk 2 g (hi | x0..x3) and 2 g + 1 (lo | x4..x7) of the lane's k group ----
  const int swz = gm_swz16(c);
  const char* xrow = smem + (wm * 64 + c) * 128;                     // + t * 16 * 128
  const char* wrow = smem + (BM + wn * (BN / 2) + c) * 128;          // + j * 16 * 128
  const int ch[2] = {16 * ((2 * g) ^ swz), 16 * ((2 * g + 1) ^ swz)};

  f32x4 acc[NF][NT];
#pragma unroll
  for (int j = 0; j < NF; ++j)
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[j][t] = (f32x4){0.f, 0.f, 0.f, 0.f};

  const int nkt = p.nkt;
#pragma unroll
  for (int i = 0; i < NI; ++i) dma(i, 0, 0);
  __builtin_amdgcn_s_waitcnt(vmcnt(0));
  __syncthreads();

  for (int kt = 0; kt < nkt; ++kt) {
    const int st = kt & 1;
    const bool more = kt + 1 < nkt;
    const char* xs = xrow + st * STAGE;
    const char* ws = wrow + st * STAGE;
    frag xa[2][NT];              // [hi | lo][token tile]: the stage's X fragments, read once
    frag wa[3][2];               // [feature tile % 3][hi | lo]: two tiles ahead of the MFMAs
    auto load_w = [&](const int j) {
      wa[j % 3][0] = *reinterpret_cast<const frag*>(ws + j * 2048 + ch[0]);
      wa[j % 3][1] = *reinterpret_cast<const frag*>(ws + j * 2048 + ch[1]);
    };
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      xa[0][t] = *reinterpret_cast<const frag*>(xs + t * 2048 + ch[0]);
      xa[1][t] = *reinterpret_cast<const frag*>(xs + t * 2048 + ch[1]);
    }
    load_w(0);
    load_w(1);
    if (AF32) {
      // fp32 A rows: the two chunks hold x0..x3 / x4..x7 of the lane's k group (the bytes an HL8 group takes): split them here
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        const f32x4 a = __builtin_bit_cast(f32x4, xa[0][t]), b = __builtin_bit_cast(f32x4, xa[1][t]);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          f16_t hh, ll;
          hl_split(a[e], hh, ll);
          xa[0][t][e] = hh; xa[1][t][e] = ll;
          hl_split(b[e], hh, ll);
          xa[0][t][4 + e] = hh; xa[1][t][4 + e] = ll;
        }
      }
    }
    // the DMA plan of the 32x32x16 form: a feature tile's 12 MFMAs take the cycles of one of its sub-steps (6 of twice the length)
    constexpr int DMA_BY = 4;
    constexpr int PER = (NI + DMA_BY - 1) / DMA_BY;
#pragma unroll
    for (int j = 0; j < NF; ++j) {
      if (j + 2 < NF) load_w(j + 2);
      const frag wh = wa[j % 3][0], wl = wa[j % 3][1];
#pragma unroll
      for (int t = 0; t < NT; ++t) acc[j][t] = Mfma16<f16_t>::mma(wl, xa[0][t], acc[j][t]);
#pragma unroll
      for (int t = 0; t < NT; ++t) acc[j][t] = Mfma16<f16_t>::mma(wh, xa[1][t], acc[j][t]);
#pragma unroll
      for (int t = 0; t < NT; ++t) acc[j][t] = Mfma16<f16_t>::mma(wh, xa[0][t], acc[j][t]);
      if (more) {
#pragma unroll
        for (int i = j * PER; i < (j + 1) * PER && i < NI; ++i) dma(i, kt + 1, st ^ 1);
      }
    }
    __builtin_amdgcn_s_waitcnt(vmcnt(0));      // this wave's DMA writes of stage t+1 have landed
    __syncthreads();                          // ... and everybody's; all reads of stage t are done
  }

  // ---- epilogue: lane = token c of a 16-token tile, registers = features 4 g .. 4 g + 3 of a 16-feature tile ----
  const bool has_res = p.resid != nullptr;
  float* sbias = reinterpret_cast<float*>(smem);     // the tile's bias values go through LDS once, as in the 32x32x16 form
  if (tid < BN) sbias[tid] = (p.bias != nullptr && n0 + tid < p.N) ? p.bias[n0 + tid] : 0.f;
  __syncthreads();
  long orow[NT];                                     // output row of this lane's four tokens (identity, or the caller's row map: -1 drops the row)
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const int m = m0 + wm * 64 + t * 16 + c;
    orow[t] = (m < p.M) ? (p.out_row != nullptr ? (long)p.out_row[m] : (long)m) : -1;
  }
  // residual rows: the two quads of pair blk + 1 are requested before pair blk is processed
  float4 rq[2][2];
  auto load_res = [&](const int blk, float4 (&dst)[2]) {
    const int t = blk / (NF / 2), jp = blk % (NF / 2);
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int n = n0 + wn * (BN / 2) + jp * 32 + 16 * i + 4 * g;
      dst[i] = (has_res && orow[t] >= 0 && n < p.N) ? *reinterpret_cast<const float4*>(p.resid + orow[t] * p.ldr + n) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
  };
  load_res(0, rq[0]);
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const long m = orow[t];
#pragma unroll
    for (int jp = 0; jp < NF / 2; ++jp) {
      const int blk = t * (NF / 2) + jp;
      if (blk + 1 < NT * (NF / 2)) load_res(blk + 1, rq[(blk + 1) & 1]);
      const int nb = n0 + wn * (BN / 2) + jp * 32;              // first feature of the pair
      float x[2][4];
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int e = 0; e < 4; ++e) x[i][e] = acc[2 * jp + i][t][e];
      gm_epi_vals16(x, rq[blk & 1], sbias + (nb - n0), m, m >= 0, nb, g, p, has_res);
    }
  }
}

template <int BN, bool SPLIT, int VAR, int MS = 32>
__global__ __launch_bounds__(512, 2) void gemm_kernel(const GemmParams pin) {
  static_assert(MS == 32 || (MS == 16 && BN == 320 && SPLIT && (VAR == 0 || VAR == 2)),
                "the 16x16x32 form exists for the wide split instances (HL8 and fp32 A rows) only");
  GemmParams p = pin;
  gm_alpha_dev(p);
  int vtile = -1;
  if (VAR == 8) {
    // batched with the INNER index fastest (grid: tiles * n_inner x n_outer): the n_inner problems of one row tile share their A operand (the
    // heads of the folded fusion attention all read the visual stream), so they run back to back inside ONE XCD's contiguous range of ids
    // and the 256 KB A tile is fetched once into that XCD's L2 instead of once per head (PMC: 1.57 GB fetched per launch for 0.18 GB of A)
    const int nblk = p.tiles_m * p.tiles_n * p.nbi;
    const int id = blockIdx.x, xcd = id & 7, j = id >> 3;
    const int q = nblk >> 3, r = nblk & 7;
    const int v = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + j;
    const int bo = blockIdx.y, bi = v % p.nbi;
    vtile = v / p.nbi;
    p.A += bo * p.a_bo + bi * p.a_bi;
    p.W += bo * p.w_bo + bi * p.w_bi;
    p.out += bo * p.o_bo + bi * p.o_bi;
    if (p.sm_mask != nullptr) p.sm_mask += (long)bo * p.sm_L;
    if (p.sm_bias != nullptr) p.sm_bias += ((long)bo * p.nbi + bi) * p.N;
  } else if (gridDim.y > 1) {                   // batched: one (outer, inner) problem per blockIdx.y
    const int bo = blockIdx.y / p.nbi, bi = blockIdx.y - bo * p.nbi;
    p.A += bo * p.a_bo + bi * p.a_bi;
    p.W += bo * p.w_bo + bi * p.w_bi;
    p.out += bo * p.o_bo + bi * p.o_bi;
    if (p.sm_mask != nullptr) p.sm_mask += (long)bo * p.sm_L;
    if (p.sm_bias != nullptr) p.sm_bias += (long)blockIdx.y * p.N;
    if (p.resid != nullptr) p.resid += bo * p.r_bo + bi * p.r_bi;
  }
  constexpr int BM = 256;
  constexpr int ROWS = BM + BN;                // rows of one LDS stage: the A tile then the W tile
  constexpr int STAGE = ROWS * 128;            // bytes
  constexpr int NI = ROWS / 64;                // DMA instructions per wave and stage (one covers 8 rows x 128 B)
  constexpr int NJ = BN / 64;                  // 32-feature blocks per wave
  constexpr int KS = SPLIT ? 2 : 4;            // k16 steps per stage
  constexpr int SUB = KS * NJ;                 // (k-step, feature block) sub-steps per stage
  constexpr bool AF32 = VAR == 2 || VAR == 6;  // A rows are plain fp32, split in registers
  constexpr bool LNE = VAR == 4 || VAR == 6;   // residual add + LayerNorm epilogue (separate instances: the plain kernels' code is unchanged)
  typedef Mfma32<f16_t>::frag frag;

  extern __shared__ __attribute__((aligned(128))) char smem[];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave & 3, wn = wave >> 2;
  const int li = lane & 31, hi = lane >> 5;

  // ---- block -> tile (bijective XCD-aware order: XCD x owns a contiguous range of tile ids) ----
  int tm, tn;
  {
    const int nblk = p.tiles_m * p.tiles_n;
    const int id = blockIdx.x, xcd = id & 7, j = id >> 3;
    const int q = nblk >> 3, r = nblk & 7;
    const int v = (VAR == 8) ? vtile : (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + j;
    if (p.group_m > 1) {
      const int gsz = p.group_m * p.tiles_n;
      const int g = v / gsz, w = v - g * gsz;
      const int rows = min(p.group_m, p.tiles_m - g * p.group_m);      // the last group may be shorter
      tn = w / rows;
      tm = g * p.group_m + (w - tn * rows);
    } else {
      tm = v / p.tiles_n;
      tn = v - tm * p.tiles_n;
    }
  }
  const int m0 = tm * BM, n0 = tn * BN;

  // ---- DMA plan: instruction i of this wave fills rows 8 * (8 i + wave) .. + 7 of the stage image; lane -> (row, chunk position) ----
  unsigned int dvoff[NI];
  {
    const int rl = lane >> 3, cp = lane & 7;
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      const int r = 8 * (8 * i + wave) + rl;              // stage row
      const int c = cp ^ (MS == 16 ? gm_swz16(r) : ((r >> 1) & 7));      // logical chunk stored at this position
      if (r < BM) {
        const int mr = min(r, p.M - 1 - m0);
        // gather: the offset is taken from the START of A (all of A within 4 GB: checked on the host)
        dvoff[i] = p.a_row != nullptr ? (unsigned int)((long)p.a_row[m0 + mr] * p.lda_b + 16 * c) : (unsigned int)((long)mr * p.lda_b + 16 * c);
      } else dvoff[i] = (unsigned int)((long)min(r - BM, p.N - 1 - n0) * p.ldw_b + 16 * c);
    }
  }
  const char* abase = p.a_row != nullptr ? p.A : p.A + (long)m0 * p.lda_b;
  const char* wbase = p.W + (long)n0 * p.ldw_b;
  const unsigned int lds0 = (unsigned int)reinterpret_cast<uintptr_t>((__attribute__((address_space(3))) char*)smem);

  auto dma = [&](const int i, const int kt, const int stage) {
    const bool isa = (8 * (8 * i + wave)) < BM;           // wave-uniform: an instruction is all-A or all-W (BM % 64 == 0)
    long ko = (long)kt * 128;
    if (isa && p.conv_kpt) {                              // implicit 3 x 3 convolution: tap of this k tile -> row shift on the padded grid
      const int tap = kt / p.conv_kpt, r = kt - tap * p.conv_kpt, dy = tap / 3;
      ko = ((long)(dy - 1) * p.conv_wp + (tap - 3 * dy - 1)) * p.lda_b + (long)r * 128;
    }
    const char* sb = (isa ? abase : wbase) + ko;
    dma16(sb, dvoff[i], __builtin_amdgcn_readfirstlane(lds0 + (unsigned int)(stage * STAGE + 1024 * (8 * i + wave))));
  };

  if constexpr (MS == 16) {
    gm_body16<BN, VAR == 2>(p, smem, dma, m0, n0, wm, wn, tid);
    return;
  }

  // ---- fragment addresses: row = tile base (multiple of 32) + li, so the swizzle term is ((li >> 1) & 7) for every tile ----
  const int swz = (li >> 1) & 7;
  const char* xrow = smem + (wm * 64 + li) * 128;                    // + t * 32 * 128
  const char* wrow = smem + (BM + wn * (BN / 2) + li) * 128;         // + j * 32 * 128
  // logical chunk of (k-step ks, lane half, lo): plain 2 ks + hi; split 2 (2 ks + hi) + lo
  auto choff = [&](const int ks, const int lo) -> int { return 16 * ((SPLIT ? (2 * (2 * ks + hi) + lo) : (2 * ks + hi)) ^ swz); };

  f32x16 acc[NJ][2];
#pragma unroll
  for (int j = 0; j < NJ; ++j)
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[j][t][r] = 0.f;

  // ---- prologue: stage 0 ----
#ifdef HIPIE_GEMM_VARIANTS
  const int nkt = (VAR == 3) ? 0 : p.nkt;     // timing experiment: the epilogue alone
  if (VAR != 3)
#else
  const int nkt = p.nkt;
#endif
  {
#pragma unroll
    for (int i = 0; i < NI; ++i) dma(i, 0, 0);
  }
  __builtin_amdgcn_s_waitcnt(vmcnt(0));
  __syncthreads();

  for (int kt = 0; kt < nkt; ++kt) {
    const int st = kt & 1;
    const bool more = kt + 1 < nkt;
    const char* xs = xrow + st * STAGE;
    const char* ws = wrow + st * STAGE;
    // software pipeline inside the stage: the fragments of sub-step s + 1 are requested before the MFMAs of sub-step s
    frag xa[2][2][2];            // [k-step parity][hi | lo][token tile]
    frag wa[2][2];               // [sub-step parity][hi | lo]
    auto load_x = [&](const int ks) {
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        xa[ks & 1][0][t] = *reinterpret_cast<const frag*>(xs + t * 4096 + choff(ks, 0));
        if (SPLIT) xa[ks & 1][1][t] = *reinterpret_cast<const frag*>(xs + t * 4096 + choff(ks, 1));
      }
    };
    auto load_w = [&](const int s) {
      const int ks = s / NJ, j = s % NJ;
      wa[s & 1][0] = *reinterpret_cast<const frag*>(ws + j * 4096 + choff(ks, 0));
      if (SPLIT) wa[s & 1][1] = *reinterpret_cast<const frag*>(ws + j * 4096 + choff(ks, 1));
    };
    load_x(0);
    load_w(0);
    // DMA plan: the instructions of stage t + 1 are issued in the FIRST sub-steps of stage t, PER sub-step as many as it takes to be
    // done by sub-step DMA_BY: a fill needs 1-2 us from issue to landing and the stage ends with vmcnt(0), so a late issue stalls
    // every wave at the barrier (measured: one DMA per sub-step over the whole stage cost ~15 % of the split kernel's rate)
    constexpr int DMA_BY = SPLIT ? 4 : 6;                        // sub-steps that carry DMA instructions
    constexpr int PER = (NI + DMA_BY - 1) / DMA_BY;
    frag cx[2][2];               // AF32 (fp32 A rows): the k-step's A fragments split in registers, [hi | lo][token tile]
#pragma unroll
    for (int s = 0; s < SUB; ++s) {
      const int ks = s / NJ, j = s % NJ;
      if (s + 1 < SUB) {
        if ((s + 1) % NJ == 0) load_x(ks + 1);
        load_w(s + 1);
      }
      if (AF32 && j == 0) {
        // the two 16-byte chunks of a group hold x0..x3 / x4..x7 as fp32 (the same 32 bytes an HL8 group takes): split them here
#pragma unroll
        for (int t = 0; t < 2; ++t) {
          const f32x4 a = __builtin_bit_cast(f32x4, xa[ks & 1][0][t]), b = __builtin_bit_cast(f32x4, xa[ks & 1][1][t]);
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            f16_t hh, ll;
            hl_split(a[e], hh, ll);
            cx[0][t][e] = hh; cx[1][t][e] = ll;
            hl_split(b[e], hh, ll);
            cx[0][t][4 + e] = hh; cx[1][t][4 + e] = ll;
          }
        }
      }
      const frag wh = wa[s & 1][0];
      const frag xh0 = AF32 ? cx[0][0] : xa[ks & 1][0][0], xh1 = AF32 ? cx[0][1] : xa[ks & 1][0][1];
      if (SPLIT) {
        const frag wl = wa[s & 1][1];
        const frag xl0 = AF32 ? cx[1][0] : xa[ks & 1][1][0], xl1 = AF32 ? cx[1][1] : xa[ks & 1][1][1];
        acc[j][0] = Mfma32<f16_t>::mma(wl, xh0, acc[j][0]);
        acc[j][1] = Mfma32<f16_t>::mma(wl, xh1, acc[j][1]);
        acc[j][0] = Mfma32<f16_t>::mma(wh, xl0, acc[j][0]);
        acc[j][1] = Mfma32<f16_t>::mma(wh, xl1, acc[j][1]);
      }
      acc[j][0] = Mfma32<f16_t>::mma(wh, xh0, acc[j][0]);
      acc[j][1] = Mfma32<f16_t>::mma(wh, xh1, acc[j][1]);
      if (more) {
#pragma unroll
        for (int i = s * PER; i < (s + 1) * PER && i < NI; ++i) dma(i, kt + 1, st ^ 1);
      }
    }
    __builtin_amdgcn_s_waitcnt(vmcnt(0));      // this wave's DMA writes of stage t+1 have landed
    __syncthreads();                          // ... and everybody's; all reads of stage t are done
  }

  // ---- epilogue: lane = token (column of the MFMA tile), registers = features ----
  bool has_res = p.resid != nullptr;
#ifdef HIPIE_GEMM_VARIANTS
  if (VAR == 1 && p.alpha != 12345.f) return;        // timing experiment: no epilogue at all (tools/bench_gemm2.py variants)
#endif
  const int act = p.act, ofmt = p.out_fmt;
  const float alpha = p.alpha, osc = p.oscale;
  // the tile's bias values go through LDS once (the stage buffers are free after the last barrier): the per-quad bias reads are then
  // LDS reads the compiler can schedule freely between the global stores (a global read behind every store serialised the epilogue)
  float* sbias = reinterpret_cast<float*>(smem);
  if (tid < BN) sbias[tid] = (p.bias != nullptr && n0 + tid < p.N) ? p.bias[n0 + tid] : 0.f;
  if (SPLIT && LNE && BN == 256) {
    // ---- residual add + LayerNorm over the tile's 256 columns (the whole row: one column tile), the statistics of hipie_add_layernorm_dec
    //      (two passes, fp32): a lane owns 64 of its token's 256 columns per token tile; lane-local sums, one exchange with the other lane
    //      half (xor 32), one with the partner wave (wn ^ 1) through LDS.  Every residual value of a row is read before any store of that
    //      row (rows belong to ONE workgroup), so `out` may alias `resid`. ----
    float* lg = sbias + 256;                    // [256] gamma
    float* lb = lg + 256;                       // [256] beta
    float* red = lb + 256;                      // [2 wn][256 tokens] partial sums, then partial squared deviations
    if (tid < 256) { lg[tid] = p.ln_g[tid]; lb[tid] = p.ln_b[tid]; }
    __syncthreads();
    float su[2] = {0.f, 0.f};
    // residual quads of block (t, j + 1) are requested before block (t, j) is summed (two buffers: hoisting all 32 loads would spill)
    f32x4 rr[2][4];
    auto ln_res = [&](const int blk, f32x4 (&dst)[4]) {
      const int t = blk / NJ, j = blk % NJ;
      const int m = min(m0 + wm * 64 + t * 32 + li, p.M - 1);       // rows beyond M re-read the last row (never stored): no branch
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int n = wn * (BN / 2) + j * 32 + 8 * g + 4 * hi;
        dst[g] = *reinterpret_cast<const f32x4*>(p.resid + (long)m * p.ldr + n);
      }
    };
    ln_res(0, rr[0]);
#pragma unroll
    for (int blk = 0; blk < 2 * NJ; ++blk) {
      const int t = blk / NJ, j = blk % NJ;
      if (blk + 1 < 2 * NJ) ln_res(blk + 1, rr[(blk + 1) & 1]);
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int n = wn * (BN / 2) + j * 32 + 8 * g + 4 * hi;
        const f32x4 b4 = *reinterpret_cast<const f32x4*>(sbias + n);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          float x = acc[j][t][4 * g + e] * p.alpha + b4[e];
          x += rr[blk & 1][g][e];
          acc[j][t][4 * g + e] = x;
          su[t] += x;
        }
      }
#if defined(__HIP_DEVICE_COMPILE__)
      __builtin_amdgcn_sched_barrier(0);
#endif
    }
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      su[t] += __shfl_xor(su[t], 32);
      if (hi == 0) red[wn * 256 + wm * 64 + t * 32 + li] = su[t];
    }
    __syncthreads();
    float mean[2], sq[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      mean[t] = (su[t] + red[(wn ^ 1) * 256 + wm * 64 + t * 32 + li]) / 256.f;
      float q = 0.f;
#pragma unroll
      for (int j = 0; j < NJ; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) { const float d = acc[j][t][r] - mean[t]; q += d * d; }
      sq[t] = q + __shfl_xor(q, 32);
    }
    __syncthreads();                             // everybody has read the partial sums
#pragma unroll
    for (int t = 0; t < 2; ++t)
      if (hi == 0) red[wn * 256 + wm * 64 + t * 32 + li] = sq[t];
    __syncthreads();
    float rstd[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) rstd[t] = rsqrtf((sq[t] + red[(wn ^ 1) * 256 + wm * 64 + t * 32 + li]) / 256.f + p.ln_eps);
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      // t outside e: a (t = 0, t = 1) pair of `x - mean[t]` would be SLP-packed into v_pk_add_f32 with op_sel [0,1] -- the form of the
      // gfx950 packed-fp32 erratum (tests/test_isa_hazards.py refuses it)
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int n = wn * (BN / 2) + j * 32 + 8 * g + 4 * hi;
          const f32x4 g4 = *reinterpret_cast<const f32x4*>(lg + n), b4 = *reinterpret_cast<const f32x4*>(lb + n);
#pragma unroll
          for (int e = 0; e < 4; ++e) acc[j][t][4 * g + e] = (acc[j][t][4 * g + e] - mean[t]) * rstd[t] * g4[e] + b4[e];
        }
#if defined(__HIP_DEVICE_COMPILE__)
      __builtin_amdgcn_sched_barrier(0);         // one block's gamma / beta reads at a time (hoisted together they spill)
#endif
    }
    __syncthreads();                             // the bias table has been read by everybody
    if (tid < BN) sbias[tid] = 0.f;              // the values are final: the store path below adds a zero bias, no residual, alpha 1
    p.alpha = 1.f; p.act = 0; p.oscale = 1.f; p.out_fmt = HIPIE_F32;   // compile-time facts of this instance from here on
    has_res = false;
  }
  if (SPLIT && (VAR == 0 || VAR == 8) && BN == 256 && p.softmax) {
    // ---- row softmax over the tile's columns (the whole row: one column tile).  A lane owns 64 of its token's 256 columns per token
    //      tile (its lane half's 4 of every 8, this wave's 128-column half): lane-local reduction, one exchange with the other lane half
    //      (xor 32), one with the partner wave (wn ^ 1) through LDS.  Column validity enters as a 0 / -inf table. ----
    float* kb = sbias + 256;                    // [256] 0 | -inf per column
    float* red = kb + 256;                      // [2 wn][256 tokens] partial max, then partial sums
    float* cb = red + 512;                      // [256] VAR 8: the logit bias of the column (q-side bias folded into the keys: bq . k_j)
    if (tid < 256) kb[tid] = (tid < p.sm_L && (p.sm_mask == nullptr || p.sm_mask[tid] != 0)) ? 0.f : -INFINITY;
    if (VAR == 8 && tid < 256) cb[tid] = (p.sm_bias != nullptr && tid < p.N) ? p.sm_bias[tid] : 0.f;
    __syncthreads();
    const float cl = p.sm_clamp;
    float mx[2] = {-INFINITY, -INFINITY};
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int j = 0; j < NJ; ++j)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const f32x4 k4 = *reinterpret_cast<const f32x4*>(kb + wn * (BN / 2) + j * 32 + 8 * g + 4 * hi);
          f32x4 c4 = {0.f, 0.f, 0.f, 0.f};
          if (VAR == 8) c4 = *reinterpret_cast<const f32x4*>(cb + wn * (BN / 2) + j * 32 + 8 * g + 4 * hi);
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            float x = acc[j][t][4 * g + e] * p.alpha;
            if (VAR == 8) x += c4[e];
            if (cl > 0.f) x = __builtin_amdgcn_fmed3f(x, -cl, cl);
            x += k4[e];
            acc[j][t][4 * g + e] = x;
            mx[t] = fmaxf(mx[t], x);
          }
        }
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      mx[t] = fmaxf(mx[t], __shfl_xor(mx[t], 32));
      if (hi == 0) red[wn * 256 + wm * 64 + t * 32 + li] = mx[t];
    }
    __syncthreads();
    float sm[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const float m = fmaxf(mx[t], red[(wn ^ 1) * 256 + wm * 64 + t * 32 + li]);
      const float m2 = (m == -INFINITY) ? 0.f : m * 1.4426950408889634f;
      float su = 0.f;
#pragma unroll
      for (int j = 0; j < NJ; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const float pv = __builtin_amdgcn_exp2f(acc[j][t][r] * 1.4426950408889634f - m2);     // exp2(-inf) = 0 on masked columns
          acc[j][t][r] = pv;
          su += pv;
        }
      sm[t] = su + __shfl_xor(su, 32);
    }
    __syncthreads();                             // everybody has read the partial maxima
#pragma unroll
    for (int t = 0; t < 2; ++t)
      if (hi == 0) red[wn * 256 + wm * 64 + t * 32 + li] = sm[t];
    __syncthreads();
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const float tot = sm[t] + red[(wn ^ 1) * 256 + wm * 64 + t * 32 + li];
      const float inv = tot > 0.f ? 1.f / tot : 0.f;
#pragma unroll
      for (int j = 0; j < NJ; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[j][t][r] *= inv;
    }
    p.alpha = 1.f;                               // the values are final: the store path below adds the (zero) bias and writes HL8
  }
  __syncthreads();
  // residual rows: the four quads of block (t, j + 1) are requested before block (t, j) is processed
  float4 rq[2][4];
  // output row of this lane's two tokens (identity, or the caller's row map: -1 drops the row)
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
  // LayerNorm epilogue: the normalised rows leave twice -- fp32 (the stream), then HL8 (the operand of the GEMM that follows)
  const int passes = (LNE && p.out2 != nullptr) ? 2 : 1;
#pragma unroll
  for (int pass = 0; pass < 2; ++pass) {
    if (pass >= passes) break;
    if (pass == 1) { p.out = p.out2; p.ldo = p.ldo2; p.out_fmt = HIPIE_HL8; }
    load_res(0, 0, rq[0]);
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const long m = orow[t];
      const bool mok = m >= 0;
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        const int blk = t * NJ + j;
        if (blk + 1 < 2 * NJ) load_res((blk + 1) / NJ, (blk + 1) % NJ, rq[(blk + 1) & 1]);
        const int nb = n0 + wn * (BN / 2) + j * 32;             // first feature of the 32-row MFMA block
        gm_epi_quads<0, 4>(acc[j][t], rq[blk & 1], sbias + (nb - n0), m, mok, nb, hi, p, has_res);
#if defined(__HIP_DEVICE_COMPILE__)
        if (LNE) __builtin_amdgcn_sched_barrier(0);            // its store blocks are straight-line code: scheduled together they spill
#endif
      }
    }
  }
}



// ------------------------------------------------------------------------------------------------------------------------------
// gemm_small_kernel: the split product for SMALL problems (round 4) -- the decoder / BERT / head linears (M = 1.5k .. 8k rows) fill
// 7 .. 80 of the 256 x 256 tiles above, i.e. a fraction of the 256 CUs, each walking the whole K range alone: 14 ms of the step were
// ~250 launches of 0.03 .. 0.19 ms that are pure latency.  Here the tile is 64 tokens x 128 features on 4 waves (wave w owns feature
// block w: one 32-row MFMA block x 2 token tiles = 32 accumulator registers), 3 LDS slots of a k32 step (192 rows x 128 B = 24 KB:
// two workgroups per CU), one barrier per step: M = 2400, N = 256 becomes 76 workgroups of 8 short steps instead of 10 of them, and
// M = 1552, N = 768, K = 3072 (BERT's output dense) 150 instead of 21.  Same operand formats, swizzle and epilogue as gemm_kernel.
template <int VAR>
__global__ __launch_bounds__(256, 2) void gemm_small_kernel(const GemmParams pin) {
  GemmParams p = pin;
  gm_alpha_dev(p);
  constexpr int BM = 64, BN = 128, ROWS = BM + BN, STAGE = ROWS * 128, NI = ROWS / 32;      // NI: DMA instructions per wave and stage
  typedef Mfma32<f16_t>::frag frag;
  extern __shared__ __attribute__((aligned(128))) char smem[];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 31, hi = lane >> 5;
  const int tm = blockIdx.x / p.tiles_n, tn = blockIdx.x - tm * p.tiles_n;
  const int m0 = tm * BM, n0 = tn * BN;

  unsigned int dvoff[NI];
  {
    const int rl = lane >> 3, cp = lane & 7;
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      const int r = 8 * (4 * i + wave) + rl;              // stage row
      const int c = cp ^ ((r >> 1) & 7);
      if (r < BM) dvoff[i] = (unsigned int)((long)min(r, p.M - 1 - m0) * p.lda_b + 16 * c);
      else dvoff[i] = (unsigned int)((long)min(r - BM, p.N - 1 - n0) * p.ldw_b + 16 * c);
    }
  }
  const char* abase = p.A + (long)m0 * p.lda_b;
  const char* wbase = p.W + (long)n0 * p.ldw_b;
  const unsigned int lds0 = (unsigned int)reinterpret_cast<uintptr_t>((__attribute__((address_space(3))) char*)smem);
  auto dma_stage = [&](const int kt, const int slot) {
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      const bool isa = (8 * (4 * i + wave)) < BM;         // wave-uniform (BM % 8 == 0)
      dma16((isa ? abase : wbase) + (long)kt * 128, dvoff[i],
               __builtin_amdgcn_readfirstlane(lds0 + (unsigned int)(slot * STAGE + 1024 * (4 * i + wave))));
    }
  };

  const int swz = (li >> 1) & 7;
  const char* xrow = smem + li * 128;                               // + t * 32 * 128
  const char* wrow = smem + (BM + wave * 32 + li) * 128;
  auto choff = [&](const int ks, const int lo) -> int { return 16 * ((2 * (2 * ks + hi) + lo) ^ swz); };

  f32x16 acc[2];
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;

  const int nkt = p.nkt;
  dma_stage(0, 0);
  if (nkt > 1) dma_stage(1, 1);
  int slot = 0;
  for (int kt = 0; kt < nkt; ++kt) {
    if (kt + 1 < nkt) __builtin_amdgcn_s_waitcnt(vmcnt(NI));      // stage kt landed; stage kt + 1 may still be in flight
    else __builtin_amdgcn_s_waitcnt(vmcnt(0));
    __syncthreads();                                                // ... for every wave; all reads of stage kt - 1 are done
    if (kt + 2 < nkt) dma_stage(kt + 2, slot == 0 ? 2 : slot - 1);
    const char* xs = xrow + slot * STAGE;
    const char* ws = wrow + slot * STAGE;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      frag xh[2], xl[2];
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        xh[t] = *reinterpret_cast<const frag*>(xs + t * 4096 + choff(ks, 0));
        xl[t] = *reinterpret_cast<const frag*>(xs + t * 4096 + choff(ks, 1));
      }
      const frag wh = *reinterpret_cast<const frag*>(ws + choff(ks, 0));
      const frag wl = *reinterpret_cast<const frag*>(ws + choff(ks, 1));
      if (VAR == 2) {
        // fp32 A rows: the two 16-byte pieces hold x0..x3 / x4..x7 of the lane's k group (gemm_kernel VAR 2)
#pragma unroll
        for (int t = 0; t < 2; ++t) {
          const f32x4 a = __builtin_bit_cast(f32x4, xh[t]), b = __builtin_bit_cast(f32x4, xl[t]);
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            f16_t hh, ll;
            hl_split(a[e], hh, ll);
            xh[t][e] = hh; xl[t][e] = ll;
            hl_split(b[e], hh, ll);
            xh[t][4 + e] = hh; xl[t][4 + e] = ll;
          }
        }
      }
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        acc[t] = Mfma32<f16_t>::mma(wl, xh[t], acc[t]);
        acc[t] = Mfma32<f16_t>::mma(wh, xl[t], acc[t]);
        acc[t] = Mfma32<f16_t>::mma(wh, xh[t], acc[t]);
      }
    }
    slot = slot == 2 ? 0 : slot + 1;
  }

  // ---- epilogue ----
  const bool has_res = p.resid != nullptr;
  __syncthreads();                                                  // the last stage's reads are done: its slot holds the bias values now
  float* sbias = reinterpret_cast<float*>(smem);
  if (tid < BN) sbias[tid] = (p.bias != nullptr && n0 + tid < p.N) ? p.bias[n0 + tid] : 0.f;
  __syncthreads();
  const int nb = n0 + wave * 32;
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const int mm = m0 + t * 32 + li;
    const long m = (mm < p.M) ? (p.out_row != nullptr ? (long)p.out_row[mm] : (long)mm) : -1;
    float4 rq[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int n = nb + 8 * g + 4 * hi;
      rq[g] = (has_res && m >= 0 && n < p.N) ? *reinterpret_cast<const float4*>(p.resid + m * p.ldr + n) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    gm_epi_quads<0, 4>(acc[t], rq, sbias + wave * 32, m, m >= 0, nb, hi, p, has_res);
  }
}

template <int VAR>
static int launch_gemm_small(GemmParams& p, hipStream_t st) {
  constexpr size_t lds = (size_t)3 * (64 + 128) * 128;
  p.tiles_m = (p.M + 63) / 64;
  p.tiles_n = (p.N + 127) / 128;
  auto kern = gemm_small_kernel<VAR>;
  static LdsLimit limit;
  limit.raise((const void*)kern, lds);
  hipLaunchKernelGGL(kern, dim3((unsigned)(p.tiles_m * p.tiles_n)), dim3(256), lds, st, p);
  return check_launch("gemm_small");
}

#ifdef HIPIE_GEMM_VARIANTS
#include "../../tools/ubench/gemm_overlap_study.h"     // round-4 timing study: not part of the product, lives with the micro-benchmarks
#endif

template <int BN, bool SPLIT, int VAR = 0, int MS = 32>
static int launch_gemm(GemmParams& p, hipStream_t st, int batches = 1) {
  constexpr size_t lds = (size_t)2 * (256 + BN) * 128;
  p.tiles_m = (p.M + 255) / 256;
  p.tiles_n = (p.N + BN - 1) / BN;
  // wide outputs (qkv: 12 column tiles, fc1: 16): the blocks of an XCD walk groups of 8 row panels with the row panel fastest, so the 32
  // workgroups resident on an XCD hold 8 A panels x 4 W panels instead of 2 x 16 -- 40 % fewer operand rows through that XCD's L2.
  // Same-box A/B (profiles/r06_gemm_tile_order.txt): qkv 0.894 -> 0.874 ms, fc1 1.099 -> 1.076 ms; up to 4 column tiles the plain order already is 8 x 4.
  p.group_m = p.tiles_n > 4 ? 8 : 0;
  auto kern = gemm_kernel<BN, SPLIT, VAR, MS>;
  static LdsLimit limit;
  limit.raise((const void*)kern, lds);
  if (VAR == 8)       // inner index fastest inside blockIdx.x (see the kernel): grid = tiles * n_inner x n_outer
    hipLaunchKernelGGL(kern, dim3((unsigned)(p.tiles_m * p.tiles_n * p.nbi), (unsigned)(batches / p.nbi)), dim3(512), lds, st, p);
  else
    hipLaunchKernelGGL(kern, dim3((unsigned)(p.tiles_m * p.tiles_n), (unsigned)batches), dim3(512), lds, st, p);
  return check_launch("gemm");
}

// ---- host: the recurring parts of GemmParams.  Strides and batch offsets arrive in fp16 elements (split rows: 2 K of them) ----
static inline void gm_set_operands(GemmParams& p, const void* A, long lda, const void* W, long ldw, int M, int N, int K, int kq = 32) {
  p.A = (const char*)A; p.W = (const char*)W;
  p.lda_b = lda * 2; p.ldw_b = ldw * 2;
  p.M = M; p.N = N; p.K = K; p.nkt = K / kq;     // kq = elements per 128-byte k tile
}

// osz = bytes per element of the output format (HL8: 2, the offsets count fp16 elements)
static inline void gm_set_batch(GemmParams& p, int n_inner, long a_outer, long a_inner, long w_outer, long w_inner, long o_outer, long o_inner,
                                long osz) {
  p.nbi = n_inner;
  p.a_bo = a_outer * 2; p.a_bi = a_inner * 2; p.w_bo = w_outer * 2; p.w_bi = w_inner * 2; p.o_bo = o_outer * osz; p.o_bi = o_inner * osz;
}

// ---- host: the argument checks the entry points share.  `who` is the entry point's name, the prefix of its messages; the result is 0 or
// HIPIE_EINVAL with the message set (use through HIPIE_TRY) ----
// operand rows: at least epr fp16 elements, 16-byte pieces; the kernels address a tile's rows with 32-bit byte offsets from the tile's
// first row: 256 rows of A, bn (the widest column tile the entry point can take: 320 | 256) rows of W
static inline int gm_check_operands(const char* who, long lda, long ldw, int epr, int bn) {
  if (!(lda >= epr && ldw >= epr && lda % 8 == 0 && ldw % 8 == 0))
    return set_err(HIPIE_EINVAL, "%s: operand row strides %ld / %ld (>= %d, multiples of 8)", who, lda, ldw, epr);
  if (!(256 * lda * 2 < (1L << 31) && bn * ldw * 2 < (1L << 31))) return set_err(HIPIE_EINVAL, "%s: row stride too large", who);
  return 0;
}

static inline int gm_check_out(const char* who, long ldo, int out_fmt, int N) {
  const int opr = out_fmt == HIPIE_HL8 ? 2 * N : N;
  if (!(ldo >= opr && ldo % 4 == 0)) return set_err(HIPIE_EINVAL, "%s: output row stride %ld (>= %d)", who, ldo, opr);
  return 0;
}

static inline int gm_check_resid(const char* who, const float* resid, long ldr, int N) {
  if (!(resid == nullptr || (ldr >= N && ldr % 4 == 0))) return set_err(HIPIE_EINVAL, "%s: residual row stride %ld", who, ldr);
  return 0;
}

// batched forms: one (outer, inner) problem per blockIdx.y
static inline int gm_check_batch_shape(const char* who, int n_outer, int n_inner) {
  if (!(n_outer > 0 && n_inner > 0 && (long)n_outer * n_inner <= 65535)) return set_err(HIPIE_EINVAL, "%s: %d x %d problems", who, n_outer, n_inner);
  return 0;
}

static inline int gm_check_batch_offsets(const char* who, long a_outer, long a_inner, long w_outer, long w_inner, long o_outer, long o_inner) {
  if (!(((a_outer | a_inner | w_outer | w_inner) % 8) == 0 && ((o_outer | o_inner) % 4) == 0))
    return set_err(HIPIE_EINVAL, "%s: batch offsets must keep 16-byte alignment", who);
  return 0;
}

static inline int gm_check_aligned(const char* who, std::initializer_list<const void*> ptrs) {
  for (const void* q : ptrs)
    if ((uintptr_t)q % 16 != 0) return set_err(HIPIE_EINVAL, "%s: pointers must be 16-byte aligned", who);
  return 0;
}

}  // namespace hipie
