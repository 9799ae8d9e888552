// attn_train_tile.h -- what the instances of the fused training attention share (attn_train.hip: 224 operand columns, 128-row workgroups;
// attn_train_win.hip: 128 columns, one workgroup per short item): the v / dO geometry, the range shifts, the three-product MFMA step, the
// register re-split of two C tiles and the row-contracting LDS operand read.  The lane layout they rely on is in attn_train.hip's header.
#pragma once
#include "common.h"
#include "mfma.h"

namespace hipie {

constexpr int AT_DV = 80;           // columns of v / O
constexpr int AT_DVP = 96;          // v / dO columns as a contraction (3 k-steps), zero padded by the caller
constexpr int AT_VS = AT_DV + 8;    // row stride (halfs) of the forward's row-major v tile in LDS
constexpr int AT_DS = AT_DVP + 8;   // row stride (halfs) of a row-major v / dO tile in LDS

constexpr float kAtShift = 8.317766166719343f;     // 12 ln 2: probabilities enter the P . v / P^T . dO products as 2^12 p (p <= 1 leaves fp16's
                                                    // normal range at 6e-5, and a row of 4096 keys has p ~ 2e-4: the lo half would be a subnormal)
constexpr float kAtDsScale = 16.f;                 // dS = P (dP - delta) is split as 16 dS: with max |dO| in [8, 16) a row of 4096 keys has
                                                    // |dS| ~ 5e-3, whose lo half would be a subnormal; |dS| <= P (1 - P) range(dP) keeps 16 dS in range
typedef f16x8 at_frag;

__device__ __forceinline__ f32x4 at_mma3(at_frag ah, at_frag al, at_frag bh, at_frag bl, f32x4 c) {
  c = __builtin_amdgcn_mfma_f32_16x16x32_f16(al, bh, c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, bl, c, 0, 0, 0);
  return __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, bh, c, 0, 0, 0);
}

// 2 x 4 values (two C tiles) -> one hi / lo operand
__device__ __forceinline__ void at_split8(const f32x4& a, const f32x4& b, at_frag& h, at_frag& l) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    f16_t hh, ll;
    hl_split(a[i], hh, ll);
    h[i] = hh; l[i] = ll;
    hl_split(b[i], hh, ll);
    h[4 + i] = hh; l[4 + i] = ll;
  }
}

// The operand of a product that contracts over the ROWS of a row-major LDS tile (keys or queries): lane (c, g) needs tile[r + j][col + c] for
// the rows r = 16 tp + 4 g + j and 16 (tp + 1) + 4 g + j, j = 0..3 -- two ds_read_b64_tr_b16 (mfma.h: lane c of a 16-lane group points at
// &tile[r0 + c / 4][c0 + 4 (c % 4)] and receives tile[r0 + j][c0 + c]), no transposed copy of the tile.
__device__ __forceinline__ at_frag at_rows8(const f16_t* tile, int ls, int tp, int col, int c, int g) {
  const f16_t* p0 = tile + (16 * tp + 4 * g + (c >> 2)) * ls + col + 4 * (c & 3);
  const f16x4 a = Mfma32<f16_t>::tr_read(p0), b = Mfma32<f16_t>::tr_read(p0 + 16 * ls);
  return __builtin_shufflevector(a, b, 0, 1, 2, 3, 4, 5, 6, 7);
}

}  // namespace hipie
