// attn_train_tile.h -- the fused training attention, forward + backward, split-fp16 operands: the three kernels, their staging
// and their launchers, ONCE, for the two instances that are built from them:
//     attn_train.hip      the GLOBAL ViT blocks:   224 operand columns, 128-row workgroups, N a multiple of 128
//     attn_train_win.hip  the WINDOWED ViT blocks: 128 operand columns, one workgroup per item of 1 <= N <= 256 tokens, no row padding
//
// What it replaces: Attention.forward between the qkv and proj Linears, hipie/backbone/vit.py:69-80, with add_decomposed_rel_pos
// (hipie/backbone/utils.py:96-125) folded into the operands by the caller (hipie_amd/training/net.vit_attention):
//     q' = [scale q, rel_h(q, :), rel_w(q, :), 0..]   k' = [k, onehot(key row), onehot(key column), 0..]      (DQ columns; a 14 x 14 window has 108)
//     O = softmax(q' k'^T) v          and its gradients dq' (whose columns 80.. are d rel_h / d rel_w), dk (the first 80 columns of dk'), dv
// so the kernels are a PLAIN attention with d_qk = DQ and d_v = 80 -- no (heads, N, N) tensor in HBM, forward or backward (the materialised
// formulation is 12.3 ms per ViT-H block at two 1024^2 images and keeps 2 GB per block alive for the backward).
//
// Arithmetic: every operand is an fp16 pair (hi = fp16(x), lo = fp16(x - hi)) and every product is three v_mfma_f32_16x16x32_f16 (hi hi,
// hi lo, lo hi) accumulated in fp32 -- the library's split form (hipie_gemm, vit_attn_split.hip), 2.7 x the rate of the fp32 matrix pipe
// the library GEMMs of the materialised formulation run on.  P and dS are split again in registers, as 2^12 p and 16 dS.  The caller scales
// dO by a power of two into fp16's normal range and scales the gradients back.
//
// Lane layout of v_mfma_f32_16x16x32_f16 (c = lane & 15, g = lane >> 4): A: row c, 8 k-values of k-group g; B: column c, the same 8
// k-values; C/D: rows 4 g + i (i = 0..3), column c.  The contraction index is a dummy: A and B only have to agree on which value sits in
// slot (g, j).  Two C tiles of the logits therefore ARE one operand of the next product over keys / queries (slots j = 0..3 from tile t,
// 4..7 from tile t + 1: keys 16 t + 4 g + j), and the other operand reads the same 2 x 4 ROWS of a row-major LDS tile with ds_read_b64_tr_b16.
//
// Shape.  An ITEM is one head (global) or one (window, head): N tokens, dense in HBM.  A wave owns QT 16-row tiles of it (queries, or keys
// in backward 1), a workgroup 16 QT WAVES rows; the other side streams through LDS in TR-row tiles:
//     forward    S^T = K' Q'^T per TR-key tile, online softmax per query column, O^T += V^T P^T
//     backward 1 per TR-query tile  S = Q' K'^T, P = exp(S - lse), dP = dO V^T, dS = P (dP - delta), dV += P^T dO, dK += dS^T Q'[:, :80]
//     backward 2 per TR-key tile    S^T, P^T, dP^T = V dO^T, dS^T, dQ'^T += K'^T dS^T
// (two backward kernels: a single one would have to reduce dK / dV or dQ' across the waves through LDS.)  All three are software-pipelined:
// the next tile travels global -> registers while the current one is computed on, then into the other LDS buffer; one barrier per tile.
//     global:   QT = 1, 8 waves, grid N/128 x BH (at_locate places the workgroups of a head on one XCD)
//     windowed: QT = 2, so every k' / v (q' / dO) fragment read from LDS feeds two MFMA chains -- with one tile per wave the 4-k-step loop
//               is bound by the LDS reads, not by the MFMAs.  ONE workgroup per item, sized from it:
//               N <= 128: 4 waves      N <= 224: 7 waves (a 196-token window: 13 of 14 tiles live, 7 streamed tiles)      N <= 256: 8 waves
//
// Rows beyond N exist only in a RAGGED instance (the windowed one).  Every row index is clamped to N - 1 before it becomes an address (the
// tile then holds copies of the item's last row: finite data of the SAME item; no other item's rows and nothing past the last item are
// read).  Masking is by index:
//     forward / backward 2: a key >= N gets logit -inf before the row maximum / dS^T = 0, so its probability is exactly 0;
//     backward 1: p = dS = 0 for a query >= N (it would otherwise be added into dK / dV) and for a key >= N;
//     outputs (O, lse, dq', dk, dv) are stored for rows < N only.
// A non-ragged instance compiles to code with none of this.
//
// Budget per workgroup (figures of the gfx950 build).
//     global    LDS  forward 80 KB, backward 1 84.5 KB, backward 2 84 KB at TR = 32: past the default dynamic limit of 64 KB, hence the
//                    LdsLimit of the launchers
//               VGPR forward 171, backward 1 256 (the limit of 512 threads, no spill), backward 2 236
//     windowed, 7 waves (the 196-token window)
//               LDS  forward 56.0 KB (2 x (k' pair 32 x 136 + v pair 32 x 88) halfs), backward 1 60.5 KB (q' pair + dO pair 32 x 104, lse,
//                    delta), backward 2 60.0 KB: within the default dynamic limit, two workgroups per CU by LDS
//               VGPR the launch bounds (448 / 512 threads: two waves per SIMD) allow 256.  forward 244, no spill.  backward 1 256 with 78
//                    registers spilled (220 bytes of scratch per lane: the owned k' / v fragments 112, the dK / dV accumulators 80, P and dS
//                    32, the prefetch 25); backward 2 256 with 23 spilled.  The spills are the known cost of two tiles per wave in the
//                    backward; see docs/next_round.md.
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

// One instance of the kernels: DQ_ operand columns (224 | 128), QT_ 16-row tiles per wave, WAVES_ waves per workgroup, TR_ rows of the
// tile that streams through LDS per step, RAGGED_: items of any length (see above).  Everything else follows.
template <int DQ_, int QT_, int WAVES_, int TR_, bool RAGGED_> struct AtCfg {
  static constexpr int DQ = DQ_, QT = QT_, WAVES = WAVES_, TR = TR_;
  static constexpr bool RAGGED = RAGGED_;
  static constexpr int KSTEPS = DQ / 32;            // MFMA k-steps of a q' k'^T product
  static constexpr int DQ_TILES = DQ / 16;          // 16-column tiles of dQ'
  static constexpr int KS = DQ + 8;                 // row stride (halfs) of a row-major q' / k' tile in LDS
  static constexpr int NT = TR / 16;                // 16-row tiles of a streamed tile
  static constexpr int THREADS = 64 * WAVES, WG_ROWS = 16 * QT * WAVES;
  // halfs per LDS buffer: forward k' pair + v pair; backward 1 q' pair + dO pair + lse and delta (floats); backward 2 k' pair + v pair
  static constexpr int kFwdBuf = 2 * TR * KS + 2 * TR * AT_VS;
  static constexpr int kBwdKvBuf = 2 * TR * KS + 2 * TR * AT_DS + 4 * TR;
  static constexpr int kBwdQBuf = 2 * TR * KS + 2 * TR * AT_DS;
  static constexpr size_t kFwdLds = 2 * kFwdBuf * sizeof(f16_t), kBwdKvLds = 2 * kBwdKvBuf * sizeof(f16_t),        // two buffers
                          kBwdQLds = 2 * kBwdQBuf * sizeof(f16_t);
  static_assert(DQ % 32 == 0 && TR % 32 == 0 && kFwdLds <= 160 * 1024 && kBwdKvLds <= 160 * 1024 && kBwdQLds <= 160 * 1024, "LDS budget");
};

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

// workgroup -> (first row of its item in the (BH N)-row operands, first of its rows within the item).
// Non-ragged: (head bh, WG_ROWS-row block).  With BH a multiple of 8, the workgroups of ONE head run on ONE XCD (the dispatcher places
// workgroup id on XCD id % 8): the 32 workgroups of a 4096-token head stream the same 5 MB of k' / v (or q' / dO) tiles, which then live in
// that XCD's 4 MB L2 instead of eight heads' tiles competing for it.  A placement hint only.
// Ragged: one workgroup per item.
template <class C> __device__ __forceinline__ void at_locate(int N, int BH, long& item, int& row0) {
  if constexpr (C::RAGGED) {
    item = (long)blockIdx.x * N;
    row0 = 0;
  } else {
    const int id = blockIdx.x, per_head = N / C::WG_ROWS;
    if ((BH & 7) == 0) {
      const int w = id >> 3;
      item = ((long)(w / per_head) * 8 + (id & 7)) * N;
      row0 = (w % per_head) * C::WG_ROWS;
    } else {
      item = (long)(id / per_head) * N;
      row0 = (id % per_head) * C::WG_ROWS;
    }
  }
}

// row `r` of an item as a row of the operands; a ragged item's rows >= N read its row N - 1
template <class C> __device__ __forceinline__ long at_row(long item, int r, int N) {
  if constexpr (C::RAGGED) r = min(r, N - 1);
  return item + r;
}

// Staging of a streamed tile (rows row0 .. row0 + TR - 1 of ONE item, COLS halfs each, dense -> row-major LDS tile with a padded row stride)
// in two halves, for the software pipeline of all three kernels: global -> registers (in flight while the current tile is computed on),
// registers -> the OTHER LDS buffer, one barrier per tile.  (Keeping each thread's LDS offsets in registers instead of recomputing idx /
// chunks-per-row every tile removes 130 VALU instructions per tile and is 15 % SLOWER -- measured on one box; not kept.)
template <class C, int COLS> struct AtStage {
  static constexpr int kCpr = COLS / 8, kChunks = C::TR * kCpr, kPer = (kChunks + C::THREADS - 1) / C::THREADS;
  at_frag r[kPer];
  // Branch-free on purpose: threads beyond the tile's last chunk re-load and re-store that chunk (same value, same address).  With the
  // loads under `if (idx < kChunks)` the compiler put an s_waitcnt vmcnt(0) between them -- six serialised L2 round trips at the top of
  // every tile instead of six loads in flight behind the compute.
  __device__ __forceinline__ void fetch(const f16_t* plane, long item, int row0, int n, int tid) {
    const f16_t* src = plane + (item + (C::RAGGED ? 0 : row0)) * COLS;        // ragged: row0 stays in the index, which is clamped row by row
#pragma unroll
    for (int k = 0; k < kPer; ++k) {
      const int idx = min(tid + k * C::THREADS, kChunks - 1);
      int row = idx / kCpr;
      if constexpr (C::RAGGED) row = min(row0 + row, n - 1);
      r[k] = *reinterpret_cast<const at_frag*>(src + row * COLS + (idx % kCpr) * 8);
    }
  }
  __device__ __forceinline__ void commit(f16_t* dst, int ls, int tid) const {
#pragma unroll
    for (int k = 0; k < kPer; ++k) {
      const int idx = min(tid + k * C::THREADS, kChunks - 1);
      *reinterpret_cast<at_frag*>(dst + (idx / kCpr) * ls + (idx % kCpr) * 8) = r[k];
    }
  }
};

// ---- forward: a wave owns 16 QT queries, the keys stream through LDS ---------------------------------------------------------------------
template <class C>
__global__ __launch_bounds__(C::THREADS) void at_fwd_kernel(const f16_t* __restrict__ Qh, const f16_t* __restrict__ Ql,
                                                            const f16_t* __restrict__ Kh, const f16_t* __restrict__ Kl,
                                                            const f16_t* __restrict__ Vh, const f16_t* __restrict__ Vl,
                                                            float* __restrict__ O, float* __restrict__ LSE, int N, int BH) {
  extern __shared__ __attribute__((aligned(16))) char at_smem[];
  constexpr int DQ = C::DQ, KS = C::KS, TR = C::TR, NT = C::NT, QT = C::QT, kBuf = C::kFwdBuf;
  f16_t* sbase = reinterpret_cast<f16_t*>(at_smem);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, c = lane & 15, g = lane >> 4;
  long item;
  int row0;
  at_locate<C>(N, BH, item, row0);
  const int q0 = row0 + wave * 16 * QT;
  at_frag qh[QT][C::KSTEPS], ql[QT][C::KSTEPS];
#pragma unroll
  for (int qt = 0; qt < QT; ++qt) {
    const long row = at_row<C>(item, q0 + 16 * qt + c, N) * DQ + 8 * g;
#pragma unroll
    for (int s = 0; s < C::KSTEPS; ++s) {
      qh[qt][s] = *reinterpret_cast<const at_frag*>(Qh + row + 32 * s);
      ql[qt][s] = *reinterpret_cast<const at_frag*>(Ql + row + 32 * s);
    }
  }
  f32x4 o[QT][5];
  float m[QT], lsum[QT];
#pragma unroll
  for (int qt = 0; qt < QT; ++qt) {
    m[qt] = -INFINITY;
    lsum[qt] = 0.f;
#pragma unroll
    for (int j = 0; j < 5; ++j) o[qt][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  AtStage<C, DQ> fkh, fkl;
  AtStage<C, AT_DV> fvh, fvl;
  auto fetch = [&](int kb) {
    fkh.fetch(Kh, item, kb, N, tid);
    fkl.fetch(Kl, item, kb, N, tid);
    fvh.fetch(Vh, item, kb, N, tid);
    fvl.fetch(Vl, item, kb, N, tid);
  };
  auto commit = [&](int buf) {
    f16_t* b = sbase + buf * kBuf;
    fkh.commit(b, KS, tid);
    fkl.commit(b + TR * KS, KS, tid);
    fvh.commit(b + 2 * TR * KS, AT_VS, tid);
    fvl.commit(b + 2 * TR * KS + TR * AT_VS, AT_VS, tid);
  };
  fetch(0);
  commit(0);
  __syncthreads();
  for (int kb = 0, it = 0; kb < N; kb += TR, ++it) {
    const bool more = kb + TR < N;
    if (more) fetch(kb + TR);
    const f16_t* sKh = sbase + (it & 1) * kBuf;
    const f16_t* sKl = sKh + TR * KS;
    const f16_t* sVh = sKl + TR * KS;
    const f16_t* sVl = sVh + TR * AT_VS;
    f32x4 acc[QT][NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
#pragma unroll
      for (int qt = 0; qt < QT; ++qt) acc[qt][t] = f32x4{0.f, 0.f, 0.f, 0.f};
      const int off = (16 * t + c) * KS + 8 * g;
#pragma unroll
      for (int s = 0; s < C::KSTEPS; ++s) {
        const at_frag kh = *reinterpret_cast<const at_frag*>(sKh + off + 32 * s), kl = *reinterpret_cast<const at_frag*>(sKl + off + 32 * s);
#pragma unroll
        for (int qt = 0; qt < QT; ++qt) acc[qt][t] = at_mma3(kh, kl, qh[qt][s], ql[qt][s], acc[qt][t]);   // S^T: rows = keys 16 t + 4 g + i, column = query c
      }
    }
    at_frag ph[QT][NT / 2], pl[QT][NT / 2];
#pragma unroll
    for (int qt = 0; qt < QT; ++qt) {
      if constexpr (C::RAGGED) {
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
          for (int i = 0; i < 4; ++i)
            if (kb + 16 * t + 4 * g + i >= N) acc[qt][t][i] = -INFINITY;        // a key beyond the item: probability exactly 0 (key kb is always live)
      }
      float mx = acc[qt][0][0];
#pragma unroll
      for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int i = 0; i < 4; ++i) mx = fmaxf(mx, acc[qt][t][i]);
      mx = fmaxf(mx, __shfl_xor(mx, 16));
      mx = fmaxf(mx, __shfl_xor(mx, 32));
      const float mn = fmaxf(m[qt], mx);
      const float alpha = __expf(m[qt] - mn);
      m[qt] = mn;
      lsum[qt] *= alpha;
#pragma unroll
      for (int j = 0; j < 5; ++j) o[qt][j] *= alpha;
#pragma unroll
      for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          acc[qt][t][i] = __expf(acc[qt][t][i] - mn + kAtShift);                // 2^12 p: its fp16 pair is exact to 2^-22 down to p = 2^-16
          lsum[qt] += acc[qt][t][i];
        }
#pragma unroll
      for (int tp = 0; tp < NT; tp += 2) at_split8(acc[qt][tp], acc[qt][tp + 1], ph[qt][tp / 2], pl[qt][tp / 2]);
    }
#pragma unroll
    for (int tp = 0; tp < NT; tp += 2)
#pragma unroll
      for (int j = 0; j < 5; ++j) {
        const at_frag vh = at_rows8(sVh, AT_VS, tp, 16 * j, c, g), vl = at_rows8(sVl, AT_VS, tp, 16 * j, c, g);
#pragma unroll
        for (int qt = 0; qt < QT; ++qt) o[qt][j] = at_mma3(vh, vl, ph[qt][tp / 2], pl[qt][tp / 2], o[qt][j]);   // O^T: rows = d 16 j + 4 g + i, column = query c
      }
    if (more) commit((it & 1) ^ 1);
    __syncthreads();
  }
#pragma unroll
  for (int qt = 0; qt < QT; ++qt) {
    float ltot = lsum[qt];
    ltot += __shfl_xor(ltot, 16);
    ltot += __shfl_xor(ltot, 32);
    const float inv = 1.f / ltot;
    const int q = q0 + 16 * qt + c;
    if (!C::RAGGED || q < N) {
      float* orow = O + (item + q) * AT_DV + 4 * g;
#pragma unroll
      for (int j = 0; j < 5; ++j)
        *reinterpret_cast<float4*>(orow + 16 * j) = make_float4(o[qt][j][0] * inv, o[qt][j][1] * inv, o[qt][j][2] * inv, o[qt][j][3] * inv);
      if (g == 0) LSE[item + q] = m[qt] + logf(ltot) - kAtShift;
    }
  }
}

// ---- backward 1: dK (the first 80 columns of dK') and dV; a wave owns 16 QT keys, the queries stream through LDS ---------------------------
template <class C>
__global__ __launch_bounds__(C::THREADS) void at_bwd_kv_kernel(const f16_t* __restrict__ Qh, const f16_t* __restrict__ Ql,
                                                               const f16_t* __restrict__ Kh, const f16_t* __restrict__ Kl,
                                                               const f16_t* __restrict__ Vh, const f16_t* __restrict__ Vl,
                                                               const f16_t* __restrict__ Dh, const f16_t* __restrict__ Dl,
                                                               const float* __restrict__ LSE, const float* __restrict__ DELTA,
                                                               float* __restrict__ dK, float* __restrict__ dV, int N, int BH) {
  extern __shared__ __attribute__((aligned(16))) char at_smem[];
  constexpr int DQ = C::DQ, KS = C::KS, TR = C::TR, NT = C::NT, QT = C::QT, kBuf = C::kBwdKvBuf;
  f16_t* sbase = reinterpret_cast<f16_t*>(at_smem);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, c = lane & 15, g = lane >> 4;
  long item;
  int row0;
  at_locate<C>(N, BH, item, row0);
  const int k0 = row0 + wave * 16 * QT;
  at_frag kh[QT][C::KSTEPS], kl[QT][C::KSTEPS], vh[QT][3], vl[QT][3];
#pragma unroll
  for (int kt = 0; kt < QT; ++kt) {
    const long r = at_row<C>(item, k0 + 16 * kt + c, N);
#pragma unroll
    for (int s = 0; s < C::KSTEPS; ++s) {
      kh[kt][s] = *reinterpret_cast<const at_frag*>(Kh + r * DQ + 8 * g + 32 * s);
      kl[kt][s] = *reinterpret_cast<const at_frag*>(Kl + r * DQ + 8 * g + 32 * s);
    }
#pragma unroll
    for (int s = 0; s < 3; ++s) {
      vh[kt][s] = *reinterpret_cast<const at_frag*>(Vh + r * AT_DVP + 8 * g + 32 * s);
      vl[kt][s] = *reinterpret_cast<const at_frag*>(Vl + r * AT_DVP + 8 * g + 32 * s);
    }
  }
  f32x4 dv[QT][5], dk[QT][5];
#pragma unroll
  for (int kt = 0; kt < QT; ++kt)
#pragma unroll
    for (int j = 0; j < 5; ++j) dv[kt][j] = dk[kt][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  AtStage<C, DQ> fqh, fql;
  AtStage<C, AT_DVP> fdh, fdl;
  float fstat = 0.f;
  const int si = min(tid, 2 * TR - 1);                                          // branch-free: threads beyond 2 TR repeat the last entry
  auto fetch = [&](int qb) {
    fqh.fetch(Qh, item, qb, N, tid);
    fql.fetch(Ql, item, qb, N, tid);
    fdh.fetch(Dh, item, qb, N, tid);
    fdl.fetch(Dl, item, qb, N, tid);
    fstat = (si < TR ? LSE : DELTA)[at_row<C>(item, qb + (si < TR ? si : si - TR), N)];
  };
  auto commit = [&](int buf) {
    f16_t* b = sbase + buf * kBuf;
    fqh.commit(b, KS, tid);
    fql.commit(b + TR * KS, KS, tid);
    fdh.commit(b + 2 * TR * KS, AT_DS, tid);
    fdl.commit(b + 2 * TR * KS + TR * AT_DS, AT_DS, tid);
    reinterpret_cast<float*>(b + 2 * TR * KS + 2 * TR * AT_DS)[si] = fstat;
  };
  fetch(0);
  commit(0);
  __syncthreads();
  for (int qb = 0, it = 0; qb < N; qb += TR, ++it) {
    const bool more = qb + TR < N;
    if (more) fetch(qb + TR);                                                   // in flight while this tile is computed on
    const f16_t* sQh = sbase + (it & 1) * kBuf;
    const f16_t* sQl = sQh + TR * KS;
    const f16_t* sDh = sQl + TR * KS;
    const f16_t* sDl = sDh + TR * AT_DS;
    const float* sLse = reinterpret_cast<const float*>(sDl + TR * AT_DS);
    const float* sDel = sLse + TR;
    f32x4 p[QT][NT], ds[QT][NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      f32x4 acc[QT], dp[QT];
#pragma unroll
      for (int kt = 0; kt < QT; ++kt) acc[kt] = dp[kt] = f32x4{0.f, 0.f, 0.f, 0.f};
      const int off = (16 * t + c) * KS + 8 * g;
#pragma unroll
      for (int s = 0; s < C::KSTEPS; ++s) {
        const at_frag ah = *reinterpret_cast<const at_frag*>(sQh + off + 32 * s), al = *reinterpret_cast<const at_frag*>(sQl + off + 32 * s);
#pragma unroll
        for (int kt = 0; kt < QT; ++kt) acc[kt] = at_mma3(ah, al, kh[kt][s], kl[kt][s], acc[kt]);         // S: rows = queries 16 t + 4 g + i, column = key c
      }
      const int doff = (16 * t + c) * AT_DS + 8 * g;
#pragma unroll
      for (int s = 0; s < 3; ++s) {
        const at_frag ah = *reinterpret_cast<const at_frag*>(sDh + doff + 32 * s), al = *reinterpret_cast<const at_frag*>(sDl + doff + 32 * s);
#pragma unroll
        for (int kt = 0; kt < QT; ++kt) dp[kt] = at_mma3(ah, al, vh[kt][s], vl[kt][s], dp[kt]);           // dP = dO v^T, same layout
      }
      const float4 l4 = *reinterpret_cast<const float4*>(sLse + 16 * t + 4 * g), d4 = *reinterpret_cast<const float4*>(sDel + 16 * t + 4 * g);
      const float lq[4] = {l4.x, l4.y, l4.z, l4.w}, dq_[4] = {d4.x, d4.y, d4.z, d4.w};
#pragma unroll
      for (int kt = 0; kt < QT; ++kt)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const bool live = !C::RAGGED || (qb + 16 * t + 4 * g + i < N && k0 + 16 * kt + c < N);   // a padding query would be summed into dK / dV
          const float pv = live ? __expf(acc[kt][i] - lq[i]) : 0.f;
          p[kt][t][i] = pv * 4096.f;
          ds[kt][t][i] = pv * (dp[kt][i] - dq_[i]) * kAtDsScale;
        }
    }
#pragma unroll
    for (int tp = 0; tp < NT; tp += 2) {
      at_frag ph[QT], pl[QT], sh[QT], sl[QT];
#pragma unroll
      for (int kt = 0; kt < QT; ++kt) {
        at_split8(p[kt][tp], p[kt][tp + 1], ph[kt], pl[kt]);
        at_split8(ds[kt][tp], ds[kt][tp + 1], sh[kt], sl[kt]);
      }
#pragma unroll
      for (int j = 0; j < 5; ++j) {
        const at_frag doh = at_rows8(sDh, AT_DS, tp, 16 * j, c, g), dol = at_rows8(sDl, AT_DS, tp, 16 * j, c, g);
        const at_frag qqh = at_rows8(sQh, KS, tp, 16 * j, c, g), qql = at_rows8(sQl, KS, tp, 16 * j, c, g);
#pragma unroll
        for (int kt = 0; kt < QT; ++kt) {
          dv[kt][j] = at_mma3(ph[kt], pl[kt], doh, dol, dv[kt][j]);             // dV: rows = keys 4 g + i, column = d 16 j + c
          dk[kt][j] = at_mma3(sh[kt], sl[kt], qqh, qql, dk[kt][j]);             // dK: rows = keys, column = dim 16 j + c
        }
      }
    }
    if (more) commit((it & 1) ^ 1);                                             // the other buffer: everyone left it at the previous barrier
    __syncthreads();
  }
#pragma unroll
  for (int kt = 0; kt < QT; ++kt)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int key = k0 + 16 * kt + 4 * g + i;
      if (!C::RAGGED || key < N) {
#pragma unroll
        for (int j = 0; j < 5; ++j) {
          const long at = (item + key) * AT_DV + 16 * j + c;
          dV[at] = dv[kt][j][i] * (1.f / 4096.f);
          dK[at] = dk[kt][j][i] * (1.f / kAtDsScale);
        }
      }
    }
}

// ---- backward 2: dQ' (all DQ columns); a wave owns 16 QT queries, the keys stream through LDS ----------------------------------------------
template <class C>
__global__ __launch_bounds__(C::THREADS) void at_bwd_q_kernel(const f16_t* __restrict__ Qh, const f16_t* __restrict__ Ql,
                                                              const f16_t* __restrict__ Kh, const f16_t* __restrict__ Kl,
                                                              const f16_t* __restrict__ Vh, const f16_t* __restrict__ Vl,
                                                              const f16_t* __restrict__ Dh, const f16_t* __restrict__ Dl,
                                                              const float* __restrict__ LSE, const float* __restrict__ DELTA,
                                                              float* __restrict__ dQ, int N, int BH) {
  extern __shared__ __attribute__((aligned(16))) char at_smem[];
  constexpr int DQ = C::DQ, KS = C::KS, TR = C::TR, NT = C::NT, QT = C::QT, kBuf = C::kBwdQBuf;
  f16_t* sbase = reinterpret_cast<f16_t*>(at_smem);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, c = lane & 15, g = lane >> 4;
  long item;
  int row0;
  at_locate<C>(N, BH, item, row0);
  const int q0 = row0 + wave * 16 * QT;
  at_frag qh[QT][C::KSTEPS], ql[QT][C::KSTEPS], dh[QT][3], dl[QT][3];
  float lse[QT], delta[QT];
#pragma unroll
  for (int qt = 0; qt < QT; ++qt) {
    const long r = at_row<C>(item, q0 + 16 * qt + c, N);
#pragma unroll
    for (int s = 0; s < C::KSTEPS; ++s) {
      qh[qt][s] = *reinterpret_cast<const at_frag*>(Qh + r * DQ + 8 * g + 32 * s);
      ql[qt][s] = *reinterpret_cast<const at_frag*>(Ql + r * DQ + 8 * g + 32 * s);
    }
#pragma unroll
    for (int s = 0; s < 3; ++s) {
      dh[qt][s] = *reinterpret_cast<const at_frag*>(Dh + r * AT_DVP + 8 * g + 32 * s);
      dl[qt][s] = *reinterpret_cast<const at_frag*>(Dl + r * AT_DVP + 8 * g + 32 * s);
    }
    lse[qt] = LSE[r];
    delta[qt] = DELTA[r];
  }
  f32x4 dq[QT][C::DQ_TILES];
#pragma unroll
  for (int qt = 0; qt < QT; ++qt)
#pragma unroll
    for (int j = 0; j < C::DQ_TILES; ++j) dq[qt][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  AtStage<C, DQ> fkh, fkl;
  AtStage<C, AT_DVP> fvh, fvl;
  auto fetch = [&](int kb) {
    fkh.fetch(Kh, item, kb, N, tid);
    fkl.fetch(Kl, item, kb, N, tid);
    fvh.fetch(Vh, item, kb, N, tid);
    fvl.fetch(Vl, item, kb, N, tid);
  };
  auto commit = [&](int buf) {
    f16_t* b = sbase + buf * kBuf;
    fkh.commit(b, KS, tid);
    fkl.commit(b + TR * KS, KS, tid);
    fvh.commit(b + 2 * TR * KS, AT_DS, tid);
    fvl.commit(b + 2 * TR * KS + TR * AT_DS, AT_DS, tid);
  };
  fetch(0);
  commit(0);
  __syncthreads();
  for (int kb = 0, it = 0; kb < N; kb += TR, ++it) {
    const bool more = kb + TR < N;
    if (more) fetch(kb + TR);
    const f16_t* sKh = sbase + (it & 1) * kBuf;
    const f16_t* sKl = sKh + TR * KS;
    const f16_t* sVh = sKl + TR * KS;
    const f16_t* sVl = sVh + TR * AT_DS;
    f32x4 ds[QT][NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      f32x4 acc[QT], dp[QT];
#pragma unroll
      for (int qt = 0; qt < QT; ++qt) acc[qt] = dp[qt] = f32x4{0.f, 0.f, 0.f, 0.f};
      const int off = (16 * t + c) * KS + 8 * g;
#pragma unroll
      for (int s = 0; s < C::KSTEPS; ++s) {
        const at_frag ah = *reinterpret_cast<const at_frag*>(sKh + off + 32 * s), al = *reinterpret_cast<const at_frag*>(sKl + off + 32 * s);
#pragma unroll
        for (int qt = 0; qt < QT; ++qt) acc[qt] = at_mma3(ah, al, qh[qt][s], ql[qt][s], acc[qt]);         // S^T: rows = keys 16 t + 4 g + i, column = query c
      }
      const int voff = (16 * t + c) * AT_DS + 8 * g;
#pragma unroll
      for (int s = 0; s < 3; ++s) {
        const at_frag ah = *reinterpret_cast<const at_frag*>(sVh + voff + 32 * s), al = *reinterpret_cast<const at_frag*>(sVl + voff + 32 * s);
#pragma unroll
        for (int qt = 0; qt < QT; ++qt) dp[qt] = at_mma3(ah, al, dh[qt][s], dl[qt][s], dp[qt]);           // dP^T = v dO^T, same layout
      }
#pragma unroll
      for (int qt = 0; qt < QT; ++qt)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const bool live = !C::RAGGED || kb + 16 * t + 4 * g + i < N;          // a key beyond the item: probability exactly 0
          ds[qt][t][i] = live ? __expf(acc[qt][i] - lse[qt]) * (dp[qt][i] - delta[qt]) * kAtDsScale : 0.f;
        }
    }
#pragma unroll
    for (int tp = 0; tp < NT; tp += 2) {
      at_frag sh[QT], sl[QT];
#pragma unroll
      for (int qt = 0; qt < QT; ++qt) at_split8(ds[qt][tp], ds[qt][tp + 1], sh[qt], sl[qt]);
#pragma unroll
      for (int j = 0; j < C::DQ_TILES; ++j) {
        const at_frag kkh = at_rows8(sKh, KS, tp, 16 * j, c, g), kkl = at_rows8(sKl, KS, tp, 16 * j, c, g);
#pragma unroll
        for (int qt = 0; qt < QT; ++qt) dq[qt][j] = at_mma3(kkh, kkl, sh[qt], sl[qt], dq[qt][j]);         // dQ'^T: rows = dims 16 j + 4 g + i, column = query c
      }
    }
    if (more) commit((it & 1) ^ 1);
    __syncthreads();
  }
#pragma unroll
  for (int qt = 0; qt < QT; ++qt) {
    const int q = q0 + 16 * qt + c;
    if (!C::RAGGED || q < N) {
      float* out = dQ + (item + q) * DQ + 4 * g;
#pragma unroll
      for (int j = 0; j < C::DQ_TILES; ++j)
        *reinterpret_cast<float4*>(out + 16 * j) = make_float4(dq[qt][j][0] * (1.f / kAtDsScale), dq[qt][j][1] * (1.f / kAtDsScale),
                                                               dq[qt][j][2] * (1.f / kAtDsScale), dq[qt][j][3] * (1.f / kAtDsScale));
    }
  }
}

// ---- host: the entry check and the launchers of both instances ---------------------------------------------------------------------------
// `n_ok` / `rule`: the instance's condition on N and its wording
static inline int at_check(const char* who, bool pointers, int BH, int N, bool n_ok, const char* rule) {
  HIPIE_REQUIRE(pointers, "%s: null pointer", who);
  HIPIE_REQUIRE(BH > 0 && N > 0 && n_ok, "%s: BH=%d N=%d (%s)", who, BH, N, rule);
  return 0;
}

// dynamic LDS of one kernel instantiation: above the default limit only for the global instance (one LdsLimit per instantiation)
template <class C, size_t LDS> static void at_lds(const void* kernel) {
  if constexpr (LDS > 64 * 1024) {
    static LdsLimit limit;
    limit.raise(kernel, LDS);
  }
}

struct AtArgs {      // the operands of hipie_attn_train*_forward / _backward, as the entries receive them
  const void *q_hi, *q_lo, *k_hi, *k_lo, *v_hi, *v_lo, *do_hi, *do_lo, *lse, *delta;
  void *out, *lse_out, *dq, *dk, *dv;
};

template <class C> static void at_forward(hipStream_t st, unsigned grid, const AtArgs& a, int BH, int N) {
  at_lds<C, C::kFwdLds>((const void*)at_fwd_kernel<C>);
  hipLaunchKernelGGL(at_fwd_kernel<C>, dim3(grid), dim3(C::THREADS), C::kFwdLds, st, (const f16_t*)a.q_hi, (const f16_t*)a.q_lo, (const f16_t*)a.k_hi,
                     (const f16_t*)a.k_lo, (const f16_t*)a.v_hi, (const f16_t*)a.v_lo, (float*)a.out, (float*)a.lse_out, N, BH);
}

template <class C> static void at_backward(hipStream_t st, unsigned grid, const AtArgs& a, int BH, int N) {
  at_lds<C, C::kBwdKvLds>((const void*)at_bwd_kv_kernel<C>);
  at_lds<C, C::kBwdQLds>((const void*)at_bwd_q_kernel<C>);
  hipLaunchKernelGGL(at_bwd_kv_kernel<C>, dim3(grid), dim3(C::THREADS), C::kBwdKvLds, st, (const f16_t*)a.q_hi, (const f16_t*)a.q_lo, (const f16_t*)a.k_hi,
                     (const f16_t*)a.k_lo, (const f16_t*)a.v_hi, (const f16_t*)a.v_lo, (const f16_t*)a.do_hi, (const f16_t*)a.do_lo, (const float*)a.lse,
                     (const float*)a.delta, (float*)a.dk, (float*)a.dv, N, BH);
  hipLaunchKernelGGL(at_bwd_q_kernel<C>, dim3(grid), dim3(C::THREADS), C::kBwdQLds, st, (const f16_t*)a.q_hi, (const f16_t*)a.q_lo, (const f16_t*)a.k_hi,
                     (const f16_t*)a.k_lo, (const f16_t*)a.v_hi, (const f16_t*)a.v_lo, (const f16_t*)a.do_hi, (const f16_t*)a.do_lo, (const float*)a.lse,
                     (const float*)a.delta, (float*)a.dq, N, BH);
}

}  // namespace hipie
