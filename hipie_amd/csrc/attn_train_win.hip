// attn_train_win.hip -- the short-sequence instance of the fused training attention (attn_train.hip): forward + backward for the WINDOWED ViT
// blocks of the training step, split-fp16 operands.
//
// What it replaces: Attention.forward between the qkv and proj Linears, hipie/backbone/vit.py:69-80, with add_decomposed_rel_pos
// (hipie/backbone/utils.py:96-125) folded into the operands by the caller (hipie_amd/training/net.vit_attention), for the 14 x 14 windows:
//     q' = [scale q, rel_h(q, :), rel_w(q, :), 0..]   k' = [k, onehot(key row), onehot(key column), 0..]      (128 columns; a window has 108)
//     O = softmax(q' k'^T) v          and its gradients dq', dk (the first 80 columns of dk'), dv
// The arithmetic is attn_train.hip's (attn_train_tile.h): fp16 hi / lo pairs, three v_mfma_f32_16x16x32_f16 per product accumulated in fp32,
// P and dS re-split in registers as 2^12 p and 16 dS, dO scaled by a power of two by the caller.  The lane layout is described there.
//
// Shape.  An ITEM is one (window, head): N tokens, 1 <= N <= 256, dense in HBM (no row padding).  ONE workgroup per item; a wave owns TWO
// 16-row tiles (32 queries, or 32 keys in backward 1), so every k' / v (q' / dO) fragment read from LDS feeds two MFMA chains -- with one
// tile per wave the 4-k-step loop is bound by the LDS reads, not by the MFMAs.  The workgroup is sized from the item:
//     N <= 128: 4 waves      N <= 224: 7 waves (a 196-token window: 13 of 14 tiles live)      N <= 256: 8 waves
// The other side streams through LDS in 32-row tiles, double buffered, one barrier per tile (7 tiles for a window).
//     forward    S^T = K' Q'^T per 32-key tile, online softmax per query column, O^T += V^T P^T
//     backward 1 per 32-query tile  S = Q' K'^T, P = exp(S - lse), dP = dO V^T, dS = P (dP - delta), dV += P^T dO, dK += dS^T Q'[:, :80]
//     backward 2 per 32-key tile    S^T, P^T, dP^T = V dO^T, dS^T, dQ'^T += K'^T dS^T
// (the two-kernel split of the global path: a single backward kernel would have to reduce dK / dV or dQ' across the waves through LDS.)
//
// Rows beyond N exist only here.  Every row index is clamped to N - 1 before it becomes an address (the tile then holds copies of the item's
// last row: finite data of the SAME item; no other item's rows and nothing past the last item are read).  Masking is by index:
//     forward / backward 2: a key >= N gets logit -inf before the row maximum / dS^T = 0, so its probability is exactly 0;
//     backward 1: p = dS = 0 for a query >= N (it would otherwise be added into dK / dV) and for a key >= N;
//     outputs (O, lse, dq', dk, dv) are stored for rows < N only.
//
// Budget per workgroup (7 waves, the 196-token window; figures of the gfx950 build):
//     LDS  forward 56.0 KB (2 x (k' pair 32 x 136 + v pair 32 x 88) halfs), backward 1 60.5 KB (q' pair + dO pair 32 x 104, lse, delta),
//          backward 2 60.0 KB: within the default dynamic limit, two workgroups per CU by LDS
//     VGPR the launch bounds (448 / 512 threads: two waves per SIMD) allow 256.  forward 244, no spill.  backward 1 256 with 78 registers
//          spilled (220 bytes of scratch per lane: the owned k' / v fragments 112, the dK / dV accumulators 80, P and dS 32, the prefetch 25);
//          backward 2 256 with 23 spilled.  The spills are the known cost of two tiles per wave in the backward; see docs/next_round.md.
#include "attn_train_tile.h"

namespace hipie {

constexpr int AW_DQ = 128;          // columns of q' / k' (4 MFMA k-steps of 32)
constexpr int AW_KS = AW_DQ + 8;    // row stride (halfs) of a row-major q' / k' tile in LDS
constexpr int AW_TR = 32;           // rows of the tile that streams through LDS per step
constexpr int AW_QT = 2;            // 16-row tiles a wave owns
constexpr int AW_MAX_N = 256;

// Staging of a streamed tile (rows row0 .. row0 + 31 of ONE item, COLS halfs each, dense) -> row-major LDS tile with a padded row stride:
// global -> registers while the current tile is computed on, registers -> the other LDS buffer.  Rows >= n read the item's row n - 1.
// Branch-free like attn_train.hip's AtStage: threads beyond the last chunk repeat it.
template <int COLS, int THREADS> struct AwStage {
  static constexpr int kCpr = COLS / 8, kChunks = AW_TR * kCpr, kPer = (kChunks + THREADS - 1) / THREADS;
  at_frag r[kPer];
  __device__ __forceinline__ void fetch(const f16_t* item, int row0, int n, int tid) {
#pragma unroll
    for (int k = 0; k < kPer; ++k) {
      const int idx = min(tid + k * THREADS, kChunks - 1);
      const int row = min(row0 + idx / kCpr, n - 1);
      r[k] = *reinterpret_cast<const at_frag*>(item + row * COLS + (idx % kCpr) * 8);
    }
  }
  __device__ __forceinline__ void commit(f16_t* dst, int ls, int tid) const {
#pragma unroll
    for (int k = 0; k < kPer; ++k) {
      const int idx = min(tid + k * THREADS, kChunks - 1);
      *reinterpret_cast<at_frag*>(dst + (idx / kCpr) * ls + (idx % kCpr) * 8) = r[k];
    }
  }
};

template <int WAVES>
__global__ __launch_bounds__(64 * WAVES) void attn_win_fwd_kernel(const f16_t* __restrict__ Qh, const f16_t* __restrict__ Ql,
                                                                  const f16_t* __restrict__ Kh, const f16_t* __restrict__ Kl,
                                                                  const f16_t* __restrict__ Vh, const f16_t* __restrict__ Vl,
                                                                  float* __restrict__ O, float* __restrict__ LSE, int N) {
  extern __shared__ __attribute__((aligned(16))) char aw_smem[];
  constexpr int T = 64 * WAVES;
  constexpr int kBuf = 2 * AW_TR * AW_KS + 2 * AW_TR * AT_VS;                   // halfs per buffer: k' pair, v pair
  f16_t* sbase = reinterpret_cast<f16_t*>(aw_smem);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, c = lane & 15, g = lane >> 4;
  const long item = (long)blockIdx.x * N;                                       // first row of the item
  const int q0 = wave * 16 * AW_QT;
  at_frag qh[AW_QT][4], ql[AW_QT][4];
#pragma unroll
  for (int qt = 0; qt < AW_QT; ++qt) {
    const long row = (item + min(q0 + 16 * qt + c, N - 1)) * AW_DQ + 8 * g;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      qh[qt][s] = *reinterpret_cast<const at_frag*>(Qh + row + 32 * s);
      ql[qt][s] = *reinterpret_cast<const at_frag*>(Ql + row + 32 * s);
    }
  }
  f32x4 o[AW_QT][5];
  float m[AW_QT], lsum[AW_QT];
#pragma unroll
  for (int qt = 0; qt < AW_QT; ++qt) {
    m[qt] = -INFINITY;
    lsum[qt] = 0.f;
#pragma unroll
    for (int j = 0; j < 5; ++j) o[qt][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  AwStage<AW_DQ, T> fkh, fkl;
  AwStage<AT_DV, T> fvh, fvl;
  auto fetch = [&](int kb) {
    fkh.fetch(Kh + item * AW_DQ, kb, N, tid);
    fkl.fetch(Kl + item * AW_DQ, kb, N, tid);
    fvh.fetch(Vh + item * AT_DV, kb, N, tid);
    fvl.fetch(Vl + item * AT_DV, kb, N, tid);
  };
  auto commit = [&](int buf) {
    f16_t* b = sbase + buf * kBuf;
    fkh.commit(b, AW_KS, tid);
    fkl.commit(b + AW_TR * AW_KS, AW_KS, tid);
    fvh.commit(b + 2 * AW_TR * AW_KS, AT_VS, tid);
    fvl.commit(b + 2 * AW_TR * AW_KS + AW_TR * AT_VS, AT_VS, tid);
  };
  fetch(0);
  commit(0);
  __syncthreads();
  for (int kb = 0, it = 0; kb < N; kb += AW_TR, ++it) {
    const bool more = kb + AW_TR < N;
    if (more) fetch(kb + AW_TR);
    const f16_t* sKh = sbase + (it & 1) * kBuf;
    const f16_t* sKl = sKh + AW_TR * AW_KS;
    const f16_t* sVh = sKl + AW_TR * AW_KS;
    const f16_t* sVl = sVh + AW_TR * AT_VS;
    f32x4 acc[AW_QT][2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
#pragma unroll
      for (int qt = 0; qt < AW_QT; ++qt) acc[qt][t] = f32x4{0.f, 0.f, 0.f, 0.f};
      const int off = (16 * t + c) * AW_KS + 8 * g;
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const at_frag kh = *reinterpret_cast<const at_frag*>(sKh + off + 32 * s), kl = *reinterpret_cast<const at_frag*>(sKl + off + 32 * s);
#pragma unroll
        for (int qt = 0; qt < AW_QT; ++qt) acc[qt][t] = at_mma3(kh, kl, qh[qt][s], ql[qt][s], acc[qt][t]);   // S^T: rows = keys 16 t + 4 g + i, column = query c
      }
    }
    at_frag ph[AW_QT], pl[AW_QT];
#pragma unroll
    for (int qt = 0; qt < AW_QT; ++qt) {
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int i = 0; i < 4; ++i)
          if (kb + 16 * t + 4 * g + i >= N) acc[qt][t][i] = -INFINITY;          // a key beyond the item: probability exactly 0 (key kb is always live)
      float mx = acc[qt][0][0];
#pragma unroll
      for (int t = 0; t < 2; ++t)
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
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          acc[qt][t][i] = __expf(acc[qt][t][i] - mn + kAtShift);                // 2^12 p
          lsum[qt] += acc[qt][t][i];
        }
      at_split8(acc[qt][0], acc[qt][1], ph[qt], pl[qt]);
    }
#pragma unroll
    for (int j = 0; j < 5; ++j) {
      const at_frag vh = at_rows8(sVh, AT_VS, 0, 16 * j, c, g), vl = at_rows8(sVl, AT_VS, 0, 16 * j, c, g);
#pragma unroll
      for (int qt = 0; qt < AW_QT; ++qt) o[qt][j] = at_mma3(vh, vl, ph[qt], pl[qt], o[qt][j]);               // O^T: rows = d 16 j + 4 g + i, column = query c
    }
    if (more) commit((it & 1) ^ 1);
    __syncthreads();
  }
#pragma unroll
  for (int qt = 0; qt < AW_QT; ++qt) {
    float ltot = lsum[qt];
    ltot += __shfl_xor(ltot, 16);
    ltot += __shfl_xor(ltot, 32);
    const float inv = 1.f / ltot;
    const int q = q0 + 16 * qt + c;
    if (q < N) {
      float* orow = O + (item + q) * AT_DV + 4 * g;
#pragma unroll
      for (int j = 0; j < 5; ++j)
        *reinterpret_cast<float4*>(orow + 16 * j) = make_float4(o[qt][j][0] * inv, o[qt][j][1] * inv, o[qt][j][2] * inv, o[qt][j][3] * inv);
      if (g == 0) LSE[item + q] = m[qt] + logf(ltot) - kAtShift;
    }
  }
}

// ---- backward 1: dK (the first 80 columns of dK') and dV; a wave owns 32 keys, the queries stream through LDS --------------------------------
template <int WAVES>
__global__ __launch_bounds__(64 * WAVES) void attn_win_bwd_kv_kernel(const f16_t* __restrict__ Qh, const f16_t* __restrict__ Ql,
                                                                     const f16_t* __restrict__ Kh, const f16_t* __restrict__ Kl,
                                                                     const f16_t* __restrict__ Vh, const f16_t* __restrict__ Vl,
                                                                     const f16_t* __restrict__ Dh, const f16_t* __restrict__ Dl,
                                                                     const float* __restrict__ LSE, const float* __restrict__ DELTA,
                                                                     float* __restrict__ dK, float* __restrict__ dV, int N) {
  extern __shared__ __attribute__((aligned(16))) char aw_smem[];
  constexpr int T = 64 * WAVES;
  constexpr int kBuf = 2 * AW_TR * AW_KS + 2 * AW_TR * AT_DS + 4 * AW_TR;       // halfs per buffer: q' pair, dO pair, lse + delta (floats)
  f16_t* sbase = reinterpret_cast<f16_t*>(aw_smem);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, c = lane & 15, g = lane >> 4;
  const long item = (long)blockIdx.x * N;
  const int k0 = wave * 16 * AW_QT;
  at_frag kh[AW_QT][4], kl[AW_QT][4], vh[AW_QT][3], vl[AW_QT][3];
#pragma unroll
  for (int kt = 0; kt < AW_QT; ++kt) {
    const long r = item + min(k0 + 16 * kt + c, N - 1);
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      kh[kt][s] = *reinterpret_cast<const at_frag*>(Kh + r * AW_DQ + 8 * g + 32 * s);
      kl[kt][s] = *reinterpret_cast<const at_frag*>(Kl + r * AW_DQ + 8 * g + 32 * s);
    }
#pragma unroll
    for (int s = 0; s < 3; ++s) {
      vh[kt][s] = *reinterpret_cast<const at_frag*>(Vh + r * AT_DVP + 8 * g + 32 * s);
      vl[kt][s] = *reinterpret_cast<const at_frag*>(Vl + r * AT_DVP + 8 * g + 32 * s);
    }
  }
  f32x4 dv[AW_QT][5], dk[AW_QT][5];
#pragma unroll
  for (int kt = 0; kt < AW_QT; ++kt)
#pragma unroll
    for (int j = 0; j < 5; ++j) dv[kt][j] = dk[kt][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  AwStage<AW_DQ, T> fqh, fql;
  AwStage<AT_DVP, T> fdh, fdl;
  float fstat = 0.f;
  const int si = min(tid, 2 * AW_TR - 1);                                      // branch-free: threads beyond 2 AW_TR repeat the last entry
  auto fetch = [&](int qb) {
    fqh.fetch(Qh + item * AW_DQ, qb, N, tid);
    fql.fetch(Ql + item * AW_DQ, qb, N, tid);
    fdh.fetch(Dh + item * AT_DVP, qb, N, tid);
    fdl.fetch(Dl + item * AT_DVP, qb, N, tid);
    fstat = (si < AW_TR ? LSE : DELTA)[item + min(qb + (si < AW_TR ? si : si - AW_TR), N - 1)];
  };
  auto commit = [&](int buf) {
    f16_t* b = sbase + buf * kBuf;
    fqh.commit(b, AW_KS, tid);
    fql.commit(b + AW_TR * AW_KS, AW_KS, tid);
    fdh.commit(b + 2 * AW_TR * AW_KS, AT_DS, tid);
    fdl.commit(b + 2 * AW_TR * AW_KS + AW_TR * AT_DS, AT_DS, tid);
    reinterpret_cast<float*>(b + 2 * AW_TR * AW_KS + 2 * AW_TR * AT_DS)[si] = fstat;
  };
  fetch(0);
  commit(0);
  __syncthreads();
  for (int qb = 0, it = 0; qb < N; qb += AW_TR, ++it) {
    const bool more = qb + AW_TR < N;
    if (more) fetch(qb + AW_TR);
    const f16_t* sQh = sbase + (it & 1) * kBuf;
    const f16_t* sQl = sQh + AW_TR * AW_KS;
    const f16_t* sDh = sQl + AW_TR * AW_KS;
    const f16_t* sDl = sDh + AW_TR * AT_DS;
    const float* sLse = reinterpret_cast<const float*>(sDl + AW_TR * AT_DS);
    const float* sDel = sLse + AW_TR;
    f32x4 p[AW_QT][2], ds[AW_QT][2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      f32x4 acc[AW_QT], dp[AW_QT];
#pragma unroll
      for (int kt = 0; kt < AW_QT; ++kt) acc[kt] = dp[kt] = f32x4{0.f, 0.f, 0.f, 0.f};
      const int off = (16 * t + c) * AW_KS + 8 * g;
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const at_frag ah = *reinterpret_cast<const at_frag*>(sQh + off + 32 * s), al = *reinterpret_cast<const at_frag*>(sQl + off + 32 * s);
#pragma unroll
        for (int kt = 0; kt < AW_QT; ++kt) acc[kt] = at_mma3(ah, al, kh[kt][s], kl[kt][s], acc[kt]);       // S: rows = queries 16 t + 4 g + i, column = key c
      }
      const int doff = (16 * t + c) * AT_DS + 8 * g;
#pragma unroll
      for (int s = 0; s < 3; ++s) {
        const at_frag ah = *reinterpret_cast<const at_frag*>(sDh + doff + 32 * s), al = *reinterpret_cast<const at_frag*>(sDl + doff + 32 * s);
#pragma unroll
        for (int kt = 0; kt < AW_QT; ++kt) dp[kt] = at_mma3(ah, al, vh[kt][s], vl[kt][s], dp[kt]);         // dP = dO v^T, same layout
      }
      const float4 l4 = *reinterpret_cast<const float4*>(sLse + 16 * t + 4 * g), d4 = *reinterpret_cast<const float4*>(sDel + 16 * t + 4 * g);
      const float lq[4] = {l4.x, l4.y, l4.z, l4.w}, dq_[4] = {d4.x, d4.y, d4.z, d4.w};
#pragma unroll
      for (int kt = 0; kt < AW_QT; ++kt)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const bool live = qb + 16 * t + 4 * g + i < N && k0 + 16 * kt + c < N;     // a padding query would be summed into dK / dV
          const float pv = live ? __expf(acc[kt][i] - lq[i]) : 0.f;
          p[kt][t][i] = pv * 4096.f;
          ds[kt][t][i] = pv * (dp[kt][i] - dq_[i]) * kAtDsScale;
        }
    }
    at_frag ph[AW_QT], pl[AW_QT], sh[AW_QT], sl[AW_QT];
#pragma unroll
    for (int kt = 0; kt < AW_QT; ++kt) {
      at_split8(p[kt][0], p[kt][1], ph[kt], pl[kt]);
      at_split8(ds[kt][0], ds[kt][1], sh[kt], sl[kt]);
    }
#pragma unroll
    for (int j = 0; j < 5; ++j) {
      const at_frag doh = at_rows8(sDh, AT_DS, 0, 16 * j, c, g), dol = at_rows8(sDl, AT_DS, 0, 16 * j, c, g);
      const at_frag qqh = at_rows8(sQh, AW_KS, 0, 16 * j, c, g), qql = at_rows8(sQl, AW_KS, 0, 16 * j, c, g);
#pragma unroll
      for (int kt = 0; kt < AW_QT; ++kt) {
        dv[kt][j] = at_mma3(ph[kt], pl[kt], doh, dol, dv[kt][j]);              // dV: rows = keys 4 g + i, column = d 16 j + c
        dk[kt][j] = at_mma3(sh[kt], sl[kt], qqh, qql, dk[kt][j]);              // dK: rows = keys, column = dim 16 j + c
      }
    }
    if (more) commit((it & 1) ^ 1);
    __syncthreads();
  }
#pragma unroll
  for (int kt = 0; kt < AW_QT; ++kt)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int key = k0 + 16 * kt + 4 * g + i;
      if (key < N) {
#pragma unroll
        for (int j = 0; j < 5; ++j) {
          const long at = (item + key) * AT_DV + 16 * j + c;
          dV[at] = dv[kt][j][i] * (1.f / 4096.f);
          dK[at] = dk[kt][j][i] * (1.f / kAtDsScale);
        }
      }
    }
}

// ---- backward 2: dQ' (all 128 columns); a wave owns 32 queries, the keys stream through LDS ---------------------------------------------------
template <int WAVES>
__global__ __launch_bounds__(64 * WAVES) void attn_win_bwd_q_kernel(const f16_t* __restrict__ Qh, const f16_t* __restrict__ Ql,
                                                                    const f16_t* __restrict__ Kh, const f16_t* __restrict__ Kl,
                                                                    const f16_t* __restrict__ Vh, const f16_t* __restrict__ Vl,
                                                                    const f16_t* __restrict__ Dh, const f16_t* __restrict__ Dl,
                                                                    const float* __restrict__ LSE, const float* __restrict__ DELTA,
                                                                    float* __restrict__ dQ, int N) {
  extern __shared__ __attribute__((aligned(16))) char aw_smem[];
  constexpr int T = 64 * WAVES;
  constexpr int kBuf = 2 * AW_TR * AW_KS + 2 * AW_TR * AT_DS;                   // halfs per buffer: k' pair, v pair
  f16_t* sbase = reinterpret_cast<f16_t*>(aw_smem);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, c = lane & 15, g = lane >> 4;
  const long item = (long)blockIdx.x * N;
  const int q0 = wave * 16 * AW_QT;
  at_frag qh[AW_QT][4], ql[AW_QT][4], dh[AW_QT][3], dl[AW_QT][3];
  float lse[AW_QT], delta[AW_QT];
#pragma unroll
  for (int qt = 0; qt < AW_QT; ++qt) {
    const long r = item + min(q0 + 16 * qt + c, N - 1);
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      qh[qt][s] = *reinterpret_cast<const at_frag*>(Qh + r * AW_DQ + 8 * g + 32 * s);
      ql[qt][s] = *reinterpret_cast<const at_frag*>(Ql + r * AW_DQ + 8 * g + 32 * s);
    }
#pragma unroll
    for (int s = 0; s < 3; ++s) {
      dh[qt][s] = *reinterpret_cast<const at_frag*>(Dh + r * AT_DVP + 8 * g + 32 * s);
      dl[qt][s] = *reinterpret_cast<const at_frag*>(Dl + r * AT_DVP + 8 * g + 32 * s);
    }
    lse[qt] = LSE[r];
    delta[qt] = DELTA[r];
  }
  f32x4 dq[AW_QT][8];
#pragma unroll
  for (int qt = 0; qt < AW_QT; ++qt)
#pragma unroll
    for (int j = 0; j < 8; ++j) dq[qt][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  AwStage<AW_DQ, T> fkh, fkl;
  AwStage<AT_DVP, T> fvh, fvl;
  auto fetch = [&](int kb) {
    fkh.fetch(Kh + item * AW_DQ, kb, N, tid);
    fkl.fetch(Kl + item * AW_DQ, kb, N, tid);
    fvh.fetch(Vh + item * AT_DVP, kb, N, tid);
    fvl.fetch(Vl + item * AT_DVP, kb, N, tid);
  };
  auto commit = [&](int buf) {
    f16_t* b = sbase + buf * kBuf;
    fkh.commit(b, AW_KS, tid);
    fkl.commit(b + AW_TR * AW_KS, AW_KS, tid);
    fvh.commit(b + 2 * AW_TR * AW_KS, AT_DS, tid);
    fvl.commit(b + 2 * AW_TR * AW_KS + AW_TR * AT_DS, AT_DS, tid);
  };
  fetch(0);
  commit(0);
  __syncthreads();
  for (int kb = 0, it = 0; kb < N; kb += AW_TR, ++it) {
    const bool more = kb + AW_TR < N;
    if (more) fetch(kb + AW_TR);
    const f16_t* sKh = sbase + (it & 1) * kBuf;
    const f16_t* sKl = sKh + AW_TR * AW_KS;
    const f16_t* sVh = sKl + AW_TR * AW_KS;
    const f16_t* sVl = sVh + AW_TR * AT_DS;
    f32x4 ds[AW_QT][2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      f32x4 acc[AW_QT], dp[AW_QT];
#pragma unroll
      for (int qt = 0; qt < AW_QT; ++qt) acc[qt] = dp[qt] = f32x4{0.f, 0.f, 0.f, 0.f};
      const int off = (16 * t + c) * AW_KS + 8 * g;
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const at_frag ah = *reinterpret_cast<const at_frag*>(sKh + off + 32 * s), al = *reinterpret_cast<const at_frag*>(sKl + off + 32 * s);
#pragma unroll
        for (int qt = 0; qt < AW_QT; ++qt) acc[qt] = at_mma3(ah, al, qh[qt][s], ql[qt][s], acc[qt]);       // S^T: rows = keys 16 t + 4 g + i, column = query c
      }
      const int voff = (16 * t + c) * AT_DS + 8 * g;
#pragma unroll
      for (int s = 0; s < 3; ++s) {
        const at_frag ah = *reinterpret_cast<const at_frag*>(sVh + voff + 32 * s), al = *reinterpret_cast<const at_frag*>(sVl + voff + 32 * s);
#pragma unroll
        for (int qt = 0; qt < AW_QT; ++qt) dp[qt] = at_mma3(ah, al, dh[qt][s], dl[qt][s], dp[qt]);         // dP^T = v dO^T, same layout
      }
#pragma unroll
      for (int qt = 0; qt < AW_QT; ++qt)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const bool live = kb + 16 * t + 4 * g + i < N;                        // a key beyond the item: probability exactly 0
          ds[qt][t][i] = live ? __expf(acc[qt][i] - lse[qt]) * (dp[qt][i] - delta[qt]) * kAtDsScale : 0.f;
        }
    }
    at_frag sh[AW_QT], sl[AW_QT];
#pragma unroll
    for (int qt = 0; qt < AW_QT; ++qt) at_split8(ds[qt][0], ds[qt][1], sh[qt], sl[qt]);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const at_frag kkh = at_rows8(sKh, AW_KS, 0, 16 * j, c, g), kkl = at_rows8(sKl, AW_KS, 0, 16 * j, c, g);
#pragma unroll
      for (int qt = 0; qt < AW_QT; ++qt) dq[qt][j] = at_mma3(kkh, kkl, sh[qt], sl[qt], dq[qt][j]);         // dQ'^T: rows = dims 16 j + 4 g + i, column = query c
    }
    if (more) commit((it & 1) ^ 1);
    __syncthreads();
  }
#pragma unroll
  for (int qt = 0; qt < AW_QT; ++qt) {
    const int q = q0 + 16 * qt + c;
    if (q < N) {
      float* out = dQ + (item + q) * AW_DQ + 4 * g;
#pragma unroll
      for (int j = 0; j < 8; ++j)
        *reinterpret_cast<float4*>(out + 16 * j) = make_float4(dq[qt][j][0] * (1.f / kAtDsScale), dq[qt][j][1] * (1.f / kAtDsScale),
                                                               dq[qt][j][2] * (1.f / kAtDsScale), dq[qt][j][3] * (1.f / kAtDsScale));
    }
  }
}

constexpr size_t kAwFwdLds = 2 * (size_t)(2 * AW_TR * AW_KS + 2 * AW_TR * AT_VS) * sizeof(f16_t);                                          // two buffers
constexpr size_t kAwBwdKvLds = 2 * ((size_t)(2 * AW_TR * AW_KS + 2 * AW_TR * AT_DS) * sizeof(f16_t) + 2 * AW_TR * sizeof(float));
constexpr size_t kAwBwdQLds = 2 * (size_t)(2 * AW_TR * AW_KS + 2 * AW_TR * AT_DS) * sizeof(f16_t);
static_assert(kAwFwdLds <= 64 * 1024 && kAwBwdKvLds <= 64 * 1024 && kAwBwdQLds <= 64 * 1024, "LDS budget: within the default dynamic limit");

// the shared entry check of the two windowed entries
static int aw_check(const char* who, bool pointers, int BH, int N) {
  HIPIE_REQUIRE(pointers, "%s: null pointer", who);
  HIPIE_REQUIRE(BH > 0 && N > 0 && N <= AW_MAX_N, "%s: BH=%d N=%d (BH >= 1, 1 <= N <= %d)", who, BH, N, AW_MAX_N);
  return 0;
}

template <int WAVES> static void aw_forward(hipStream_t st, int BH, int N, const f16_t* qh, const f16_t* ql, const f16_t* kh, const f16_t* kl,
                                            const f16_t* vh, const f16_t* vl, float* out, float* lse) {
  hipLaunchKernelGGL(attn_win_fwd_kernel<WAVES>, dim3((unsigned)BH), dim3(64 * WAVES), kAwFwdLds, st, qh, ql, kh, kl, vh, vl, out, lse, N);
}

template <int WAVES> static void aw_backward(hipStream_t st, int BH, int N, const f16_t* qh, const f16_t* ql, const f16_t* kh, const f16_t* kl,
                                             const f16_t* vh, const f16_t* vl, const f16_t* dh, const f16_t* dl, const float* lse,
                                             const float* delta, float* dq, float* dk, float* dv) {
  hipLaunchKernelGGL(attn_win_bwd_kv_kernel<WAVES>, dim3((unsigned)BH), dim3(64 * WAVES), kAwBwdKvLds, st, qh, ql, kh, kl, vh, vl, dh, dl, lse, delta,
                     dk, dv, N);
  hipLaunchKernelGGL(attn_win_bwd_q_kernel<WAVES>, dim3((unsigned)BH), dim3(64 * WAVES), kAwBwdQLds, st, qh, ql, kh, kl, vh, vl, dh, dl, lse, delta, dq,
                     N);
}

}  // namespace hipie

using namespace hipie;

extern "C" int hipie_attn_train_win_forward(const void* q_hi, const void* q_lo, const void* k_hi, const void* k_lo, const void* v_hi, const void* v_lo,
                                            void* out, void* lse, int BH, int N, void* stream) {
  HIPIE_TRY(aw_check("attn_train_win_forward", q_hi && q_lo && k_hi && k_lo && v_hi && v_lo && out && lse, BH, N));
  const auto run = N <= 128 ? aw_forward<4> : N <= 224 ? aw_forward<7> : aw_forward<8>;
  run((hipStream_t)stream, BH, N, (const f16_t*)q_hi, (const f16_t*)q_lo, (const f16_t*)k_hi, (const f16_t*)k_lo, (const f16_t*)v_hi,
      (const f16_t*)v_lo, (float*)out, (float*)lse);
  return check_launch("attn_train_win_forward");
}

extern "C" int hipie_attn_train_win_backward(const void* q_hi, const void* q_lo, const void* k_hi, const void* k_lo, const void* v_hi,
                                             const void* v_lo, const void* do_hi, const void* do_lo, const void* lse, const void* delta, void* dq,
                                             void* dk, void* dv, int BH, int N, void* stream) {
  HIPIE_TRY(aw_check("attn_train_win_backward", q_hi && q_lo && k_hi && k_lo && v_hi && v_lo && do_hi && do_lo && lse && delta && dq && dk && dv,
                     BH, N));
  const auto run = N <= 128 ? aw_backward<4> : N <= 224 ? aw_backward<7> : aw_backward<8>;
  run((hipStream_t)stream, BH, N, (const f16_t*)q_hi, (const f16_t*)q_lo, (const f16_t*)k_hi, (const f16_t*)k_lo, (const f16_t*)v_hi,
      (const f16_t*)v_lo, (const f16_t*)do_hi, (const f16_t*)do_lo, (const float*)lse, (const float*)delta, (float*)dq, (float*)dk, (float*)dv);
  return check_launch("attn_train_win_backward");
}
