// attn_f32_train.hip -- the decoders' query self-attention for the TRAINING step, forward and backward, in exact fp32: nn.MultiheadAttention
// with q = k = tgt + query_pos, v = tgt, 8 heads x 32 and the de-noising self-attention mask (deformable_transformer_dino.py:418-436,
// dino_decoder.py:222-248).  The arithmetic of attn_f32.hip (fp32 FMA chains in a fixed order, an online softmax in the log2 domain; the
// decoders amplify operand rounding by two to three orders of magnitude, see there) plus what training needs: the log-sum-exp of every row,
// a mask per (query, key) pair shared by the images and heads, and a backward that recomputes the probabilities from the log-sum-exp --
// nothing of N x N elements is written, forward or backward.
//
// Operands: qk (B, N, 2 H 32) rows of the q | k in-projection (q of head h at column h * 32, k at H * 32 + h * 32), v (B, N, H 32) rows,
// blocked (N, N) uint8, 1 = query i may NOT see key j (torch's attn_mask: the bool tensor's own storage), or null.
//
//   forward   s_ij = (scale log2 e) q_i . k_j,   lse_i = max_j s_ij + log2 sum_j 2^(s_ij - max)   [log2 units],   o_i = sum_j 2^(s_ij - lse_i) v_j
//   backward  p_ij = 2^(s_ij - lse_i)  (s recomputed with the forward's own chains),   delta_i = dO_i . O_i,   dp_ij = dO_i . v_j,
//             ds_ij = p_ij (dp_ij - delta_i),   dq_i = scale sum_j ds_ij k_j,   dk_j = scale sum_i ds_ij q_i,   dv_j = sum_i p_ij dO_i
//
// Three kernels of one shape: a workgroup owns 64 rows and QA_SPLIT waves; lane l of every wave holds row l's operands and accumulators in
// registers, the other side's rows are staged in LDS by the workgroup, QA_SPLIT * 32 at a time, and wave s reads the s-th 32 of them back as
// broadcasts.  The forward and the dQ pass own query rows and sweep the keys, the dK / dV pass owns key rows and sweeps the queries in query
// order.  One thread per (row, wave) runs attn_f32_kernel's loop over its share; the waves' partial results of a row are then folded in
// wave order through LDS (qa_fold_waves).  No reduction across lanes, no atomics: the same bits from call to call.
// Why the split: with one wave per row block (attn_f32_kernel's scheme as it stands) a call is 288 waves on 1024 SIMDs, each a serial chain
// over all N keys -- measured 3.5 x the time of the materialised formulation at N = 1110 (docs/measurements.md).
// A row with every key blocked has lse = -inf, an output of zeros, and contributes exactly zero to every gradient (p is SELECTED to 0
// there, never computed as 2^(s + inf)).
#include "common.h"

namespace hipie {

constexpr int QA_HD = 32;       // head width
constexpr int QA_T = 32;        // rows of the other side per LDS tile
constexpr int QA_SPLIT = 4;     // waves per 64 rows, each with a quarter of the other side (1 and 2 were measured too: docs/measurements.md)

struct QAParams {
  const float *qk, *v;
  const unsigned char* blocked;         // (N, N), 1 = blocked, images m_sb apart (0: shared); or null
  const float *out, *lse, *d_out;       // backward: the forward's results and the output gradient
  float *o, *l;                         // forward: out (B, N, H 32), lse (B, H, N)
  float *d_qk, *d_v, *delta;            // backward: (B, N, 2 H 32), (B, N, H 32), workspace (B, H, N)
  int B, H, N;
  long qk_sb, qk_st, v_sb, v_st, do_sb, do_st, m_sb;       // batch / row strides in elements
  float scale, scale_log2e;
};

// a . row with `a` in registers and `row` 32 floats in LDS: the two chains of attn_f32_kernel, in its order.  Every kernel below forms s_ij
// with this function on (scaled q, k) -- which of the two sits in registers does not change a product -- so the backward's s has the forward's bits.
__device__ __forceinline__ float qa_dot(const float (&a)[QA_HD], const float* row) {
  float a0 = 0.f, a1 = 0.f;
#pragma unroll
  for (int d = 0; d < QA_HD; d += 8) {
    const float4 r4 = *reinterpret_cast<const float4*>(row + d), r5 = *reinterpret_cast<const float4*>(row + d + 4);
    a0 = fmaf(a[d], r4.x, a0); a0 = fmaf(a[d + 1], r4.y, a0); a0 = fmaf(a[d + 2], r4.z, a0); a0 = fmaf(a[d + 3], r4.w, a0);
    a1 = fmaf(a[d + 4], r5.x, a1); a1 = fmaf(a[d + 5], r5.y, a1); a1 = fmaf(a[d + 6], r5.z, a1); a1 = fmaf(a[d + 7], r5.w, a1);
  }
  return a0 + a1;
}

// acc += c * row
__device__ __forceinline__ void qa_axpy(float (&acc)[QA_HD], float c, const float* row) {
#pragma unroll
  for (int d = 0; d < QA_HD; d += 4) {
    const float4 r = *reinterpret_cast<const float4*>(row + d);
    acc[d] = fmaf(c, r.x, acc[d]); acc[d + 1] = fmaf(c, r.y, acc[d + 1]); acc[d + 2] = fmaf(c, r.z, acc[d + 2]); acc[d + 3] = fmaf(c, r.w, acc[d + 3]);
  }
}

__device__ __forceinline__ void qa_load_row(const float* src, float mul, float (&dst)[QA_HD]) {
#pragma unroll
  for (int d = 0; d < QA_HD; d += 4) {
    const float4 t = *reinterpret_cast<const float4*>(src + d);
    dst[d] = t.x * mul; dst[d + 1] = t.y * mul; dst[d + 2] = t.z * mul; dst[d + 3] = t.w * mul;
  }
}

__device__ __forceinline__ void qa_store_row(float* dst, const float (&src)[QA_HD], float mul) {
#pragma unroll
  for (int d = 0; d < QA_HD; d += 4) *reinterpret_cast<float4*>(dst + d) = make_float4(src[d] * mul, src[d + 1] * mul, src[d + 2] * mul, src[d + 3] * mul);
}

// S * QA_T rows of 32 floats, rows r0 .. of `base` (row stride st; rows past N - 1 repeat the last row: finite, never counted), times mul,
// into LDS by the workgroup's 64 S threads: 16-byte pieces, coalesced along the head
template <int S>
__device__ __forceinline__ void qa_stage(float* dst, const float* base, long st, int r0, int N, float mul) {
  for (int i = threadIdx.x; i < S * QA_T * QA_HD / 4; i += 64 * S) {
    const int j = i / (QA_HD / 4), d = 4 * (i % (QA_HD / 4));
    const float4 t = *reinterpret_cast<const float4*>(base + (long)min(r0 + j, N - 1) * st + d);
    *reinterpret_cast<float4*>(dst + j * QA_HD + d) = make_float4(t.x * mul, t.y * mul, t.z * mul, t.w * mul);
  }
}

// The mask word of this lane's QUERY row for the keys k0 .. k0 + 31: bit j set = key k0 + j is blocked or past the last key.  A lane's own
// 32 bytes would be 64 scattered lines per load; instead the wave walks its 64 rows two at a time -- lanes 0-31 read the 32 bytes of one row,
// lanes 32-63 those of the next, a ballot turns them into the two words -- and every lane keeps the word of its row.  row0: the wave's first row.
__device__ __forceinline__ unsigned qa_row_mask(const unsigned char* m, int N, int row0, int k0) {
  if (m == nullptr) return N - k0 >= QA_T ? 0u : ~0u << (N - k0);
  const int lane = threadIdx.x & 63, col = k0 + (lane & 31);
  unsigned mine = 0;
  for (int it = 0; it < 32; ++it) {
    const int row = row0 + 2 * it + (lane >> 5);
    unsigned char byte = 1;
    if (row < N && col < N) byte = m[(long)row * N + col];
    const unsigned long long both = __ballot(byte != 0);
    const unsigned word = (lane & 1) ? (unsigned)(both >> 32) : (unsigned)both;
    if ((lane >> 1) == it) mine = word;
  }
  return mine;
}

// where a workgroup works: (image, head, first of its 64 rows); its waves share the rows and split the other side
struct QAItem {
  int b, h, r0;
  __device__ __forceinline__ QAItem(const QAParams& p) {
    const int tiles = (p.N + 63) / 64, bh = blockIdx.x / tiles;
    b = bh / p.H;
    h = bh % p.H;
    r0 = (blockIdx.x % tiles) * 64;
  }
};

// The waves of a workgroup hold partial results for the same 64 rows.  They are folded in WAVE ORDER through one LDS image, column-major
// (word d of lane l at d * 64 + l: conflict free): wave 0 writes, wave 1 reads, folds and writes, ... -- ((w0 + w1) + w2) + w3, the same
// order in every call.  The last wave ends with the result.  `fold(buf)` reads the image and folds it into the caller's registers,
// `put(buf)` writes them.  Every thread of the workgroup calls this (it holds barriers).
template <int S, typename Put, typename Fold>
__device__ __forceinline__ void qa_fold_waves(float* buf, Put&& put, Fold&& fold) {
  const int wave = threadIdx.x >> 6;
#pragma unroll
  for (int step = 1; step < S; ++step) {
    __syncthreads();                                   // the image (or, at first, the staging tile under it) has been consumed
    if (wave == step - 1) put(buf);
    __syncthreads();
    if (wave == step) fold(buf);
  }
}

// Forward: 64 query rows per workgroup, one thread per (row, wave); wave s of S takes the s-th 32 keys of every staged chunk of S * 32.
template <int S>
__global__ __launch_bounds__(64 * S) void qattn_train_fwd_kernel(const QAParams p) {
  __shared__ __attribute__((aligned(16))) float ks[S * QA_T * QA_HD];
  __shared__ __attribute__((aligned(16))) float vs[S * QA_T * QA_HD];
  const QAItem w(p);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, qi = w.r0 + lane;
  const bool live = qi < p.N;
  const float* qkb = p.qk + w.b * p.qk_sb;
  float q[QA_HD], o[QA_HD];
  qa_load_row(qkb + (long)min(qi, p.N - 1) * p.qk_st + w.h * QA_HD, p.scale_log2e, q);
#pragma unroll
  for (int d = 0; d < QA_HD; ++d) o[d] = 0.f;
  float m_run = -INFINITY, l_run = 0.f;
  const float* kb = qkb + (p.H + w.h) * QA_HD;
  const float* vb = p.v + w.b * p.v_sb + w.h * QA_HD;
  const unsigned char* mb = p.blocked ? p.blocked + w.b * p.m_sb : nullptr;
  for (int c0 = 0; c0 < p.N; c0 += S * QA_T) {
    __syncthreads();                                   // the previous chunk has been consumed
    qa_stage<S>(ks, kb, p.qk_st, c0, p.N, 1.f);
    qa_stage<S>(vs, vb, p.v_st, c0, p.N, 1.f);
    __syncthreads();
    const int k0 = c0 + wave * QA_T;
    if (k0 >= p.N) continue;                           // the same for the whole wave; the barriers are above
    const unsigned bits = qa_row_mask(mb, p.N, w.r0, k0);
    const float* kt = ks + wave * QA_T * QA_HD;
    const float* vt = vs + wave * QA_T * QA_HD;
    float s[QA_T];
    float mx = -INFINITY;
#pragma unroll
    for (int j = 0; j < QA_T; ++j) {
      s[j] = (bits >> j & 1u) ? -INFINITY : qa_dot(q, kt + j * QA_HD);
      mx = fmaxf(mx, s[j]);
    }
    if (mx > m_run) {                                  // per-lane branch: the rescale is rare after the first tiles
      const float alpha = __builtin_amdgcn_exp2f(m_run - mx);      // m_run = -inf -> 0
      m_run = mx;
      l_run *= alpha;
#pragma unroll
      for (int d = 0; d < QA_HD; ++d) o[d] *= alpha;
    }
    if (m_run != -INFINITY) {                          // else every key so far blocked: nothing to add (and no -inf - -inf)
#pragma unroll
      for (int j = 0; j < QA_T; ++j) {
        const float pj = __builtin_amdgcn_exp2f(s[j] - m_run);
        l_run += pj;
        qa_axpy(o, pj, vt + j * QA_HD);
      }
    }
  }
  // the waves' (max, sum, o) of a row, folded in wave order as two steps of the online softmax
  qa_fold_waves<S>(ks,
      [&](float* buf) {
        vs[lane] = m_run;                              // o in the K tile's place (32 x 64 words), max and sum in the V tile's
        vs[64 + lane] = l_run;
#pragma unroll
        for (int d = 0; d < QA_HD; ++d) buf[d * 64 + lane] = o[d];
      },
      [&](const float* buf) {
        const float m0 = vs[lane], l0 = vs[64 + lane];
        const float m = fmaxf(m0, m_run);
        const bool none = m == -INFINITY;              // both sides fully blocked so far: no -inf - -inf
        const float a0 = none ? 0.f : __builtin_amdgcn_exp2f(m0 - m), a1 = none ? 0.f : __builtin_amdgcn_exp2f(m_run - m);
        m_run = m;
        l_run = fmaf(l0, a0, l_run * a1);
#pragma unroll
        for (int d = 0; d < QA_HD; ++d) o[d] = fmaf(buf[d * 64 + lane], a0, o[d] * a1);
      });
  if (live && wave == S - 1) {
    const bool any = l_run > 0.f;
    qa_store_row(p.o + ((long)w.b * p.N + qi) * (p.H * QA_HD) + w.h * QA_HD, o, any ? 1.f / l_run : 0.f);
    p.l[((long)w.b * p.H + w.h) * p.N + qi] = any ? m_run + log2f(l_run) : -INFINITY;
  }
}

// dQ pass: the forward's split of the keys; also writes delta for the dK / dV pass
template <int S>
__global__ __launch_bounds__(64 * S) void qattn_train_dq_kernel(const QAParams p) {
  __shared__ __attribute__((aligned(16))) float ks[S * QA_T * QA_HD];
  __shared__ __attribute__((aligned(16))) float vs[S * QA_T * QA_HD];
  const QAItem w(p);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, qi = w.r0 + lane, qc = min(qi, p.N - 1);
  const bool live = qi < p.N;
  const float* qkb = p.qk + w.b * p.qk_sb;
  float q[QA_HD], g[QA_HD], dq[QA_HD];
  qa_load_row(qkb + (long)qc * p.qk_st + w.h * QA_HD, p.scale_log2e, q);
  qa_load_row(p.d_out + w.b * p.do_sb + (long)qc * p.do_st + w.h * QA_HD, 1.f, g);
  float delta;
  {
    const float* orow = p.out + ((long)w.b * p.N + qc) * (p.H * QA_HD) + w.h * QA_HD;
    float d0 = 0.f, d1 = 0.f;                          // two chains, fixed order
#pragma unroll
    for (int d = 0; d < QA_HD; d += 8) {
      const float4 o4 = *reinterpret_cast<const float4*>(orow + d), o5 = *reinterpret_cast<const float4*>(orow + d + 4);
      d0 = fmaf(g[d], o4.x, d0); d0 = fmaf(g[d + 1], o4.y, d0); d0 = fmaf(g[d + 2], o4.z, d0); d0 = fmaf(g[d + 3], o4.w, d0);
      d1 = fmaf(g[d + 4], o5.x, d1); d1 = fmaf(g[d + 5], o5.y, d1); d1 = fmaf(g[d + 6], o5.z, d1); d1 = fmaf(g[d + 7], o5.w, d1);
    }
    delta = d0 + d1;
  }
#pragma unroll
  for (int d = 0; d < QA_HD; ++d) dq[d] = 0.f;
  const float lse = p.lse[((long)w.b * p.H + w.h) * p.N + qc];
  const bool dead = lse == -INFINITY;                  // every key blocked: p = 0 for the whole row
  const float* kb = qkb + (p.H + w.h) * QA_HD;
  const float* vb = p.v + w.b * p.v_sb + w.h * QA_HD;
  const unsigned char* mb = p.blocked ? p.blocked + w.b * p.m_sb : nullptr;
  for (int c0 = 0; c0 < p.N; c0 += S * QA_T) {
    __syncthreads();
    qa_stage<S>(ks, kb, p.qk_st, c0, p.N, 1.f);
    qa_stage<S>(vs, vb, p.v_st, c0, p.N, 1.f);
    __syncthreads();
    const int k0 = c0 + wave * QA_T;
    if (k0 >= p.N) continue;                           // the same for the whole wave
    unsigned bits = qa_row_mask(mb, p.N, w.r0, k0);    // the ballots in it want every lane
    if (dead) bits = ~0u;
    const float* kt = ks + wave * QA_T * QA_HD;
    const float* vt = vs + wave * QA_T * QA_HD;
#pragma unroll 4
    for (int j = 0; j < QA_T; ++j) {
      const float s = qa_dot(q, kt + j * QA_HD);
      const float dp = qa_dot(g, vt + j * QA_HD);
      const float pj = (bits >> j & 1u) ? 0.f : __builtin_amdgcn_exp2f(s - lse);
      qa_axpy(dq, pj * (dp - delta), kt + j * QA_HD);
    }
  }
  qa_fold_waves<S>(ks,
      [&](float* buf) {
#pragma unroll
        for (int d = 0; d < QA_HD; ++d) buf[d * 64 + lane] = dq[d];
      },
      [&](const float* buf) {
#pragma unroll
        for (int d = 0; d < QA_HD; ++d) dq[d] = buf[d * 64 + lane] + dq[d];
      });
  if (live && wave == S - 1) {
    p.delta[((long)w.b * p.H + w.h) * p.N + qi] = delta;
    qa_store_row(p.d_qk + ((long)w.b * p.N + qi) * (2 * p.H * QA_HD) + w.h * QA_HD, dq, p.scale);
  }
}

// dK / dV pass: 64 key rows per workgroup; wave s takes the s-th 32 queries of every staged chunk of S * 32, in query order
template <int S, bool WANT_DK, bool WANT_DV>
__global__ __launch_bounds__(64 * S) void qattn_train_dkv_kernel(const QAParams p) {
  __shared__ __attribute__((aligned(16))) float qs[S * QA_T * QA_HD];     // scaled q
  __shared__ __attribute__((aligned(16))) float gs[S * QA_T * QA_HD];     // dO
  __shared__ float ls[S * QA_T], ds_[S * QA_T];                            // lse, delta
  const QAItem w(p);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, kj = w.r0 + lane, kc = min(kj, p.N - 1);
  const bool live = kj < p.N;
  const float* qkb = p.qk + w.b * p.qk_sb;
  float k[QA_HD], v[QA_HD], dk[QA_HD], dv[QA_HD];
  qa_load_row(qkb + (long)kc * p.qk_st + (p.H + w.h) * QA_HD, 1.f, k);
  qa_load_row(p.v + w.b * p.v_sb + (long)kc * p.v_st + w.h * QA_HD, 1.f, v);
#pragma unroll
  for (int d = 0; d < QA_HD; ++d) dk[d] = dv[d] = 0.f;
  const float* qb = qkb + w.h * QA_HD;
  const float* gb = p.d_out + w.b * p.do_sb + w.h * QA_HD;
  const long row_bh = ((long)w.b * p.H + w.h) * p.N;
  const unsigned char* mb = p.blocked ? p.blocked + w.b * p.m_sb : nullptr;
  for (int c0 = 0; c0 < p.N; c0 += S * QA_T) {
    __syncthreads();
    qa_stage<S>(qs, qb, p.qk_st, c0, p.N, p.scale_log2e);
    qa_stage<S>(gs, gb, p.do_st, c0, p.N, 1.f);
    if (threadIdx.x < S * QA_T) {                      // a query past the last one: lse = -inf, counted as a fully blocked row
      const int t = threadIdx.x;
      const bool in = c0 + t < p.N;
      ls[t] = in ? p.lse[row_bh + c0 + t] : -INFINITY;
      ds_[t] = (WANT_DK && in) ? p.delta[row_bh + c0 + t] : 0.f;
    }
    __syncthreads();
    const int i0 = c0 + wave * QA_T;
    if (i0 >= p.N) continue;                           // the same for the whole wave
    unsigned bits = 0;                                 // bit i: query i0 + i may not see this key (consecutive lanes: consecutive bytes)
    if (mb != nullptr && live) {
#pragma unroll 8
      for (int i = 0; i < QA_T; ++i)
        if (i0 + i < p.N && mb[(long)(i0 + i) * p.N + kj] != 0) bits |= 1u << i;
    }
    const float* qt = qs + wave * QA_T * QA_HD;
    const float* gt = gs + wave * QA_T * QA_HD;
#pragma unroll 4
    for (int i = 0; i < QA_T; ++i) {
      const float lse = ls[wave * QA_T + i];
      const float s = qa_dot(k, qt + i * QA_HD);
      const float pi = ((bits >> i & 1u) || lse == -INFINITY) ? 0.f : __builtin_amdgcn_exp2f(s - lse);
      if (WANT_DV) qa_axpy(dv, pi, gt + i * QA_HD);
      if (WANT_DK) {
        const float dp = qa_dot(v, gt + i * QA_HD);
        qa_axpy(dk, pi * (dp - ds_[wave * QA_T + i]), qt + i * QA_HD);
      }
    }
  }
  if (WANT_DK)
    qa_fold_waves<S>(qs,
        [&](float* buf) {
#pragma unroll
          for (int d = 0; d < QA_HD; ++d) buf[d * 64 + lane] = dk[d];
        },
        [&](const float* buf) {
#pragma unroll
          for (int d = 0; d < QA_HD; ++d) dk[d] = buf[d * 64 + lane] + dk[d];
        });
  if (WANT_DV)
    qa_fold_waves<S>(gs,
        [&](float* buf) {
#pragma unroll
          for (int d = 0; d < QA_HD; ++d) buf[d * 64 + lane] = dv[d];
        },
        [&](const float* buf) {
#pragma unroll
          for (int d = 0; d < QA_HD; ++d) dv[d] = buf[d * 64 + lane] + dv[d];
        });
  if (live && wave == S - 1) {
    // dk was summed over the staged q' = (scale log2 e) q:  scale q = q' ln 2
    if (WANT_DK) qa_store_row(p.d_qk + ((long)w.b * p.N + kj) * (2 * p.H * QA_HD) + (p.H + w.h) * QA_HD, dk, 0.6931471805599453f);
    if (WANT_DV) qa_store_row(p.d_v + ((long)w.b * p.N + kj) * (p.H * QA_HD) + w.h * QA_HD, dv, 1.f);
  }
}

static int qa_split() {
  const char* e = study_env("HIPIE_QATTN_SPLIT");      // study builds only: 1 | 2 waves per 64 rows
  const int s = e != nullptr ? atoi(e) : QA_SPLIT;
  return s == 1 || s == 2 ? s : QA_SPLIT;
}

static inline bool qa_al16(const void* a) { return ((uintptr_t)a & 15) == 0; }

}  // namespace hipie

#define QA_LAUNCH(kernel, what)                                                                             \
  do {                                                                                                      \
    const dim3 grid(B * H * ((N + 63) / 64));                                                               \
    if (split == 1) hipLaunchKernelGGL((kernel(1)), grid, dim3(64), 0, st, p);                              \
    else if (split == 2) hipLaunchKernelGGL((kernel(2)), grid, dim3(128), 0, st, p);                        \
    else hipLaunchKernelGGL((kernel(4)), grid, dim3(256), 0, st, p);                                        \
    HIPIE_TRY(check_launch(what));                                                                          \
  } while (0)
#define QA_FWD(S) qattn_train_fwd_kernel<S>
#define QA_DQ(S) qattn_train_dq_kernel<S>
#define QA_DKV(S) qattn_train_dkv_kernel<S, true, true>
#define QA_DK(S) qattn_train_dkv_kernel<S, true, false>
#define QA_DV(S) qattn_train_dkv_kernel<S, false, true>

// what the two entries refuse alike
static int qa_check(const char* who, const void* qk, const void* v, int B, int H, int N, int head_dim, int64_t qk_sb, int64_t qk_st, int64_t v_sb,
                    int64_t v_st, int64_t mask_sb) {
  using namespace hipie;
  HIPIE_REQUIRE(head_dim == QA_HD, "%s: head_dim 32 only (got %d)", who, head_dim);
  HIPIE_REQUIRE(B > 0 && H > 0 && N > 0 && (int64_t)B * H * ((N + 63) / 64) < (1ll << 31), "%s: bad shape B=%d H=%d N=%d", who, B, H, N);
  HIPIE_REQUIRE(qa_al16(qk) && qa_al16(v) && ((qk_sb | qk_st | v_sb | v_st) & 3) == 0,
                "%s: pointers must be 16-byte aligned and strides multiples of 4 elements", who);
  HIPIE_REQUIRE(qk_st >= 2 * H * QA_HD && v_st >= H * QA_HD && mask_sb >= 0, "%s: a row stride below the row's width, or a negative mask stride", who);
  return HIPIE_OK;
}

extern "C" int hipie_attn_f32_train_forward(const float* qk, const float* v, const unsigned char* blocked, float* out, float* lse, int B, int H,
                                            int N, int head_dim, int64_t qk_sb, int64_t qk_st, int64_t v_sb, int64_t v_st, int64_t mask_sb,
                                            float scale, void* stream) {
  using namespace hipie;
  HIPIE_REQUIRE(qk && v && out && lse, "attn_f32_train_forward: null pointer");
  HIPIE_TRY(qa_check("attn_f32_train_forward", qk, v, B, H, N, head_dim, qk_sb, qk_st, v_sb, v_st, mask_sb));
  HIPIE_REQUIRE(qa_al16(out), "attn_f32_train_forward: pointers must be 16-byte aligned and strides multiples of 4 elements");
  QAParams p = {};
  p.qk = qk; p.v = v; p.blocked = blocked; p.o = out; p.l = lse;
  p.B = B; p.H = H; p.N = N;
  p.qk_sb = qk_sb; p.qk_st = qk_st; p.v_sb = v_sb; p.v_st = v_st; p.m_sb = mask_sb;
  p.scale = scale; p.scale_log2e = scale * 1.4426950408889634f;
  hipStream_t st = (hipStream_t)stream;
  const int split = qa_split();
  QA_LAUNCH(QA_FWD, "attn_f32_train_forward");
  return HIPIE_OK;
}

extern "C" int64_t hipie_attn_f32_train_backward_ws_bytes(int B, int H, int N) {
  if (B <= 0 || H <= 0 || N <= 0) return 16;
  return (int64_t)B * H * N * (int64_t)sizeof(float);
}

extern "C" int hipie_attn_f32_train_backward(const float* qk, const float* v, const unsigned char* blocked, const float* out, const float* lse,
                                             const float* d_out, float* d_qk, float* d_v, void* ws, int64_t ws_bytes, int B, int H, int N,
                                             int head_dim, int64_t qk_sb, int64_t qk_st, int64_t v_sb, int64_t v_st, int64_t mask_sb,
                                             int64_t do_sb, int64_t do_st, float scale, void* stream) {
  using namespace hipie;
  HIPIE_REQUIRE(qk && v && out && lse && d_out && ws, "attn_f32_train_backward: null pointer");
  HIPIE_TRY(qa_check("attn_f32_train_backward", qk, v, B, H, N, head_dim, qk_sb, qk_st, v_sb, v_st, mask_sb));
  HIPIE_REQUIRE(qa_al16(out) && qa_al16(d_out) && qa_al16(d_qk) && qa_al16(d_v) && ((uintptr_t)ws & 3) == 0 && ((do_sb | do_st) & 3) == 0,
                "attn_f32_train_backward: pointers must be 16-byte aligned and strides multiples of 4 elements");
  HIPIE_REQUIRE(do_st >= H * QA_HD, "attn_f32_train_backward: a row stride below the row's width, or a negative mask stride");
  const int64_t need = hipie_attn_f32_train_backward_ws_bytes(B, H, N);
  HIPIE_REQUIRE(ws_bytes >= need, "attn_f32_train_backward: workspace of %lld bytes, need %lld", (long long)ws_bytes, (long long)need);
  if (d_qk == nullptr && d_v == nullptr) return HIPIE_OK;      // every input frozen: nothing is launched
  QAParams p = {};
  p.qk = qk; p.v = v; p.blocked = blocked; p.out = out; p.lse = lse; p.d_out = d_out;
  p.d_qk = d_qk; p.d_v = d_v; p.delta = (float*)ws;
  p.B = B; p.H = H; p.N = N;
  p.qk_sb = qk_sb; p.qk_st = qk_st; p.v_sb = v_sb; p.v_st = v_st; p.do_sb = do_sb; p.do_st = do_st; p.m_sb = mask_sb;
  p.scale = scale; p.scale_log2e = scale * 1.4426950408889634f;
  hipStream_t st = (hipStream_t)stream;
  const int split = qa_split();
  if (d_qk == nullptr) {                                       // frozen q | k rows: dV alone, no delta
    QA_LAUNCH(QA_DV, "attn_f32_train_backward (dV)");
    return HIPIE_OK;
  }
  QA_LAUNCH(QA_DQ, "attn_f32_train_backward (dQ)");
  if (d_v != nullptr) QA_LAUNCH(QA_DKV, "attn_f32_train_backward (dK, dV)");
  else QA_LAUNCH(QA_DK, "attn_f32_train_backward (dK)");
  return HIPIE_OK;
}
