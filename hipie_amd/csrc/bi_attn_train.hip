// bi_attn_train.hip -- the core of the vision-language fusion attention for the TRAINING step, forward and backward, in exact fp32: what lies
// between the four input projections and the two output projections of BiMultiHeadAttention.forward (fuse_helper.py:54-139), both
// directions, with the block's attention dropout.  Nothing of Nv x L elements is written to HBM, forward or backward.
//
// Per (image b, head h), q_i / vv_i rows of visual token i, k_j / vl_j rows of text token j, all 256 wide, att[b, j] the text mask:
//   raw_ij = scale q_i . k_j,  s_ij = clamp(raw_ij, -50000, 50000)
//   pv_ij = softmax over the ATTENDED j of s_ij (0 where att = 0),   pl_ij = softmax over ALL i of s_ij per column j (no mask)
//   out_v_i = sum_j pv_ij kv_ij vl_j,   out_l_j = sum_i pl_ij kl_ij vv_i       (kv, kl: the dropout keep factors, 0 or 1 / (1 - r))
//   backward, with dv_i = dOv_i . out_v_i and dl_j = dOl_j . out_l_j:
//   ds_ij = (pv_ij (kv_ij dOv_i . vl_j - dv_i) + pl_ij (kl_ij vv_i . dOl_j - dl_j)) [|raw_ij| <= 50000]
//   dq_i = scale sum_j ds_ij k_j,  dk_j = scale sum_i ds_ij q_i,  dvl_j = sum_i pv_ij kv_ij dOv_i,  dvv_i = sum_j pl_ij kl_ij dOl_j
// The reference's +1 on the attended logits cancels in the softmax; its second clamp (on wT - max) only touches entries whose
// probability is 0 in fp32 already.  An image with NO attended token is outside the contract: out_v = 0, lse_v = -inf, and that direction
// contributes exactly zero gradient (the probabilities are SELECTED to 0); the reference gives a uniform row there.
//
// Every product runs on v_mfma_f32_32x32x2_f32: exact fp32, bitwise an fmaf chain over the head dimension in its natural order
// (mfma.h has the lane layout).  Two kernel shapes, 4 waves each, built from the same pieces:
//   V  a workgroup owns 32 visual rows and the whole text (L <= 256 = 8 tiles of 32, wave w takes tiles w and w + 4): the image -> text
//      softmax rows, out_v, d_q, d_vv.  The logit tile has the text index down the registers and the visual index on the lanes.
//   T  a workgroup owns 32 text rows and one SEGMENT of the visual rows, swept 128 at a time in order (wave w takes 32 of them): the
//      column statistics, out_l, d_k, d_vl.  The tile has the visual index down the registers and the text index on the lanes.
//      The segments' partial results (at most 8 per text row) go to the workspace and are folded in segment order by a small kernel.
// Both form a tile with ba_product: the two operand panels are staged through LDS 32 columns of the head at a time, and the chain over the
// 256 columns is the same in every kernel -- so s_ij has the same bits wherever it is recomputed (a product a * b does not change with
// the side an operand sits on).  The second product of a pass (probabilities times rows) sums over the index that lies down the
// registers: the waves put their tiles into one LDS image and each wave then owns two 32-column blocks of the output and runs the whole
// sum in index order.  No atomics, no order that depends on timing: the same bits from call to call.
//
// Statistics in log2 units, as a PAIR per row: the maximum mx and ls = log2 sum 2^(s - mx).  p = 2^((s - mx) - ls) in the forward and in
// the backward.  lse = mx + ls is written as well, but is not what the backward reads: a clamped row has logits of 50000 log2 e = 72135,
// where one float has an ulp of 0.008 -- a 0.5 % error in every probability of the row.
//
// Dropout: keep(seed, direction, b, h, i, j) = [mix(mix(i ^ seed_lo) ^ seed_hi ^ (j | direction << 8 | h << 9 | b << 19)) >= thr] with
// mix the 32-bit finaliser below and thr = round(r 2^32): a function of the indices only, the same in every kernel.
#include "common.h"
#include "mfma.h"

namespace hipie {

constexpr int BA_HD = 256;      // head width
constexpr int BA_DC = 32;       // columns of the head per staged panel
constexpr int BA_PS = 33;       // panel row stride in floats (odd: the 32 rows of a tile fall into 32 banks)
constexpr int BA_LMAX = 256;    // text rows: 8 tiles, two per wave of a V workgroup
constexpr int BA_VB = 128;      // visual rows per sweep step of a T workgroup
constexpr int BA_MAXSEG = 8;    // segments of the visual rows per text tile
constexpr float BA_LOG2E = 1.4426950408889634f;

struct BAParams {
  const float *q, *k, *vv, *vl;
  const unsigned char* att;                              // (B, L), 1 = attended
  const float *st_v, *st_l;                              // (B, H, Nv, 2) / (B, H, L, 2): (mx, ls) per row; the forward writes them through sv / sl
  const float *out_v, *out_l, *d_ov, *d_ol;              // backward: the forward's outputs and the output gradients
  float *o_v, *o_l, *l_v, *l_l, *sv, *sl;                // forward outputs
  float *d_q, *d_k, *d_vv, *d_vl;                        // backward outputs, contiguous; null = not wanted
  float *stat, *part0, *part1, *delta_v, *delta_l;       // workspace
  int B, H, Nv, L, nseg, seglen;
  long q_sb, q_st, k_sb, k_st, vv_sb, vv_st, vl_sb, vl_st, dov_sb, dov_st, dol_sb, dol_st;     // batch / row strides in elements
  float scale, keep_inv;
  unsigned thr, seed_lo, seed_hi;
};

__device__ __forceinline__ unsigned ba_mix(unsigned x) {
  x ^= x >> 16; x *= 0x85ebca6bu; x ^= x >> 13; x *= 0xc2b2ae35u; x ^= x >> 16;
  return x;
}

// the dropout keep factor of element (i, j) of direction dir (0: image -> text, 1: text -> image): 0 or 1 / (1 - r); 1 at r = 0
__device__ __forceinline__ float ba_keep(const BAParams& p, unsigned dir, int b, int h, int i, int j) {
  if (p.thr == 0u) return 1.f;
  unsigned x = ba_mix((unsigned)i ^ p.seed_lo);
  x = ba_mix(x ^ p.seed_hi ^ ((unsigned)j | dir << 8 | (unsigned)h << 9 | (unsigned)b << 19));
  return x >= p.thr ? p.keep_inv : 0.f;
}

// THE logit of every kernel, from the accumulated scale q . k: clamped, in log2 units.  contract(off): a product the compiler may not fuse
// with the subtraction of the maximum that follows -- fma(s, log2 e, -mx) keeps the product's rounding error, 1e-3 at a clamped logit,
// which one kernel would then see and another not (measured: out_l off by 7.5e-4 on a clamped row)
__device__ __forceinline__ float ba_logit(float raw) {
#pragma clang fp contract(off)
  return fminf(fmaxf(raw, -50000.f), 50000.f) * BA_LOG2E;
}
__device__ __forceinline__ float ba_inrange(float raw) { return (raw >= -50000.f && raw <= 50000.f) ? 1.f : 0.f; }
// 2^((s - mx) - ls), selected to 0 where the row has no entry
__device__ __forceinline__ float ba_prob(float s, float mx, float ls) { return mx == -INFINITY ? 0.f : __builtin_amdgcn_exp2f((s - mx) - ls); }

// `rows` rows r0 .. of `base` (row stride st; rows past N - 1 repeat the last row: finite, never counted), columns d0 .. d0 + 31, times
// mul, into a panel by the workgroup's 256 threads: 16-byte loads, coalesced along the head
__device__ __forceinline__ void ba_stage(float* pan, const float* base, long st, int r0, int N, int rows, int d0, float mul) {
  for (int x = threadIdx.x; x < rows * (BA_DC / 4); x += 256) {
    const int r = x / (BA_DC / 4), c = 4 * (x % (BA_DC / 4));
    const float4 t = *reinterpret_cast<const float4*>(base + (long)min(r0 + r, N - 1) * st + d0 + c);
    float* d = pan + r * BA_PS + c;
    d[0] = t.x * mul; d[1] = t.y * mul; d[2] = t.z * mul; d[3] = t.w * mul;
  }
}

// acc[x] += (tile wave + 4 x of the R rows) . (the 32 C rows)^T over the 256 columns: R rows down the registers (row crow(r, hi) of the
// tile in register r), C rows on the lanes.  R: nRt tiles of 32 rows from row Rr0 of Rg, C: 32 rows from row Cr0 of Cg.  `pan`: 32 + 32 nRt
// panel rows.  Every thread of the workgroup calls this (it holds barriers); it begins with one, so what the caller read from `pan`
// before is safe.
template <int X>
__device__ __forceinline__ void ba_product(f32x16 (&acc)[X], float* pan, const float* Rg, long Rst, int Rr0, int RN, int nRt, float Rmul,
                                           const float* Cg, long Cst, int Cr0, int CN, float Cmul) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, li = lane & 31, hi = lane >> 5;
  float* panC = pan;
  float* panR = pan + 32 * BA_PS;
  for (int d0 = 0; d0 < BA_HD; d0 += BA_DC) {
    __syncthreads();
    ba_stage(panC, Cg, Cst, Cr0, CN, 32, d0, Cmul);
    ba_stage(panR, Rg, Rst, Rr0, RN, nRt * 32, d0, Rmul);
    __syncthreads();
#pragma unroll
    for (int x = 0; x < X; ++x) {
      const int t = wave + 4 * x;
      if (t < nRt) {
        const float* rp = panR + (t * 32 + li) * BA_PS + hi;
        const float* cp = panC + li * BA_PS + hi;
#pragma unroll
        for (int kk = 0; kk < BA_DC / 2; ++kk) acc[x] = __builtin_amdgcn_mfma_f32_32x32x2f32(rp[2 * kk], cp[2 * kk], acc[x], 0, 0, 0);
      }
    }
  }
}

template <int X>
__device__ __forceinline__ void ba_zero(f32x16 (&acc)[X]) {
#pragma unroll
  for (int x = 0; x < X; ++x)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[x][r] = 0.f;
}

// out^T block (32 columns c0 .. of the output, down the registers) x (the 32 lanes' index) = sum over n rows of  rows[n][c0 ..] * img[n][lane]:
// img an LDS image of n x 32 (n even, or the row after the last one zero), rows from global memory with row stride st, N of them valid
__device__ __forceinline__ f32x16 ba_apply(f32x16 o, const float* img, int n, const float* rows, long st, int r0, int N, int c0) {
  const int lane = threadIdx.x & 63, li = lane & 31, hi = lane >> 5;
  for (int x = 0; x < n; x += 2)
    o = __builtin_amdgcn_mfma_f32_32x32x2f32(rows[(long)min(r0 + x + hi, N - 1) * st + c0 + li], img[(x + hi) * 32 + li], o, 0, 0, 0);
  return o;
}

// registers of an output block -> 4 x 16 bytes of a row: columns c0 + 8 g + 4 hi .. + 3
__device__ __forceinline__ void ba_store(float* row, const f32x16& o, int c0, float mul) {
  const int hi = (threadIdx.x & 63) >> 5;
#pragma unroll
  for (int g = 0; g < 4; ++g)
    *reinterpret_cast<float4*>(row + c0 + 8 * g + 4 * hi) = make_float4(o[4 * g] * mul, o[4 * g + 1] * mul, o[4 * g + 2] * mul, o[4 * g + 3] * mul);
}

// ------------------------------------------------------------------------------------------------ V: 32 visual rows, the whole text
struct BAItemV {
  int b, h, bh, i0;
  __device__ __forceinline__ BAItemV(const BAParams& p) {
    const int nib = (p.Nv + 31) / 32;
    bh = blockIdx.x / nib;
    b = bh / p.H;
    h = bh % p.H;
    i0 = (blockIdx.x % nib) * 32;
  }
};

// forward: the image -> text softmax rows and out_v
__global__ __launch_bounds__(256) void ba_fwd_v_kernel(const BAParams p) {
  __shared__ __attribute__((aligned(16))) float lds[(32 + BA_LMAX) * BA_PS];     // the panels, then the probability image (L x 32)
  __shared__ float red[4 * 32];
  __shared__ unsigned char satt[BA_LMAX];
  const BAItemV w(p);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 31, hi = lane >> 5;
  const int nT = (p.L + 31) / 32, i = w.i0 + li;
  satt[tid] = tid < p.L ? p.att[(long)w.b * p.L + tid] : 0;
  f32x16 acc[2];
  ba_zero(acc);
  ba_product<2>(acc, lds, p.k + w.b * p.k_sb + w.h * BA_HD, p.k_st, 0, p.L, nT, 1.f, p.q + w.b * p.q_sb + w.h * BA_HD, p.q_st, w.i0, p.Nv, p.scale);
  float m = -INFINITY;
#pragma unroll
  for (int x = 0; x < 2; ++x)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int t = wave + 4 * x, j = t * 32 + crow(r, hi);
      const bool ok = t < nT && j < p.L && satt[min(j, BA_LMAX - 1)] != 0;
      acc[x][r] = ok ? ba_logit(acc[x][r]) : -INFINITY;
      m = fmaxf(m, acc[x][r]);
    }
  m = fmaxf(m, __shfl_xor(m, 32));
  if (hi == 0) red[wave * 32 + li] = m;
  __syncthreads();
  const float mx = fmaxf(fmaxf(red[li], red[32 + li]), fmaxf(red[64 + li], red[96 + li]));
  __syncthreads();
  float l = 0.f;
#pragma unroll
  for (int x = 0; x < 2; ++x)
#pragma unroll
    for (int r = 0; r < 16; ++r)
      if (acc[x][r] != -INFINITY) l += __builtin_amdgcn_exp2f(acc[x][r] - mx);
  l = __shfl(l, li) + __shfl(l, li + 32);
  if (hi == 0) red[wave * 32 + li] = l;
  __syncthreads();
  const float sum = ((red[li] + red[32 + li]) + red[64 + li]) + red[96 + li];      // wave order
  const float ls = mx == -INFINITY ? 0.f : log2f(sum);
  if (wave == 0 && hi == 0 && i < p.Nv) {
    const long at = (long)w.bh * p.Nv + i;
    p.sv[2 * at] = mx;
    p.sv[2 * at + 1] = ls;
    p.l_v[at] = mx == -INFINITY ? -INFINITY : mx + ls;
  }
  // the panels have been consumed (the barriers above): the probability image takes their place
#pragma unroll
  for (int x = 0; x < 2; ++x) {
    const int t = wave + 4 * x;
    if (t < nT) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int j = t * 32 + crow(r, hi);
        const float pv = acc[x][r] == -INFINITY ? 0.f : ba_prob(acc[x][r], mx, ls);
        lds[j * 32 + li] = pv * ba_keep(p, 0u, w.b, w.h, i, j);
      }
    }
  }
  __syncthreads();
#pragma unroll
  for (int y = 0; y < 2; ++y) {                        // every lane takes part in the product (a lane's operand is an output COLUMN)
    f32x16 o[1];
    ba_zero(o);
    o[0] = ba_apply(o[0], lds, (p.L + 1) & ~1, p.vl + w.b * p.vl_sb + w.h * BA_HD, p.vl_st, 0, p.L, (wave + 4 * y) * 32);
    if (i < p.Nv) ba_store(p.o_v + ((long)w.b * p.Nv + i) * ((long)p.H * BA_HD) + w.h * BA_HD, o[0], (wave + 4 * y) * 32, 1.f);
  }
}

// backward: d_q and d_vv
__global__ __launch_bounds__(256) void ba_bwd_v_kernel(const BAParams p) {
  __shared__ __attribute__((aligned(16))) float lds[(32 + BA_LMAX) * BA_PS];     // the panels, then one L x 32 image at a time
  __shared__ float smx[BA_LMAX], sls[BA_LMAX], sdl[BA_LMAX];
  __shared__ unsigned char satt[BA_LMAX];
  const BAItemV w(p);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 31, hi = lane >> 5;
  const int nT = (p.L + 31) / 32, i = w.i0 + li, ic = min(i, p.Nv - 1);
  const bool want_q = p.d_q != nullptr, want_vv = p.d_vv != nullptr;
  {
    const int jc = min(tid, p.L - 1);
    satt[tid] = tid < p.L ? p.att[(long)w.b * p.L + tid] : 0;
    smx[tid] = p.st_l[2 * ((long)w.bh * p.L + jc)];
    sls[tid] = p.st_l[2 * ((long)w.bh * p.L + jc) + 1];
    sdl[tid] = want_q ? p.delta_l[(long)w.bh * p.L + jc] : 0.f;
  }
  const float mv = p.st_v[2 * ((long)w.bh * p.Nv + ic)], lsv = p.st_v[2 * ((long)w.bh * p.Nv + ic) + 1];
  const float dv = want_q ? p.delta_v[(long)w.bh * p.Nv + ic] : 0.f;
  const float* kb = p.k + w.b * p.k_sb + w.h * BA_HD;
  const float* dolb = p.d_ol + w.b * p.dol_sb + w.h * BA_HD;
  f32x16 s[2], gv[2], gl[2];
  ba_zero(s); ba_zero(gv); ba_zero(gl);
  ba_product<2>(s, lds, kb, p.k_st, 0, p.L, nT, 1.f, p.q + w.b * p.q_sb + w.h * BA_HD, p.q_st, w.i0, p.Nv, p.scale);
  if (want_q) {
    ba_product<2>(gv, lds, p.vl + w.b * p.vl_sb + w.h * BA_HD, p.vl_st, 0, p.L, nT, 1.f, p.d_ov + w.b * p.dov_sb + w.h * BA_HD, p.dov_st, w.i0, p.Nv, 1.f);
    ba_product<2>(gl, lds, dolb, p.dol_st, 0, p.L, nT, 1.f, p.vv + w.b * p.vv_sb + w.h * BA_HD, p.vv_st, w.i0, p.Nv, 1.f);
  }
  // s -> pl kl, gv -> ds
#pragma unroll
  for (int x = 0; x < 2; ++x)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int t = wave + 4 * x, j = t * 32 + crow(r, hi), jc = min(j, BA_LMAX - 1);
      const bool okj = t < nT && j < p.L;
      const float raw = s[x][r], s2 = ba_logit(raw);
      const float pl = okj ? ba_prob(s2, smx[jc], sls[jc]) : 0.f;
      const float kl = ba_keep(p, 1u, w.b, w.h, i, j);
      if (want_q) {
        const float pv = (okj && satt[jc] != 0) ? ba_prob(s2, mv, lsv) : 0.f;
        const float kv = ba_keep(p, 0u, w.b, w.h, i, j);
        gv[x][r] = (pv * (kv * gv[x][r] - dv) + pl * (kl * gl[x][r] - sdl[jc])) * ba_inrange(raw);
      }
      s[x][r] = pl * kl;
    }
  const int n = (p.L + 1) & ~1;
  if (want_q) {
    __syncthreads();                                   // the panels have been consumed
#pragma unroll
    for (int x = 0; x < 2; ++x)
      if (wave + 4 * x < nT)
#pragma unroll
        for (int r = 0; r < 16; ++r) lds[((wave + 4 * x) * 32 + crow(r, hi)) * 32 + li] = gv[x][r];
    __syncthreads();
#pragma unroll
    for (int y = 0; y < 2; ++y) {
      f32x16 o[1];
      ba_zero(o);
      o[0] = ba_apply(o[0], lds, n, kb, p.k_st, 0, p.L, (wave + 4 * y) * 32);
      if (i < p.Nv) ba_store(p.d_q + ((long)w.b * p.Nv + i) * ((long)p.H * BA_HD) + w.h * BA_HD, o[0], (wave + 4 * y) * 32, p.scale);
    }
  }
  if (want_vv) {
    __syncthreads();                                   // the panels, or the ds image, have been consumed
#pragma unroll
    for (int x = 0; x < 2; ++x)
      if (wave + 4 * x < nT)
#pragma unroll
        for (int r = 0; r < 16; ++r) lds[((wave + 4 * x) * 32 + crow(r, hi)) * 32 + li] = s[x][r];
    __syncthreads();
#pragma unroll
    for (int y = 0; y < 2; ++y) {
      f32x16 o[1];
      ba_zero(o);
      o[0] = ba_apply(o[0], lds, n, dolb, p.dol_st, 0, p.L, (wave + 4 * y) * 32);
      if (i < p.Nv) ba_store(p.d_vv + ((long)w.b * p.Nv + i) * ((long)p.H * BA_HD) + w.h * BA_HD, o[0], (wave + 4 * y) * 32, 1.f);
    }
  }
}

// ------------------------------------------------------------------------------------------------ T: 32 text rows, one segment of the visual rows
// MODE 0: the column statistics (max, sum) of the segment -> stat;  1: out_l partials -> part0;  2: d_k partials -> part0, d_vl -> part1
template <int MODE>
__global__ __launch_bounds__(256) void ba_t_kernel(const BAParams p) {
  __shared__ __attribute__((aligned(16))) float pan[(32 + BA_VB) * BA_PS];
  __shared__ float img0[MODE >= 1 ? BA_VB * 32 : 1], img1[MODE == 2 ? BA_VB * 32 : 1];
  __shared__ float srow[MODE == 2 ? 3 * BA_VB : 1];                            // (mx, ls, delta) of the step's visual rows
  __shared__ float red[2 * 4 * 32];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 31, hi = lane >> 5;
  const int nT = (p.L + 31) / 32;
  const int seg = blockIdx.x % p.nseg, jt = (blockIdx.x / p.nseg) % nT, bh = blockIdx.x / (p.nseg * nT), b = bh / p.H, h = bh % p.H;
  const int j0 = jt * 32, j = j0 + li, jc = min(j, p.L - 1);
  const bool okj = j < p.L;
  const int ibeg = seg * p.seglen, iend = min(p.Nv, ibeg + p.seglen);
  const bool want_k = MODE == 2 && p.d_k != nullptr, want_vl = MODE == 2 && p.d_vl != nullptr;
  float ml = 0.f, lsl = 0.f, dl = 0.f;
  bool attj = false;
  if (MODE >= 1) {
    ml = p.st_l[2 * ((long)bh * p.L + jc)];
    lsl = p.st_l[2 * ((long)bh * p.L + jc) + 1];
  }
  if (MODE == 2) {
    dl = want_k ? p.delta_l[(long)bh * p.L + jc] : 0.f;
    attj = p.att[(long)b * p.L + jc] != 0;
  }
  const float* qb = p.q + b * p.q_sb + h * BA_HD;
  const float* kb = p.k + b * p.k_sb + h * BA_HD;
  const float* vvb = p.vv + b * p.vv_sb + h * BA_HD;
  const float* dovb = MODE == 2 ? p.d_ov + b * p.dov_sb + h * BA_HD : nullptr;
  float m_run = -INFINITY, l_run = 0.f;
  f32x16 o0[2], o1[2];
  ba_zero(o0); ba_zero(o1);
  for (int i0 = ibeg; i0 < iend; i0 += BA_VB) {
    const int nRt = min(4, (iend - i0 + 31) / 32);
    if (MODE == 2 && tid < BA_VB) {                    // last step's readers are behind its barriers
      const long at = (long)bh * p.Nv + min(i0 + tid, p.Nv - 1);
      srow[tid] = p.st_v[2 * at];
      srow[BA_VB + tid] = p.st_v[2 * at + 1];
      srow[2 * BA_VB + tid] = want_k ? p.delta_v[at] : 0.f;
    }
    f32x16 s[1], gv[1], gl[1];
    ba_zero(s); ba_zero(gv); ba_zero(gl);
    ba_product<1>(s, pan, qb, p.q_st, i0, p.Nv, nRt, p.scale, kb, p.k_st, j0, p.L, 1.f);
    if (want_k) {
      ba_product<1>(gv, pan, dovb, p.dov_st, i0, p.Nv, nRt, 1.f, p.vl + b * p.vl_sb + h * BA_HD, p.vl_st, j0, p.L, 1.f);
      ba_product<1>(gl, pan, vvb, p.vv_st, i0, p.Nv, nRt, 1.f, p.d_ol + b * p.dol_sb + h * BA_HD, p.dol_st, j0, p.L, 1.f);
    }
    if (MODE == 0) {
      if (wave < nRt) {
        float tm = -INFINITY;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const bool oki = i0 + wave * 32 + crow(r, hi) < iend;
          s[0][r] = oki ? ba_logit(s[0][r]) : -INFINITY;
          tm = fmaxf(tm, s[0][r]);
        }
        if (tm > m_run) {
          l_run *= __builtin_amdgcn_exp2f(m_run - tm);                         // m_run = -inf -> 0
          m_run = tm;
        }
        if (m_run != -INFINITY) {
#pragma unroll
          for (int r = 0; r < 16; ++r) l_run += __builtin_amdgcn_exp2f(s[0][r] - m_run);
        }
      }
    } else {
      if (wave < nRt) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int il = wave * 32 + crow(r, hi), i = i0 + il;
          const bool ok = okj && i < iend;
          const float raw = s[0][r], s2 = ba_logit(raw);
          const float pl = ok ? ba_prob(s2, ml, lsl) : 0.f;
          const float kl = ba_keep(p, 1u, b, h, i, j);
          if (MODE == 1) {
            img0[il * 32 + li] = pl * kl;
          } else {
            const float pv = (ok && attj) ? ba_prob(s2, srow[il], srow[BA_VB + il]) : 0.f;
            const float kv = ba_keep(p, 0u, b, h, i, j);
            if (want_k) img0[il * 32 + li] = (pv * (kv * gv[0][r] - srow[2 * BA_VB + il]) + pl * (kl * gl[0][r] - dl)) * ba_inrange(raw);
            if (want_vl) img1[il * 32 + li] = pv * kv;
          }
        }
      }
      __syncthreads();
#pragma unroll
      for (int y = 0; y < 2; ++y) {
        if (MODE == 1) o0[y] = ba_apply(o0[y], img0, nRt * 32, vvb, p.vv_st, i0, p.Nv, (wave + 4 * y) * 32);
        if (want_k) o0[y] = ba_apply(o0[y], img0, nRt * 32, qb, p.q_st, i0, p.Nv, (wave + 4 * y) * 32);
        if (want_vl) o1[y] = ba_apply(o1[y], img1, nRt * 32, dovb, p.dov_st, i0, p.Nv, (wave + 4 * y) * 32);
      }
    }
  }
  if (MODE == 0) {
    // the two half-waves of a column, then the four waves, folded in a fixed order as steps of the online softmax
    const float ma = __shfl(m_run, li), mb = __shfl(m_run, li + 32), la = __shfl(l_run, li), lb = __shfl(l_run, li + 32);
    float m = fmaxf(ma, mb);
    float l = m == -INFINITY ? 0.f : la * __builtin_amdgcn_exp2f(ma - m) + lb * __builtin_amdgcn_exp2f(mb - m);
    if (hi == 0) {
      red[wave * 32 + li] = m;
      red[128 + wave * 32 + li] = l;
    }
    __syncthreads();
    if (wave == 0 && hi == 0 && okj) {
      m = -INFINITY;
      for (int x = 0; x < 4; ++x) m = fmaxf(m, red[x * 32 + li]);
      l = 0.f;
      for (int x = 0; x < 4; ++x)
        if (red[x * 32 + li] != -INFINITY) l += red[128 + x * 32 + li] * __builtin_amdgcn_exp2f(red[x * 32 + li] - m);
      const long at = ((long)seg * p.B * p.H + bh) * p.L + j;
      p.stat[2 * at] = m;
      p.stat[2 * at + 1] = l;
    }
  } else if (okj) {
    const long at = (((long)seg * p.B * p.H + bh) * p.L + j) * BA_HD;
#pragma unroll
    for (int y = 0; y < 2; ++y) {
      if (MODE == 1 || want_k) ba_store(p.part0 + at, o0[y], (wave + 4 * y) * 32, 1.f);
      if (want_vl) ba_store(p.part1 + at, o1[y], (wave + 4 * y) * 32, 1.f);
    }
  }
}

// the segments' column statistics -> (mx, ls) and lse per text row, in segment order.  Every segment holds at least one visual row.
__global__ __launch_bounds__(256) void ba_fold_stat_kernel(const BAParams p) {
  const long n = (long)p.B * p.H * p.L, at = (long)blockIdx.x * 256 + threadIdx.x;
  if (at >= n) return;
  float m = -INFINITY;
  for (int sg = 0; sg < p.nseg; ++sg) m = fmaxf(m, p.stat[2 * (sg * n + at)]);
  float l = 0.f;
  for (int sg = 0; sg < p.nseg; ++sg) l += p.stat[2 * (sg * n + at) + 1] * __builtin_amdgcn_exp2f(p.stat[2 * (sg * n + at)] - m);
  const float ls = log2f(l);
  p.sl[2 * at] = m;
  p.sl[2 * at + 1] = ls;
  p.l_l[at] = m + ls;
}

// out (B, L, H 256) = mul * the sum of the segments' (nseg, B, H, L, 256) partial rows, in segment order; 4 columns per thread
__global__ __launch_bounds__(256) void ba_fold_rows_kernel(const float* part, float* out, int nseg, int B, int H, int L, float mul) {
  const long n4 = (long)B * H * L * (BA_HD / 4), at = (long)blockIdx.x * 256 + threadIdx.x;
  if (at >= n4) return;
  const int d = 4 * (int)(at % (BA_HD / 4));
  const long row = at / (BA_HD / 4);                     // (b H + h) L + j
  const int j = (int)(row % L), bh = (int)(row / L), b = bh / H, h = bh % H;
  float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int sg = 0; sg < nseg; ++sg) {
    const float4 t = *reinterpret_cast<const float4*>(part + ((long)sg * B * H * L + row) * BA_HD + d);
    a.x += t.x; a.y += t.y; a.z += t.z; a.w += t.w;
  }
  *reinterpret_cast<float4*>(out + ((long)b * L + j) * ((long)H * BA_HD) + h * BA_HD + d) = make_float4(a.x * mul, a.y * mul, a.z * mul, a.w * mul);
}

// delta_v (B, H, Nv) = dOv . out_v and delta_l (B, H, L) = dOl . out_l per head, each ONE fmaf chain over the 256 columns in their natural
// order -- the chain of the matrix instruction, so that where a probability is exactly 1 (a single attended token, a single visual row)
// dO . v - delta is exactly 0 as in exact arithmetic.  One wave per 64 (image, row, head) items: the rows are staged through LDS 32
// columns at a time with coalesced 16-byte loads, lane l then runs item l's chain.
__global__ __launch_bounds__(64) void ba_delta_kernel(const BAParams p) {
  __shared__ float gs[64 * BA_PS], os[64 * BA_PS];
  const long nv = (long)p.B * p.H * p.Nv, n = nv + (long)p.B * p.H * p.L, first = (long)blockIdx.x * 64;
  const int lane = threadIdx.x;
  float d = 0.f;
  for (int d0 = 0; d0 < BA_HD; d0 += BA_DC) {
    __syncthreads();
    for (int x = lane; x < 64 * (BA_DC / 4); x += 64) {
      const int it = x / (BA_DC / 4), c = 4 * (x % (BA_DC / 4));
      const long at = min(first + it, n - 1);
      const bool vis = at < nv;
      const long y = vis ? at : at - nv;                 // (b N + r) H + h
      const int N = vis ? p.Nv : p.L, h = (int)(y % p.H), r = (int)((y / p.H) % N), b = (int)(y / ((long)p.H * N));
      const float* g = (vis ? p.d_ov + b * p.dov_sb + r * p.dov_st : p.d_ol + b * p.dol_sb + r * p.dol_st) + h * BA_HD + d0 + c;
      const float* o = (vis ? p.out_v : p.out_l) + ((long)b * N + r) * ((long)p.H * BA_HD) + h * BA_HD + d0 + c;
      const float4 g4 = *reinterpret_cast<const float4*>(g), o4 = *reinterpret_cast<const float4*>(o);
      float* gd = gs + it * BA_PS + c;
      float* od = os + it * BA_PS + c;
      gd[0] = g4.x; gd[1] = g4.y; gd[2] = g4.z; gd[3] = g4.w;
      od[0] = o4.x; od[1] = o4.y; od[2] = o4.z; od[3] = o4.w;
    }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < BA_DC; ++c) d = fmaf(gs[lane * BA_PS + c], os[lane * BA_PS + c], d);
  }
  const long at = first + lane;
  if (at >= n) return;
  const bool vis = at < nv;
  const long y = vis ? at : at - nv;
  const int N = vis ? p.Nv : p.L, h = (int)(y % p.H), r = (int)((y / p.H) % N), b = (int)(y / ((long)p.H * N));
  (vis ? p.delta_v : p.delta_l)[((long)b * p.H + h) * N + r] = d;
}

// the split of the visual rows into segments of whole sweep steps: at most BA_MAXSEG, none empty
static void ba_segments(int Nv, int* nseg, int* seglen) {
  const int steps = (Nv + BA_VB - 1) / BA_VB;
  *seglen = ((steps + BA_MAXSEG - 1) / BA_MAXSEG) * BA_VB;
  *nseg = (Nv + *seglen - 1) / *seglen;
}

static inline bool ba_al16(const void* a) { return ((uintptr_t)a & 15) == 0; }
static inline int64_t ba_up4(int64_t n) { return (n + 3) & ~(int64_t)3; }

// what the two entries refuse alike, and the parameters they share
static int ba_setup(const char* who, BAParams& p, const float* q, const float* k, const float* vv, const float* vl, const unsigned char* att,
                    int B, int H, int Nv, int L, int head_dim, int64_t q_sb, int64_t q_st, int64_t k_sb, int64_t k_st, int64_t vv_sb,
                    int64_t vv_st, int64_t vl_sb, int64_t vl_st, double dropout, int64_t seed) {
  HIPIE_REQUIRE(q && k && vv && vl && att, "%s: null pointer", who);
  HIPIE_REQUIRE(head_dim == BA_HD, "%s: head_dim 256 only (got %d)", who, head_dim);
  HIPIE_REQUIRE(L >= 1 && L <= BA_LMAX, "%s: 1 <= L <= %d text rows only (got %d)", who, BA_LMAX, L);
  HIPIE_REQUIRE(B > 0 && B <= 4096 && H > 0 && H <= 512 && Nv > 0 && (int64_t)B * H * ((Nv + 31) / 32) < (1ll << 31) &&
                    (int64_t)B * H * ((int64_t)Nv + L) < (1ll << 32),
                "%s: bad shape B=%d H=%d Nv=%d", who, B, H, Nv);
  HIPIE_REQUIRE(ba_al16(q) && ba_al16(k) && ba_al16(vv) && ba_al16(vl) && ((q_sb | q_st | k_sb | k_st | vv_sb | vv_st | vl_sb | vl_st) & 3) == 0,
                "%s: pointers must be 16-byte aligned and strides multiples of 4 elements", who);
  HIPIE_REQUIRE(q_st >= H * BA_HD && k_st >= H * BA_HD && vv_st >= H * BA_HD && vl_st >= H * BA_HD, "%s: a row stride below the row's width", who);
  HIPIE_REQUIRE(dropout >= 0.0 && dropout < 1.0, "%s: dropout rate %g outside [0, 1)", who, dropout);
  p.q = q; p.k = k; p.vv = vv; p.vl = vl; p.att = att;
  p.B = B; p.H = H; p.Nv = Nv; p.L = L;
  ba_segments(Nv, &p.nseg, &p.seglen);
  p.q_sb = q_sb; p.q_st = q_st; p.k_sb = k_sb; p.k_st = k_st; p.vv_sb = vv_sb; p.vv_st = vv_st; p.vl_sb = vl_sb; p.vl_st = vl_st;
  p.scale = 0.0625f;                                     // 256^-0.5
  const double thr = dropout * 4294967296.0 + 0.5;
  p.thr = dropout == 0.0 ? 0u : (unsigned)(thr >= 4294967295.0 ? 4294967295.0 : (thr < 1.0 ? 1.0 : thr));
  p.keep_inv = (float)(1.0 / (1.0 - dropout));
  p.seed_lo = (unsigned)((uint64_t)seed & 0xffffffffu);
  p.seed_hi = (unsigned)((uint64_t)seed >> 32);
  return HIPIE_OK;
}

}  // namespace hipie

#define BA_LAUNCH(kernel, blocks, what, ...)                                                       \
  do {                                                                                             \
    hipLaunchKernelGGL(kernel, dim3((unsigned)(blocks)), dim3(256), 0, st, __VA_ARGS__);           \
    HIPIE_TRY(check_launch(what));                                                                 \
  } while (0)

extern "C" int64_t hipie_bi_attn_train_forward_ws_bytes(int B, int H, int Nv, int L) {
  using namespace hipie;
  if (B <= 0 || H <= 0 || Nv <= 0 || L <= 0) return 16;
  int nseg, seglen;
  ba_segments(Nv, &nseg, &seglen);
  const int64_t rows = (int64_t)nseg * B * H * L;
  return (ba_up4(2 * rows) + rows * BA_HD) * (int64_t)sizeof(float);
}

extern "C" int hipie_bi_attn_train_forward(const float* q, const float* k, const float* vv, const float* vl, const unsigned char* att,
                                           float* out_v, float* out_l, float* lse_v, float* lse_l, float* stat_v, float* stat_l, void* ws,
                                           int64_t ws_bytes, int B, int H, int Nv, int L, int head_dim, int64_t q_sb, int64_t q_st,
                                           int64_t k_sb, int64_t k_st, int64_t vv_sb, int64_t vv_st, int64_t vl_sb, int64_t vl_st,
                                           double dropout, int64_t seed, void* stream) {
  using namespace hipie;
  BAParams p = {};
  HIPIE_REQUIRE(out_v && out_l && lse_v && lse_l && stat_v && stat_l && ws, "bi_attn_train_forward: null pointer");
  HIPIE_TRY(ba_setup("bi_attn_train_forward", p, q, k, vv, vl, att, B, H, Nv, L, head_dim, q_sb, q_st, k_sb, k_st, vv_sb, vv_st, vl_sb, vl_st,
                     dropout, seed));
  HIPIE_REQUIRE(ba_al16(out_v) && ba_al16(out_l) && ba_al16(ws), "bi_attn_train_forward: pointers must be 16-byte aligned and strides multiples of 4 elements");
  const int64_t need = hipie_bi_attn_train_forward_ws_bytes(B, H, Nv, L);
  HIPIE_REQUIRE(ws_bytes >= need, "bi_attn_train_forward: workspace of %lld bytes, need %lld", (long long)ws_bytes, (long long)need);
  const int64_t rows = (int64_t)p.nseg * B * H * L;
  p.o_v = out_v; p.o_l = out_l; p.l_v = lse_v; p.l_l = lse_l; p.sv = stat_v; p.sl = stat_l; p.st_l = stat_l;
  p.stat = (float*)ws;
  p.part0 = (float*)ws + ba_up4(2 * rows);
  hipStream_t st = (hipStream_t)stream;
  const int nT = (L + 31) / 32;
  BA_LAUNCH(ba_t_kernel<0>, (int64_t)B * H * nT * p.nseg, "bi_attn_train_forward (column statistics)", p);
  BA_LAUNCH(ba_fold_stat_kernel, ((int64_t)B * H * L + 255) / 256, "bi_attn_train_forward (statistics fold)", p);
  BA_LAUNCH(ba_fwd_v_kernel, (int64_t)B * H * ((Nv + 31) / 32), "bi_attn_train_forward (out_v)", p);
  BA_LAUNCH(ba_t_kernel<1>, (int64_t)B * H * nT * p.nseg, "bi_attn_train_forward (out_l)", p);
  BA_LAUNCH(ba_fold_rows_kernel, ((int64_t)B * H * L * (BA_HD / 4) + 255) / 256, "bi_attn_train_forward (out_l fold)", p.part0, out_l, p.nseg, B, H, L, 1.f);
  return HIPIE_OK;
}

extern "C" int64_t hipie_bi_attn_train_backward_ws_bytes(int B, int H, int Nv, int L) {
  using namespace hipie;
  if (B <= 0 || H <= 0 || Nv <= 0 || L <= 0) return 16;
  int nseg, seglen;
  ba_segments(Nv, &nseg, &seglen);
  const int64_t rows = (int64_t)nseg * B * H * L;
  return (ba_up4((int64_t)B * H * Nv) + ba_up4((int64_t)B * H * L) + 2 * rows * BA_HD) * (int64_t)sizeof(float);
}

extern "C" int hipie_bi_attn_train_backward(const float* q, const float* k, const float* vv, const float* vl, const unsigned char* att,
                                            const float* out_v, const float* out_l, const float* stat_v, const float* stat_l,
                                            const float* d_out_v, const float* d_out_l, float* d_q, float* d_k, float* d_vv, float* d_vl,
                                            void* ws, int64_t ws_bytes, int B, int H, int Nv, int L, int head_dim, int64_t q_sb,
                                            int64_t q_st, int64_t k_sb, int64_t k_st, int64_t vv_sb, int64_t vv_st, int64_t vl_sb,
                                            int64_t vl_st, int64_t dov_sb, int64_t dov_st, int64_t dol_sb, int64_t dol_st, double dropout,
                                            int64_t seed, void* stream) {
  using namespace hipie;
  BAParams p = {};
  HIPIE_REQUIRE(out_v && out_l && stat_v && stat_l && d_out_v && d_out_l && ws, "bi_attn_train_backward: null pointer");
  HIPIE_TRY(ba_setup("bi_attn_train_backward", p, q, k, vv, vl, att, B, H, Nv, L, head_dim, q_sb, q_st, k_sb, k_st, vv_sb, vv_st, vl_sb, vl_st,
                     dropout, seed));
  HIPIE_REQUIRE(ba_al16(out_v) && ba_al16(out_l) && ba_al16(d_out_v) && ba_al16(d_out_l) && ba_al16(d_q) && ba_al16(d_k) && ba_al16(d_vv) &&
                    ba_al16(d_vl) && ba_al16(ws) && ((dov_sb | dov_st | dol_sb | dol_st) & 3) == 0,
                "bi_attn_train_backward: pointers must be 16-byte aligned and strides multiples of 4 elements");
  HIPIE_REQUIRE(dov_st >= H * BA_HD && dol_st >= H * BA_HD, "bi_attn_train_backward: a row stride below the row's width");
  const int64_t need = hipie_bi_attn_train_backward_ws_bytes(B, H, Nv, L);
  HIPIE_REQUIRE(ws_bytes >= need, "bi_attn_train_backward: workspace of %lld bytes, need %lld", (long long)ws_bytes, (long long)need);
  if (!d_q && !d_k && !d_vv && !d_vl) return HIPIE_OK;       // every input frozen: nothing is launched
  const int64_t rows = (int64_t)p.nseg * B * H * L;
  p.out_v = out_v; p.out_l = out_l; p.st_v = stat_v; p.st_l = stat_l; p.d_ov = d_out_v; p.d_ol = d_out_l;
  p.d_q = d_q; p.d_k = d_k; p.d_vv = d_vv; p.d_vl = d_vl;
  p.dov_sb = dov_sb; p.dov_st = dov_st; p.dol_sb = dol_sb; p.dol_st = dol_st;
  p.delta_v = (float*)ws;
  p.delta_l = p.delta_v + ba_up4((int64_t)B * H * Nv);
  p.part0 = p.delta_l + ba_up4((int64_t)B * H * L);
  p.part1 = p.part0 + rows * BA_HD;
  hipStream_t st = (hipStream_t)stream;
  const int nT = (L + 31) / 32;
  const int64_t fold = ((int64_t)B * H * L * (BA_HD / 4) + 255) / 256;
  if (d_q || d_k) {                                          // the logit gradient needs the two deltas; d_vv and d_vl do not
    hipLaunchKernelGGL(ba_delta_kernel, dim3((unsigned)(((int64_t)B * H * ((int64_t)Nv + L) + 63) / 64)), dim3(64), 0, st, p);
    HIPIE_TRY(check_launch("bi_attn_train_backward (delta)"));
  }
  if (d_q || d_vv) BA_LAUNCH(ba_bwd_v_kernel, (int64_t)B * H * ((Nv + 31) / 32), "bi_attn_train_backward (d_q, d_vv)", p);
  if (d_k || d_vl) BA_LAUNCH(ba_t_kernel<2>, (int64_t)B * H * nT * p.nseg, "bi_attn_train_backward (d_k, d_vl)", p);
  if (d_k) BA_LAUNCH(ba_fold_rows_kernel, fold, "bi_attn_train_backward (d_k fold)", p.part0, d_k, p.nseg, B, H, L, p.scale);
  if (d_vl) BA_LAUNCH(ba_fold_rows_kernel, fold, "bi_attn_train_backward (d_vl fold)", p.part1, d_vl, p.nseg, B, H, L, 1.f);
  return HIPIE_OK;
}
