// row_norm.h -- what the HBM-bound row kernels share, one definition each: the LayerNorm row of layernorm.hip and layernorm_bwd.hip (lane
// layout, two-pass statistics, affine output) and the deterministic sum of partial rows behind layernorm_bwd.hip and act_bwd.hip.
#pragma once
#include "common.h"
#include "wave.h"

namespace hipie {

constexpr int LN_MAXV = 8;     // up to 8 x 4 elements per lane: C <= 2048

// ---- one wave owns one row of C values (C % 4 == 0): vector i of a lane is the 4 columns from col(i), where on(i) ------------------------
struct LnRow {
  int lane, nv, tail;          // nv full vectors per lane (64 lanes x 4 columns each), then one more for lane < tail
  __device__ __forceinline__ explicit LnRow(int C) : lane(threadIdx.x & 63), nv(C / 256), tail((C - nv * 256) / 4) {}
  __device__ __forceinline__ bool on(int i) const { return (i < nv) || (i == nv && lane < tail); }
  __device__ __forceinline__ int col(int i) const { return i * 256 + lane * 4; }
};

// mean and rstd of the row in v, in every lane, from `sum` = the lane's own sum of its `on` vectors in i, e order (added up where the row is loaded)
template <int NV>
__device__ __forceinline__ void ln_row_stats(const LnRow& r, const float (&v)[NV][4], float sum, int C, float eps, float& mean, float& rstd) {
  mean = wave_sum(sum) / (float)C;
  float sq = 0.f;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    if (r.on(i)) {
#pragma unroll
      for (int e = 0; e < 4; ++e) { const float d = v[i][e] - mean; sq += d * d; }
    }
  }
  rstd = rsqrtf(wave_sum(sq) / (float)C + eps);
}

// o = LN(v) * gamma + beta for one vector; g, b point at its 4 columns of gamma and beta
__device__ __forceinline__ void ln_affine(const float (&v)[4], float mean, float rstd, const float* g, const float* b, float (&o)[4]) {
  float gv[4], bv[4];
  Vec4<float>::load(g, gv);
  Vec4<float>::load(b, bv);
#pragma unroll
  for (int e = 0; e < 4; ++e) o[e] = (v[e] - mean) * rstd * gv[e] + bv[e];
}

// ---- ws (nparts, ncols) -> the column sums, columns < split into out_a and the rest into out_b ------------------------------------------
// A workgroup owns COLS columns; thread (group, col) adds the partial rows group, group + GROUPS, ... in order, the GROUPS group sums are
// added in order by the threads of group 0.  No atomics: GROUPS and COLS fix the order of the additions, and so the bits.
// the sum of column `col` of ws (nparts, ncols), valid in the threads of group 0 (T: float, or double partials -- pair_loss.hip)
template <int GROUPS, int COLS, typename T>
__device__ __forceinline__ T partial_rows_column(const T* __restrict__ ws, int nparts, int ncols, int col, T (*red)[COLS]) {
  const int cx = threadIdx.x % COLS, grp = threadIdx.x / COLS;
  T acc = 0;
  if (col < ncols) {
#pragma unroll 8
    for (int p = grp; p < nparts; p += GROUPS) acc += ws[(long)p * ncols + col];
  }
  red[grp][cx] = acc;
  __syncthreads();
  T t = 0;
  if (grp == 0 && col < ncols) {
    t = red[0][cx];
#pragma unroll
    for (int k = 1; k < GROUPS; ++k) t += red[k][cx];
  }
  return t;
}

template <int GROUPS, int COLS>
__global__ __launch_bounds__(256) void partial_rows_sum_kernel(const float* __restrict__ ws, float* __restrict__ out_a,
                                                               float* __restrict__ out_b, int split, int nparts, int ncols) {
  static_assert(GROUPS * COLS == 256, "one thread per (group, column)");
  __shared__ float red[GROUPS][COLS];
  const int col = blockIdx.x * COLS + threadIdx.x % COLS;
  const float t = partial_rows_column<GROUPS, COLS, float>(ws, nparts, ncols, col, red);
  if (threadIdx.x / COLS == 0 && col < ncols) {
    if (col < split) out_a[col] = t;
    else out_b[col - split] = t;
  }
}

template <int GROUPS, int COLS>
static int partial_rows_sum(const char* what, const float* ws, float* out_a, float* out_b, int split, int nparts, int ncols, hipStream_t st) {
  hipLaunchKernelGGL((partial_rows_sum_kernel<GROUPS, COLS>), dim3((unsigned)((ncols + COLS - 1) / COLS)), dim3(256), 0, st, ws, out_a, out_b,
                     split, nparts, ncols);
  return check_launch(what);
}

}  // namespace hipie
