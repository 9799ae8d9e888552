// conv_wgrad.hip -- weight and bias gradient of the dense 3 x 3 / stride 1 / padding 1 convolution of the training step, on the zero-padded
// pixel grid hipie_conv3x3_split computes on (B (H+2) (W+2) rows of channels, zero border, Wp + 1 guard rows on both ends).
//
//   dW[n, tap, c] = sum_rows g[row, n] * x[row + shift(tap), c],   shift(ty, tx) = (ty - 1) Wp + (tx - 1)
//   db[n]         = sum_rows g[row, n],                             g = dy, or with the ReLU fused into the node dy * [y > 0]
//
// The contraction runs over the pixel rows, the SLOW axis of both row-major operands.  Nothing is transposed in memory: both tiles are staged
// row-major in LDS as fp16 hi / lo planes of 32-column blocks (64-byte rows, so the 4 rows x 64 bytes a half wave reads are 256 contiguous
// bytes: conflict-free) and ds_read_b64_tr_b16 hands each lane 4 consecutive ROWS of one column -- the k-contiguous MFMA operand of a
// matrix stored with k as the row index (mfma.h).  A tap is a row offset of the x tile's read address, nothing else.
//
// Decomposition: a workgroup owns (chunk of WG_CHUNK grid rows) x (64 n) x (64 c) x (one tap ROW ty).  With the tap row in the grid the x
// tile needs a halo of ONE row on each side instead of Wp + 1 (131 rows at a 128-wide map: with a halo that deep a 64-row stage would read
// x five times over, and a stage deep enough to amortise it would not fit LDS beside the dy tile), the three taps of the row are the read
// offsets 0, 1, 2 into that tile, and a wave carries 3 accumulator tiles instead of 9.  Per stage of 64 rows: dy 64 x 64 and x 66 x 64 are
// loaded once as fp32, masked (dy), split and stored; each of the 4 waves owns one 32 x 32 (n, c) tile for the 3 taps and issues 9 MFMAs
// (three-product split: hi hi, hi lo, lo hi) per 16-row step from 16 transposing reads.
// Per-chunk partials go to the workspace, partial row `chunk` = [dW (N, 9, C) | db (N)]; partial_rows_sum of row_norm.h adds the partial rows
// in chunk order.  No atomics: two calls give the same bits.  db comes from the fp32 values as they are staged (before the split), summed
// per thread in row order and folded over the 16 thread rows in a fixed order, by the workgroups of c block 0 and tap row 0.
#include "common.h"
#include "mfma.h"
#include "row_norm.h"
#include "wave.h"

namespace hipie {

constexpr int WG_CHUNK = 2048;      // grid rows per partial (hipie_amd/ops.py conv3x3_wgrad sizes the workspace with the same number)
constexpr int WG_R = 64;            // rows per LDS stage
constexpr int WG_T = 64;            // n and c extent of a workgroup: 2 x 2 tiles of 32 x 32, one per wave
constexpr int WG_FIN_COLS = 64;     // the partial-row sum: a workgroup owns 64 columns, 4 groups of partial rows each
constexpr int WG_FIN_GROUPS = 4;

// one fp32 quad -> 4 hi and 4 lo fp16 values at (32-column block, row, column in block) of the planes H / L ([2][ROWS][32])
__device__ __forceinline__ void wg_store_split(f16_t* H, f16_t* L, int plane_rows, int row, int q, const float (&v)[4]) {
  f16x4 h, l;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    f16_t a, b;
    hl_split(v[e], a, b);
    h[e] = a;
    l[e] = b;
  }
  const int o = ((q >> 3) * plane_rows + row) * 32 + (q & 7) * 4;
  *reinterpret_cast<f16x4*>(H + o) = h;
  *reinterpret_cast<f16x4*>(L + o) = l;
}

template <bool MASK>
__global__ __launch_bounds__(256) void conv3x3_wgrad_kernel(const float* __restrict__ x, long ldx, const float* __restrict__ dy, long ldg,
                                                            const float* __restrict__ y, long rows, int Wp, int C, int N,
                                                            float* __restrict__ ws, long ncols, int want_db) {
  typedef Mfma32<f16_t>::frag frag;
  typedef Mfma32<f16_t>::half_frag hfrag;
  __shared__ __attribute__((aligned(16))) f16_t gH[2 * WG_R * 32], gL[2 * WG_R * 32];
  __shared__ __attribute__((aligned(16))) f16_t xH[2 * (WG_R + 2) * 32], xL[2 * (WG_R + 2) * 32];
  __shared__ float red[16][WG_T];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int cblocks = (C + WG_T - 1) / WG_T;
  const int n0 = (blockIdx.y / cblocks) * WG_T, c0 = (blockIdx.y % cblocks) * WG_T;
  const int ty = blockIdx.z;
  const long chunk0 = (long)blockIdx.x * WG_CHUNK;
  const long chunk1 = chunk0 + WG_CHUNK < rows ? chunk0 + WG_CHUNK : rows;
  const long guard = (long)Wp + 1;
  const bool do_db = want_db && c0 == 0 && ty == 0;

  const int srow = tid >> 4, sq = tid & 15;               // staging: thread -> (row within 16, quad of 4 columns)
  const bool n_on = n0 + 4 * sq < N, c_on = c0 + 4 * sq < C;
  float bsum[4] = {0.f, 0.f, 0.f, 0.f};

  const int nt = wave >> 1, ct = wave & 1;                // compute: wave -> 32 x 32 tile of (n, c)
  const int l16 = lane & 15, g1 = (lane >> 4) & 1, hi = lane >> 5;
  const int foff = (4 * hi + (l16 >> 2)) * 32 + 16 * g1 + 4 * (l16 & 3);     // rows 4 hi .. + 3 (and + 8), column lane & 31 of a block
  const f16_t* aH = gH + nt * WG_R * 32 + foff;
  const f16_t* aL = gL + nt * WG_R * 32 + foff;
  const f16_t* bH = xH + ct * (WG_R + 2) * 32 + foff;
  const f16_t* bL = xL + ct * (WG_R + 2) * 32 + foff;

  f32x16 acc[3];
#pragma unroll
  for (int t = 0; t < 3; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;

  for (long r0 = chunk0; r0 < chunk1; r0 += WG_R) {
    // ---- stage g = dy (* [y > 0]): rows r0 .. r0 + 63, zero beyond the chunk and beyond N ----
#pragma unroll
    for (int i = 0; i < WG_R / 16; ++i) {
      const int row = srow + 16 * i;
      const long gr = r0 + row;
      float v[4] = {0.f, 0.f, 0.f, 0.f};
      if (n_on && gr < chunk1) {
        const long o = gr * ldg + n0 + 4 * sq;
        Vec4<float>::load(dy + o, v);
        if (MASK) {
          float m[4];
          Vec4<float>::load(y + o, m);
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] = m[e] > 0.f ? v[e] : 0.f;
        }
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) bsum[e] += v[e];
      wg_store_split(gH, gL, WG_R, row, sq, v);
    }
    // ---- stage x: rows r0 + (ty - 1) Wp - 1 .. + 65, zero outside the grid and its guard rows and beyond C ----
    const long xr0 = r0 + (long)(ty - 1) * Wp - 1;
#pragma unroll
    for (int i = 0; i < (WG_R + 2 + 15) / 16; ++i) {
      const int row = srow + 16 * i;
      if (row < WG_R + 2) {
        const long xr = xr0 + row;
        float v[4] = {0.f, 0.f, 0.f, 0.f};
        if (c_on && xr >= -guard && xr < rows + guard) Vec4<float>::load(x + xr * ldx + c0 + 4 * sq, v);
        wg_store_split(xH, xL, WG_R + 2, row, sq, v);
      }
    }
    __syncthreads();
    // ---- 4 steps of 16 rows: A = g^T (n, rows), B = x (rows + tx, c) for the taps tx = 0, 1, 2 of this tap row ----
#pragma unroll
    for (int ks = 0; ks < WG_R / 16; ++ks) {
      const int ko = 16 * ks * 32;
      const hfrag a0 = Mfma32<f16_t>::tr_read(aH + ko), a1 = Mfma32<f16_t>::tr_read(aH + ko + 8 * 32);
      const hfrag a2 = Mfma32<f16_t>::tr_read(aL + ko), a3 = Mfma32<f16_t>::tr_read(aL + ko + 8 * 32);
      frag ah, al;
#pragma unroll
      for (int j = 0; j < 4; ++j) { ah[j] = a0[j]; ah[4 + j] = a1[j]; al[j] = a2[j]; al[4 + j] = a3[j]; }
#pragma unroll
      for (int tx = 0; tx < 3; ++tx) {
        const int bo = ko + tx * 32;
        const hfrag b0 = Mfma32<f16_t>::tr_read(bH + bo), b1 = Mfma32<f16_t>::tr_read(bH + bo + 8 * 32);
        const hfrag b2 = Mfma32<f16_t>::tr_read(bL + bo), b3 = Mfma32<f16_t>::tr_read(bL + bo + 8 * 32);
        frag bh, bl;
#pragma unroll
        for (int j = 0; j < 4; ++j) { bh[j] = b0[j]; bh[4 + j] = b1[j]; bl[j] = b2[j]; bl[4 + j] = b3[j]; }
        acc[tx] = Mfma32<f16_t>::mma(ah, bh, acc[tx]);
        acc[tx] = Mfma32<f16_t>::mma(ah, bl, acc[tx]);
        acc[tx] = Mfma32<f16_t>::mma(al, bh, acc[tx]);
      }
    }
    __syncthreads();
  }

  // ---- the chunk's partial: dW[n, 3 ty + tx, c] of this workgroup's tiles ----
  float* part = ws + (long)blockIdx.x * ncols;
  const int nb = n0 + 32 * nt, cb = c0 + 32 * ct;
  if (nb < N && cb < C) {
#pragma unroll
    for (int tx = 0; tx < 3; ++tx)
#pragma unroll
      for (int r = 0; r < 16; ++r)
        part[((long)(nb + crow(r, hi)) * 9 + 3 * ty + tx) * C + cb + (lane & 31)] = acc[tx][r];
  }
  if (do_db) {                                            // block-uniform
#pragma unroll
    for (int e = 0; e < 4; ++e) red[srow][4 * sq + e] = bsum[e];
    __syncthreads();
    if (tid < WG_T && n0 + tid < N) {
      float t = red[0][tid];
#pragma unroll
      for (int k = 1; k < 16; ++k) t += red[k][tid];
      part[(long)N * 9 * C + n0 + tid] = t;
    }
  }
}

}  // namespace hipie

extern "C" int hipie_conv3x3_wgrad(const float* x, int64_t ldx, const float* dy, int64_t ldg, const float* y, int64_t rows, int Wp, int C,
                                   int N, float* dw, float* db, void* ws, int64_t ws_bytes, void* stream) {
  using namespace hipie;
  HIPIE_REQUIRE(x && dy && dw && ws, "conv3x3_wgrad: null pointer");
  HIPIE_REQUIRE(rows > 0 && rows < (1L << 31) && Wp >= 3 && C > 0 && C % 32 == 0 && N > 0 && N % 32 == 0,
                "conv3x3_wgrad: rows=%ld Wp=%d C=%d N=%d (C %% 32, N %% 32)", (long)rows, Wp, C, N);
  HIPIE_REQUIRE((long)N * 9 * C + N < (1L << 31), "conv3x3_wgrad: N=%d x 9 x C=%d too large", N, C);
  HIPIE_REQUIRE(ldx >= C && ldx % 4 == 0 && ldg >= N && ldg % 4 == 0, "conv3x3_wgrad: row strides %ld / %ld (>= C / N, multiples of 4)",
                (long)ldx, (long)ldg);
  for (const void* p : {(const void*)x, (const void*)dy, (const void*)y, (const void*)dw, (const void*)db, (const void*)ws})
    HIPIE_REQUIRE(((uintptr_t)p % 16) == 0, "conv3x3_wgrad: pointers must be 16-byte aligned");
  const long nchunk = (rows + WG_CHUNK - 1) / WG_CHUNK;
  const long ncols = (long)N * 9 * C + (db != nullptr ? N : 0);
  const long long need = (long long)nchunk * ((long)N * 9 * C + N) * (long long)sizeof(float);
  HIPIE_REQUIRE(ws_bytes >= need, "conv3x3_wgrad: workspace of %lld bytes, need %lld", (long long)ws_bytes, need);
  const long blocks_y = (long)((N + WG_T - 1) / WG_T) * ((C + WG_T - 1) / WG_T);
  HIPIE_REQUIRE(blocks_y <= 65535, "conv3x3_wgrad: N=%d x C=%d too many blocks", N, C);
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)nchunk, (unsigned)blocks_y, 3);
  float* w = (float*)ws;
  if (y != nullptr)
    hipLaunchKernelGGL((conv3x3_wgrad_kernel<true>), grid, dim3(256), 0, st, x, (long)ldx, dy, (long)ldg, y, (long)rows, Wp, C, N, w, ncols,
                       db != nullptr ? 1 : 0);
  else
    hipLaunchKernelGGL((conv3x3_wgrad_kernel<false>), grid, dim3(256), 0, st, x, (long)ldx, dy, (long)ldg, y, (long)rows, Wp, C, N, w, ncols,
                       db != nullptr ? 1 : 0);
  HIPIE_TRY(check_launch("conv3x3_wgrad (partial products)"));
  return partial_rows_sum<WG_FIN_GROUPS, WG_FIN_COLS>("conv3x3_wgrad (partial-row sum)", w, dw, db, N * 9 * C, (int)nchunk, (int)ncols, st);
}
