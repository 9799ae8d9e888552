// layernorm_bwd.hip -- backward of the fused residual-add + LayerNorm of layernorm.hip (fp32, the training step; HBM-bound).
//
//   forward:   s = x + delta;  y = LN(s) * gamma + beta           (hipie_add_layernorm; s is what the forward saved)
//   backward:  xhat = (s - mean) * rstd;  g = gy * gamma
//              dx     = rstd * (g - mean_c(g) - xhat * mean_c(g * xhat)) + gres      (gres: the residual stream's gradient at s, optional)
//              dgamma = sum_rows gy * xhat;   dbeta = sum_rows gy
//
// Replaces torch.autograd through nn.LayerNorm as Block.forward uses it (hipie/backbone/vit.py:212-230, eps 1e-6) and the post-norm
// residuals of DeformableTransformerEncoderLayer.forward (deformable_transformer_dino.py:384-394): the library's layer-norm backward, its
// separate parameter reduction and the accumulation of the residual gradient (three passes) become one.  mean and rstd are RECOMPUTED from
// s on LnRow and ln_row_stats of row_norm.h: the forward kernels' lane layout, and add_layernorm_dec_kernel's own code for the two wave
// reductions and the variance pass (add_layernorm_kernel has the same statements written out) -- the row is read anyway, so no
// statistics tensors are saved.  One wave owns one row at a time (16-byte vector accesses, the forward's lane
// layout) and walks rows with a grid stride; the grid is min(ceil(rows / 4), LNB_MAX_WG) workgroups of four waves, a function of `rows`
// alone.  Bytes per row: C * 4 * (|s| + |gy| + |gres| + |dx|) = 16 C.
//
// dgamma / dbeta: every wave keeps its partial sums in registers over all its rows; at the end the four waves of a workgroup are added
// through LDS in wave order and the workgroup writes ONE partial row (2 C floats) into the workspace; partial_rows_sum_kernel<16, 16> adds
// the partial rows in a fixed order.  No atomics: the results are bit-reproducible from call to call.
#include "common.h"
#include "row_norm.h"

namespace hipie {

constexpr int LNB_MAX_WG = 1024;     // workgroups of the row kernel = partial rows in the workspace: 16 waves per CU on 256 CUs
constexpr int LNB_FIN_COLS = 16;     // the partial-row sum: a workgroup owns 16 columns, 16 groups of partial rows each
constexpr int LNB_FIN_GROUPS = 16;

// NV = vectors per lane = ceil(C / 256): the last one may be partial (lane < tail)
template <int NV, bool PARAMS>
__global__ __launch_bounds__(256) void layernorm_bwd_kernel(const float* __restrict__ s, const float* __restrict__ gy, const float* gres,
                                                            const float* __restrict__ gamma, float* dx, float* __restrict__ ws, long rows,
                                                            int C, float eps) {
  static_assert(NV <= LN_MAXV, "the forward's limit");
  __shared__ float part[PARAMS ? 3 * 2 * NV * 256 : 1];      // waves 1-3 park their partial sums here for wave 0
  const int wave = threadIdx.x >> 6;
  const LnRow r(C);
  float gm[NV][4], dg[NV][4], db[NV][4];
#pragma unroll
  for (int i = 0; i < NV; ++i) {
#pragma unroll
    for (int e = 0; e < 4; ++e) gm[i][e] = dg[i][e] = db[i][e] = 0.f;
    if (r.on(i)) Vec4<float>::load(gamma + r.col(i), gm[i]);
  }
  const float inv_c = 1.f / (float)C;
  for (long row = (long)blockIdx.x * 4 + wave; row < rows; row += (long)gridDim.x * 4) {
    const long base = row * C;
    float v[NV][4], g[NV][4];
    float sum = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      if (r.on(i)) {
        Vec4<float>::load(s + base + r.col(i), v[i]);
        Vec4<float>::load(gy + base + r.col(i), g[i]);
#pragma unroll
        for (int e = 0; e < 4; ++e) sum += v[i][e];
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[i][e] = g[i][e] = 0.f;
      }
    }
    float mean, rstd;
    ln_row_stats(r, v, sum, C, eps, mean, rstd);
    // v <- xhat, g <- gy * gamma (gy itself goes into the parameter sums first); the two row means of the input gradient
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const bool on = r.on(i);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float xh = on ? (v[i][e] - mean) * rstd : 0.f;
        if (PARAMS) {
          dg[i][e] += g[i][e] * xh;
          db[i][e] += g[i][e];
        }
        const float t = g[i][e] * gm[i][e];
        v[i][e] = xh;
        g[i][e] = t;
        s1 += t;
        s2 += t * xh;
      }
    }
    const float m1 = wave_sum(s1) * inv_c, m2 = wave_sum(s2) * inv_c;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      if (r.on(i)) {
        const long c = base + r.col(i);
        float o[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = rstd * (g[i][e] - m1 - v[i][e] * m2);
        if (gres != nullptr) {            // dx may BE gres: the lane reads its own four values before it writes them
          float q[4];
          Vec4<float>::load(gres + c, q);
#pragma unroll
          for (int e = 0; e < 4; ++e) o[e] += q[e];
        }
        Vec4<float>::store(dx + c, o);
      }
    }
  }
  if (PARAMS) {
    // every wave reaches this point (a wave without rows holds zeros).  Lane-major LDS layout: consecutive lanes are 16 bytes apart.
    if (wave > 0) {
      float* p = part + (wave - 1) * 2 * NV * 256;
#pragma unroll
      for (int i = 0; i < NV; ++i) {
        Vec4<float>::store(p + r.col(i), dg[i]);
        Vec4<float>::store(p + NV * 256 + r.col(i), db[i]);
      }
    }
    __syncthreads();
    if (wave == 0) {
      float* out = ws + (long)blockIdx.x * 2 * C;
#pragma unroll
      for (int i = 0; i < NV; ++i) {
#pragma unroll
        for (int w = 0; w < 3; ++w) {                 // ((w0 + w1) + w2) + w3
          const float* p = part + w * 2 * NV * 256;
          float a[4], b[4];
          Vec4<float>::load(p + r.col(i), a);
          Vec4<float>::load(p + NV * 256 + r.col(i), b);
#pragma unroll
          for (int e = 0; e < 4; ++e) { dg[i][e] += a[e]; db[i][e] += b[e]; }
        }
        if (r.on(i)) {
          Vec4<float>::store(out + r.col(i), dg[i]);
          Vec4<float>::store(out + C + r.col(i), db[i]);
        }
      }
    }
  }
}

static inline int lnb_workgroups(int64_t rows) {
  const int64_t want = (rows + 3) / 4;
  return (int)(want < LNB_MAX_WG ? want : LNB_MAX_WG);
}

template <int NV>
static void launch_lnb(bool params, int grid, hipStream_t st, const float* s, const float* gy, const float* gres, const float* gamma, float* dx,
                       float* ws, long rows, int C, float eps) {
  if (params)
    hipLaunchKernelGGL((layernorm_bwd_kernel<NV, true>), dim3(grid), dim3(256), 0, st, s, gy, gres, gamma, dx, ws, rows, C, eps);
  else
    hipLaunchKernelGGL((layernorm_bwd_kernel<NV, false>), dim3(grid), dim3(256), 0, st, s, gy, gres, gamma, dx, ws, rows, C, eps);
}

}  // namespace hipie

extern "C" int64_t hipie_layernorm_backward_ws_bytes(int64_t rows, int C) {
  if (rows <= 0 || C <= 0) return 16;
  return (int64_t)hipie::lnb_workgroups(rows) * 2 * C * (int64_t)sizeof(float);
}

extern "C" int hipie_layernorm_backward(const float* s, const float* gy, const float* gres, const float* gamma, float* dx, float* dgamma,
                                        float* dbeta, void* ws, int64_t ws_bytes, int64_t rows, int C, float eps, void* stream) {
  using namespace hipie;
  HIPIE_REQUIRE(rows >= 0 && C > 0 && C % 4 == 0 && C <= LN_MAXV * 256, "layernorm_backward: C=%d must be a multiple of 4 and <= %d", C, LN_MAXV * 256);
  HIPIE_REQUIRE((dgamma == nullptr) == (dbeta == nullptr), "layernorm_backward: dgamma and dbeta go together (both or neither)");
  hipStream_t st = (hipStream_t)stream;
  const bool params = dgamma != nullptr;
  if (rows == 0) {
    if (params) {
      if (hipMemsetAsync(dgamma, 0, (size_t)C * sizeof(float), st) != hipSuccess || hipMemsetAsync(dbeta, 0, (size_t)C * sizeof(float), st) != hipSuccess)
        return check_launch("layernorm_backward (zero fill)");
    }
    return HIPIE_OK;
  }
  HIPIE_REQUIRE(s && gy && gamma && dx, "layernorm_backward: null pointer");
  HIPIE_REQUIRE((const float*)dx != s && (const float*)dx != gy, "layernorm_backward: dx must not alias s or gy (only gres)");
  HIPIE_REQUIRE((((uintptr_t)s | (uintptr_t)gy | (uintptr_t)gres | (uintptr_t)gamma | (uintptr_t)dx | (uintptr_t)ws) & 15) == 0,
                "layernorm_backward: buffers must be 16-byte aligned");
  HIPIE_REQUIRE(!params || (ws != nullptr && ws_bytes >= hipie_layernorm_backward_ws_bytes(rows, C)),
                "layernorm_backward: workspace of %lld bytes, need %lld", (long long)ws_bytes, (long long)hipie_layernorm_backward_ws_bytes(rows, C));
  const int grid = lnb_workgroups(rows);
  float* w = (float*)ws;
  switch ((C + 255) / 256) {
    case 1: launch_lnb<1>(params, grid, st, s, gy, gres, gamma, dx, w, rows, C, eps); break;
    case 2: launch_lnb<2>(params, grid, st, s, gy, gres, gamma, dx, w, rows, C, eps); break;
    case 3: launch_lnb<3>(params, grid, st, s, gy, gres, gamma, dx, w, rows, C, eps); break;
    case 4: launch_lnb<4>(params, grid, st, s, gy, gres, gamma, dx, w, rows, C, eps); break;
    case 5: launch_lnb<5>(params, grid, st, s, gy, gres, gamma, dx, w, rows, C, eps); break;
    case 6: launch_lnb<6>(params, grid, st, s, gy, gres, gamma, dx, w, rows, C, eps); break;
    case 7: launch_lnb<7>(params, grid, st, s, gy, gres, gamma, dx, w, rows, C, eps); break;
    default: launch_lnb<8>(params, grid, st, s, gy, gres, gamma, dx, w, rows, C, eps); break;
  }
  const int rc = check_launch("layernorm_backward");
  if (rc != HIPIE_OK || !params) return rc;
  return partial_rows_sum<LNB_FIN_GROUPS, LNB_FIN_COLS>("layernorm_backward (partial-row sum)", w, dgamma, dbeta, C, grid, 2 * C, st);
}
