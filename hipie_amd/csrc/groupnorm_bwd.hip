// groupnorm_bwd.hip -- backward of the NCHW fp32 GroupNorm (+ ReLU) of groupnorm.hip for the training step (HBM-bound).
//
//   forward:   y = act(xhat * gamma_c + beta_c),  xhat = (x - mean) * rstd per (image, group of 8 channels);  act = ReLU or nothing
//   backward:  m = 1, or with ReLU m = [fmaf(x, sc, sh) > 0] from the forward's own sc / sh (gn_scale_shift_nchw): the forward's `y > 0`
//              bit for bit, so neither y nor a mask is saved;   g = dy * m,   n = 8 HW
//              dx     = rstd * (gamma_c * g - (s1 + xhat * s2) / n),   s1 = sum_group gamma_c g,   s2 = sum_group gamma_c g xhat
//              dgamma = sum_{b, pixels} g * xhat,   dbeta = sum_{b, pixels} g
//
// Replaces torch.autograd through the nn.GroupNorm(32, 256) (+ F.relu) of the conv + GN blocks after the backbone (input_proj of both heads,
// deformable_detr.py:139-160; the lateral / output convs and the mask_features head of the pixel decoder, maskdino_encoder.py:262-300): the
// library's two-pass group-norm backward in front of the ReLU backward, about 8 transfers of the tensor and a saved pre-ReLU map, become 5
// transfers (x, dy; x, dy, dx) and no second map.  mean / rstd come from the forward (stat, (B, G, 2)).
//
// Pass 1, one workgroup per (chunk, image * channel) -- the forward's chunking, gn_nchw_chunks, so the workgroups of a row walk contiguous
// memory: (sum g xhat, sum g) of the chunk into the workspace, laid out (B * nchunk) partial rows of 2 C floats.
// Pass 2, the same grid: wave 0 first adds its group's 8 x nchunk partials, weighted with gamma, in a fixed order (every workgroup of a
// group gets the same bits), then the chunk's dx.   Finisher: partial_rows_sum of row_norm.h adds the partial rows in a fixed order.
// No atomics: the results are bit-reproducible from call to call.
#include "common.h"
#include "groupnorm.h"
#include "row_norm.h"

namespace hipie {

constexpr int GNB_FIN_COLS = 16;     // the partial-row sum: a workgroup owns 16 columns, 16 groups of partial rows each
constexpr int GNB_FIN_GROUPS = 16;

// what both passes know of their (chunk, image, channel): the statistics, the forward's fma and the element range
struct GnbRow {
  int c, b, e0, e1;
  float mean, rstd, gamma, sc, sh;
  __device__ __forceinline__ GnbRow(const float* stat, const float* gm, const float* bt, int HW, int C, int per) {
    const int bc = blockIdx.y;
    c = bc % C;
    b = bc / C;
    const float* sp = stat + ((long)b * (C / GN_CPG) + c / GN_CPG) * 2;
    mean = sp[0];
    rstd = sp[1];
    gamma = gm[c];
    gn_scale_shift_nchw(gamma, bt[c], 0.f, mean, rstd, sc, sh);
    e0 = blockIdx.x * per + threadIdx.x * 8;
    e1 = min(HW, (blockIdx.x + 1) * per);
  }
};

template <bool RELU>
__global__ __launch_bounds__(256) void gn_bwd_partial_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                             const float* __restrict__ stat, const float* __restrict__ gamma,
                                                             const float* __restrict__ beta, float* __restrict__ ws, int HW, int C,
                                                             int nchunk, int per) {
  __shared__ float red[2][4];
  const GnbRow r(stat, gamma, beta, HW, C, per);
  const float* xp = x + (long)blockIdx.y * HW;
  const float* gp = dy + (long)blockIdx.y * HW;
  float sg = 0.f, sgx = 0.f;
  for (int e = r.e0; e < r.e1; e += 256 * 8) {
    float v[8], d[8];
    V8<float>::ld(xp + e, v);
    V8<float>::ld(gp + e, d);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const float g = (!RELU || fmaf(v[i], r.sc, r.sh) > 0.f) ? d[i] : 0.f;
      sg += g;
      sgx = fmaf(g, (v[i] - r.mean) * r.rstd, sgx);
    }
  }
  sg = wave_sum(sg);
  sgx = wave_sum(sgx);
  if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = sgx; red[1][threadIdx.x >> 6] = sg; }
  __syncthreads();
  if (threadIdx.x == 0) {
    float* o = ws + ((long)r.b * nchunk + blockIdx.x) * 2 * C + r.c;       // partial row (b, chunk): [sum g xhat (C) | sum g (C)]
    o[0] = red[0][0] + red[0][1] + red[0][2] + red[0][3];
    o[C] = red[1][0] + red[1][1] + red[1][2] + red[1][3];
  }
}

template <bool RELU>
__global__ __launch_bounds__(256) void gn_bwd_dx_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                        const float* __restrict__ stat, const float* __restrict__ gamma,
                                                        const float* __restrict__ beta, const float* __restrict__ ws,
                                                        float* __restrict__ dx, int HW, int C, int nchunk, int per) {
  __shared__ float sums[2];
  const GnbRow r(stat, gamma, beta, HW, C, per);
  if (threadIdx.x < 64) {
    const int c0 = (r.c / GN_CPG) * GN_CPG, K = nchunk * GN_CPG;
    float s1 = 0.f, s2 = 0.f;
    for (int k = threadIdx.x; k < K; k += 64) {                            // k = (channel of the group, chunk)
      const int cc = c0 + k / nchunk;
      const float* p = ws + ((long)r.b * nchunk + k % nchunk) * 2 * C + cc;
      const float gm = gamma[cc];
      s2 = fmaf(gm, p[0], s2);
      s1 = fmaf(gm, p[C], s1);
    }
    s1 = wave_sum(s1);
    s2 = wave_sum(s2);
    if (threadIdx.x == 0) { sums[0] = s1; sums[1] = s2; }
  }
  __syncthreads();
  const float inv_n = 1.f / ((float)HW * GN_CPG);
  const float s1 = sums[0], s2 = sums[1];
  const float* xp = x + (long)blockIdx.y * HW;
  const float* gp = dy + (long)blockIdx.y * HW;
  float* op = dx + (long)blockIdx.y * HW;
  for (int e = r.e0; e < r.e1; e += 256 * 8) {
    float v[8], d[8];
    V8<float>::ld(xp + e, v);
    V8<float>::ld(gp + e, d);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const float g = (!RELU || fmaf(v[i], r.sc, r.sh) > 0.f) ? d[i] : 0.f;
      const float xh = (v[i] - r.mean) * r.rstd;
      d[i] = r.rstd * (r.gamma * g - (s1 + xh * s2) * inv_n);
    }
    V8<float>::st(op + e, d);
  }
}

}  // namespace hipie

extern "C" int64_t hipie_group_norm_backward_ws_bytes(int B, int C, int HW) {
  if (B <= 0 || C <= 0 || HW <= 0) return 16;
  int nchunk, per;
  hipie::gn_nchw_chunks(HW, nchunk, per);
  return (int64_t)B * nchunk * 2 * C * (int64_t)sizeof(float);
}

extern "C" int hipie_group_norm_backward(const float* x, const float* dy, const float* stat, const float* gamma, const float* beta,
                                         float* dx, float* dgamma, float* dbeta, void* ws, int64_t ws_bytes, int B, int C, int HW,
                                         int groups, int relu, void* stream) {
  using namespace hipie;
  HIPIE_REQUIRE(x && dy && stat && gamma && beta && ws, "group_norm_backward: null pointer");
  HIPIE_REQUIRE(B >= 0 && C > 0 && HW > 0, "group_norm_backward: bad shape");
  HIPIE_REQUIRE(groups > 0 && C == groups * GN_CPG && groups <= 64 && 256 % groups == 0,
                "group_norm_backward: %d channels in %d groups unsupported (8 channels per group, 256 %% groups == 0)", C, groups);
  HIPIE_REQUIRE(HW % 8 == 0, "group_norm_backward: NCHW needs H*W %% 8 == 0 (got %d)", HW);
  HIPIE_REQUIRE((dgamma == nullptr) == (dbeta == nullptr), "group_norm_backward: dgamma and dbeta go together (both or neither)");
  const int64_t need = hipie_group_norm_backward_ws_bytes(B, C, HW);
  HIPIE_REQUIRE(ws_bytes >= need, "group_norm_backward: workspace of %lld bytes, need %lld", (long long)ws_bytes, (long long)need);
  if (B == 0 || (dx == nullptr && dgamma == nullptr)) return HIPIE_OK;
  hipStream_t st = (hipStream_t)stream;
  int nchunk, per;
  gn_nchw_chunks(HW, nchunk, per);
  const dim3 grid(nchunk, B * C);
  float* w = (float*)ws;
  if (relu) hipLaunchKernelGGL((gn_bwd_partial_kernel<true>), grid, dim3(256), 0, st, x, dy, stat, gamma, beta, w, HW, C, nchunk, per);
  else hipLaunchKernelGGL((gn_bwd_partial_kernel<false>), grid, dim3(256), 0, st, x, dy, stat, gamma, beta, w, HW, C, nchunk, per);
  int rc = check_launch("group_norm_backward (partial sums)");
  if (rc != HIPIE_OK) return rc;
  if (dx != nullptr) {
    if (relu) hipLaunchKernelGGL((gn_bwd_dx_kernel<true>), grid, dim3(256), 0, st, x, dy, stat, gamma, beta, (const float*)w, dx, HW, C, nchunk, per);
    else hipLaunchKernelGGL((gn_bwd_dx_kernel<false>), grid, dim3(256), 0, st, x, dy, stat, gamma, beta, (const float*)w, dx, HW, C, nchunk, per);
    rc = check_launch("group_norm_backward");
    if (rc != HIPIE_OK) return rc;
  }
  if (dgamma == nullptr) return HIPIE_OK;
  return partial_rows_sum<GNB_FIN_GROUPS, GNB_FIN_COLS>("group_norm_backward (partial-row sum)", w, dgamma, dbeta, C, B * nchunk, 2 * C, st);
}
