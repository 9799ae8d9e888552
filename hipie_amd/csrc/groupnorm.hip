// groupnorm.hip -- GroupNorm(32 groups of 8 channels) of the conv + GN blocks after the backbone (input_proj of both heads,
// the FPN lateral / output convs and the mask_features head of the MaskDINO pixel decoder: deformable_detr.py:139-160,
// maskdino_encoder.py:262-300), with the pieces eager PyTorch runs as separate passes folded in:
//   * channels-last input is normalised in place of layout (the library path first copies NHWC -> NCHW),
//   * an optional per-channel pre-bias (the bias of a bias-less library transposed conv), and an optional ReLU,
//   * output in the same layout, any of f32 / f16 / bf16.
// Two launches: partial (sum, sum of squares) per (image, group, chunk) in fp32, then the apply pass, which first reduces the
// partials of its groups (deterministic: no atomics).  HBM-bound: 2 reads + 1 write of the tensor.
// The sums are SHIFTED: every value has K = (first value of its group, pre-bias included) subtracted before it is accumulated --
// var = E[(a-K)^2] - (E[a-K])^2 is then free of the cancellation that E[a^2] - mean^2 suffers when |mean| >> std (real
// convolution biases folded in as pre-bias), at the cost of one extra scalar load per block.
// For the training step (hipie_group_norm_train_forward): the same two NCHW launches, then a finisher that writes the (mean, rstd) the
// apply pass used per (image, group) for groupnorm_bwd.hip.
#include "common.h"
#include "groupnorm.h"
#include "wave.h"

namespace hipie {

// ---- channels-last: x (B, HW, C), C = 8 G.  thread -> (group = t % G, pixel lane = t / G) ----
template <typename T>
__global__ __launch_bounds__(256) void gn_stats_nhwc_kernel(const T* __restrict__ x, const float* __restrict__ prebias,
                                                            float* __restrict__ part, int HW, int G, int nchunk, int per) {
  __shared__ float red[2][256];
  const int b = blockIdx.y, chunk = blockIdx.x;
  const int g = threadIdx.x % G, pl = threadIdx.x / G, npl = 256 / G;
  const int C = G * GN_CPG;
  float pb[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) pb[i] = prebias ? prebias[g * 8 + i] : 0.f;
  const int p1 = min(HW, (chunk + 1) * per);
  const float K = (float)x[(long)b * HW * C + g * 8] + pb[0];          // the group's shift: its first value
  float s = 0.f, ss = 0.f;
  for (int p = chunk * per + pl; p < p1; p += npl) {
    float v[8];
    V8<T>::ld(x + ((long)b * HW + p) * C + g * 8, v);
#pragma unroll
    for (int i = 0; i < 8; ++i) { const float a = v[i] + pb[i] - K; s += a; ss = fmaf(a, a, ss); }
  }
  red[0][threadIdx.x] = s;
  red[1][threadIdx.x] = ss;
  __syncthreads();
  if (threadIdx.x < G) {
    for (int k = 1; k < npl; ++k) { s += red[0][threadIdx.x + k * G]; ss += red[1][threadIdx.x + k * G]; }
    float* o = part + (((long)b * G + g) * nchunk + chunk) * 2;
    o[0] = s; o[1] = ss;
  }
}

// sum and sum of squares of a group's SHIFTED values (shift K, n values) -> the group's mean and rstd
__device__ __forceinline__ void gn_mean_rstd(float s, float ss, float n, float K, float eps, float& mean, float& rstd) {
  const float ms = s / n;                                                // mean of the shifted values
  mean = K + ms;
  rstd = rsqrtf(fmaxf(ss / n - ms * ms, 0.f) + eps);
}

// channels-last, thread t < G: the partials of group t of image b, added in chunk order -> stat[0][t] = mean, stat[1][t] = rstd
template <typename T>
__device__ __forceinline__ void gn_group_stats_nhwc(const T* x, const float* prebias, const float* part, int b, int HW, int G, int nchunk,
                                                    float eps, float (&stat)[2][64]) {
  const int t = threadIdx.x;
  float s = 0.f, ss = 0.f;
  const float* pp = part + ((long)b * G + t) * nchunk * 2;
  for (int k = 0; k < nchunk; ++k) { s += pp[2 * k]; ss += pp[2 * k + 1]; }
  const float K = (float)x[(long)b * HW * (G * GN_CPG) + t * 8] + (prebias ? prebias[t * 8] : 0.f);
  gn_mean_rstd(s, ss, (float)HW * GN_CPG, K, eps, stat[0][t], stat[1][t]);
}

// y = v * sc + sh for the 8 channels of group g: the normalisation, gamma / beta and the pre-bias in one fma per value
__device__ __forceinline__ void gn_scale_shift(const float* gamma, const float* beta, const float* prebias, int g, float mean, float rstd,
                                               float (&sc)[8], float (&sh)[8]) {
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    sc[i] = rstd * gamma[g * 8 + i];
    sh[i] = beta[g * 8 + i] + ((prebias ? prebias[g * 8 + i] : 0.f) - mean) * sc[i];
  }
}

template <typename T, typename OutT>
__global__ __launch_bounds__(256) void gn_apply_nhwc_kernel(const T* __restrict__ x, const float* __restrict__ prebias,
                                                            const float* __restrict__ part, const float* __restrict__ gamma,
                                                            const float* __restrict__ beta, OutT* __restrict__ out, int HW, int G,
                                                            int nchunk, int per, float eps, int relu) {
  __shared__ float stat[2][64];
  const int b = blockIdx.y, chunk = blockIdx.x;
  const int g = threadIdx.x % G, pl = threadIdx.x / G, npl = 256 / G;
  const int C = G * GN_CPG;
  if (threadIdx.x < G) gn_group_stats_nhwc(x, prebias, part, b, HW, G, nchunk, eps, stat);
  __syncthreads();
  float sc[8], sh[8];
  gn_scale_shift(gamma, beta, prebias, g, stat[0][g], stat[1][g], sc, sh);
  const int p1 = min(HW, (chunk + 1) * per);
  for (int p = chunk * per + pl; p < p1; p += npl) {
    const long off = ((long)b * HW + p) * C + g * 8;
    float v[8];
    V8<T>::ld(x + off, v);
#pragma unroll
    for (int i = 0; i < 8; ++i) { v[i] = fmaf(v[i], sc[i], sh[i]); if (relu) v[i] = fmaxf(v[i], 0.f); }
    V8<OutT>::st(out + off, v);
  }
}

// ---- NHWC in, NCHW out (channels_last = 2): the normalised map leaves pixel-fastest -- the operand layout of the mask contraction
// (hipie_mask_einsum) -- without the 2 x (B, C, HW) transposing copy that followed the channels-last pass.  A workgroup owns 64 pixels of
// one image: the channels-last rows are read as the plain kernel reads them, the normalised values cross an LDS tile [channel][pixel]
// and leave as 256-byte runs of one channel.  HW % 64 == 0.
constexpr int GN_TP = 64;             // pixels per tile
template <typename T, typename OutT>
__global__ __launch_bounds__(256) void gn_apply_nhwc_to_nchw_kernel(const T* __restrict__ x, const float* __restrict__ prebias,
                                                                    const float* __restrict__ part, const float* __restrict__ gamma,
                                                                    const float* __restrict__ beta, OutT* __restrict__ out, int HW, int G,
                                                                    int nchunk, float eps, int relu) {
  extern __shared__ __attribute__((aligned(16))) float gn_tile[];      // [C][GN_TP + 1]
  __shared__ float stat[2][64];
  const int b = blockIdx.y, p0 = blockIdx.x * GN_TP;
  const int g = threadIdx.x % G, pl = threadIdx.x / G, npl = 256 / G;
  const int C = G * GN_CPG;
  if (threadIdx.x < G) gn_group_stats_nhwc(x, prebias, part, b, HW, G, nchunk, eps, stat);
  __syncthreads();
  float sc[8], sh[8];
  gn_scale_shift(gamma, beta, prebias, g, stat[0][g], stat[1][g], sc, sh);
  for (int p = pl; p < GN_TP; p += npl) {
    float v[8];
    V8<T>::ld(x + ((long)b * HW + p0 + p) * C + g * 8, v);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      v[i] = fmaf(v[i], sc[i], sh[i]);
      if (relu) v[i] = fmaxf(v[i], 0.f);
      gn_tile[(g * 8 + i) * (GN_TP + 1) + p] = v[i];
    }
  }
  __syncthreads();
  struct alignas(sizeof(OutT) * 4) Pack { OutT v[4]; };
  const int q = threadIdx.x & 15, cr = threadIdx.x >> 4;                 // 16 threads x 4 pixels = one channel's 64 pixels; 16 channels per pass
  for (int c = cr; c < C; c += 16) {
    Pack o;
#pragma unroll
    for (int i = 0; i < 4; ++i) o.v[i] = elem<OutT>::from_f32(gn_tile[c * (GN_TP + 1) + 4 * q + i]);
    *reinterpret_cast<Pack*>(out + ((long)b * C + c) * HW + p0 + 4 * q) = o;
  }
}

// ---- NCHW: x (B, C, HW).  one block per (chunk, image * channel); 8 elements per thread per step ----
template <typename T>
__global__ __launch_bounds__(256) void gn_stats_nchw_kernel(const T* __restrict__ x, const float* __restrict__ prebias,
                                                            float* __restrict__ part, int HW, int C, int nchunk, int per) {
  __shared__ float red[2][4];
  const int bc = blockIdx.y, chunk = blockIdx.x;
  const int c = bc % C, b = bc / C;
  const float pb = prebias ? prebias[c] : 0.f;
  const T* xp = x + (long)bc * HW;
  const int e1 = min(HW, (chunk + 1) * per);
  const int c0 = (c / GN_CPG) * GN_CPG;                                  // the group's shift: the first value of its first channel
  const float K = (float)x[((long)b * C + c0) * HW] + (prebias ? prebias[c0] : 0.f);
  float s = 0.f, ss = 0.f;
  for (int e = chunk * per + threadIdx.x * 8; e < e1; e += 256 * 8) {
    float v[8];
    V8<T>::ld(xp + e, v);
#pragma unroll
    for (int i = 0; i < 8; ++i) { const float a = v[i] + pb - K; s += a; ss = fmaf(a, a, ss); }
  }
  s = wave_sum(s);
  ss = wave_sum(ss);
  if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = s; red[1][threadIdx.x >> 6] = ss; }
  __syncthreads();
  if (threadIdx.x == 0) {
    const int G = C / GN_CPG, g = c / GN_CPG, K = nchunk * GN_CPG;
    float* o = part + (((long)b * G + g) * K + (c % GN_CPG) * nchunk + chunk) * 2;
    o[0] = red[0][0] + red[0][1] + red[0][2] + red[0][3];
    o[1] = red[1][0] + red[1][1] + red[1][2] + red[1][3];
  }
}

template <typename T, typename OutT>
__global__ __launch_bounds__(256) void gn_apply_nchw_kernel(const T* __restrict__ x, const float* __restrict__ prebias,
                                                            const float* __restrict__ part, const float* __restrict__ gamma,
                                                            const float* __restrict__ beta, OutT* __restrict__ out, int HW, int C,
                                                            int nchunk, int per, float eps, int relu) {
  __shared__ float stat[2];
  const int bc = blockIdx.y, chunk = blockIdx.x;
  const int c = bc % C, b = bc / C;
  if (threadIdx.x < 64) {
    const int G = C / GN_CPG, g = c / GN_CPG, K = nchunk * GN_CPG;
    const float* pp = part + ((long)b * G + g) * K * 2;
    float s = 0.f, ss = 0.f;
    for (int k = threadIdx.x; k < K; k += 64) { s += pp[2 * k]; ss += pp[2 * k + 1]; }
    s = wave_sum(s);
    ss = wave_sum(ss);
    if (threadIdx.x == 0) {
      const int c0 = g * GN_CPG;
      const float K = (float)x[((long)b * C + c0) * HW] + (prebias ? prebias[c0] : 0.f);
      gn_mean_rstd(s, ss, (float)HW * GN_CPG, K, eps, stat[0], stat[1]);
    }
  }
  __syncthreads();
  const float sc = stat[1] * gamma[c];
  const float sh = beta[c] + ((prebias ? prebias[c] : 0.f) - stat[0]) * sc;
  const T* xp = x + (long)bc * HW;
  OutT* op = out + (long)bc * HW;
  const int e1 = min(HW, (chunk + 1) * per);
  for (int e = chunk * per + threadIdx.x * 8; e < e1; e += 256 * 8) {
    float v[8];
    V8<T>::ld(xp + e, v);
#pragma unroll
    for (int i = 0; i < 8; ++i) { v[i] = fmaf(v[i], sc, sh); if (relu) v[i] = fmaxf(v[i], 0.f); }
    V8<OutT>::st(op + e, v);
  }
}

// NCHW, the training forward: stat (B, G, 2) = the (mean, rstd) of every (image, group).  One wave per (image, group) runs the statements
// of wave 0 of gn_apply_nchw_kernel on the same partials -- the same additions in the same order, so the bits the apply pass normalised with.
template <typename T>
__global__ __launch_bounds__(64) void gn_stat_nchw_kernel(const T* __restrict__ x, const float* __restrict__ part, float* __restrict__ stat_out,
                                                          int HW, int C, int nchunk, float eps) {
  const int G = C / GN_CPG, g = blockIdx.x % G, b = blockIdx.x / G, K = nchunk * GN_CPG;
  const float* pp = part + ((long)b * G + g) * K * 2;
  float s = 0.f, ss = 0.f;
  for (int k = threadIdx.x; k < K; k += 64) { s += pp[2 * k]; ss += pp[2 * k + 1]; }
  s = wave_sum(s);
  ss = wave_sum(ss);
  if (threadIdx.x == 0) {
    const float K0 = (float)x[((long)b * C + g * GN_CPG) * HW];
    float mean, rstd;
    gn_mean_rstd(s, ss, (float)HW * GN_CPG, K0, eps, mean, rstd);
    stat_out[(long)blockIdx.x * 2] = mean;
    stat_out[(long)blockIdx.x * 2 + 1] = rstd;
  }
}

template <typename T, typename OutT>
static int launch_gn(const void* x, const float* prebias, const float* gamma, const float* beta, void* out, float* part, int B,
                     int C, int HW, int nhwc, float eps, int relu, hipStream_t st) {
  const int G = C / GN_CPG;
  if (nhwc) {
    const int npl = 256 / G;
    int nchunk = max(1, min(64, HW / (npl * 16)));
    const int per = (HW + nchunk - 1) / nchunk;
    nchunk = (HW + per - 1) / per;
    hipLaunchKernelGGL((gn_stats_nhwc_kernel<T>), dim3(nchunk, B), dim3(256), 0, st, (const T*)x, prebias, part, HW, G, nchunk, per);
    if (nhwc == 2) {                         // channels-last in, NCHW out
      const size_t lds = (size_t)C * (GN_TP + 1) * sizeof(float);
      auto kern = gn_apply_nhwc_to_nchw_kernel<T, OutT>;
      static LdsLimit limit;
      limit.raise((const void*)kern, lds);
      hipLaunchKernelGGL(kern, dim3(HW / GN_TP, B), dim3(256), lds, st, (const T*)x, prebias, part, gamma, beta, (OutT*)out, HW, G, nchunk,
                         eps, relu);
      return check_launch("group_norm");
    }
    hipLaunchKernelGGL((gn_apply_nhwc_kernel<T, OutT>), dim3(nchunk, B), dim3(256), 0, st, (const T*)x, prebias, part, gamma, beta,
                       (OutT*)out, HW, G, nchunk, per, eps, relu);
  } else {
    int nchunk, per;
    gn_nchw_chunks(HW, nchunk, per);
    hipLaunchKernelGGL((gn_stats_nchw_kernel<T>), dim3(nchunk, B * C), dim3(256), 0, st, (const T*)x, prebias, part, HW, C, nchunk, per);
    hipLaunchKernelGGL((gn_apply_nchw_kernel<T, OutT>), dim3(nchunk, B * C), dim3(256), 0, st, (const T*)x, prebias, part, gamma,
                       beta, (OutT*)out, HW, C, nchunk, per, eps, relu);
  }
  return check_launch("group_norm");
}

}  // namespace hipie

extern "C" int hipie_group_norm(const void* x, const float* prebias, const float* gamma, const float* beta, void* out,
                                float* workspace, int B, int C, int HW, int groups, int channels_last, float eps, int relu,
                                int x_dtype, int out_dtype, void* stream) {
  using namespace hipie;
  HIPIE_REQUIRE(x && gamma && beta && out && workspace, "group_norm: null pointer");
  HIPIE_REQUIRE(B >= 0 && C > 0 && HW > 0, "group_norm: bad shape");
  HIPIE_REQUIRE(groups > 0 && C == groups * GN_CPG && groups <= 64 && 256 % groups == 0,
                "group_norm: %d channels in %d groups unsupported (8 channels per group, 256 %% groups == 0)", C, groups);
  HIPIE_REQUIRE(channels_last || HW % 8 == 0, "group_norm: NCHW needs H*W %% 8 == 0 (got %d)", HW);
  HIPIE_REQUIRE(channels_last >= 0 && channels_last <= 2 && (channels_last != 2 || HW % 64 == 0),
                "group_norm: channels_last %d (0 NCHW, 1 channels-last, 2 channels-last in / NCHW out: H*W %% 64 == 0, got %d)", channels_last, HW);
  if (B == 0) return HIPIE_OK;
  hipStream_t st = (hipStream_t)stream;
  return with_dtype(x_dtype, "group_norm: bad x dtype", [&](auto tx) {
    return with_dtype(out_dtype, "group_norm: bad out dtype", [&](auto to) {
      return launch_gn<decltype(tx), decltype(to)>(x, prebias, gamma, beta, out, workspace, B, C, HW, channels_last, eps, relu, st);
    });
  });
}

extern "C" int hipie_group_norm_train_forward(const float* x, const float* gamma, const float* beta, float* y, float* stat,
                                              float* workspace, int B, int C, int HW, int groups, float eps, int relu, void* stream) {
  using namespace hipie;
  HIPIE_REQUIRE(x && gamma && beta && y && stat && workspace, "group_norm_train: null pointer");
  HIPIE_REQUIRE(B >= 0 && C > 0 && HW > 0, "group_norm_train: bad shape");
  HIPIE_REQUIRE(groups > 0 && C == groups * GN_CPG && groups <= 64 && 256 % groups == 0,
                "group_norm_train: %d channels in %d groups unsupported (8 channels per group, 256 %% groups == 0)", C, groups);
  HIPIE_REQUIRE(HW % 8 == 0, "group_norm_train: NCHW needs H*W %% 8 == 0 (got %d)", HW);
  if (B == 0) return HIPIE_OK;
  hipStream_t st = (hipStream_t)stream;
  const int rc = launch_gn<float, float>(x, nullptr, gamma, beta, y, workspace, B, C, HW, 0, eps, relu, st);
  if (rc != HIPIE_OK) return rc;
  int nchunk, per;
  gn_nchw_chunks(HW, nchunk, per);
  hipLaunchKernelGGL((gn_stat_nchw_kernel<float>), dim3(B * groups), dim3(64), 0, st, x, (const float*)workspace, stat, HW, C, nchunk, eps);
  return check_launch("group_norm_train (statistics)");
}
