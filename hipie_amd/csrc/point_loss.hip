// point_loss.hip -- the element-wise losses of the training criteria (fp32), forward and backward:
//
//   point-sampled mask loss    lg = bilinear(src[n], pts[n, p]),  lab = bilinear(tgt[tgt_index[n]], pts[n, p])       (matcher.point_sample)
//                              lmask[n] = mean_p term(lg, lab)       term: mode 0 = sigmoid CE, mode 1 = focal (gamma 2, alpha)
//                              ldice[n] = 1 - (2 sum s lab + 1) / (sum s + sum lab + 1),  s = sigmoid(lg)
//   token focal loss           sum over kept (b, q, t) of focal(logits, onehot)
//
// Replaces, per criterion call of hipie_amd/training/criterion.py: the gather of the matched target masks, two grid_sample launches, the
// ~18 element-wise passes of dense_focal_loss / sigmoid_ce_loss + dice_loss and their autograd mirrors (the library grid-sampler backward
// among them); and the boolean indexing of token_focal_loss (a nonzero: a host wait for the whole queue).
//
// Point loss, forward: a workgroup of 256 threads owns PL_CHUNK points of one instance (blockIdx.x = n * splits + split); a thread adds
// its PL_CHUNK / 256 points in order, a wave adds its lanes by the xor butterfly of wave_sum, the four wave sums are added through LDS in
// wave order and written as one partial (4 floats) into the workspace (N, splits, 4); a second kernel adds an instance's partials in split
// order.  The grid is a function of (N, P) alone and nothing is atomic: bit-reproducible from call to call.
// Point loss, backward: the same grid; every point recomputes its two samples and adds its gradient to the (up to) four corners of
// d_src[n] it read with fp32 hardware atomics -- as the library's grid-sampler backward and hipie_msda_backward do.  Nothing of size N x P
// is stored between the two.  d_src is zeroed here.  The order of the additions is not fixed: NOT bit-reproducible.  (A wave whose lanes
// all hit one element adds its sum once: add_corner.)
// Offsets inside one map are 32-bit (H * W < 2^31, checked); the base of instance n is 64-bit.
#include "common.h"
#include "point_sample.h"
#include "wave.h"

namespace hipie {

constexpr int PL_THREADS = 256;
constexpr int PL_CHUNK = 1024;               // points per workgroup: 4 per thread
constexpr int TF_MAX_WG = 1024;              // workgroups (= partial sums) of the token focal forward: 4 per thread of the second stage
constexpr int TF_PER_WG = 1024;              // elements per workgroup before the grid stops growing

// ---- the element-wise terms (Sigmoid, sigmoid_parts and the bilinear sample: point_sample.h) ---------------------------------------------
// binary_cross_entropy_with_logits(x, t) in the stable softplus form, t in [0, 1]
__device__ __forceinline__ float ce_value(float x, float t, const Sigmoid& s) { return fmaxf(x, 0.f) - x * t + s.l1p; }

// FOCAL: criterion._focal with gamma = 2: ce * (1 - p_t)^2 [* (alpha t + (1 - alpha)(1 - t)) when alpha >= 0], 1 - p_t = p (1 - t) + (1 - p) t
template <bool FOCAL>
__device__ __forceinline__ float term_value(float x, float t, const Sigmoid& s, float alpha) {
  const float ce = ce_value(x, t, s);
  if (!FOCAL) return ce;
  const float u = s.p * (1.f - t) + s.q * t;
  const float at = alpha >= 0.f ? alpha * t + (1.f - alpha) * (1.f - t) : 1.f;
  return at * (ce * (u * u));
}

// d term / d x.  d ce / d x = p - t, written p (1 - t) - (1 - p) t;  d (1 - p_t) / d x = p (1 - p) (1 - 2 t)
template <bool FOCAL>
__device__ __forceinline__ float term_grad(float x, float t, const Sigmoid& s, float alpha) {
  const float dce = s.p * (1.f - t) - s.q * t;
  if (!FOCAL) return dce;
  const float ce = ce_value(x, t, s);
  const float u = s.p * (1.f - t) + s.q * t;
  const float at = alpha >= 0.f ? alpha * t + (1.f - alpha) * (1.f - t) : 1.f;
  return at * (dce * (u * u) + 2.f * ce * u * (s.p * s.q) * (1.f - 2.f * t));
}

// ---- sums over a workgroup, in a fixed order ---------------------------------------------------------------------------------------------
// v[0..K) summed over the 256 threads: butterfly inside a wave, the four waves in order through LDS.  The result is valid in thread 0.
template <int K>
__device__ __forceinline__ void block_sum(float (&v)[K], float (*red)[K]) {
#pragma unroll
  for (int k = 0; k < K; ++k) v[k] = wave_sum(v[k]);
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < K; ++k) red[wave][k] = v[k];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 0; k < K; ++k) {
      float t = red[0][k];
#pragma unroll
      for (int w = 1; w < PL_THREADS / 64; ++w) t += red[w][k];
      v[k] = t;
    }
  }
}

// ---- point-sampled mask loss -------------------------------------------------------------------------------------------------------------
struct PointLossArgs {
  const float* src;                          // (N, H, W)
  const float* tgt;                          // (T, Ht, Wt)
  const int64_t* tgt_index;                  // (N): row of tgt; a value outside [0, T) reads as an all-zero target
  const float* pts;                          // (N, P, 2): (x, y)
  int H, W, Ht, Wt, P, splits;
  int64_t T;
  float alpha;
};

// the maps of the instance a workgroup works on; tgt == nullptr: all-zero target
struct Instance {
  long n;
  int split;
  const float* src;
  const float* tgt;
  const float* pts;
};

__device__ __forceinline__ Instance instance_of(const PointLossArgs& a) {
  Instance i;
  i.n = blockIdx.x / a.splits;
  i.split = blockIdx.x % a.splits;
  i.src = a.src + i.n * ((long)a.H * a.W);
  const int64_t row = a.tgt_index[i.n];
  i.tgt = row >= 0 && row < a.T ? a.tgt + row * ((long)a.Ht * a.Wt) : nullptr;
  i.pts = a.pts + i.n * ((long)a.P * 2);
  return i;
}

// ws (N, splits, 4): sum term, sum s lab, sum s, sum lab over the workgroup's points
template <bool FOCAL>
__global__ __launch_bounds__(PL_THREADS) void point_loss_forward_kernel(const PointLossArgs a, float* __restrict__ ws) {
  __shared__ float red[PL_THREADS / 64][4];
  const Instance in = instance_of(a);
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int k = 0; k < PL_CHUNK / PL_THREADS; ++k) {
    const int p = in.split * PL_CHUNK + k * PL_THREADS + threadIdx.x;
    if (p < a.P) {
      const float x = in.pts[2 * p], y = in.pts[2 * p + 1];
      const float lg = sample(in.src, corners_of(x, y, a.H, a.W));
      const float lab = in.tgt ? sample(in.tgt, corners_of(x, y, a.Ht, a.Wt)) : 0.f;
      const Sigmoid s = sigmoid_parts(lg);
      acc[0] += term_value<FOCAL>(lg, lab, s, a.alpha);
      acc[1] += s.p * lab;
      acc[2] += s.p;
      acc[3] += lab;
    }
  }
  block_sum<4>(acc, red);
  if (threadIdx.x == 0) {
    float* o = ws + (long)blockIdx.x * 4;
    o[0] = acc[0]; o[1] = acc[1]; o[2] = acc[2]; o[3] = acc[3];
  }
}

// one thread per instance: its partials in split order -> lmask, ldice, sums (N, 3)
__global__ __launch_bounds__(PL_THREADS) void point_loss_finish_kernel(const float* __restrict__ ws, float* __restrict__ lmask,
                                                                       float* __restrict__ ldice, float* __restrict__ sums, long N, int splits,
                                                                       int P) {
  const long n = (long)blockIdx.x * PL_THREADS + threadIdx.x;
  if (n >= N) return;
  const float* w = ws + n * splits * 4;
  float t[4] = {w[0], w[1], w[2], w[3]};
  for (int s = 1; s < splits; ++s) {
#pragma unroll
    for (int k = 0; k < 4; ++k) t[k] += w[s * 4 + k];
  }
  lmask[n] = t[0] / (float)P;
  ldice[n] = 1.f - (2.f * t[1] + 1.f) / (t[2] + t[3] + 1.f);
  sums[n * 3 + 0] = t[1];
  sums[n * 3 + 1] = t[2];
  sums[n * 3 + 2] = t[3];
}

// d[off] += v for the lanes with v != 0, called by the whole wave.  When all of them hit ONE element (a map of a few pixels: every point
// reads the same corner) the wave adds its sum once: 64 atomics on one address would be served one after the other, and their fp32 running
// sum would lose what the butterfly keeps.
__device__ __forceinline__ void add_corner(float* d, int off, float v) {
  const unsigned long long live = __ballot(v != 0.f);
  if (live == 0) return;
  const int lead = __ffsll((long long)live) - 1;
  const int first = __shfl(off, lead);
  if (__all(v == 0.f || off == first)) {
    const float t = wave_sum(v);
    if ((int)(threadIdx.x & 63) == lead) unsafeAtomicAdd(d + first, t);
  } else if (v != 0.f) {
    unsafeAtomicAdd(d + off, v);             // hardware L2 atomic (global_atomic_add_f32), not a CAS loop
  }
}

// d loss / d lg of one point = g_mask / P * term' + g_dice * d ldice / d s * s (1 - s), with A = sum s lab, D = sum s + sum lab + 1:
//   d ldice / d s_p = -(2 lab_p D - (2 A + 1)) / D^2
// MERGE = false: one atomic per lane and corner, no add_corner (study builds only: the A/B of tools/bench_point_loss.py)
template <bool FOCAL, bool MERGE>
__global__ __launch_bounds__(PL_THREADS) void point_loss_backward_kernel(const PointLossArgs a, const float* __restrict__ sums,
                                                                         const float* __restrict__ g_mask, const float* __restrict__ g_dice,
                                                                         float* __restrict__ d_src) {
  const Instance in = instance_of(a);
  const float gm = g_mask[in.n] / (float)a.P, gd = g_dice[in.n];
  const float A = sums[in.n * 3], D = sums[in.n * 3 + 1] + sums[in.n * 3 + 2] + 1.f;
  const float c1 = -2.f * gd / D, c0 = gd * (2.f * A + 1.f) / (D * D);
  float* d = d_src + in.n * ((long)a.H * a.W);
#pragma unroll
  for (int k = 0; k < PL_CHUNK / PL_THREADS; ++k) {
    const int p = in.split * PL_CHUNK + k * PL_THREADS + threadIdx.x;
    Corners c = {};
    float g = 0.f;                           // a lane past P adds nothing
    if (p < a.P) {
      const float x = in.pts[2 * p], y = in.pts[2 * p + 1];
      c = corners_of(x, y, a.H, a.W);
      const float lg = sample(in.src, c);
      const float lab = in.tgt ? sample(in.tgt, corners_of(x, y, a.Ht, a.Wt)) : 0.f;
      const Sigmoid s = sigmoid_parts(lg);
      g = gm * term_grad<FOCAL>(lg, lab, s, a.alpha) + (c1 * lab + c0) * (s.p * s.q);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float v = g != 0.f ? c.w[j] * g : 0.f;
      if (MERGE) add_corner(d, v != 0.f ? c.off[j] : 0, v);
      else if (v != 0.f) unsafeAtomicAdd(d + c.off[j], v);
    }
  }
}

static inline int point_loss_splits(int P) { return P > 0 ? (P + PL_CHUNK - 1) / PL_CHUNK : 1; }

// the checks the two entry points share; fills `a`
static int point_loss_check(const char* who, PointLossArgs& a, const float* src, const float* tgt, const int64_t* tgt_index, const float* pts,
                            int64_t N, int H, int W, int64_t T, int Ht, int Wt, int P, int mode, float alpha, float gamma) {
  HIPIE_REQUIRE(mode == 0 || mode == 1, "%s: mode=%d must be 0 (sigmoid CE) or 1 (focal)", who, mode);
  HIPIE_REQUIRE(gamma == 2.f, "%s: gamma=%g: only the focal exponent 2 is built", who, (double)gamma);
  HIPIE_REQUIRE(N >= 0 && T >= 0 && H >= 0 && W >= 0 && Ht >= 0 && Wt >= 0, "%s: negative size", who);
  if (N == 0) return HIPIE_OK;
  HIPIE_REQUIRE(P > 0, "%s: P=%d points for N=%lld instances", who, P, (long long)N);
  HIPIE_REQUIRE(H > 0 && W > 0 && (int64_t)H * W < (1ll << 31), "%s: H*W=%lld must be in [1, 2^31) (32-bit offsets inside a map)", who,
                (long long)H * W);
  HIPIE_REQUIRE(T == 0 || (Ht > 0 && Wt > 0 && (int64_t)Ht * Wt < (1ll << 31)),
                "%s: Ht*Wt=%lld must be in [1, 2^31) (32-bit offsets inside a map)", who, (long long)Ht * Wt);
  HIPIE_REQUIRE(N * point_loss_splits(P) < (1ll << 31), "%s: N=%lld x %d point chunks exceed the grid", who, (long long)N, point_loss_splits(P));
  HIPIE_REQUIRE(src && tgt_index && pts && (tgt || T == 0), "%s: null pointer", who);
  a.src = src; a.tgt = tgt; a.tgt_index = tgt_index; a.pts = pts;
  a.H = H; a.W = W; a.Ht = Ht; a.Wt = Wt; a.P = P; a.splits = point_loss_splits(P);
  a.T = T; a.alpha = alpha;
  return HIPIE_OK;
}

// ---- token focal loss ----------------------------------------------------------------------------------------------------------------------
struct TokenFocalArgs {
  const float* logits;                       // (B, Q, T)
  const float* onehot;                       // (B, Q, T)
  const uint8_t* keep;                       // (B, T) or nullptr: token t of image b counts when keep[b, t] != 0
  long n, QT;                                // B * Q * T, Q * T
  int T;
  float alpha;
};

__device__ __forceinline__ bool token_kept(const TokenFocalArgs& a, long i) {
  return a.keep == nullptr || a.keep[(i / a.QT) * a.T + i % a.T] != 0;
}

__global__ __launch_bounds__(PL_THREADS) void token_focal_forward_kernel(const TokenFocalArgs a, float* __restrict__ ws) {
  __shared__ float red[PL_THREADS / 64][1];
  float acc[1] = {0.f};
  for (long i = (long)blockIdx.x * PL_THREADS + threadIdx.x; i < a.n; i += (long)gridDim.x * PL_THREADS) {
    if (token_kept(a, i)) {
      const float x = a.logits[i];
      acc[0] += term_value<true>(x, a.onehot[i], sigmoid_parts(x), a.alpha);
    }
  }
  block_sum<1>(acc, red);
  if (threadIdx.x == 0) ws[blockIdx.x] = acc[0];
}

// one workgroup: thread t adds the partials t, t + 256, ... in order, then the workgroup sum
__global__ __launch_bounds__(PL_THREADS) void token_focal_finish_kernel(const float* __restrict__ ws, float* __restrict__ out, int parts) {
  __shared__ float red[PL_THREADS / 64][1];
  float acc[1] = {0.f};
  for (int i = threadIdx.x; i < parts; i += PL_THREADS) acc[0] += ws[i];
  block_sum<1>(acc, red);
  if (threadIdx.x == 0) out[0] = acc[0];
}

__global__ __launch_bounds__(PL_THREADS) void token_focal_backward_kernel(const TokenFocalArgs a, const float* __restrict__ g,
                                                                          float* __restrict__ dlogits) {
  const float go = g[0];
  for (long i = (long)blockIdx.x * PL_THREADS + threadIdx.x; i < a.n; i += (long)gridDim.x * PL_THREADS) {
    float d = 0.f;                           // a dropped token: exactly 0, whatever g holds
    if (token_kept(a, i)) {
      const float x = a.logits[i];
      d = go * term_grad<true>(x, a.onehot[i], sigmoid_parts(x), a.alpha);
    }
    dlogits[i] = d;
  }
}

static inline int token_focal_parts(int64_t n) {
  const int64_t want = (n + TF_PER_WG - 1) / TF_PER_WG;
  return (int)(want < 1 ? 1 : want < TF_MAX_WG ? want : TF_MAX_WG);
}

static int token_focal_check(const char* who, TokenFocalArgs& a, const float* logits, const float* onehot, const uint8_t* keep, int B, int Q, int T,
                             float alpha, float gamma) {
  HIPIE_REQUIRE(gamma == 2.f, "%s: gamma=%g: only the focal exponent 2 is built", who, (double)gamma);
  HIPIE_REQUIRE(B >= 0 && Q >= 0 && T >= 0, "%s: negative size", who);
  a.n = (long)B * Q * T;
  if (a.n == 0) return HIPIE_OK;
  HIPIE_REQUIRE(logits && onehot, "%s: null pointer", who);
  a.logits = logits; a.onehot = onehot; a.keep = keep;
  a.QT = (long)Q * T; a.T = T; a.alpha = alpha;
  return HIPIE_OK;
}

}  // namespace hipie

extern "C" int64_t hipie_point_mask_loss_ws_bytes(int64_t N, int P) {
  if (N <= 0 || P <= 0) return 16;
  return N * hipie::point_loss_splits(P) * 4 * (int64_t)sizeof(float);
}

extern "C" int hipie_point_mask_loss_forward(const float* src, const float* tgt, const int64_t* tgt_index, const float* pts, float* lmask,
                                             float* ldice, float* sums, void* ws, int64_t ws_bytes, int64_t N, int H, int W, int64_t T, int Ht,
                                             int Wt, int P, int mode, float alpha, float gamma, void* stream) {
  using namespace hipie;
  PointLossArgs a;
  HIPIE_TRY(point_loss_check("point_mask_loss_forward", a, src, tgt, tgt_index, pts, N, H, W, T, Ht, Wt, P, mode, alpha, gamma));
  if (N == 0) return HIPIE_OK;
  HIPIE_REQUIRE(lmask && ldice && sums && ws, "point_mask_loss_forward: null pointer");
  HIPIE_REQUIRE(ws_bytes >= hipie_point_mask_loss_ws_bytes(N, P), "point_mask_loss_forward: workspace of %lld bytes, %lld needed",
                (long long)ws_bytes, (long long)hipie_point_mask_loss_ws_bytes(N, P));
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)(N * a.splits));
  if (mode == 1) hipLaunchKernelGGL(point_loss_forward_kernel<true>, grid, dim3(PL_THREADS), 0, st, a, (float*)ws);
  else hipLaunchKernelGGL(point_loss_forward_kernel<false>, grid, dim3(PL_THREADS), 0, st, a, (float*)ws);
  HIPIE_TRY(check_launch("point_mask_loss_forward"));
  hipLaunchKernelGGL(point_loss_finish_kernel, dim3((unsigned)((N + PL_THREADS - 1) / PL_THREADS)), dim3(PL_THREADS), 0, st, (const float*)ws,
                     lmask, ldice, sums, (long)N, a.splits, P);
  return check_launch("point_mask_loss_forward (partial sum)");
}

extern "C" int hipie_point_mask_loss_backward(const float* src, const float* tgt, const int64_t* tgt_index, const float* pts, const float* sums,
                                              const float* g_mask, const float* g_dice, float* d_src, int64_t N, int H, int W, int64_t T, int Ht,
                                              int Wt, int P, int mode, float alpha, float gamma, void* stream) {
  using namespace hipie;
  PointLossArgs a;
  HIPIE_TRY(point_loss_check("point_mask_loss_backward", a, src, tgt, tgt_index, pts, N, H, W, T, Ht, Wt, P, mode, alpha, gamma));
  if (N == 0) return HIPIE_OK;
  HIPIE_REQUIRE(sums && g_mask && g_dice && d_src, "point_mask_loss_backward: null pointer");
  HIPIE_REQUIRE((const float*)d_src != src, "point_mask_loss_backward: d_src must not alias src");
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(d_src, 0, (size_t)N * H * W * sizeof(float), st) != hipSuccess) return check_launch("point_mask_loss_backward (zero fill)");
  const dim3 grid((unsigned)(N * a.splits));
  auto kernel = mode == 1 ? point_loss_backward_kernel<true, true> : point_loss_backward_kernel<false, true>;
  if (study_env("HIPIE_POINT_LOSS_PLAIN")) kernel = mode == 1 ? point_loss_backward_kernel<true, false> : point_loss_backward_kernel<false, false>;
  hipLaunchKernelGGL(kernel, grid, dim3(PL_THREADS), 0, st, a, sums, g_mask, g_dice, d_src);
  return check_launch("point_mask_loss_backward");
}

extern "C" int64_t hipie_token_focal_ws_bytes(int64_t n) {
  const int64_t b = (int64_t)hipie::token_focal_parts(n) * (int64_t)sizeof(float);
  return b < 16 ? 16 : b;
}

extern "C" int hipie_token_focal_forward(const float* logits, const float* onehot, const uint8_t* keep, float* out, void* ws, int64_t ws_bytes, int B,
                                         int Q, int T, float alpha, float gamma, void* stream) {
  using namespace hipie;
  TokenFocalArgs a;
  HIPIE_TRY(token_focal_check("token_focal_forward", a, logits, onehot, keep, B, Q, T, alpha, gamma));
  hipStream_t st = (hipStream_t)stream;
  if (a.n == 0) return HIPIE_OK;             // nothing is written: the caller's sum over nothing
  HIPIE_REQUIRE(out && ws, "token_focal_forward: null pointer");
  HIPIE_REQUIRE(ws_bytes >= hipie_token_focal_ws_bytes(a.n), "token_focal_forward: workspace of %lld bytes, %lld needed", (long long)ws_bytes,
                (long long)hipie_token_focal_ws_bytes(a.n));
  const int parts = token_focal_parts(a.n);
  hipLaunchKernelGGL(token_focal_forward_kernel, dim3((unsigned)parts), dim3(PL_THREADS), 0, st, a, (float*)ws);
  HIPIE_TRY(check_launch("token_focal_forward"));
  hipLaunchKernelGGL(token_focal_finish_kernel, dim3(1), dim3(PL_THREADS), 0, st, (const float*)ws, out, parts);
  return check_launch("token_focal_forward (partial sum)");
}

extern "C" int hipie_token_focal_backward(const float* logits, const float* onehot, const uint8_t* keep, const float* g, float* dlogits, int B, int Q,
                                          int T, float alpha, float gamma, void* stream) {
  using namespace hipie;
  TokenFocalArgs a;
  HIPIE_TRY(token_focal_check("token_focal_backward", a, logits, onehot, keep, B, Q, T, alpha, gamma));
  if (a.n == 0) return HIPIE_OK;
  HIPIE_REQUIRE(g && dlogits, "token_focal_backward: null pointer");
  const int64_t want = (a.n + PL_THREADS - 1) / PL_THREADS;
  const dim3 grid((unsigned)(want < (1 << 20) ? want : (1 << 20)));
  hipLaunchKernelGGL(token_focal_backward_kernel, grid, dim3(PL_THREADS), 0, (hipStream_t)stream, a, g, dlogits);
  return check_launch("token_focal_backward");
}
