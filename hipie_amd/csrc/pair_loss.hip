// pair_loss.hip -- what the training criteria do with the matched (query, target) pairs of one call, forward and backward:
//
//   box losses      loss_bbox, loss_giou [, loss_boxiou] of criterion.DetCriterion.loss_boxes (mode 0) and criterion.MaskCriterion.loss_boxes
//                   (mode 1) as FINAL scalars -- normalised and re-weighted here, the criterion adds no scalar arithmetic
//   positive one-hot  onehot[b, q_i] = pos_map[b, t_i] of criterion._positive_onehot: a zero fill and one scatter
//
// Replaces, per loss_boxes call: the index gathers, about a hundred element-wise launches with their autograd mirrors, and one host wait
// (`thing.sum() == 0` / the degenerate-box check of boxes.generalized_box_iou as Python bools).
//
// The pairs arrive as the matchers leave them: per image two int64 device arrays.  Their addresses and the images' first pair sit in the
// kernel arguments (PairList, B <= 64): no index tensor is built, nothing is copied to the device per call.
//
// mode 0   L1 and boxes.paired_giou_loss (the intersection counts only where the boxes overlap, 1e-7 in both quotients), each pair weighted
//          by is_thing[b, t] (or 1), reweight = K / (sum weights + 1e-6); loss_boxiou = mean(BCE_with_logits(score, paired IoU) * weight) *
//          reweight, the IoU target without gradient.  No "no thing among the pairs" branch: every masked sum is then exactly 0, and so are
//          the three losses and every gradient (reweight is finite: K / 1e-6) -- what the criterion's branch returns.
// mode 1   L1 and 1 - boxes.generalized_box_iou (each extent clamped at 0, 1e-7 in the hull quotient only: match_cost.h's box_pair); with
//          is_thing the stuff pairs are left out (a filter: they are not even evaluated), no re-weighting.  A box with x1 < x0 or y1 < y0 (or
//          a NaN) among the evaluated pairs sets bit 1 of the status word -- the ValueError of the torch path, raised by whoever reads it.
// Ties of max / min follow torch.maximum / torch.minimum (half the gradient to each side), |x| has gradient 0 at 0, clamp(min=0) passes the
// gradient at exactly 0 (torch.clamp) -- src == tgt is a case users construct.
//
// Arithmetic: the inputs are fp32; a pair is evaluated in fp64 (a few hundred pairs per call: the kernels are launch-bound) and rounded once.
// Forward: a workgroup of 256 threads owns 256 pairs, wave_sum per wave, the four waves in order through LDS, one partial row (4 doubles)
// per workgroup in the workspace; ONE finishing workgroup adds the rows in the order of row_norm.h's partial_rows_column and forms the
// scalars.  No atomics: bit-reproducible.  The per-pair gradients are stored (K, 9) for the backward.
// Backward: d_boxes / d_iou are zero-filled and every pair adds its scaled gradient with a global fp32 atomic: duplicates of an (image, query)
// sum; with one target per (image, query) -- what every matcher yields -- each element receives one addition and the result is bit-reproducible.
#include "common.h"
#include "match_cost.h"
#include "row_norm.h"
#include "wave.h"

namespace hipie {

constexpr int PB_THREADS = 256;              // pairs per workgroup
constexpr int PB_GROUPS = 64, PB_COLS = 4;   // the finisher: 64 partial rows per pass over 4 columns
constexpr int PB_MAX_B = 64;                 // images whose pair lists fit the kernel arguments
constexpr int PB_MAX_K = 65536;              // pairs per call
constexpr int PB_GRAD = 9;                   // stored per pair: d L1 (4), d GIoU loss (4), d BCE (1), weighted
constexpr int OH_THREADS = 128;

constexpr unsigned PB_ST_BOX = 1u;           // a degenerate box (mode 1)
constexpr unsigned PB_ST_INDEX = 2u;         // a query or target index out of range: the pair is left out

// the pair lists of a batch, by value in the kernel arguments
struct PairList {
  const int64_t* q[PB_MAX_B];
  const int64_t* t[PB_MAX_B];
  int start[PB_MAX_B + 1];                   // first pair of image b; start[B] = K
  int B;
};

struct Pair {
  int b;
  int64_t q, t;
};

// pair k of the batch: a wave-uniform scan of at most 64 boundaries
__device__ __forceinline__ Pair pair_of(const PairList& pl, int k, bool with_t) {
  int b = 0;
  while (b + 1 < pl.B && k >= pl.start[b + 1]) ++b;
  Pair p;
  p.b = b;
  p.q = pl.q[b][k - pl.start[b]];
  p.t = with_t ? pl.t[b][k - pl.start[b]] : 0;
  return p;
}

struct PairArgs {
  const float* boxes;                        // (B, Q, 4) cxcywh by strides (in elements), the 4 coordinates dense
  long bs_b, bs_q;
  const float* iou;                          // (B, Q) logits by strides, or nullptr
  long is_b, is_q;
  const float* tgt_boxes;                    // (B, Tmax, 4)
  const uint8_t* is_thing;                   // (B, Tmax), or nullptr: every pair counts
  int Q, Tmax, K;
  double count;
};

// d max(a, b) / d a and d min(a, b) / d a as torch.maximum / torch.minimum define them
__device__ __forceinline__ double dmax_a(double a, double b) { return a > b ? 1.0 : a == b ? 0.5 : 0.0; }
__device__ __forceinline__ double dmin_a(double a, double b) { return a < b ? 1.0 : a == b ? 0.5 : 0.0; }

// loss = 1 - GIoU of the pair (a: prediction, b: target) and its gradient for a's corners (x0, y0, x1, y1); iou = boxes.paired_iou
// MODE 0: boxes.paired_giou_loss;  MODE 1: 1 - boxes.generalized_box_iou (the terms themselves: match_cost.h)
template <int MODE>
__device__ __forceinline__ void giou_loss_grad(const BoxCorners<double>& a, const BoxCorners<double>& b, double& loss, double& iou,
                                               double (&g)[4]) {
  const double eh = 1e-7, eu = MODE == 0 ? 1e-7 : 0.0;
  const BoxPairTerms<double> p = box_pair(a, b);
  iou = p.inter / p.uni;
  const double rw = fmin(a.x1, b.x1) - fmax(a.x0, b.x0), rh = fmin(a.y1, b.y1) - fmax(a.y0, b.y0);
  const double cw = fmax(a.x1, b.x1) - fmin(a.x0, b.x0), ch = fmax(a.y1, b.y1) - fmin(a.y0, b.y0);
  double I, U, H, iw, ih, hw, hh;
  bool on_iw, on_ih, on_hw, on_hh;           // where the extent passes its gradient
  if (MODE == 0) {
    const bool overlap = rh > 0.0 && rw > 0.0;
    iw = overlap ? rw : 0.0;
    ih = overlap ? rh : 0.0;
    on_iw = on_ih = overlap;
    hw = cw; hh = ch;
    on_hw = on_hh = true;
    I = iw * ih;
    U = (box_area(a) + box_area(b)) - I;
    H = hw * hh;
    loss = 1.0 - (I / (U + eu) - (H - U) / (H + eh));
  } else {
    iw = fmax(rw, 0.0); ih = fmax(rh, 0.0);
    hw = fmax(cw, 0.0); hh = fmax(ch, 0.0);
    on_iw = rw >= 0.0; on_ih = rh >= 0.0; on_hw = cw >= 0.0; on_hh = ch >= 0.0;
    I = p.inter;
    U = p.uni;
    H = hw * hh;
    loss = 1.0 - p.giou;
  }
  // loss = 1 - I / (U + eu) + (H - U) / (H + eh),  U = area(a) + area(b) - I
  const double dU = I / ((U + eu) * (U + eu)) - 1.0 / (H + eh);
  const double dI = -1.0 / (U + eu) - dU;
  const double dH = (U + eh) / ((H + eh) * (H + eh));
  const double d_iw = on_iw ? dI * ih : 0.0, d_ih = on_ih ? dI * iw : 0.0;
  const double d_hw = on_hw ? dH * hh : 0.0, d_hh = on_hh ? dH * hw : 0.0;
  const double wa = a.x1 - a.x0, ha = a.y1 - a.y0;
  g[0] = -d_iw * dmax_a(a.x0, b.x0) - dU * ha - d_hw * dmin_a(a.x0, b.x0);
  g[1] = -d_ih * dmax_a(a.y0, b.y0) - dU * wa - d_hh * dmin_a(a.y0, b.y0);
  g[2] = d_iw * dmin_a(a.x1, b.x1) + dU * ha + d_hw * dmax_a(a.x1, b.x1);
  g[3] = d_ih * dmin_a(a.y1, b.y1) + dU * wa + d_hh * dmax_a(a.y1, b.y1);
}

// ws: (nparts, 4) doubles -- sum w l1, sum w giou loss, sum w bce, sum w -- then nparts status words
template <int MODE>
__global__ __launch_bounds__(PB_THREADS) void pair_box_loss_forward_kernel(const PairList pl, const PairArgs a, float* __restrict__ pair_grad,
                                                                           double* __restrict__ ws, unsigned* __restrict__ ws_status) {
  __shared__ double red[PB_THREADS / 64][4];
  __shared__ unsigned red_st[PB_THREADS / 64];
  const int k = blockIdx.x * PB_THREADS + threadIdx.x;
  double v[4] = {0.0, 0.0, 0.0, 0.0};
  float pg[PB_GRAD] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  unsigned st = 0;
  if (k < a.K) {
    const Pair pr = pair_of(pl, k, true);
    if (pr.q < 0 || pr.q >= a.Q || pr.t < 0 || pr.t >= a.Tmax) {
      st = PB_ST_INDEX;
    } else {
      const double w = a.is_thing ? (a.is_thing[(long)pr.b * a.Tmax + pr.t] != 0 ? 1.0 : 0.0) : 1.0;
      if (MODE == 0 || w != 0.0) {           // mode 0 multiplies by the weight (as the criterion does), mode 1 filters
        const float* sb = a.boxes + pr.b * a.bs_b + pr.q * a.bs_q;
        const float* tb = a.tgt_boxes + ((long)pr.b * a.Tmax + pr.t) * 4;
        const BoxCorners<double> sx = box_xyxy<double>(sb), tx = box_xyxy<double>(tb);
        if (MODE == 1 && (box_degenerate(sx) || box_degenerate(tx))) st = PB_ST_BOX;
        double l1 = 0.0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const double d = (double)sb[j] - (double)tb[j];
          l1 += fabs(d);
          pg[j] = (float)(w * (d > 0.0 ? 1.0 : d < 0.0 ? -1.0 : 0.0));
        }
        double gl, iou, g[4];
        giou_loss_grad<MODE>(sx, tx, gl, iou, g);
        // x0 = cx - w / 2, x1 = cx + w / 2
        pg[4] = (float)(w * (g[0] + g[2]));
        pg[5] = (float)(w * (g[1] + g[3]));
        pg[6] = (float)(w * (0.5 * (g[2] - g[0])));
        pg[7] = (float)(w * (0.5 * (g[3] - g[1])));
        v[0] = w * l1;
        v[1] = w * gl;
        v[3] = w;
        if (MODE == 0 && a.iou) {            // binary_cross_entropy_with_logits in the softplus form; d / d x = sigmoid(x) - target
          const double x = (double)a.iou[pr.b * a.is_b + pr.q * a.is_q];
          v[2] = w * (fmax(x, 0.0) - x * iou + log1p(exp(-fabs(x))));
          pg[8] = (float)(w * (1.0 / (1.0 + exp(-x)) - iou));
        }
      }
    }
#pragma unroll
    for (int j = 0; j < PB_GRAD; ++j) pair_grad[(long)k * PB_GRAD + j] = pg[j];
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) v[j] = wave_sum(v[j]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) st |= (unsigned)__shfl_xor((int)st, o);
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int j = 0; j < 4; ++j) red[wave][j] = v[j];
    red_st[wave] = st;
  }
  __syncthreads();
  if (threadIdx.x < 4) {
    double t = red[0][threadIdx.x];
#pragma unroll
    for (int w = 1; w < PB_THREADS / 64; ++w) t += red[w][threadIdx.x];
    ws[(long)blockIdx.x * 4 + threadIdx.x] = t;
  }
  if (threadIdx.x == 0) ws_status[blockIdx.x] = red_st[0] | red_st[1] | red_st[2] | red_st[3];
}

// out: 3 floats (loss_bbox, loss_giou, loss_boxiou), one float of padding, then 2 doubles: the factors the backward multiplies the
// stored per-pair gradients by (boxes, box IoU)
__device__ __forceinline__ double* pair_scales(float* out) { return reinterpret_cast<double*>(out + 4); }
__device__ __forceinline__ const double* pair_scales(const float* out) { return reinterpret_cast<const double*>(out + 4); }

template <int MODE>
__global__ __launch_bounds__(PB_THREADS) void pair_box_loss_finish_kernel(const double* __restrict__ ws, const unsigned* __restrict__ ws_status,
                                                                          int nparts, int K, double count, float* __restrict__ out,
                                                                          int* __restrict__ status) {
  static_assert(PB_GROUPS * PB_COLS == PB_THREADS, "one thread per (group, column)");
  __shared__ double red[PB_GROUPS][PB_COLS];
  __shared__ double tot[PB_COLS];
  __shared__ unsigned red_st[PB_THREADS / 64];
  const double t = partial_rows_column<PB_GROUPS, PB_COLS, double>(ws, nparts, PB_COLS, threadIdx.x % PB_COLS, red);
  if (threadIdx.x < PB_COLS) tot[threadIdx.x] = t;
  unsigned st = 0;
  for (int p = threadIdx.x; p < nparts; p += PB_THREADS) st |= ws_status[p];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) st |= (unsigned)__shfl_xor((int)st, o);
  if ((threadIdx.x & 63) == 0) red_st[threadIdx.x >> 6] = st;
  __syncthreads();
  if (threadIdx.x == 0) {
    double s_box, s_iou;
    if (MODE == 0) {
      const double reweight = (double)K / (tot[3] + 1e-6);
      s_box = reweight / count;
      s_iou = reweight / (double)K;
    } else {
      s_box = 1.0 / count;
      s_iou = 0.0;
    }
    out[0] = (float)(tot[0] * s_box);
    out[1] = (float)(tot[1] * s_box);
    out[2] = (float)(tot[2] * s_iou);
    out[3] = 0.f;
    pair_scales(out)[0] = s_box;
    pair_scales(out)[1] = s_iou;
    status[0] = (int)(red_st[0] | red_st[1] | red_st[2] | red_st[3]);
  }
}

// d_boxes (B, Q, 4) and d_iou (B, Q) dense and zero-filled by the caller; g_*: the upstream gradients of the three scalars, on the device
__global__ __launch_bounds__(PB_THREADS) void pair_box_loss_backward_kernel(const PairList pl, int K, int Q, const float* __restrict__ out,
                                                                            const float* __restrict__ pair_grad, const float* __restrict__ g_bbox,
                                                                            const float* __restrict__ g_giou, const float* __restrict__ g_boxiou,
                                                                            float* __restrict__ d_boxes, float* __restrict__ d_iou) {
  const int k = blockIdx.x * PB_THREADS + threadIdx.x;
  if (k >= K) return;
  const Pair pr = pair_of(pl, k, false);
  if (pr.q < 0 || pr.q >= Q) return;         // the forward left the pair out and set PB_ST_INDEX
  const double* s = pair_scales(out);
  const double gb = (double)g_bbox[0] * s[0], gg = (double)g_giou[0] * s[0];
  const float* pg = pair_grad + (long)k * PB_GRAD;
  float* d = d_boxes + ((long)pr.b * Q + pr.q) * 4;
#pragma unroll
  for (int j = 0; j < 4; ++j) unsafeAtomicAdd(d + j, (float)(gb * (double)pg[j] + gg * (double)pg[4 + j]));
  if (d_iou) unsafeAtomicAdd(d_iou + (long)pr.b * Q + pr.q, (float)((double)g_boxiou[0] * s[1] * (double)pg[8]));
}

// onehot (B, Q, L) zero-filled by the caller; a workgroup per pair copies the target's row of pos_map (B, Tmax, L) as exact 0 / 1.
// A pair whose indices are out of range is left out (the torch indexing would have raised).
__global__ __launch_bounds__(OH_THREADS) void positive_onehot_kernel(const PairList pl, const uint8_t* __restrict__ pos_map,
                                                                     float* __restrict__ onehot, int Q, int Tmax, int L) {
  const Pair pr = pair_of(pl, (int)blockIdx.x, true);
  if (pr.q < 0 || pr.q >= Q || pr.t < 0 || pr.t >= Tmax) return;
  const uint8_t* src = pos_map + ((long)pr.b * Tmax + pr.t) * L;
  float* dst = onehot + ((long)pr.b * Q + pr.q) * L;
  for (int l = threadIdx.x; l < L; l += OH_THREADS) dst[l] = src[l] != 0 ? 1.f : 0.f;
}

static inline int pair_parts(int64_t K) { return K > 0 ? (int)((K + PB_THREADS - 1) / PB_THREADS) : 0; }

// the pair lists of a call from the HOST arrays of the entry points; fills pl and K.  pair_t == nullptr: the targets are not needed.
static int pair_list_check(const char* who, PairList& pl, int& K, const int64_t* const* pair_q, const int64_t* const* pair_t, bool need_t,
                           const int64_t* pair_n, int B, int Q, int Tmax) {
  HIPIE_REQUIRE(B >= 0 && Q >= 0 && Tmax >= 0, "%s: negative size", who);
  HIPIE_REQUIRE(B <= PB_MAX_B, "%s: B=%d images, the pair lists of at most %d fit the kernel arguments", who, B, PB_MAX_B);
  HIPIE_REQUIRE(B == 0 || (pair_q && pair_n && (pair_t || !need_t)), "%s: null pair list", who);
  int64_t k = 0;
  for (int b = 0; b < B; ++b) {
    HIPIE_REQUIRE(pair_n[b] >= 0, "%s: image %d has %lld pairs", who, b, (long long)pair_n[b]);
    HIPIE_REQUIRE(pair_n[b] == 0 || (pair_q[b] && (!need_t || pair_t[b])), "%s: image %d: null pair list", who, b);
    HIPIE_REQUIRE(pair_n[b] == 0 || (Q > 0 && (Tmax > 0 || !need_t)), "%s: image %d has pairs, but Q=%d, Tmax=%d", who, b, Q, Tmax);
    pl.q[b] = pair_q[b];
    pl.t[b] = need_t ? pair_t[b] : nullptr;
    pl.start[b] = (int)k;
    k += pair_n[b];
    HIPIE_REQUIRE(k <= PB_MAX_K, "%s: more than %d pairs", who, PB_MAX_K);
  }
  for (int b = B; b < PB_MAX_B; ++b) {
    pl.q[b] = pl.t[b] = nullptr;
    pl.start[b] = (int)k;
  }
  pl.start[PB_MAX_B] = (int)k;
  pl.B = B;
  K = (int)k;
  return HIPIE_OK;
}

}  // namespace hipie

extern "C" int64_t hipie_pair_box_loss_ws_bytes(int64_t K) {
  const int64_t b = (int64_t)hipie::pair_parts(K) * (4 * (int64_t)sizeof(double) + (int64_t)sizeof(unsigned));
  return b < 16 ? 16 : (b + 15) / 16 * 16;
}

extern "C" int hipie_pair_box_loss_forward(const float* boxes, int64_t box_stride_b, int64_t box_stride_q, const float* iou, int64_t iou_stride_b,
                                           int64_t iou_stride_q, const int64_t* const* pair_q, const int64_t* const* pair_t, const int64_t* pair_n,
                                           const float* tgt_boxes, const uint8_t* is_thing, float* out, float* pair_grad, int* status, void* ws,
                                           int64_t ws_bytes, int B, int Q, int Tmax, int mode, double count, void* stream) {
  using namespace hipie;
  const char* who = "pair_box_loss_forward";
  HIPIE_REQUIRE(mode == 0 || mode == 1, "%s: mode=%d must be 0 (DetCriterion) or 1 (MaskCriterion)", who, mode);
  HIPIE_REQUIRE(mode == 0 || iou == nullptr, "%s: mode 1 has no box-IoU loss", who);
  HIPIE_REQUIRE(count > 0.0 && count < 1e30, "%s: count=%g must be positive and finite", who, count);
  PairList pl;
  PairArgs a;
  HIPIE_TRY(pair_list_check(who, pl, a.K, pair_q, pair_t, true, pair_n, B, Q, Tmax));
  if (a.K == 0) return HIPIE_OK;             // nothing is written: the caller's `src.sum() * 0.0`
  HIPIE_REQUIRE(boxes && tgt_boxes && out && pair_grad && status && ws, "%s: null pointer", who);
  HIPIE_REQUIRE(box_stride_q >= 4 && box_stride_b >= 0 && (B == 1 || box_stride_b >= (int64_t)Q * box_stride_q),
                "%s: box strides (%lld, %lld) do not describe (B, Q, 4) rows", who, (long long)box_stride_b, (long long)box_stride_q);
  HIPIE_REQUIRE(!iou || (iou_stride_q >= 1 && iou_stride_b >= 0 && (B == 1 || iou_stride_b >= (int64_t)Q * iou_stride_q)),
                "%s: iou strides (%lld, %lld) do not describe (B, Q) elements", who, (long long)iou_stride_b, (long long)iou_stride_q);
  HIPIE_REQUIRE(((uintptr_t)out & 7) == 0 && ((uintptr_t)ws & 7) == 0, "%s: out and ws must be 8-byte aligned", who);
  HIPIE_REQUIRE(ws_bytes >= hipie_pair_box_loss_ws_bytes(a.K), "%s: workspace of %lld bytes, %lld needed", who, (long long)ws_bytes,
                (long long)hipie_pair_box_loss_ws_bytes(a.K));
  a.boxes = boxes; a.bs_b = (long)box_stride_b; a.bs_q = (long)box_stride_q;
  a.iou = iou; a.is_b = (long)iou_stride_b; a.is_q = (long)iou_stride_q;
  a.tgt_boxes = tgt_boxes; a.is_thing = is_thing;
  a.Q = Q; a.Tmax = Tmax; a.count = count;
  hipStream_t st = (hipStream_t)stream;
  const int nparts = pair_parts(a.K);
  double* wsd = (double*)ws;
  unsigned* wss = (unsigned*)(wsd + (long)nparts * 4);
  if (mode == 0) hipLaunchKernelGGL(pair_box_loss_forward_kernel<0>, dim3((unsigned)nparts), dim3(PB_THREADS), 0, st, pl, a, pair_grad, wsd, wss);
  else hipLaunchKernelGGL(pair_box_loss_forward_kernel<1>, dim3((unsigned)nparts), dim3(PB_THREADS), 0, st, pl, a, pair_grad, wsd, wss);
  HIPIE_TRY(check_launch(who));
  if (mode == 0) hipLaunchKernelGGL(pair_box_loss_finish_kernel<0>, dim3(1), dim3(PB_THREADS), 0, st, (const double*)wsd, (const unsigned*)wss, nparts,
                                    a.K, count, out, status);
  else hipLaunchKernelGGL(pair_box_loss_finish_kernel<1>, dim3(1), dim3(PB_THREADS), 0, st, (const double*)wsd, (const unsigned*)wss, nparts, a.K,
                          count, out, status);
  return check_launch("pair_box_loss_forward (partial sum)");
}

extern "C" int hipie_pair_box_loss_backward(const int64_t* const* pair_q, const int64_t* pair_n, const float* out, const float* pair_grad,
                                            const float* g_bbox, const float* g_giou, const float* g_boxiou, float* d_boxes, float* d_iou, int B,
                                            int Q, void* stream) {
  using namespace hipie;
  const char* who = "pair_box_loss_backward";
  PairList pl;
  int K = 0;
  HIPIE_TRY(pair_list_check(who, pl, K, pair_q, nullptr, false, pair_n, B, Q, 0));
  hipStream_t st = (hipStream_t)stream;
  if ((int64_t)B * Q == 0) return HIPIE_OK;
  HIPIE_REQUIRE(d_boxes, "%s: null pointer", who);
  HIPIE_REQUIRE(K == 0 || (out && pair_grad && g_bbox && g_giou && (g_boxiou || !d_iou)), "%s: null pointer", who);
  HIPIE_REQUIRE(((uintptr_t)out & 7) == 0, "%s: out must be 8-byte aligned", who);
  if (hipMemsetAsync(d_boxes, 0, (size_t)B * Q * 4 * sizeof(float), st) != hipSuccess) return check_launch("pair_box_loss_backward (zero fill)");
  if (d_iou && hipMemsetAsync(d_iou, 0, (size_t)B * Q * sizeof(float), st) != hipSuccess) return check_launch("pair_box_loss_backward (zero fill)");
  if (K == 0) return HIPIE_OK;
  hipLaunchKernelGGL(pair_box_loss_backward_kernel, dim3((unsigned)pair_parts(K)), dim3(PB_THREADS), 0, st, pl, K, Q, out, pair_grad, g_bbox, g_giou,
                     g_boxiou, d_boxes, d_iou);
  return check_launch(who);
}

extern "C" int hipie_positive_onehot(const int64_t* const* pair_q, const int64_t* const* pair_t, const int64_t* pair_n, const uint8_t* pos_map,
                                     float* onehot, int B, int Q, int Tmax, int L, void* stream) {
  using namespace hipie;
  const char* who = "positive_onehot";
  HIPIE_REQUIRE(L >= 0, "%s: negative size", who);
  PairList pl;
  int K = 0;
  HIPIE_TRY(pair_list_check(who, pl, K, pair_q, pair_t, true, pair_n, B, Q, Tmax));
  const int64_t n = (int64_t)B * Q * L;
  if (n == 0) return HIPIE_OK;
  HIPIE_REQUIRE(onehot && (pos_map || K == 0), "%s: null pointer", who);
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(onehot, 0, (size_t)n * sizeof(float), st) != hipSuccess) return check_launch("positive_onehot (zero fill)");
  if (K == 0) return HIPIE_OK;
  hipLaunchKernelGGL(positive_onehot_kernel, dim3((unsigned)K), dim3(OH_THREADS), 0, st, pl, pos_map, onehot, Q, Tmax, L);
  return check_launch(who);
}
