// point_select.hip -- the two forward-only (no_grad) places of the training criteria and matchers that sample a mask at points (fp32):
//
//   importance point selection   pts[n] = the k of C uniform candidates whose sampled logit is closest to 0, then P - k fresh points
//                                (criterion.uncertain_points: PointRend's get_uncertain_point_coords_with_randomness)
//   matcher mask costs           ce (Q, T), dice (Q, T) of every (prediction, target) pair at P shared points (matcher.mask_costs)
//
// Replaces, per criterion call: a (N, 3P) grid_sample, abs / neg, the library top-k (12 launches, csrc/topk.hip) and a gather + cat; per
// matcher call: two grid_sample launches, the three (Q, P) tensors softplus(-x), softplus(x), sigmoid(x), the (T, P) tensor 1 - t, three
// GEMMs and the broadcast arithmetic of the dice quotient.  The bilinear sample is point_sample.h's, the key tk_key of topk_key.h.
//
// Selection.  Score of candidate c = -|bilinear(src[n], cand[n, c])|; the k LARGEST scores are chosen (the smallest |logit|), ties at the
// threshold in ascending candidate index, -0.0 ties with +0.0, a NaN sample counts as the largest score (torch.topk, topk.hip).
// pts[n, 0:k] holds the chosen candidates in ASCENDING CANDIDATE INDEX -- torch.topk returns them sorted by score; the losses are sums over
// the points, so only their summation order differs -- and pts[n, k:P] = rest[n].
//   1. us_keys_kernel: a workgroup of 256 threads samples 1024 candidates of one instance (blockIdx.x = n * splits + split) and writes
//      their order-preserving 32-bit keys to the workspace (N, C).
//   2. us_select_kernel: one workgroup of 1024 threads per instance.  The 4-pass 8-bit radix select of topk.hip over the key row (147 KB
//      at C = 37632: re-read from L2, not staged) finds the key T of the k-th largest score; then every wave counts, in its contiguous
//      segment of the row, the keys above T and equal to T, and a second sweep ranks the chosen ones by ballot and writes them at their
//      rank: index order, no sort, no limit on k.  The same workgroup copies rest[n].
// The only atomics are the integer LDS histogram counts (their result does not depend on the order) and the grid is a function of (N, C):
// two calls give identical bits.
//
// Costs.  With x = sample(pred[q]), t = sample(tgt[j]), s = sigmoid(x):
//      ce   = (sum_p softplus(-x) t + softplus(x) (1 - t)) / P = (sum_p softplus(x) - sum_p x t) / P      (softplus(-x) - softplus(x) = -x)
//      dice = 1 - (2 sum_p s t + 1) / (sum_p s + sum_p t + 1)
// so a query needs sum softplus(x), sum s and two dot-product rows against the T sampled targets.
//   1. mc_targets_kernel: the targets are sampled ONCE into the workspace, (T, Ps) with Ps = P rounded up to the 2048-point chunk and
//      zeros behind P; a workgroup also leaves the sum of its 1024 samples.
//   2. mc_dots_kernel: a workgroup of 256 threads owns 4 queries x 2048 points (blockIdx.x = query block * splits + split): a thread
//      samples its 8 points of the 4 queries into registers -- the Q x P samples never reach HBM -- and then walks the targets two at a
//      time: two float4 loads per target, 16 partial sums (4 queries x 2 targets x {x t, s t}) per thread, which the wave adds by a
//      reduce-scatter (reduce16: 17 lane exchanges for the 16 sums instead of 96) and the four waves add in order through LDS.
//   3. mc_finish_kernel: a thread per (q, j) adds the partials in split order and forms ce and dice.
// No atomics, a fixed order of additions, grids that are functions of (Q, T, P): bit-reproducible.
// Offsets inside one map are 32-bit (H * W < 2^31, checked); the base of a map is 64-bit.
#include "common.h"
#include "point_sample.h"
#include "topk_key.h"
#include "wave.h"

namespace hipie {

constexpr int US_THREADS = 256;
constexpr int US_CHUNK = 1024;               // candidates per workgroup of the key kernel: 4 per thread
constexpr int US_SELECT_THREADS = 1024;      // the selection: 16 waves per instance
constexpr int MC_THREADS = 256;
constexpr int MC_TCHUNK = 1024;              // target samples per workgroup of mc_targets_kernel: 4 per thread
constexpr int MC_CHUNK = 2048;               // points per workgroup of mc_dots_kernel: 2 x 4 consecutive points per thread
constexpr int MC_QB = 4;                     // queries per workgroup of mc_dots_kernel

// ---- importance point selection ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(US_THREADS) void us_keys_kernel(const float* __restrict__ src, const float* __restrict__ cand,
                                                             unsigned int* __restrict__ keys, int H, int W, int C, int splits) {
  const long n = blockIdx.x / splits;
  const int split = blockIdx.x % splits;
  const float* map = src + n * ((long)H * W);
  const float* xy = cand + n * ((long)C * 2);
  unsigned int* row = keys + n * (long)C;
#pragma unroll
  for (int k = 0; k < US_CHUNK / US_THREADS; ++k) {
    const int c = split * US_CHUNK + k * US_THREADS + threadIdx.x;
    if (c < C) row[c] = tk_key(-fabsf(sample(map, corners_of(xy[2 * c], xy[2 * c + 1], H, W))));
  }
}

// keys (N, C), cand (N, C, 2), rest (N, P - k, 2) -> pts (N, P, 2)
__global__ __launch_bounds__(US_SELECT_THREADS) void us_select_kernel(const unsigned int* __restrict__ keys, const float* __restrict__ cand,
                                                                      const float* __restrict__ rest, float* __restrict__ pts, int C, int k,
                                                                      int P) {
  __shared__ unsigned int hist[256];
  __shared__ unsigned int s_prefix, s_krem;
  __shared__ unsigned int wave_gt[US_SELECT_THREADS / 64], wave_eq[US_SELECT_THREADS / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long n = blockIdx.x;
  const unsigned int* row = keys + n * (long)C;
  const float* xy = cand + n * ((long)C * 2);
  float* out = pts + n * ((long)P * 2);

  const int nrest = (P - k) * 2;
  for (int i = tid; i < nrest; i += US_SELECT_THREADS) out[2 * k + i] = rest[n * (long)nrest + i];
  if (k == 0) return;                            // the same for every thread

  // ---- radix select of the k-th largest key (topk.hip) ----
  unsigned int prefix = 0u, mask = 0u, krem = (unsigned int)k;
  for (int pass = 3; pass >= 0; --pass) {
    const int shift = 8 * pass;
    if (tid < 256) hist[tid] = 0u;
    __syncthreads();
    for (int i = tid; i < C; i += US_SELECT_THREADS) {
      const unsigned int kk = row[i];
      if ((kk & mask) == prefix) atomicAdd(&hist[(kk >> shift) & 255u], 1u);
    }
    __syncthreads();
    if (tid == 0) {
      unsigned int cum = 0u;
      int d = 255;
      for (; d > 0; --d) {
        if (cum + hist[d] >= krem) break;
        cum += hist[d];
      }
      s_prefix = prefix | ((unsigned int)d << shift);
      s_krem = krem - cum;
    }
    __syncthreads();
    prefix = s_prefix;
    krem = s_krem;
    mask |= 0xFFu << shift;
  }
  const unsigned int T = prefix;                 // key of the k-th largest score; the first krem (>= 1) candidates equal to T are taken

  // ---- compaction in index order: a wave owns a contiguous segment, counts first, then writes at the rank ----
  const int seg = ((C + US_SELECT_THREADS - 1) / US_SELECT_THREADS) * 64;      // indices per wave, a multiple of 64
  const int beg = wave * seg, end = min(C, beg + seg);
  const unsigned long long below = (1ull << lane) - 1ull;
  unsigned int ngt = 0u, neq = 0u;
  for (int i0 = beg; i0 < end; i0 += 64) {
    const int i = i0 + lane;
    const unsigned int kk = (i < end) ? row[i] : 0u;
    ngt += (unsigned int)__builtin_popcountll(__builtin_amdgcn_ballot_w64((i < end) && kk > T));
    neq += (unsigned int)__builtin_popcountll(__builtin_amdgcn_ballot_w64((i < end) && kk == T));
  }
  if (lane == 0) { wave_gt[wave] = ngt; wave_eq[wave] = neq; }
  __syncthreads();
  unsigned int eq_run = 0u, gt_run = 0u;         // equal / above in the segments in front of this one
  for (int w = 0; w < wave; ++w) { eq_run += wave_eq[w]; gt_run += wave_gt[w]; }
  unsigned int out_run = gt_run + min(eq_run, krem);
  for (int i0 = beg; i0 < end; i0 += 64) {
    const int i = i0 + lane;
    const unsigned int kk = (i < end) ? row[i] : 0u;
    const bool eq = (i < end) && kk == T;
    const unsigned long long eb = __builtin_amdgcn_ballot_w64(eq);
    const bool chosen = ((i < end) && kk > T) || (eq && eq_run + (unsigned int)__builtin_popcountll(eb & below) < krem);
    const unsigned long long cb = __builtin_amdgcn_ballot_w64(chosen);
    if (chosen) {
      // pos < k: the select leaves G keys above T and krem = k - G to take of those equal to it, so exactly k are chosen
      const unsigned int pos = out_run + (unsigned int)__builtin_popcountll(cb & below);
      out[2 * pos] = xy[2 * i];
      out[2 * pos + 1] = xy[2 * i + 1];
    }
    eq_run += (unsigned int)__builtin_popcountll(eb);
    out_run += (unsigned int)__builtin_popcountll(cb);
  }
}

static inline int us_splits(int C) { return C > 0 ? (C + US_CHUNK - 1) / US_CHUNK : 1; }

// ---- matcher mask costs --------------------------------------------------------------------------------------------------------------------
static inline int mc_splits(int P) { return P > 0 ? (P + MC_CHUNK - 1) / MC_CHUNK : 1; }

// the workspace, in floats: tsamp (T, Ps) | tpart (T, Ps / 1024) | part (splits, Q, T, 2) | qpart (splits, Q, 2)
struct CostWs {
  int splits, nts;
  int64_t Ps, tsamp, tpart, part, qpart, total;
};

static inline CostWs mc_layout(int64_t Q, int64_t T, int P) {
  CostWs w;
  w.splits = mc_splits(P);
  w.Ps = (int64_t)w.splits * MC_CHUNK;
  w.nts = (int)(w.Ps / MC_TCHUNK);
  w.tsamp = 0;
  w.tpart = w.tsamp + T * w.Ps;
  w.part = w.tpart + T * w.nts;
  w.qpart = w.part + (int64_t)w.splits * Q * T * 2;
  w.total = w.qpart + (int64_t)w.splits * Q * 2;
  return w;
}

// tsamp[j, p] = sample(tgt[j], coords[p]) for p < P, 0 for P <= p < Ps;  tpart[j, chunk] = the sum of the chunk's samples
__global__ __launch_bounds__(MC_THREADS) void mc_targets_kernel(const float* __restrict__ tgt, const float* __restrict__ coords,
                                                                float* __restrict__ tsamp, float* __restrict__ tpart, int Ht, int Wt, int P,
                                                                long Ps, int nts) {
  __shared__ float red[MC_THREADS / 64];
  const long j = blockIdx.x / nts;
  const int chunk = blockIdx.x % nts;
  const float* map = tgt + j * ((long)Ht * Wt);
  float acc = 0.f;
#pragma unroll
  for (int k = 0; k < MC_TCHUNK / MC_THREADS; ++k) {
    const int p = chunk * MC_TCHUNK + k * MC_THREADS + threadIdx.x;
    const float v = p < P ? sample(map, corners_of(coords[2 * p], coords[2 * p + 1], Ht, Wt)) : 0.f;
    tsamp[j * Ps + p] = v;
    acc += v;
  }
  acc = wave_sum(acc);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) tpart[j * nts + chunk] = ((red[0] + red[1]) + red[2]) + red[3];
}

// one step of reduce16: the lanes l and l ^ O split the first 2 * HALF values between them and add what the other one holds of their half
template <int HALF, int O>
__device__ __forceinline__ void reduce_step(float (&v)[16], int lane) {
  const bool up = (lane & O) != 0;
#pragma unroll
  for (int i = 0; i < HALF; ++i) {
    const float keep = up ? v[i + HALF] : v[i];
    const float give = up ? v[i] : v[i + HALF];
    v[i] = keep + __shfl_xor(give, O);
  }
}

// 16 values per lane -> the sum over the wave's 64 lanes of value reduce16_index(lane & 15), in a fixed order of additions
__device__ __forceinline__ float reduce16(float (&v)[16]) {
  const int lane = threadIdx.x & 63;
  reduce_step<8, 1>(v, lane);
  reduce_step<4, 2>(v, lane);
  reduce_step<2, 4>(v, lane);
  reduce_step<1, 8>(v, lane);
  float r = v[0];
  r += __shfl_xor(r, 16);
  r += __shfl_xor(r, 32);
  return r;
}

__device__ __forceinline__ int reduce16_index(int l) { return ((l & 1) << 3) | ((l & 2) << 1) | ((l & 4) >> 1) | ((l & 8) >> 3); }

struct CostArgs {
  const float* pred;                         // (Q, H, W)
  const float* coords;                       // (P, 2)
  const float* tsamp;                        // (T, Ps)
  float* part;                               // (splits, Q, T, 2): sum x t, sum s t over the split's points
  float* qpart;                              // (splits, Q, 2): sum softplus(x), sum s
  long Ps;
  int Q, T, H, W, P, splits;
};

__global__ __launch_bounds__(MC_THREADS) void mc_dots_kernel(const CostArgs a) {
  __shared__ float red[2][MC_THREADS / 64][16];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int q0 = (blockIdx.x / a.splits) * MC_QB, split = blockIdx.x % a.splits;
  const int pa = split * MC_CHUNK + tid * 4, pb = pa + MC_CHUNK / 2;      // the thread's two runs of 4 consecutive points

  // ---- the samples of the 4 queries at the thread's 8 points; a point behind P counts nothing ----
  float x[MC_QB][8], s[MC_QB][8], qs[2 * MC_QB];
#pragma unroll
  for (int i = 0; i < 2 * MC_QB; ++i) qs[i] = 0.f;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const int p = (e < 4 ? pa : pb) + (e & 3);
    if (p < a.P) {
      const Corners c = corners_of(a.coords[2 * p], a.coords[2 * p + 1], a.H, a.W);
#pragma unroll
      for (int qi = 0; qi < MC_QB; ++qi) {
        const float v = sample(a.pred + (long)min(q0 + qi, a.Q - 1) * ((long)a.H * a.W), c);      // a query behind Q: read as the last, not written
        const Sigmoid g = sigmoid_parts(v);
        x[qi][e] = v;
        s[qi][e] = g.p;
        qs[2 * qi] += fmaxf(v, 0.f) + g.l1p;   // softplus(v)
        qs[2 * qi + 1] += g.p;
      }
    } else {
#pragma unroll
      for (int qi = 0; qi < MC_QB; ++qi) x[qi][e] = s[qi][e] = 0.f;
    }
  }
#pragma unroll
  for (int i = 0; i < 2 * MC_QB; ++i) qs[i] = wave_sum(qs[i]);
  if (lane == 0) {
#pragma unroll
    for (int i = 0; i < 2 * MC_QB; ++i) red[1][wave][i] = qs[i];
  }
  __syncthreads();
  if (tid < 2 * MC_QB && q0 + (tid >> 1) < a.Q)
    a.qpart[((long)split * a.Q + q0 + (tid >> 1)) * 2 + (tid & 1)] = ((red[1][0][tid] + red[1][1][tid]) + red[1][2][tid]) + red[1][3][tid];

  // ---- the dot products, two targets at a time: acc[(qi * 2 + jj) * 2 + {x t, s t}] ----
  // red is double-buffered: buffer b is written again two rounds later, behind the barrier of the round between, which its readers have passed
  int buf = 0;
  for (int j0 = 0; j0 < a.T; j0 += 2, buf ^= 1) {
    float acc[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.f;
#pragma unroll
    for (int jj = 0; jj < 2; ++jj) {
      const float* row = a.tsamp + (long)min(j0 + jj, a.T - 1) * a.Ps;                             // a target behind T: read as the last, not written
      float t[2][4];
      Vec4<float>::load(row + pa, t[0]);
      Vec4<float>::load(row + pb, t[1]);
#pragma unroll
      for (int qi = 0; qi < MC_QB; ++qi) {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          acc[(qi * 2 + jj) * 2] += x[qi][e] * t[e >> 2][e & 3];
          acc[(qi * 2 + jj) * 2 + 1] += s[qi][e] * t[e >> 2][e & 3];
        }
      }
    }
    const float r = reduce16(acc);
    if (lane < 16) red[buf][wave][reduce16_index(lane)] = r;
    __syncthreads();
    if (tid < 16) {
      const int q = q0 + (tid >> 2), j = j0 + ((tid >> 1) & 1);
      if (q < a.Q && j < a.T)
        a.part[(((long)split * a.Q + q) * a.T + j) * 2 + (tid & 1)] = ((red[buf][0][tid] + red[buf][1][tid]) + red[buf][2][tid]) + red[buf][3][tid];
    }
  }
}

// a thread per (q, j): the partials in split order -> ce, dice
__global__ __launch_bounds__(MC_THREADS) void mc_finish_kernel(const float* __restrict__ part, const float* __restrict__ qpart,
                                                               const float* __restrict__ tpart, float* __restrict__ ce, float* __restrict__ dice,
                                                               long Q, long T, int P, int splits, int nts) {
  const long i = (long)blockIdx.x * MC_THREADS + threadIdx.x;
  if (i >= Q * T) return;
  const long q = i / T, j = i % T;
  float xt = 0.f, st = 0.f, sp = 0.f, ss = 0.f, ts = 0.f;
  for (int k = 0; k < splits; ++k) {
    xt += part[((k * Q + q) * T + j) * 2];
    st += part[((k * Q + q) * T + j) * 2 + 1];
    sp += qpart[(k * Q + q) * 2];
    ss += qpart[(k * Q + q) * 2 + 1];
  }
  for (int k = 0; k < nts; ++k) ts += tpart[j * nts + k];
  ce[i] = (sp - xt) / (float)P;
  dice[i] = 1.f - (2.f * st + 1.f) / (ss + ts + 1.f);
}

}  // namespace hipie

extern "C" int64_t hipie_uncertain_points_ws_bytes(int64_t N, int C) {
  if (N <= 0 || C <= 0) return 16;
  return N * C * (int64_t)sizeof(unsigned int);
}

extern "C" int hipie_uncertain_points(const float* src, const float* cand, const float* rest, float* pts, void* ws, int64_t ws_bytes, int64_t N,
                                      int H, int W, int C, int P, int k, void* stream) {
  using namespace hipie;
  HIPIE_REQUIRE(N >= 0 && H >= 0 && W >= 0 && C >= 0 && P >= 0, "uncertain_points: negative size");
  HIPIE_REQUIRE(k >= 0 && k <= C, "uncertain_points: k=%d must be in [0, C=%d]", k, C);
  HIPIE_REQUIRE(k <= P, "uncertain_points: k=%d exceeds P=%d points", k, P);
  if (N == 0 || P == 0) return HIPIE_OK;
  HIPIE_REQUIRE(P < (1 << 30) && C < (1 << 30), "uncertain_points: P=%d, C=%d must be below 2^30", P, C);
  HIPIE_REQUIRE(N < (1ll << 31) && N * us_splits(C) < (1ll << 31), "uncertain_points: N=%lld x %d candidate chunks exceed the grid", (long long)N,
                us_splits(C));
  HIPIE_REQUIRE(pts && (rest || k == P), "uncertain_points: null pointer");
  hipStream_t st = (hipStream_t)stream;
  if (k > 0) {
    HIPIE_REQUIRE(H > 0 && W > 0 && (int64_t)H * W < (1ll << 31), "uncertain_points: H*W=%lld must be in [1, 2^31) (32-bit offsets inside a map)",
                  (long long)H * W);
    HIPIE_REQUIRE(src && cand && ws, "uncertain_points: null pointer");
    HIPIE_REQUIRE(ws_bytes >= hipie_uncertain_points_ws_bytes(N, C), "uncertain_points: workspace of %lld bytes, %lld needed", (long long)ws_bytes,
                  (long long)hipie_uncertain_points_ws_bytes(N, C));
    const int splits = us_splits(C);
    hipLaunchKernelGGL(us_keys_kernel, dim3((unsigned)(N * splits)), dim3(US_THREADS), 0, st, src, cand, (unsigned int*)ws, H, W, C, splits);
    HIPIE_TRY(check_launch("uncertain_points (keys)"));
  }
  hipLaunchKernelGGL(us_select_kernel, dim3((unsigned)N), dim3(US_SELECT_THREADS), 0, st, (const unsigned int*)ws, cand, rest, pts, C, k, P);
  return check_launch("uncertain_points");
}

extern "C" int64_t hipie_mask_match_cost_ws_bytes(int64_t Q, int64_t T, int P) {
  if (Q <= 0 || T <= 0 || P <= 0) return 16;
  return hipie::mc_layout(Q, T, P).total * (int64_t)sizeof(float);
}

extern "C" int hipie_mask_match_cost(const float* pred, const float* tgt, const float* coords, float* ce, float* dice, void* ws, int64_t ws_bytes,
                                     int64_t Q, int H, int W, int64_t T, int Ht, int Wt, int P, void* stream) {
  using namespace hipie;
  HIPIE_REQUIRE(Q >= 0 && T >= 0 && H >= 0 && W >= 0 && Ht >= 0 && Wt >= 0, "mask_match_cost: negative size");
  if (Q == 0 || T == 0) return HIPIE_OK;
  HIPIE_REQUIRE(P > 0 && P < (1 << 30), "mask_match_cost: P=%d points must be in [1, 2^30)", P);
  HIPIE_REQUIRE(H > 0 && W > 0 && (int64_t)H * W < (1ll << 31), "mask_match_cost: H*W=%lld must be in [1, 2^31) (32-bit offsets inside a map)",
                (long long)H * W);
  HIPIE_REQUIRE(Ht > 0 && Wt > 0 && (int64_t)Ht * Wt < (1ll << 31), "mask_match_cost: Ht*Wt=%lld must be in [1, 2^31) (32-bit offsets inside a map)",
                (long long)Ht * Wt);
  const CostWs w = mc_layout(Q, T, P);
  const int64_t qblocks = (Q + MC_QB - 1) / MC_QB;
  HIPIE_REQUIRE(Q < (1ll << 31) && T < (1ll << 31) && qblocks * w.splits < (1ll << 31) && T * w.nts < (1ll << 31) &&
                    (Q * T + MC_THREADS - 1) / MC_THREADS < (1ll << 31),
                "mask_match_cost: Q=%lld, T=%lld exceed the grid", (long long)Q, (long long)T);
  HIPIE_REQUIRE(pred && tgt && coords && ce && dice && ws, "mask_match_cost: null pointer");
  HIPIE_REQUIRE(((uintptr_t)ws & 15) == 0, "mask_match_cost: the workspace must be 16-byte aligned");
  HIPIE_REQUIRE(ws_bytes >= hipie_mask_match_cost_ws_bytes(Q, T, P), "mask_match_cost: workspace of %lld bytes, %lld needed", (long long)ws_bytes,
                (long long)hipie_mask_match_cost_ws_bytes(Q, T, P));
  hipStream_t st = (hipStream_t)stream;
  float* f = (float*)ws;
  hipLaunchKernelGGL(mc_targets_kernel, dim3((unsigned)(T * w.nts)), dim3(MC_THREADS), 0, st, tgt, coords, f + w.tsamp, f + w.tpart, Ht, Wt, P,
                     (long)w.Ps, w.nts);
  HIPIE_TRY(check_launch("mask_match_cost (targets)"));
  CostArgs a;
  a.pred = pred; a.coords = coords; a.tsamp = f + w.tsamp; a.part = f + w.part; a.qpart = f + w.qpart;
  a.Ps = (long)w.Ps; a.Q = (int)Q; a.T = (int)T; a.H = H; a.W = W; a.P = P; a.splits = w.splits;
  hipLaunchKernelGGL(mc_dots_kernel, dim3((unsigned)(qblocks * w.splits)), dim3(MC_THREADS), 0, st, a);
  HIPIE_TRY(check_launch("mask_match_cost (dot products)"));
  hipLaunchKernelGGL(mc_finish_kernel, dim3((unsigned)((Q * T + MC_THREADS - 1) / MC_THREADS)), dim3(MC_THREADS), 0, st, (const float*)(f + w.part),
                     (const float*)(f + w.qpart), (const float*)(f + w.tpart), ce, dice, (long)Q, (long)T, P, w.splits, w.nts);
  return check_launch("mask_match_cost");
}
