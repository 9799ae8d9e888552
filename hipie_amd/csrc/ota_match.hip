// ota_match.hip -- the one-to-many SimOTA matching of the foreground queries (matcher.HungarianMatcher.forward_ota; fp32, no gradient):
//
//   hipie_ota_cost     cost, iou (B, Tmax, Q) of a batch of images from the raw logits      (matcher.ota_cost)
//   hipie_ota_assign   the dynamic-k assignment on those two buffers, one workgroup an image  (matcher.dynamic_k_assign)
//
// Replaces, per image and decoder level: about forty small launches of the cost, the host wait of generalized_box_iou's check, a Python loop
// over the targets with a topk, an index-put and a host wait each, and the repair loop's `while bool(...)`.  Here: two launches for the whole
// batch and three small result vectors the host reads in one copy.  Both buffers are TARGET-major: the column of a target is contiguous.
//
// Cost (ota_cost_kernel, a workgroup of 256 threads per 8 queries of an image).  The focal token costs of the 8 query rows are computed once
// into LDS; the positive maps of the image are packed into bit words in LDS by ballot; a thread per (query, target) then adds the token costs
// of the target's positive tokens in ascending token order, divides by their count (no positive token: 0 / 0 = NaN as the reference's mean
// over nothing, and status bit 1), subtracts 3 x GIoU, adds 100 where the query centre is not both inside the target box and within
// center_radius / stride of its centre, and 10000 on queries that are candidates of no target of the image (an LDS flag per query).  The box
// terms and the token cost are match_cost.h's.  Columns behind n_tgt[b] hold +inf / 0.  The first workgroup of an image also checks every
// box of the image (status bit 0) and every positive map (bit 1) and writes the image's status word with a plain store.
//
// Assignment (ota_assign_kernel, 1024 threads).  The match matrix is a bitmap in LDS, Q rows of ceil(Tmax / 32) words (at most 128 KB).
//   1. The waves take the target columns in turn: up to ten rounds of a wave arg-max over (IoU, index) give the min(Q, 10) largest IoUs, added
//      in descending order; k = max(1, (int)sum); k rounds of a wave arg-min over (cost, index) give the k cheapest queries, whose bits are set
//      with LDS integer atomics.  A round excludes what the rounds before it took by ORDER -- the entries after the last pick in (value,
//      index) order -- so nothing is marked and the column is simply re-read (it is a few KB in L2).
//   2. A thread per row: a row with more than one bit keeps the cheapest target of its row.  The set of these rows is kept (a bit per row of
//      the thread, in a register) -- the reference evaluates it once and re-uses the stale set in the repair loop.
//   3. Repair loop, while a target in front of n_tgt has no query: every row with a match gets cost[row, :] += 100000 in memory (fp32, so the
//      rounding and the accumulated additions are the reference's), every empty target takes the arg-min of its column, and if a row now has
//      several matches the rows of the stale set are reset to their current cheapest target.  Capped at Q rounds (status bit 2); the reference
//      would not return there.
//   4. The matched rows in ascending order with the lowest set bit of each (match[chosen].max(1)[1] returns the first maximum), compacted by
//      ballot rank as in point_select.hip; per target the matched query of the smallest cost.
// Every tie goes to the lowest index.  The only atomics are integer LDS atomics whose result does not depend on their order, the grids are
// functions of (B, Q): two calls give identical bits.
#include "common.h"
#include "match_cost.h"
#include "wave.h"

namespace hipie {

constexpr int OC_THREADS = 256;
constexpr int OC_QB = 8;                     // queries per workgroup of the cost kernel
constexpr int OA_THREADS = 1024;             // the assignment: 16 waves per image
constexpr int OA_WAVES = OA_THREADS / 64;
constexpr int OTA_MAX_Q = 4096, OTA_MAX_T = 256, OTA_MAX_L = 1024;
constexpr int OA_MAXW = OTA_MAX_T / 32;      // bitmap words per row
constexpr int OA_MAXROWS = OTA_MAX_Q / OA_THREADS;      // rows per thread

// ---- the cost --------------------------------------------------------------------------------------------------------------------------
struct OtaCostArgs {
  const float* logits;                       // (B, Q, L)
  const float* boxes;                        // (B, Q, 4) cxcywh
  const float* tgt_boxes;                    // (B, Tmax, 4) cxcywh
  const unsigned char* pos_map;              // (B, Tmax, L)
  const int* n_tgt;                          // (B,)
  float* cost;                               // (B, Tmax, Q)
  float* iou;                                // (B, Tmax, Q)
  int* status;                               // (B,)
  int Q, Tmax, L;
  float r;                                   // center_radius / stride
};

struct Centre {
  bool inside, near;
};

// matcher.ota_cost: the query centre strictly inside the target box / within r of the target centre
__device__ __forceinline__ Centre centre_terms(const float* __restrict__ qb, const float* __restrict__ tb, const BoxXYXY& t, float r) {
#pragma clang fp contract(off)
  const float cx = qb[0], cy = qb[1];
  Centre c;
  c.inside = cx > t.x0 && cx < t.x1 && cy > t.y0 && cy < t.y1;
  c.near = cx > tb[0] - r && cx < tb[0] + r && cy > tb[1] - r && cy < tb[1] + r;
  return c;
}

__global__ __launch_bounds__(OC_THREADS) void ota_cost_kernel(const OtaCostArgs a) {
#pragma clang fp contract(off)
  extern __shared__ float oc_lds[];          // tok (OC_QB, L) | bits (Tmax, ceil(L / 32))
  __shared__ unsigned int s_cand[OC_QB];
  __shared__ unsigned int s_status;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.y, q0 = blockIdx.x * OC_QB;
  const int Q = a.Q, Tmax = a.Tmax, L = a.L, LW = (L + 31) >> 5;
  const int nq = min(OC_QB, Q - q0);
  const int nt = min(max(a.n_tgt[b], 0), Tmax);
  float* tok = oc_lds;
  unsigned int* bits = reinterpret_cast<unsigned int*>(oc_lds + OC_QB * L);
  const float* qboxes = a.boxes + ((long)b * Q + q0) * 4;
  const float* tboxes = a.tgt_boxes + (long)b * Tmax * 4;

  // the token costs of the query rows, once
  const float* lg = a.logits + ((long)b * Q + q0) * L;
  for (int i = tid; i < nq * L; i += OC_THREADS) tok[i] = focal_token_cost(lg[i]);
  // the positive maps as bit words: a wave reads 64 tokens of a target and votes
  const unsigned char* pm = a.pos_map + (long)b * Tmax * L;
  for (int t = wave; t < nt; t += OC_THREADS / 64) {
    for (int l0 = 0; l0 < L; l0 += 64) {
      const int l = l0 + lane;
      const unsigned long long v = __builtin_amdgcn_ballot_w64(l < L && pm[(long)t * L + l] != 0);
      if (lane == 0) bits[t * LW + (l0 >> 5)] = (unsigned int)v;
      if (lane == 32 && (l0 >> 5) + 1 < LW) bits[t * LW + (l0 >> 5) + 1] = (unsigned int)(v >> 32);
    }
  }
  if (tid < OC_QB) s_cand[tid] = 0u;
  if (tid == 0) s_status = 0u;
  __syncthreads();

  // a query is a candidate when its centre is inside the box or near the centre of ANY target
  for (int p = tid; p < nq * nt; p += OC_THREADS) {
    const int t = p / nq, qi = p - t * nq;
    const Centre c = centre_terms(qboxes + qi * 4, tboxes + t * 4, box_xyxy(tboxes + t * 4), a.r);
    if (c.inside || c.near) atomicOr(&s_cand[qi], 1u);
  }
  // the image's status word: its first workgroup looks at every box and every positive map
  if (blockIdx.x == 0) {
    unsigned int st = 0u;
    for (int i = tid; i < Q + nt; i += OC_THREADS)
      if (box_degenerate(box_xyxy(i < Q ? a.boxes + ((long)b * Q + i) * 4 : tboxes + (i - Q) * 4))) st |= 1u;
    for (int t = tid; t < nt; t += OC_THREADS) {
      unsigned int any = 0u;
      for (int w = 0; w < LW; ++w) any |= bits[t * LW + w];
      if (any == 0u) st |= 2u;
    }
    if (st) atomicOr(&s_status, st);
  }
  __syncthreads();
  if (blockIdx.x == 0 && tid == 0) a.status[b] = (int)s_status;

  for (int p = tid; p < nq * Tmax; p += OC_THREADS) {
    const int t = p / nq, qi = p - t * nq;
    const long o = ((long)b * Tmax + t) * Q + q0 + qi;
    if (t >= nt) {                           // never read by the assignment: defined values
      a.cost[o] = INFINITY;
      a.iou[o] = 0.f;
      continue;
    }
    float sum = 0.f, cnt = 0.f;              // the target's positive tokens in ascending order
    for (int w = 0; w < LW; ++w) {
      unsigned int m = bits[t * LW + w];
      while (m) {
        sum += tok[qi * L + (w << 5) + __builtin_ctz(m)];
        cnt += 1.f;
        m &= m - 1u;
      }
    }
    const BoxXYXY tb = box_xyxy(tboxes + t * 4);
    const BoxPair bp = box_pair(box_xyxy(qboxes + qi * 4), tb);
    const Centre c = centre_terms(qboxes + qi * 4, tboxes + t * 4, tb, a.r);
    float v = (sum / cnt - 3.f * bp.giou) + ((c.inside && c.near) ? 0.f : 100.f);
    if (!s_cand[qi]) v += 10000.f;
    a.cost[o] = v;
    a.iou[o] = bp.inter / bp.uni;
  }
}

// ---- the assignment --------------------------------------------------------------------------------------------------------------------
struct Pick {
  float v;
  int i;                                     // -1: nothing
};

// (v, i) in front of (m.v, m.i)?  the smaller value, at equal values the lower index
__device__ __forceinline__ bool pick_before(float v, int i, const Pick& m) { return m.i < 0 || v < m.v || (v == m.v && i < m.i); }

// the first of the 64 lanes' picks in that order, in every lane
__device__ __forceinline__ Pick wave_first(Pick m) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(m.v, o);
    const int oi = __shfl_xor(m.i, o);
    if (oi >= 0 && pick_before(ov, oi, m)) {
      m.v = ov;
      m.i = oi;
    }
  }
  return m;
}

// the first entry of sign * col[0:Q] that comes AFTER `prev` in (value, index) order (prev.i < 0: the first of all), over a whole wave
__device__ __forceinline__ Pick column_next(const float* col, int Q, float sign, const Pick& prev, int lane) {
  Pick m;
  m.v = 0.f;
  m.i = -1;
  for (int i = lane; i < Q; i += 64) {
    const float v = sign * col[i];
    if ((prev.i < 0 || v > prev.v || (v == prev.v && i > prev.i)) && (m.i < 0 || v < m.v)) {
      m.v = v;
      m.i = i;
    }
  }
  return wave_first(m);
}

__device__ __forceinline__ unsigned int wave_or(unsigned int x) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x |= (unsigned int)__shfl_xor((int)x, o);
  return x;
}

// match[row] = the cheapest target of the row alone (matcher.dynamic_k_assign's keep_cheapest); the row belongs to the calling thread
__device__ __forceinline__ void keep_cheapest(unsigned int* bm, const float* cost, int row, int Q, int nt, int W) {
  float bv = cost[row];
  int bt = 0;
  for (int t = 1; t < nt; ++t) {
    const float v = cost[(long)t * Q + row];
    if (v < bv) {
      bv = v;
      bt = t;
    }
  }
  for (int w = 0; w < W; ++w) bm[row * W + w] = 0u;
  bm[row * W + (bt >> 5)] = 1u << (bt & 31);
}

struct OtaAssignArgs {
  float* cost;                               // (B, Tmax, Q), modified in place
  const float* iou;                          // (B, Tmax, Q)
  const int* n_tgt;                          // (B,)
  int* pair_q;                               // (B, Q)
  int* pair_t;                               // (B, Q)
  int* best;                                 // (B, Tmax)
  int* n_pairs;                              // (B,)
  int* status;                               // (B,)
  int* rounds;                               // (B,)
  int Q, Tmax;
};

__global__ __launch_bounds__(OA_THREADS) void ota_assign_kernel(const OtaAssignArgs a) {
  extern __shared__ unsigned int bm[];       // (Q, W)
  __shared__ unsigned int s_col[OA_MAXW];
  __shared__ unsigned int s_multi;
  __shared__ unsigned int s_wcnt[OA_WAVES];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.x, Q = a.Q, Tmax = a.Tmax, W = (Tmax + 31) >> 5;
  const int nt = min(max(a.n_tgt[b], 0), Tmax);
  float* cost = a.cost + (long)b * Tmax * Q;
  const float* iou = a.iou + (long)b * Tmax * Q;
  int* best = a.best + (long)b * Tmax;

  if (nt == 0) {                             // the same for every thread
    for (int t = tid; t < Tmax; t += OA_THREADS) best[t] = 0;
    if (tid == 0) {
      a.n_pairs[b] = 0;
      a.rounds[b] = 0;
    }
    return;
  }
  for (int i = tid; i < Q * W; i += OA_THREADS) bm[i] = 0u;
  __syncthreads();

  // ---- 1. every target takes its k cheapest queries, k from its largest IoUs ----
  for (int t = wave; t < nt; t += OA_WAVES) {
    const float* ic = iou + (long)t * Q;
    const float* cc = cost + (long)t * Q;
    Pick prev;
    prev.v = 0.f;
    prev.i = -1;
    float sum = 0.f;
    for (int r = 0; r < min(Q, 10); ++r) {
      prev = column_next(ic, Q, -1.f, prev, lane);
      if (prev.i < 0) break;                 // NaN entries only: the same for the whole wave
      sum += -prev.v;
    }
    const int k = min(sum >= 1.f ? min((int)sum, 10) : 1, Q);
    prev.i = -1;
    for (int r = 0; r < k; ++r) {
      prev = column_next(cc, Q, 1.f, prev, lane);
      if (prev.i < 0) break;
      if (lane == 0) atomicOr(&bm[prev.i * W + (t >> 5)], 1u << (t & 31));
    }
  }
  __syncthreads();

  // ---- 2. a row claimed by several targets keeps the cheapest; the set of these rows stays as it is now ----
  unsigned int contested = 0u;
#pragma unroll
  for (int j = 0; j < OA_MAXROWS; ++j) {
    const int row = tid + j * OA_THREADS;
    if (row < Q) {
      int n = 0;
      for (int w = 0; w < W; ++w) n += __builtin_popcount(bm[row * W + w]);
      if (n > 1) {
        contested |= 1u << j;
        keep_cheapest(bm, cost, row, Q, nt, W);
      }
    }
  }

  // ---- 3. the repair loop ----
  int rounds = 0;
  bool capped = false;
  for (;;) {
    if (tid < OA_MAXW) s_col[tid] = 0u;
    if (tid == 0) s_multi = 0u;
    __syncthreads();
    unsigned int col[OA_MAXW];
#pragma unroll
    for (int w = 0; w < OA_MAXW; ++w) col[w] = 0u;
#pragma unroll
    for (int j = 0; j < OA_MAXROWS; ++j) {
      const int row = tid + j * OA_THREADS;
      if (row < Q) {
#pragma unroll
        for (int w = 0; w < OA_MAXW; ++w)
          if (w < W) col[w] |= bm[row * W + w];
      }
    }
#pragma unroll
    for (int w = 0; w < OA_MAXW; ++w) {
      if (w < W) {
        const unsigned int v = wave_or(col[w]);
        if (lane == 0 && v) atomicOr(&s_col[w], v);
      }
    }
    __syncthreads();
    bool empty = false;                      // a target in front of nt without a query: the same for every thread
    for (int w = 0; w < W; ++w) {
      const int n = min(32, nt - w * 32);
      const unsigned int valid = n <= 0 ? 0u : (n == 32 ? 0xFFFFFFFFu : (1u << n) - 1u);
      empty = empty || (~s_col[w] & valid) != 0u;
    }
    if (!empty) break;
    if (rounds >= Q) {
      capped = true;
      break;
    }
    ++rounds;
    // every row with a match moves behind the free ones, in all its columns: the fp32 addition in memory
#pragma unroll
    for (int j = 0; j < OA_MAXROWS; ++j) {
      const int row = tid + j * OA_THREADS;
      if (row < Q) {
        unsigned int any = 0u;
        for (int w = 0; w < W; ++w) any |= bm[row * W + w];
        if (any)
          for (int t = 0; t < nt; ++t) cost[(long)t * Q + row] += 100000.f;
      }
    }
    __syncthreads();
    // every empty target takes the cheapest query of its column
    for (int t = wave; t < nt; t += OA_WAVES) {
      if ((s_col[t >> 5] >> (t & 31)) & 1u) continue;
      Pick none;
      none.v = 0.f;
      none.i = -1;
      const Pick m = column_next(cost + (long)t * Q, Q, 1.f, none, lane);
      if (lane == 0 && m.i >= 0) atomicOr(&bm[m.i * W + (t >> 5)], 1u << (t & 31));
    }
    __syncthreads();
    // a row with several matches anywhere: the rows of the STALE contested set go to their current cheapest target
    bool multi = false;
#pragma unroll
    for (int j = 0; j < OA_MAXROWS; ++j) {
      const int row = tid + j * OA_THREADS;
      if (row < Q) {
        int n = 0;
        for (int w = 0; w < W; ++w) n += __builtin_popcount(bm[row * W + w]);
        multi = multi || n > 1;
      }
    }
    if (multi) atomicOr(&s_multi, 1u);
    __syncthreads();
    if (s_multi) {
#pragma unroll
      for (int j = 0; j < OA_MAXROWS; ++j)
        if ((contested >> j) & 1u) keep_cheapest(bm, cost, tid + j * OA_THREADS, Q, nt, W);
    }
    __syncthreads();
  }

  // ---- 4. the matched rows in ascending order with their first target: a wave owns a contiguous segment, counts, then writes at the rank ----
  const int seg = ((Q + OA_THREADS - 1) / OA_THREADS) * 64;
  const int beg = wave * seg, end = min(Q, beg + seg);
  const unsigned long long below = (1ull << lane) - 1ull;
  unsigned int n = 0u;
  for (int i0 = beg; i0 < end; i0 += 64) {
    const int row = i0 + lane;
    unsigned int any = 0u;
    if (row < end)
      for (int w = 0; w < W; ++w) any |= bm[row * W + w];
    n += (unsigned int)__builtin_popcountll(__builtin_amdgcn_ballot_w64(any != 0u));
  }
  if (lane == 0) s_wcnt[wave] = n;
  __syncthreads();
  unsigned int run = 0u, total = 0u;
  for (int w = 0; w < OA_WAVES; ++w) {
    if (w < wave) run += s_wcnt[w];
    total += s_wcnt[w];
  }
  int* pq = a.pair_q + (long)b * Q;
  int* pt = a.pair_t + (long)b * Q;
  for (int i0 = beg; i0 < end; i0 += 64) {
    const int row = i0 + lane;
    int first = -1;
    if (row < end) {
      for (int w = W - 1; w >= 0; --w) {
        const unsigned int m = bm[row * W + w];
        if (m) first = (w << 5) + __builtin_ctz(m);
      }
    }
    const unsigned long long cb = __builtin_amdgcn_ballot_w64(first >= 0);
    if (first >= 0) {
      const unsigned int pos = run + (unsigned int)__builtin_popcountll(cb & below);      // < the number of matched rows <= Q
      pq[pos] = row;
      pt[pos] = first;
    }
    run += (unsigned int)__builtin_popcountll(cb);
  }
  // per target the matched query of the smallest cost (the reference's arg-min of the column with +inf on everything unmatched)
  for (int t = wave; t < Tmax; t += OA_WAVES) {
    Pick m;
    m.v = 0.f;
    m.i = -1;
    if (t < nt) {
      for (int i = lane; i < Q; i += 64) {
        if (!((bm[i * W + (t >> 5)] >> (t & 31)) & 1u)) continue;
        const float v = cost[(long)t * Q + i];
        if (m.i < 0 || v < m.v) {
          m.v = v;
          m.i = i;
        }
      }
      m = wave_first(m);
    }
    if (lane == 0) best[t] = max(m.i, 0);
  }
  if (tid == 0) {
    a.n_pairs[b] = (int)total;
    a.rounds[b] = rounds;
    if (capped) a.status[b] |= 4;
  }
}

static inline bool ota_within_limits(int Q, int Tmax) { return Q <= OTA_MAX_Q && Tmax <= OTA_MAX_T; }

}  // namespace hipie

extern "C" int64_t hipie_ota_match_ws_bytes(int64_t B, int64_t Q, int64_t Tmax) {
  if (B <= 0 || Q <= 0 || Tmax <= 0) return 16;
  return 2 * B * Tmax * Q * (int64_t)sizeof(float);
}

extern "C" int hipie_ota_cost(const float* logits, const float* boxes, const float* tgt_boxes, const unsigned char* pos_map, const int* n_tgt,
                              float* cost, float* iou, int* status, int64_t B, int Q, int Tmax, int L, float center_radius, float stride,
                              void* stream) {
  using namespace hipie;
  HIPIE_REQUIRE(B >= 0 && Q >= 0 && Tmax >= 0 && L >= 0, "ota_cost: negative size");
  if (B == 0 || Q == 0 || Tmax == 0) return HIPIE_OK;
  HIPIE_REQUIRE(ota_within_limits(Q, Tmax) && L >= 1 && L <= OTA_MAX_L, "ota_cost: Q=%d, Tmax=%d, L=%d outside Q <= %d, Tmax <= %d, 1 <= L <= %d", Q, Tmax,
                L, OTA_MAX_Q, OTA_MAX_T, OTA_MAX_L);
  HIPIE_REQUIRE(B <= 65535, "ota_cost: B=%lld images exceed the grid", (long long)B);
  HIPIE_REQUIRE(stride > 0.f, "ota_cost: stride=%g must be positive", (double)stride);
  HIPIE_REQUIRE(logits && boxes && tgt_boxes && pos_map && n_tgt && cost && iou && status, "ota_cost: null pointer");
  OtaCostArgs a;
  a.logits = logits; a.boxes = boxes; a.tgt_boxes = tgt_boxes; a.pos_map = pos_map; a.n_tgt = n_tgt; a.cost = cost; a.iou = iou; a.status = status;
  a.Q = Q; a.Tmax = Tmax; a.L = L;
  a.r = (float)((double)center_radius / (double)stride);
  const size_t lds = ((size_t)OC_QB * L + (size_t)Tmax * ((L + 31) / 32)) * sizeof(float);
  static LdsLimit limit;
  limit.raise((const void*)ota_cost_kernel, lds, 48 << 10);
  hipLaunchKernelGGL(ota_cost_kernel, dim3((unsigned)ceil_div(Q, OC_QB), (unsigned)B), dim3(OC_THREADS), lds, (hipStream_t)stream, a);
  return check_launch("ota_cost");
}

extern "C" int hipie_ota_assign(float* cost, const float* iou, const int* n_tgt, int* pair_q, int* pair_t, int* best, int* n_pairs, int* status,
                                int* rounds, int64_t B, int Q, int Tmax, void* stream) {
  using namespace hipie;
  HIPIE_REQUIRE(B >= 0 && Q >= 0 && Tmax >= 0, "ota_assign: negative size");
  if (B == 0 || Q == 0 || Tmax == 0) return HIPIE_OK;
  HIPIE_REQUIRE(ota_within_limits(Q, Tmax), "ota_assign: Q=%d, Tmax=%d outside Q <= %d, Tmax <= %d", Q, Tmax, OTA_MAX_Q, OTA_MAX_T);
  HIPIE_REQUIRE(B < (1ll << 31), "ota_assign: B=%lld images exceed the grid", (long long)B);
  HIPIE_REQUIRE(cost && iou && n_tgt && pair_q && pair_t && best && n_pairs && status && rounds, "ota_assign: null pointer");
  OtaAssignArgs a;
  a.cost = cost; a.iou = iou; a.n_tgt = n_tgt; a.pair_q = pair_q; a.pair_t = pair_t; a.best = best; a.n_pairs = n_pairs; a.status = status;
  a.rounds = rounds; a.Q = Q; a.Tmax = Tmax;
  const size_t lds = (size_t)Q * ((Tmax + 31) / 32) * sizeof(unsigned int);
  static LdsLimit limit;
  limit.raise((const void*)ota_assign_kernel, lds, 48 << 10);
  hipLaunchKernelGGL(ota_assign_kernel, dim3((unsigned)B), dim3(OA_THREADS), lds, (hipStream_t)stream, a);
  return check_launch("ota_assign");
}
