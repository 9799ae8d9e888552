// hungarian_cost.hip -- the cost matrices of the one-to-one Hungarian matchers for a whole batch (matcher.cost_matrix; fp32, no gradient):
//
//   hipie_hungarian_cost   C = w.cls x class cost + w.l1 x L1 + w.giou x (-GIoU) + w.mask x ce + w.dice x dice, every image of the batch
//
// Replaces, per image and matcher call: about forty small launches (sigmoid, the element-wise passes of the focal token cost, the matmul with
// the positive map, cdist, generalized_box_iou, the index puts of the stuff mean, two nan_to_num, the weighted sums) and the host wait of
// generalized_box_iou's check.  Here: one launch for the batch, two with the stuff mean.  The output is PACKED and QUERY-major: image b is a
// dense row-major (Q, n_tgt[b]) block at element Q * t_off[b], which is what scipy's linear_sum_assignment reads after one copy to the host.
//
// Cost (hungarian_cost_kernel, a workgroup of 256 threads per 8 queries of an image).  The focal token costs of the 8 query rows are computed
// once into LDS; in map mode the positive maps of the image are packed into bit words in LDS by ballot and a thread per (query, target) adds
// the token costs of the target's positive tokens in ascending order and divides by their count (no positive token: 0 / 0 = NaN, as the
// reference's mean over nothing); in ids mode the class cost is the token cost of column labels[t].  Lanes run over the targets of a row, so
// the stores of a workgroup are one contiguous run.  The box terms and the token cost are match_cost.h's.  The first workgroup of an image
// checks every box of the image (status bit 0) and every label (bit 3) and writes the image's status word with a plain store.
//
// Stuff mean (hungarian_mean_kernel, the pre-pass; a workgroup per 64 queries of an image).  Every non-thing column of L1 and of -GIoU takes
// the mean over all (query, thing) entries of its image.  A workgroup adds its entries in float64 -- a thread its own in ascending order, the
// 64 lanes of a wave by butterfly, the four waves in order -- and leaves the two partial sums in `ws`; every workgroup of the cost kernel adds
// the partial sums of its image in ascending order and divides by Q x things.  No floating-point atomics, the grids are functions of (B, Q):
// two calls give identical bits.  After the mean every NaN of the two box costs becomes 0 (nan_to_num; infinities stay).
#include "common.h"
#include "match_cost.h"

namespace hipie {

constexpr int HC_THREADS = 256;
constexpr int HC_QB = 8;                     // queries per workgroup of the cost kernel
constexpr int HM_QB = 64;                    // queries per workgroup of the pre-pass
constexpr int HC_MAX_Q = 4096, HC_MAX_T = 256, HC_MAX_L = 1024;
constexpr int HC_ST_BOX = 1, HC_ST_LABEL = 8, HC_ST_OFFSET = 16;

struct HungarianArgs {
  const float* logits;                       // (B, Q, L), image stride ls_b
  const float* boxes;                        // (B, Q, 4) cxcywh, image stride bs_b; null: no box costs
  const float* tgt_boxes;                    // (B, Tmax, 4) cxcywh
  const int* n_tgt;                          // (B,)
  const int* t_off;                          // (B,) exclusive prefix sum of n_tgt
  const unsigned char* pos_map;              // (B, Tmax, L) | null
  const int* labels;                         // (B, Tmax) | null
  const unsigned char* is_thing;             // (B, Tmax), read with the stuff mean only
  const float* ce;                           // packed like C | null
  const float* dice;                         // packed like C | null
  double* part;                              // (B, NB, 2): the partial sums of the stuff mean
  float* C;                                  // Q * sum_t elements
  int* status;                               // (B,)
  long ls_b, bs_b, sum_t;
  int Q, Tmax, L, NB;
  float w_cls, w_l1, w_giou, w_mask, w_dice;
  int with_boxes, stuff_mean;
};

// torch.cdist(p=1) of two cxcywh rows: the four |differences|, added in order
__device__ __forceinline__ float box_l1(const float* __restrict__ a, const float* __restrict__ b) {
#pragma clang fp contract(off)
  return ((fabsf(a[0] - b[0]) + fabsf(a[1] - b[1])) + fabsf(a[2] - b[2])) + fabsf(a[3] - b[3]);
}

__device__ __forceinline__ double wave_sum_f64(double x) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o);
  return x;
}

// ---- the pre-pass of the stuff mean ----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(HC_THREADS) void hungarian_mean_kernel(const HungarianArgs a) {
#pragma clang fp contract(off)
  __shared__ double s_part[HC_THREADS / 64][2];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.y, q0 = blockIdx.x * HM_QB;
  const int nq = min(HM_QB, a.Q - q0);
  const int nt = min(max(a.n_tgt[b], 0), a.Tmax);
  const float* qboxes = a.boxes + (long)b * a.bs_b + (long)q0 * 4;
  const float* tboxes = a.tgt_boxes + (long)b * a.Tmax * 4;
  const unsigned char* thing = a.is_thing + (long)b * a.Tmax;
  double s_l1 = 0.0, s_gi = 0.0;
  for (int p = tid; p < nq * nt; p += HC_THREADS) {
    const int qi = p / nt, t = p - qi * nt;
    if (!thing[t]) continue;
    const float* qb = qboxes + qi * 4;
    const float* tb = tboxes + t * 4;
    s_l1 += (double)box_l1(qb, tb);
    s_gi += (double)(-box_pair(box_xyxy(qb), box_xyxy(tb)).giou);
  }
  s_l1 = wave_sum_f64(s_l1);
  s_gi = wave_sum_f64(s_gi);
  if (lane == 0) {
    s_part[wave][0] = s_l1;
    s_part[wave][1] = s_gi;
  }
  __syncthreads();
  if (tid < 2) {
    double s = 0.0;
    for (int w = 0; w < HC_THREADS / 64; ++w) s += s_part[w][tid];
    a.part[((long)b * a.NB + blockIdx.x) * 2 + tid] = s;
  }
}

// ---- the cost --------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(HC_THREADS) void hungarian_cost_kernel(const HungarianArgs a) {
#pragma clang fp contract(off)
  extern __shared__ float hc_lds[];          // tok (HC_QB, L) | bits (Tmax, ceil(L / 32)) in map mode
  __shared__ unsigned int s_status;
  __shared__ int s_things;
  __shared__ float s_mean[2];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.y, q0 = blockIdx.x * HC_QB;
  const int Q = a.Q, Tmax = a.Tmax, L = a.L, LW = (L + 31) >> 5;
  const int nq = min(HC_QB, Q - q0);
  const int nt_all = min(max(a.n_tgt[b], 0), Tmax);
  const long off = a.t_off[b];
  const bool fits = off >= 0 && off + nt_all <= a.sum_t;      // the image's block lies inside C
  const int nt = fits ? nt_all : 0;
  float* tok = hc_lds;
  unsigned int* bits = reinterpret_cast<unsigned int*>(hc_lds + HC_QB * L);
  const bool boxes_on = a.with_boxes != 0, mean_on = boxes_on && a.stuff_mean != 0;
  const float* qboxes = boxes_on ? a.boxes + (long)b * a.bs_b + (long)q0 * 4 : nullptr;
  const float* tboxes = boxes_on ? a.tgt_boxes + (long)b * Tmax * 4 : nullptr;
  const unsigned char* thing = mean_on ? a.is_thing + (long)b * Tmax : nullptr;
  const int* labels = a.labels ? a.labels + (long)b * Tmax : nullptr;

  if (tid == 0) {
    s_status = fits ? 0u : (unsigned int)HC_ST_OFFSET;
    s_things = 0;
  }
  // the token costs of the query rows, once
  const float* lg = a.logits + (long)b * a.ls_b + (long)q0 * L;
  for (int i = tid; i < nq * L; i += HC_THREADS) tok[i] = focal_token_cost(lg[i]);
  // the positive maps as bit words: a wave reads 64 tokens of a target and votes
  if (a.pos_map) {
    const unsigned char* pm = a.pos_map + (long)b * Tmax * L;
    for (int t = wave; t < nt; t += HC_THREADS / 64) {
      for (int l0 = 0; l0 < L; l0 += 64) {
        const int l = l0 + lane;
        const unsigned long long v = __builtin_amdgcn_ballot_w64(l < L && pm[(long)t * L + l] != 0);
        if (lane == 0) bits[t * LW + (l0 >> 5)] = (unsigned int)v;
        if (lane == 32 && (l0 >> 5) + 1 < LW) bits[t * LW + (l0 >> 5) + 1] = (unsigned int)(v >> 32);
      }
    }
  }
  __syncthreads();

  // the things of the image (an integer count: the order of the additions does not matter)
  if (mean_on) {
    int n = 0;
    for (int t = tid; t < nt; t += HC_THREADS) n += thing[t] ? 1 : 0;
    if (n) atomicAdd(&s_things, n);
  }
  // the image's status word: its first workgroup looks at every box and every label
  if (blockIdx.x == 0) {
    unsigned int st = 0u;
    if (boxes_on) {
      for (int i = tid; i < Q + nt_all; i += HC_THREADS)
        if (box_degenerate(box_xyxy(i < Q ? a.boxes + (long)b * a.bs_b + (long)i * 4 : tboxes + (i - Q) * 4))) st |= (unsigned int)HC_ST_BOX;
    }
    if (labels) {
      for (int t = tid; t < nt_all; t += HC_THREADS)
        if (labels[t] < 0 || labels[t] >= L) st |= (unsigned int)HC_ST_LABEL;
    }
    if (st) atomicOr(&s_status, st);
  }
  __syncthreads();
  if (blockIdx.x == 0 && tid == 0) a.status[b] = (int)s_status;
  // the two means: the partial sums of the pre-pass in ascending order, the same additions in every workgroup of the image
  if (mean_on && tid < 2) {
    double s = 0.0;
    for (int i = 0; i < a.NB; ++i) s += a.part[((long)b * a.NB + i) * 2 + tid];
    s_mean[tid] = (float)(s / ((double)Q * (double)s_things));          // no thing: 0 / 0 = NaN, zeroed below
  }
  if (mean_on) __syncthreads();

  // rows q0 .. q0 + nq of the image's (Q, nt) block are one contiguous run: entry p of it is (query p / nt, target p % nt)
  const long base = Q * off + (long)q0 * nt;
  for (int p = tid; p < nq * nt; p += HC_THREADS) {
    const int qi = p / nt, t = p - qi * nt;
    float cls;
    if (labels) {
      const int l = labels[t];
      cls = (l >= 0 && l < L) ? tok[qi * L + l] : NAN;
    } else {
      float sum = 0.f, cnt = 0.f;            // the target's positive tokens in ascending order
      for (int w = 0; w < LW; ++w) {
        unsigned int m = bits[t * LW + w];
        while (m) {
          sum += tok[qi * L + (w << 5) + __builtin_ctz(m)];
          cnt += 1.f;
          m &= m - 1u;
        }
      }
      cls = sum / cnt;
    }
    float c = a.w_cls * cls;
    if (boxes_on) {
      float l1, gi;
      if (mean_on && !thing[t]) {
        l1 = s_mean[0];
        gi = s_mean[1];
      } else {
        const float* qb = qboxes + qi * 4;
        const float* tb = tboxes + t * 4;
        l1 = box_l1(qb, tb);
        gi = -box_pair(box_xyxy(qb), box_xyxy(tb)).giou;
      }
      if (mean_on) {                         // nan_to_num(nan=0, posinf=inf, neginf=-inf)
        l1 = l1 != l1 ? 0.f : l1;
        gi = gi != gi ? 0.f : gi;
      }
      c = (c + a.w_l1 * l1) + a.w_giou * gi;
    }
    if (a.ce) c = (c + a.w_mask * a.ce[base + p]) + a.w_dice * a.dice[base + p];
    a.C[base + p] = c;
  }
}

static inline int hungarian_mean_blocks(int Q) { return ceil_div(Q, HM_QB); }

}  // namespace hipie

extern "C" int64_t hipie_hungarian_cost_bytes(int64_t Q, int64_t sum_t) {
  if (Q <= 0 || sum_t <= 0) return 0;
  return Q * sum_t * (int64_t)sizeof(float);
}

extern "C" int64_t hipie_hungarian_cost_ws_bytes(int64_t B, int64_t Q) {
  if (B <= 0 || Q <= 0) return 16;
  return B * ((Q + hipie::HM_QB - 1) / hipie::HM_QB) * 2 * (int64_t)sizeof(double);
}

extern "C" int hipie_hungarian_cost(const float* logits, int64_t logits_stride, const float* boxes, int64_t boxes_stride, const float* tgt_boxes,
                                    const int* n_tgt, const int* t_off, const unsigned char* pos_map, const int* labels,
                                    const unsigned char* is_thing, const float* ce, const float* dice, float* C, int* status, void* ws,
                                    int64_t ws_bytes, int64_t B, int Q, int Tmax, int L, int64_t sum_t, float w_cls, float w_l1, float w_giou,
                                    float w_mask, float w_dice, int with_boxes, int stuff_takes_mean, void* stream) {
  using namespace hipie;
  HIPIE_REQUIRE(B >= 0 && Q >= 0 && Tmax >= 0 && L >= 0 && sum_t >= 0, "hungarian_cost: negative size");
  if (B == 0 || Q == 0 || Tmax == 0) return HIPIE_OK;
  HIPIE_REQUIRE(Q <= HC_MAX_Q && Tmax <= HC_MAX_T && L >= 1 && L <= HC_MAX_L, "hungarian_cost: Q=%d, Tmax=%d, L=%d outside Q <= %d, Tmax <= %d, 1 <= L <= %d", Q,
                Tmax, L, HC_MAX_Q, HC_MAX_T, HC_MAX_L);
  HIPIE_REQUIRE(B <= 65535, "hungarian_cost: B=%lld images exceed the grid", (long long)B);
  HIPIE_REQUIRE(sum_t <= B * (int64_t)Tmax, "hungarian_cost: sum_t=%lld exceeds B x Tmax", (long long)sum_t);
  HIPIE_REQUIRE((pos_map != nullptr) != (labels != nullptr), "hungarian_cost: exactly one of pos_map and labels");
  HIPIE_REQUIRE((ce != nullptr) == (dice != nullptr), "hungarian_cost: ce and dice come together");
  HIPIE_REQUIRE(logits && n_tgt && t_off && status && (C || sum_t == 0), "hungarian_cost: null pointer");
  HIPIE_REQUIRE(!with_boxes || (boxes && tgt_boxes), "hungarian_cost: null pointer (boxes, tgt_boxes with the box costs)");
  HIPIE_REQUIRE(logits_stride >= (int64_t)Q * L && (!with_boxes || boxes_stride >= (int64_t)Q * 4), "hungarian_cost: image strides %lld, %lld below a dense image",
                (long long)logits_stride, (long long)boxes_stride);
  const bool mean = with_boxes && stuff_takes_mean;
  const int NB = hungarian_mean_blocks(Q);
  if (mean) {
    HIPIE_REQUIRE(is_thing && ws, "hungarian_cost: null pointer (is_thing, ws with the stuff mean)");
    HIPIE_REQUIRE(((uintptr_t)ws & 7u) == 0 && ws_bytes >= hipie_hungarian_cost_ws_bytes(B, Q), "hungarian_cost: workspace of %lld bytes on an 8-byte boundary needed, got %lld",
                  (long long)hipie_hungarian_cost_ws_bytes(B, Q), (long long)ws_bytes);
  }
  HungarianArgs a;
  a.logits = logits; a.boxes = with_boxes ? boxes : nullptr; a.tgt_boxes = tgt_boxes; a.n_tgt = n_tgt; a.t_off = t_off; a.pos_map = pos_map; a.labels = labels;
  a.is_thing = is_thing; a.ce = ce; a.dice = dice; a.part = static_cast<double*>(ws); a.C = C; a.status = status;
  a.ls_b = logits_stride; a.bs_b = boxes_stride; a.sum_t = sum_t;
  a.Q = Q; a.Tmax = Tmax; a.L = L; a.NB = NB;
  a.w_cls = w_cls; a.w_l1 = w_l1; a.w_giou = w_giou; a.w_mask = w_mask; a.w_dice = w_dice;
  a.with_boxes = with_boxes ? 1 : 0; a.stuff_mean = mean ? 1 : 0;
  if (mean) {
    hipLaunchKernelGGL(hungarian_mean_kernel, dim3((unsigned)NB, (unsigned)B), dim3(HC_THREADS), 0, (hipStream_t)stream, a);
    HIPIE_TRY(check_launch("hungarian_cost (stuff mean)"));
  }
  const size_t lds = ((size_t)HC_QB * L + (pos_map ? (size_t)Tmax * ((L + 31) / 32) : 0)) * sizeof(float);
  static LdsLimit limit;
  limit.raise((const void*)hungarian_cost_kernel, lds, 48 << 10);
  hipLaunchKernelGGL(hungarian_cost_kernel, dim3((unsigned)ceil_div(Q, HC_QB), (unsigned)B), dim3(HC_THREADS), lds, (hipStream_t)stream, a);
  return check_launch("hungarian_cost");
}
