// hungarian_assign.hip -- the one-to-one assignment of the Hungarian matchers for a whole batch, on the packed costs of hungarian_cost.hip:
//
//   hipie_hungarian_assign   per image the pairs of scipy.optimize.linear_sum_assignment on its (Q, n_tgt[b]) block, int64, on the device
//
// Replaces, per matcher call: the device -> host copy of the packed costs, the host wait for it, scipy once per image on the host and the
// host -> device copy of the pairs at every place that indexes with them.  Here: one launch for the batch, a workgroup of 256 threads per
// image (as ota_assign_kernel); nothing is read by the host but, when the caller asks for them, the B status words.
//
// The solver is scipy's: the shortest-augmenting-path algorithm of Crouse ("On implementing 2D rectangular assignment algorithms", 2016),
// restated operation for operation.  It has no multiplication and no reduction whose order could change a sum: float64 adds, subtracts and
// compares on the widened fp32 costs (exact), and ONE rule among equal candidates.  Kept, both decide ties:
//   * the reduced cost is ((minVal + C[i][j]) - u[i]) - v[j], in this order;
//   * the list of unscanned columns starts as nc-1 .. 0 and a removed entry is replaced by the last one;
//   * the next column is the one with the lowest `shortest`; among equals an unassigned column at the LARGEST list position wins, and
//     without an unassigned one the SMALLEST position -- the data-parallel form of the sequential scan's
//     `s < lowest || (s == lowest && row4col[j] == -1)`.
// The solver has nr = min(Q, n) <= 256 rows and nc = max(Q, n) <= 4096 columns; with Q > n the rows are the targets and the columns the
// queries (scipy's transposition), and the pairs are sorted by query afterwards (a rank-by-counting pass over at most 256 distinct values).
//
// State, in LDS (22 bytes per column + 3 KB: 91 KB at nc = 4096): v and shortest as float64; path, row4col and the list `remaining` as
// 16-bit values; u, col4row and the columns scanned for the current row per solver row.  A thread scans the list positions tid, tid + 256,
// ...; the selection is a butterfly over (value, key) in every wave and four LDS slots across them, with key = (unassigned ? 0x10000 + it :
// 0xFFFF - it) << 12 | column, so that "better" is one comparison on distinct keys and every thread derives the same winner.  Two barriers
// per scanned column.  The prologue checks the block for NaN / -inf (scipy's "invalid numeric entries"; +inf is legal) and, with Q > n,
// writes it solver-row-major (targets x queries) into the workspace, so that the row read of every iteration is contiguous.
//
// Every loop has a compile-time bound: a row's search scans at most nr columns (status bit 128 when that cap is hit, which valid input
// cannot reach), the augmentation walks at most nr steps.  Every barrier is reached by the whole workgroup: what ends a search early
// (an infeasible matrix, the cap) is derived from the same LDS words by every thread.  Any non-zero status -- the cost kernel's own bits
// are carried over -- leaves the image's pairs all 0, which are valid indices.
#include "common.h"

namespace hipie {

constexpr int HA_THREADS = 256, HA_WAVES = HA_THREADS / 64;
constexpr int HA_MAX_Q = 4096, HA_MAX_T = 256;           // hungarian_cost's limits
constexpr int HA_MAX_R = 256, HA_MAX_C = 4096;           // solver rows min(Q, n), solver columns max(Q, n)
constexpr int HA_ST_OFFSET = 16, HA_ST_INVALID = 32, HA_ST_INFEASIBLE = 64, HA_ST_CAP = 128;
constexpr int HA_FREE = 0x10000;                         // keys of unassigned columns start here

struct AssignArgs {
  const float* C;                            // hungarian_cost's packed output, Q * sum_t elements
  const int* cost_status;                    // (B,) the cost kernel's status words
  const int* n_tgt;                          // (B,)
  const int* t_off;                          // (B,)
  float* ws;                                 // Q * sum_t elements: the blocks with Q > n, solver-row-major
  long long* pair_q;                         // (B, K)
  long long* pair_t;                         // (B, K)
  int* status;                               // (B,)
  long sum_t;
  int Q, Tmax, K, ncm;                       // ncm: the column capacity of the LDS arrays
};

// is candidate (ov, ok) better than (bv, bk)?  keys of real candidates are distinct; a thread without one holds (+inf, -1)
__device__ __forceinline__ bool ha_better(double ov, int ok, double bv, int bk) { return ov < bv || (ov == bv && ok > bk); }

__global__ __launch_bounds__(HA_THREADS) void hungarian_assign_kernel(const AssignArgs a) {
#pragma clang fp contract(off)
  extern __shared__ double ha_lds[];
  __shared__ double s_val[HA_WAVES];
  __shared__ int s_key[HA_WAVES];
  __shared__ unsigned int s_status;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.x, Q = a.Q, ncm = a.ncm, K = a.K;
  double* v = ha_lds;
  double* shortest = v + ncm;
  double* u = shortest + ncm;
  unsigned short* path = reinterpret_cast<unsigned short*>(u + HA_MAX_R);
  short* row4col = reinterpret_cast<short*>(path + ncm);
  unsigned short* remaining = reinterpret_cast<unsigned short*>(row4col + ncm);
  short* col4row = reinterpret_cast<short*>(remaining + ncm);
  unsigned short* scanned = reinterpret_cast<unsigned short*>(col4row + HA_MAX_R);

  const int n = min(max(a.n_tgt[b], 0), a.Tmax);
  const long off = a.t_off[b];
  const bool fits = off >= 0 && off + n <= a.sum_t;          // the image's block lies inside C
  const bool transposed = Q > n;
  const int nr = transposed ? n : Q, nc = transposed ? Q : n;          // nr <= 256, nc <= 4096 <= ncm by the entry's limits
  const double INF = __builtin_inf();
  if (tid == 0) s_status = (unsigned int)a.cost_status[b] | (fits ? 0u : (unsigned int)HA_ST_OFFSET);
  __syncthreads();
  const unsigned int carried = s_status;
  __syncthreads();

  // ---- prologue: the validity scan and, with Q > n, the solver-row-major copy -----------------------------------------------------------
  const float* Cb = a.C + (long)Q * (fits ? off : 0);
  float* Wb = a.ws + (long)Q * (fits ? off : 0);
  if (carried == 0u && nr > 0) {
    bool bad = false;
    const int total = nr * nc;                               // <= 2^20
    for (int p = tid; p < total; p += HA_THREADS) {
      float x;
      if (transposed) {
        const int t = p / nc, q = p - t * nc;
        x = Cb[(long)q * n + t];
        Wb[p] = x;
      } else {
        x = Cb[p];
      }
      bad |= (x != x) || (x == -__builtin_inff());
    }
    if (bad) atomicOr(&s_status, (unsigned int)HA_ST_INVALID);
  }
  __syncthreads();                                           // the copy is read by other threads below; the status by all
  const unsigned int before = s_status;
  unsigned int fail = 0u;                                    // uniform: every thread derives it from the same LDS words

  if (before == 0u && nr > 0) {
    const float* M = transposed ? Wb : Cb;                   // (nr, nc) row-major
    for (int j = tid; j < nc; j += HA_THREADS) {
      v[j] = 0.0;
      row4col[j] = (short)-1;
      path[j] = (unsigned short)0xFFFF;
    }
    for (int r = tid; r < nr; r += HA_THREADS) {
      u[r] = 0.0;
      col4row[r] = (short)-1;
    }
    for (int cur = 0; cur < HA_MAX_R; ++cur) {
      if (cur >= nr || fail) break;
      for (int j = tid; j < nc; j += HA_THREADS) {
        shortest[j] = INF;
        remaining[j] = (unsigned short)(nc - 1 - j);
      }
      __syncthreads();
      double minVal = 0.0;
      int i = cur, n_rem = nc, sink = -1, n_it = 0;
      for (int k = 0; k < HA_MAX_R; ++k) {                   // a search scans at most cur + 1 <= nr columns
        if (k >= nr) break;
        const float* row = M + (long)i * nc;
        const double ui = u[i];
        double bv = INF;
        int bk = -1;
        for (int it = tid; it < n_rem; it += HA_THREADS) {
          const int j = remaining[it];
          const double r = ((minVal + (double)row[j]) - ui) - v[j];
          double s = shortest[j];
          if (r < s) {
            path[j] = (unsigned short)i;
            shortest[j] = r;
            s = r;
          }
          const int key = ((row4col[j] < 0 ? HA_FREE + it : 0xFFFF - it) << 12) | j;
          if (ha_better(s, key, bv, bk)) {
            bv = s;
            bk = key;
          }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
          const double ov = __shfl_xor(bv, o);
          const int ok = __shfl_xor(bk, o);
          if (ha_better(ov, ok, bv, bk)) {
            bv = ov;
            bk = ok;
          }
        }
        if (lane == 0) {
          s_val[wave] = bv;
          s_key[wave] = bk;
        }
        __syncthreads();
        bv = s_val[0];
        bk = s_key[0];
#pragma unroll
        for (int w = 1; w < HA_WAVES; ++w) {
          const double ov = s_val[w];
          const int ok = s_key[w];
          if (ha_better(ov, ok, bv, bk)) {
            bv = ov;
            bk = ok;
          }
        }
        minVal = bv;
        if (minVal == INF) {                                 // every column left is out of reach (bk may be -1: nothing is indexed with it)
          fail = (unsigned int)HA_ST_INFEASIBLE;
          break;
        }
        const int j = bk & 4095, pref = bk >> 12;
        const bool is_free = pref >= HA_FREE;
        const int index = is_free ? pref - HA_FREE : 0xFFFF - pref;
        const int owner = row4col[j];
        if (tid == 0) {
          scanned[k] = (unsigned short)j;
          remaining[index] = remaining[n_rem - 1];
        }
        --n_rem;
        n_it = k + 1;
        if (is_free) sink = j; else i = owner;
        __syncthreads();
        if (sink >= 0) break;
      }
      if (!fail && sink < 0) fail = (unsigned int)HA_ST_CAP;
      if (fail) break;
      // the dual variables: the scanned columns are distinct, and so are the rows that own all of them but the sink
      for (int k = tid; k < n_it; k += HA_THREADS) {
        const int j = scanned[k];
        const double d = minVal - shortest[j];
        v[j] = v[j] - d;
        if (k < n_it - 1) {
          const int r = row4col[j];
          u[r] = u[r] + d;
        }
      }
      if (tid == 0) u[cur] = u[cur] + minVal;
      __syncthreads();
      if (tid == 0) {                                        // augment along the path back to `cur`
        int j = sink;
        for (int s = 0; s < HA_MAX_R; ++s) {
          const int r = path[j];
          if (r >= nr) break;                                // cannot happen: a column on the path was reached in this search
          row4col[j] = (short)r;
          const int t = col4row[r];
          col4row[r] = (short)j;
          j = t;
          if (r == cur || j < 0) break;
        }
      }
      __syncthreads();
    }
  }

  // ---- the pairs ------------------------------------------------------------------------------------------------------------------------
  const unsigned int st = before | fail;
  if (tid == 0) a.status[b] = (int)st;
  long long* pq = a.pair_q + (long)b * K;
  long long* pt = a.pair_t + (long)b * K;
  const int np = st ? 0 : nr;
  for (int k = np + tid; k < K; k += HA_THREADS) {
    pq[k] = 0;
    pt[k] = 0;
  }
  if (!transposed) {
    for (int r = tid; r < np; r += HA_THREADS) {
      pq[r] = r;
      pt[r] = col4row[r];
    }
  } else {
    for (int t = tid; t < np; t += HA_THREADS) {             // rows are targets: sorted by query, a rank by counting
      const int q = col4row[t];
      int rank = 0;
      for (int o = 0; o < HA_MAX_R; ++o) {
        if (o >= np) break;
        rank += col4row[o] < q ? 1 : 0;
      }
      pq[rank] = q;
      pt[rank] = t;
    }
  }
}

static inline int assign_columns(int Q, int Tmax) { return (max(Q, Tmax) + 3) & ~3; }

}  // namespace hipie

extern "C" int64_t hipie_hungarian_assign_ws_bytes(int64_t Q, int64_t sum_t) {
  if (Q <= 0 || sum_t <= 0) return 16;
  return Q * sum_t * (int64_t)sizeof(float);
}

extern "C" int hipie_hungarian_assign(const float* C, const int* cost_status, const int* n_tgt, const int* t_off, int64_t* pair_q, int64_t* pair_t,
                                      int* status, void* ws, int64_t ws_bytes, int64_t B, int Q, int Tmax, int64_t sum_t, void* stream) {
  using namespace hipie;
  HIPIE_REQUIRE(B >= 0 && Q >= 0 && Tmax >= 0 && sum_t >= 0, "hungarian_assign: negative size");
  if (B == 0 || Q == 0 || Tmax == 0) return HIPIE_OK;
  HIPIE_REQUIRE(Q <= HA_MAX_Q && Tmax <= HA_MAX_T, "hungarian_assign: Q=%d, Tmax=%d outside Q <= %d, Tmax <= %d", Q, Tmax, HA_MAX_Q, HA_MAX_T);
  HIPIE_REQUIRE(B <= 65535, "hungarian_assign: B=%lld images exceed the grid", (long long)B);
  HIPIE_REQUIRE(sum_t <= B * (int64_t)Tmax, "hungarian_assign: sum_t=%lld exceeds B x Tmax", (long long)sum_t);
  HIPIE_REQUIRE(cost_status && n_tgt && t_off && pair_q && pair_t && status && (C || sum_t == 0), "hungarian_assign: null pointer");
  HIPIE_REQUIRE(ws || sum_t == 0, "hungarian_assign: null pointer (ws)");
  HIPIE_REQUIRE(sum_t == 0 || (((uintptr_t)ws & 3u) == 0 && ws_bytes >= hipie_hungarian_assign_ws_bytes(Q, sum_t)),
                "hungarian_assign: workspace of %lld bytes on a 4-byte boundary needed, got %lld", (long long)hipie_hungarian_assign_ws_bytes(Q, sum_t),
                (long long)ws_bytes);
  AssignArgs a;
  a.C = C; a.cost_status = cost_status; a.n_tgt = n_tgt; a.t_off = t_off; a.ws = static_cast<float*>(ws);
  a.pair_q = reinterpret_cast<long long*>(pair_q); a.pair_t = reinterpret_cast<long long*>(pair_t); a.status = status;
  a.sum_t = sum_t; a.Q = Q; a.Tmax = Tmax; a.K = min(Q, Tmax); a.ncm = assign_columns(Q, Tmax);
  const size_t lds = (size_t)a.ncm * (2 * sizeof(double) + 3 * sizeof(short)) + (size_t)HA_MAX_R * (sizeof(double) + 2 * sizeof(short));
  static LdsLimit limit;
  limit.raise((const void*)hungarian_assign_kernel, lds, 48 << 10);
  hipLaunchKernelGGL(hungarian_assign_kernel, dim3((unsigned)B), dim3(HA_THREADS), lds, (hipStream_t)stream, a);
  return check_launch("hungarian_assign");
}
