// act_bwd.hip -- the pointwise activation between the two linears of an MLP, for the training step (fp32, HBM-bound):
//
//   forward:   a = act(u)                                 u = x . W1^T + b1 (rows, N);  act: 1 = exact-erf GELU, 2 = ReLU (hipie_gemm's codes)
//   backward:  du    = g * act'(u)                        g = d loss / d a;  du may BE g
//              a     = act(u)            (optional)       RECOMPUTED, the bits of the forward kernel: the graph does not keep `a`
//              dbias = sum_rows du       (optional)       the gradient of b1
//
// Replaces, in the backward of timm's Mlp (fc1 -> GELU -> fc2, hipie/backbone/vit.py:193-197) and of the encoder FFN (linear1 -> ReLU ->
// linear2, deformable_transformer_dino.py:384-394): the library's gelu_backward / threshold_backward, the separate row sum for the bias
// gradient, and the saved copy of `a`.  One pass: bytes per element 4 * (|u| + |g| + |du| + |a|).
//
// Lanes run along columns, 16 bytes each: a workgroup of 256 threads owns a tile of 1024 columns (blockIdx.x) and walks rows in chunks of
// ACT_ROWS (blockIdx.y, grid stride): the ACT_ROWS loads of u and of g are issued before the first use.  No LDS on the element path.
// dbias: every thread keeps the partial sums of its four columns in registers over all its rows and writes them into row blockIdx.y of
// the workspace (nparts, N); partial_rows_sum_kernel<8, 32> (row_norm.h) adds the partial rows in a fixed order.  No atomics: bit-reproducible from call to call.
// The grid -- ceil(N / 1024) x min(ceil(rows / ACT_ROWS), max(1, ACT_MAX_WG / ceil(N / 1024))) -- is a function of (rows, N) alone.
#include "common.h"
#include "gelu.h"
#include "row_norm.h"

namespace hipie {

constexpr int ACT_ROWS = 4;          // rows per workgroup and grid stride: 8 x 16-byte loads in flight per lane
constexpr int ACT_COLS = 1024;       // columns per workgroup: 256 threads x 4
constexpr int ACT_MAX_WG = 2048;     // workgroups of the element kernel: 8 per CU on 256 CUs (32 waves per CU)
constexpr int ACT_FWD_MAX_WG = 1 << 20;      // workgroups of the forward kernel (268 M elements before a thread takes a second piece)
constexpr int ACT_FIN_COLS = 32;     // the partial-row sum: a workgroup owns 32 columns (128-byte row pieces), 8 groups of partial rows each
constexpr int ACT_FIN_GROUPS = 8;

template <int ACT>
__device__ __forceinline__ float act_value(float u) {
  return ACT == 1 ? gm_gelu(u) : (u > 0.f ? u : 0.f);
}

// g * act'(u).  ReLU selects (it does not multiply): u <= 0 gives +0 whatever g holds, like the library's threshold_backward
template <int ACT>
__device__ __forceinline__ float act_grad(float u, float g) {
  return ACT == 1 ? g * gm_gelu_grad(u) : (u > 0.f ? g : 0.f);
}

// one 16-byte piece per thread (a grid-stride loop only beyond ACT_FWD_MAX_WG workgroups)
template <int ACT>
__global__ __launch_bounds__(256) void act_forward_kernel(const float* __restrict__ u, float* __restrict__ a, long n4) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
    const float4 v = reinterpret_cast<const float4*>(u)[i];
    reinterpret_cast<float4*>(a)[i] = make_float4(act_value<ACT>(v.x), act_value<ACT>(v.y), act_value<ACT>(v.z), act_value<ACT>(v.w));
  }
}

// g and du carry no __restrict__: they may be the same buffer (a lane reads its own four values of every row before it writes them)
template <int ACT, bool WANT_A, bool WANT_B>
__global__ __launch_bounds__(256) void act_backward_kernel(const float* __restrict__ u, const float* g, float* du, float* __restrict__ a,
                                                           float* __restrict__ ws, long rows, int N) {
  const int col = blockIdx.x * ACT_COLS + threadIdx.x * 4;
  if (col >= N) return;                                   // N % 4 == 0: a lane's four columns are all inside or all outside
  float sum[4] = {0.f, 0.f, 0.f, 0.f};
  for (long r0 = (long)blockIdx.y * ACT_ROWS; r0 < rows; r0 += (long)gridDim.y * ACT_ROWS) {
    float4 uv[ACT_ROWS], gv[ACT_ROWS];
#pragma unroll
    for (int k = 0; k < ACT_ROWS; ++k) {
      if (r0 + k < rows) {
        const long at = (r0 + k) * N + col;
        uv[k] = *reinterpret_cast<const float4*>(u + at);
        gv[k] = *reinterpret_cast<const float4*>(g + at);
      }
    }
#pragma unroll
    for (int k = 0; k < ACT_ROWS; ++k) {
      if (r0 + k < rows) {
        const long at = (r0 + k) * N + col;
        const float4 d = make_float4(act_grad<ACT>(uv[k].x, gv[k].x), act_grad<ACT>(uv[k].y, gv[k].y), act_grad<ACT>(uv[k].z, gv[k].z),
                                     act_grad<ACT>(uv[k].w, gv[k].w));
        *reinterpret_cast<float4*>(du + at) = d;
        if (WANT_A)
          *reinterpret_cast<float4*>(a + at) = make_float4(act_value<ACT>(uv[k].x), act_value<ACT>(uv[k].y), act_value<ACT>(uv[k].z),
                                                           act_value<ACT>(uv[k].w));
        if (WANT_B) { sum[0] += d.x; sum[1] += d.y; sum[2] += d.z; sum[3] += d.w; }
      }
    }
  }
  if (WANT_B) *reinterpret_cast<float4*>(ws + (long)blockIdx.y * N + col) = make_float4(sum[0], sum[1], sum[2], sum[3]);
}

static inline int act_col_tiles(int N) { return (N + ACT_COLS - 1) / ACT_COLS; }

// partial rows = workgroups along the rows
static inline int act_row_parts(int64_t rows, int N) {
  const int64_t want = (rows + ACT_ROWS - 1) / ACT_ROWS;
  const int most = ACT_MAX_WG / act_col_tiles(N) > 0 ? ACT_MAX_WG / act_col_tiles(N) : 1;
  return (int)(want < most ? want : most);
}

template <int ACT>
static void launch_act_bwd(bool want_a, bool want_b, dim3 grid, hipStream_t st, const float* u, const float* g, float* du, float* a, float* ws,
                           long rows, int N) {
  if (want_a && want_b) hipLaunchKernelGGL((act_backward_kernel<ACT, true, true>), grid, dim3(256), 0, st, u, g, du, a, ws, rows, N);
  else if (want_a) hipLaunchKernelGGL((act_backward_kernel<ACT, true, false>), grid, dim3(256), 0, st, u, g, du, a, ws, rows, N);
  else if (want_b) hipLaunchKernelGGL((act_backward_kernel<ACT, false, true>), grid, dim3(256), 0, st, u, g, du, a, ws, rows, N);
  else hipLaunchKernelGGL((act_backward_kernel<ACT, false, false>), grid, dim3(256), 0, st, u, g, du, a, ws, rows, N);
}

}  // namespace hipie

extern "C" int hipie_act_forward(const float* u, float* a, int64_t rows, int N, int act, void* stream) {
  using namespace hipie;
  HIPIE_REQUIRE(rows >= 0 && N >= 0 && N % 4 == 0, "act_forward: rows=%lld, N=%d: N must be a multiple of 4", (long long)rows, N);
  HIPIE_REQUIRE(act == 1 || act == 2, "act_forward: act=%d must be 1 (GELU) or 2 (ReLU)", act);
  if (rows == 0 || N == 0) return HIPIE_OK;
  HIPIE_REQUIRE(u && a, "act_forward: null pointer");
  HIPIE_REQUIRE((const float*)a != u, "act_forward: a must not alias u");
  HIPIE_REQUIRE((((uintptr_t)u | (uintptr_t)a) & 15) == 0, "act_forward: buffers must be 16-byte aligned");
  const long n4 = (long)rows * N / 4;
  const long want = (n4 + 255) / 256;
  const dim3 grid((unsigned)(want < ACT_FWD_MAX_WG ? want : ACT_FWD_MAX_WG));
  if (act == 1) hipLaunchKernelGGL(act_forward_kernel<1>, grid, dim3(256), 0, (hipStream_t)stream, u, a, n4);
  else hipLaunchKernelGGL(act_forward_kernel<2>, grid, dim3(256), 0, (hipStream_t)stream, u, a, n4);
  return check_launch("act_forward");
}

extern "C" int64_t hipie_act_backward_ws_bytes(int64_t rows, int N) {
  if (rows <= 0 || N <= 0) return 16;
  return (int64_t)hipie::act_row_parts(rows, N) * N * (int64_t)sizeof(float);
}

extern "C" int hipie_act_backward(const float* u, const float* g, float* du, float* a, float* dbias, void* ws, int64_t rows, int N, int act,
                                  void* stream) {
  using namespace hipie;
  HIPIE_REQUIRE(rows >= 0 && N >= 0 && N % 4 == 0, "act_backward: rows=%lld, N=%d: N must be a multiple of 4", (long long)rows, N);
  HIPIE_REQUIRE(act == 1 || act == 2, "act_backward: act=%d must be 1 (GELU) or 2 (ReLU)", act);
  HIPIE_REQUIRE(dbias == nullptr || ws != nullptr, "act_backward: dbias needs the workspace of hipie_act_backward_ws_bytes");
  hipStream_t st = (hipStream_t)stream;
  if (rows == 0 || N == 0) {
    if (dbias != nullptr && N > 0 && hipMemsetAsync(dbias, 0, (size_t)N * sizeof(float), st) != hipSuccess)
      return check_launch("act_backward (zero fill)");
    return HIPIE_OK;
  }
  HIPIE_REQUIRE(u && g && du, "act_backward: null pointer");
  HIPIE_REQUIRE((const float*)du != u && (a == nullptr || ((const float*)a != u && (const float*)a != g && a != du)),
                "act_backward: du must not alias u, a must not alias u, g or du (du may alias g)");
  HIPIE_REQUIRE((((uintptr_t)u | (uintptr_t)g | (uintptr_t)du | (uintptr_t)a | (uintptr_t)dbias | (uintptr_t)ws) & 15) == 0,
                "act_backward: buffers must be 16-byte aligned");
  const int parts = act_row_parts(rows, N);
  const dim3 grid((unsigned)act_col_tiles(N), (unsigned)parts);
  if (act == 1) launch_act_bwd<1>(a != nullptr, dbias != nullptr, grid, st, u, g, du, a, (float*)ws, (long)rows, N);
  else launch_act_bwd<2>(a != nullptr, dbias != nullptr, grid, st, u, g, du, a, (float*)ws, (long)rows, N);
  const int rc = check_launch("act_backward");
  if (rc != HIPIE_OK || dbias == nullptr) return rc;
  return partial_rows_sum<ACT_FIN_GROUPS, ACT_FIN_COLS>("act_backward (partial-row sum)", (const float*)ws, dbias, nullptr, N, parts, N, st);
}
