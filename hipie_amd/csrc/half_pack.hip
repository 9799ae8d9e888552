// half_pack.hip -- the fp16 operands of the HALF-precision training linears (functions.HalfLinearFunction / HalfMlpFunction; the opt-in
// policy net.half_policy).  Arithmetic contract of a linear y = x . W^T + b the policy takes:
//   forward    x16 = fp16(x), W16 = fp16(W): round to nearest even, values beyond +-65504 saturate (as hl_split does), NO scale;
//              y = x16 . W16^T + b, ONE fp16 MFMA product, fp32 accumulation, fp32 output, the bias in the epilogue (hipie_gemm, HIPIE_F16)
//   backward   {s, 1 / s} = hipie_grad_scale(dy);  g16 = fp16(s dy) as rows and as (s dy)^T;  db = column sums of the UNSCALED dy;
//              dx = (1 / s) g16 . W16 (hipie_gemm_scaled, HIPIE_F16);  dW = (1 / s) g16^T . x16^T, the contraction over the token rows
//              (padded to 64: the F16 k tile), cut into chunks (hipie_gemm_batched_f16), added in chunk order (hipie_splitk_finish)
// Every scale factor is an exact power of two and every sum has a fixed order: the results for 2^e dy are 2^e times those for dy, bit for bit.
//   hipie_half_pack   ONE pass over x (rows, N), fp32 or fp16 rows: fp16 rows of s x, fp16 rows of (s x)^T with zero pad columns, column sums
//   hipie_act_half    a16 = fp16(act(u)) in one pass: the operand of the second linear of an MLP without an fp32 `a` in HBM
// Bandwidth kernels.  half_pack: a thread loads 8 consecutive values of a row (branch-free: clamped index, then select), writes the row
// operand from its registers and puts the fp32 values into a 128-row x 64-column LDS tile that the transposed store and the column sum
// read.  Element (r, c) of the tile lives in dword 64 r + ((c + 4 ((r >> 3) & 7)) & 63): the columns of a group of 8 rows are rotated by 4
// per group.  The transposing read -- a lane reads the 8 rows of group g at column c, ds_read_b32, banks (a / 4) mod 32 per 32-lane half --
// puts the 8 groups x 4 columns of a half on 4 (g & 7) + (c & 3) + const: 32 different banks (the unrotated [128][65] layout of
// to_hl8_t_kernel puts the groups g, g + 4, g + 8, g + 12 on one bank: 4-way; tools/lds_swizzle_check.py enumerates both).  Both global stores are 16 bytes
// per lane along the contiguous dimension: 8 lanes x 16 B of one row, 16 lanes x 16 B = 256 B of one transposed row.
#include "wave.h"
#include "gelu.h"

namespace hipie {

constexpr int kHpRows = 128, kHpCols = 64;

__device__ __forceinline__ int hp_at(int r, int c) { return r * kHpCols + ((c + 4 * ((r >> 3) & 7)) & (kHpCols - 1)); }

// fp16(x), round to nearest even, saturated at +-65504 like hl_split's hi
__device__ __forceinline__ f16_t hp_half(float x) { return (f16_t)__builtin_fminf(__builtin_fmaxf(x, -65504.f), 65504.f); }

__device__ __forceinline__ void hp_load8(const float* p, float (&v)[8]) {
  const float4 a = *reinterpret_cast<const float4*>(p), b = *reinterpret_cast<const float4*>(p + 4);
  v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
}
__device__ __forceinline__ void hp_load8(const f16_t* p, float (&v)[8]) {
  const f16x8 a = *reinterpret_cast<const f16x8*>(p);
#pragma unroll
  for (int e = 0; e < 8; ++e) v[e] = (float)a[e];
}

// block (tr, tc): rows 128 tr .., columns 64 tc .. of x.  scale / out_r / out_t / ws may each be null (kernel arguments: the branches and the
// barriers are uniform).  ws[tr][c] = the tile's column sum of the UNSCALED values in grad_pack_kernel's order: four runs of 32 rows in row
// order, then the four in run order.
template <typename T>
__global__ __launch_bounds__(256) void half_pack_kernel(const T* __restrict__ x, long ldx, const float* __restrict__ scale, f16_t* __restrict__ out_r,
                                                        long ldo, f16_t* __restrict__ out_t, long ldt, float* __restrict__ ws, long rows, int N,
                                                        long rows_p) {
  __shared__ __attribute__((aligned(16))) float tile[kHpRows * kHpCols];
  __shared__ float colp[4][kHpCols];
  const long r0 = (long)blockIdx.x * kHpRows;
  const int c0 = blockIdx.y * kHpCols;
  const int tid = threadIdx.x;
  const float s = scale != nullptr ? scale[0] : 1.f;
  const bool staged = out_t != nullptr || ws != nullptr;
#pragma unroll
  for (int it = 0; it < kHpRows * (kHpCols / 8) / 256; ++it) {         // unit = (row i, group g of 8 columns): 8 lanes read 256 B (fp32) of a row
    const int k = tid + it * 256, i = k >> 3, g = k & 7;
    const long r = r0 + i;
    const int c = c0 + 8 * g;
    const bool in = r < rows && c < N;                                 // N % 8 == 0: a group is in or out
    float v[8];
    hp_load8(x + (r < rows ? r : rows - 1) * ldx + (c < N ? c : N - 8), v);
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = in ? v[e] : 0.f;
    if (out_r != nullptr && in) {
      f16x8 h;
#pragma unroll
      for (int e = 0; e < 8; ++e) h[e] = hp_half(v[e] * s);
      *reinterpret_cast<f16x8*>(out_r + r * ldo + c) = h;
    }
    if (staged) {
      // the two 16-byte halves of the group in the order (g >> 2, then the other): the 8 lanes of a ds_write_b128 lane group hit 8 different
      // 4-bank slots of the 32 store banks (in the order 0, 1 lanes g and g + 4 share a slot)
      const bool sw = (g >> 2) & 1;
      const float4 first = make_float4(sw ? v[4] : v[0], sw ? v[5] : v[1], sw ? v[6] : v[2], sw ? v[7] : v[3]);
      const float4 second = make_float4(sw ? v[0] : v[4], sw ? v[1] : v[5], sw ? v[2] : v[6], sw ? v[3] : v[7]);
      *reinterpret_cast<float4*>(tile + hp_at(i, 8 * g + (sw ? 4 : 0))) = first;
      *reinterpret_cast<float4*>(tile + hp_at(i, 8 * g + (sw ? 0 : 4))) = second;
    }
  }
  if (!staged) return;
  __syncthreads();
  if (out_t != nullptr) {
    const int lane = tid & 63, wave = tid >> 6;
    const int g = (lane & 7) + 8 * (lane >> 5), cq = (lane >> 3) & 3;  // a 32-lane half: 8 row groups x 4 columns
    const long m = r0 + 8 * g;
#pragma unroll
    for (int it = 0; it < kHpCols / 16; ++it) {                        // unit = (output row c, group g of 8 source rows)
      const int c = 4 * (4 * it + wave) + cq;
      f16x8 h;
#pragma unroll
      for (int e = 0; e < 8; ++e) h[e] = hp_half(tile[hp_at(8 * g + e, c)] * s);
      if (c0 + c < N && m < rows_p)                                    // rows <= m < rows_p: the tile holds zeros there
        *reinterpret_cast<f16x8*>(out_t + (long)(c0 + c) * ldt + m) = h;
    }
  }
  if (ws != nullptr) {
    const int c = tid & (kHpCols - 1), q = tid >> 6;
    float a = 0.f;
    for (int i = 0; i < kHpRows / 4; ++i) a += tile[hp_at(q * (kHpRows / 4) + i, c)];
    colp[q][c] = a;
    __syncthreads();
    if (tid < kHpCols && c0 + c < N) ws[(long)blockIdx.x * N + c0 + c] = ((colp[0][c] + colp[1][c]) + colp[2][c]) + colp[3][c];
  }
}

// dbias[c] = the tiles' column sums in tile order
__global__ __launch_bounds__(256) void half_bias_finish_kernel(const float* __restrict__ ws, long tiles, int N, float* __restrict__ db) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= N) return;
  float a = ws[c];
  for (long t = 1; t < tiles; ++t) a += ws[t * N + c];
  db[c] = a;
}

// 8 values per thread: two 16-byte loads, one 16-byte store.  ACT 1: gm_gelu (gelu.h, the formula of act_forward_kernel), 2: ReLU
template <int ACT>
__global__ __launch_bounds__(256) void act_half_kernel(const float* __restrict__ u, f16_t* __restrict__ a, long n8) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n8; i += (long)gridDim.x * 256) {
    float v[8];
    hp_load8(u + 8 * i, v);
    f16x8 h;
#pragma unroll
    for (int e = 0; e < 8; ++e) h[e] = (f16_t)(ACT == 1 ? gm_gelu(v[e]) : (v[e] > 0.f ? v[e] : 0.f));
    reinterpret_cast<f16x8*>(a)[i] = h;
  }
}

static inline bool hp_aligned(const void* p) { return ((uintptr_t)p % 16) == 0; }

}  // namespace hipie

using namespace hipie;

extern "C" int64_t hipie_half_pack_ws_bytes(int64_t rows_p, int N) {
  if (rows_p <= 0 || N <= 0) return 0;
  return (rows_p + kHpRows - 1) / kHpRows * (int64_t)N * 4;
}

extern "C" int hipie_half_pack(const void* x, int64_t ldx, int x_fmt, const void* scale, void* out_rows, int64_t ldo, void* out_t, int64_t ldt,
                               void* dbias, void* ws, int64_t rows, int N, int64_t rows_p, void* stream) {
  HIPIE_REQUIRE(x, "half_pack: null pointer");
  HIPIE_REQUIRE(x_fmt == HIPIE_F32 || x_fmt == HIPIE_F16, "half_pack: input format %d (HIPIE_F32 | HIPIE_F16)", x_fmt);
  HIPIE_REQUIRE(rows > 0 && N > 0 && N % 8 == 0, "half_pack: rows=%ld N=%d (N must be a multiple of 8)", (long)rows, N);
  HIPIE_REQUIRE(rows_p >= rows && rows_p % 64 == 0, "half_pack: rows_p=%ld (>= rows=%ld, a multiple of 64)", (long)rows_p, (long)rows);
  const int per16 = x_fmt == HIPIE_F32 ? 4 : 8;
  HIPIE_REQUIRE(ldx >= N && ldx % per16 == 0, "half_pack: input row stride %ld (>= N, a multiple of %d)", (long)ldx, per16);
  HIPIE_REQUIRE(out_rows == nullptr || (ldo >= N && ldo % 8 == 0), "half_pack: row operand stride %ld (>= N, a multiple of 8)", (long)ldo);
  HIPIE_REQUIRE(out_t == nullptr || (ldt >= rows_p && ldt % 8 == 0), "half_pack: transposed operand stride %ld (>= rows_p, a multiple of 8)", (long)ldt);
  HIPIE_REQUIRE((dbias == nullptr) == (ws == nullptr), "half_pack: dbias and its workspace come together");
  HIPIE_REQUIRE(hp_aligned(x) && hp_aligned(out_rows) && hp_aligned(out_t) && ((uintptr_t)scale % 4) == 0 && ((uintptr_t)dbias % 4) == 0 &&
                ((uintptr_t)ws % 4) == 0, "half_pack: x and the operands must be 16-byte aligned, scale / dbias / ws 4-byte aligned");
  const long tiles_r = (rows_p + kHpRows - 1) / kHpRows, tiles_c = (N + kHpCols - 1) / kHpCols;
  HIPIE_REQUIRE(tiles_c <= 65535 && tiles_r < (1L << 31), "half_pack: N=%d too wide / too many rows", N);
  if (out_rows == nullptr && out_t == nullptr && dbias == nullptr) return 0;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)tiles_r, (unsigned)tiles_c);
  if (x_fmt == HIPIE_F32)
    hipLaunchKernelGGL(half_pack_kernel<float>, grid, dim3(256), 0, st, (const float*)x, (long)ldx, (const float*)scale, (f16_t*)out_rows, (long)ldo,
                       (f16_t*)out_t, (long)ldt, (float*)ws, (long)rows, N, (long)rows_p);
  else
    hipLaunchKernelGGL(half_pack_kernel<f16_t>, grid, dim3(256), 0, st, (const f16_t*)x, (long)ldx, (const float*)scale, (f16_t*)out_rows, (long)ldo,
                       (f16_t*)out_t, (long)ldt, (float*)ws, (long)rows, N, (long)rows_p);
  if (dbias != nullptr)
    hipLaunchKernelGGL(half_bias_finish_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, st, (const float*)ws, tiles_r, N, (float*)dbias);
  return check_launch("half_pack");
}

extern "C" int hipie_act_half(const void* u, void* a16, int64_t rows, int N, int act, void* stream) {
  HIPIE_REQUIRE(rows >= 0 && N >= 0 && N % 8 == 0, "act_half: rows=%ld N=%d (N must be a multiple of 8)", (long)rows, N);
  HIPIE_REQUIRE(act == 1 || act == 2, "act_half: act=%d must be 1 (GELU) or 2 (ReLU)", act);
  if (rows == 0 || N == 0) return HIPIE_OK;
  HIPIE_REQUIRE(u && a16, "act_half: null pointer");
  HIPIE_REQUIRE(hp_aligned(u) && hp_aligned(a16), "act_half: buffers must be 16-byte aligned");
  const long n8 = (long)rows * N / 8;
  const long want = (n8 + 255) / 256;
  const dim3 grid((unsigned)(want < (1L << 20) ? want : (1L << 20)));
  if (act == 1) hipLaunchKernelGGL(act_half_kernel<1>, grid, dim3(256), 0, (hipStream_t)stream, (const float*)u, (f16_t*)a16, n8);
  else hipLaunchKernelGGL(act_half_kernel<2>, grid, dim3(256), 0, (hipStream_t)stream, (const float*)u, (f16_t*)a16, n8);
  return check_launch("act_half");
}
