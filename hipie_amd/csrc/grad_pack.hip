// grad_pack.hip -- scaled gradient operands of the training linears (functions.ScaledSplitLinearFunction / ScaledMlpFunction): the output
// gradient dy of a Linear enters two split-fp16 products (dx = dy . W and dW = dy^T . x) as hi = fp16(dy), lo = fp16(dy - hi), which is
// 2^-22 accurate only while dy is a NORMAL fp16 number: below 6.1e-5 the pair loses bits, below 6e-8 it is zero, above 65504 it saturates.
// Here dy is multiplied by a power of two s chosen on the device from its largest magnitude before it is split, and the products are
// multiplied by 1 / s where they are written (GemmParams::alpha_dev, splitk_finish_kernel): every factor is an exact power of two, nothing
// waits for the host, no floating-point atomic, the same bits on every call.
//   hipie_grad_scale      dy -> {s, 1 / s}: s = 2^e with amax * 2^e in [2^14, 2^15)
//   hipie_grad_pack       ONE pass over dy: the HL8 rows of s dy (A operand of dx), the HL8 rows of (s dy)^T (operand of dW), db = sum_m dy
//   hipie_splitk_finish   sum of the split-K partial products in chunk order, times the device scalar
// Bandwidth kernels: a 128-row x 64-column tile of dy goes through LDS once and leaves three times, 16-byte stores on both operands.
#include "wave.h"

namespace hipie {

// max |x| as an INTEGER maximum of the bit patterns without their sign: the order of non-negative floats is the order of their bits, a
// NaN sorts above inf (fmaxf would drop it), and an integer maximum does not depend on the order it is taken in
__global__ __launch_bounds__(256) void grad_amax_kernel(const float* __restrict__ x, long ldx, long rows, int n4, unsigned int* __restrict__ out) {
  __shared__ int part[4];
  const long total = rows * n4;
  int m = 0;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const long r = i / n4;
    const int c = (int)(i - r * n4);
    const uint4 v = *reinterpret_cast<const uint4*>(x + r * ldx + 4 * c);
    m = max(max(m, (int)(v.x & 0x7fffffffu)), (int)(v.y & 0x7fffffffu));
    m = max(max(m, (int)(v.z & 0x7fffffffu)), (int)(v.w & 0x7fffffffu));
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) m = max(m, __shfl_xor(m, off));
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) atomicMax(out, (unsigned int)max(max(part[0], part[1]), max(part[2], part[3])));
}

// the bits of amax (blk[0]) -> blk = {s, 1 / s}.  e from the exponent FIELD (a subnormal amax: from its leading bit), clamped to +-126 so
// that both floats are normal; amax == 0, inf or NaN: {1, 1}
__global__ void grad_scale_finish_kernel(unsigned int* __restrict__ blk) {
  const unsigned int b = blk[0];
  const int field = (int)(b >> 23);
  int e = 0;
  if (b != 0u && field != 255) {
    const int E = field ? field - 127 : (31 - __clz((int)b)) - 149;        // amax in [2^E, 2^(E+1))
    e = min(max(14 - E, -126), 126);
  }
  blk[0] = (unsigned int)(127 + e) << 23;
  blk[1] = (unsigned int)(127 - e) << 23;
}

constexpr int kGpRows = 128, kGpCols = 64;

// block (tr, tc): rows 128 tr .., columns 64 tc .. of dy.  out_r / out_t / ws may each be null.  The split is hl_split(dy * s), the
// expression of to_hl8_kernel and to_hl8_t_kernel (gemm.hip): the same bits.  ws[tr][c] = the tile's column sum of the UNSCALED values:
// four runs of 32 rows in row order, then the four in run order.
__global__ __launch_bounds__(256) void grad_pack_kernel(const float* __restrict__ dy, long ldx, const float* __restrict__ scale,
                                                        f16_t* __restrict__ out_r, long ldo, f16_t* __restrict__ out_t, long ldt,
                                                        float* __restrict__ ws, long rows, int N, long rows_p) {
  __shared__ float tile[kGpRows][kGpCols + 1];
  __shared__ float colp[4][kGpCols];
  const long r0 = (long)blockIdx.x * kGpRows;
  const int c0 = blockIdx.y * kGpCols;
  const int tid = threadIdx.x;
  const float s = scale[0];
  for (int k = tid; k < kGpRows * (kGpCols / 4); k += 256) {           // coalesced along the columns; N % 8 == 0: a float4 is in or out
    const int i = k / (kGpCols / 4), j = (k % (kGpCols / 4)) * 4;
    float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
    if (r0 + i < rows && c0 + j < N) q = *reinterpret_cast<const float4*>(dy + (r0 + i) * ldx + c0 + j);
    tile[i][j] = q.x; tile[i][j + 1] = q.y; tile[i][j + 2] = q.z; tile[i][j + 3] = q.w;
  }
  __syncthreads();
  if (out_r != nullptr) {
    for (int u = tid; u < kGpRows * (kGpCols / 8); u += 256) {         // unit = (row i, group of 8 columns): 32 contiguous bytes of an HL8 row
      const int g = u % (kGpCols / 8), i = u / (kGpCols / 8);
      if (r0 + i >= rows || c0 + 8 * g >= N) continue;
      f16x8 h, l;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        f16_t hh, ll;
        hl_split(tile[i][8 * g + e] * s, hh, ll);
        h[e] = hh;
        l[e] = ll;
      }
      f16_t* dst = out_r + (r0 + i) * ldo + 2 * (c0 + 8 * g);
      *reinterpret_cast<f16x8*>(dst) = h;
      *reinterpret_cast<f16x8*>(dst + 8) = l;
    }
  }
  if (out_t != nullptr) {
    for (int u = tid; u < kGpCols * (kGpRows / 8); u += 256) {         // unit = (output row c, group of 8 source rows), as to_hl8_t_kernel
      const int g = u % (kGpRows / 8), c = u / (kGpRows / 8);
      const long m = r0 + 8 * g;
      if (c0 + c >= N || m >= rows_p) continue;                        // rows <= m < rows_p: the tile holds zeros there
      f16x8 h, l;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        f16_t hh, ll;
        hl_split(tile[8 * g + e][c] * s, hh, ll);
        h[e] = hh;
        l[e] = ll;
      }
      f16_t* dst = out_t + (long)(c0 + c) * ldt + 2 * m;
      *reinterpret_cast<f16x8*>(dst) = h;
      *reinterpret_cast<f16x8*>(dst + 8) = l;
    }
  }
  if (ws != nullptr) {                                                 // kernel argument: the barrier below is uniform
    const int c = tid & (kGpCols - 1), q = tid >> 6;
    float a = 0.f;
    for (int i = 0; i < kGpRows / 4; ++i) a += tile[q * (kGpRows / 4) + i][c];
    colp[q][c] = a;
    __syncthreads();
    if (tid < kGpCols && c0 + c < N) ws[(long)blockIdx.x * N + c0 + c] = ((colp[0][c] + colp[1][c]) + colp[2][c]) + colp[3][c];
  }
}

// db[c] = the tiles' column sums in tile order
__global__ __launch_bounds__(256) void grad_bias_finish_kernel(const float* __restrict__ ws, long tiles, int N, float* __restrict__ db) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= N) return;
  float a = ws[c];
  for (long t = 1; t < tiles; ++t) a += ws[t * N + c];
  db[c] = a;
}

// out = (part[0] + part[1] + ... + part[nk - 1]) * alpha, four elements per thread; the partial products of ONE batched launch in chunk order
__global__ __launch_bounds__(256) void splitk_finish_kernel(const float4* __restrict__ part, int nk, long n4, const float* __restrict__ alpha_dev,
                                                            float4* __restrict__ out) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n4) return;
  const float a = alpha_dev != nullptr ? *alpha_dev : 1.f;
  float4 acc = part[i];
  for (int k = 1; k < nk; ++k) {
    const float4 v = part[(long)k * n4 + i];
    acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
  }
  out[i] = make_float4(acc.x * a, acc.y * a, acc.z * a, acc.w * a);
}

static inline bool gp_aligned(const void* p) { return ((uintptr_t)p % 16) == 0; }

}  // namespace hipie

using namespace hipie;

extern "C" int hipie_grad_scale(const void* x, int64_t ldx, int64_t rows, int N, void* scale, void* stream) {
  HIPIE_REQUIRE(x && scale, "grad_scale: null pointer");
  HIPIE_REQUIRE(rows > 0 && N > 0 && N % 4 == 0 && ldx >= N && ldx % 4 == 0 && rows * (int64_t)N < (1L << 40),
                "grad_scale: rows=%ld N=%d ldx=%ld (N and the row stride multiples of 4)", (long)rows, N, (long)ldx);
  HIPIE_REQUIRE(gp_aligned(x) && ((uintptr_t)scale % 8) == 0, "grad_scale: x must be 16-byte aligned, the scale block 8-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(scale, 0, 8, st) != hipSuccess) return check_launch("grad_scale");
  const long total = rows * (N / 4);
  const unsigned blocks = (unsigned)(total / 1024 + 1 < 2048 ? total / 1024 + 1 : 2048);        // at least 4 float4 per thread
  hipLaunchKernelGGL(grad_amax_kernel, dim3(blocks), dim3(256), 0, st, (const float*)x, (long)ldx, (long)rows, N / 4, (unsigned int*)scale);
  hipLaunchKernelGGL(grad_scale_finish_kernel, dim3(1), dim3(1), 0, st, (unsigned int*)scale);
  return check_launch("grad_scale");
}

extern "C" int64_t hipie_grad_pack_ws_bytes(int64_t rows_p, int N) {
  if (rows_p <= 0 || N <= 0) return 0;
  return (rows_p + kGpRows - 1) / kGpRows * (int64_t)N * 4;
}

extern "C" int hipie_grad_pack(const void* dy, int64_t ldx, const void* scale, void* out_rows, int64_t ldo, void* out_t, int64_t ldt, void* dbias,
                               void* ws, int64_t rows, int N, int64_t rows_p, void* stream) {
  HIPIE_REQUIRE(dy && scale, "grad_pack: null pointer");
  HIPIE_REQUIRE(rows > 0 && N > 0 && N % 8 == 0, "grad_pack: rows=%ld N=%d (N must be a multiple of 8)", (long)rows, N);
  HIPIE_REQUIRE(rows_p >= rows && rows_p % 32 == 0, "grad_pack: rows_p=%ld (>= rows=%ld, a multiple of 32)", (long)rows_p, (long)rows);
  HIPIE_REQUIRE(ldx >= N && ldx % 4 == 0, "grad_pack: dy row stride %ld (>= N, a multiple of 4)", (long)ldx);
  HIPIE_REQUIRE(out_rows == nullptr || (ldo >= 2 * (int64_t)N && ldo % 8 == 0), "grad_pack: row operand stride %ld (>= 2 N, a multiple of 8)", (long)ldo);
  HIPIE_REQUIRE(out_t == nullptr || (ldt >= 2 * rows_p && ldt % 8 == 0), "grad_pack: transposed operand stride %ld (>= 2 rows_p, a multiple of 8)",
                (long)ldt);
  HIPIE_REQUIRE((dbias == nullptr) == (ws == nullptr), "grad_pack: dbias and its workspace come together");
  HIPIE_REQUIRE(gp_aligned(dy) && gp_aligned(out_rows) && gp_aligned(out_t) && ((uintptr_t)scale % 4) == 0 && ((uintptr_t)dbias % 4) == 0 &&
                ((uintptr_t)ws % 4) == 0, "grad_pack: dy and the operands must be 16-byte aligned, scale / dbias / ws 4-byte aligned");
  const long tiles_r = (rows_p + kGpRows - 1) / kGpRows, tiles_c = (N + kGpCols - 1) / kGpCols;
  HIPIE_REQUIRE(tiles_c <= 65535 && tiles_r < (1L << 31), "grad_pack: N=%d too wide / too many rows", N);
  if (out_rows == nullptr && out_t == nullptr && dbias == nullptr) return 0;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(grad_pack_kernel, dim3((unsigned)tiles_r, (unsigned)tiles_c), dim3(256), 0, st, (const float*)dy, (long)ldx, (const float*)scale,
                     (f16_t*)out_rows, (long)ldo, (f16_t*)out_t, (long)ldt, (float*)ws, (long)rows, N, (long)rows_p);
  if (dbias != nullptr)
    hipLaunchKernelGGL(grad_bias_finish_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, st, (const float*)ws, tiles_r, N, (float*)dbias);
  return check_launch("grad_pack");
}

extern "C" int hipie_splitk_finish(const void* part, int nk, int64_t n, const float* alpha_dev, void* out, void* stream) {
  HIPIE_REQUIRE(part && out, "splitk_finish: null pointer");
  HIPIE_REQUIRE(nk > 0 && nk <= 64 && n > 0 && n % 4 == 0, "splitk_finish: nk=%d n=%ld (1..64 partial products of a multiple of 4 elements)", nk, (long)n);
  HIPIE_REQUIRE(gp_aligned(part) && gp_aligned(out) && ((uintptr_t)alpha_dev % 4) == 0, "splitk_finish: part / out must be 16-byte aligned");
  const long n4 = n / 4;
  hipLaunchKernelGGL(splitk_finish_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const float4*)part, nk, n4, alpha_dev,
                     (float4*)out);
  return check_launch("splitk_finish");
}
