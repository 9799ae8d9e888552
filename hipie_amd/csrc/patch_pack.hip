// patch_pack.hip -- the map-to-rows pack of the training projections (functions.PatchConvFunction; the opt-in group "projections" of
// training/net.py): a convolution whose kernel equals its stride, and a transposed one, are linears over PATCH ROWS plus a layout change.
// hipie_patch_pack does the layout change once, as the producer of the GEMM operands: ONE pass over a 4-D fp32 map x of logical shape
// (B, C, H, W), given by its four element strides (NCHW-dense and channels-last maps are read in place), with the patch size k
// (H % k == 0, W % k == 0):
//   patch row   m = (b H/k + h) W/k + w                   M = B (H/k) (W/k)
//   column      n = c k^2 + i k + j                        N = C k^2        element x[b, c, h k + i, w k + j]
// the column order of weight.reshape(Cout, Cin k k) of a convolution and of weight.view(Cin, Cout k k) of a transposed one.  It writes, each
// unless NULL: the fp32 rows (M, N); the HL8 rows of s x (the bits of hipie_to_hl8, scale = s); the HL8 rows of (s x)^T with zero pad
// columns (the bits of hipie_to_hl8_t); the per-CHANNEL sums of the unscaled values (per-tile column sums in a workspace, added in tile
// order and, per channel, in column order: no floating-point atomic, the same bits on every call).  s = scale[0], the device block of
// hipie_grad_scale, or 1.
// A block handles a tile of 128 patch rows x 64 columns, the tile and the rotated LDS layout of half_pack.hip (element (r, c) in dword
// 64 r + ((c + 4 ((r >> 3) & 7)) & 63)).  The address of an element is rowoff(m) + coloff(n), so the map is walked in one of three ways:
//   ROWS    8 consecutive columns are contiguous in memory: a channels-last map with k = 1, an NCHW map with k % 8 == 0 (the 16 x 16 patch
//           embedding).  half_pack's walk: a thread loads 8 values of a row, writes the fp32 / HL8 rows from its registers and stages the
//           tile for the transposed store and the sums.
//   PIXELS  8 consecutive patch rows are contiguous: an NCHW map with k = 1 -- a channel's pixels ARE a row of the transposed operand, so
//           out_t is written from the registers, no transpose; only the image boundary (a group of rows may straddle two images: the
//           scalar walk) and the pad columns need care.  The tile is staged for the row outputs and the sums.  The lanes are those of
//           half_pack's transposing read, so the staging ds_write_b32 is its mirror: 32 different banks per 32-lane half.
//   GATHER  everything else (k = 2: the output gradient of the transposed convolutions): one scalar load per element, the lanes along
//           the direction that is contiguous in memory (j, then w, for NCHW; the channel for channels-last), all outputs from the tile.
// Loads are 16 bytes where the host found every address of the walk aligned (`vec`), scalar otherwise (an odd W makes NCHW rows unaligned).
// The row outputs of PIXELS / GATHER read the tile with ds_read_b128, the two 16-byte halves of a group of 8 columns in the order
// ((i >> 1) & 1, then the other): the 16 lanes of a ds_read_b128 lane group then hit 16 different 16-byte slots of the 256-byte bank row
// (tools/lds_swizzle_check.py enumerates this read and the PIXELS staging store).  Global stores are 16 bytes per lane, 8 lanes to a row
// piece of 128 (fp32) or 256 (HL8) bytes.
#include "wave.h"

namespace hipie {

constexpr int kPpRows = 128, kPpCols = 64;
enum { kPpModeRows = 0, kPpModePixels = 1, kPpModeGather = 2 };

struct PatchGeom {
  long sb, sc, sh, sw;        // element strides of the (B, C, H, W) map
  long M, rows_p;
  int Hp, Wp, k, N;           // patch grid, patch size, N = C k^2
  int vec;                    // every 16-byte load of the walk is aligned
  int order;                  // GATHER: 0 columns fastest, 1 (j, row, column group) for NCHW, 2 (channel, tap, row) for channels-last
};

__device__ __forceinline__ int pp_at(int r, int c) { return r * kPpCols + ((c + 4 * ((r >> 3) & 7)) & (kPpCols - 1)); }

__device__ __forceinline__ long pp_rowoff(const PatchGeom& g, long m) {
  const int hw = g.Hp * g.Wp, mi = (int)m;          // M < 2^31 (checked by the entry): 32-bit divisions
  const int b = mi / hw, rem = mi - b * hw, h = rem / g.Wp, w = rem - h * g.Wp;
  return b * g.sb + (long)h * g.k * g.sh + (long)w * g.k * g.sw;
}

__device__ __forceinline__ long pp_coloff(const PatchGeom& g, int n) {
  const int k2 = g.k * g.k, c = n / k2, t = n - c * k2, i = t / g.k, j = t - i * g.k;
  return c * g.sc + i * g.sh + j * g.sw;
}

__device__ __forceinline__ void pp_store_f32(float* dst, const float (&v)[8]) {
  *reinterpret_cast<float4*>(dst) = make_float4(v[0], v[1], v[2], v[3]);
  *reinterpret_cast<float4*>(dst + 4) = make_float4(v[4], v[5], v[6], v[7]);
}

// [8 hi | 8 lo] of s v: hl_split(v * s), the expression of to_hl8_kernel / to_hl8_t_kernel / grad_pack_kernel
__device__ __forceinline__ void pp_store_hl8(f16_t* dst, const float (&v)[8], float s) {
  f16x8 h, l;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    f16_t hh, ll;
    hl_split(v[e] * s, hh, ll);
    h[e] = hh;
    l[e] = ll;
  }
  *reinterpret_cast<f16x8*>(dst) = h;
  *reinterpret_cast<f16x8*>(dst + 8) = l;
}

// block (tr, tc): patch rows 128 tr .., columns 64 tc ..  scale / out_f / out_r / out_t / ws may each be null (kernel arguments: the
// branches and the barriers are uniform).  ws[tr][n] = the tile's column sum of the UNSCALED values in grad_pack_kernel's order: four runs
// of 32 rows in row order, then the four in run order.
template <int MODE>
__global__ __launch_bounds__(256) void patch_pack_kernel(const float* __restrict__ x, const PatchGeom g, const float* __restrict__ scale,
                                                         float* __restrict__ out_f, long ldf, f16_t* __restrict__ out_r, long ldo,
                                                         f16_t* __restrict__ out_t, long ldt, float* __restrict__ ws) {
  __shared__ __attribute__((aligned(16))) float tile[kPpRows * kPpCols];
  __shared__ float colp[4][kPpCols];
  const long r0 = (long)blockIdx.x * kPpRows;
  const int c0 = blockIdx.y * kPpCols;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float s = scale != nullptr ? scale[0] : 1.f;
  const bool want_rows = out_f != nullptr || out_r != nullptr;

  if (MODE == kPpModeRows) {
    const bool staged = out_t != nullptr || ws != nullptr;
#pragma unroll
    for (int it = 0; it < kPpRows * (kPpCols / 8) / 256; ++it) {       // unit = (row i, group q of 8 columns): 8 lanes read 256 B of a row
      const int u = tid + it * 256, i = u >> 3, q = u & 7;
      const long m = r0 + i;
      const int n = c0 + 8 * q;
      const bool in = m < g.M && n < g.N;                              // N % 8 == 0: a group is in or out
      float v[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = 0.f;
      if (in) {
        const float* p = x + pp_rowoff(g, m) + pp_coloff(g, n);
        if (g.vec) {
          const float4 a = *reinterpret_cast<const float4*>(p), b = *reinterpret_cast<const float4*>(p + 4);
          v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
        } else {
#pragma unroll
          for (int e = 0; e < 8; ++e) v[e] = p[e];
        }
        if (out_f != nullptr) pp_store_f32(out_f + m * ldf + n, v);
        if (out_r != nullptr) pp_store_hl8(out_r + m * ldo + 2 * n, v, s);
      }
      if (staged) {                                                    // half_pack's staging store: the half (q >> 2) first
        const bool sw = (q >> 2) & 1;
        *reinterpret_cast<float4*>(tile + pp_at(i, 8 * q + (sw ? 4 : 0))) =
            make_float4(sw ? v[4] : v[0], sw ? v[5] : v[1], sw ? v[6] : v[2], sw ? v[7] : v[3]);
        *reinterpret_cast<float4*>(tile + pp_at(i, 8 * q + (sw ? 0 : 4))) =
            make_float4(sw ? v[0] : v[4], sw ? v[1] : v[5], sw ? v[2] : v[6], sw ? v[3] : v[7]);
      }
    }
    if (!staged) return;
  } else if (MODE == kPpModePixels) {
    const bool staged = want_rows || ws != nullptr;
    const int q = (lane & 7) + 8 * (lane >> 5), cq = (lane >> 3) & 3;  // a 32-lane half: 8 row groups x 4 columns
    const long m = r0 + 8 * q;
#pragma unroll
    for (int it = 0; it < kPpCols / 16; ++it) {                        // unit = (column c, group q of 8 rows): 8 lanes read 256 B of a channel
      const int c = 4 * (4 * it + wave) + cq, n = c0 + c;
      float v[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = 0.f;
      if (n < g.N && m < g.M) {
        const float* p = x + pp_coloff(g, n);
        if (g.vec) {                                                   // M % 4 == 0 and no float4 straddles an image
          const float4 a = *reinterpret_cast<const float4*>(p + pp_rowoff(g, m));
          v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
          if (m + 4 < g.M) {
            const float4 b = *reinterpret_cast<const float4*>(p + pp_rowoff(g, m + 4));
            v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
          }
        } else {
#pragma unroll
          for (int e = 0; e < 8; ++e)
            if (m + e < g.M) v[e] = p[pp_rowoff(g, m + e)];
        }
      }
      if (out_t != nullptr && n < g.N && m < g.rows_p)                 // M <= m < rows_p: zeros
        pp_store_hl8(out_t + (long)n * ldt + 2 * m, v, s);
      if (staged) {
#pragma unroll
        for (int e = 0; e < 8; ++e) tile[pp_at(8 * q + e, c)] = v[e];
      }
    }
    if (!staged) return;
  } else {
    const int k = g.k, k2 = k * k;
    for (int u = tid; u < kPpRows * kPpCols; u += 256) {
      int r, c;
      if (g.order == 1) {                                              // u = j + k (r + 128 column group)
        const int t = u / k;
        r = t & (kPpRows - 1);
        c = (t >> 7) * k + (u - t * k);
      } else if (g.order == 2) {                                       // u = channel + (64 / k^2) (tap + k^2 r)
        const int ch = kPpCols / k2, t = u / ch;
        r = u >> 6;
        c = (u - t * ch) * k2 + (t - (t / k2) * k2);
      } else {
        r = u >> 6;
        c = u & (kPpCols - 1);
      }
      const long m = r0 + r;
      const int n = c0 + c;
      tile[pp_at(r, c)] = (m < g.M && n < g.N) ? x[pp_rowoff(g, m) + pp_coloff(g, n)] : 0.f;
    }
  }
  __syncthreads();

  if (MODE != kPpModeRows && want_rows) {
#pragma unroll
    for (int it = 0; it < kPpRows * (kPpCols / 8) / 256; ++it) {       // unit = (row i, group q of 8 columns)
      const int u = tid + it * 256, i = u >> 3, q = u & 7;
      const long m = r0 + i;
      const int n = c0 + 8 * q;
      if (m >= g.M || n >= g.N) continue;
      const bool sw = (i >> 1) & 1;
      const float4 first = *reinterpret_cast<const float4*>(tile + pp_at(i, 8 * q + (sw ? 4 : 0)));
      const float4 second = *reinterpret_cast<const float4*>(tile + pp_at(i, 8 * q + (sw ? 0 : 4)));
      const float4 a = sw ? second : first, b = sw ? first : second;
      const float v[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
      if (out_f != nullptr) pp_store_f32(out_f + m * ldf + n, v);
      if (out_r != nullptr) pp_store_hl8(out_r + m * ldo + 2 * n, v, s);
    }
  }
  if (MODE != kPpModePixels && out_t != nullptr) {                     // half_pack's transposing read
    const int q = (lane & 7) + 8 * (lane >> 5), cq = (lane >> 3) & 3;
    const long m = r0 + 8 * q;
#pragma unroll
    for (int it = 0; it < kPpCols / 16; ++it) {                        // unit = (output row c, group q of 8 patch rows)
      const int c = 4 * (4 * it + wave) + cq;
      float v[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = tile[pp_at(8 * q + e, c)];
      if (c0 + c < g.N && m < g.rows_p)                                // M <= m < rows_p: the tile holds zeros there
        pp_store_hl8(out_t + (long)(c0 + c) * ldt + 2 * m, v, s);
    }
  }
  if (ws != nullptr) {
    const int c = tid & (kPpCols - 1), q = tid >> 6;
    float a = 0.f;
    for (int i = 0; i < kPpRows / 4; ++i) a += tile[pp_at(q * (kPpRows / 4) + i, c)];
    colp[q][c] = a;
    __syncthreads();
    if (tid < kPpCols && c0 + c < g.N) ws[(long)blockIdx.x * g.N + c0 + c] = ((colp[0][c] + colp[1][c]) + colp[2][c]) + colp[3][c];
  }
}

// dsum[c] = the k^2 columns of channel c in column order, each the tiles' column sums in tile order
__global__ __launch_bounds__(256) void patch_sum_finish_kernel(const float* __restrict__ ws, long tiles, int N, int k2, int C, float* __restrict__ dsum) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= C) return;
  float total = 0.f;
  for (int t = 0; t < k2; ++t) {
    const int n = c * k2 + t;
    float a = ws[n];
    for (long tr = 1; tr < tiles; ++tr) a += ws[tr * N + n];
    total = t == 0 ? a : total + a;
  }
  dsum[c] = total;
}

static inline bool pp_aligned(const void* p) { return ((uintptr_t)p % 16) == 0; }

}  // namespace hipie

using namespace hipie;

extern "C" int64_t hipie_patch_pack_ws_bytes(int64_t rows_p, int N) {
  if (rows_p <= 0 || N <= 0) return 0;
  return (rows_p + kPpRows - 1) / kPpRows * (int64_t)N * 4;
}

extern "C" int hipie_patch_pack(const void* x, int B, int C, int H, int W, int64_t sb, int64_t sc, int64_t sh, int64_t sw, int k, const void* scale,
                                void* out_f32, int64_t ldf, void* out_rows, int64_t ldo, void* out_t, int64_t ldt, int64_t rows_p, void* dsum,
                                void* ws, int64_t ws_bytes, void* stream) {
  HIPIE_REQUIRE(x, "patch_pack: null pointer");
  HIPIE_REQUIRE(B > 0 && C > 0 && H > 0 && W > 0 && k > 0 && k <= 64, "patch_pack: map (%d, %d, %d, %d), k=%d (non-empty, 1 <= k <= 64)", B, C, H, W, k);
  HIPIE_REQUIRE(H % k == 0 && W % k == 0, "patch_pack: k=%d must divide H=%d and W=%d", k, H, W);
  const int64_t M = (int64_t)B * (H / k) * (W / k), N64 = (int64_t)C * k * k;
  HIPIE_REQUIRE(N64 % 8 == 0 && N64 < (1L << 22) && M < (1L << 31), "patch_pack: N=%ld (C k^2 must be a multiple of 8, below 2^22), M=%ld (below 2^31)",
                (long)N64, (long)M);
  const int N = (int)N64;
  HIPIE_REQUIRE(sw == 1 || sc == 1, "patch_pack: strides (%ld, %ld, %ld, %ld): the unit stride must be that of W or of C", (long)sb, (long)sc, (long)sh,
                (long)sw);
  HIPIE_REQUIRE(sb >= 0 && sc > 0 && sh > 0 && sw > 0, "patch_pack: strides (%ld, %ld, %ld, %ld) must be positive", (long)sb, (long)sc, (long)sh, (long)sw);
  HIPIE_REQUIRE(((uintptr_t)x % 4) == 0 && ((uintptr_t)scale % 4) == 0 && ((uintptr_t)dsum % 4) == 0 && ((uintptr_t)ws % 4) == 0,
                "patch_pack: x / scale / dsum / ws must be 4-byte aligned");
  if (out_f32 == nullptr && out_rows == nullptr && out_t == nullptr && dsum == nullptr) return HIPIE_OK;
  HIPIE_REQUIRE(rows_p >= M && rows_p % 32 == 0 && rows_p < (1L << 31), "patch_pack: rows_p=%ld (>= M=%ld, a multiple of 32)", (long)rows_p, (long)M);
  HIPIE_REQUIRE(out_f32 == nullptr || (ldf >= N && ldf % 4 == 0), "patch_pack: fp32 row stride %ld (>= N=%d, a multiple of 4)", (long)ldf, N);
  HIPIE_REQUIRE(out_rows == nullptr || (ldo >= 2 * (int64_t)N && ldo % 8 == 0), "patch_pack: row operand stride %ld (>= 2 N, a multiple of 8)", (long)ldo);
  HIPIE_REQUIRE(out_t == nullptr || (ldt >= 2 * rows_p && ldt % 8 == 0), "patch_pack: transposed operand stride %ld (>= 2 rows_p, a multiple of 8)",
                (long)ldt);
  HIPIE_REQUIRE(pp_aligned(out_f32) && pp_aligned(out_rows) && pp_aligned(out_t), "patch_pack: the outputs must be 16-byte aligned");
  HIPIE_REQUIRE((dsum == nullptr) == (ws == nullptr), "patch_pack: dsum and its workspace come together");
  const int64_t need = hipie_patch_pack_ws_bytes(rows_p, N);
  HIPIE_REQUIRE(ws == nullptr || ws_bytes >= need, "patch_pack: workspace of %ld bytes, need %ld", (long)ws_bytes, (long)need);
  const long tiles_r = (rows_p + kPpRows - 1) / kPpRows, tiles_c = (N + kPpCols - 1) / kPpCols;
  HIPIE_REQUIRE(tiles_c <= 65535, "patch_pack: N=%d too wide", N);

  PatchGeom g;
  g.sb = sb; g.sc = sc; g.sh = sh; g.sw = sw;
  g.M = M; g.rows_p = rows_p;
  g.Hp = H / k; g.Wp = W / k; g.k = k; g.N = N;
  g.vec = 0; g.order = 0;
  const bool base16 = pp_aligned(x);
  int mode;
  if (sc == 1 && k == 1) {                        // channels-last pixels are rows
    mode = kPpModeRows;
    g.vec = base16 && sb % 4 == 0 && sh % 4 == 0 && sw % 4 == 0;
  } else if (sw == 1 && k % 8 == 0) {             // 8 consecutive j of a patch line
    mode = kPpModeRows;
    g.vec = base16 && sb % 4 == 0 && sc % 4 == 0 && sh % 4 == 0;
  } else if (sw == 1 && k == 1) {                 // a channel's pixels are a row of the transposed operand
    mode = kPpModePixels;
    g.vec = base16 && sh == W && ((int64_t)H * W) % 4 == 0 && sb % 4 == 0 && sc % 4 == 0;
  } else {
    mode = kPpModeGather;
    g.order = (sw == 1 && kPpCols % k == 0) ? 1 : ((sc == 1 && kPpCols % (k * k) == 0) ? 2 : 0);
  }
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)tiles_r, (unsigned)tiles_c);
#define HIPIE_PP_LAUNCH(MODE_)                                                                                                                     \
  hipLaunchKernelGGL(patch_pack_kernel<MODE_>, grid, dim3(256), 0, st, (const float*)x, g, (const float*)scale, (float*)out_f32, (long)ldf, \
                     (f16_t*)out_rows, (long)ldo, (f16_t*)out_t, (long)ldt, (float*)ws)
  if (mode == kPpModeRows) HIPIE_PP_LAUNCH(kPpModeRows);
  else if (mode == kPpModePixels) HIPIE_PP_LAUNCH(kPpModePixels);
  else HIPIE_PP_LAUNCH(kPpModeGather);
#undef HIPIE_PP_LAUNCH
  if (dsum != nullptr)
    hipLaunchKernelGGL(patch_sum_finish_kernel, dim3((unsigned)((C + 255) / 256)), dim3(256), 0, st, (const float*)ws, tiles_r, N, k * k, C, (float*)dsum);
  return check_launch("patch_pack");
}
