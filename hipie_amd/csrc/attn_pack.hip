// attn_pack.hip -- the operand pack / unpack passes around the fused training attention (attn_train.hip, attn_train_win.hip) of a ViT block:
// qkv rows (B', N, 3 heads 80) -> the fp16 planes of q' / k' / v and the head-major q; the gradient of the token-major output -> the planes
// of dO and v, delta and the power-of-two range of dO; dq' / dk / dv and the rel-pos terms -> d(qkv), written once.  Bandwidth kernels: the
// 80-float segment of a head is contiguous on both sides of the token-major <-> head-major change, so every thread moves 8 (or 4)
// consecutive columns with 16-byte accesses and nothing goes through LDS.  The planes carry the bits hipie_to_f16_pair gives (hl_split).
#include "wave.h"

namespace hipie {

constexpr int AP_HD = 80;            // head width: 10 chunks of 8 columns, 20 float4

struct ApRel {                       // a (BH, H, W, K) rel-pos operand as the library product left it: element strides, K stride included
  const float* p;
  long sb, sh, sw, sk;
};

struct ApTerm {                      // a (BH, H, W, 80) gradient term, 80 contiguous floats per token: element strides of the other three
  const float* p;
  long sb, sh, sw;
};

__device__ __forceinline__ void ap_load8(const float* p, float (&x)[8]) {
  const float4 a = *reinterpret_cast<const float4*>(p), b = *reinterpret_cast<const float4*>(p + 4);
  x[0] = a.x; x[1] = a.y; x[2] = a.z; x[3] = a.w; x[4] = b.x; x[5] = b.y; x[6] = b.z; x[7] = b.w;
}

__device__ __forceinline__ void ap_store_pair(f16_t* hi, f16_t* lo, long at, const float (&x)[8]) {
  f16x8 h, l;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    f16_t hh, ll;
    hl_split(x[e], hh, ll);
    h[e] = hh;
    l[e] = ll;
  }
  *reinterpret_cast<f16x8*>(hi + at) = h;
  *reinterpret_cast<f16x8*>(lo + at) = l;
}

// one thread per 8-column chunk; per (head, row < Np): cols / 8 chunks of k', 10 of v, 10 of the head-major q
__global__ __launch_bounds__(256) void ap_pack_kv_kernel(const float* __restrict__ qkv, float* __restrict__ rq, f16_t* __restrict__ k_hi,
                                                         f16_t* __restrict__ k_lo, f16_t* __restrict__ v_hi, f16_t* __restrict__ v_lo, int heads,
                                                         int H, int W, int Np, int cols, long total) {
  const long gid = (long)blockIdx.x * 256 + threadIdx.x;
  if (gid >= total) return;
  const int N = H * W, kc = cols / 8, per = kc + 20;
  const long row = gid / per;                                   // bh * Np + n
  const int item = (int)(gid - row * per);
  const long bh = row / Np;
  const int n = (int)(row - bh * Np);
  const long b = bh / heads;
  const int h = (int)(bh - b * heads);
  const bool real = n < N;
  const float* tok = qkv + ((b * N + n) * 3 * heads + h) * AP_HD;            // q of this (token, head); k: + heads * 80, v: + 2 heads * 80
  float x[8];
  if (item < kc) {
    const int c0 = item * 8, cq = AP_HD + H + W;
    if (real && c0 < AP_HD) {
      ap_load8(tok + (long)heads * AP_HD + c0, x);
    } else {
      const int kh = AP_HD + n / W, kw = AP_HD + H + n % W;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int c = c0 + e;
        x[e] = real ? ((c == kh || c == kw) ? 1.f : 0.f) : ((c == cq && Np != N) ? -30000.f : 0.f);
      }
    }
    ap_store_pair(k_hi, k_lo, row * cols + c0, x);
  } else if (item < kc + 10) {
    const int c0 = (item - kc) * 8;
    if (real) {
      ap_load8(tok + 2L * heads * AP_HD + c0, x);
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) x[e] = 0.f;
    }
    ap_store_pair(v_hi, v_lo, row * AP_HD + c0, x);
  } else if (real) {
    const int c0 = (item - kc - 10) * 8;
    float* dst = rq + (bh * N + n) * AP_HD + c0;
    *reinterpret_cast<float4*>(dst) = *reinterpret_cast<const float4*>(tok + c0);
    *reinterpret_cast<float4*>(dst + 4) = *reinterpret_cast<const float4*>(tok + c0 + 4);
  }
}

// one thread per 8-column chunk of q' = [rq * qscale | rel_h | rel_w | 1 on real rows of the padded form | 0..]
__global__ __launch_bounds__(256) void ap_pack_q_kernel(const float* __restrict__ rq, ApRel rh, ApRel rw, f16_t* __restrict__ q_hi,
                                                        f16_t* __restrict__ q_lo, int H, int W, int Np, int cols, float qscale, long total) {
  const long gid = (long)blockIdx.x * 256 + threadIdx.x;
  if (gid >= total) return;
  const int N = H * W, kc = cols / 8;
  const long row = gid / kc;
  const int c0 = (int)(gid - row * kc) * 8;
  const long bh = row / Np;
  const int n = (int)(row - bh * Np);
  float x[8];
  if (n >= N) {
#pragma unroll
    for (int e = 0; e < 8; ++e) x[e] = 0.f;
  } else if (c0 < AP_HD) {
    ap_load8(rq + (bh * N + n) * AP_HD + c0, x);
#pragma unroll
    for (int e = 0; e < 8; ++e) x[e] *= qscale;
  } else {
    const int qh = n / W, qw = n - qh * W, cq = AP_HD + H + W;
    const float* ph = rh.p + bh * rh.sb + qh * rh.sh + qw * rh.sw;
    const float* pw = rw.p + bh * rw.sb + qh * rw.sh + qw * rw.sw;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int c = c0 + e - AP_HD;
      x[e] = c < H ? ph[c * rh.sk] : c < H + W ? pw[(c - H) * rw.sk] : (c == H + W && Np != N) ? 1.f : 0.f;
    }
  }
  ap_store_pair(q_hi, q_lo, row * cols + c0, x);
}

// max |x| over n4 float4: the maximum of non-negative floats is the maximum of their bit patterns, so one atomicMax per workgroup on a
// zeroed word gives the same float whatever the order.  NaN entries are dropped (fmaxf), where torch's amax would propagate them.
__global__ __launch_bounds__(256) void ap_amax_kernel(const float4* __restrict__ x, long n4, unsigned int* __restrict__ out) {
  __shared__ float part[4];
  float m = 0.f;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
    const float4 v = x[i];
    m = fmaxf(fmaxf(m, fmaxf(fabsf(v.x), fabsf(v.y))), fmaxf(fabsf(v.z), fabsf(v.w)));
  }
  m = wave_max(m);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) atomicMax(out, __float_as_uint(fmaxf(fmaxf(part[0], part[1]), fmaxf(part[2], part[3]))));
}

// 16 lanes per (head, row < Np): lanes 0..9 take 8 columns of dO (token-major), out and v each, lanes 10 and 11 the zero columns 80..95;
// delta = scale * sum_c dO * out: 8 products per lane in column order, then the xor butterfly of wave_sum cut to the 16 lanes of a row (four
// rows share a wave) -- a fixed order
__global__ __launch_bounds__(256) void ap_pack_grad_kernel(const float* __restrict__ go, const float* __restrict__ out, const f16_t* __restrict__ v_hi,
                                                           const f16_t* __restrict__ v_lo, const float* __restrict__ scale, f16_t* __restrict__ do_hi,
                                                           f16_t* __restrict__ do_lo, f16_t* __restrict__ w_hi, f16_t* __restrict__ w_lo,
                                                           float* __restrict__ delta, int heads, int H, int W, int Np, long rows) {
  const long gid = (long)blockIdx.x * 256 + threadIdx.x;
  const long row = gid >> 4;                                    // bh * Np + n
  const int lane = (int)(gid & 15), c0 = lane * 8, N = H * W;
  const bool live = row < rows && lane < 12;
  const float sc = *scale;
  float part = 0.f;
  if (live) {
    const long bh = row / Np;
    const int n = (int)(row - bh * Np);
    const long b = bh / heads;
    const int h = (int)(bh - b * heads);
    float g[8];
    f16x8 vh, vl;
#pragma unroll
    for (int e = 0; e < 8; ++e) g[e] = 0.f, vh[e] = (f16_t)0.f, vl[e] = (f16_t)0.f;
    if (lane < 10) {
      vh = *reinterpret_cast<const f16x8*>(v_hi + row * AP_HD + c0);
      vl = *reinterpret_cast<const f16x8*>(v_lo + row * AP_HD + c0);
      if (n < N) {
        float o[8];
        ap_load8(go + ((b * N + n) * heads + h) * AP_HD + c0, g);
        ap_load8(out + row * AP_HD + c0, o);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          part += g[e] * o[e];
          g[e] *= sc;
        }
      }
    }
    ap_store_pair(do_hi, do_lo, row * 96 + c0, g);
    *reinterpret_cast<f16x8*>(w_hi + row * 96 + c0) = vh;
    *reinterpret_cast<f16x8*>(w_lo + row * 96 + c0) = vl;
  }
#pragma unroll
  for (int o = 8; o > 0; o >>= 1) part += __shfl_xor(part, o);
  if (live && lane == 0) delta[row] = part * sc;
}

// one thread per float4 of d(qkv) (B', N, 3, heads, 80): the address is 4 * gid
__global__ __launch_bounds__(256) void ap_unpack_grad_kernel(const float* __restrict__ dq, const float* __restrict__ dk, const float* __restrict__ dv,
                                                             ApTerm th, ApTerm tw, const float* __restrict__ inv, float* __restrict__ dqkv, int heads,
                                                             int H, int W, int Np, int cols, float qscale, long total) {
  const long gid = (long)blockIdx.x * 256 + threadIdx.x;
  if (gid >= total) return;
  const int N = H * W;
  const long seg = gid / 20;                                    // ((b * N + n) * 3 + s) * heads + h
  const int c0 = (int)(gid - seg * 20) * 4;
  const long t3 = seg / heads;
  const int h = (int)(seg - t3 * heads);
  const long tokn = t3 / 3;
  const int s = (int)(t3 - tokn * 3);
  const long b = tokn / N;
  const int n = (int)(tokn - b * N);
  const long bh = b * heads + h, row = bh * Np + n;
  const float iv = *inv;
  float4 r;
  if (s == 0) {
    r = *reinterpret_cast<const float4*>(dq + row * cols + c0);
    r.x *= qscale; r.y *= qscale; r.z *= qscale; r.w *= qscale;
    const int qh = n / W, qw = n - qh * W;
    const float4 a = *reinterpret_cast<const float4*>(th.p + bh * th.sb + qh * th.sh + qw * th.sw + c0);
    r.x += a.x; r.y += a.y; r.z += a.z; r.w += a.w;
    if (tw.p) {
      const float4 c = *reinterpret_cast<const float4*>(tw.p + bh * tw.sb + qh * tw.sh + qw * tw.sw + c0);
      r.x += c.x; r.y += c.y; r.z += c.z; r.w += c.w;
    }
  } else {
    r = *reinterpret_cast<const float4*>((s == 1 ? dk : dv) + row * AP_HD + c0);
  }
  r.x *= iv; r.y *= iv; r.z *= iv; r.w *= iv;
  *reinterpret_cast<float4*>(dqkv + gid * 4) = r;
}

}  // namespace hipie

using namespace hipie;

static bool ap_aligned(const void* p) { return ((uintptr_t)p % 16) == 0; }

// the geometry every entry shares: B' images or windows, heads, an H x W grid (N = H W rows per item), Np rows per item in the planes
// (N, or N rounded up to 128: the padded form), cols operand columns (has_cols: the entry has them)
static int ap_check(const char* who, bool pointers, bool aligned, int B, int heads, int H, int W, int Np, int cols, bool has_cols = true) {
  HIPIE_REQUIRE(pointers, "%s: null pointer", who);
  HIPIE_REQUIRE(B > 0 && heads > 0 && H > 0 && W > 0 && H <= 4096 && W <= 4096 && (long)B * heads < (1L << 24), "%s: B=%d heads=%d H=%d W=%d", who, B,
                heads, H, W);
  const int N = H * W, Nr = (N + 127) / 128 * 128;
  HIPIE_REQUIRE(Np == N || Np == Nr, "%s: Np=%d is neither N=%d nor N rounded up to 128 (%d)", who, Np, N, Nr);
  HIPIE_REQUIRE((long)B * heads * Np < (1L << 32), "%s: B * heads * Np = %ld rows (at most 2^32)", who, (long)B * heads * Np);     // 64 threads per row at most
  if (has_cols) {
    HIPIE_REQUIRE(cols == 224 || cols == 128, "%s: cols=%d (224: the global instance, 128: the windows)", who, cols);
    HIPIE_REQUIRE(AP_HD + H + W + (Np != N ? 1 : 0) <= cols, "%s: 80+H+W%s = %d operand columns > cols=%d (H=%d W=%d)", who, Np != N ? "+1" : "",
                  AP_HD + H + W + (Np != N ? 1 : 0), cols, H, W);
  }
  HIPIE_REQUIRE(aligned, "%s: every operand must be 16-byte aligned", who);
  return 0;
}

static unsigned ap_blocks(long threads) { return (unsigned)((threads + 255) / 256); }

extern "C" int hipie_attn_pack_kv(const void* qkv, void* rq, void* k_hi, void* k_lo, void* v_hi, void* v_lo, int B, int heads, int H, int W, int Np,
                                  int cols, void* stream) {
  HIPIE_TRY(ap_check("attn_pack_kv", qkv && rq && k_hi && k_lo && v_hi && v_lo,
                     ap_aligned(qkv) && ap_aligned(rq) && ap_aligned(k_hi) && ap_aligned(k_lo) && ap_aligned(v_hi) && ap_aligned(v_lo), B, heads, H, W,
                     Np, cols));
  const long total = (long)B * heads * Np * (cols / 8 + 20);
  hipLaunchKernelGGL(ap_pack_kv_kernel, dim3(ap_blocks(total)), dim3(256), 0, (hipStream_t)stream, (const float*)qkv, (float*)rq, (f16_t*)k_hi,
                     (f16_t*)k_lo, (f16_t*)v_hi, (f16_t*)v_lo, heads, H, W, Np, cols, total);
  return check_launch("attn_pack_kv");
}

extern "C" int hipie_attn_pack_q(const void* rq, const void* rel_h, int64_t hs_b, int64_t hs_h, int64_t hs_w, int64_t hs_k, const void* rel_w,
                                 int64_t ws_b, int64_t ws_h, int64_t ws_w, int64_t ws_k, void* q_hi, void* q_lo, int B, int heads, int H, int W, int Np,
                                 int cols, float qscale, void* stream) {
  HIPIE_TRY(ap_check("attn_pack_q", rq && rel_h && rel_w && q_hi && q_lo, ap_aligned(rq) && ap_aligned(q_hi) && ap_aligned(q_lo), B, heads, H, W, Np,
                     cols));
  HIPIE_REQUIRE(hs_b >= 0 && hs_h >= 0 && hs_w >= 0 && hs_k >= 0 && ws_b >= 0 && ws_h >= 0 && ws_w >= 0 && ws_k >= 0,
                "attn_pack_q: negative rel-pos stride");
  const long total = (long)B * heads * Np * (cols / 8);
  const ApRel rh{(const float*)rel_h, (long)hs_b, (long)hs_h, (long)hs_w, (long)hs_k}, rw{(const float*)rel_w, (long)ws_b, (long)ws_h, (long)ws_w, (long)ws_k};
  hipLaunchKernelGGL(ap_pack_q_kernel, dim3(ap_blocks(total)), dim3(256), 0, (hipStream_t)stream, (const float*)rq, rh, rw, (f16_t*)q_hi, (f16_t*)q_lo,
                     H, W, Np, cols, qscale, total);
  return check_launch("attn_pack_q");
}

extern "C" int hipie_attn_grad_amax(const void* go, int64_t n, void* amax, void* stream) {
  HIPIE_REQUIRE(go && amax, "attn_grad_amax: null pointer");
  HIPIE_REQUIRE(n > 0 && n % 4 == 0 && n < (1L << 40), "attn_grad_amax: n=%ld (positive, a multiple of 4)", (long)n);
  HIPIE_REQUIRE(ap_aligned(go) && ((uintptr_t)amax % 4) == 0, "attn_grad_amax: go must be 16-byte aligned, amax 4-byte aligned");
  if (hipMemsetAsync(amax, 0, 4, (hipStream_t)stream) != hipSuccess) return check_launch("attn_grad_amax");
  const long n4 = n / 4;
  const unsigned blocks = (unsigned)(n4 / 1024 + 1 < 2048 ? n4 / 1024 + 1 : 2048);         // at least 4 float4 per thread
  hipLaunchKernelGGL(ap_amax_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, (const float4*)go, n4, (unsigned int*)amax);
  return check_launch("attn_grad_amax");
}

extern "C" int hipie_attn_pack_grad(const void* go, const void* out, const void* v_hi, const void* v_lo, const void* scale, void* do_hi, void* do_lo,
                                    void* v96_hi, void* v96_lo, void* delta, int B, int heads, int H, int W, int Np, void* stream) {
  HIPIE_TRY(ap_check("attn_pack_grad", go && out && v_hi && v_lo && scale && do_hi && do_lo && v96_hi && v96_lo && delta,
                     ap_aligned(go) && ap_aligned(out) && ap_aligned(v_hi) && ap_aligned(v_lo) && ap_aligned(do_hi) && ap_aligned(do_lo) &&
                         ap_aligned(v96_hi) && ap_aligned(v96_lo),
                     B, heads, H, W, Np, 0, false));
  const long rows = (long)B * heads * Np;
  hipLaunchKernelGGL(ap_pack_grad_kernel, dim3(ap_blocks(rows * 16)), dim3(256), 0, (hipStream_t)stream, (const float*)go, (const float*)out,
                     (const f16_t*)v_hi, (const f16_t*)v_lo, (const float*)scale, (f16_t*)do_hi, (f16_t*)do_lo, (f16_t*)v96_hi, (f16_t*)v96_lo,
                     (float*)delta, heads, H, W, Np, rows);
  return check_launch("attn_pack_grad");
}

extern "C" int hipie_attn_unpack_grad(const void* dq, const void* dk, const void* dv, const void* dq_h, int64_t hs_b, int64_t hs_h, int64_t hs_w,
                                      const void* dq_w, int64_t ws_b, int64_t ws_h, int64_t ws_w, const void* inv, void* dqkv, int B, int heads, int H,
                                      int W, int Np, int cols, float qscale, void* stream) {
  HIPIE_TRY(ap_check("attn_unpack_grad", dq && dk && dv && dq_h && inv && dqkv,
                     ap_aligned(dq) && ap_aligned(dk) && ap_aligned(dv) && ap_aligned(dq_h) && ap_aligned(dq_w) && ap_aligned(dqkv), B, heads, H, W, Np,
                     cols));
  HIPIE_REQUIRE(hs_b >= 0 && hs_h >= 0 && hs_w >= 0 && ws_b >= 0 && ws_h >= 0 && ws_w >= 0 && (hs_b | hs_h | hs_w | ws_b | ws_h | ws_w) % 4 == 0,
                "attn_unpack_grad: the strides of the rel-pos terms must be non-negative multiples of 4 elements (16-byte aligned rows)");
  const long total = (long)B * H * W * 3 * heads * 20;
  const ApTerm th{(const float*)dq_h, (long)hs_b, (long)hs_h, (long)hs_w}, tw{(const float*)dq_w, (long)ws_b, (long)ws_h, (long)ws_w};
  hipLaunchKernelGGL(ap_unpack_grad_kernel, dim3(ap_blocks(total)), dim3(256), 0, (hipStream_t)stream, (const float*)dq, (const float*)dk,
                     (const float*)dv, th, tw, (const float*)inv, (float*)dqkv, heads, H, W, Np, cols, qscale, total);
  return check_launch("attn_unpack_grad");
}
