// optim_step.hip -- the tail of a training iteration behind backward(): the total gradient norm, the clip and the AdamW update of every
// parameter tensor of the model, fp32, in two passes over memory:
//
//   hipie_optim_grad_norm    norm = | grad_scale x (all gradients) |_2 as one device float           (reads g: 4 B per parameter)
//   hipie_optim_adamw_step   g' = clip(grad_scale x g), decoupled weight decay, m, v and p updated     (reads p, g, m, v, writes p, m, v: 28 B)
//
// Replaces torch.nn.utils.clip_grad_norm_ (_foreach_norm over 1241 tensors, a stack, a norm, the coefficient, _foreach_mul_ reading and writing
// every gradient) and torch.optim.AdamW's multi-tensor step.  The clipped gradients are never written: the coefficient is one scalar that the
// update applies as it reads g.  Nothing is read by the host.
//
// Operands.  A SEGMENT TABLE on the device, one 48-byte record per parameter tensor: the addresses of p, g, m, v, the element count and the index
// of the tensor's hyper-parameter group; g == 0: no gradient this step.  A CHUNK MAP on the device, one (segment, element offset) pair per
// HIPIE_OPTIM_CHUNK = 16384 elements of a tensor (the last chunk of a tensor is partial, a 3-element bias is a chunk of its own): a function of the
// sizes alone.  Both kernels run a grid-stride loop over the chunks, a workgroup of 256 threads per chunk, at most 2048 workgroups.
//
// Elements.  Thread t of a chunk owns the GROUPS of four consecutive elements t, t + 256, ... of the chunk, whatever the addresses are: a group is
// one 16-byte access on every tensor whose address (base + chunk offset: the chunk size keeps the base's alignment) is 16-byte aligned, and four
// 4-byte accesses otherwise -- gradients that are views into a flat bucket at any element offset (training/ddp.py) take that path for g alone.
//
// Norm (optim_sqnorm_kernel, optim_norm_finish_kernel).  A thread adds the squares of its elements in float64, one accumulator per position in the
// group, in ascending order; the four are added as (0 + 1) + (2 + 3), the 64 lanes of a wave by butterfly, the four waves in order: one float64
// partial sum per chunk, in the chunk's own slot of `ws`.  The finisher (one workgroup) adds the partial sums -- thread t those of chunks t, t + 256,
// ... in ascending order, then the same tree -- and writes (float)(sqrt(sum) x |grad_scale|).  No atomics; neither the grid nor the schedule nor the
// alignment of a gradient enters the order of the additions: two calls give the same bits, separate gradient tensors and bucket views too.
//
// Update (optim_tick_kernel, optim_adamw_kernel).  The tick advances the step count t of every segment that has a gradient and writes its bias
// corrections, computed in float64: bc[s] = (1 - beta1^t, sqrt(1 - beta2^t)).  The update computes, in fp32 without contraction, in the order of
// torch's single-tensor AdamW:   c = min(max_norm / (norm + 1e-6), 1) with a NaN kept (no clipping: 1);   g' = (g x grad_scale) x c;
//   p = p x (1 - lr wd);   m = lerp(m, g', 1 - beta1);   v = v x beta2 + ((1 - beta2) g') g';   p = p - (lr / bc1) (m / (sqrt(v) / sqrt(bc2) + eps)).
// A segment without a gradient is skipped whole: no decay, m and v untouched, no tick.
#include "common.h"
#include "wave.h"

namespace hipie {

constexpr int OS_THREADS = 256;
constexpr int OS_CHUNK = HIPIE_OPTIM_CHUNK;
constexpr int OS_MAX_GRID = 2048;
constexpr int OS_MAX_HYPER = 8;

struct OptimSegment {                            // the record of the segment table (include/hipie_mi355.h)
  float* p;
  float* g;
  float* m;
  float* v;
  int64_t numel;
  int32_t group;
  int32_t reserved;
};
static_assert(sizeof(OptimSegment) == 48, "segment record");

struct OptimChunk {                              // the entry of the chunk map
  int64_t segment;
  int64_t offset;
};

struct OptimHyper {                              // by value: a scheduler that changes lr every iteration touches nothing on the device
  float lr[OS_MAX_HYPER];
  float decay[OS_MAX_HYPER];                     // (float)(1 - lr wd)
  float omb1, beta2, omb2, eps, max_norm, grad_scale;
  int n_groups, write_grads;
};

// the chunk's segment and extent, or false for an entry that does not lie inside its segment (never written by the binding; nothing is touched)
__device__ __forceinline__ bool chunk_of(const OptimSegment* __restrict__ table, int64_t n_seg, const OptimChunk* __restrict__ map, int64_t ci,
                                         int64_t& seg, OptimSegment& s, int64_t& off, int& n) {
  const OptimChunk c = map[ci];
  if (c.segment < 0 || c.segment >= n_seg) return false;
  seg = c.segment;
  s = table[c.segment];
  if (c.offset < 0 || c.offset >= s.numel) return false;
  off = c.offset;
  n = (int)(s.numel - off < (int64_t)OS_CHUNK ? s.numel - off : (int64_t)OS_CHUNK);
  return true;
}

__device__ __forceinline__ bool aligned16(const float* p) { return ((uintptr_t)p & 15u) == 0; }

// The tensors' addresses come out of the table, where the compiler cannot see that they are global memory (it would use flat accesses, which
// also wait on the LDS counter): the address space is stated here.
typedef __attribute__((address_space(1))) float gf32;
typedef __attribute__((address_space(1))) f32x4 gf32x4;
__device__ __forceinline__ gf32* as_global(float* p) { return (gf32*)p; }

// elements i .. i + 3 of a chunk of n: one 16-byte load when the tensor allows it and the group is whole, else element by element (0 beyond n)
__device__ __forceinline__ void load_group(const gf32* __restrict__ x, bool vec, int i, int n, float (&r)[4]) {
  if (vec && i + 4 <= n) {
    const f32x4 q = *reinterpret_cast<const gf32x4*>(x + i);
#pragma unroll
    for (int j = 0; j < 4; ++j) r[j] = q[j];
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) r[j] = i + j < n ? x[i + j] : 0.f;
  }
}

__device__ __forceinline__ void store_group(gf32* __restrict__ x, bool vec, int i, int n, const float (&r)[4]) {
  if (vec && i + 4 <= n) {
    f32x4 q;
#pragma unroll
    for (int j = 0; j < 4; ++j) q[j] = r[j];
    *reinterpret_cast<gf32x4*>(x + i) = q;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (i + j < n) x[i + j] = r[j];
  }
}

// the sum over the workgroup in a fixed order, valid in thread 0: the wave butterfly, then the four waves in order
__device__ __forceinline__ double block_sum_f64(double x, double* s_wave) {
  x = wave_sum(x);
  if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = x;
  __syncthreads();
  double s = 0.0;
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 0; w < OS_THREADS / 64; ++w) s += s_wave[w];
  }
  __syncthreads();                               // s_wave is free for the next chunk
  return s;
}

// ---- pass A: one float64 partial sum of g^2 per chunk ----------------------------------------------------------------------------------
__global__ __launch_bounds__(OS_THREADS) void optim_sqnorm_kernel(const OptimSegment* __restrict__ table, int64_t n_seg, const OptimChunk* __restrict__ map,
                                                                  int64_t n_chunks, double* __restrict__ part) {
  __shared__ double s_wave[OS_THREADS / 64];
  const int tid = threadIdx.x;
  for (int64_t ci = blockIdx.x; ci < n_chunks; ci += gridDim.x) {
    OptimSegment s;
    int64_t seg, off;
    int n;
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    if (chunk_of(table, n_seg, map, ci, seg, s, off, n) && s.g) {
      const gf32* g = as_global(s.g + off);
      const bool vec = aligned16(s.g + off);
      for (int k = tid; k * 4 < n; k += OS_THREADS) {
        float r[4];
        load_group(g, vec, k * 4, n, r);
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j] = fma((double)r[j], (double)r[j], acc[j]);
      }
    }
    const double sum = block_sum_f64((acc[0] + acc[1]) + (acc[2] + acc[3]), s_wave);
    if (tid == 0) part[ci] = sum;
  }
}

__global__ __launch_bounds__(OS_THREADS) void optim_norm_finish_kernel(const double* __restrict__ part, int64_t n_chunks, float grad_scale,
                                                                       float* __restrict__ norm) {
  __shared__ double s_wave[OS_THREADS / 64];
  double acc = 0.0;
  for (int64_t i = threadIdx.x; i < n_chunks; i += OS_THREADS) acc += part[i];
  const double sum = block_sum_f64(acc, s_wave);
  if (threadIdx.x == 0) *norm = (float)(sqrt(sum) * fabs((double)grad_scale));
}

// ---- pass B -------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(OS_THREADS) void optim_tick_kernel(const OptimSegment* __restrict__ table, int64_t n_seg, int32_t* __restrict__ steps,
                                                                float* __restrict__ bc, double beta1, double beta2) {
  const int64_t s = (int64_t)blockIdx.x * OS_THREADS + threadIdx.x;
  if (s >= n_seg || !table[s].g) return;
  const int32_t t = steps[s] + 1;
  steps[s] = t;
  bc[2 * s] = (float)(1.0 - pow(beta1, (double)t));
  bc[2 * s + 1] = (float)sqrt(1.0 - pow(beta2, (double)t));
}

__global__ __launch_bounds__(OS_THREADS) void optim_adamw_kernel(const OptimSegment* __restrict__ table, int64_t n_seg, const OptimChunk* __restrict__ map,
                                                                 int64_t n_chunks, const float* __restrict__ bc, const float* __restrict__ norm,
                                                                 const OptimHyper h) {
#pragma clang fp contract(off)
  const int tid = threadIdx.x;
  float c = 1.f;
  if (norm) {                                    // torch: clamp(max_norm / (total_norm + 1e-6), max=1.0); `c > 1` is false for a NaN, which stays
    c = h.max_norm / (*norm + 1e-6f);
    c = c > 1.f ? 1.f : c;
  }
  for (int64_t ci = blockIdx.x; ci < n_chunks; ci += gridDim.x) {
    OptimSegment s;
    int64_t seg, off;
    int n;
    if (!chunk_of(table, n_seg, map, ci, seg, s, off, n) || !s.g || !s.p || !s.m || !s.v) continue;
    if (s.group < 0 || s.group >= h.n_groups) continue;
    const float decay = h.decay[s.group];
    const float step_size = h.lr[s.group] / bc[2 * seg];
    const float bc2_sqrt = bc[2 * seg + 1];
    gf32* p = as_global(s.p + off);
    gf32* g = as_global(s.g + off);
    gf32* m = as_global(s.m + off);
    gf32* v = as_global(s.v + off);
    const bool vp = aligned16(s.p + off), vg = aligned16(s.g + off), vm = aligned16(s.m + off), vv = aligned16(s.v + off);
    for (int k = tid; k * 4 < n; k += OS_THREADS) {
      const int i = k * 4;
      float rp[4], rg[4], rm[4], rv[4];
      load_group(p, vp, i, n, rp);
      load_group(g, vg, i, n, rg);
      load_group(m, vm, i, n, rm);
      load_group(v, vv, i, n, rv);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float gc = (rg[j] * h.grad_scale) * c;
        rg[j] = gc;
        const float pd = rp[j] * decay;
        const float mn = h.omb1 < 0.5f ? rm[j] + h.omb1 * (gc - rm[j]) : gc - (gc - rm[j]) * (1.f - h.omb1);      // torch.lerp's two forms
        const float vn = rv[j] * h.beta2 + (h.omb2 * gc) * gc;
        const float denom = sqrtf(vn) / bc2_sqrt + h.eps;
        rp[j] = pd - step_size * (mn / denom);
        rm[j] = mn;
        rv[j] = vn;
      }
      store_group(p, vp, i, n, rp);
      store_group(m, vm, i, n, rm);
      store_group(v, vv, i, n, rv);
      if (h.write_grads) store_group(g, vg, i, n, rg);
    }
  }
}

static inline unsigned optim_grid(int64_t n_chunks) { return (unsigned)(n_chunks < OS_MAX_GRID ? n_chunks : OS_MAX_GRID); }

}  // namespace hipie

extern "C" int hipie_optim_chunk(void) { return hipie::OS_CHUNK; }

extern "C" int64_t hipie_optim_norm_ws_bytes(int64_t n_chunks) {
  if (n_chunks <= 0) return 8;
  return n_chunks * (int64_t)sizeof(double);
}

extern "C" int hipie_optim_grad_norm(const void* table, int64_t n_seg, const void* map, int64_t n_chunks, void* ws, int64_t ws_bytes, float grad_scale,
                                     float* norm, void* stream) {
  using namespace hipie;
  HIPIE_REQUIRE(n_seg >= 0 && n_chunks >= 0, "optim_grad_norm: negative count (n_seg=%lld, n_chunks=%lld)", (long long)n_seg, (long long)n_chunks);
  if (n_seg == 0 || n_chunks == 0) return HIPIE_OK;             // nothing to add: *norm is not written
  HIPIE_REQUIRE(table && map && ws && norm, "optim_grad_norm: null pointer (table, map, workspace, norm)");
  HIPIE_REQUIRE(((uintptr_t)table & 7u) == 0 && ((uintptr_t)map & 7u) == 0, "optim_grad_norm: table and map on an 8-byte boundary needed");
  HIPIE_REQUIRE(((uintptr_t)ws & 7u) == 0 && ws_bytes >= hipie_optim_norm_ws_bytes(n_chunks), "optim_grad_norm: workspace of %lld bytes on an 8-byte boundary needed, got %lld",
                (long long)hipie_optim_norm_ws_bytes(n_chunks), (long long)ws_bytes);
  hipLaunchKernelGGL(optim_sqnorm_kernel, dim3(optim_grid(n_chunks)), dim3(OS_THREADS), 0, (hipStream_t)stream, static_cast<const OptimSegment*>(table), n_seg,
                     static_cast<const OptimChunk*>(map), n_chunks, static_cast<double*>(ws));
  HIPIE_TRY(check_launch("optim_grad_norm (partial sums)"));
  hipLaunchKernelGGL(optim_norm_finish_kernel, dim3(1), dim3(OS_THREADS), 0, (hipStream_t)stream, static_cast<const double*>(ws), n_chunks, grad_scale, norm);
  return check_launch("optim_grad_norm");
}

extern "C" int hipie_optim_adamw_step(const void* table, int64_t n_seg, const void* map, int64_t n_chunks, int32_t* steps, float* bc, const double* group_lr,
                                      const double* group_wd, int n_groups, double beta1, double beta2, double eps, const float* norm, double max_norm,
                                      float grad_scale, int write_grads, void* stream) {
  using namespace hipie;
  HIPIE_REQUIRE(n_seg >= 0 && n_chunks >= 0 && n_groups >= 0, "optim_adamw_step: negative count (n_seg=%lld, n_chunks=%lld, n_groups=%d)", (long long)n_seg,
                (long long)n_chunks, n_groups);
  HIPIE_REQUIRE(n_groups <= OS_MAX_HYPER, "optim_adamw_step: %d groups, at most %d", n_groups, OS_MAX_HYPER);
  HIPIE_REQUIRE(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0, "optim_adamw_step: betas (%g, %g) outside [0, 1)", beta1, beta2);
  HIPIE_REQUIRE(eps > 0.0, "optim_adamw_step: eps=%g must be positive", eps);
  HIPIE_REQUIRE(!norm || max_norm >= 0.0, "optim_adamw_step: max_norm=%g is negative", max_norm);      // a NaN is refused too
  if (n_seg == 0 || n_chunks == 0) return HIPIE_OK;
  HIPIE_REQUIRE(table && map && steps && bc, "optim_adamw_step: null pointer (table, map, steps, bc)");
  HIPIE_REQUIRE(n_groups >= 1 && group_lr && group_wd, "optim_adamw_step: null pointer (group_lr, group_wd) or no group");
  HIPIE_REQUIRE(((uintptr_t)table & 7u) == 0 && ((uintptr_t)map & 7u) == 0, "optim_adamw_step: table and map on an 8-byte boundary needed");
  OptimHyper h;
  memset(&h, 0, sizeof(h));
  for (int i = 0; i < n_groups; ++i) {
    h.lr[i] = (float)group_lr[i];
    h.decay[i] = (float)(1.0 - group_lr[i] * group_wd[i]);
  }
  h.omb1 = (float)(1.0 - beta1); h.beta2 = (float)beta2; h.omb2 = (float)(1.0 - beta2); h.eps = (float)eps;
  h.max_norm = (float)max_norm; h.grad_scale = grad_scale;
  h.n_groups = n_groups; h.write_grads = write_grads ? 1 : 0;
  const OptimSegment* tab = static_cast<const OptimSegment*>(table);
  hipLaunchKernelGGL(optim_tick_kernel, dim3((unsigned)((n_seg + OS_THREADS - 1) / OS_THREADS)), dim3(OS_THREADS), 0, (hipStream_t)stream, tab, n_seg, steps, bc, beta1,
                     beta2);
  HIPIE_TRY(check_launch("optim_adamw_step (step counts)"));
  hipLaunchKernelGGL(optim_adamw_kernel, dim3(optim_grid(n_chunks)), dim3(OS_THREADS), 0, (hipStream_t)stream, tab, n_seg, static_cast<const OptimChunk*>(map), n_chunks,
                     bc, norm, h);
  return check_launch("optim_adamw_step");
}
