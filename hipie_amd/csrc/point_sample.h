// point_sample.h -- what the kernels that sample a mask at points share (point_loss.hip, point_select.hip), one definition each: the
// bilinear sample of matcher.point_sample (grid_sample, align_corners=False, zero padding, (x, y) in [0, 1]^2) and the stable sigmoid /
// softplus parts of a logit.
#pragma once
#include "common.h"

namespace hipie {

// ---- the element-wise terms ------------------------------------------------------------------------------------------------------------
struct Sigmoid {
  float p, q, l1p;                           // sigmoid(x), 1 - sigmoid(x) (no cancellation: sigmoid(-x)), log(1 + exp(-|x|))
};

__device__ __forceinline__ Sigmoid sigmoid_parts(float x) {
  const float e = expf(-fabsf(x));
  const float r = 1.f / (1.f + e);
  Sigmoid s;
  s.p = x >= 0.f ? r : e * r;
  s.q = x >= 0.f ? e * r : r;
  s.l1p = log1pf(e);
  return s;
}

// ---- bilinear sampling: grid_sample(align_corners=False, zero padding) at (x, y) in [0, 1]^2 ----------------------------------------
struct Corners {
  int off[4];                                // y * W + x of the nw, ne, sw, se corner; 0 for a corner outside the map
  float w[4];                                // its weight; 0 outside
};

__device__ __forceinline__ Corners corners_of(float x, float y, int H, int W) {
  // pixel coordinate x * W - 0.5 in one rounding.  The clamp keeps float -> int defined for any input and moves nothing that has a corner
  // inside the map: below -1 and from W on every corner is outside anyway.  A NaN coordinate becomes -2: the sample is 0.
  const float ix = fminf(fmaxf(fmaf(x, (float)W, -0.5f), -2.f), (float)W + 1.f);
  const float iy = fminf(fmaxf(fmaf(y, (float)H, -0.5f), -2.f), (float)H + 1.f);
  const float fx = floorf(ix), fy = floorf(iy);
  const int x0 = (int)fx, y0 = (int)fy;
  const float wx1 = ix - fx, wy1 = iy - fy;
  const float wx0 = 1.f - wx1, wy0 = 1.f - wy1;
  Corners c;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int xi = x0 + (k & 1), yi = y0 + (k >> 1);
    const bool in = xi >= 0 && xi < W && yi >= 0 && yi < H;
    c.off[k] = in ? yi * W + xi : 0;
    c.w[k] = in ? ((k & 1) ? wx1 : wx0) * ((k >> 1) ? wy1 : wy0) : 0.f;
  }
  return c;
}

// a corner of weight 0 is not read (outside the map, or in it with the point on a pixel centre)
__device__ __forceinline__ float sample(const float* __restrict__ map, const Corners& c) {
  float v = 0.f;
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (c.w[k] != 0.f) v += c.w[k] * map[c.off[k]];
  return v;
}

}  // namespace hipie
