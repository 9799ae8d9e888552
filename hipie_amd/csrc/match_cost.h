// match_cost.h -- what the kernels of the matching costs share (ota_match.hip: the SimOTA cost; hungarian_cost.hip: the class and box costs
// of matcher.cost_matrix), one definition each: the cxcywh -> xyxy corners, the pairwise box terms (intersection, union, GIoU with the 1e-7 of
// boxes.generalized_box_iou) and the focal token cost of matcher.focal_token_cost.  The operations and their order are those of the torch
// formulation in fp32; floating-point contraction is off inside, so that no product is fused into the sum behind it.
#pragma once
#include "common.h"
#include "point_sample.h"

namespace hipie {

// T: float (the matching costs, in torch's fp32 operation order) or double (pair_loss.hip, which rounds once at the end)
template <typename T>
struct BoxCorners {
  T x0, y0, x1, y1;
};
typedef BoxCorners<float> BoxXYXY;

__device__ __forceinline__ float box_max(float a, float b) { return fmaxf(a, b); }
__device__ __forceinline__ float box_min(float a, float b) { return fminf(a, b); }
__device__ __forceinline__ double box_max(double a, double b) { return fmax(a, b); }
__device__ __forceinline__ double box_min(double a, double b) { return fmin(a, b); }
__device__ __forceinline__ float box_eps(float) { return 1e-7f; }
__device__ __forceinline__ double box_eps(double) { return 1e-7; }

// boxes.box_cxcywh_to_xyxy: c - 0.5 s, c + 0.5 s
template <typename T = float>
__device__ __forceinline__ BoxCorners<T> box_xyxy(const float* __restrict__ b) {
#pragma clang fp contract(off)
  const T hw = (T)0.5f * (T)b[2], hh = (T)0.5f * (T)b[3];
  BoxCorners<T> r;
  r.x0 = (T)b[0] - hw;
  r.y0 = (T)b[1] - hh;
  r.x1 = (T)b[0] + hw;
  r.y1 = (T)b[1] + hh;
  return r;
}

// the check of boxes.generalized_box_iou: a corner pair out of order -- or a NaN -- is a caller error
template <typename T>
__device__ __forceinline__ bool box_degenerate(const BoxCorners<T>& a) { return !(a.x1 >= a.x0) || !(a.y1 >= a.y0); }

template <typename T>
__device__ __forceinline__ T box_area(const BoxCorners<T>& a) {
#pragma clang fp contract(off)
  return (a.x1 - a.x0) * (a.y1 - a.y0);
}

template <typename T>
struct BoxPairTerms {
  T inter, uni, giou;                        // boxes._pairwise_inter_union, boxes.generalized_box_iou; IoU = inter / uni
};
typedef BoxPairTerms<float> BoxPair;

template <typename T>
__device__ __forceinline__ BoxPairTerms<T> box_pair(const BoxCorners<T>& a, const BoxCorners<T>& b) {
#pragma clang fp contract(off)
  BoxPairTerms<T> p;
  const T iw = box_max(box_min(a.x1, b.x1) - box_max(a.x0, b.x0), (T)0);
  const T ih = box_max(box_min(a.y1, b.y1) - box_max(a.y0, b.y0), (T)0);
  p.inter = iw * ih;
  p.uni = (box_area(a) + box_area(b)) - p.inter;
  const T hw = box_max(box_max(a.x1, b.x1) - box_min(a.x0, b.x0), (T)0);
  const T hh = box_max(box_max(a.y1, b.y1) - box_min(a.y0, b.y0), (T)0);
  const T hull = hw * hh;
  p.giou = p.inter / p.uni - (hull - p.uni) / (hull + box_eps((T)0));
  return p;
}

// matcher.focal_token_cost of the logit x (gamma = 2): the focal cost of calling the token positive minus that of calling it negative.
// 1 - sigmoid(x) is taken as sigmoid(-x) (sigmoid_parts), which has no cancellation; everything else is the torch expression.
__device__ __forceinline__ float focal_token_cost(float x, float alpha = 0.25f) {
#pragma clang fp contract(off)
  const Sigmoid g = sigmoid_parts(x);
  const float neg = ((1.f - alpha) * (g.p * g.p)) * (-logf(g.q + 1e-8f));
  const float pos = (alpha * (g.q * g.q)) * (-logf(g.p + 1e-8f));
  return pos - neg;
}

}  // namespace hipie
