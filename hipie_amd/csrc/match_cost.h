// match_cost.h -- what the kernels of the matching costs share (ota_match.hip: the SimOTA cost; hungarian_cost.hip: the class and box costs
// of matcher.cost_matrix), one definition each: the cxcywh -> xyxy corners, the pairwise box terms (intersection, union, GIoU with the 1e-7 of
// boxes.generalized_box_iou) and the focal token cost of matcher.focal_token_cost.  The operations and their order are those of the torch
// formulation in fp32; floating-point contraction is off inside, so that no product is fused into the sum behind it.
#pragma once
#include "common.h"
#include "point_sample.h"

namespace hipie {

struct BoxXYXY {
  float x0, y0, x1, y1;
};

// boxes.box_cxcywh_to_xyxy: c - 0.5 s, c + 0.5 s
__device__ __forceinline__ BoxXYXY box_xyxy(const float* __restrict__ b) {
#pragma clang fp contract(off)
  const float hw = 0.5f * b[2], hh = 0.5f * b[3];
  BoxXYXY r;
  r.x0 = b[0] - hw;
  r.y0 = b[1] - hh;
  r.x1 = b[0] + hw;
  r.y1 = b[1] + hh;
  return r;
}

// the check of boxes.generalized_box_iou: a corner pair out of order -- or a NaN -- is a caller error
__device__ __forceinline__ bool box_degenerate(const BoxXYXY& a) { return !(a.x1 >= a.x0) || !(a.y1 >= a.y0); }

__device__ __forceinline__ float box_area(const BoxXYXY& a) {
#pragma clang fp contract(off)
  return (a.x1 - a.x0) * (a.y1 - a.y0);
}

struct BoxPair {
  float inter, uni, giou;                    // boxes._pairwise_inter_union, boxes.generalized_box_iou; IoU = inter / uni
};

__device__ __forceinline__ BoxPair box_pair(const BoxXYXY& a, const BoxXYXY& b) {
#pragma clang fp contract(off)
  BoxPair p;
  const float iw = fmaxf(fminf(a.x1, b.x1) - fmaxf(a.x0, b.x0), 0.f);
  const float ih = fmaxf(fminf(a.y1, b.y1) - fmaxf(a.y0, b.y0), 0.f);
  p.inter = iw * ih;
  p.uni = (box_area(a) + box_area(b)) - p.inter;
  const float hw = fmaxf(fmaxf(a.x1, b.x1) - fminf(a.x0, b.x0), 0.f);
  const float hh = fmaxf(fmaxf(a.y1, b.y1) - fminf(a.y0, b.y0), 0.f);
  const float hull = hw * hh;
  p.giou = p.inter / p.uni - (hull - p.uni) / (hull + 1e-7f);
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
