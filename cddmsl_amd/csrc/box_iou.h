// Device predicates that restate a numpy / torch call exactly, shared by the box kernels: iou_pair (boxes.hip, proposal_recall.hip),
// score_before (coco_match.hip, proposal_recall.hip), np_min / np_max (coco_match.hip, voc_match.hip).
#pragma once
#include "common.h"

// pairwise_iou (structures/boxes.py:322-367) for one pair: one IEEE f32 operation per operation of the reference, in its order.  The
// translation units are built with contraction off, the division is a true division, and an empty intersection gives exactly 0.

// g = the ground-truth box (x0, y0, x1, y1); the other box by value with its area ap = (x1 - x0) * (y1 - y0).  area_g + area_p is the
// reference's area1[:, None] + area2 whichever of the two it calls boxes1: an f32 addition commutes.
__device__ __forceinline__ float iou_pair(const float* g, float x0, float y0, float x1, float y1, float ap) {
  float w = fminf(g[2], x1) - fmaxf(g[0], x0);
  float h = fminf(g[3], y1) - fmaxf(g[1], y0);
  w = fmaxf(w, 0.f); h = fmaxf(h, 0.f);
  float inter = w * h;
  float ag = (g[2] - g[0]) * (g[3] - g[1]);
  return inter > 0.f ? inter / (ag + ap - inter) : 0.f;
}

// np.argsort(-score, kind="mergesort") and logits.sort(descending=True) made stable: does (score sq, input index q) come before
// (sp, p)?  Descending, NaN last, equal scores by input index: a total order, so a rank is a count and no sort is needed.
__device__ __forceinline__ bool score_before(float sq, int q, float sp, int p) {
  const bool nq = sq != sq, np = sp != sp;
  if (nq || np) return (!nq && np) || (nq && np && q < p);
  return sq > sp || (sq == sp && q < p);
}

// np.minimum / np.maximum (and torch.min / torch.max of two tensors) on doubles: the first operand unless the second is strictly
// beyond it (a NaN first operand stays)
__device__ __forceinline__ double np_min(double a, double b) { return (a <= b || a != a) ? a : b; }
__device__ __forceinline__ double np_max(double a, double b) { return (a >= b || a != a) ? a : b; }
