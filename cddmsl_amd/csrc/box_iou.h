// pairwise_iou (structures/boxes.py:322-367) for one pair, shared by the matcher kernels (boxes.hip) and the proposal-recall walk
// (proposal_recall.hip): one IEEE f32 operation per operation of the reference, in its order.  The translation units are built with
// contraction off, the division is a true division, and an empty intersection gives exactly 0.
#pragma once
#include "common.h"

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
