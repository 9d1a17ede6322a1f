// Soft-NMS at inference on gfx950: the per-category walk of Bodla et al. (arXiv 1704.04503) as ONE launch per image.
//
// Reference call sites replaced (paths under detectron2/):
//   batched_soft_nms (coordinate shift per category)          layers/soft_nms.py:85-132
//   _soft_nms (argmax / pairwise_iou / decay / prune loop)    layers/soft_nms.py:186-261
//   pairwise_iou                                              structures/boxes.py:322-367
// The reference walks ALL candidates in one Python loop -- per pick an argmax, a pairwise_iou, a decay, a boolean compaction and
// two .item() readbacks.  Boxes of different categories are shifted apart, their IoU is 0 and every decay between them is exactly
// 1 (expf(-0) == 1), so the walk factors into independent walks per category whose picks, ordered by (rescored score descending,
// input index ascending), are the reference's keep list: inside a category scores only fall, and equal scores are picked in index
// order, so that order is one stable descending sort of a dense [K] score array.  One coupling between categories remains: the
// reference tests every remaining score against prune after every pick, so after its FIRST pick (the global arg-max) a candidate of
// another category that starts at or below prune is gone although its decay was 1.  k_snms_prep finds that first pick's category;
// every other category drops such candidates on arrival.
//
// Structure: a stable radix sort of the category ids (rocPRIM) groups the candidates into segments in input-index order; ONE
// WORKGROUP of 256 threads walks one category.  A single wave would need no barrier per pick but holds its candidates in
// registers: the required 2048 candidates of one category are 32 per lane x 6 values = 192 VGPRs of fully unrolled code.  The
// workgroup keeps the segment (shifted box, area, score; a dead candidate's score is -inf) in 48 KiB of LDS for the whole walk and
// pays ONE barrier per pick: each thread folds the arg-max of its own candidates into the decay pass, the four waves' partial
// winners go through LDS slots that alternate with the pick's parity (a slot is rewritten two barriers after it was read).
// Nothing but the pick's own score goes to memory between picks.  A category with more than SN_LDS candidates runs the SAME walk
// on its slice of the scratch buffer (L2-resident, slower): the only cap the caller can hit is the total, K <= SN_MAXK, and that
// one is checked on the host before anything is launched.
//
// Arithmetic: every f32 operation below is one IEEE operation in the reference's association order (the build has contraction
// off, division is correctly rounded); linear and hard contain no transcendental and are defined bit for bit, gaussian up to
// expf's documented 1 ulp.  Scores must be finite (a -inf or NaN score is never picked).
#include "common.h"
#include <climits>
#include <cstring>
#include <rocprim/rocprim.hpp>

namespace {

constexpr int SN_T = 256;         // threads of a walk workgroup
constexpr int SN_LDS = 2048;      // candidates of one category held in LDS; larger categories walk in the scratch buffer
constexpr int SN_MAXK = 32768;    // candidates per call
constexpr int SN_GRID = 1024;     // walk workgroups launched at most (each loops over the segments)
#define SN_NEG_INF (-__builtin_huge_valf())

struct SnCtl { float off; int nseg; int has_first; long long first_cat; };

__device__ __forceinline__ bool sn_better(float s, int p, float s2, int p2) { return s > s2 || (s == s2 && p < p2); }

// off = max over all coordinates + 1 (batched_soft_nms: boxes.max() + 1); the category of the reference's FIRST pick (the largest score
// of all, lowest index among equals); iota for the category sort; pick scores start at -inf
__global__ __launch_bounds__(1024) void k_snms_prep(const float* boxes, const float* scores, const long long* idxs, int K, SnCtl* ctl,
                                                     int* iota, float* pick_score) {
  __shared__ float wm[16], ws[16];
  __shared__ int wp[16];
  const int t = threadIdx.x;
  float m = SN_NEG_INF, bs = SN_NEG_INF;
  int bp = INT_MAX;
  for (int i = t; i < K; i += 1024) {
    const f32x4 b = ((const f32x4*)boxes)[i];
    m = fmaxf(fmaxf(m, fmaxf(b.x, b.y)), fmaxf(b.z, b.w));
    const float s = scores[i];
    if (s > bs) { bs = s; bp = i; }               // (ascending i, strict: the lowest index of equal scores)
    iota[i] = i;
    pick_score[i] = SN_NEG_INF;
  }
  m = wave_max(m);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float s2 = __shfl_xor(bs, o, 64);
    const int p2 = __shfl_xor(bp, o, 64);
    if (sn_better(s2, p2, bs, bp)) { bs = s2; bp = p2; }
  }
  if ((t & 63) == 0) { wm[t >> 6] = m; ws[t >> 6] = bs; wp[t >> 6] = bp; }
  __syncthreads();
  if (t == 0) {
    for (int w = 1; w < 16; ++w) {
      m = fmaxf(m, wm[w]);
      if (sn_better(ws[w], wp[w], bs, bp)) { bs = ws[w]; bp = wp[w]; }
    }
    ctl->off = m + 1.0f;
    ctl->nseg = 0;
    ctl->has_first = bp != INT_MAX;
    ctl->first_cat = bp != INT_MAX ? idxs[bp] : 0;
  }
}

// segment starts of the sorted category ids, in any order (the walks are independent)
__global__ void k_snms_segs(const long long* cat, int K, SnCtl* ctl, int* seg_start) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= K) return;
  if (i == 0 || cat[i] != cat[i - 1]) seg_start[atomicAdd(&ctl->nseg, 1)] = i;
}

// the walk over one segment of n candidates whose state is at x0..sc (LDS or scratch); ord[j] = input index of candidate j
__device__ __forceinline__ void sn_walk(const float* x0, const float* y0, const float* x1, const float* y1, const float* ar, float* sc,
                                        int n, const int* ord, float* pick_score, int method, float sigma, float thr, float prune,
                                        int cap, float* r_s, int* r_p) {
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  float bs = SN_NEG_INF;
  int bp = INT_MAX;
  for (int j = t; j < n; j += SN_T) {             // (ascending j and a strict comparison: the lowest index of equal scores)
    const float s = sc[j];
    if (s > bs) { bs = s; bp = j; }
  }
  for (int pick = 0; cap < 0 || pick < cap; ++pick) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float s2 = __shfl_xor(bs, o, 64);
      const int p2 = __shfl_xor(bp, o, 64);
      if (sn_better(s2, p2, bs, bp)) { bs = s2; bp = p2; }
    }
    const int par = (pick & 1) * (SN_T / 64);
    if (lane == 0) { r_s[par + wv] = bs; r_p[par + wv] = bp; }
    __syncthreads();
    float ws = r_s[par];
    int wp = r_p[par];
#pragma unroll
    for (int w = 1; w < SN_T / 64; ++w)
      if (sn_better(r_s[par + w], r_p[par + w], ws, wp)) { ws = r_s[par + w]; wp = r_p[par + w]; }
    if (wp == INT_MAX) break;                     // nobody left (block-uniform)
    const float tx0 = x0[wp], ty0 = y0[wp], tx1 = x1[wp], ty1 = y1[wp], ta = ar[wp];
    if (t == 0) pick_score[ord[wp]] = ws;         // the rescored score is the value at pick time
    bs = SN_NEG_INF;
    bp = INT_MAX;
    for (int j = t; j < n; j += SN_T) {           // a thread reads and writes the scores of its own candidates only
      float s = sc[j];
      if (!(s > SN_NEG_INF)) continue;
      if (j == wp) { sc[j] = SN_NEG_INF; continue; }
      float w = fminf(tx1, x1[j]) - fmaxf(tx0, x0[j]);
      float h = fminf(ty1, y1[j]) - fmaxf(ty0, y0[j]);
      w = fmaxf(w, 0.f); h = fmaxf(h, 0.f);
      const float inter = w * h;
      const float iou = inter > 0.f ? inter / (ta + ar[j] - inter) : 0.f;
      float decay;
      if (method == 1) decay = iou > thr ? 1.f - iou : 1.f;
      else if (method == 2) decay = iou < thr ? 1.f : 0.f;
      else decay = expf(-(iou * iou) / sigma);
      s = s * decay;
      if (!(s > prune)) s = SN_NEG_INF;
      sc[j] = s;
      if (s > bs) { bs = s; bp = j; }
    }
  }
}

__global__ __launch_bounds__(SN_T) void k_snms_walk(const float* boxes, const float* scores, const long long* cat, const int* order,
                                                     const int* seg_start, const SnCtl* ctl, float* gstate, float* pick_score, int K,
                                                     int method, float sigma, float thr, float prune, int cap) {
  __shared__ float l_x0[SN_LDS], l_y0[SN_LDS], l_x1[SN_LDS], l_y1[SN_LDS], l_ar[SN_LDS], l_sc[SN_LDS];
  __shared__ float r_s[2 * SN_T / 64];
  __shared__ int r_p[2 * SN_T / 64];
  __shared__ int s_end;
  const int t = threadIdx.x;
  const int nseg = ctl->nseg;
  const float off = ctl->off;
  const bool has_first = ctl->has_first != 0;
  const long long first_cat = ctl->first_cat;
  for (int s = blockIdx.x; s < nseg; s += gridDim.x) {
    __syncthreads();                              // the previous segment's walk is over
    const int start = seg_start[s];
    const long long c = cat[start];
    if (t == 0) s_end = K;
    __syncthreads();
    for (int j = start + t; j < K; j += SN_T)
      if (cat[j] != c) { atomicMin(&s_end, j); break; }
    __syncthreads();
    const int n = s_end - start;
    const bool in_lds = n <= SN_LDS;
    float *g_x0 = gstate + start, *g_y0 = g_x0 + K, *g_x1 = g_y0 + K, *g_y1 = g_x1 + K, *g_ar = g_y1 + K, *g_sc = g_ar + K;
    float* x0 = in_lds ? l_x0 : g_x0;
    float* y0 = in_lds ? l_y0 : g_y0;
    float* x1 = in_lds ? l_x1 : g_x1;
    float* y1 = in_lds ? l_y1 : g_y1;
    float* ar = in_lds ? l_ar : g_ar;
    float* sc = in_lds ? l_sc : g_sc;
    // The reference walks ALL categories at once and tests every remaining score against prune after EVERY pick, its first
    // included: outside the first pick's category the decay is exactly 1, so a candidate that starts at or below prune is
    // dropped there before its own category ever picks.  Inside the first pick's category the walk below does that test itself.
    const bool prune_on_arrival = !(has_first && c == first_cat);
    const float sh = (float)c * off;              // idxs.to(boxes) * (max_coordinate + 1), then one rounded addition per coordinate
    for (int j = t; j < n; j += SN_T) {
      const int i = order[start + j];
      const f32x4 b = ((const f32x4*)boxes)[i];
      const float a0 = b.x + sh, b0 = b.y + sh, a1 = b.z + sh, b1 = b.w + sh;
      x0[j] = a0; y0[j] = b0; x1[j] = a1; y1[j] = b1;
      ar[j] = (a1 - a0) * (b1 - b0);
      const float s0 = scores[i];
      sc[j] = (prune_on_arrival && !(s0 > prune)) ? SN_NEG_INF : s0;
    }
    __syncthreads();
    if (in_lds) sn_walk(l_x0, l_y0, l_x1, l_y1, l_ar, l_sc, n, order + start, pick_score, method, sigma, thr, prune, cap, r_s, r_p);
    else sn_walk(g_x0, g_y0, g_x1, g_y1, g_ar, g_sc, n, order + start, pick_score, method, sigma, thr, prune, cap, r_s, r_p);
  }
}

// order2 = stable descending order of pick_score: the picks are a prefix of it
__global__ void k_snms_finish(const float* pick_score, const int* order2, long* keep, float* keep_scores, int* nkeep, int K, int max_keep) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= K) return;
  const int lim = max_keep < 0 ? K : min(K, max_keep);
  const int o = order2[i];
  const float s = pick_score[o];
  const bool v = i < lim && s > SN_NEG_INF;
  const bool vn = i + 1 < lim && pick_score[order2[i + 1]] > SN_NEG_INF;
  keep[i] = v ? (long)o : -1L;
  if (v) keep_scores[i] = s;
  if (v && !vn) nkeep[0] = i + 1;
  if (i == 0 && !v) nkeep[0] = 0;
}

}  // namespace

extern "C" int cddmsl_soft_nms(const float* boxes, const float* scores, const long* idxs, long* keep, float* keep_scores, int* nkeep,
                               int K, int method, float sigma, float iou_threshold, float prune_threshold, int max_keep, void* temp,
                               size_t* temp_bytes, void* stream) {
  if (K < 0 || K > SN_MAXK || !temp_bytes || method < 0 || method > 2 || (method == 0 && !(sigma > 0.f)) || max_keep < -1) return CDDMSL_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  if (K == 0) {
    if (temp) return hipMemsetAsync(nkeep, 0, sizeof(int), st) == hipSuccess ? CDDMSL_OK : CDDMSL_ERR_LAUNCH;
    *temp_bytes = 0;
    return CDDMSL_OK;
  }
  size_t sort_bytes = 0, rp = 0;
  int rc = cddmsl_sort_desc(nullptr, nullptr, nullptr, nullptr, nullptr, 1, K, nullptr, &sort_bytes, stream);
  if (rc != CDDMSL_OK) return rc;
  if (rocprim::radix_sort_pairs(nullptr, rp, (long long*)nullptr, (long long*)nullptr, (int*)nullptr, (int*)nullptr, (size_t)K, 0, 64, st) != hipSuccess)
    return CDDMSL_ERR_LAUNCH;
  auto al = [](size_t b) { return (b + 255) & ~(size_t)255; };
  const size_t k4 = al((size_t)K * 4);
  const size_t o_rp = al(sort_bytes), o_cat = o_rp + al(rp), o_iota = o_cat + al((size_t)K * 8), o_ord = o_iota + k4, o_seg = o_ord + k4,
               o_ctl = o_seg + k4, o_st = o_ctl + 256, o_ps = o_st + al((size_t)K * 24), o_ko = o_ps + k4, o_si = o_ko + k4, o_o2 = o_si + k4,
               total = o_o2 + k4;
  if (!temp) { *temp_bytes = total; return CDDMSL_OK; }
  if (*temp_bytes < total) return CDDMSL_ERR_ARG;
  char* t = (char*)temp;
  long long* cat = (long long*)(t + o_cat);
  int *iota = (int*)(t + o_iota), *ord = (int*)(t + o_ord), *seg = (int*)(t + o_seg), *o2 = (int*)(t + o_o2);
  SnCtl* ctl = (SnCtl*)(t + o_ctl);
  float* ps = (float*)(t + o_ps);
  const unsigned blocks = (unsigned)((K + 255) / 256);
  k_snms_prep<<<dim3(1), dim3(1024), 0, st>>>(boxes, scores, (const long long*)idxs, K, ctl, iota, ps);
  if (rocprim::radix_sort_pairs(t + o_rp, rp, (const long long*)idxs, cat, iota, ord, (size_t)K, 0, 64, st) != hipSuccess) return CDDMSL_ERR_LAUNCH;
  k_snms_segs<<<dim3(blocks), dim3(256), 0, st>>>(cat, K, ctl, seg);
  // (the number of categories is known on the device only: up to SN_GRID workgroups are launched, one per possible segment, and
  // those beyond nseg return at once -- deliberate, a readback of nseg would cost more than the idle workgroups)
  k_snms_walk<<<dim3(K < SN_GRID ? K : SN_GRID), dim3(SN_T), 0, st>>>(boxes, scores, cat, ord, seg, ctl, (float*)(t + o_st), ps, K, method, sigma,
                                                                     iou_threshold, prune_threshold, max_keep);
  size_t sb = sort_bytes;
  rc = cddmsl_sort_desc(ps, (float*)(t + o_ko), (int*)(t + o_si), o2, nullptr, 1, K, t, &sb, stream);
  if (rc != CDDMSL_OK) return rc;
  k_snms_finish<<<dim3(blocks), dim3(256), 0, st>>>(ps, o2, keep, keep_scores, nkeep, K, max_keep);
  return launch_status();
}
