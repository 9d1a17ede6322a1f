// Proposal recall on gfx950: the per-image body of _evaluate_box_proposals (evaluation/coco_evaluation.py:517-571) for every
// (image, proposal limit, area range) of a batch in ONE launch.
//
// Host yardstick reproduced bit for bit: cddmsl_amd/evaluation.py proposal_cover_host.  What the reference does per image and what
// happens here:
//   inds = objectness_logits.sort(descending=True)   rank = #{better proposals of the image}: a total order (logit descending, NaN
//                                                    last, equal logits by input index), so no sort is needed
//   predictions[:limit]                              the boxes of ranks < min(P, limit) go to LDS in rank order
//   gt_boxes[valid_gt_inds]                          the boxes whose range bit is set, compacted in data-set order (ballot + popcount)
//   overlaps = pairwise_iou(proposals, gt)           never stored: a column (one box against the unused proposals) is recomputed
//                                                    when it is needed, with iou_pair (box_iou.h)
//   min(P', G') times: overlaps.max(dim=0), then     every box keeps (best IoU, best rank) over the unused proposals; a pick is the
//   .max(dim=0); record; row and column = -1         arg-max of those over the live boxes (first maximum: lowest box, and inside the
//                                                    column lowest rank); only the columns whose best was the retired proposal are
//                                                    recomputed
// The reference records by iteration number and sorts all recorded values afterwards; recording on the box gives the same multiset.
// Structure: one workgroup of 4 waves per (image, limit, range).  A column is computed by one wave (lanes stride over the ranks,
// shuffle reduction); the pick is made by wave 0.  No atomics; every output slot has exactly one writer.
//
// Caps (named in the Python wrapper): PR_MAXP proposals and PR_MAXG ground-truth boxes of one image.  An image beyond a cap, or with
// inconsistent offsets, sets over[b] = 1 and writes nothing else: the caller walks that image on the host, it is never truncated.
#include "common.h"
#include "box_iou.h"

namespace {

constexpr int PR_MAXP = 2048;     // proposals of one image
constexpr int PR_MAXG = 512;      // ground-truth boxes of one image
constexpr int PR_MAXL = 4;        // proposal limits per launch
constexpr int PR_MAXA = 8;        // area ranges per launch (one bit each in gt_rng)
constexpr int PR_THREADS = 256;
constexpr int PR_WAVES = PR_THREADS / 64;
constexpr float PR_RETIRED = -2.f;   // s_best of a box that has been picked (an IoU is >= 0, a column without proposals -1)

// one wave: box j against the unused proposals of ranks [0, Pk) -> (best IoU, its lowest rank) in s_best[j] / s_bestr[j]
__device__ __forceinline__ void pr_column(int j, int lane, int Pk, const f32x4* s_pb, const f32x4* s_gb, const unsigned int* s_used,
                                          float* s_best, int* s_bestr) {
  const float* g = (const float*)&s_gb[j];
  float bv = -1.f;
  int br = 0x7fffffff;
  for (int r = lane; r < Pk; r += 64) {
    if ((s_used[r >> 5] >> (r & 31)) & 1u) continue;
    const f32x4 pb = s_pb[r];
    const float v = iou_pair(g, pb.x, pb.y, pb.z, pb.w, (pb.z - pb.x) * (pb.w - pb.y));
    if (v > bv) { bv = v; br = r; }               // (ranks ascend inside a lane: the first maximum stays)
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(bv, o, 64);
    const int orr = __shfl_xor(br, o, 64);
    if (ov > bv || (ov == bv && orr < br)) { bv = ov; br = orr; }
  }
  if (lane == 0) { s_best[j] = bv; s_bestr[j] = br; }
}

__global__ __launch_bounds__(PR_THREADS) void k_proposal_cover(
    const float* __restrict__ boxes, const float* __restrict__ logits, const long long* __restrict__ off,
    const long long* __restrict__ img_idx, long long P_total, const float* __restrict__ gt_boxes,
    const unsigned char* __restrict__ gt_rng, const long long* __restrict__ gt_off, long long n_images, long long G_total,
    const int* __restrict__ limits, int L, int A, const long long* __restrict__ cover_off, long long Gb, float* __restrict__ cover,
    int* __restrict__ over) {
  __shared__ f32x4 s_pb[PR_MAXP];                 // kept proposals, by rank
  __shared__ f32x4 s_gb[PR_MAXG];                 // in-range boxes, in data-set order
  __shared__ float s_scratch[PR_MAXP];            // first the logits; after the ranking the four per-box arrays below
  __shared__ unsigned int s_used[PR_MAXP / 32];   // retired proposals, bit = rank
  __shared__ int s_n, s_pick;
  float* s_best = s_scratch;                                               // [PR_MAXG]
  int* s_bestr = (int*)(s_scratch + PR_MAXG);                              // [PR_MAXG]
  float* s_rec = s_scratch + 2 * PR_MAXG;                                  // [PR_MAXG] the IoU recorded on the box
  unsigned short* s_gidx = (unsigned short*)(s_scratch + 3 * PR_MAXG);     // [PR_MAXG] position -> box of the image

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.x / (L * A), rem = blockIdx.x % (L * A), l = rem / A, a = rem % A;
  // ---- (block-uniform) offsets and caps
  const long long p0 = off[b], p1 = off[b + 1], im = img_idx[b];
  bool bad = p0 < 0 || p1 < p0 || p1 > P_total || im < 0 || im >= n_images;
  long long g0 = 0, g1 = 0, c0 = 0;
  if (!bad) {
    g0 = gt_off[im]; g1 = gt_off[im + 1]; c0 = cover_off[b];
    bad = g0 < 0 || g1 < g0 || g1 > G_total || c0 < 0 || c0 > Gb || g1 - g0 > Gb - c0 || p1 - p0 > PR_MAXP || g1 - g0 > PR_MAXG;
  }
  if (l == 0 && a == 0 && tid == 0) over[b] = bad ? 1 : 0;
  if (bad) return;
  const int P = (int)(p1 - p0), G = (int)(g1 - g0);
  if (G == 0) return;
  float* out = cover + ((long long)(l * A + a) * Gb + c0);
  if (P == 0) {                                   // the reference skips such an image before it counts its boxes
    for (int g = tid; g < G; g += PR_THREADS) out[g] = -1.f;
    return;
  }
  const int lim = limits[l];
  const int Pk = lim < P ? (lim > 0 ? lim : 0) : P;

  // ---- ranks; the kept proposals in rank order
  for (int p = tid; p < P; p += PR_THREADS) s_scratch[p] = logits[p0 + p];
  for (int w = tid; w < PR_MAXP / 32; w += PR_THREADS) s_used[w] = 0u;
  __syncthreads();
  for (int p = tid; p < P; p += PR_THREADS) {
    const float sp = s_scratch[p];
    int r = 0;
    for (int q = 0; q < P; ++q) r += score_before(s_scratch[q], q, sp, p) ? 1 : 0;
    if (r < Pk) s_pb[r] = ((const f32x4*)boxes)[p0 + p];
  }
  __syncthreads();                                // the logits are dead: s_scratch becomes the per-box arrays
  // ---- the boxes of this range, in data-set order (wave 0); a box outside the range is not counted
  if (wave == 0) {
    const unsigned long long below = (1ull << lane) - 1ull;
    int n = 0;
    for (int base = 0; base < G; base += 64) {
      const int g = base + lane;
      const bool in = g < G;
      const bool f = in && ((gt_rng[g0 + g] >> a) & 1u);
      const unsigned long long m = __ballot(f);
      if (f) {
        const int pos = n + __popcll(m & below);
        s_gb[pos] = ((const f32x4*)gt_boxes)[g0 + g];
        s_gidx[pos] = (unsigned short)g;
        s_rec[pos] = 0.f;
      } else if (in) {
        out[g] = -1.f;
      }
      n += __popcll(m);
    }
    if (lane == 0) s_n = n;
  }
  __syncthreads();
  const int Gn = s_n;
  for (int j = wave; j < Gn; j += PR_WAVES) pr_column(j, lane, Pk, s_pb, s_gb, s_used, s_best, s_bestr);
  __syncthreads();

  // ---- the walk
  const int iters = Pk < Gn ? Pk : Gn;
  for (int it = 0; it < iters; ++it) {
    if (wave == 0) {
      float bv = PR_RETIRED;
      int bj = 0x7fffffff;
      for (int j = lane; j < Gn; j += 64) {
        const float v = s_best[j];
        if (v > bv) { bv = v; bj = j; }
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(bv, o, 64);
        const int oj = __shfl_xor(bj, o, 64);
        if (ov > bv || (ov == bv && oj < bj)) { bv = ov; bj = oj; }
      }
      // it < min(Pk, Gn): a live box and an unused proposal exist, so bj is a box and its rank a proposal (guarded all the same)
      if (lane == 0) {
        int r = -1;
        if (bj < Gn) {
          r = s_bestr[bj];
          s_rec[bj] = bv;
          s_best[bj] = PR_RETIRED;
          if (r >= 0 && r < Pk) s_used[r >> 5] |= 1u << (r & 31);
        }
        s_pick = r;
      }
    }
    __syncthreads();
    const int r = s_pick;
    for (int j = wave; j < Gn; j += PR_WAVES)
      if (s_best[j] != PR_RETIRED && s_bestr[j] == r) pr_column(j, lane, Pk, s_pb, s_gb, s_used, s_best, s_bestr);   // (wave-uniform)
    __syncthreads();
  }
  for (int j = tid; j < Gn; j += PR_THREADS) out[s_gidx[j]] = s_rec[j];      // 0.0 where the walk ended before the box
}

}  // namespace

extern "C" int cddmsl_proposal_cover(const float* boxes, const float* logits, const long* off, const long* img_idx, int B, long P_total,
                                     const float* gt_boxes, const unsigned char* gt_rng, const long* gt_off, long n_images, long G_total,
                                     const int* limits, int L, int A, const long* cover_off, long Gb, float* cover, int* over,
                                     void* stream) {
  if (B < 0 || P_total < 0 || n_images < 0 || G_total < 0 || Gb < 0 || L < 1 || L > PR_MAXL || A < 1 || A > PR_MAXA ||
      (long long)B * L * A > 0x7fffffffLL)
    return CDDMSL_ERR_ARG;
  if (B == 0) return CDDMSL_OK;
  if (!off || !img_idx || !gt_off || !limits || !cover_off || !over || ((uintptr_t)boxes & 15) || ((uintptr_t)gt_boxes & 15))
    return CDDMSL_ERR_ARG;
  if (P_total > 0 && (!boxes || !logits)) return CDDMSL_ERR_ARG;
  if (G_total > 0 && (!gt_boxes || !gt_rng)) return CDDMSL_ERR_ARG;
  if (Gb > 0 && !cover) return CDDMSL_ERR_ARG;
  k_proposal_cover<<<dim3((unsigned)(B * L * A)), dim3(PR_THREADS), 0, (hipStream_t)stream>>>(
      boxes, logits, (const long long*)off, (const long long*)img_idx, (long long)P_total, gt_boxes, gt_rng, (const long long*)gt_off,
      (long long)n_images, (long long)G_total, limits, L, A, (const long long*)cover_off, (long long)Gb, cover, over);
  return launch_status();
}
