// COCO box matching on gfx950: COCOeval.evaluateImg's greedy walk for every (image, class) of a batch in ONE launch.
//
// Host yardstick reproduced bit for bit: cddmsl_amd/evaluation.py _coco_match + coco_box_iou (pycocotools cocoeval.py evaluateImg,
// maskUtils.iou on boxes), called once per (image, class, area range).  What the host does per call and what happens here:
//   dorder = argsort(-score, mergesort)[:max_dets]   rank = #{better detections of the same (image, class)}: a total order (score
//                                                    descending, NaN last, equal scores by input index), so no sort is needed
//   gorder = argsort(gt_ig, mergesort)               the stable partition "non-ignored first", one per area range (gt_ig depends on it)
//   ious   = coco_box_iou(dt, gt, crowd)             f64, the host's operations in the host's order; independent of the area range,
//                                                    so ONE row per detection serves all walks
//   the T x D x G walk                               lane a * T + t walks (threshold t, range a): the walks are independent of each
//                                                    other and sequential in the detection index
// Structure: ONE WAVE per (image, class).  The class's detections and ground-truth boxes are compacted into LDS in input order
// (ballot + popcount), ranks are counted from LDS, and then detection after detection the wave computes that detection's IoU row
// cooperatively into LDS (two rows alternate, one barrier per detection) and the T * A lanes walk it.  Each lane keeps the
// matched set of ITS walk as 256 bits in LDS, indexed by the box's position in its range's order.  The wave's ballot of the
// lanes' flags IS the output mask (bit a * T + t).  No atomics anywhere; every output element has exactly one writer.
//
// Caps (reported by the Python wrapper): CM_MAXD detections and CM_MAXG ground-truth boxes of one class in one image, CM_KEEP kept
// detections.  An (image, class) beyond a cap sets over[b] = 1 and writes nothing: the caller matches that image on the host, it
// is never truncated.  rank is pre-set to -1 and the masks to 0, so a detection no wave owns (class outside [0, K)) is dropped.
#include "common.h"
#include "box_iou.h"

namespace {

constexpr int CM_MAXD = 1024;     // detections of one class in one image
constexpr int CM_MAXG = 256;      // ground-truth boxes of one class in one image
constexpr int CM_KEEP = 128;      // kept detections per (image, class): max_dets <= CM_KEEP

__global__ __launch_bounds__(64) void k_coco_match(const float* __restrict__ dt_boxes, const float* __restrict__ dt_scores,
                                                   const long long* __restrict__ dt_cls, const long long* __restrict__ dt_off,
                                                   const long long* __restrict__ img_idx, long long D_total, long long n_images,
                                                   const double* __restrict__ gt_xywh, const double* __restrict__ gt_area,
                                                   const unsigned char* __restrict__ gt_crowd, const long long* __restrict__ gt_cls,
                                                   const long long* __restrict__ gt_off, const double* __restrict__ thrs, int T,
                                                   const double* __restrict__ rngs, int A, int K, int max_dets, int* __restrict__ rank,
                                                   long long* __restrict__ matched, long long* __restrict__ ignored, int* __restrict__ over) {
  __shared__ int s_didx[CM_MAXD];                 // detections of this class, in input order: offset inside the image
  __shared__ float s_score[CM_MAXD];
  __shared__ int s_kd[CM_KEEP];                   // rank -> position in s_didx
  __shared__ double s_db[CM_KEEP][4], s_da[CM_KEEP];
  __shared__ double s_gb[CM_MAXG][4], s_ga[CM_MAXG], s_gfield[CM_MAXG];
  __shared__ unsigned char s_gcrowd[CM_MAXG];
  __shared__ unsigned short s_gord[4][CM_MAXG];   // per range: position -> box (non-ignored first, stable)
  __shared__ unsigned char s_gig[4][CM_MAXG];     // per range, by position: ignored
  __shared__ double s_iou[2][CM_MAXG];
  __shared__ unsigned int s_gtm[CM_MAXG / 32][64];  // per lane: matched set of its walk, bit = position

  const int lane = threadIdx.x;
  const int b = blockIdx.x / K, k = blockIdx.x % K;
  const long long d0 = dt_off[b], d1 = dt_off[b + 1], im = img_idx[b];
  if (d0 < 0 || d1 < d0 || d1 > D_total || im < 0 || im >= n_images) {       // (uniform) inconsistent offsets: leave it to the host
    if (lane == 0) over[b] = 1;
    return;
  }
  const unsigned long long below = (1ull << lane) - 1ull;

  // ---- this class's detections, in input order
  int Dk = 0;
  for (long long base = d0; base < d1; base += 64) {
    const long long i = base + lane;
    const bool f = i < d1 && dt_cls[i] == (long long)k;
    const unsigned long long m = __ballot(f);
    if (f) {
      const int pos = Dk + __popcll(m & below);
      if (pos < CM_MAXD) { s_didx[pos] = (int)(i - d0); s_score[pos] = dt_scores[i]; }
    }
    Dk += __popcll(m);
  }
  if (Dk == 0) return;                            // nothing to write for this (image, class)
  if (Dk > CM_MAXD) {
    if (lane == 0) over[b] = 1;
    return;
  }
  // ---- this class's ground truth, in input order
  const long long g0 = gt_off[im], g1 = gt_off[im + 1];
  int Gk = 0;
  for (long long base = g0; base < g1; base += 64) {
    const long long i = base + lane;
    const bool f = i < g1 && gt_cls[i] == (long long)k;
    const unsigned long long m = __ballot(f);
    if (f) {
      const int pos = Gk + __popcll(m & below);
      if (pos < CM_MAXG) {
        const double x = gt_xywh[4 * i], y = gt_xywh[4 * i + 1], w = gt_xywh[4 * i + 2], h = gt_xywh[4 * i + 3];
        s_gb[pos][0] = x; s_gb[pos][1] = y; s_gb[pos][2] = w; s_gb[pos][3] = h;
        s_ga[pos] = w * h;
        s_gfield[pos] = gt_area[i];
        s_gcrowd[pos] = gt_crowd[i] != 0;
      }
    }
    Gk += __popcll(m);
  }
  if (Gk > CM_MAXG) {
    if (lane == 0) over[b] = 1;
    return;
  }
  __syncthreads();

  // ---- ranks; the kept detections in rank order
  for (int p = lane; p < Dk; p += 64) {
    const float sp = s_score[p];
    int r = 0;
    for (int q = 0; q < Dk; ++q) r += score_before(s_score[q], q, sp, p) ? 1 : 0;
    const bool kept = r < max_dets;
    if (kept) s_kd[r] = p;
    rank[d0 + s_didx[p]] = kept ? r : -1;
  }
  // ---- per range: the stable partition of the ground truth (lane a does range a; a few hundred steps)
  if (lane < A) {
    const double lo = rngs[2 * lane], hi = rngs[2 * lane + 1];
    int n = 0;
    for (int pass = 0; pass < 2; ++pass)
      for (int g = 0; g < Gk; ++g) {
        const double ar = s_gfield[g];
        const bool ig = s_gcrowd[g] || ar < lo || ar > hi;
        if ((int)ig == pass) { s_gord[lane][n] = (unsigned short)g; s_gig[lane][n] = ig; ++n; }
      }
  }
#pragma unroll
  for (int w = 0; w < CM_MAXG / 32; ++w) s_gtm[w][lane] = 0u;
  __syncthreads();
  const int Dn = Dk < max_dets ? Dk : max_dets;
  for (int j = lane; j < Dn; j += 64) {
    const f32x4 bx = ((const f32x4*)dt_boxes)[d0 + s_didx[s_kd[j]]];
    const double x0 = (double)bx.x, y0 = (double)bx.y, x1 = (double)bx.z, y1 = (double)bx.w;
    const double w = x1 - x0, h = y1 - y0;
    s_db[j][0] = x0; s_db[j][1] = y0; s_db[j][2] = w; s_db[j][3] = h;
    s_da[j] = w * h;
  }
  __syncthreads();

  const int nwalk = T * A;
  const int wa = lane < nwalk ? lane / T : 0, wt = lane < nwalk ? lane % T : 0;
  const double thr = thrs[wt], rlo = rngs[2 * wa], rhi = rngs[2 * wa + 1];
  for (int d = 0; d < Dn; ++d) {
    double* row = s_iou[d & 1];
    const double dx = s_db[d][0], dy = s_db[d][1], dw = s_db[d][2], dh = s_db[d][3], da = s_da[d];
    for (int g = lane; g < Gk; g += 64) {
      const double gx = s_gb[g][0], gy = s_gb[g][1], gw = s_gb[g][2], gh = s_gb[g][3];
      const double iw = np_min(dx + dw, gx + gw) - np_max(dx, gx);
      const double ih = np_min(dy + dh, gy + gh) - np_max(dy, gy);
      const double inter = np_max(iw, 0.0) * np_max(ih, 0.0);
      const double uni = s_gcrowd[g] ? da : da + s_ga[g] - inter;
      row[g] = inter / uni;
    }
    __syncthreads();      // the row is complete; the previous detection's walks (on the other row) are over
    bool dtm = false, dtig = false;
    if (lane < nwalk) {
      double iou = thr;
      int m = -1;
      for (int j = 0; j < Gk; ++j) {
        const int g = s_gord[wa][j];
        const bool crowd = s_gcrowd[g] != 0;
        if (((s_gtm[j >> 5][lane] >> (j & 31)) & 1u) && !crowd) continue;
        if (m > -1 && !s_gig[wa][m] && s_gig[wa][j]) break;
        const double v = row[g];
        if (v < iou) continue;                    // (a NaN is never below: it is taken, and nothing is below it afterwards)
        iou = v;
        m = j;
      }
      if (m > -1) {
        dtm = true;
        dtig = s_gig[wa][m] != 0;
        s_gtm[m >> 5][lane] |= 1u << (m & 31);
      } else {
        dtig = da < rlo || da > rhi;
      }
    }
    const unsigned long long mm = __ballot(dtm), mi = __ballot(dtig);
    if (lane == 0) {
      const long long i = d0 + s_didx[s_kd[d]];
      matched[i] = (long long)mm;
      ignored[i] = (long long)mi;
    }
  }
}

}  // namespace

extern "C" int cddmsl_coco_match(const float* dt_boxes, const float* dt_scores, const long* dt_cls, const long* dt_off, const long* img_idx,
                                 int B, long D_total, const double* gt_xywh, const double* gt_area, const unsigned char* gt_crowd,
                                 const long* gt_cls, const long* gt_off, long n_images, const double* thrs, int T, const double* area_rngs,
                                 int A, int K, int max_dets, int* rank, long* matched, long* ignored, int* over, void* stream) {
  if (B < 0 || D_total < 0 || n_images < 0 || T < 1 || A < 1 || A > 4 || T * A > 64 || K < 1 || max_dets < 1 || max_dets > CM_KEEP ||
      (long long)B * K > 0x7fffffffLL)
    return CDDMSL_ERR_ARG;
  if (B == 0) return CDDMSL_OK;
  if (!dt_off || !img_idx || !gt_off || !thrs || !area_rngs || !over || ((uintptr_t)dt_boxes & 15)) return CDDMSL_ERR_ARG;
  if (D_total > 0 && (!dt_boxes || !dt_scores || !dt_cls || !rank || !matched || !ignored)) return CDDMSL_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(over, 0, sizeof(int) * (size_t)B, st) != hipSuccess) return CDDMSL_ERR_LAUNCH;
  if (D_total > 0) {
    if (hipMemsetAsync(rank, 0xff, sizeof(int) * (size_t)D_total, st) != hipSuccess) return CDDMSL_ERR_LAUNCH;
    if (hipMemsetAsync(matched, 0, sizeof(long long) * (size_t)D_total, st) != hipSuccess) return CDDMSL_ERR_LAUNCH;
    if (hipMemsetAsync(ignored, 0, sizeof(long long) * (size_t)D_total, st) != hipSuccess) return CDDMSL_ERR_LAUNCH;
  }
  k_coco_match<<<dim3((unsigned)(B * K)), dim3(64), 0, st>>>(
      dt_boxes, dt_scores, (const long long*)dt_cls, (const long long*)dt_off, (const long long*)img_idx, (long long)D_total,
      (long long)n_images, gt_xywh, gt_area, gt_crowd, (const long long*)gt_cls, (const long long*)gt_off, thrs, T, area_rngs, A, K,
      max_dets, rank, (long long*)matched, (long long*)ignored, over);
  return launch_status();
}
