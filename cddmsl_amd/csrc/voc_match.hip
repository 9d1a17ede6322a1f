// Pascal VOC devkit matching on gfx950: class_ap's greedy walk for every (class, image) of a test set, at all IoU thresholds, in
// ONE launch.
//
// Host yardstick reproduced bit for bit: cddmsl_amd/evaluation.py class_ap (detectron2 pascal_voc_evaluation.py voc_eval), called
// once per (class, threshold) on detections that went through the reference's result-file text lines.  What the host does and what
// happens here:
//   float(f"{x0 + 1:.1f}") ...        the text round trip, per detection: rint(double(x) * 10.0) / 10.0 (an f32 times 10 is exact in
//                                     f64, Python rounds the exact value half-even, the division is the nearest double, which is
//                                     what float("...") returns); the + 1 on xmin / ymin is an f32 addition
//   order = argsort(-confidence)      stays on the host (it needs the whole class): the caller hands over `perm`, the detections
//                                     segment by segment -- a segment is one (class, image) -- in that order inside each segment.
//                                     Only detections of one (class, image) interact, so the segments are independent
//   ov = inter / union; argmax        f64, the host's operations in the host's order, contraction off; lanes stride over the
//                                     segment's boxes and the wave reduces (overlap, index) to the FIRST maximum with shuffles
//                                     (np.argmax: a NaN counts as the maximum, the first NaN wins)
//   the walk, once per threshold      the ten walks read the same best / arg: `best > thr` becomes a T-bit mask (ballot), the box's
//                                     claimed state is T bits in a workspace, and tp / fp fall out as mask operations
// Structure: ONE WAVE per segment; detections of a segment one after the other (the claimed bits make them sequential).  Lane g
// keeps box g of the segment in registers; a segment with more than 64 boxes reads the rest from global memory per detection.
// There is NO cap on boxes or detections per segment.  No atomics: tp / fp of a detection, the claimed bits of a ground-truth row and
// bad[s] each have one writer (lane 0 of the segment's wave, provided perm lists a detection once and seg_gt a row once).
#include "common.h"
#include "box_iou.h"

namespace {

// np.argmax's order: does (v, box g) stand before (b, box a)?  A negative index is "nothing yet".
__device__ __forceinline__ bool vm_before(double v, int g, double b, int a) {
  if (g < 0) return false;
  if (a < 0) return true;
  const bool nv = v != v, nb = b != b;
  if (nv != nb) return nv;
  if (!nv && v != b) return v > b;
  return g < a;
}

// class_ap's overlap of detection (bx0, by0, bx1, by1), area barea, with ground-truth box (g0, g1, g2, g3)
__device__ __forceinline__ double vm_overlap(double bx0, double by0, double bx1, double by1, double barea, double g0, double g1, double g2,
                                             double g3) {
  const double iw = np_max(np_min(g2, bx1) - np_max(g0, bx0) + 1.0, 0.0);
  const double ih = np_max(np_min(g3, by1) - np_max(g1, by0) + 1.0, 0.0);
  const double inter = iw * ih;
  const double uni = barea + (g2 - g0 + 1.0) * (g3 - g1 + 1.0) - inter;
  return inter / uni;
}

__global__ __launch_bounds__(64) void k_voc_match(const float* __restrict__ boxes, long long D, const long long* __restrict__ perm, long long P,
                                                  const long long* __restrict__ seg_off, const long long* __restrict__ seg_gt,
                                                  const double* __restrict__ gt_boxes, const unsigned char* __restrict__ gt_difficult,
                                                  const long long* __restrict__ gt_off, long long R, long long G,
                                                  const double* __restrict__ thrs, int T, unsigned short* __restrict__ tp,
                                                  unsigned short* __restrict__ fp, unsigned short* claimed, int* __restrict__ bad) {
  const int lane = threadIdx.x;
  const long long s = blockIdx.x;
  const long long d0 = seg_off[s], d1 = seg_off[s + 1], row = seg_gt[s];
  bool ok = d0 >= 0 && d1 >= d0 && d1 <= P && row >= 0 && row < R;       // (uniform)
  long long g0 = 0, g1 = 0;
  if (ok) {
    g0 = gt_off[row];
    g1 = gt_off[row + 1];
    ok = g0 >= 0 && g1 >= g0 && g1 <= G && g1 - g0 <= 0x7fffffffLL;
  }
  if (!ok) {                                      // inconsistent offsets: nothing is read or written beyond this flag
    if (lane == 0) bad[s] = 1;
    return;
  }
  const int Gk = (int)(g1 - g0);
  const bool has = lane < Gk;
  double r0 = 0.0, r1 = 0.0, r2 = 0.0, r3 = 0.0;
  if (has) {
    const double* q = gt_boxes + 4 * (g0 + lane);
    r0 = q[0]; r1 = q[1]; r2 = q[2]; r3 = q[3];
  }
  const double thr = lane < T ? thrs[lane] : 0.0;
  const unsigned tmask = (1u << T) - 1u;
  int nbad = 0;
  for (long long j = d0; j < d1; ++j) {
    const long long p = perm[j];
    if (p < 0 || p >= D) {                        // (uniform) not a detection: skipped, the segment is flagged
      nbad = 1;
      continue;
    }
    const f32x4 bx = ((const f32x4*)boxes)[p];
    const double bx0 = rint((double)(bx.x + 1.0f) * 10.0) / 10.0, by0 = rint((double)(bx.y + 1.0f) * 10.0) / 10.0;
    const double bx1 = rint((double)bx.z * 10.0) / 10.0, by1 = rint((double)bx.w * 10.0) / 10.0;
    const double barea = (bx1 - bx0 + 1.0) * (by1 - by0 + 1.0);
    double best = -INFINITY;
    int arg = -1;
    if (has) {
      best = vm_overlap(bx0, by0, bx1, by1, barea, r0, r1, r2, r3);
      arg = lane;
    }
    for (int g = lane + 64; g < Gk; g += 64) {
      const double* q = gt_boxes + 4 * (g0 + g);
      const double v = vm_overlap(bx0, by0, bx1, by1, barea, q[0], q[1], q[2], q[3]);
      if (vm_before(v, g, best, arg)) { best = v; arg = g; }
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {           // butterfly over a total order: every lane ends with the first maximum
      const double ob = __shfl_xor(best, m, 64);
      const int oa = __shfl_xor(arg, m, 64);
      if (vm_before(ob, oa, best, arg)) { best = ob; arg = oa; }
    }
    const unsigned above = (unsigned)__ballot(lane < T && best > thr);      // bit t: best > thrs[t] (false for a NaN and for -inf)
    if (lane == 0) {
      unsigned t_ = 0u, f_ = ~above & tmask;
      if (above != 0u && arg >= 0 && gt_difficult[g0 + arg] == 0) {
        const unsigned c = claimed[g0 + arg];
        t_ = above & ~c;
        f_ |= above & c;
        claimed[g0 + arg] = (unsigned short)(c | above);
      }
      tp[p] = (unsigned short)t_;
      fp[p] = (unsigned short)f_;
    }
  }
  if (lane == 0) bad[s] = nbad;
}

}  // namespace

extern "C" int cddmsl_voc_match(const float* boxes, long D, const long* perm, long P, const long* seg_off, const long* seg_gt, long S,
                                const double* gt_boxes, const unsigned char* gt_difficult, const long* gt_off, long R, long G,
                                const double* thrs, int T, unsigned short* tp, unsigned short* fp, int* bad, void* temp, void* stream) {
  if (D < 0 || P < 0 || S < 0 || R < 0 || G < 0 || T < 1 || T > 16 || S > 0x7fffffffL) return CDDMSL_ERR_ARG;
  if (((uintptr_t)boxes & 15) || ((uintptr_t)gt_boxes & 7) || ((uintptr_t)tp & 1) || ((uintptr_t)fp & 1) || ((uintptr_t)temp & 1))
    return CDDMSL_ERR_ARG;
  if (D > 0 && (!boxes || !tp || !fp)) return CDDMSL_ERR_ARG;
  if (P > 0 && !perm) return CDDMSL_ERR_ARG;
  if (S > 0 && (!seg_off || !seg_gt || !gt_off || !thrs || !bad)) return CDDMSL_ERR_ARG;
  if (G > 0 && (!gt_boxes || !gt_difficult || !temp)) return CDDMSL_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  if (D > 0) {                                    // a detection no segment lists keeps both masks 0
    if (hipMemsetAsync(tp, 0, sizeof(unsigned short) * (size_t)D, st) != hipSuccess) return CDDMSL_ERR_LAUNCH;
    if (hipMemsetAsync(fp, 0, sizeof(unsigned short) * (size_t)D, st) != hipSuccess) return CDDMSL_ERR_LAUNCH;
  }
  if (S == 0) return CDDMSL_OK;
  if (G > 0 && hipMemsetAsync(temp, 0, sizeof(unsigned short) * (size_t)G, st) != hipSuccess) return CDDMSL_ERR_LAUNCH;
  k_voc_match<<<dim3((unsigned)S), dim3(64), 0, st>>>(boxes, (long long)D, (const long long*)perm, (long long)P, (const long long*)seg_off,
                                                     (const long long*)seg_gt, gt_boxes, gt_difficult, (const long long*)gt_off,
                                                     (long long)R, (long long)G, thrs, T, tp, fp, (unsigned short*)temp, bad);
  return launch_status();
}
