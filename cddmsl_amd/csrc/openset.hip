// Open-vocabulary inference on gfx950: region x test-vocabulary cosine logits on the exact-f32 MFMA, and the per-image candidate
// selection that follows it, as one launch sequence with ONE host readback (the candidate count).
//
// Reference call sites replaced (paths under detectron2/):
//   FastRCNNOutputLayers.forward, test_cls_score branch     modeling/roi_heads/fast_rcnn.py:546-565
//   predict_probs (softmax over the K+1 logits)             modeling/roi_heads/fast_rcnn.py:793-810
//   inference (geometric mean with the RPN objectness)      modeling/roi_heads/fast_rcnn.py:706-710
//   fast_rcnn_inference_single_image, up to the NMS         modeling/roi_heads/fast_rcnn.py:155-180
//
// cddmsl_openset_logits -- two kernels, no scratch, no atomics:
//   k_os_logits  grid (class tiles of 128, row panels of 32), 4 waves: wave w owns the 32 x 32 tile of classes 32w.. of its
//                workgroup's class tile and walks D in steps of 8 with Mma<float> (v_mfma_f32_32x32x2_f32, f32 accumulation).  Each
//                lane feeds the MFMA straight from memory: 16 B of its row of x, scaled by the row's 1 / max(||x||, eps) (one
//                rounded multiply per element, the x_hat of k_cosine_logits_fwd, formed with the same summation order), and 16 B
//                of its class's unit embedding.  Nothing is staged in LDS but the 32 inverse norms: a row panel is 128 KiB at
//                D = 1024 and is re-read from L2 by the class tiles, which is what spreads R = 1000 x K = 1203 over 320
//                workgroups instead of 32.  Rows >= R and classes >= K read a clamped (valid) address and store nothing.
//   k_os_stats   one wave per row over the K+1 logits just written (L2-resident): writes the exact 0 of the background column,
//                m = max, l = sum expf(logit - m) in lane-strided order with one wave reduction each.
// The split over classes with a row pass as its merge was chosen over one workgroup per row panel with the statistics in
// registers: the logits are an output anyway, re-reading them costs R (K+1) 4 bytes, and the panel form leaves 7/8 of the CUs idle.
//
// cddmsl_openset_select -- count, scan, write; one wave per row, the row's scores are evaluated twice by the same expression
// (same bits), no atomic decides an order:
//   k_os_count   valid[r] (all ldb box values and all K+1 scores finite) and the row's number of (score > thresh, c < K) entries
//   k_os_scan    exclusive scan of the row counts in one workgroup; the total goes to count[0]
//   k_os_write   entries in (row, class) order -- mask.nonzero()'s -- through a wave ballot and a prefix popcount; each entry
//                carries its row, class, score and the clipped box of that class.  Entries at or beyond cap are not written.
#include "gemm_common.h"

namespace {

constexpr int OS_BM = 32;        // rows of a panel
constexpr int OS_BN = 128;       // classes of a workgroup's tile: 4 waves x 32
constexpr int OS_MAXK = 16384;

__global__ __launch_bounds__(256) void k_os_logits(const float* x, const float* wn, float* logits, int R, int D, int K, int ld, float invT,
                                                   float eps) {
  __shared__ float s_iv[OS_BM];
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const int r0 = blockIdx.y * OS_BM, c0 = blockIdx.x * OS_BN + wv * 32;
  // inverse norms of the panel's rows: 8 rows per wave, k_cosine_logits_fwd's summation order
  for (int i = 0; i < OS_BM / 4; ++i) {
    const int rr = min(r0 + wv * (OS_BM / 4) + i, R - 1);
    const float* xr = x + (size_t)rr * D;
    float ss = 0.f;
    for (int d = lane; d < D; d += 64) ss += xr[d] * xr[d];
    ss = wave_sum(ss);
    if (lane == 0) s_iv[wv * (OS_BM / 4) + i] = 1.0f / fmaxf(sqrtf(ss), eps);
  }
  __syncthreads();
  if (c0 >= K) return;                             // (wave-uniform; no barrier follows)
  const int r = lane & 31, h = lane >> 5;
  const float iv = s_iv[r];
  const float* xa = x + (size_t)min(r0 + r, R - 1) * D;
  const float* wb = wn + (size_t)min(c0 + r, K - 1) * D;
  f32x16 acc;
#pragma unroll
  for (int g = 0; g < 16; ++g) acc[g] = 0.f;
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  for (int kb = 0; kb < D; kb += 8) {              // (wave-uniform trip count; D % 8 == 4 ends on zeros in the upper half-wave)
    const int d0 = kb + 4 * h;
    f32x4 a = zero, b = zero;
    if (d0 < D) {
      a = *(const f32x4*)(xa + d0);
      b = *(const f32x4*)(wb + d0);
      a = a * iv;
    }
    Mma<float>::step(acc, __builtin_bit_cast(u32x4, a), __builtin_bit_cast(u32x4, b));
  }
  const int c = c0 + r;
  if (c >= K) return;
#pragma unroll
  for (int g = 0; g < 16; ++g) {
    const int row = r0 + (g & 3) + 8 * (g >> 2) + 4 * h;
    if (row < R) logits[(size_t)row * ld + c] = acc[g] * invT;
  }
}

__global__ __launch_bounds__(256) void k_os_stats(float* logits, float* stats, int R, int K, int ld) {
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (r >= R) return;
  float* lr = logits + (size_t)r * ld;
  float m = 0.f;                                   // the background logit
  for (int c = lane; c < K; c += 64) m = fmaxf(m, lr[c]);
  m = wave_max(m);
  float l = 0.f;
  for (int c = lane; c <= K; c += 64) l += expf((c < K ? lr[c] : 0.f) - m);
  l = wave_sum(l);
  if (lane == 0) { lr[K] = 0.f; stats[2 * r] = m; stats[2 * r + 1] = l; }
}

__device__ __forceinline__ bool os_finite(float v) { return fabsf(v) <= 3.402823466e38f; }   // false for NaN and +-inf

__device__ __forceinline__ float os_score(float logit, float m, float l, bool has_obj, float obj) {
  const float p = expf(logit - m) / l;
  return has_obj ? sqrtf(p * obj) : p;
}

__global__ __launch_bounds__(256) void k_os_count(const float* logits, const float* stats, int ld, const float* boxes, int ldb,
                                                  const float* objectness, int R, int K, float thresh, unsigned char* valid, int* rowcnt) {
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (r >= R) return;
  const float* lr = logits + (size_t)r * ld;
  const float m = stats[2 * r], l = stats[2 * r + 1];
  const bool has_obj = objectness != nullptr;
  const float obj = has_obj ? objectness[r] : 0.f;
  int bad = 0, n = 0;
  for (int j = lane; j < ldb; j += 64) bad |= !os_finite(boxes[(size_t)r * ldb + j]);
  for (int c = lane; c <= K; c += 64) {
    const float s = os_score(lr[c], m, l, has_obj, obj);
    bad |= !os_finite(s);
    n += (c < K && s > thresh) ? 1 : 0;
  }
  bad = __any(bad);
  n = (int)wave_sum((float)n);                     // (<= 16384 per row: exact in f32)
  if (lane == 0) { valid[r] = bad ? 0 : 1; rowcnt[r] = bad ? 0 : n; }
}

__global__ __launch_bounds__(1024) void k_os_scan(const int* cnt, int* off, int* total, int R) {
  __shared__ int ws[16];
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  int carry = 0;
  for (int base = 0; base < R; base += 1024) {
    const int i = base + t;
    const int v = i < R ? cnt[i] : 0;
    int s = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int y = __shfl_up(s, o, 64);
      if (lane >= o) s += y;
    }
    if (lane == 63) ws[wv] = s;
    __syncthreads();
    int before = 0, all = 0;
    for (int w = 0; w < 16; ++w) { before += w < wv ? ws[w] : 0; all += ws[w]; }
    if (i < R) off[i] = carry + before + s - v;
    carry += all;
    __syncthreads();
  }
  if (t == 0) total[0] = carry;
}

__global__ __launch_bounds__(256) void k_os_write(const float* logits, const float* stats, int ld, const float* boxes, int ldb,
                                                  const float* objectness, int R, int K, float img_h, float img_w, float thresh,
                                                  const unsigned char* valid, const int* rowoff, int* cand_row, int* cand_cls,
                                                  float* cand_score, float* cand_box, int cap) {
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (r >= R || !valid[r]) return;                 // (wave-uniform)
  const float* lr = logits + (size_t)r * ld;
  const float m = stats[2 * r], l = stats[2 * r + 1];
  const bool has_obj = objectness != nullptr;
  const float obj = has_obj ? objectness[r] : 0.f;
  int pos = rowoff[r];
  for (int cb = 0; cb < K; cb += 64) {
    const int c = cb + lane;
    float s = 0.f;
    bool sel = false;
    if (c < K) {
      s = os_score(lr[c], m, l, has_obj, obj);
      sel = s > thresh;
    }
    const unsigned long long mask = __ballot(sel);
    if (sel) {
      const int p = pos + __popcll(mask & ((1ull << lane) - 1ull));
      if (p < cap) {
        const f32x4 b = *(const f32x4*)(boxes + (size_t)r * ldb + (ldb == 4 ? 0 : 4 * c));
        f32x4 o;                                   // Boxes.clip: x to [0, w], y to [0, h]
        o.x = fminf(fmaxf(b.x, 0.f), img_w);
        o.y = fminf(fmaxf(b.y, 0.f), img_h);
        o.z = fminf(fmaxf(b.z, 0.f), img_w);
        o.w = fminf(fmaxf(b.w, 0.f), img_h);
        cand_row[p] = r;
        cand_cls[p] = c;
        cand_score[p] = s;
        ((f32x4*)cand_box)[p] = o;
      }
    }
    pos += __popcll(mask);
  }
}

}  // namespace

extern "C" int cddmsl_openset_logits(const float* x, const float* wn, float* logits, float* stats, int R, int D, int K, int ld,
                                     float temperature, float eps, void* stream) {
  if (R < 0 || D < 4 || (D & 3) || K < 1 || K > OS_MAXK || ld < K + 1 || !(temperature > 0.f)) return CDDMSL_ERR_ARG;
  if (R == 0) return CDDMSL_OK;
  if (!x || !wn || !logits || !stats) return CDDMSL_ERR_ARG;
  if (((uintptr_t)x | (uintptr_t)wn) & 15) return CDDMSL_ERR_ARG;          // rows of x and wn are read as 16-byte vectors (D % 4 == 0)
  hipStream_t st = (hipStream_t)stream;
  const float invT = 1.0f / temperature;
  k_os_logits<<<dim3((K + OS_BN - 1) / OS_BN, (R + OS_BM - 1) / OS_BM), dim3(256), 0, st>>>(x, wn, logits, R, D, K, ld, invT, eps);
  k_os_stats<<<dim3((R + 3) / 4), dim3(256), 0, st>>>(logits, stats, R, K, ld);
  return launch_status();
}

extern "C" int cddmsl_openset_select(const float* logits, const float* stats, int ld, const float* boxes, int ldb, const float* objectness,
                                     int R, int K, float img_h, float img_w, float score_thresh, int* cand_row, int* cand_cls,
                                     float* cand_score, float* cand_box, unsigned char* valid, int* count, int cap, void* temp,
                                     size_t* temp_bytes, void* stream) {
  if (R < 0 || K < 1 || K > OS_MAXK || ld < K + 1 || (ldb != 4 && ldb != 4 * K) || cap < 0 || !temp_bytes) return CDDMSL_ERR_ARG;
  const size_t rb = (((size_t)R * 4) + 255) & ~(size_t)255, total = 2 * rb;
  if (!temp) { *temp_bytes = total; return CDDMSL_OK; }
  if (*temp_bytes < total || !count) return CDDMSL_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  if (R == 0) return hipMemsetAsync(count, 0, sizeof(int), st) == hipSuccess ? CDDMSL_OK : CDDMSL_ERR_LAUNCH;
  if (!logits || !stats || !boxes || !valid || (cap > 0 && (!cand_row || !cand_cls || !cand_score || !cand_box))) return CDDMSL_ERR_ARG;
  if (((uintptr_t)boxes | (uintptr_t)cand_box) & 15) return CDDMSL_ERR_ARG;   // a box is read and written as one 16-byte vector
  int* rowcnt = (int*)temp;
  int* rowoff = (int*)((char*)temp + rb);
  const unsigned blocks = (unsigned)((R + 3) / 4);
  k_os_count<<<dim3(blocks), dim3(256), 0, st>>>(logits, stats, ld, boxes, ldb, objectness, R, K, score_thresh, valid, rowcnt);
  k_os_scan<<<dim3(1), dim3(1024), 0, st>>>(rowcnt, rowoff, count, R);
  k_os_write<<<dim3(blocks), dim3(256), 0, st>>>(logits, stats, ld, boxes, ldb, objectness, R, K, img_h, img_w, score_thresh, valid, rowoff,
                                                 cand_row, cand_cls, cand_score, cand_box, cap);
  return launch_status();
}
