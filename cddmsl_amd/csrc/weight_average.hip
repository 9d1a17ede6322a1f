// Weight averaging during training (MODEL_EMA: EMA / SWA) on gfx950: cddmsl_weight_average, one multi-tensor launch family in the
// style of cddmsl_sgd_step_groups (elementwise.hip), linked into a library of its own (see include/cddmsl_weight_average.h for why).
#include "common.h"
#include "cddmsl_weight_average.h"   // the compiler checks the entry point's definition against its declaration

namespace {

// avg += w (p - avg) per element (torch.lerp's expression for w < 0.5, what torch.optim.swa_utils computes), or avg = p bit for bit.
// p is only read.  The batch travels by value like SgdGBatch: 128 items of 24 bytes + 129 chunk offsets + the scalars = 3596 bytes of
// kernel arguments.  Unlike k_sgd_groups the grid is ONE-SHOT and flat: a block takes one chunk of AVG_CHUNK elements of one tensor and
// finds the tensor by bisecting c0 (c0[i] = chunks of the tensors before i).  With grid.y = tensor and one grid.x for all, the largest
// tensor of the detector (9.4 M of 48.4 M elements) was left to 256 looping blocks when every other tensor had finished: measured 0.234 ms
// against 0.143 ms for torch._foreach_lerp_, whose chunks are balanced the same way as these.
struct AvgItem { float* e; const float* p; long n; };
constexpr int AVG_MAX = 128;
constexpr int AVG_CHUNK = 4096;                   // elements per block: 256 threads x 4 accesses of 16 bytes
constexpr long AVG_MAX_SIZE = (long)AVG_CHUNK << 30;   // per tensor, so that a batch's chunk count stays far inside an int
struct AvgBatch { AvgItem it[AVG_MAX]; int c0[AVG_MAX + 1]; int count; };
static_assert(sizeof(AvgBatch) + 4 + 256 <= 4096, "AvgBatch + scalar + hidden arguments exceed the kernel-argument limit");

template <int COPY>
__device__ __forceinline__ float avg_one(float e, float p, float w) { return COPY ? p : e + w * (p - e); }

template <int COPY>
__global__ void __launch_bounds__(256) k_weight_average(AvgBatch b, float w) {
  int lo = 0, hi = b.count;                       // the tensor of this block: the last one with c0 <= blockIdx.x
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (b.c0[mid] <= (int)blockIdx.x) lo = mid; else hi = mid;
  }
  const AvgItem& t = b.it[lo];
  const long base = (long)((int)blockIdx.x - b.c0[lo]) * AVG_CHUNK;
  const long end = base + AVG_CHUNK < t.n ? base + AVG_CHUNK : t.n;
  // 16-byte accesses when e and p are both 16-byte aligned (a chunk starts at a multiple of 4 elements), scalar otherwise and for the
  // last n % 4 elements, which belong to the tensor's last chunk
  if (((((size_t)t.e) | ((size_t)t.p)) & 15) == 0) {
    const long j0 = (base >> 2) + threadIdx.x, j1 = end >> 2;
    float4 p[4], e[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const long j = j0 + k * 256;
      if (j < j1) {
        p[k] = ((const float4*)t.p)[j];
        if (!COPY) e[k] = ((const float4*)t.e)[j];
      }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const long j = j0 + k * 256;
      if (j < j1) {
        float4 r;
        r.x = avg_one<COPY>(e[k].x, p[k].x, w);
        r.y = avg_one<COPY>(e[k].y, p[k].y, w);
        r.z = avg_one<COPY>(e[k].z, p[k].z, w);
        r.w = avg_one<COPY>(e[k].w, p[k].w, w);
        ((float4*)t.e)[j] = r;
      }
    }
    const long i = (j1 << 2) + threadIdx.x;
    if (i < end) t.e[i] = avg_one<COPY>(COPY ? 0.f : t.e[i], t.p[i], w);
  } else {
    for (long i = base + threadIdx.x; i < end; i += 256) t.e[i] = avg_one<COPY>(COPY ? 0.f : t.e[i], t.p[i], w);
  }
}

}  // namespace

// Weight averaging after the step: avg / params are host pointer arrays as above; tensors are batched AVG_MAX per launch, empty ones left
// out of the batch.  Every argument is checked before the first launch.
extern "C" int cddmsl_weight_average(float** avg, const float** params, const long* sizes, int count, float w, int copy, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (count < 0) return CDDMSL_ERR_ARG;
  if (!copy && !(w >= 0.0f && w <= 1.0f)) return CDDMSL_ERR_ARG;      // (a NaN fails both comparisons)
  for (int i = 0; i < count; ++i) if (sizes[i] < 0 || sizes[i] > AVG_MAX_SIZE) return CDDMSL_ERR_ARG;
  bool launched = false;
  for (int base = 0; base < count;) {
    AvgBatch b;
    b.count = 0;
    long chunks = 0;
    for (; base < count && b.count < AVG_MAX; ++base) {
      if (sizes[base] == 0) continue;
      const long c = (sizes[base] + AVG_CHUNK - 1) / AVG_CHUNK;
      if (chunks + c > 0x7fffffffL) break;                             // (the next launch takes it)
      b.it[b.count].e = avg[base]; b.it[b.count].p = params[base]; b.it[b.count].n = sizes[base];
      b.c0[b.count++] = (int)chunks;
      chunks += c;
    }
    if (b.count == 0) break;
    for (int i = b.count; i <= AVG_MAX; ++i) b.c0[i] = (int)chunks;
    if (copy) k_weight_average<1><<<dim3((unsigned)chunks), dim3(256), 0, st>>>(b, w);
    else k_weight_average<0><<<dim3((unsigned)chunks), dim3(256), 0, st>>>(b, w);
    launched = true;
  }
  return launched ? launch_status() : CDDMSL_OK;
}
