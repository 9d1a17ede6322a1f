// Sparse backward pass of the RPN head (3x3 conv + ReLU -> fused objectness / delta heads).  The sampled RPN loss leaves the
// gradient of the heads' output non-zero on at most BATCH_SIZE_PER_IMAGE rows per image (rpn.py:365-429), so the two long GEMMs of
// the 3x3 convolution's backward run over those rows only.  The kernels here are the bookkeeping around the existing GEMM entry
// points: find the active rows, gather operand rows, and sum the per-tap partial input gradients back onto the map.
//   mark     marks[p]   = 1 where row p of dy holds anything but +-0 (a NaN counts: the dense route would spread it too)
//   compact  rows[cap]  = the marked positions in ascending order, -1 behind them; slot[p] = index of p in rows or -1;
//                         *overflow = 1 when more than cap rows are marked (the rows past cap are dropped: the caller must raise)
//   gather   dst[s][:]  = src[rows[s]][:] in the compute dtype (src may be f32), zeros for rows[s] < 0
//   im2col   X[s][tap][c] = x[n][h + kh - pad][w + kw - pad][c] of position rows[s] = (n, h, w), zeros outside the image
//   dx       dx[p][c]   = sum over taps, in tap order, of P[tap][slot[p + tap - pad]][c]  (f32 partials, rounded once)
// No atomics: every output element has one writer and a fixed summation order.
// Declared in include/cddmsl_hip.h with every other entry point of libcddmsl_hip.so (common.h includes it: the compiler checks
// each definition against its declaration).
#include "common.h"

namespace {

inline unsigned grid_for(long n, int per = 256) {
  long b = (n + per - 1) / per;
  return (unsigned)(b < 1 ? 1 : (b > 65536 ? 65536 : b));
}

// one block per 256 rows: the block's 16-byte chunks are read back to back, a non-zero chunk raises its row's flag in LDS
// (every writer stores the same 1: no atomic needed)
__global__ __launch_bounds__(256) void k_rpn_mark_rows(const u32x4* __restrict__ dy, int* __restrict__ marks, long rows, int cpr, unsigned absmask) {
  __shared__ int flag[256];
  for (long r0 = (long)blockIdx.x * 256; r0 < rows; r0 += (long)gridDim.x * 256) {
    flag[threadIdx.x] = 0;
    __syncthreads();
    const long nr = rows - r0 < 256 ? rows - r0 : 256, nch = nr * cpr;
    const u32x4* base = dy + r0 * cpr;
    for (long i = threadIdx.x; i < nch; i += 256) {
      const u32x4 v = base[i];
      if ((v[0] | v[1] | v[2] | v[3]) & absmask) flag[(unsigned)i / (unsigned)cpr] = 1;
    }
    __syncthreads();
    if (threadIdx.x < nr) marks[r0 + threadIdx.x] = flag[threadIdx.x];
    __syncthreads();
  }
}

// ONE block of 16 waves.  Wave w owns the contiguous span [w * span, (w + 1) * span) and walks it 64 positions at a time (coalesced):
// a ballot gives the step's marks, a popcount below the lane its rank.  Pass 1 counts per wave, LDS holds the 16 totals, pass 2 writes.
__global__ __launch_bounds__(1024) void k_rpn_compact(const int* __restrict__ marks, int* __restrict__ rows, int* __restrict__ slot,
                                                      int* __restrict__ overflow, int M, int cap) {
  __shared__ int wtot[16];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int span = (((M + 15) / 16) + 63) / 64 * 64;
  const long lo = (long)wv * span;
  const long hi = lo + span < M ? lo + span : M;
  int cnt = 0;
  for (long i0 = lo; i0 < hi; i0 += 64) {
    const long i = i0 + lane;
    const bool m = i < hi && marks[i] != 0;
    cnt += __popcll(__ballot(m));
  }
  if (lane == 0) wtot[wv] = cnt;
  __syncthreads();
  int base = 0, total = 0;
  for (int k = 0; k < 16; ++k) { if (k < wv) base += wtot[k]; total += wtot[k]; }
  for (long i0 = lo; i0 < hi; i0 += 64) {
    const long i = i0 + lane;
    const bool m = i < hi && marks[i] != 0;
    const unsigned long long b = __ballot(m);
    if (i < hi) {
      const int s = base + __popcll(b & ((1ull << lane) - 1ull));
      if (m && s < cap) { rows[s] = (int)i; slot[i] = s; }
      else slot[i] = -1;
    }
    base += __popcll(b);
  }
  for (int j = total + threadIdx.x; j < cap; j += 1024) rows[j] = -1;
  if (threadIdx.x == 0 && total > cap) *overflow = 1;
}

// one thread per 16-byte chunk of dst; SRC32: the source rows are f32 and T is bf16 (two source chunks per destination chunk)
template <bool SRC32>
__global__ __launch_bounds__(256) void k_rpn_gather_rows(const u32x4* __restrict__ src, const int* __restrict__ rows, u32x4* __restrict__ dst,
                                                         long nch, int cpr) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < nch; i += (long)gridDim.x * 256) {
    const int s = (int)(i / cpr), c = (int)(i - (long)s * cpr);
    const int r = rows[s];
    u32x4 o = {0u, 0u, 0u, 0u};
    if (r >= 0) {
      if constexpr (SRC32) {
        const f32x4 a = __builtin_bit_cast(f32x4, src[((long)r * cpr + c) * 2]), b = __builtin_bit_cast(f32x4, src[((long)r * cpr + c) * 2 + 1]);
        o[0] = pack2bf(a[0], a[1]); o[1] = pack2bf(a[2], a[3]); o[2] = pack2bf(b[0], b[1]); o[3] = pack2bf(b[2], b[3]);
      } else {
        o = src[(long)r * cpr + c];
      }
    }
    dst[i] = o;
  }
}

// one thread per 16-byte chunk of X [cap][KH*KW][cpp]
__global__ __launch_bounds__(256) void k_rpn_im2col_rows(const u32x4* __restrict__ x, const int* __restrict__ rows, u32x4* __restrict__ out,
                                                         long nch, int H, int W, int cpp, int KH, int KW, int pad) {
  const int taps = KH * KW;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < nch; i += (long)gridDim.x * 256) {
    const long st = i / cpp;
    const int c = (int)(i - st * cpp), s = (int)(st / taps), tap = (int)(st - (long)s * taps);
    const int r = rows[s];
    u32x4 o = {0u, 0u, 0u, 0u};
    if (r >= 0) {
      const int w = r % W, nh = r / W, h = nh % H, n = nh / H;
      const int hh = h + tap / KW - pad, ww = w + tap % KW - pad;
      if (hh >= 0 && hh < H && ww >= 0 && ww < W) o = x[(((long)n * H + hh) * W + ww) * cpp + c];
    }
    out[i] = o;
  }
}

// one thread per 16-byte chunk of dx [positions][Cin]: 8 (bf16) or 4 (f32) channels, summed over the taps in tap order
template <bool BF16>
__global__ __launch_bounds__(256) void k_rpn_dx_gather(const f32x4* __restrict__ P, const int* __restrict__ slot, u32x4* __restrict__ dx,
                                                       long nch, int cap, int H, int W, int cpp, int KH, int KW, int pad) {
  constexpr int Q = BF16 ? 2 : 1;                 // f32x4 quads of P per output chunk
  const long tap_stride = (long)cap * cpp * Q;    // in quads
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < nch; i += (long)gridDim.x * 256) {
    const long p = i / cpp;
    const int c = (int)(i - p * cpp);
    const int w = (int)(p % W);
    const long nh = p / W;
    const int h = (int)(nh % H);
    f32x4 a0 = {0.f, 0.f, 0.f, 0.f}, a1 = {0.f, 0.f, 0.f, 0.f};
    for (int kh = 0; kh < KH; ++kh) {
      const int hh = h + kh - pad;
      if (hh < 0 || hh >= H) continue;
      for (int kw = 0; kw < KW; ++kw) {
        const int ww = w + kw - pad;
        if (ww < 0 || ww >= W) continue;
        const int s = slot[p + (long)(kh - pad) * W + (kw - pad)];
        if (s < 0) continue;
        const f32x4* q = P + (long)(kh * KW + kw) * tap_stride + ((long)s * cpp + c) * Q;
        a0 += q[0];
        if constexpr (BF16) a1 += q[1];
      }
    }
    u32x4 o;
    if constexpr (BF16) { o[0] = pack2bf(a0[0], a0[1]); o[1] = pack2bf(a0[2], a0[3]); o[2] = pack2bf(a1[0], a1[1]); o[3] = pack2bf(a1[2], a1[3]); }
    else o = __builtin_bit_cast(u32x4, a0);
    dx[i] = o;
  }
}

inline bool aligned16(const void* p) { return ((size_t)p & 15) == 0; }

}  // namespace

extern "C" int cddmsl_rpn_mark_rows(const void* dy, int* marks, long rows, int cols, int src_f32, int dtype, void* stream) {
  if ((dtype != 0 && dtype != 1) || rows < 0 || rows > 0x40000000L || cols <= 0 || !dy || !marks || !aligned16(dy)) return CDDMSL_ERR_ARG;
  const int es = (src_f32 || dtype == 1) ? 4 : 2;
  if (((long)cols * es) % 16) return CDDMSL_ERR_ARG;
  if (rows == 0) return CDDMSL_OK;
  const int cpr = cols * es / 16;
  if (cpr > 0x7fffff) return CDDMSL_ERR_ARG;
  hipLaunchKernelGGL(k_rpn_mark_rows, dim3(grid_for(rows)), dim3(256), 0, (hipStream_t)stream, (const u32x4*)dy, marks, rows, cpr,
                     es == 4 ? 0x7fffffffu : 0x7fff7fffu);      // every element's bits without its sign
  return launch_status();
}

extern "C" int cddmsl_rpn_compact_rows(const int* marks, int* rows_out, int* slot, int* overflow, long positions, int cap, void* stream) {
  if (positions <= 0 || positions > 0x40000000L || cap <= 0 || !marks || !rows_out || !slot || !overflow) return CDDMSL_ERR_ARG;
  hipLaunchKernelGGL(k_rpn_compact, dim3(1), dim3(1024), 0, (hipStream_t)stream, marks, rows_out, slot, overflow, (int)positions, cap);
  return launch_status();
}

extern "C" int cddmsl_rpn_gather_rows(const void* src, const int* rows, void* dst, int cap, int cols, int src_f32, int dtype, void* stream) {
  if ((dtype != 0 && dtype != 1) || cap <= 0 || cols <= 0 || !src || !rows || !dst || !aligned16(src) || !aligned16(dst)) return CDDMSL_ERR_ARG;
  const int es = dtype == 0 ? 2 : 4;
  if (((long)cols * es) % 16) return CDDMSL_ERR_ARG;
  const int cpr = cols * es / 16;
  const long nch = (long)cap * cpr;
  if (src_f32 && dtype == 0)
    hipLaunchKernelGGL(k_rpn_gather_rows<true>, dim3(grid_for(nch)), dim3(256), 0, (hipStream_t)stream, (const u32x4*)src, rows, (u32x4*)dst, nch, cpr);
  else
    hipLaunchKernelGGL(k_rpn_gather_rows<false>, dim3(grid_for(nch)), dim3(256), 0, (hipStream_t)stream, (const u32x4*)src, rows, (u32x4*)dst, nch, cpr);
  return launch_status();
}

extern "C" int cddmsl_rpn_im2col_rows(const void* x, const int* rows, void* out, int cap, int Nimg, int H, int W, int Cin, int KH, int KW,
                                      int pad, int dtype, void* stream) {
  if ((dtype != 0 && dtype != 1) || cap <= 0 || Nimg <= 0 || H <= 0 || W <= 0 || Cin <= 0 || KH <= 0 || KW <= 0 || pad < 0) return CDDMSL_ERR_ARG;
  if (2 * pad != KH - 1 || 2 * pad != KW - 1 || (long)Nimg * H * W > 0x40000000L) return CDDMSL_ERR_ARG;       // "same" convolutions, stride 1
  if (!x || !rows || !out || !aligned16(x) || !aligned16(out)) return CDDMSL_ERR_ARG;
  const int es = dtype == 0 ? 2 : 4;
  if (((long)Cin * es) % 16) return CDDMSL_ERR_ARG;
  const int cpp = Cin * es / 16;
  const long nch = (long)cap * KH * KW * cpp;
  hipLaunchKernelGGL(k_rpn_im2col_rows, dim3(grid_for(nch)), dim3(256), 0, (hipStream_t)stream, (const u32x4*)x, rows, (u32x4*)out, nch, H, W,
                     cpp, KH, KW, pad);
  return launch_status();
}

extern "C" int cddmsl_rpn_dx_gather(const float* P, const int* slot, void* dx, int cap, int Nimg, int H, int W, int Cin, int KH, int KW,
                                    int pad, int dtype, void* stream) {
  if ((dtype != 0 && dtype != 1) || cap <= 0 || Nimg <= 0 || H <= 0 || W <= 0 || Cin <= 0 || KH <= 0 || KW <= 0 || pad < 0) return CDDMSL_ERR_ARG;
  if (2 * pad != KH - 1 || 2 * pad != KW - 1 || (long)Nimg * H * W > 0x40000000L) return CDDMSL_ERR_ARG;
  if (!P || !slot || !dx || !aligned16(P) || !aligned16(dx)) return CDDMSL_ERR_ARG;
  const int es = dtype == 0 ? 2 : 4;
  if (((long)Cin * es) % 16) return CDDMSL_ERR_ARG;
  const int cpp = Cin * es / 16;
  const long nch = (long)Nimg * H * W * cpp;
  if (dtype == 0)
    hipLaunchKernelGGL(k_rpn_dx_gather<true>, dim3(grid_for(nch)), dim3(256), 0, (hipStream_t)stream, (const f32x4*)P, slot, (u32x4*)dx, nch, cap,
                       H, W, cpp, KH, KW, pad);
  else
    hipLaunchKernelGGL(k_rpn_dx_gather<false>, dim3(grid_for(nch)), dim3(256), 0, (hipStream_t)stream, (const f32x4*)P, slot, (u32x4*)dx, nch, cap,
                       H, W, cpp, KH, KW, pad);
  return launch_status();
}
