// CLIP text encoder (RegionCLIP's language tower: detectron2/modeling/backbone/clip_backbone.py:273-317,732-877), forward only --
// the reference freezes it (clip_rcnn.py:438-439).  The linears run on the conv/GEMM kernels (gemm_conv.hip and the kernel files it dispatches to) and the two per-layer
// LayerNorms on the mapper's LayerNorm kernel (losses.hip), and the token + positional embedding (encode_text's first two lines) on
// pos_embed (gpt2.hip); this file holds what those do not cover:
//   attn_causal   o = softmax(q k^T dh^-0.5 + mask) v per (sequence, head), keys j <= query i (build_attention_mask), dh = 64
//   quick_gelu    x * sigmoid(1.702 x) in place on the c_fc output (QuickGELU), and gelu_new, GPT-2's tanh GELU, on its prefill's:
//                 one in-place kernel for both
//   text_pool     ln_final of each sequence's EOT row, optionally averaged over groups of consecutive rows (the concept mean)
#include "common.h"

namespace {

// ---------------------------------------------------------------------------------------------------------------------------
// Causal attention for short sequences (CLIP's text transformer: t <= 77 tokens, heads of 64).  bf16 MFMA
// (v_mfma_f32_32x32x16_bf16), f32 softmax.  One WAVE per (sequence, head), four per workgroup (so a workgroup is not one wave when a
// (sequence, head) is a single 32-row tile, as it is at t = 16..32).  A wave walks its query tiles i0 = 0, 32, ..; for each it forms
// S = Q K^T only for the key tiles j0 <= i0 (tiles above the diagonal are skipped, not computed and masked), masks j > i inside the
// diagonal tile, and takes O = P V over keys [0, i0 + 32).  Q and K are contracted along their columns, so their MFMA fragments come
// straight from global memory; V is contracted along its rows and P along its columns, so both go through a per-wave LDS image (V
// read with ds_read_b64_tr_b16).  Row i of the output depends on q_i, k_j, v_j for j <= i only, in an order that does not depend on t.
constexpr int CDH = 64;                 // head dim (4 k-steps of 16)
constexpr int VRS = CDH * 2 + 16;       // V image row stride in bytes (128 data + 16 pad)

__device__ __forceinline__ void mma(f32x16& acc, const u32x4& a, const u32x4& b) {
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), acc, 0, 0, 0);
}
// operand contracted along its columns, from global: lane (r, hh) <- row row0 + r, elements 16 kk + 8 hh ..+8; rows >= t read as zero
__device__ __forceinline__ u32x4 gfrag(const char* g, int ld, int t, int row0, int kk, int lane) {
  const int row = row0 + (lane & 31);
  u32x4 v = {0u, 0u, 0u, 0u};
  if (row < t) v = *(const u32x4*)(g + ((long)row * ld + kk * 16 + (lane >> 5) * 8) * 2);
  return v;
}
// the same from an LDS image with row stride rs bytes
__device__ __forceinline__ u32x4 lfrag_cols(const char* img, int rs, int kk, int lane) {
  return *(const u32x4*)(img + (lane & 31) * rs + (kk * 16 + (lane >> 5) * 8) * 2);
}
// operand contracted along its rows (transposing read): lane (c, hh) <- column col0 + c, rows 16 kk + 8 hh ..+8
__device__ __forceinline__ u32x4 lfrag_rows(const char* img, int rs, int col0, int kk, int lane) {
  const int g = lane >> 4, li = lane & 15, q = li >> 2, pp = li & 3, hh = g >> 1;
  const int col = col0 + 16 * (g & 1) + 4 * pp;
  const char* a0 = img + (kk * 16 + 8 * hh + q) * rs + col * 2;
  const i16x4 v0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) i16x4*)a0);
  const i16x4 v1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) i16x4*)(a0 + 4 * rs));
  const u32x2 p0 = __builtin_bit_cast(u32x2, v0), p1 = __builtin_bit_cast(u32x2, v1);
  return u32x4{p0[0], p0[1], p1[0], p1[1]};
}
// max / sum over the 32 lanes that share lane >> 5 (one row of a C tile)
__device__ __forceinline__ float row_max(float v) {
#pragma unroll
  for (int o = 16; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ float row_sum(float v) {
#pragma unroll
  for (int o = 16; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

template <int NT>   // t <= 32 NT
__global__ __launch_bounds__(256) void k_attn_causal_fwd(const char* __restrict__ qkv, char* __restrict__ o, int nseq, int t, int heads,
                                                         int ldqkv, int ldo, float scale) {
  constexpr int PRS = NT * 64 + 16;                 // P image: 32 query rows x 32 NT keys, bf16, + 16 pad
  constexpr int VIMG = 32 * NT * VRS, PIMG = 32 * PRS;
  __shared__ __attribute__((aligned(16))) char lds[4 * (VIMG + PIMG)];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const long items = (long)nseq * heads, item0 = (long)blockIdx.x * 4 + w;
  const bool live = item0 < items;
  const long item = live ? item0 : items - 1;       // a spare wave recomputes the last item and stores nothing (no early exit:
                                                    // the transposed reads and the barriers need every lane of every wave)
  const int s = (int)(item / heads), h = (int)(item - (long)s * heads);
  const int W = heads * CDH;
  char* Vi = lds + w * (VIMG + PIMG);
  char* Pi = Vi + VIMG;
  const long r0 = (long)s * t;
  const char* qg = qkv + (r0 * ldqkv + h * CDH) * 2;
  const char* kg = qg + (long)W * 2;
  const char* vg = qg + (long)W * 4;
  char* og = o + (r0 * ldo + h * CDH) * 2;
#pragma unroll
  for (int it = 0; it < NT * 4; ++it) {             // V rows [0, 32 NT) -> image, 8 chunks of 16 B per row; rows >= t zeroed
    const int c = it * 64 + lane, row = c >> 3, ch = c & 7;
    u32x4 v = {0u, 0u, 0u, 0u};
    if (row < t) v = *(const u32x4*)(vg + (long)row * ldqkv * 2 + ch * 16);
    *(u32x4*)(Vi + row * VRS + ch * 16) = v;
  }
  __syncthreads();
  const int c = lane & 31, hh = lane >> 5;
#pragma unroll
  for (int it = 0; it < NT; ++it) {
    const int i0 = 32 * it;
    if (i0 >= t) break;                               // (uniform: every wave of the grid has the same t)
    u32x4 qf[4];
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) qf[kk] = gfrag(qg, ldqkv, t, i0, kk, lane);
    f32x16 S[NT];
#pragma unroll
    for (int jt = 0; jt <= it; ++jt) {
#pragma unroll
      for (int r = 0; r < 16; ++r) S[jt][r] = 0.f;
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) mma(S[jt], qf[kk], gfrag(kg, ldqkv, t, 32 * jt, kk, lane));
    }
#pragma unroll
    for (int g = 0; g < 16; ++g) {
      const int i = i0 + (g & 3) + 8 * (g >> 2) + 4 * hh;   // query row of register g; key of this lane in tile jt: 32 jt + c
      float m = -INFINITY;
#pragma unroll
      for (int jt = 0; jt <= it; ++jt) {
        const float v = (32 * jt + c <= i) ? S[jt][g] * scale : -INFINITY;
        S[jt][g] = v;
        m = fmaxf(m, v);
      }
      m = row_max(m);                                 // finite: key j = i is always present
      float sum = 0.f;
#pragma unroll
      for (int jt = 0; jt <= it; ++jt) { const float e = __expf(S[jt][g] - m); S[jt][g] = e; sum += e; }
      const float inv = 1.f / row_sum(sum);
#pragma unroll
      for (int jt = 0; jt <= it; ++jt) S[jt][g] *= inv;
    }
#pragma unroll
    for (int jt = 0; jt <= it; ++jt)
#pragma unroll
      for (int g = 0; g < 16; ++g)
        *(unsigned short*)(Pi + ((g & 3) + 8 * (g >> 2) + 4 * hh) * PRS + (32 * jt + c) * 2) = f2bf(S[jt][g]);
    __syncthreads();
    f32x16 acc[2];
#pragma unroll
    for (int ct = 0; ct < 2; ++ct)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[ct][r] = 0.f;
#pragma unroll
    for (int kk = 0; kk < 2 * (it + 1); ++kk) {
      const u32x4 pa = lfrag_cols(Pi, PRS, kk, lane);
#pragma unroll
      for (int ct = 0; ct < 2; ++ct) mma(acc[ct], pa, lfrag_rows(Vi, VRS, ct * 32, kk, lane));
    }
    if (live) {
#pragma unroll
      for (int ct = 0; ct < 2; ++ct)
#pragma unroll
        for (int g = 0; g < 16; ++g) {
          const int r = i0 + (g & 3) + 8 * (g >> 2) + 4 * hh;
          if (r < t) *(unsigned short*)(og + ((long)r * ldo + ct * 32 + c) * 2) = f2bf(acc[ct][g]);
        }
    }
    __syncthreads();                                  // the next query tile rewrites the P image
  }
}

// ---------------------------------------------------------------------------------------------------------------------------
// In-place activation F (qgelu / gelu_new, common.h) on T = __bf16 or float, 16 bytes per thread
template <float (*F)(float), typename T>
__global__ __launch_bounds__(256) void k_act_inplace(void* x, long n16) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n16) return;
  if constexpr (sizeof(T) == 2) {
    u32x4 u = ((u32x4*)x)[i];
#pragma unroll
    for (int e = 0; e < 4; ++e) u[e] = pack2bf(F(bf2f(u[e] & 0xffff)), F(bf2f(u[e] >> 16)));
    ((u32x4*)x)[i] = u;
  } else {
    float4 v = ((float4*)x)[i];
    v.x = F(v.x); v.y = F(v.y); v.z = F(v.z); v.w = F(v.w);
    ((float4*)x)[i] = v;
  }
}

// ---------------------------------------------------------------------------------------------------------------------------
// ln_final on gathered rows: output row r = (1/group) sum_p LN(x[rows[r*group + p]]).  One wave per output row, the row in
// registers (W <= 1024, W % 64 == 0); LayerNorm is per row, so normalising only the gathered EOT rows is exact.
constexpr int POOL_MAXK = 16;

__global__ __launch_bounds__(256) void k_text_pool(const float* __restrict__ x, const long* __restrict__ rows, const float* __restrict__ gamma,
                                                   const float* __restrict__ beta, void* __restrict__ y, long R, int nout, int group, int W,
                                                   float eps, int dtype) {
  const int lane = threadIdx.x & 63;
  const long r = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= nout) return;
  const int nk = W / 64;
  float acc[POOL_MAXK];
#pragma unroll
  for (int k = 0; k < POOL_MAXK; ++k) acc[k] = 0.f;
  for (int p = 0; p < group; ++p) {
    long src = rows[r * group + p];
    src = (src < 0 || src >= R) ? 0 : src;          // (memory safety only: the host builds rows in range)
    const float* xr = x + src * W;
    float v[POOL_MAXK], s = 0.f;
#pragma unroll
    for (int k = 0; k < POOL_MAXK; ++k) {
      v[k] = k < nk ? xr[k * 64 + lane] : 0.f;
      s += v[k];
    }
    const float mean = wave_sum(s) / W;
    float q = 0.f;
#pragma unroll
    for (int k = 0; k < POOL_MAXK; ++k)
      if (k < nk) { const float d = v[k] - mean; q += d * d; }
    const float rstd = rsqrtf(wave_sum(q) / W + eps);
#pragma unroll
    for (int k = 0; k < POOL_MAXK; ++k)
      if (k < nk) acc[k] += (v[k] - mean) * rstd * gamma[k * 64 + lane] + beta[k * 64 + lane];
  }
  const float inv = 1.f / group;
#pragma unroll
  for (int k = 0; k < POOL_MAXK; ++k)
    if (k < nk) {
      const long i = r * W + k * 64 + lane;
      if (dtype == 0) ((unsigned short*)y)[i] = f2bf(acc[k] * inv);
      else ((float*)y)[i] = acc[k] * inv;
    }
}

inline bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

template <float (*F)(float)>
int act_inplace(void* x, long numel, int dtype, void* stream) {
  if (numel < 0 || (dtype != 0 && dtype != 1) || !al16(x) || (numel % (dtype == 0 ? 8 : 4))) return CDDMSL_ERR_ARG;
  if (numel == 0) return CDDMSL_OK;
  const long n16 = numel / (dtype == 0 ? 8 : 4);
  const dim3 grid((unsigned)((n16 + 255) / 256));
  if (dtype == 0) hipLaunchKernelGGL((k_act_inplace<F, __bf16>), grid, dim3(256), 0, (hipStream_t)stream, x, n16);
  else hipLaunchKernelGGL((k_act_inplace<F, float>), grid, dim3(256), 0, (hipStream_t)stream, x, n16);
  return launch_status();
}

}  // namespace

extern "C" int cddmsl_attn_causal_fwd(const void* qkv, void* o, int nseq, int t, int heads, int dh, int ldqkv, int ldo, float scale, int dtype,
                                      void* stream) {
  if (dtype != 0 || dh != CDH || nseq < 0 || t <= 0 || t > 128 || heads <= 0) return CDDMSL_ERR_ARG;
  if ((ldqkv & 7) || (ldo & 7) || ldqkv < 3 * heads * dh || ldo < heads * dh || !al16(qkv) || !al16(o)) return CDDMSL_ERR_ARG;
  if (nseq == 0) return CDDMSL_OK;
  const long wgs = ((long)nseq * heads + 3) / 4;
  if (wgs > 0x7fffffffL) return CDDMSL_ERR_ARG;
  const dim3 grid((unsigned)wgs), blk(256);
  const hipStream_t st = (hipStream_t)stream;
  const char* q = (const char*)qkv;
  char* out = (char*)o;
  switch ((t + 31) / 32) {
    case 1: hipLaunchKernelGGL(k_attn_causal_fwd<1>, grid, blk, 0, st, q, out, nseq, t, heads, ldqkv, ldo, scale); break;
    case 2: hipLaunchKernelGGL(k_attn_causal_fwd<2>, grid, blk, 0, st, q, out, nseq, t, heads, ldqkv, ldo, scale); break;
    case 3: hipLaunchKernelGGL(k_attn_causal_fwd<3>, grid, blk, 0, st, q, out, nseq, t, heads, ldqkv, ldo, scale); break;
    default: hipLaunchKernelGGL(k_attn_causal_fwd<4>, grid, blk, 0, st, q, out, nseq, t, heads, ldqkv, ldo, scale); break;
  }
  return launch_status();
}

extern "C" int cddmsl_quick_gelu(void* x, long numel, int dtype, void* stream) { return act_inplace<qgelu>(x, numel, dtype, stream); }
extern "C" int cddmsl_gelu_new(void* x, long numel, int dtype, void* stream) { return act_inplace<gelu_new>(x, numel, dtype, stream); }

extern "C" int cddmsl_text_pool(const float* x, const long* rows, const float* gamma, const float* beta, void* y, long R, int nout, int group,
                                int W, float eps, int dtype, void* stream) {
  if (R <= 0 || nout < 0 || group <= 0 || W <= 0 || (W & 63) || W > 64 * POOL_MAXK || (dtype != 0 && dtype != 1)) return CDDMSL_ERR_ARG;
  if (nout == 0) return CDDMSL_OK;
  hipLaunchKernelGGL(k_text_pool, dim3((unsigned)((nout + 3) / 4)), dim3(256), 0, (hipStream_t)stream, x, rows, gamma, beta, y, R, nout,
                     group, W, eps, dtype);
  return launch_status();
}
