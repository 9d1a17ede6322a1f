// Training the ClipCap mapper against a frozen GPT-2 (the reference's clipcap.py: ClipCaptionModel.forward + train, --only_prefix): the
// kernels the forward-only stack (text_encoder.hip, gpt2.hip, losses.hip) does not have.
//   attn_causal_bwd        backward of attn_causal_fwd (text_encoder.hip): dq | dk | dv from q | k | v and dO, probabilities recomputed
//   gelu_new_bwd           dx = dy * d/dx gelu_new(x) on the c_fc output kept from before the in-place activation
//   token_ce_fwd / _bwd    F.cross_entropy(logits [R][V] f32, target, ignore_index) over a vocabulary-sized row
//   layernorm_bwd_params   dgamma / dbeta, the affine gradients cddmsl_layernorm_bwd leaves out
//   adamw_step             torch.optim.AdamW over a list of f32 tensors
// No floating-point atomics anywhere in this file: every reduction has a fixed order (a workspace and a second pass where it spans
// workgroups), so one call gives the same bits twice.
#include "common.h"
#include <math.h>

namespace {

inline bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// ---------------------------------------------------------------------------------------------------------------------------
// Causal attention backward, t <= 128 tokens, heads of 64.  One workgroup = one (sequence, head), four waves; wave w owns query rows
// [32w, 32w + 32) for S / P / dP / dS / dQ and key rows [32w, 32w + 32) for dV / dK.  Only the tiles on or below the diagonal exist:
//     S  = Q K^T, dP = dO V^T     key tiles jt <= w            (Q, K, dO contracted along their columns; V straight from global)
//     dS = P o (dP - rowsum(dP o P)) * scale                   (masked entries: P = 0, so dS = 0)
//     dV[j] = sum_{i >= j} P[i][j] dO[i],  dK[j] = sum_{i >= j} dS[i][j] Q[i]      query tiles it >= w (contracted along rows: transposing reads)
//     dQ[i] = sum_{j <= i} dS[i][j] K[j]                       key tiles jt <= w
// Q, K, dO live as [128][64] bf16 images in LDS (row stride 144 B), P and then dS as a [128][128] image (row stride 272 B): 88 KiB.
// Rows >= t of every image are zero: a padding query row has dO = 0, hence dP = 0 and dS = 0, and adds nothing to dV / dK.
constexpr int BDH = 64;                  // head dim (4 k-steps of 16)
constexpr int BT = 128;                  // most tokens
constexpr int ORS = BDH * 2 + 16;        // operand image row stride in bytes
constexpr int XRS = BT * 2 + 16;         // P / dS image row stride in bytes
constexpr int OIMG = BT * ORS, XIMG = BT * XRS;

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
// the same from an LDS image (img points at the tile's first row)
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
// global [t][64] bf16 (row stride ld elements) -> image, rows t..127 zeroed: 128 rows x 8 chunks of 16 B = 4 per thread of the 256
__device__ __forceinline__ void stage(char* img, const char* g, int t, int ld, int tid) {
#pragma unroll
  for (int it = 0; it < 4; ++it) {
    const int c = it * 256 + tid, row = c >> 3, ch = c & 7;
    u32x4 v = {0u, 0u, 0u, 0u};
    if (row < t) v = *(const u32x4*)(g + (long)row * ld * 2 + ch * 16);
    *(u32x4*)(img + row * ORS + ch * 16) = v;
  }
}
// C tile (rows row0.., cols col0..) -> the P / dS image as bf16
__device__ __forceinline__ void put_x(char* Xi, int row0, int col0, const f32x16& a, int lane) {
  const int c = col0 + (lane & 31), hh = lane >> 5;
#pragma unroll
  for (int g = 0; g < 16; ++g) *(unsigned short*)(Xi + (row0 + (g & 3) + 8 * (g >> 2) + 4 * hh) * XRS + c * 2) = f2bf(a[g]);
}
// C tile -> global bf16, rows < t only
__device__ __forceinline__ void store_tile(char* gp, int ld, int t, int row0, int col0, const f32x16& a, int lane) {
  const int c = col0 + (lane & 31), hh = lane >> 5;
#pragma unroll
  for (int g = 0; g < 16; ++g) {
    const int r = row0 + (g & 3) + 8 * (g >> 2) + 4 * hh;
    if (r < t) *(unsigned short*)(gp + ((long)r * ld + c) * 2) = f2bf(a[g]);
  }
}

__global__ __launch_bounds__(256) void k_attn_causal_bwd(const char* __restrict__ qkv, const char* __restrict__ dout, char* __restrict__ dqkv,
                                                         int t, int heads, int ldqkv, int ldo, float scale) {
  __shared__ __attribute__((aligned(16))) char lds[3 * OIMG + XIMG];
  char *Qi = lds, *Ki = lds + OIMG, *Di = lds + 2 * OIMG, *Xi = lds + 3 * OIMG;
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int s = blockIdx.x / heads, h = blockIdx.x - s * heads;
  const int W = heads * BDH;
  const long r0 = (long)s * t;
  const char* qg = qkv + (r0 * ldqkv + h * BDH) * 2;
  const char* kg = qg + (long)W * 2;
  const char* vg = qg + (long)W * 4;
  const char* dg = dout + (r0 * ldo + h * BDH) * 2;
  char* dqg = dqkv + (r0 * ldqkv + h * BDH) * 2;
  char* dkg = dqg + (long)W * 2;
  char* dvg = dqg + (long)W * 4;
  stage(Qi, qg, t, ldqkv, tid);
  stage(Ki, kg, t, ldqkv, tid);
  stage(Di, dg, t, ldo, tid);
  __syncthreads();
  const int nt = (t + 31) >> 5, i0 = 32 * w;
  const bool active = w < nt;                       // (wave-uniform: a wave whose rows are all padding only keeps the barriers)
  const int c = lane & 31, hh = lane >> 5;
  f32x16 P[4], dP[4];
  if (active) {
    u32x4 qf[4], df[4];
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      qf[kk] = lfrag_cols(Qi + i0 * ORS, ORS, kk, lane);
      df[kk] = lfrag_cols(Di + i0 * ORS, ORS, kk, lane);
    }
#pragma unroll
    for (int jt = 0; jt < 4; ++jt) {
#pragma unroll
      for (int r = 0; r < 16; ++r) { P[jt][r] = 0.f; dP[jt][r] = 0.f; }
      if (jt <= w) {
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
          mma(P[jt], qf[kk], lfrag_cols(Ki + 32 * jt * ORS, ORS, kk, lane));
          mma(dP[jt], df[kk], gfrag(vg, ldqkv, t, 32 * jt, kk, lane));
        }
      }
    }
#pragma unroll
    for (int g = 0; g < 16; ++g) {
      const int i = i0 + (g & 3) + 8 * (g >> 2) + 4 * hh;     // query row of register g; key of this lane in tile jt: 32 jt + c
      float m = -INFINITY;
#pragma unroll
      for (int jt = 0; jt < 4; ++jt) {
        const float v = (jt <= w && 32 * jt + c <= i) ? P[jt][g] * scale : -INFINITY;
        P[jt][g] = v;
        m = fmaxf(m, v);
      }
      m = row_max(m);                                         // finite: key j = i is always present
      float sum = 0.f;
#pragma unroll
      for (int jt = 0; jt < 4; ++jt) { const float e = __expf(P[jt][g] - m); P[jt][g] = e; sum += e; }
      const float inv = 1.f / row_sum(sum);
      float rs = 0.f;
#pragma unroll
      for (int jt = 0; jt < 4; ++jt) { P[jt][g] *= inv; rs += dP[jt][g] * P[jt][g]; }
      rs = row_sum(rs);
#pragma unroll
      for (int jt = 0; jt < 4; ++jt) dP[jt][g] = P[jt][g] * (dP[jt][g] - rs) * scale;   // dS
    }
#pragma unroll
    for (int jt = 0; jt < 4; ++jt)
      if (jt <= w) put_x(Xi, i0, 32 * jt, P[jt], lane);
  }
  __syncthreads();                                  // dV needs the rows of P of every wave at or below this one
  if (active) {
    f32x16 av[2];
#pragma unroll
    for (int ct = 0; ct < 2; ++ct)
#pragma unroll
      for (int r = 0; r < 16; ++r) av[ct][r] = 0.f;
#pragma unroll
    for (int kk = 0; kk < 8; ++kk) {
      if (kk >= 2 * w && kk < 2 * nt) {
        const u32x4 pa = lfrag_rows(Xi, XRS, i0, kk, lane);
#pragma unroll
        for (int ct = 0; ct < 2; ++ct) mma(av[ct], pa, lfrag_rows(Di, ORS, ct * 32, kk, lane));     // dV[j] = sum_i P[i][j] dO[i]
      }
    }
#pragma unroll
    for (int ct = 0; ct < 2; ++ct) store_tile(dvg, ldqkv, t, i0, ct * 32, av[ct], lane);
  }
  __syncthreads();                                  // every wave is done reading P: the image now takes dS
  if (active) {
#pragma unroll
    for (int jt = 0; jt < 4; ++jt)
      if (jt <= w) put_x(Xi, i0, 32 * jt, dP[jt], lane);
  }
  __syncthreads();
  if (active) {
    f32x16 aq[2], ak[2];
#pragma unroll
    for (int ct = 0; ct < 2; ++ct)
#pragma unroll
      for (int r = 0; r < 16; ++r) { aq[ct][r] = 0.f; ak[ct][r] = 0.f; }
#pragma unroll
    for (int kk = 0; kk < 8; ++kk) {
      if (kk < 2 * (w + 1)) {
        const u32x4 sc = lfrag_cols(Xi + i0 * XRS, XRS, kk, lane);
#pragma unroll
        for (int ct = 0; ct < 2; ++ct) mma(aq[ct], sc, lfrag_rows(Ki, ORS, ct * 32, kk, lane));     // dQ[i] = sum_j dS[i][j] K[j]
      }
      if (kk >= 2 * w && kk < 2 * nt) {
        const u32x4 sr = lfrag_rows(Xi, XRS, i0, kk, lane);
#pragma unroll
        for (int ct = 0; ct < 2; ++ct) mma(ak[ct], sr, lfrag_rows(Qi, ORS, ct * 32, kk, lane));     // dK[j] = sum_i dS[i][j] Q[i]
      }
    }
#pragma unroll
    for (int ct = 0; ct < 2; ++ct) {
      store_tile(dqg, ldqkv, t, i0, ct * 32, aq[ct], lane);
      store_tile(dkg, ldqkv, t, i0, ct * 32, ak[ct], lane);
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------------
// d/dx of gelu_new(x) = 0.5 x (1 + tanh(u)), u = k (x + a x^3):  0.5 (1 + tanh u) + 0.5 x (1 - tanh^2 u) k (1 + 3 a x^2)
__device__ __forceinline__ float gelu_new_grad(float x) {
  const float k = 0.7978845608028654f, a = 0.044715f;
  const float th = tanhf(k * (x + a * x * x * x));
  return 0.5f * (1.f + th) + 0.5f * x * (1.f - th * th) * k * (1.f + 3.f * a * x * x);
}
template <typename T>
__global__ __launch_bounds__(256) void k_gelu_new_bwd(const void* __restrict__ x, const void* __restrict__ dy, void* __restrict__ dx, long numel) {
  constexpr int VW = sizeof(T) == 2 ? 8 : 4;
  const long i = (long)blockIdx.x * 256 + threadIdx.x, nv = numel / VW;
  if (i < nv) {
    if constexpr (sizeof(T) == 2) {
      const u32x4 a = ((const u32x4*)x)[i], g = ((const u32x4*)dy)[i];
      u32x4 o;
#pragma unroll
      for (int e = 0; e < 4; ++e)
        o[e] = pack2bf(bf2f(g[e] & 0xffff) * gelu_new_grad(bf2f(a[e] & 0xffff)), bf2f(g[e] >> 16) * gelu_new_grad(bf2f(a[e] >> 16)));
      ((u32x4*)dx)[i] = o;
    } else {
      const float4 a = ((const float4*)x)[i], g = ((const float4*)dy)[i];
      ((float4*)dx)[i] = make_float4(g.x * gelu_new_grad(a.x), g.y * gelu_new_grad(a.y), g.z * gelu_new_grad(a.z), g.w * gelu_new_grad(a.w));
    }
  } else {
    const long e = nv * VW + (i - nv);              // the tail that fills no whole 16 bytes: one element per thread
    if (e < numel) {
      if constexpr (sizeof(T) == 2)
        ((unsigned short*)dx)[e] = f2bf(bf2f(((const unsigned short*)dy)[e]) * gelu_new_grad(bf2f(((const unsigned short*)x)[e])));
      else
        ((float*)dx)[e] = ((const float*)dy)[e] * gelu_new_grad(((const float*)x)[e]);
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------------
// Token cross-entropy.  One workgroup per row: every thread keeps a running (max, sum exp) over its columns, the 256 pairs are
// combined in a fixed tree.  Columns >= V are never read as classes (a whole float4 is read only where all four columns are < V).
__device__ __forceinline__ void lse_add(float& m, float& s, float v) {
  if (v > m) { s = s * __expf(m - v) + 1.f; m = v; }
  else if (v != -INFINITY) s += __expf(v - m);           // (a -inf logit adds nothing, also while the maximum is still -inf)
}
__device__ __forceinline__ void lse_merge(float& m, float& s, float m2, float s2) {
  const float mm = fmaxf(m, m2);
  if (mm == -INFINITY) { m = mm; s = 0.f; return; }          // both empty
  s = s * __expf(m - mm) + s2 * __expf(m2 - mm);
  m = mm;
}
__global__ __launch_bounds__(256) void k_token_ce_fwd(const float* __restrict__ logits, int ld, const long* __restrict__ target, int V,
                                                      long ignore_index, float* __restrict__ lse, float* __restrict__ row_loss) {
  const long r = blockIdx.x;
  const int tid = threadIdx.x;
  const long tg = target[r];
  if (tg == ignore_index) {                                    // (uniform per workgroup)
    if (tid == 0) { lse[r] = 0.f; row_loss[r] = 0.f; }
    return;
  }
  const float* row = logits + r * (long)ld;
  float m = -INFINITY, s = 0.f;
  const int v4 = V >> 2;
  for (int i = tid; i < v4; i += 256) {
    const float4 x = ((const float4*)row)[i];
    lse_add(m, s, x.x); lse_add(m, s, x.y); lse_add(m, s, x.z); lse_add(m, s, x.w);
  }
  for (int cidx = (v4 << 2) + tid; cidx < V; cidx += 256) lse_add(m, s, row[cidx]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float m2 = __shfl_xor(m, o, 64), s2 = __shfl_xor(s, o, 64);
    lse_merge(m, s, m2, s2);
  }
  __shared__ float rm[4], rsum[4];
  if ((tid & 63) == 0) { rm[tid >> 6] = m; rsum[tid >> 6] = s; }
  __syncthreads();
  if (tid == 0) {
    float M = rm[0], S = rsum[0];
#pragma unroll
    for (int k = 1; k < 4; ++k) lse_merge(M, S, rm[k], rsum[k]);
    const float l = M + logf(S);
    lse[r] = l;
    // a target outside [0, V) that is not ignore_index has no class: the loss says so instead of reading out of the row
    // (max - target logit first: exact-ish where both sit far from zero, then the small log term)
    row_loss[r] = (tg >= 0 && tg < V) ? (M - row[tg]) + logf(S) : __builtin_nanf("");
  }
}
// sum_count[0] = sum of the row losses, [1] = the number of rows whose target is not ignore_index; one workgroup, fixed order
__global__ __launch_bounds__(256) void k_token_ce_sum(const float* __restrict__ row_loss, const long* __restrict__ target, long R,
                                                      long ignore_index, float* __restrict__ sum_count) {
  const int tid = threadIdx.x;
  float s = 0.f, n = 0.f;
  for (long r = tid; r < R; r += 256)
    if (target[r] != ignore_index) { s += row_loss[r]; n += 1.f; }
  __shared__ float ss[256], sn[256];
  ss[tid] = s; sn[tid] = n;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) { ss[tid] += ss[tid + o]; sn[tid] += sn[tid + o]; }
    __syncthreads();
  }
  if (tid == 0) { sum_count[0] = ss[0]; sum_count[1] = sn[0]; }
}
// dlogits[r][c] = (softmax(logits[r])[c] - [c == target[r]]) * gscale for c < V on a row that counts, else 0; four columns per thread
// (ld % 8 == 0).  With f32 output a thread writes exactly the 16 bytes it read, so dlogits may be logits.
template <typename T>
__global__ __launch_bounds__(256) void k_token_ce_bwd(const float* logits, int ld, const long* __restrict__ target, const float* __restrict__ lse,
                                                      float gscale, void* dlogits, int V, long ignore_index) {
  const long r = blockIdx.x;
  const int c4 = blockIdx.y * 256 + threadIdx.x;
  if (c4 * 4 >= ld) return;
  const long tg = target[r];
  const bool on = tg != ignore_index;
  const float l = lse[r];
  const float4 x = ((const float4*)(logits + r * (long)ld))[c4];
  const float xs[4] = {x.x, x.y, x.z, x.w};
  float o[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int cidx = c4 * 4 + e;
    o[e] = (on && cidx < V) ? (__expf(xs[e] - l) - (cidx == tg ? 1.f : 0.f)) * gscale : 0.f;
  }
  if constexpr (sizeof(T) == 2) ((u32x2*)((char*)dlogits + r * (long)ld * 2))[c4] = u32x2{pack2bf(o[0], o[1]), pack2bf(o[2], o[3])};
  else ((float4*)((float*)dlogits + r * (long)ld))[c4] = make_float4(o[0], o[1], o[2], o[3]);
}

// ---------------------------------------------------------------------------------------------------------------------------
// LayerNorm affine gradients: dgamma[d] = sum_r dy[r][d] (x[r][d] - mean[r]) rstd[r], dbeta[d] = sum_r dy[r][d].  Pass 1: a workgroup
// owns 64 columns x one chunk of rows (4 row lanes, combined in order) and writes its partial pair into the workspace; pass 2: one
// thread per column adds the chunks in order.
template <typename T>
__global__ __launch_bounds__(256) void k_ln_params_part(const void* __restrict__ dy, const float* __restrict__ x, const float* __restrict__ mean,
                                                        const float* __restrict__ rstd, float* __restrict__ part, long R, int D, long chunk_rows) {
  const int cl = threadIdx.x & 63, rl = threadIdx.x >> 6;
  const int col = blockIdx.x * 64 + cl;
  const long rb = (long)blockIdx.y * chunk_rows, re = rb + chunk_rows < R ? rb + chunk_rows : R;
  float sg = 0.f, sb = 0.f;
  if (col < D)
    for (long r = rb + rl; r < re; r += 4) {
      const long i = r * D + col;
      float g;
      if constexpr (sizeof(T) == 2) g = bf2f(((const unsigned short*)dy)[i]);
      else g = ((const float*)dy)[i];
      sg += g * ((x[i] - mean[r]) * rstd[r]);
      sb += g;
    }
  __shared__ float lg[4][64], lb[4][64];
  lg[rl][cl] = sg; lb[rl][cl] = sb;
  __syncthreads();
  if (rl == 0 && col < D) {
    part[((long)blockIdx.y * 2) * D + col] = ((lg[0][cl] + lg[1][cl]) + lg[2][cl]) + lg[3][cl];
    part[((long)blockIdx.y * 2 + 1) * D + col] = ((lb[0][cl] + lb[1][cl]) + lb[2][cl]) + lb[3][cl];
  }
}
__global__ __launch_bounds__(256) void k_ln_params_final(const float* __restrict__ part, float* __restrict__ dgamma, float* __restrict__ dbeta,
                                                         int D, int chunks, int accumulate) {
  const int col = blockIdx.x * 256 + threadIdx.x;
  if (col >= D) return;
  float sg = 0.f, sb = 0.f;
  for (int k = 0; k < chunks; ++k) { sg += part[((long)k * 2) * D + col]; sb += part[((long)k * 2 + 1) * D + col]; }
  dgamma[col] = accumulate ? dgamma[col] + sg : sg;
  dbeta[col] = accumulate ? dbeta[col] + sb : sb;
}
inline long ln_chunk_rows(long R) {                  // 64 rows per chunk, more once that would make over 256 chunks
  long cr = 64;
  if (R > 64 * 256) cr = (((R + 255) / 256) + 3) & ~3L;
  return cr;
}

// ---------------------------------------------------------------------------------------------------------------------------
// torch.optim.AdamW (amsgrad off, maximize off) on one element, in torch's order: decoupled decay, exp_avg.lerp_(g, 1 - beta1),
// exp_avg_sq = beta2 v + (1 - beta2) g g, denom = sqrt(v) / sqrt(1 - beta2^step) + eps, p -= lr / (1 - beta1^step) * m / denom.
// A NaN gradient element reaches m, v and p of that element through the arithmetic alone; nothing crosses tensors.
struct AdamItem { float* p; const float* g; float* m; float* v; long n; };
constexpr int ADAM_MAX = 80;
struct AdamBatch { AdamItem it[ADAM_MAX]; int count; };
static_assert(sizeof(AdamBatch) + 7 * 4 + 256 <= 4096, "AdamBatch + scalars + hidden arguments exceed the kernel-argument limit");

__device__ __forceinline__ void adamw_one(float& p, float g, float& m, float& v, float decay, float omb1, float beta2, float omb2,
                                          float bc2s, float eps, float step_size) {
  p = p * decay;
  m = m + (g - m) * omb1;
  v = v * beta2 + omb2 * g * g;
  const float denom = sqrtf(v) / bc2s + eps;
  p = p - step_size * (m / denom);
}
__global__ __launch_bounds__(256) void k_adamw(AdamBatch b, float decay, float omb1, float beta2, float omb2, float bc2s, float eps, float step_size) {
  const AdamItem& t = b.it[blockIdx.y];
  const long tid = (long)blockIdx.x * blockDim.x + threadIdx.x, nth = (long)gridDim.x * blockDim.x;
  long done = 0;
  if (((((size_t)t.g) | ((size_t)t.p) | ((size_t)t.m) | ((size_t)t.v)) & 15) == 0) {
    const long n4 = t.n >> 2;
    for (long i = tid; i < n4; i += nth) {
      float4 p = ((float4*)t.p)[i], m = ((float4*)t.m)[i], v = ((float4*)t.v)[i];
      const float4 g = ((const float4*)t.g)[i];
      adamw_one(p.x, g.x, m.x, v.x, decay, omb1, beta2, omb2, bc2s, eps, step_size);
      adamw_one(p.y, g.y, m.y, v.y, decay, omb1, beta2, omb2, bc2s, eps, step_size);
      adamw_one(p.z, g.z, m.z, v.z, decay, omb1, beta2, omb2, bc2s, eps, step_size);
      adamw_one(p.w, g.w, m.w, v.w, decay, omb1, beta2, omb2, bc2s, eps, step_size);
      ((float4*)t.m)[i] = m;
      ((float4*)t.v)[i] = v;
      ((float4*)t.p)[i] = p;
    }
    done = n4 << 2;
  }
  for (long i = done + tid; i < t.n; i += nth) {
    float p = t.p[i], m = t.m[i], v = t.v[i];
    adamw_one(p, t.g[i], m, v, decay, omb1, beta2, omb2, bc2s, eps, step_size);
    t.m[i] = m;
    t.v[i] = v;
    t.p[i] = p;
  }
}

}  // namespace

extern "C" int cddmsl_attn_causal_bwd(const void* qkv, const void* dout, void* dqkv, int nseq, int t, int heads, int dh, int ldqkv, int ldo,
                                      float scale, int dtype, void* stream) {
  if (dtype != 0 || dh != BDH || nseq < 0 || t <= 0 || t > BT || heads <= 0) return CDDMSL_ERR_ARG;
  if ((ldqkv & 7) || (ldo & 7) || ldqkv < 3 * heads * dh || ldo < heads * dh || !al16(qkv) || !al16(dout) || !al16(dqkv)) return CDDMSL_ERR_ARG;
  if (nseq == 0) return CDDMSL_OK;
  if ((long)nseq * heads > 0x7fffffffL) return CDDMSL_ERR_ARG;
  hipLaunchKernelGGL(k_attn_causal_bwd, dim3((unsigned)(nseq * heads)), dim3(256), 0, (hipStream_t)stream, (const char*)qkv,
                     (const char*)dout, (char*)dqkv, t, heads, ldqkv, ldo, scale);
  return launch_status();
}

extern "C" int cddmsl_gelu_new_bwd(const void* x_pre, const void* dy, void* dx, long numel, int dtype, void* stream) {
  if (numel < 0 || (dtype != 0 && dtype != 1) || !al16(x_pre) || !al16(dy) || !al16(dx)) return CDDMSL_ERR_ARG;
  if (numel == 0) return CDDMSL_OK;
  const int vw = dtype == 0 ? 8 : 4;
  const long threads = numel / vw + numel % vw;
  const long blocks = (threads + 255) / 256;
  if (blocks > 0x7fffffffL) return CDDMSL_ERR_ARG;
  const dim3 grid((unsigned)blocks);
  if (dtype == 0) hipLaunchKernelGGL(k_gelu_new_bwd<__bf16>, grid, dim3(256), 0, (hipStream_t)stream, x_pre, dy, dx, numel);
  else hipLaunchKernelGGL(k_gelu_new_bwd<float>, grid, dim3(256), 0, (hipStream_t)stream, x_pre, dy, dx, numel);
  return launch_status();
}

extern "C" int cddmsl_token_ce_fwd(const float* logits, int ld, const long* target, long R, int V, long ignore_index, float* lse,
                                   float* row_loss, float* sum_count, void* stream) {
  if (R < 0 || R > 0x7fffffffL || V <= 0 || V > ld || (ld & 7) || !al16(logits)) return CDDMSL_ERR_ARG;
  if (R == 0) return CDDMSL_OK;
  const hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_token_ce_fwd, dim3((unsigned)R), dim3(256), 0, st, logits, ld, target, V, ignore_index, lse, row_loss);
  hipLaunchKernelGGL(k_token_ce_sum, dim3(1), dim3(256), 0, st, (const float*)row_loss, target, R, ignore_index, sum_count);
  return launch_status();
}

extern "C" int cddmsl_token_ce_bwd(const float* logits, int ld, const long* target, const float* lse, float gscale, void* dlogits, long R,
                                   int V, long ignore_index, int dtype_out, void* stream) {
  if (R < 0 || R > 0x7fffffffL || V <= 0 || V > ld || (ld & 7) || !al16(logits) || !al16(dlogits)) return CDDMSL_ERR_ARG;
  if (dtype_out != 0 && dtype_out != 1) return CDDMSL_ERR_ARG;
  if (dtype_out == 0 && dlogits == (const void*)logits) return CDDMSL_ERR_ARG;      // only an f32 result may overwrite the logits
  if (R == 0) return CDDMSL_OK;
  const int chunks = (ld / 4 + 255) / 256;
  if (chunks > 65535) return CDDMSL_ERR_ARG;
  const dim3 grid((unsigned)R, (unsigned)chunks);
  if (dtype_out == 0) hipLaunchKernelGGL(k_token_ce_bwd<__bf16>, grid, dim3(256), 0, (hipStream_t)stream, logits, ld, target, lse, gscale, dlogits, V, ignore_index);
  else hipLaunchKernelGGL(k_token_ce_bwd<float>, grid, dim3(256), 0, (hipStream_t)stream, logits, ld, target, lse, gscale, dlogits, V, ignore_index);
  return launch_status();
}

extern "C" int cddmsl_layernorm_bwd_params_workspace(long R, int D) {
  if (R <= 0 || D <= 0) return -1;
  const long cr = ln_chunk_rows(R), chunks = (R + cr - 1) / cr, bytes = chunks * 2 * D * 4;
  return bytes > 0x7fffffffL ? -1 : (int)bytes;
}

extern "C" int cddmsl_layernorm_bwd_params(const void* dy, const float* x, const float* mean, const float* rstd, float* dgamma, float* dbeta,
                                           float* ws, long ws_bytes, long R, int D, int accumulate, int dtype, void* stream) {
  if (R <= 0 || D <= 0 || (dtype != 0 && dtype != 1) || (accumulate != 0 && accumulate != 1)) return CDDMSL_ERR_ARG;
  const int need = cddmsl_layernorm_bwd_params_workspace(R, D);
  if (need < 0 || ws == nullptr || ws_bytes < need) return CDDMSL_ERR_ARG;
  const long cr = ln_chunk_rows(R), chunks = (R + cr - 1) / cr;
  const hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)((D + 63) / 64), (unsigned)chunks);
  if (grid.y > 65535) return CDDMSL_ERR_ARG;
  if (dtype == 0) hipLaunchKernelGGL(k_ln_params_part<__bf16>, grid, dim3(256), 0, st, dy, x, mean, rstd, ws, R, D, cr);
  else hipLaunchKernelGGL(k_ln_params_part<float>, grid, dim3(256), 0, st, dy, x, mean, rstd, ws, R, D, cr);
  hipLaunchKernelGGL(k_ln_params_final, dim3((unsigned)((D + 255) / 256)), dim3(256), 0, st, (const float*)ws, dgamma, dbeta, D, (int)chunks,
                     accumulate);
  return launch_status();
}

extern "C" int cddmsl_adamw_step(float** params, const float** grads, float** exp_avg, float** exp_avg_sq, const long* sizes, int count,
                                 float lr, float beta1, float beta2, float eps, float weight_decay, long step, void* stream) {
  if (count < 0 || step < 1 || !(beta1 >= 0.f && beta1 < 1.f) || !(beta2 >= 0.f && beta2 < 1.f) || !(eps >= 0.f)) return CDDMSL_ERR_ARG;
  for (int i = 0; i < count; ++i)
    if (sizes[i] < 0) return CDDMSL_ERR_ARG;
  // the scalars as torch's single-tensor path forms them: Python doubles, rounded to f32 where they meet the tensors
  const double bc1 = 1.0 - pow((double)beta1, (double)step), bc2 = 1.0 - pow((double)beta2, (double)step);
  const float step_size = (float)((double)lr / bc1), bc2s = (float)sqrt(bc2);
  const float decay = (float)(1.0 - (double)lr * (double)weight_decay), omb1 = (float)(1.0 - (double)beta1), omb2 = (float)(1.0 - (double)beta2);
  const hipStream_t st = (hipStream_t)stream;
  for (int base = 0; base < count; base += ADAM_MAX) {
    AdamBatch b;
    b.count = count - base < ADAM_MAX ? count - base : ADAM_MAX;
    long mx = 0;
    for (int i = 0; i < b.count; ++i) {
      b.it[i].p = params[base + i]; b.it[i].g = grads[base + i]; b.it[i].m = exp_avg[base + i]; b.it[i].v = exp_avg_sq[base + i];
      b.it[i].n = sizes[base + i];
      if (sizes[base + i] > mx) mx = sizes[base + i];
    }
    long gx = (mx + 256 * 8 - 1) / (256 * 8);
    gx = gx < 1 ? 1 : (gx > 256 ? 256 : gx);
    hipLaunchKernelGGL(k_adamw, dim3((unsigned)gx, (unsigned)b.count), dim3(256), 0, st, b, decay, omb1, beta2, omb2, bc2s, eps, step_size);
  }
  return launch_status();
}
