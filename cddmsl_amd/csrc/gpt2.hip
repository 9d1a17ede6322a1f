// GPT-2 decoder for ClipCap captioning (the reference's gen_captions.py / clipcap.py generate2), forward only.  The prefill (40 prefix
// rows per caption) runs on the conv/GEMM kernels, the LayerNorm kernel and attn_causal (text_encoder.hip); a decode step has one row
// per caption, and this file holds what makes that step cheap:
//   skinny_gemm    y[M][N] = x[M][K] @ w[N][K]^T for M <= 64, bf16 operands, f32 accumulation: 32-column tiles x a fixed K split
//                  over workgroups (so N = 768 still covers the chip), f32 partial slabs, then one epilogue launch that sums the
//                  slabs in split order and adds bias / the f32 residual / gelu_new.  The split depends on (N, K) only, and every
//                  output element is a function of its own row of x: a row's result does not depend on M or on the other rows.
//   lm_head_argmax argmax_v (h @ wte^T)[m][v], lowest index on ties (torch.argmax), without writing the logits: a per-32-row-tile
//                  (max, index) per row, then one reduction launch per row.  Optional f32 logits for tests.
//   decode_attn    one query row per (sequence, head) against a KV cache of positions 0..L-2 plus this step's own key / value, which
//                  it appends to the cache at position L-1 (the cache is never copied).
//   lm_head_topk   the row's B best (logit, index) pairs in the arg-max's order and its log-sum-exp, for beam search
//   beam_step      length-normalised beam selection, one wave per caption; permutes the token history and the cache ancestry table
//   decode_attn_beam  decode_attn over a prefix cache shared by a caption's beams and a generated cache read through the ancestry
//                  table: beams change owner every step and no cache row is ever copied
//   pos_embed      x[r] = (tab[ids[r]] or src[r]) + wpe[pos0 + r % t]: the decode step's token + position, the prefill's prefix +
//                  position, and the CLIP text encoder's token + position (text_embed: contiguous ids, pos0 = 0).
// The prefill's in-place gelu_new runs on text_encoder.hip's activation kernel.
#include "common.h"

namespace {

inline bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

__device__ __forceinline__ void mma(f32x16& acc, const u32x4& a, const u32x4& b) {
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), acc, 0, 0, 0);
}

// ---------------------------------------------------------------------------------------------------------------------------
// Skinny GEMM main loop.  A workgroup (4 waves) owns 32 output columns n0.. and the K chunks [c0, c1) of 64 elements; wave w takes
// chunks c0 + w, c0 + w + 4, ..  In a chunk, lane (r = lane & 31, hh = lane >> 5) reads 64 contiguous bytes of row r of the weight
// tile (and of x's row tile): elements 64 c + 32 hh + 8 j .. +8 feed MFMA j (j = 0..3).  A and B use the same element-to-slot map, so
// the four MFMAs sum exactly the 64 products of the chunk.  Rows m >= M and columns n >= N read as zero.  The four waves' sums are
// added in wave order by wave 0 through LDS, so the reduction order is fixed.
constexpr int SK_MAXM = 64;

__device__ __forceinline__ void load64(const char* p, bool ok, u32x4 (&v)[4]) {
#pragma unroll
  for (int j = 0; j < 4; ++j) v[j] = ok ? ((const u32x4*)p)[j] : u32x4{0u, 0u, 0u, 0u};
}

template <int MT>
__device__ __forceinline__ void tile_dot(const char* __restrict__ x, const char* __restrict__ w, int M, int N, int K, int n0, int c0, int c1,
                                         f32x16 (&acc)[MT], float* red) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int r = lane & 31, hh = lane >> 5;
  const bool nok = n0 + r < N;
  const char* wr = w + ((long)(nok ? n0 + r : 0) * K + 32 * hh) * 2;
  const char* xr[MT];
  bool mok[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
    mok[mt] = mt * 32 + r < M;
    xr[mt] = x + ((long)(mok[mt] ? mt * 32 + r : 0) * K + 32 * hh) * 2;
  }
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int g = 0; g < 16; ++g) acc[mt][g] = 0.f;
  int c = c0 + wv;
  for (; c + 4 < c1; c += 8) {                  // two chunks in flight per wave
    u32x4 b0[4], b1[4], a0[MT][4], a1[MT][4];
    load64(wr + (long)c * 128, nok, b0);
    load64(wr + (long)(c + 4) * 128, nok, b1);
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) { load64(xr[mt] + (long)c * 128, mok[mt], a0[mt]); load64(xr[mt] + (long)(c + 4) * 128, mok[mt], a1[mt]); }
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) mma(acc[mt], a0[mt][j], b0[j]);
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) mma(acc[mt], a1[mt][j], b1[j]);
  }
  if (c < c1) {
    u32x4 b0[4], a0[MT][4];
    load64(wr + (long)c * 128, nok, b0);
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) load64(xr[mt] + (long)c * 128, mok[mt], a0[mt]);
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) mma(acc[mt], a0[mt][j], b0[j]);
  }
  // red [3][MT][16][64]: waves 1..3 park their sums, wave 0 adds them in wave order
  if (wv > 0) {
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int g = 0; g < 16; ++g) red[(((wv - 1) * MT + mt) * 16 + g) * 64 + lane] = acc[mt][g];
  }
  __syncthreads();
  if (wv == 0) {
#pragma unroll
    for (int q = 0; q < 3; ++q)
#pragma unroll
      for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int g = 0; g < 16; ++g) acc[mt][g] += red[((q * MT + mt) * 16 + g) * 64 + lane];
  }
}

// C tile register g of lane (c, hh) holds row (g & 3) + 8 (g >> 2) + 4 hh, column c
__device__ __forceinline__ int crow(int g, int hh) { return (g & 3) + 8 * (g >> 2) + 4 * hh; }

template <int MT>
__global__ __launch_bounds__(256) void k_skinny_partial(const char* __restrict__ x, const char* __restrict__ w, float* __restrict__ part,
                                                        int M, int N, int K, int S) {
  __shared__ float red[3 * MT * 16 * 64];
  const int nch = K / 64, s = blockIdx.y, n0 = blockIdx.x * 32;
  const int c0 = (int)((long)nch * s / S), c1 = (int)((long)nch * (s + 1) / S);
  f32x16 acc[MT];
  tile_dot<MT>(x, w, M, N, K, n0, c0, c1, acc, red);
  if (threadIdx.x >= 64) return;
  const int lane = threadIdx.x, c = lane & 31, hh = lane >> 5, n = n0 + c;
  if (n >= N) return;
  float* ps = part + (long)s * M * N;
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int g = 0; g < 16; ++g) {
      const int m = mt * 32 + crow(g, hh);
      if (m < M) ps[(long)m * N + n] = acc[mt][g];
    }
}

// epilogue: 4 columns per thread; y = sum_s part[s] (s ascending) + bias [+ residual] -> f32, or -> bf16, or gelu_new -> bf16
__global__ __launch_bounds__(256) void k_skinny_epilogue(const float* __restrict__ part, const float* __restrict__ bias,
                                                         const float* residual, void* y, int M, int N, int S, int epi) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  const long n4 = (long)M * N / 4;
  if (i >= n4) return;
  const long e = i * 4;
  const int n = (int)(e % N);
  float4 a = ((const float4*)(part + e))[0];
  for (int s = 1; s < S; ++s) {
    const float4 b = ((const float4*)(part + (long)s * M * N + e))[0];
    a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w;
  }
  if (bias) { const float4 b = ((const float4*)(bias + n))[0]; a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w; }
  if (epi == 1) {
    if (residual) { const float4 b = ((const float4*)(residual + e))[0]; a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w; }
    ((float4*)((float*)y + e))[0] = a;
    return;
  }
  if (epi == 2) { a.x = gelu_new(a.x); a.y = gelu_new(a.y); a.z = gelu_new(a.z); a.w = gelu_new(a.w); }
  ((u32x2*)((unsigned short*)y + e))[0] = u32x2{pack2bf(a.x, a.y), pack2bf(a.z, a.w)};
}

// the fixed K split of an (N, K) shape: enough workgroups for the 256 CUs, never more splits than 64-element chunks
int skinny_splits(int N, int K) {
  const int tiles = (N + 31) / 32, nch = K / 64;
  int S = (256 + tiles - 1) / tiles;
  return S < nch ? S : nch;
}

// ---------------------------------------------------------------------------------------------------------------------------
// LM head: the skinny GEMM's tile (S = 1, the whole K in one workgroup), then per row the best (value, index) of the tile's 32
// columns.  Columns v >= V are -inf.  Order: larger value first, lower index among equal values -- a total order, so the result
// does not depend on the reduction tree.
__device__ __forceinline__ bool better(float a, int ia, float b, int ib) { return a > b || (a == b && ia < ib); }

template <int MT>
__global__ __launch_bounds__(256) void k_lm_head_partial(const char* __restrict__ h, const char* __restrict__ wte, float* __restrict__ pval,
                                                         int* __restrict__ pidx, float* __restrict__ logits, int M, int V, int K) {
  __shared__ float red[3 * MT * 16 * 64];
  const int n0 = blockIdx.x * 32, tiles = gridDim.x;
  f32x16 acc[MT];
  tile_dot<MT>(h, wte, M, V, K, n0, 0, K / 64, acc, red);
  if (threadIdx.x >= 64) return;
  const int lane = threadIdx.x, c = lane & 31, hh = lane >> 5, n = n0 + c;
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int g = 0; g < 16; ++g) {
      const int m = mt * 32 + crow(g, hh);
      float v = n < V ? acc[mt][g] : -INFINITY;
      if (logits && m < M && n < V) logits[(long)m * V + n] = v;
      int iv = n;
#pragma unroll
      for (int o = 16; o > 0; o >>= 1) {          // within the 32 lanes of this hh
        const float ov = __shfl_xor(v, o, 64);
        const int oi = __shfl_xor(iv, o, 64);
        if (better(ov, oi, v, iv)) { v = ov; iv = oi; }
      }
      if (c == 0 && m < M) { pval[(long)m * tiles + blockIdx.x] = v; pidx[(long)m * tiles + blockIdx.x] = iv; }
    }
}

__global__ __launch_bounds__(256) void k_lm_head_final(const float* __restrict__ pval, const int* __restrict__ pidx, long* __restrict__ ids,
                                                       int ld_ids, int tiles) {
  __shared__ float sv[4];
  __shared__ int si[4];
  const int m = blockIdx.x, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  float v = -INFINITY;
  int iv = 0x7fffffff;
  for (int t = threadIdx.x; t < tiles; t += 256) {
    const float a = pval[(long)m * tiles + t];
    const int ia = pidx[(long)m * tiles + t];
    if (better(a, ia, v, iv)) { v = a; iv = ia; }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(v, o, 64);
    const int oi = __shfl_xor(iv, o, 64);
    if (better(ov, oi, v, iv)) { v = ov; iv = oi; }
  }
  if (lane == 0) { sv[wv] = v; si[wv] = iv; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int q = 1; q < 4; ++q)
      if (better(sv[q], si[q], v, iv)) { v = sv[q]; iv = si[q]; }
    ids[(long)m * ld_ids] = iv == 0x7fffffff ? 0 : iv;   // (all -inf / NaN rows: index 0)
  }
}

// ---------------------------------------------------------------------------------------------------------------------------
// LM head top-B with log-normaliser (beam search).  The per-tile candidates are merged through the logits buffer: the LM-head tile
// writes the f32 logits [M][V] (the caller's, or workspace), then one 512-thread workgroup per row reads its row twice.  Pass 1: thread
// t walks columns t, t + 512, .. in ascending order and keeps its 8 best under better() sorted in registers; B rounds of "best head
// over the workgroup, its owner pops" emit the row's top B.  better() is a total order, so the result is the row's top B whatever the
// tree.  Pass 2: logZ = m + log(sum_j exp(l_j - m)), m = the row maximum: per thread in ascending column order, the 64 lanes by the
// xor butterfly, the 8 waves in wave order -- fixed by V alone.  A row's outputs depend on its own logits only, and those do not depend
// on M (tile_dot), so they are bitwise independent of M and of the other rows.  No atomics.
constexpr int TK_MAXB = 8;
constexpr int TK_THREADS = 512;

template <int MT>
__global__ __launch_bounds__(256) void k_lm_head_logits(const char* __restrict__ h, const char* __restrict__ wte, float* __restrict__ logits,
                                                        int M, int V, int K) {
  __shared__ float red[3 * MT * 16 * 64];
  const int n0 = blockIdx.x * 32;
  f32x16 acc[MT];
  tile_dot<MT>(h, wte, M, V, K, n0, 0, K / 64, acc, red);
  if (threadIdx.x >= 64) return;
  const int lane = threadIdx.x, c = lane & 31, hh = lane >> 5, n = n0 + c;
  if (n >= V) return;
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int g = 0; g < 16; ++g) {
      const int m = mt * 32 + crow(g, hh);
      if (m < M) logits[(long)m * V + n] = acc[mt][g];
    }
}

__global__ __launch_bounds__(TK_THREADS) void k_lm_head_topk(const float* __restrict__ logits, float* __restrict__ vals, int* __restrict__ idx,
                                                             float* __restrict__ logZ, int V, int B) {
  __shared__ float sv[TK_THREADS / 64];
  __shared__ int si[TK_THREADS / 64];
  const int m = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const float* row = logits + (long)m * V;
  float tv[TK_MAXB];
  int ti[TK_MAXB];
#pragma unroll
  for (int q = 0; q < TK_MAXB; ++q) { tv[q] = -INFINITY; ti[q] = 0x7fffffff; }
  for (int j0 = tid; j0 < V; j0 += 8 * TK_THREADS) {           // eight loads in flight, then the inserts in ascending column order
    float x[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) { const int j = j0 + u * TK_THREADS; x[u] = j < V ? row[j] : -INFINITY; }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int j = j0 + u * TK_THREADS;
      if (j < V && better(x[u], j, tv[TK_MAXB - 1], ti[TK_MAXB - 1])) {
        tv[TK_MAXB - 1] = x[u];
        ti[TK_MAXB - 1] = j;
#pragma unroll
        for (int q = TK_MAXB - 1; q > 0; --q)
          if (better(tv[q], ti[q], tv[q - 1], ti[q - 1])) {
            const float a = tv[q]; tv[q] = tv[q - 1]; tv[q - 1] = a;
            const int ia = ti[q]; ti[q] = ti[q - 1]; ti[q - 1] = ia;
          }
      }
    }
  }
  float mx = -INFINITY;
  for (int r = 0; r < B; ++r) {
    float v = tv[0];
    int iv = ti[0];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(v, o, 64);
      const int oi = __shfl_xor(iv, o, 64);
      if (better(ov, oi, v, iv)) { v = ov; iv = oi; }
    }
    if (lane == 0) { sv[wv] = v; si[wv] = iv; }
    __syncthreads();
    v = sv[0];
    iv = si[0];
#pragma unroll
    for (int q = 1; q < TK_THREADS / 64; ++q)
      if (better(sv[q], si[q], v, iv)) { v = sv[q]; iv = si[q]; }
    __syncthreads();                                   // every thread has read sv / si before the next round writes them
    if (tid == 0) { vals[(long)m * B + r] = v; idx[(long)m * B + r] = iv == 0x7fffffff ? 0 : iv; }   // (NaN rows: index 0)
    if (r == 0) mx = v;
    if (iv == ti[0]) {                                 // the owner pops (column indices are unique)
#pragma unroll
      for (int q = 0; q < TK_MAXB - 1; ++q) { tv[q] = tv[q + 1]; ti[q] = ti[q + 1]; }
      tv[TK_MAXB - 1] = -INFINITY;
      ti[TK_MAXB - 1] = 0x7fffffff;
    }
  }
  float sum = 0.f;
  for (int j0 = tid; j0 < V; j0 += 8 * TK_THREADS) {
    float x[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) { const int j = j0 + u * TK_THREADS; x[u] = j < V ? row[j] : -INFINITY; }
#pragma unroll
    for (int u = 0; u < 8; ++u)
      if (j0 + u * TK_THREADS < V) sum += expf(x[u] - mx);
  }
  sum = wave_sum(sum);
  if (lane == 0) sv[wv] = sum;
  __syncthreads();
  if (tid == 0) {
    float a = sv[0];
    for (int q = 1; q < TK_THREADS / 64; ++q) a += sv[q];
    logZ[m] = mx + logf(a);
  }
}

// ---------------------------------------------------------------------------------------------------------------------------
// Beam selection, one wave per caption.  Lane (b = lane / B, k = lane % B) holds the k-th best token of beam b: logp = logit - logZ_b,
// cand_sum = sum_b + logp, cand_len = len_b + 1, key = cand_sum / cand_len (IEEE division), all f32 in this order.  A stopped beam
// offers itself once (lane k = 0: its own sum and length, token column 0).  A candidate's rank is the number of candidates that beat
// it: larger key, then lower (beam, token) -- a total order, so ranks 0..B-1 each have one owner.  New beam j takes rank j: its
// source's history and ancestry (old tables read, new tables written), the token unless the source was stopped, and for the cache
// the source's slot as the owner of the step just run.  step == 0: one row per caption, beam j takes the row's j-th (value, index).
__global__ __launch_bounds__(64) void k_beam_step(const float* __restrict__ vals, const int* __restrict__ idx, const float* __restrict__ logZ,
                                                  const float* __restrict__ sum_in, const int* __restrict__ len_in,
                                                  const unsigned char* __restrict__ stop_in, const int* __restrict__ hist_in,
                                                  const unsigned char* __restrict__ anc_in, float* __restrict__ sum_out,
                                                  int* __restrict__ len_out, unsigned char* __restrict__ stop_out, int* __restrict__ hist_out,
                                                  unsigned char* __restrict__ anc_out, int* __restrict__ src, long* __restrict__ next_tok,
                                                  int B, int T, int step, int stop_id) {
  const int c = blockIdx.x, lane = threadIdx.x;
  const int b = lane / B, k = lane - b * B;
  int valid = 0, v = 0, clen = 0, sstop = 0, rank = 0;
  float csum = 0.f, key = 0.f;
  if (step == 0) {
    valid = lane < B;
    if (valid) {
      v = idx[(long)c * B + k];
      csum = vals[(long)c * B + k] - logZ[c];
      clen = 1;
    }
    rank = k;
  } else {
    valid = lane < B * B;
    if (valid) {
      const long row = (long)c * B + b;
      sstop = stop_in[row] != 0;
      const float s = sum_in[row];
      const int l = len_in[row];
      if (sstop) {
        valid = k == 0;
        csum = s;
        clen = l;
      } else {
        v = idx[row * B + k];
        const float logp = vals[row * B + k] - logZ[row];
        csum = s + logp;
        clen = l + 1;
      }
      key = __fdiv_rn(csum, (float)clen);
    }
    for (int l2 = 0; l2 < B * B; ++l2) {
      const int ok2 = __shfl(valid, l2, 64), v2 = __shfl(v, l2, 64);
      const float key2 = __shfl(key, l2, 64);
      const int b2 = l2 / B;
      rank += ok2 && (key2 > key || (key2 == key && (b2 < b || (b2 == b && v2 < v))));
    }
  }
  const int ld = T - 1;
  for (int j = 0; j < B; ++j) {
    const unsigned long long owners = __ballot(valid && rank == j);
    if (!owners) continue;                              // (NaN keys only: ranks collide)
    const int w = __ffsll((long long)owners) - 1;
    const int sb = __shfl(b, w, 64), tok = __shfl(v, w, 64), was = __shfl(sstop, w, 64), nl = __shfl(clen, w, 64);
    const float ns = __shfl(csum, w, 64);
    const long nr = (long)c * B + j, sr = (long)c * B + sb;
    for (int t = lane; t < step; t += 64) hist_out[nr * T + t] = hist_in[sr * T + t];
    for (int t = lane; t < step - 1; t += 64) anc_out[nr * ld + t] = anc_in[sr * ld + t];
    if (lane == 0) {
      const int stopped = was || tok == stop_id;
      sum_out[nr] = ns;
      len_out[nr] = nl;
      stop_out[nr] = (unsigned char)stopped;
      src[nr] = sb;
      next_tok[nr] = stopped ? stop_id : tok;
      hist_out[nr * T + step] = was ? -1 : tok;
      if (step >= 1) anc_out[nr * ld + step - 1] = (unsigned char)sb;
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------------
// Decode attention.  One 256-thread workgroup per (sequence s, head h); head dim 64.  qkv row s = c_attn's output of this step
// (q | k | v column blocks of W = heads * 64).  Keys / values of positions j < L - 1 come from the cache kc / vc [nseq][Lmax][W], the
// key / value of position L - 1 from qkv itself; the workgroup also writes them to the cache at L - 1 for the next steps.
// Scores (f32, one per key, in LDS) -> softmax -> o = sum_j p_j v_j, 32 key groups x 8 column groups, summed in group order.
constexpr int DA_MAXL = 1024;

__device__ __forceinline__ void row8(const unsigned short* p, float (&v)[8]) {
  const u32x4 u = *(const u32x4*)p;
#pragma unroll
  for (int e = 0; e < 4; ++e) { v[2 * e] = bf2f(u[e] & 0xffff); v[2 * e + 1] = bf2f(u[e] >> 16); }
}

// Beam search (BEAM): row s = caption * B + beam.  Positions j < P come from the caption's prefix cache pk / pv [captions][P][W], which its
// beams share; positions P <= j < L - 1 from the generated cache kc / vc [rows][Lmax][W] at row caption * B + anc[s][j - P], position
// j - P, where anc [rows][ldanc] names the beam slot that wrote step j - P of this beam's history (k_beam_step keeps it); position L - 1
// from qkv, written to the generated cache at row s, position L - 1 - P.  No cache row ever moves.  The arithmetic and its order are
// the same in both instantiations.
struct BeamKV {
  const unsigned short* pk;
  const unsigned short* pv;
  const unsigned char* anc;
  int B, P, ldanc;
};

template <bool BEAM>
__device__ __forceinline__ const unsigned short* kv_row(const unsigned short* cache, const unsigned short* pre, const BeamKV& bm, int s,
                                                        int j, int Lmax, int W) {
  if constexpr (!BEAM) return cache + ((long)s * Lmax + j) * W;
  const int cap = s / bm.B;
  if (j < bm.P) return pre + ((long)cap * bm.P + j) * W;
  const int t = j - bm.P;
  int a = bm.anc[(long)s * bm.ldanc + t];
  a = a < bm.B ? a : bm.B - 1;                       // (memory safety only: k_beam_step writes slots < B)
  return cache + ((long)(cap * bm.B + a) * Lmax + t) * W;
}

template <bool BEAM>
__global__ __launch_bounds__(256) void k_decode_attn(const unsigned short* __restrict__ qkv, unsigned short* kc, unsigned short* vc,
                                                     unsigned short* __restrict__ o, int heads, int L, int Lmax, int ldqkv, float scale,
                                                     BeamKV bm) {
  __shared__ float q[64];
  __shared__ float sc[DA_MAXL];
  __shared__ float red[32 * 64];
  __shared__ float wred[4];
  const int W = heads * 64;
  const int s = blockIdx.x / heads, h = blockIdx.x - s * heads;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const unsigned short* qr = qkv + (long)s * ldqkv + h * 64;
  const unsigned short* knew = qr + W;
  const unsigned short* vnew = qr + 2 * W;
  const long wbase = ((long)s * Lmax + (BEAM ? L - 1 - bm.P : L - 1)) * W + h * 64;      // where this step's key / value go
  if (tid < 64) q[tid] = bf2f(qr[tid]);
  else if (tid < 72) ((u32x4*)(kc + wbase))[tid - 64] = ((const u32x4*)knew)[tid - 64];
  else if (tid < 80) ((u32x4*)(vc + wbase))[tid - 72] = ((const u32x4*)vnew)[tid - 72];
  __syncthreads();
  float m = -INFINITY;
  for (int j = tid; j < L; j += 256) {
    const unsigned short* kr = j == L - 1 ? knew : kv_row<BEAM>(kc, bm.pk, bm, s, j, Lmax, W) + h * 64;
    float d = 0.f;
#pragma unroll
    for (int c8 = 0; c8 < 8; ++c8) {
      float kv[8];
      row8(kr + c8 * 8, kv);
#pragma unroll
      for (int e = 0; e < 8; ++e) d += q[c8 * 8 + e] * kv[e];
    }
    d *= scale;
    sc[j] = d;
    m = fmaxf(m, d);
  }
  m = wave_max(m);
  if (lane == 0) wred[wv] = m;
  __syncthreads();
  m = fmaxf(fmaxf(wred[0], wred[1]), fmaxf(wred[2], wred[3]));
  float sum = 0.f;
  for (int j = tid; j < L; j += 256) { const float e = __expf(sc[j] - m); sc[j] = e; sum += e; }
  sum = wave_sum(sum);
  __syncthreads();                                   // every wave has read wred (the max) before it is reused for the sum
  if (lane == 0) wred[wv] = sum;
  __syncthreads();
  const float inv = 1.f / (wred[0] + wred[1] + wred[2] + wred[3]);
  const int c8 = tid & 7, grp = tid >> 3;
  float acc[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) acc[e] = 0.f;
  for (int j = grp; j < L; j += 32) {
    const unsigned short* vr = j == L - 1 ? vnew : kv_row<BEAM>(vc, bm.pv, bm, s, j, Lmax, W) + h * 64;
    float vv[8];
    row8(vr + c8 * 8, vv);
    const float p = sc[j];
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] += p * vv[e];
  }
#pragma unroll
  for (int e = 0; e < 8; ++e) red[grp * 64 + c8 * 8 + e] = acc[e];
  __syncthreads();
  if (tid < 64) {
    float a = 0.f;
    for (int g = 0; g < 32; ++g) a += red[g * 64 + tid];
    o[(long)s * W + h * 64 + tid] = f2bf(a * inv);
  }
}

// ---------------------------------------------------------------------------------------------------------------------------
// x[r] = (ids ? tab[ids[r * ld_ids]] : src[r]) + wpe[pos0 + r % t]; one thread per 8 columns
template <typename T> struct Row8;
template <> struct Row8<__bf16> {
  __device__ static __forceinline__ void get(const void* row, int c8, float (&v)[8]) { row8((const unsigned short*)row + c8 * 8, v); }
};
template <> struct Row8<float> {
  __device__ static __forceinline__ void get(const void* row, int c8, float (&v)[8]) {
    const float4 a = ((const float4*)row)[2 * c8], b = ((const float4*)row)[2 * c8 + 1];
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
  }
};

template <typename T>
__global__ __launch_bounds__(256) void k_pos_embed(const long* __restrict__ ids, int ld_ids, const void* __restrict__ tab,
                                                   const float* __restrict__ src, const float* __restrict__ wpe, float* __restrict__ x,
                                                   long rows, int t, int pos0, int W, int vocab) {
  const int per_row = W / 8;
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= rows * per_row) return;
  const long row = idx / per_row;
  const int c8 = (int)(idx - row * per_row);
  float v[8];
  if (ids) {
    long id = ids[row * ld_ids];
    id = (id < 0 || id >= vocab) ? 0 : id;           // (memory safety only: ids come from the LM head, always in range)
    Row8<T>::get((const char*)tab + id * (long)W * sizeof(T), c8, v);
  } else {
    Row8<float>::get(src + row * W, c8, v);
  }
  const float4* pr = (const float4*)(wpe + (long)(pos0 + row % t) * W) + 2 * c8;
  const float4 p0 = pr[0], p1 = pr[1];
  float4* out = (float4*)(x + row * W) + 2 * c8;
  out[0] = make_float4(v[0] + p0.x, v[1] + p0.y, v[2] + p0.z, v[3] + p0.w);
  out[1] = make_float4(v[4] + p1.x, v[5] + p1.y, v[6] + p1.z, v[7] + p1.w);
}

int launch_pos_embed(const long* ids, int ld_ids, const void* tab, const float* src, const float* wpe, float* x, long rows, int t, int pos0,
                     int W, int vocab, int dtype, void* stream) {
  if (rows == 0) return CDDMSL_OK;
  const long n = rows * (W / 8);
  const dim3 grid((unsigned)((n + 255) / 256));
  if (dtype == 0) hipLaunchKernelGGL(k_pos_embed<__bf16>, grid, dim3(256), 0, (hipStream_t)stream, ids, ld_ids, tab, src, wpe, x, rows, t, pos0, W, vocab);
  else hipLaunchKernelGGL(k_pos_embed<float>, grid, dim3(256), 0, (hipStream_t)stream, ids, ld_ids, tab, src, wpe, x, rows, t, pos0, W, vocab);
  return launch_status();
}

}  // namespace

extern "C" int cddmsl_skinny_gemm_workspace(int M, int N, int K) {
  if (M < 1 || M > SK_MAXM || N <= 0 || N > (1 << 20) || K <= 0 || (K & 63)) return -1;
  return skinny_splits(N, K) * M * N * 4;
}

extern "C" int cddmsl_skinny_gemm(const void* x, const void* w, const float* bias, const float* residual, void* y, float* ws, long ws_bytes,
                                  int M, int N, int K, int epi, void* stream) {
  if (M < 1 || M > SK_MAXM || N <= 0 || (N & 7) || K <= 0 || (K & 63) || epi < 0 || epi > 2) return CDDMSL_ERR_ARG;
  if (residual && epi != 1) return CDDMSL_ERR_ARG;
  if (!al16(x) || !al16(w) || !al16(y) || !al16(ws) || (bias && !al16(bias)) || (residual && !al16(residual))) return CDDMSL_ERR_ARG;
  const int S = skinny_splits(N, K);
  if (ws_bytes < (long)S * M * N * 4) return CDDMSL_ERR_ARG;
  const hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)((N + 31) / 32), (unsigned)S);
  if (M <= 32) hipLaunchKernelGGL(k_skinny_partial<1>, grid, dim3(256), 0, st, (const char*)x, (const char*)w, ws, M, N, K, S);
  else hipLaunchKernelGGL(k_skinny_partial<2>, grid, dim3(256), 0, st, (const char*)x, (const char*)w, ws, M, N, K, S);
  const long n4 = (long)M * N / 4;
  hipLaunchKernelGGL(k_skinny_epilogue, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, st, ws, bias, residual, y, M, N, S, epi);
  return launch_status();
}

extern "C" int cddmsl_lm_head_workspace(int M, int V) {
  if (M < 1 || M > SK_MAXM || V <= 0 || V > (1 << 22)) return -1;
  return M * ((V + 31) / 32) * 8;
}

extern "C" int cddmsl_lm_head_argmax(const void* h, const void* wte, long* ids, int ld_ids, float* logits, void* ws, long ws_bytes, int M,
                                     int V, int K, void* stream) {
  if (M < 1 || M > SK_MAXM || V <= 0 || K <= 0 || (K & 63) || ld_ids < 1) return CDDMSL_ERR_ARG;
  if (!al16(h) || !al16(wte) || !al16(ws)) return CDDMSL_ERR_ARG;
  const int tiles = (V + 31) / 32;
  if (ws_bytes < (long)M * tiles * 8) return CDDMSL_ERR_ARG;
  float* pval = (float*)ws;
  int* pidx = (int*)((char*)ws + (long)M * tiles * 4);
  const hipStream_t st = (hipStream_t)stream;
  if (M <= 32) hipLaunchKernelGGL(k_lm_head_partial<1>, dim3(tiles), dim3(256), 0, st, (const char*)h, (const char*)wte, pval, pidx, logits, M, V, K);
  else hipLaunchKernelGGL(k_lm_head_partial<2>, dim3(tiles), dim3(256), 0, st, (const char*)h, (const char*)wte, pval, pidx, logits, M, V, K);
  hipLaunchKernelGGL(k_lm_head_final, dim3(M), dim3(256), 0, st, pval, pidx, ids, ld_ids, tiles);
  return launch_status();
}

extern "C" int cddmsl_decode_attn(const void* qkv, void* kc, void* vc, void* o, int nseq, int heads, int dh, int L, int Lmax, int ldqkv,
                                  float scale, int dtype, void* stream) {
  if (dtype != 0 || dh != 64 || nseq < 0 || heads <= 0 || L < 1 || L > Lmax || L > DA_MAXL || (ldqkv & 7) || ldqkv < 3 * heads * 64)
    return CDDMSL_ERR_ARG;
  if (!al16(qkv) || !al16(kc) || !al16(vc) || !al16(o)) return CDDMSL_ERR_ARG;
  if (nseq == 0) return CDDMSL_OK;
  const long wgs = (long)nseq * heads;
  if (wgs > 0x7fffffffL) return CDDMSL_ERR_ARG;
  hipLaunchKernelGGL(k_decode_attn<false>, dim3((unsigned)wgs), dim3(256), 0, (hipStream_t)stream, (const unsigned short*)qkv,
                     (unsigned short*)kc, (unsigned short*)vc, (unsigned short*)o, heads, L, Lmax, ldqkv, scale, BeamKV{});
  return launch_status();
}

extern "C" int cddmsl_lm_head_topk_workspace(int M, int V) {
  if (M < 1 || M > SK_MAXM || V <= 0 || V > (1 << 22)) return -1;
  return M * V * 4;
}

extern "C" int cddmsl_lm_head_topk(const void* h, const void* wte, float* vals, int* idx, float* logZ, float* logits, void* ws, long ws_bytes,
                                   int M, int V, int K, int B, void* stream) {
  if (M < 1 || M > SK_MAXM || V <= 0 || V > (1 << 22) || K <= 0 || (K & 63) || B < 1 || B > TK_MAXB || B > V) return CDDMSL_ERR_ARG;
  if (!al16(h) || !al16(wte) || !vals || !idx || !logZ) return CDDMSL_ERR_ARG;
  if (!logits) {
    if (!ws || ws_bytes < (long)M * V * 4) return CDDMSL_ERR_ARG;
    logits = (float*)ws;
  }
  const hipStream_t st = (hipStream_t)stream;
  const int tiles = (V + 31) / 32;
  if (M <= 32) hipLaunchKernelGGL(k_lm_head_logits<1>, dim3(tiles), dim3(256), 0, st, (const char*)h, (const char*)wte, logits, M, V, K);
  else hipLaunchKernelGGL(k_lm_head_logits<2>, dim3(tiles), dim3(256), 0, st, (const char*)h, (const char*)wte, logits, M, V, K);
  hipLaunchKernelGGL(k_lm_head_topk, dim3(M), dim3(TK_THREADS), 0, st, (const float*)logits, vals, idx, logZ, V, B);
  return launch_status();
}

extern "C" int cddmsl_beam_step(const float* vals, const int* idx, const float* logZ, const float* sum_in, const int* len_in,
                                const unsigned char* stop_in, const int* hist_in, const unsigned char* anc_in, float* sum_out, int* len_out,
                                unsigned char* stop_out, int* hist_out, unsigned char* anc_out, int* src, long* next_tok, int n, int B, int T,
                                int step, int stop_id, void* stream) {
  if (n < 0 || B < 1 || B > TK_MAXB || T < 1 || step < 0 || step >= T || stop_id < -1) return CDDMSL_ERR_ARG;
  if (!vals || !idx || !logZ || !sum_out || !len_out || !stop_out || !hist_out || !src || !next_tok) return CDDMSL_ERR_ARG;
  if (step >= 1 && (!sum_in || !len_in || !stop_in || !hist_in || !anc_in || !anc_out)) return CDDMSL_ERR_ARG;
  if (n == 0) return CDDMSL_OK;
  hipLaunchKernelGGL(k_beam_step, dim3((unsigned)n), dim3(64), 0, (hipStream_t)stream, vals, idx, logZ, sum_in, len_in, stop_in, hist_in, anc_in,
                     sum_out, len_out, stop_out, hist_out, anc_out, src, next_tok, B, T, step, stop_id);
  return launch_status();
}

extern "C" int cddmsl_decode_attn_beam(const void* qkv, const void* pk, const void* pv, void* gk, void* gv, const unsigned char* anc, void* o,
                                       int rows, int B, int heads, int dh, int P, int L, int Tg, int ldanc, int ldqkv, float scale, int dtype,
                                       void* stream) {
  if (dtype != 0 || dh != 64 || rows < 0 || B < 1 || B > TK_MAXB || rows % B || heads <= 0 || P < 0 || L < P + 1 || L - P > Tg ||
      L > DA_MAXL || ldanc < L - 1 - P || (ldqkv & 7) || ldqkv < 3 * heads * 64)
    return CDDMSL_ERR_ARG;
  if (!al16(qkv) || !al16(pk) || !al16(pv) || !al16(gk) || !al16(gv) || !al16(o) || (L - 1 - P > 0 && !anc)) return CDDMSL_ERR_ARG;
  if (rows == 0) return CDDMSL_OK;
  const long wgs = (long)rows * heads;
  if (wgs > 0x7fffffffL) return CDDMSL_ERR_ARG;
  const BeamKV bm{(const unsigned short*)pk, (const unsigned short*)pv, anc, B, P, ldanc};
  hipLaunchKernelGGL(k_decode_attn<true>, dim3((unsigned)wgs), dim3(256), 0, (hipStream_t)stream, (const unsigned short*)qkv,
                     (unsigned short*)gk, (unsigned short*)gv, (unsigned short*)o, heads, L, Tg, ldqkv, scale, bm);
  return launch_status();
}

extern "C" int cddmsl_pos_embed(const long* ids, int ld_ids, const void* tab, const float* src, const float* wpe, float* x, long rows, int t,
                                int pos0, int W, int vocab, int npos, int dtype, void* stream) {
  if (rows < 0 || t <= 0 || pos0 < 0 || pos0 + t > npos || W <= 0 || (W & 7) || (dtype != 0 && dtype != 1)) return CDDMSL_ERR_ARG;
  if ((ids == nullptr) == (src == nullptr) || (ids && (tab == nullptr || ld_ids < 1 || vocab <= 0 || !al16(tab))) || (src && !al16(src))) return CDDMSL_ERR_ARG;
  if (!al16(wpe) || !al16(x)) return CDDMSL_ERR_ARG;
  return launch_pos_embed(ids, ld_ids, tab, src, wpe, x, rows, t, pos0, W, vocab, dtype, stream);
}

extern "C" int cddmsl_text_embed(const long* ids, const void* tok, const float* pos, float* x, long rows, int t, int W, int vocab, int dtype,
                                 void* stream) {
  if (rows < 0 || t <= 0 || W <= 0 || (W & 7) || vocab <= 0 || (dtype != 0 && dtype != 1)) return CDDMSL_ERR_ARG;
  if (!al16(tok) || !al16(pos) || !al16(x)) return CDDMSL_ERR_ARG;
  return launch_pos_embed(ids, 1, tok, nullptr, pos, x, rows, t, 0, W, vocab, dtype, stream);
}
