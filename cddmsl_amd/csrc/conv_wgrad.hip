// Weight-gradient kernels (kernel ids 4, 5, 6; 12 with e4m3 operands), the batched TN GEMM kernels on the same structure (kernel
// ids 7, 9) and the reduction of their splits through the workspace.  WgradArgs: gemm_common.h; data layout: see gemm_conv.hip.
#include "gemm_common.h"

namespace {

template <typename T> struct TrFrag;
template <> struct TrFrag<__bf16> {
  // Reads the MFMA operand fragment (8 reduction elements for column `col`) out of a row-major
  // [m][col] LDS image with two ds_read_b64_tr_b16: group of 16 lanes <-> 16 columns, lane 4q+p
  // supplies row q, columns 4p..4p+3, and receives its own column's 4 rows.
  __device__ static __forceinline__ u32x4 read(const u32x4* base, int mrow0, int col0, int lane) {
    int g = lane >> 4, li = lane & 15, q = li >> 2, pp = li & 3;
    int hh = g >> 1;                      // lane half = k-group of the MFMA operand
    int col = col0 + 16 * (g & 1) + 4 * pp;
    const char* b = (const char*)base;
    const char* a0 = b + (long)(mrow0 + 8 * hh + q) * (WROW * 16) + col * 2;
    const char* a1 = a0 + 4 * (WROW * 16);
    i16x4 v0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) i16x4*)a0);
    i16x4 v1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) i16x4*)a1);
    u32x2 p0 = __builtin_bit_cast(u32x2, v0), p1 = __builtin_bit_cast(u32x2, v1);
    u32x4 r = {p0[0], p0[1], p1[0], p1[1]};
    return r;
  }
  static constexpr int MSTEP = 16;  // reduction elements per Mma step
};
template <> struct TrFrag<float> {
  // f32: Mma<float>::step contracts k = 4h + j; element j of lane (r, h) = image[mrow0 + 4h + j][col0 + r]
  __device__ static __forceinline__ u32x4 read(const u32x4* base, int mrow0, int col0, int lane) {
    int r = lane & 31, hh = lane >> 5;
    const char* b = (const char*)base;
    u32x4 v;
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = *(const unsigned int*)(b + (long)(mrow0 + 4 * hh + j) * (WROW * 16) + (col0 + r) * 4);
    return v;
  }
  static constexpr int MSTEP = 8;
};

template <typename T>
__global__ __launch_bounds__(256, 2) void k_conv_wgrad(WgradArgs p) {
  constexpr int ES = Mma<T>::ES;
  constexpr int TC = 128 * ES / 16;   // chunks per 128-element tile row (bf16: 16, f32: 32)
  constexpr int COLS = 256 / ES;      // columns held per LDS image row (bf16: 128, f32: 64)
  // f32 tiles are 64 columns wide (256 B rows) so both dtypes share the 256 B + pad row geometry.
  __shared__ __attribute__((aligned(16))) u32x4 lds[2][WM * WROW];
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const int ntn = (p.Cout + COLS - 1) / COLS, ntk = (p.K + COLS - 1) / COLS;
  int bid = xcd_remap(blockIdx.x, gridDim.x);
  const int tile_k = bid % ntk; bid /= ntk;
  const int tile_n = bid % ntn; bid /= ntn;
  const int split = bid;
  const int n0 = tile_n * COLS, k0 = tile_k * COLS;
  const int mt0 = split * p.mtiles_per_split;
  const int total_mt = (p.M + WM - 1) / WM;
  const int mt1 = min(mt0 + p.mtiles_per_split, total_mt);
  (void)TC;

  // staging map: 64 rows x 16 chunks = 1024 chunks per operand; thread -> chunk cc = t&15, rows t>>4 + 16 i
  const int cc = t & 15, rb = t >> 4;
  const int kc = k0 * ES / 16 + cc;          // global K chunk of the A-operand (im2col) column
  const bool vk = kc < p.Kc;
  const int pp = vk ? kc / p.cpp : 0, coff = vk ? kc - pp * p.cpp : 0;
  const int ky = pp / p.KW, kx = pp - ky * p.KW;
  const int nc = n0 * ES / 16 + cc;          // chunk along dY's channel axis
  const bool vn = nc < p.ncc;
  const u32x4 zero = {0u, 0u, 0u, 0u};
  u32x4 rx[4], rd[4];

  auto gload = [&](int mt) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      int m = mt * WM + rb + 16 * i;
      bool vmm = m < p.M;
      unsigned mm = vmm ? m : 0;
      unsigned tq = fdiv(mm, p.dWo);
      int ox = (int)(mm - tq * p.Wo);
      unsigned img = fdiv(tq, p.dHo);
      int oy = (int)(tq - img * p.Ho);
      if (!p.pool) {
        int iy = oy * p.stride - p.pad + ky, ix = ox * p.stride - p.pad + kx;
        bool ok = vmm && vk && iy >= 0 && iy < p.Hi && ix >= 0 && ix < p.Wi;
        rx[i] = ok ? *(const u32x4*)(p.x + ((((long)img * p.Hi + iy) * p.Wi + ix) * p.cpp + coff) * 16) : zero;
      } else {
        if (vmm && vk) {
          const char* b0 = p.x + ((((long)img * p.Hi + 2 * oy) * p.Wi + 2 * ox) * p.cpp + coff) * 16;
          long rs = (long)p.Wi * p.cpp * 16, cs = (long)p.cpp * 16;
          rx[i] = avg4<T>(*(const u32x4*)b0, *(const u32x4*)(b0 + cs), *(const u32x4*)(b0 + rs), *(const u32x4*)(b0 + rs + cs));
        } else rx[i] = zero;
      }
      rd[i] = (vmm && vn) ? *(const u32x4*)(p.dy + ((long)m * p.ldd) * ES + (long)nc * 16) : zero;
    }
  };

  // wave tiling of the COLS x COLS output tile: 2x2 waves
  constexpr int WT = COLS / 2;       // per-wave extent (bf16: 64, f32: 32)
  constexpr int NT = WT / 32;        // 32x32 tiles per wave per dim (bf16: 2, f32: 1)
  const int wn = wv >> 1, wk = wv & 1;
  f32x16 acc[NT][NT];
#pragma unroll
  for (int a = 0; a < NT; ++a)
#pragma unroll
    for (int b = 0; b < NT; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;

  if (mt0 < mt1) gload(mt0);
  for (int mt = mt0; mt < mt1; ++mt) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      int row = rb + 16 * i;
      lds[0][row * WROW + cc] = rd[i];
      lds[1][row * WROW + cc] = rx[i];
    }
    __syncthreads();
    if (mt + 1 < mt1) gload(mt + 1);
#pragma unroll
    for (int ms = 0; ms < WM; ms += TrFrag<T>::MSTEP) {
      u32x4 fa[NT], fb[NT];
#pragma unroll
      for (int i = 0; i < NT; ++i) {
        fa[i] = TrFrag<T>::read(lds[0], ms, wn * WT + i * 32, lane);
        fb[i] = TrFrag<T>::read(lds[1], ms, wk * WT + i * 32, lane);
      }
#pragma unroll
      for (int a = 0; a < NT; ++a)
#pragma unroll
        for (int b = 0; b < NT; ++b) Mma<T>::step(acc[a][b], fa[a], fb[b]);
    }
    __syncthreads();
  }

  const int r = lane & 31, h = lane >> 5;
#pragma unroll
  for (int a = 0; a < NT; ++a)
#pragma unroll
    for (int b = 0; b < NT; ++b) {
      int k = k0 + wk * WT + b * 32 + r;
      if (k >= p.K) continue;
#pragma unroll
      for (int g = 0; g < 16; ++g) {
        int n = n0 + wn * WT + a * 32 + (g & 3) + 8 * (g >> 2) + 4 * h;
        if (n >= p.Cout) continue;
        float v = acc[a][b][g] * (p.scale ? p.scale[n] : 1.f);
        atomicAdd(p.dw + (long)n * p.K + k, v);
      }
    }
}

// ------------------------------------------------------------------------------------------------
// wgrad, LDS-DMA variant for stride-1 "same" convolutions (1x1/pad 0 and 3x3/pad 1: every trainable layer).
// Output pixel index == input pixel index, so both operands are walked with pointer increments (64 rows per tile);
// tiles go global -> LDS by global_load_lds (no VGPR -> LDS write pass, the limiter of the register-staged kernel
// at two blocks per CU), double-buffered with a counted vmcnt.  LDS rows are plain 256 B; the 16-byte chunk index is
// XOR-swizzled by f(row) = ((row&3)<<2) | ((row>>2)&3) -- applied to the SOURCE chunk a lane fetches and to the
// transposed reads -- which keeps ds_read_b64_tr_b16 conflict-free without row padding (padding is impossible with
// lane-linear DMA writes).
// ------------------------------------------------------------------------------------------------

// Fragment addressing is split into a per-lane part computed ONCE (fsw of rows ms + 8hh + q does not depend on the
// 16-row step ms, since ms % 16 == 0) and a compile-time row offset ms * 256 that folds into the DS immediate.
template <typename T> struct TrFragS;
template <> struct TrFragS<__bf16> {
  struct Off { int o0, o1; };
  __device__ static __forceinline__ Off prep(int col0, int lane) {
    int g = lane >> 4, li = lane & 15, q = li >> 2, pp = li & 3;
    int hh = g >> 1;
    int ch = ((col0 + 16 * (g & 1)) >> 3) + (pp >> 1);       // logical 16-byte chunk of columns 4pp..4pp+3
    int r0 = 8 * hh + q, r1 = r0 + 4;
    Off o;
    o.o0 = r0 * 256 + 16 * (ch ^ fsw(r0)) + 8 * (pp & 1);
    o.o1 = r1 * 256 + 16 * (ch ^ fsw(r1)) + 8 * (pp & 1);
    return o;
  }
  // Inline asm on purpose: through the builtin, hipcc treats the transposed read as "may alias the in-flight LDS-DMA"
  // and drains vmcnt(0) before it (no overlap with the next tile's DMA).  The asm reads are ordered by the caller's
  // counted vmcnt + barrier before, and by an explicit lgkmcnt(0) + sched_barrier after (tr_wait()).
  __device__ static __forceinline__ u32x4 read(const u32x4* base, int ms, const Off& o) {
    const unsigned a = (unsigned)(size_t)(const __attribute__((address_space(3))) char*)((const char*)base) + ms * 256;
    u32x2 p0, p1;
    asm volatile("ds_read_b64_tr_b16 %0, %1" : "=v"(p0) : "v"(a + o.o0));
    asm volatile("ds_read_b64_tr_b16 %0, %1" : "=v"(p1) : "v"(a + o.o1));
    u32x4 r = {p0[0], p0[1], p1[0], p1[1]};
    return r;
  }
  static constexpr int MSTEP = 16;
};
template <> struct TrFragS<float> {
  struct Off { int o[4]; };
  __device__ static __forceinline__ Off prep(int col0, int lane) {
    int r = lane & 31, hh = lane >> 5;
    int byte = (col0 + r) * 4;
    Off o;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      int row = 4 * hh + j;                                  // + ms (multiple of 8): fsw(row + 8k) flips bit 1 of (row>>2)&3
      o.o[j] = row * 256 + (byte & 15) + 16 * (byte >> 4);   // swizzle applied in read (depends on ms & 8)
    }
    return o;
  }
  __device__ static __forceinline__ u32x4 read(const u32x4* base, int ms, const Off& o) {
    const char* b = (const char*)base;
    u32x4 v;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      int off = o.o[j] + ms * 256;
      int row = off >> 8, ch = (off >> 4) & 15;
      v[j] = *(const unsigned int*)(b + (off & ~0xf0) + 16 * (ch ^ fsw(row)));
    }
    return v;
  }
  static constexpr int MSTEP = 8;
};

template <typename T>
__global__ __launch_bounds__(256, 2) void k_conv_wgrad_dma(WgradArgs p) {
  constexpr int ES = Mma<T>::ES;
  constexpr int COLS = 256 / ES;
  __shared__ __attribute__((aligned(16))) u32x4 lds[2][2][WM * 16];   // [buffer][dY | X][64 rows x 16 chunks]
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  p.x += (long)blockIdx.y * p.bx; p.dy += (long)blockIdx.y * p.bd;
  char* outp = (char*)p.dw + (long)blockIdx.y * p.bo;
  const int wvu = __builtin_amdgcn_readfirstlane(t >> 6);
  const int ntn = (p.Cout + COLS - 1) / COLS, ntk = (p.K + COLS - 1) / COLS;
  int bid = xcd_remap(blockIdx.x, gridDim.x);
  const int tile_k = bid % ntk; bid /= ntk;
  const int tile_n = bid % ntn; bid /= ntn;
  const int split = bid;
  const int n0 = tile_n * COLS, k0 = tile_k * COLS;
  const int mt0 = split * p.mtiles_per_split;
  const int total_mt = (p.M + WM - 1) / WM;
  const int mt1 = min(mt0 + p.mtiles_per_split, total_mt);

  const int cc = t & 15, rb = t >> 4;          // physical chunk / row of this lane's DMA slots (rows rb + 16 i)
  const int cl = cc ^ fsw(rb);                 // logical chunk it fetches (fsw(rb + 16 i) == fsw(rb))
  const int kc = k0 * ES / 16 + cl;
  const bool vk = kc < p.Kc;
  const int pp = vk ? kc / p.cpp : 0, coff = vk ? kc - pp * p.cpp : 0;
  const int ky = pp / p.KW, kx = pp - ky * p.KW;
  const int nc = n0 * ES / 16 + cl;
  const bool vn = nc < p.ncc;
  const bool taps = !(p.KH == 1 && p.KW == 1);
  const char* zp = (const char*)g_zero_page;

  int m[4];
  const char* pd[4];
  const char* px[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    m[i] = mt0 * WM + rb + 16 * i;
    pd[i] = p.dy + ((long)m[i] * p.ldd) * ES + (long)nc * 16;
    px[i] = p.x + (((long)m[i] + (long)(ky - p.pad) * p.Wi + (kx - p.pad)) * p.xrs) * 16 + (long)coff * 16;
  }
  const long dstep = (long)WM * p.ldd * ES, xstep = (long)WM * p.xrs * 16;

  auto stage = [&](int buf) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      bool vmm = m[i] < p.M;
      glds16((vmm && vn) ? pd[i] : zp, &lds[buf][0][(4 * wvu + 16 * i) * 16]);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      bool ok = (m[i] < p.M) & vk;
      if (taps) {                                  // branch-free: every lane does the (cheap) divisions
        unsigned mm = min((unsigned)m[i], (unsigned)(p.M - 1));
        unsigned tq = fdiv(mm, p.dWo);
        unsigned ox = mm - tq * p.Wo;
        unsigned oy = tq - fdiv(tq, p.dHo) * p.Ho;
        ok = ok & ((unsigned)((int)oy - p.pad + ky) < (unsigned)p.Hi) & ((unsigned)((int)ox - p.pad + kx) < (unsigned)p.Wi);
      }
      glds16(ok ? px[i] : zp, &lds[buf][1][(4 * wvu + 16 * i) * 16]);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) { m[i] += WM; pd[i] += dstep; px[i] += xstep; }
  };

  constexpr int WT = COLS / 2;
  constexpr int NT = WT / 32;
  const int wn = wv >> 1, wk = wv & 1;
  f32x16 acc[NT][NT];
#pragma unroll
  for (int a = 0; a < NT; ++a)
#pragma unroll
    for (int b = 0; b < NT; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;

  typename TrFragS<T>::Off offa[NT], offb[NT];
#pragma unroll
  for (int i = 0; i < NT; ++i) {
    offa[i] = TrFragS<T>::prep(wn * WT + i * 32, lane);
    offb[i] = TrFragS<T>::prep(wk * WT + i * 32, lane);
  }

  if (mt0 < mt1) stage(0);
  for (int mt = mt0; mt < mt1; ++mt) {
    const int cur = (mt - mt0) & 1;
    if (mt + 1 < mt1) {
      stage(cur ^ 1);
      asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
    } else {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    __builtin_amdgcn_s_barrier();
#pragma unroll
    for (int ms = 0; ms < WM; ms += TrFragS<T>::MSTEP) {
      u32x4 fa[NT], fb[NT];
#pragma unroll
      for (int i = 0; i < NT; ++i) {
        fa[i] = TrFragS<T>::read(lds[cur][0], ms, offa[i]);
        fb[i] = TrFragS<T>::read(lds[cur][1], ms, offb[i]);
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");     // asm reads are invisible to hipcc's own waitcnt pass
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int a = 0; a < NT; ++a)
#pragma unroll
        for (int b = 0; b < NT; ++b) Mma<T>::step(acc[a][b], fa[a], fb[b]);
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
  }

  const int r = lane & 31, h = lane >> 5;
  if (p.ws) {          // split reduction through the workspace: 16-byte stores in fragment order, 1 KiB per wave instruction
    f32x4* dst = (f32x4*)p.ws + ((long)(split * ntn + tile_n) * ntk + tile_k) * (4 * NT * NT * 4 * 64) + (wv * NT * NT * 4) * 64 + lane;
#pragma unroll
    for (int a = 0; a < NT; ++a)
#pragma unroll
      for (int b = 0; b < NT; ++b)
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4) {
          const f32x4 v = {acc[a][b][4 * g4], acc[a][b][4 * g4 + 1], acc[a][b][4 * g4 + 2], acc[a][b][4 * g4 + 3]};
          dst[((a * NT + b) * 4 + g4) * 64] = v;
        }
    return;
  }
#pragma unroll
  for (int a = 0; a < NT; ++a)
#pragma unroll
    for (int b = 0; b < NT; ++b) {
      int k = k0 + wk * WT + b * 32 + r;
      if (k >= p.K) continue;
#pragma unroll
      for (int g = 0; g < 16; ++g) {
        int n = n0 + wn * WT + a * 32 + (g & 3) + 8 * (g >> 2) + 4 * h;
        if (n >= p.Cout) continue;
        float v = acc[a][b][g] * (p.scale ? p.scale[n] : 1.f);
        long o = (long)n * p.ldo + k;
        if (p.direct == 0) atomicAdd((float*)outp + o, v);
        else if (p.direct == 1) ((float*)outp)[o] = v;
        else Mma<T>::store(outp + o * ES, v);
      }
    }
}

// ------------------------------------------------------------------------------------------------
// Streaming batched TN GEMM for SHORT reductions (the attention pool's per-region products: 56 or 64 reduction rows,
// thousands of regions): out_b[n][k] = sum_m A_b[m][n] B_b[m][k].  One block = one (n-tile, k-tile) column of outputs
// for a RUN of batches: the double-buffered LDS-DMA pipeline of k_conv_wgrad_dma keeps running across batch boundaries
// (the next batch's tile is in flight while this one is reduced and stored), where one-block-per-batch launches paid a
// full global-memory latency per 32 KiB tile.  Same LDS images, swizzle and transposed reads as k_conv_wgrad_dma.
// ------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256, 2) void k_gemm_tn_stream(WgradArgs p, int nbatch, int bpb) {
  constexpr int ES = Mma<T>::ES;
  constexpr int COLS = 256 / ES;
  __shared__ __attribute__((aligned(16))) u32x4 lds[2][2][WM * 16];
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const int wvu = __builtin_amdgcn_readfirstlane(t >> 6);
  const int ntk = (p.K + COLS - 1) / COLS;
  const int tile_k = blockIdx.x % ntk, tile_n = blockIdx.x / ntk;
  const int n0 = tile_n * COLS, k0 = tile_k * COLS;
  const int b0 = blockIdx.y * bpb, nb = min(bpb, nbatch - b0);
  const int nmt = (p.M + WM - 1) / WM;
  const int nit = nb * nmt;

  const int cc = t & 15, rb = t >> 4;
  const int cl = cc ^ fsw(rb);
  const int kc = k0 * ES / 16 + cl, nc = n0 * ES / 16 + cl;
  const bool vk = kc < p.Kc, vn = nc < p.ncc;
  const char* zp = (const char*)g_zero_page;
  int sb = 0, smt = 0;                               // (batch, reduction tile) of the next tile to stage
  auto stage = [&](int buf) {
    const char* db = p.dy + (long)(b0 + sb) * p.bd + (long)nc * 16;
    const char* xb = p.x + (long)(b0 + sb) * p.bx + (long)kc * 16;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int m = smt * WM + rb + 16 * i;
      const bool vm = m < p.M;
      glds16((vm && vn) ? db + ((long)m * p.ldd) * ES : zp, &lds[buf][0][(4 * wvu + 16 * i) * 16]);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int m = smt * WM + rb + 16 * i;
      const bool vm = m < p.M;
      glds16((vm && vk) ? xb + ((long)m * p.xrs) * 16 : zp, &lds[buf][1][(4 * wvu + 16 * i) * 16]);
    }
    if (++smt == nmt) { smt = 0; ++sb; }
  };

  constexpr int WT = COLS / 2;
  constexpr int NT = WT / 32;
  const int wn = wv >> 1, wk = wv & 1;
  f32x16 acc[NT][NT];
#pragma unroll
  for (int a = 0; a < NT; ++a)
#pragma unroll
    for (int b = 0; b < NT; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;
  typename TrFragS<T>::Off offa[NT], offb[NT];
#pragma unroll
  for (int i = 0; i < NT; ++i) {
    offa[i] = TrFragS<T>::prep(wn * WT + i * 32, lane);
    offb[i] = TrFragS<T>::prep(wk * WT + i * 32, lane);
  }
  const int r = lane & 31, h = lane >> 5;

  if (nit > 0) stage(0);
  int cb = 0, cmt = 0;                               // (batch, reduction tile) being reduced
  for (int it = 0; it < nit; ++it) {
    const int cur = it & 1;
    if (it + 1 < nit) {
      stage(cur ^ 1);
      asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
    } else {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    __builtin_amdgcn_s_barrier();
#pragma unroll
    for (int ms = 0; ms < WM; ms += TrFragS<T>::MSTEP) {
      u32x4 fa[NT], fb[NT];
#pragma unroll
      for (int i = 0; i < NT; ++i) {
        fa[i] = TrFragS<T>::read(lds[cur][0], ms, offa[i]);
        fb[i] = TrFragS<T>::read(lds[cur][1], ms, offb[i]);
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int a = 0; a < NT; ++a)
#pragma unroll
        for (int b = 0; b < NT; ++b) Mma<T>::step(acc[a][b], fa[a], fb[b]);
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    if (++cmt == nmt) {                              // batch complete: store its tile (the next batch's DMA is already in flight)
      char* outp = (char*)p.dw + (long)(b0 + cb) * p.bo;
#pragma unroll
      for (int a = 0; a < NT; ++a)
#pragma unroll
        for (int b = 0; b < NT; ++b) {
          const int k = k0 + wk * WT + b * 32 + r;
#pragma unroll
          for (int g = 0; g < 16; ++g) {
            const int n = n0 + wn * WT + a * 32 + (g & 3) + 8 * (g >> 2) + 4 * h;
            if (k < p.K && n < p.Cout) {
              const float v = acc[a][b][g];
              const long o = (long)n * p.ldo + k;
              if (p.direct == 0) atomicAdd((float*)outp + o, v);
              else if (p.direct == 1) ((float*)outp)[o] = v;
              else Mma<T>::store(outp + o * ES, v);
            }
            acc[a][b][g] = 0.f;
          }
        }
      cmt = 0; ++cb;
    }
  }
}

// ------------------------------------------------------------------------------------------------
// Compact streaming TN GEMM for the attention pool's per-region products when the whole reduction is ONE tile
// (M <= 64 rows) and the output is narrow (N <= 64): out_b[n][k] = sum_m A_b[m][n] B_b[m][k], bf16.
// k_gemm_tn_stream spends a 16 KiB LDS image per stage on an A operand of 2-7 KiB and keeps one stage in flight per
// block; these products are pure streaming (2.9 GB per call), so what matters is bytes in flight.  Here a stage is a
// compact A image (64 rows x 128 B) + the B image (64 rows x 256 B) = 24 KiB, three stages form a ring (two in flight,
// counted vmcnt(12)), two blocks fit a CU.  Block = one 128-column k-tile for a run of batches; wave w owns columns
// 32w..32w+31 for all (one or two) 32-row n-tiles.  Both operands are read transposed (ds_read_b64_tr_b16).
// vmcnt counts stores too and retires in issue order, so the wait for stage `it` has to allow for the previous item's
// output stores that sit between the DMAs: N = 8*NG is a template parameter and K % 128 == 0 so that this count (4*NG
// store instructions per wave and item) is a compile-time constant.
// ------------------------------------------------------------------------------------------------
template <int N>
__device__ __forceinline__ void wait_vm() { asm volatile("s_waitcnt vmcnt(%0)" :: "n"(N) : "memory"); }

// MODE 3 (the attention pool's input gradient, cddmsl_attnpool_dx; P = pixels per region): the product's rows are the token
// gradients  dtok[t] = sum_h (p[h][t] dZ[h] + dS[h][t] U[h]),  t = 0 the mean token.  Instead of storing them (and reading them back in
// a second kernel) the epilogue writes the map's gradient directly,  dx[t-1] = dtok[t] + (dtok[0] + g0) / P  for t = 1..P, zeroed where
// bit t-1 of the column's mask word is clear (the pooled map is a ReLU output: its sign bits, one 64-bit word per region and column,
// written by cddmsl_attn_tokens_fwd), and keeps the UNMASKED column sums of dtok[t] (t = 0 includes g0: the query path's gradient of
// the mean token) in registers over the block's run of regions: the positional embedding's gradient, one atomic per element at the end.
// Two more loads per wave and item (g0, mask word), issued in front of the item's stage so that the counted waits stay exact.
template <int NG, int P>
constexpr int tn_small_stores3() {
  int n = 0;
  for (int a = 0; a < (NG + 3) / 4; ++a)
    for (int g = 0; g < 16; ++g) {
      if (a * 4 + (g >> 2) >= NG) continue;
      const int n0 = a * 32 + (g & 3) + 8 * (g >> 2);
      if ((n0 >= 1 && n0 <= P) || (n0 + 4 >= 1 && n0 + 4 <= P)) ++n;
    }
  return n;
}
template <int NG, int MODE, int P = 0>
__global__ __launch_bounds__(256, 2) void k_gemm_tn_small(WgradArgs p, int nbatch, int bpb) {
  constexpr int NTN = (NG + 3) / 4, NSTORE = MODE == 3 ? tn_small_stores3<NG, P>() : 4 * NG, NML = MODE == 3 ? 2 : 0;
  constexpr int STAGE = 8192 + 16384, NST = 3;
  __shared__ __attribute__((aligned(16))) char lds[NST * STAGE];
  const int t = threadIdx.x, lane = t & 63;
  const int wvu = __builtin_amdgcn_readfirstlane(t >> 6);
  const int k0 = blockIdx.x * 128;
  const int b0 = blockIdx.y * bpb, nit = min(bpb, nbatch - b0);
  const char* zp = (const char*)g_zero_page;
  // DMA slots: A image chunk q = i*256 + t -> row q>>3, chunk q&7 (plain); B image chunk q -> row q>>4, slot q&15 (chunk ^= fsw(row))
  const int ar = t >> 3, ac = t & 7;
  const bool va = ac * 8 < p.Cout;
  const int xr = t >> 4, xc = (t & 15) ^ fsw(t >> 4);
  const int kc = (k0 >> 3) + xc;
  const bool vk = kc < p.Kc;
  int sb = 0;
  auto stage = [&](int slot) {
    char* base = lds + slot * STAGE;
    const char* db = p.dy + (long)(b0 + sb) * p.bd + ac * 16;
    const char* xb = p.x + (long)(b0 + sb) * p.bx + (long)kc * 16;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int m = ar + 32 * i;
      glds16((va && m < p.M) ? db + ((long)m * p.ldd) * 2 : zp, base + (i * 256 + wvu * 64) * 16);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int m = xr + 16 * i;
      glds16((vk && m < p.M) ? xb + ((long)m * p.xrs) * 16 : zp, base + 8192 + (i * 256 + wvu * 64) * 16);
    }
    ++sb;
  };
  f32x16 acc[NTN];
#pragma unroll
  for (int a = 0; a < NTN; ++a)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[a][r] = 0.f;
  // transposed-read addresses inside a stage
  const unsigned lbase = (unsigned)(size_t)(__attribute__((address_space(3))) char*)lds;
  unsigned aoff[NTN][2], xoff[2];
  {
    const int g = lane >> 4, li = lane & 15, q = li >> 2, pp = li & 3, hh = g >> 1;
#pragma unroll
    for (int a = 0; a < NTN; ++a) {
      const int col = a * 32 + 16 * (g & 1) + 4 * pp;
      aoff[a][0] = (8 * hh + q) * 128 + col * 2;
      aoff[a][1] = aoff[a][0] + 4 * 128;
    }
    const TrFragS<__bf16>::Off o = TrFragS<__bf16>::prep(wvu * 32, lane);
    xoff[0] = 8192 + o.o0; xoff[1] = 8192 + o.o1;
  }
  const int r = lane & 31, h = lane >> 5;
  f32x16 gacc[MODE == 3 ? NTN : 1];
  if (MODE == 3) {
#pragma unroll
    for (int a = 0; a < NTN; ++a)
#pragma unroll
      for (int g = 0; g < 16; ++g) gacc[a][g] = 0.f;
  }
  if (nit > 0) stage(0);
  if (nit > 1) stage(1);
  // One item.  KIND (compile time): 2 = two more items follow (stage it+2 is issued here), 1 = one more follows, 0 = the last.
  // The three kinds run as three pieces of straight-line code (loop, tail, tail), so that MODE 3's two per-item loads -- plain
  // loads the compiler waits for by itself, counting the DMA instructions issued behind them -- are not merged across paths with
  // different numbers of younger operations (a merged path waits for vmcnt(0), i.e. for the DMAs just issued).
  auto item = [&](int it, auto KIND) {
    constexpr int kind = decltype(KIND)::value;
    const int slot = it % NST;
    float g0v = 0.f;
    u32x2 mbv = {~0u, ~0u};
    if (MODE == 3) {                                 // this item's row vector and mask word: requested BEFORE stage it+2
      // (inline asm + a counted wait below: hipcc's own wait for a plain load issued in front of LDS-DMA instructions is vmcnt(0))
      const long ci = (long)(b0 + it) * p.K + k0 + wvu * 32 + r;
      const char* gp = (const char*)(p.g0 + ci);
      const char* mp = (const char*)(p.mbits + ci);
      asm volatile("global_load_dword %0, %1, off" : "=v"(g0v) : "v"(gp) : "memory");
      asm volatile("global_load_dwordx2 %0, %1, off" : "=v"(mbv) : "v"(mp) : "memory");
    }
    // younger than stage `it`: stage it+1 (6 DMAs), the stores of item it-1, [the two loads above,] stage it+2 (6 DMAs)
    if (kind == 2) {
      stage((it + 2) % NST);
      if (it) wait_vm<12 + NML + NSTORE>(); else wait_vm<12 + NML>();
    } else if (kind == 1) {
      if (it) wait_vm<6 + NML + NSTORE>(); else wait_vm<6 + NML>();
    } else {
      wait_vm<0>();
    }
    __builtin_amdgcn_s_barrier();
    const unsigned sbase = lbase + slot * STAGE;
#define CDDMSL_TRS(DST, A0, A1, IMM)                                                             \
  { u32x2 q0_, q1_;                                                                              \
    asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(q0_) : "v"(A0), "i"(IMM));         \
    asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(q1_) : "v"(A1), "i"(IMM));         \
    DST = u32x4{q0_[0], q0_[1], q1_[0], q1_[1]}; }
    u32x4 fa[NTN][4], fb[4];
    const unsigned x0 = sbase + xoff[0], x1 = sbase + xoff[1];
    CDDMSL_TRS(fb[0], x0, x1, 0) CDDMSL_TRS(fb[1], x0, x1, 4096) CDDMSL_TRS(fb[2], x0, x1, 8192) CDDMSL_TRS(fb[3], x0, x1, 12288)
#pragma unroll
    for (int a = 0; a < NTN; ++a) {
      const unsigned a0 = sbase + aoff[a][0], a1 = sbase + aoff[a][1];
      CDDMSL_TRS(fa[a][0], a0, a1, 0) CDDMSL_TRS(fa[a][1], a0, a1, 2048) CDDMSL_TRS(fa[a][2], a0, a1, 4096) CDDMSL_TRS(fa[a][3], a0, a1, 6144)
    }
#undef CDDMSL_TRS
    if (NTN == 1) asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(fb[0]), "+v"(fb[1]), "+v"(fb[2]), "+v"(fb[3]), "+v"(fa[0][0]), "+v"(fa[0][1]),
                               "+v"(fa[0][2]), "+v"(fa[0][3]) :: "memory");
    else asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(fb[0]), "+v"(fb[1]), "+v"(fb[2]), "+v"(fb[3]), "+v"(fa[0][0]), "+v"(fa[0][1]), "+v"(fa[0][2]),
                      "+v"(fa[0][3]), "+v"(fa[NTN - 1][0]), "+v"(fa[NTN - 1][1]), "+v"(fa[NTN - 1][2]), "+v"(fa[NTN - 1][3]) :: "memory");
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int ms = 0; ms < 4; ++ms)
#pragma unroll
      for (int a = 0; a < NTN; ++a) Mma<__bf16>::step(acc[a], fa[a][ms], fb[ms]);
    __builtin_amdgcn_s_barrier();                    // every wave is done with this slot before the next iteration restages it
    char* outp = (char*)p.dw + (long)(b0 + it) * p.bo;
    const int k = k0 + wvu * 32 + r;
    if (MODE == 3) {
      // the two loads are older than stage it+2's six DMAs (kind 2); the registers are named by the wait so that no use precedes it
      if (kind == 2) asm volatile("s_waitcnt vmcnt(6)" : "+v"(g0v), "+v"(mbv) :: "memory");
      else asm volatile("s_waitcnt vmcnt(0)" : "+v"(g0v), "+v"(mbv) :: "memory");
      // row 0 (the mean token) of this column sits in lane r (< 32), register 0: v_permlane32_swap hands the lower half-wave's values
      // to the upper one (not a DS instruction: a compiler-visible LDS operation here would make hipcc wait for the LDS-DMAs in flight)
      const unsigned a00 = __builtin_bit_cast(unsigned, acc[0][0]);
      const float t0 = __builtin_bit_cast(float, __builtin_amdgcn_permlane32_swap(a00, a00, false, false)[0]) + g0v;
      const float base = t0 * (1.0f / (float)(P > 0 ? P : 1));
      const unsigned mlo = mbv[0], mhi = mbv[1];
#pragma unroll
      for (int a = 0; a < NTN; ++a)
#pragma unroll
        for (int g = 0; g < 16; ++g) {
          const int n0 = a * 32 + (g & 3) + 8 * (g >> 2);
          const bool exists = a * 4 + (g >> 2) < NG;
          const bool lo_ok = n0 >= 1 && n0 <= P, hi_ok = n0 + 4 >= 1 && n0 + 4 <= P;       // (compile-time after unrolling)
          if (exists) {
            const int n = n0 + 4 * h;
            const float v = acc[a][g];
            gacc[a][g] += (n == 0) ? t0 : v;
            if (lo_ok || hi_ok) {
              if (h ? hi_ok : lo_ok) {
                const unsigned word = (n - 1) < 32 ? mlo : mhi;
                const bool keep = (word >> ((n - 1) & 31)) & 1u;
                Mma<__bf16>::store(outp + ((long)(n - 1) * p.ldo + k) * 2, keep ? v + base : 0.f);
              }
            }
          }
          acc[a][g] = 0.f;
        }
      return;
    }
#pragma unroll
    for (int a = 0; a < NTN; ++a)
#pragma unroll
      for (int g = 0; g < 16; ++g) {
        if (a * 4 + (g >> 2) < NG) {                 // rows 8*(4a + g/4) .. +7 exist: exactly NSTORE stores per item
          const int n = a * 32 + (g & 3) + 8 * (g >> 2) + 4 * h;
          const float v = acc[a][g];
          const long o = (long)n * p.ldo + k;
          if (MODE == 0) atomicAdd((float*)outp + o, v);
          else if (MODE == 1) ((float*)outp)[o] = v;
          else Mma<__bf16>::store(outp + o * 2, v);
        }
        acc[a][g] = 0.f;
      }
  };
  {
    int it = 0;
    for (; it + 2 < nit; ++it) item(it, std::integral_constant<int, 2>{});
    if (it + 1 < nit) { item(it, std::integral_constant<int, 1>{}); ++it; }
    if (it < nit) item(it, std::integral_constant<int, 0>{});
  }
  if (MODE == 3 && p.gpos) {
    const int k = k0 + wvu * 32 + r;
#pragma unroll
    for (int a = 0; a < NTN; ++a)
#pragma unroll
      for (int g = 0; g < 16; ++g) {
        const int n = a * 32 + (g & 3) + 8 * (g >> 2) + 4 * h;
        if (a * 4 + (g >> 2) < NG && n <= P) atomicAdd(p.gpos + (long)n * p.K + k, gacc[a][g]);
      }
  }
}

// ------------------------------------------------------------------------------------------------
// wgrad / TN GEMM on the 256x256 ping-pong structure of k_conv_fwd256 (bf16): output tile 256 n x 256 k, reduction
// tiles of 64 m rows, 8 waves (2 over n x 4 over k; 128 n x 64 k per wave), the two wave groups one barrier apart.
// Operands stay row-major in LDS ([64 rows][256 B] images, chunk ^= fsw(row)) and are read transposed
// (ds_read_b64_tr_b16).  A half-tile = one 16 KiB image: dY half h = the 64 columns {wn*128 + h*64 ..} of both wave
// rows, X half j = the 32 columns {wk*64 + j*32 ..} of all four wave columns.  Phases, restaging distance and the
// counted vmcnt are those of k_conv_fwd256.  Sources are buffer-addressed: per-lane offset constant, the m walk in soffset;
// rows past M and out-of-image filter taps set bit 31 of the lane offset (-> zeros).  Tap validity is recomputed per
// reduction tile for the lane's two rows (2 fdiv each) in the phase that stages the first X half.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(512) void k_wgrad256(WgradArgs p) {
  __shared__ __attribute__((aligned(16))) u32x4 lds[2 * 2 * 2 * 64 * 16];   // byte = buf<<16 | ab<<15 | half<<14 | row*256 + slot*16
  const int t = threadIdx.x, lane = t & 63;
#ifdef CDDMSL_TILE_STAMPS
  const unsigned long long ts_entry = __builtin_amdgcn_s_memrealtime();
  unsigned long long ts_loop = ts_entry;
#endif
  p.x += (long)blockIdx.y * p.bx; p.dy += (long)blockIdx.y * p.bd;
  char* outp = (char*)p.dw + (long)blockIdx.y * p.bo;
  const int wvu = __builtin_amdgcn_readfirstlane(t >> 6);
  const int wn = wvu >> 2, wk = wvu & 3;
  const int ntn = p.Cout >> 8, ntk = p.K >> 8;
  int bid = xcd_remap(blockIdx.x, gridDim.x);
  const int tile_k = bid % ntk; bid /= ntk;
  const int tile_n = bid % ntn; bid /= ntn;
  const int n0 = tile_n * 256, k0 = tile_k * 256;
  const int mt0 = bid * p.mtiles_per_split;
  const int nmt = min(p.mtiles_per_split, (p.M + WM - 1) / WM - mt0);
  const bool taps = !(p.KH == 1 && p.KW == 1);

  // ---- staging: thread -> LDS slot (row i*32 + (t>>4), slot t&15), logical chunk cl of that slot
  const int rb = t >> 4, cl = (t & 15) ^ fsw(rb);
  const int gd = (cl >> 3) * 16 + (cl & 7);                 // dY chunk within the 256-column tile (+ 8 per half: immediate)
  const int gx = (cl >> 2) * 8 + (cl & 3);                  // X chunk within the 256-column tile (+ 4 per half: immediate)
  const int kc = (k0 >> 3) + gx;
  const int pp = kc / p.cpp, coff = kc - pp * p.cpp;
  const int ky = pp / p.KW, kx = pp - ky * p.KW;
  unsigned vd[2], vx[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    vd[i] = (unsigned)((i * 32 + rb) * p.ldd * 2 + gd * 16);
    vx[i] = (unsigned)((((i * 32 + rb) + ky * p.Wi + kx) * p.xrs + coff) * 16);
  }
  const __amdgpu_buffer_rsrc_t rd = __builtin_amdgcn_make_buffer_rsrc((void*)(p.dy + ((long)mt0 * WM * p.ldd + n0) * 2), 0, 0x80000000u, 0x00020000);
  const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc((void*)(p.x + ((long)mt0 * WM - p.pad * p.Wi - p.pad) * p.xrs * 16), 0, 0x80000000u, 0x00020000);
  const unsigned dstep = (unsigned)(WM * p.ldd * 2), xstep = (unsigned)(WM * p.xrs * 16);
  const int mrow = mt0 * WM + rb;                            // + T*64 + i*32

  char* const L = (char*)lds;
  auto stageD = [&](auto H, int buf, int T) {                // dY half h of reduction tile T (relative to mt0)
    constexpr int h = decltype(H)::value;
    char* dst = L + (buf << 16) + (h << 14) + wvu * 1024;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const unsigned inv = (mrow + T * WM + i * 32 < p.M) ? 0u : 0x80000000u;
      // the instruction's immediate offset moves BOTH the global and the LDS address: take it back out of the LDS base (M0)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rd, (__attribute__((address_space(3))) void*)(dst + i * 8192 - h * 128), 16,
                                               (int)(vd[i] | inv), (int)(T * dstep), h * 128, 0);
    }
  };
  unsigned xinv[2];
  auto validX = [&](int T) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int m = mrow + T * WM + i * 32;
      bool ok = m < p.M;
      if (taps) {
        const unsigned mm = min((unsigned)m, (unsigned)(p.M - 1));
        const unsigned tq = fdiv(mm, p.dWo);
        const unsigned ox = mm - tq * p.Wo;
        const unsigned oy = tq - fdiv(tq, p.dHo) * p.Ho;
        ok = ok & ((unsigned)((int)oy - p.pad + ky) < (unsigned)p.Hi) & ((unsigned)((int)ox - p.pad + kx) < (unsigned)p.Wi);
      }
      xinv[i] = ok ? 0u : 0x80000000u;
    }
  };
  auto stageX = [&](auto J, int buf, int T) {
    constexpr int j = decltype(J)::value;
    char* dst = L + (buf << 16) + (1 << 15) + (j << 14) + wvu * 1024;
#pragma unroll
    for (int i = 0; i < 2; ++i)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rx, (__attribute__((address_space(3))) void*)(dst + i * 8192 - j * 64), 16,
                                               (int)(vx[i] | xinv[i]), (int)(T * xstep), j * 64, 0);
  };
  using I0 = std::integral_constant<int, 0>;
  using I1 = std::integral_constant<int, 1>;

  f32x16 acc[4][2];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;

  // ---- transposed fragment reads: per-lane byte addresses (absolute LDS), buffer bit toggled by XOR, half / 16-row step as immediates
  const unsigned lbase = (unsigned)(size_t)(__attribute__((address_space(3))) char*)L;
  unsigned adA[2][2], adB[2];
  {
#pragma unroll
    for (int a = 0; a < 2; ++a) {
      const TrFragS<__bf16>::Off o = TrFragS<__bf16>::prep(wn * 64 + a * 32, lane);
      adA[a][0] = lbase + o.o0; adA[a][1] = lbase + o.o1;
    }
    const TrFragS<__bf16>::Off o = TrFragS<__bf16>::prep(wk * 32, lane);
    adB[0] = lbase + (1u << 15) + o.o0; adB[1] = lbase + (1u << 15) + o.o1;
  }
  u32x4 fa0[2][4], fa1[2][4], fb0[4], fb1[4];
#define CDDMSL_TR2(DST, A0, A1, IMM)                                                             \
  { u32x2 q0_, q1_;                                                                              \
    asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(q0_) : "v"(A0), "i"(IMM));         \
    asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(q1_) : "v"(A1), "i"(IMM));         \
    DST = u32x4{q0_[0], q0_[1], q1_[0], q1_[1]}; }
#define CDDMSL_READ_A(HALF, FA)                                                                  \
  _Pragma("unroll") for (int a = 0; a < 2; ++a) {                                                \
    CDDMSL_TR2(FA[a][0], adA[a][0], adA[a][1], ((HALF) << 14) + 0 * 4096)                        \
    CDDMSL_TR2(FA[a][1], adA[a][0], adA[a][1], ((HALF) << 14) + 1 * 4096)                        \
    CDDMSL_TR2(FA[a][2], adA[a][0], adA[a][1], ((HALF) << 14) + 2 * 4096)                        \
    CDDMSL_TR2(FA[a][3], adA[a][0], adA[a][1], ((HALF) << 14) + 3 * 4096) }
#define CDDMSL_READ_B(HALF, FB)                                                                  \
  CDDMSL_TR2(FB[0], adB[0], adB[1], ((HALF) << 14) + 0 * 4096)                                   \
  CDDMSL_TR2(FB[1], adB[0], adB[1], ((HALF) << 14) + 1 * 4096)                                   \
  CDDMSL_TR2(FB[2], adB[0], adB[1], ((HALF) << 14) + 2 * 4096)                                   \
  CDDMSL_TR2(FB[3], adB[0], adB[1], ((HALF) << 14) + 3 * 4096)
#define CDDMSL_FLIP_A() { adA[0][0] ^= 1u << 16; adA[0][1] ^= 1u << 16; adA[1][0] ^= 1u << 16; adA[1][1] ^= 1u << 16; }
#define CDDMSL_FLIP_B() { adB[0] ^= 1u << 16; adB[1] ^= 1u << 16; }
#define CDDMSL_MMA_QUAD(I, J, FA, FB)                                               \
  _Pragma("unroll") for (int ms = 0; ms < 4; ++ms) {                                \
    Mma<__bf16>::step(acc[2 * (I)][J], FA[0][ms], FB[ms]);                          \
    Mma<__bf16>::step(acc[2 * (I) + 1][J], FA[1][ms], FB[ms]);                      \
  }
// The transposed reads are inline asm (see TrFragS): the wait that retires them names the fragments as read-write
// operands, so no MFMA that consumes them can be placed above it; the empty statement after a quadrant's MFMAs names its
// accumulators, so those MFMAs cannot sink below the phase's closing barrier (register-only instructions are otherwise
// free to cross barriers and sched_barrier alike).
#define CDDMSL_WAIT4(F) asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(F[0]), "+v"(F[1]), "+v"(F[2]), "+v"(F[3]) :: "memory");
#define CDDMSL_WAIT8(F) asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(F[0][0]), "+v"(F[0][1]), "+v"(F[0][2]), "+v"(F[0][3]), \
                                     "+v"(F[1][0]), "+v"(F[1][1]), "+v"(F[1][2]), "+v"(F[1][3]) :: "memory");
#define CDDMSL_PHASE_SYNC_IN(WAIT)                                                  \
  __builtin_amdgcn_sched_barrier(0);                                                \
  __builtin_amdgcn_s_barrier();                                                     \
  WAIT                                                                              \
  __builtin_amdgcn_sched_barrier(0);                                                \
  __builtin_amdgcn_s_setprio(1);
#define CDDMSL_PHASE_SYNC_OUT(I, J)                                                 \
  asm volatile("" : "+v"(acc[2 * (I)][J]), "+v"(acc[2 * (I) + 1][J]));              \
  __builtin_amdgcn_s_setprio(0);                                                    \
  __builtin_amdgcn_sched_barrier(0);                                                \
  __builtin_amdgcn_s_barrier();                                                     \
  __builtin_amdgcn_sched_barrier(0);

  if (nmt > 0) {
    // prologue: tile 0 complete, tile 1 without its dY half 1 (staged by phase 1 of tile 0); dY half 0 of tile 0 is read ahead
    validX(0);
    stageD(I0{}, 0, 0); stageD(I1{}, 0, 0); stageX(I0{}, 0, 0); stageX(I1{}, 0, 0);
    if (nmt > 1) {
      validX(1);
      stageD(I0{}, 1, 1); stageX(I0{}, 1, 1); stageX(I1{}, 1, 1);
      asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
    } else {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
    CDDMSL_READ_A(0, fa0)
    CDDMSL_WAIT8(fa0)
    if (wn == 1) __builtin_amdgcn_s_barrier();     // group 1 runs one barrier behind group 0
    __builtin_amdgcn_sched_barrier(0);
#ifdef CDDMSL_TILE_STAMPS
    ts_loop = __builtin_amdgcn_s_memrealtime();
#endif

    for (int kt = 0; kt < nmt; ++kt) {
      const int d = kt & 1;
      const bool more1 = kt + 1 < nmt, more2 = kt + 2 < nmt;
      // phase 1
      CDDMSL_READ_B(0, fb0)
      if (more1) stageD(I1{}, d ^ 1, kt + 1);
      CDDMSL_PHASE_SYNC_IN(CDDMSL_WAIT4(fb0))
      CDDMSL_MMA_QUAD(0, 0, fa0, fb0);
      CDDMSL_PHASE_SYNC_OUT(0, 0)
      // phase 2
      CDDMSL_READ_B(1, fb1)
      CDDMSL_FLIP_B()
      if (more2) { stageD(I0{}, d, kt + 2); validX(kt + 2); }     // (the tap tests of the X stages of phases 3 and 4: this phase has the lighter load part)
      CDDMSL_PHASE_SYNC_IN(CDDMSL_WAIT4(fb1))
      CDDMSL_MMA_QUAD(0, 1, fa0, fb1);
      CDDMSL_PHASE_SYNC_OUT(0, 1)
      // phase 3
      CDDMSL_READ_A(1, fa1)
      CDDMSL_FLIP_A()
      if (more2) {
        stageX(I0{}, d, kt + 2);
        asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
      } else {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      }
      CDDMSL_PHASE_SYNC_IN(CDDMSL_WAIT8(fa1))
      CDDMSL_MMA_QUAD(1, 1, fa1, fb1);
      CDDMSL_PHASE_SYNC_OUT(1, 1)
      // phase 4
      if (more1) { CDDMSL_READ_A(0, fa0) }
      if (more2) stageX(I1{}, d, kt + 2);
      CDDMSL_PHASE_SYNC_IN(CDDMSL_WAIT8(fa0))
      CDDMSL_MMA_QUAD(1, 0, fa1, fb0);
      CDDMSL_PHASE_SYNC_OUT(1, 0)
    }
    if (wn == 0) __builtin_amdgcn_s_barrier();
  }
#undef CDDMSL_TR2
#undef CDDMSL_WAIT4
#undef CDDMSL_WAIT8
#undef CDDMSL_READ_A
#undef CDDMSL_READ_B
#undef CDDMSL_FLIP_A
#undef CDDMSL_FLIP_B
#undef CDDMSL_MMA_QUAD
#undef CDDMSL_PHASE_SYNC_IN
#undef CDDMSL_PHASE_SYNC_OUT

#ifdef CDDMSL_TILE_STAMPS
  const unsigned long long ts_epi = __builtin_amdgcn_s_memrealtime();
#endif
  const int r = lane & 31, h = lane >> 5;
  if (p.ws) {          // split reduction through the workspace (see k_conv_wgrad_dma): 32 x 16 bytes per lane instead of 128 atomics
    store_frags((f32x4*)p.ws + ((long)(bid * ntn + tile_n) * ntk + tile_k) * (8 * 32 * 64) + (wvu * 32) * 64 + lane, acc);
  } else
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      const int k = k0 + wk * 64 + b * 32 + r;
#pragma unroll
      for (int g = 0; g < 16; ++g) {
        const int n = n0 + wn * 128 + a * 32 + (g & 3) + 8 * (g >> 2) + 4 * h;
        const float v = acc[a][b][g] * (p.scale ? p.scale[n] : 1.f);
        const long o = (long)n * p.ldo + k;
        if (p.direct == 0) atomicAdd((float*)outp + o, v);
        else if (p.direct == 1) ((float*)outp)[o] = v;
        else Mma<__bf16>::store(outp + o * 2, v);
      }
    }
#ifdef CDDMSL_TILE_STAMPS
  if (p.tstamps && lane == 0) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    unsigned long long* o = p.tstamps + ((long)blockIdx.x * 8 + wvu) * 4;
    o[0] = ts_entry; o[1] = ts_loop; o[2] = ts_epi; o[3] = __builtin_amdgcn_s_memrealtime();
  }
#endif
}

// ------------------------------------------------------------------------------------------------
// fp8 configuration (BASELINE.json configs[4]): the weight gradient of a "same" convolution on the e4m3 copies of BOTH operands
// (the activation's copy its producer wrote for the forward convolution, the output gradient's copy made for the input-gradient
// convolution), v_mfma_scale_f32_32x32x64_f8f6f4.  Output tile 256 n x 256 k, 8 waves of 128 n x 64 k as in k_wgrad256 (same
// accumulator layout: the same epilogue and k_wgrad_reduce).  Reduction tiles of 64 pixels = ONE MFMA step: an image is
// [64 pixels][256 channels] bytes, 16 KiB, 16-byte chunk c of row r stored at chunk c ^ ((r & 7) << 1); fragments are read with
// ds_read_b64_tr_b8 (tools/tr_b8_probe.hip: per 16 lanes a block of 8 rows x 16 columns of bytes, lane 2q+p supplies row q columns
// 8p.., lane i receives column i) -- lane half h takes pixels 32h..32h+31 of the tile in 4 reads, for both operands alike, which is
// all a dot product needs; a 32-lane half touches 8 rows x 32 contiguous bytes whose chunk pairs the XOR spreads over all 64 banks.
// Loop: a ring of 4 LDS buffers filled by LDS-DMA two tiles ahead (counted vmcnt), ONE barrier per tile, fragment reads issued between
// the MFMAs one half tile ahead (register plan below).  The same loop on bf16 operands (32-pixel tiles, ds_read_b64_tr_b16) was built and
// measured against k_wgrad256's ping-pong phases: 19.3-20.1 vs 17.7 ms per step for the same launches -- the bf16 kernel keeps its phases.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(512) void k_wgrad256_f8(WgradArgs p) {
  __shared__ __attribute__((aligned(16))) u32x4 lds[4 * 2 * 64 * 16];   // byte = ring<<15 | ab<<14 | row*256 + slot*16
  const int t = threadIdx.x, lane = t & 63;
  const int wvu = __builtin_amdgcn_readfirstlane(t >> 6);
  const int wn = wvu >> 2, wk = wvu & 3;
  const int ntn = p.Cout >> 8, ntk = p.K >> 8;
  int bid = xcd_remap(blockIdx.x, gridDim.x);
  const int tile_k = bid % ntk; bid /= ntk;
  const int tile_n = bid % ntn; bid /= ntn;
  const int n0 = tile_n * 256, k0 = tile_k * 256;
  const int mt0 = bid * p.mtiles_per_split;
  const int nmt_real = min(p.mtiles_per_split, (p.M + WM - 1) / WM - mt0);
  const int nmt = (nmt_real + 1) & ~1;                        // an even number of tiles (one straight-line loop body of two): the extra one is all zeros
  const int mlim = min(p.M, (mt0 + nmt_real) * WM);           // rows at or past this are not this block's
  const bool taps = !(p.KH == 1 && p.KW == 1);

  // ---- staging: wave instruction i of a thread fills rows (i*8 + wave)*4 .. +3 of an image, lane -> (row lane>>4, slot lane&15)
  const int rq = lane >> 4, r8 = (wvu & 1) * 4 + rq;
  const int cl = (lane & 15) ^ (r8 << 1);                      // logical chunk of this lane's slot
  const int pp = k0 / p.Cin, coff = (k0 - pp * p.Cin) >> 4;    // the tile's filter tap and first chunk within the pixel (256 | Cin)
  const int ky = pp / p.KW, kx = pp - ky * p.KW;
  unsigned vd[2], vx[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int row = i * 32 + wvu * 4 + rq;
    vd[i] = (unsigned)(row * p.ldd + cl * 16);
    vx[i] = (unsigned)(((row + ky * p.Wi + kx) * p.xrs + coff + cl) * 16);
  }
  const __amdgpu_buffer_rsrc_t rd = __builtin_amdgcn_make_buffer_rsrc((void*)(p.dy + ((long)mt0 * WM * p.ldd + n0)), 0, 0x80000000u, 0x00020000);
  const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc((void*)(p.x + ((long)mt0 * WM - p.pad * p.Wi - p.pad) * p.xrs * 16), 0, 0x80000000u, 0x00020000);
  const unsigned dstep = (unsigned)(WM * p.ldd), xstep = (unsigned)(WM * p.xrs * 16);
  const int mrow = mt0 * WM + wvu * 4 + rq;                    // + T*64 + i*32
  char* const L = (char*)lds;
  auto stage = [&](int T) {
    char* dst = L + ((T & 3) << 15) + wvu * 1024;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int m = mrow + T * WM + i * 32;
      bool ok = m < mlim;
      const unsigned dinv = ok ? 0u : 0x80000000u;
      if (taps) {
        const unsigned mm = min((unsigned)m, (unsigned)(p.M - 1));
        const unsigned tq = fdiv(mm, p.dWo);
        const unsigned ox = mm - tq * p.Wo;
        const unsigned oy = tq - fdiv(tq, p.dHo) * p.Ho;
        ok = ok & ((unsigned)((int)oy - p.pad + ky) < (unsigned)p.Hi) & ((unsigned)((int)ox - p.pad + kx) < (unsigned)p.Wi);
      }
      const unsigned xinv = ok ? 0u : 0x80000000u;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rd, (__attribute__((address_space(3))) void*)(dst + i * 8192), 16,
                                               (int)(vd[i] | dinv), (int)(T * dstep), 0, 0);
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rx, (__attribute__((address_space(3))) void*)(dst + (1 << 14) + i * 8192), 16,
                                               (int)(vx[i] | xinv), (int)(T * xstep), 0, 0);
    }
  };

  f32x16 acc[4][2];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;

  // ---- transposed fragment reads: per-lane byte addresses of read 0 in ring buffer 0 (+ 2048 per read: immediate)
  const unsigned lbase = (unsigned)(size_t)(__attribute__((address_space(3))) char*)L;
  unsigned adA[4], adB[2];
  {
    const int q = (lane & 15) >> 1, gb = (lane >> 4) & 1;
    const unsigned rowb = (unsigned)((32 * (lane >> 5) + q) * 256 + 8 * (lane & 1));
#pragma unroll
    for (int a = 0; a < 4; ++a) adA[a] = lbase + rowb + (unsigned)((((wn * 8 + a * 2 + gb) ^ (q << 1)) & 15) << 4);
#pragma unroll
    for (int b = 0; b < 2; ++b) adB[b] = lbase + (1u << 14) + rowb + (unsigned)((((wk * 4 + b * 2 + gb) ^ (q << 1)) & 15) << 4);
  }
  // Register plan (accumulators 128): dY fragments ONE set of 4 (32 registers), X fragments two sets of 2 (32).  A tile's 8 MFMAs run as
  // two groups: G0 = dY fragments 0,1 (while fragments 2,3 of the same tile are read), G1 = fragments 2,3 (while fragments 0,1 and the
  // X fragments of the NEXT tile are read into the registers G0 has released / the other X set).
  u32x2 fa[4][4], fb[2][2][4];                                 // [fragment][read], [register set][fragment][read]
#define CDDMSL_TR8(DST, AD, R) asm volatile("ds_read_b64_tr_b8 %0, %1 offset:%2" : "=v"(DST) : "v"(AD), "i"((R) * 2048));
#define CDDMSL_TR8x4(F, AD) CDDMSL_TR8(F[0], AD, 0) CDDMSL_TR8(F[1], AD, 1) CDDMSL_TR8(F[2], AD, 2) CDDMSL_TR8(F[3], AD, 3)
// the waits name the registers the retired reads wrote: no MFMA that consumes them (and no copy of them) can be placed above
#define CDDMSL_F8_WAIT_TOP(S)                                                                                                    \
  asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(fa[0][0]), "+v"(fa[0][1]), "+v"(fa[0][2]), "+v"(fa[0][3]),                          \
               "+v"(fa[1][0]), "+v"(fa[1][1]), "+v"(fa[1][2]), "+v"(fa[1][3]),                                                   \
               "+v"(fb[S][0][0]), "+v"(fb[S][0][1]), "+v"(fb[S][0][2]), "+v"(fb[S][0][3]),                                       \
               "+v"(fb[S][1][0]), "+v"(fb[S][1][1]), "+v"(fb[S][1][2]), "+v"(fb[S][1][3]) :: "memory");
#define CDDMSL_F8_WAIT_MID()                                                                                                     \
  asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(fa[2][0]), "+v"(fa[2][1]), "+v"(fa[2][2]), "+v"(fa[2][3]),                          \
               "+v"(fa[3][0]), "+v"(fa[3][1]), "+v"(fa[3][2]), "+v"(fa[3][3]) :: "memory");
  auto mma = [&](auto SC, auto AC, auto BC) {
    constexpr int S = decltype(SC)::value, a = decltype(AC)::value, b = decltype(BC)::value;
    const i32x8 va = {(int)fa[a][0][0], (int)fa[a][0][1], (int)fa[a][1][0], (int)fa[a][1][1],
                      (int)fa[a][2][0], (int)fa[a][2][1], (int)fa[a][3][0], (int)fa[a][3][1]};
    const i32x8 vb = {(int)fb[S][b][0][0], (int)fb[S][b][0][1], (int)fb[S][b][1][0], (int)fb[S][b][1][1],
                      (int)fb[S][b][2][0], (int)fb[S][b][2][1], (int)fb[S][b][3][0], (int)fb[S][b][3][1]};
    acc[a][b] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(va, vb, acc[a][b], 0, 0, 0, 0x7f7f7f7f, 0, 0x7f7f7f7f);
    // an MFMA is a register-only instruction: free to sink below later reads, waits and barriers (it did: all 8 of a tile ended up
    // behind the NEXT tile's barrier).  The empty volatile statement names its result, which orders it among the volatile reads / waits.
    asm volatile("" : "+v"(acc[a][b]));
    __builtin_amdgcn_sched_barrier(0);
  };
  using I0 = std::integral_constant<int, 0>;
  using I1 = std::integral_constant<int, 1>;
  using I2 = std::integral_constant<int, 2>;
  using I3 = std::integral_constant<int, 3>;
  auto body = [&](int kt, auto SC) {
    constexpr int S = decltype(SC)::value, N = S ^ 1;
    using IS = std::integral_constant<int, S>;
    if (kt + 1 < nmt) {                                        // this thread's part of tile kt+1 has landed (tile kt+2 may be in flight)
      if (kt + 2 < nmt) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
      else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_barrier();                              // ... and everyone's; every wave is past its reads of tile kt-1
    __builtin_amdgcn_sched_barrier(0);
    if (kt + 3 < nmt) stage(kt + 3);                           // into the buffer tile kt-1 occupied
    CDDMSL_F8_WAIT_TOP(S)
    __builtin_amdgcn_sched_barrier(0);
    {                                                          // G0, reading dY fragments 2, 3 of this tile
      const unsigned ro = (unsigned)(kt & 3) << 15;
      const unsigned a2 = adA[2] + ro, a3 = adA[3] + ro;
      CDDMSL_TR8x4(fa[2], a2)
      mma(IS{}, I0{}, I0{}); mma(IS{}, I0{}, I1{});
      CDDMSL_TR8x4(fa[3], a3)
      mma(IS{}, I1{}, I0{}); mma(IS{}, I1{}, I1{});
    }
    CDDMSL_F8_WAIT_MID()
    __builtin_amdgcn_sched_barrier(0);
    {                                                          // G1, reading the next tile's dY fragments 0, 1 and X fragments
      // (behind the last tile: a buffer of the ring that holds an older tile -- read and never used)
      const unsigned ro = (unsigned)((kt + 1) & 3) << 15;
      const unsigned a0 = adA[0] + ro, a1 = adA[1] + ro, b0 = adB[0] + ro, b1 = adB[1] + ro;
      // (one fragment per MFMA: issuing all four up front measured slower, 5.14 vs 4.98 ms for the RoI head's three launches)
      CDDMSL_TR8x4(fa[0], a0)
      mma(IS{}, I2{}, I0{});
      CDDMSL_TR8x4(fa[1], a1)
      mma(IS{}, I2{}, I1{});
      CDDMSL_TR8x4(fb[N][0], b0)
      mma(IS{}, I3{}, I0{});
      CDDMSL_TR8x4(fb[N][1], b1)
      mma(IS{}, I3{}, I1{});
    }
  };
  if (nmt > 0) {
    stage(0);
    if (nmt > 1) stage(1);
    if (nmt > 2) stage(2);
    if (nmt > 2) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
    else if (nmt > 1) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
    CDDMSL_TR8x4(fa[0], adA[0]) CDDMSL_TR8x4(fa[1], adA[1]) CDDMSL_TR8x4(fb[0][0], adB[0]) CDDMSL_TR8x4(fb[0][1], adB[1])
    for (int kt = 0; kt < nmt; kt += 2) {
      body(kt, I0{});
      body(kt + 1, I1{});
    }
  }
#undef CDDMSL_TR8x4
#undef CDDMSL_F8_WAIT_TOP
#undef CDDMSL_F8_WAIT_MID
#undef CDDMSL_TR8

  const int r = lane & 31, h = lane >> 5;
  if (p.ws) {          // split reduction through the workspace, accumulators in fragment order (k_wgrad256's layout: k_wgrad_reduce<8, 32>)
    store_frags((f32x4*)p.ws + ((long)(bid * ntn + tile_n) * ntk + tile_k) * (8 * 32 * 64) + (wvu * 32) * 64 + lane, acc);
  } else
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      const int k = k0 + wk * 64 + b * 32 + r;
#pragma unroll
      for (int g = 0; g < 16; ++g) {
        const int n = n0 + wn * 128 + a * 32 + (g & 3) + 8 * (g >> 2) + 4 * h;
        atomicAdd(p.dw + (long)n * p.ldo + k, acc[a][b][g] * (p.scale ? p.scale[n] : 1.f));
      }
    }
}

}  // namespace

// ------------------------------------------------------------------------------------------------
// Split reductions of the weight-gradient kernels without atomics.  64 Ki f32 atomics per 256x256 block take 50-68 us whatever
// the order (tools/tile_stamps.py: 1.3 TB/s of atomic payload chip-wide; 45 % of a layer3 launch of k_wgrad256, ~a third of a
// k_conv_wgrad_dma launch).  With a workspace registered, every block stores its accumulators as they lie in the registers
// (fragment order: 1 KiB per wave instruction), and this kernel sums a tile's splits -- one thread per 16-byte slot -- and adds the
// result, scaled, to dw: plain read-modify-write, nothing else touches dw on the stream meanwhile, and the sum is deterministic.
// WAVES x FR = waves per block x 16-byte slots per lane: 8 x 32 (k_wgrad256: 256x256 tile), 4 x 16 (k_conv_wgrad_dma, bf16: 128x128).
// ------------------------------------------------------------------------------------------------
template <int WAVES, int FR>
__global__ __launch_bounds__(256) void k_wgrad_reduce(const f32x4* ws, float* dw, const float* scale, int ntn, int ntk, int splits, int Cout, int K, int ldo) {
  constexpr int SLOTS = WAVES * FR * 64;                      // 16-byte slots per tile
  constexpr int TN = WAVES == 8 ? 256 : 128;                  // tile edge
  const int tile = blockIdx.x / (SLOTS / 256), q = (blockIdx.x % (SLOTS / 256)) * 256 + threadIdx.x;
  const int tile_k = tile % ntk, tile_n = tile / ntk;
  const long ntiles = (long)ntn * ntk;
  const f32x4* src = ws + (long)tile * SLOTS + q;
  f32x4 sum = {0.f, 0.f, 0.f, 0.f};
  int s = 0;
  for (; s + 4 <= splits; s += 4) {                            // four loads in flight
    const f32x4 a = src[(s + 0) * ntiles * SLOTS], b = src[(s + 1) * ntiles * SLOTS], c = src[(s + 2) * ntiles * SLOTS], d = src[(s + 3) * ntiles * SLOTS];
    sum += (a + b) + (c + d);
  }
  for (; s < splits; ++s) sum += src[s * ntiles * SLOTS];
  const int wv = q / (FR * 64), j = (q / 64) % FR, lane = q & 63, r = lane & 31, h = lane >> 5, g4 = j & 3;
  int a, b, wn, wk;
  if (WAVES == 8) { a = j >> 3; b = (j >> 2) & 1; wn = wv >> 2; wk = wv & 3; }
  else { a = j >> 3; b = (j >> 2) & 1; wn = wv >> 1; wk = wv & 1; }
  const int n = tile_n * TN + wn * (WAVES == 8 ? 128 : 64) + a * 32 + 8 * g4 + 4 * h;
  const int k = tile_k * TN + wk * 64 + b * 32 + r;
  if (k >= K) return;
#pragma unroll
  for (int e = 0; e < 4; ++e)
    if (n + e < Cout) dw[(long)(n + e) * ldo + k] += sum[e] * (scale ? scale[n + e] : 1.f);
}

// whether a split reduction of `blocks` tiles of `tile_floats` goes through the workspace (CDDMSL_WGRAD_WS=0: atomics, for A/B)
static bool use_workspace(long blocks, long tile_floats, void* ws, long ws_bytes) {
  if (env_int("CDDMSL_WGRAD_WS", 1) == 0) return false;
  return ws != nullptr && blocks * tile_floats * 4 <= ws_bytes;
}

// ---- launch, weight gradient
// One of the split kernels, then -- if there is more than one split and the workspace holds every block's accumulators -- the
// reduction of the splits into dw (otherwise the blocks add to dw with atomics).  WAVES x FR as for k_wgrad_reduce.
template <int WAVES, int FR>
static void launch_wgrad_split(void (*kernel)(WgradArgs), WgradArgs& a, const Plan& p, hipStream_t st, void* wsp, long ws_bytes) {
  constexpr int TN = WAVES == 8 ? 256 : 128, SLOTS = WAVES * FR * 64;
  const int ntn = (a.Cout + TN - 1) / TN, ntk = (a.K + TN - 1) / TN;
  const bool ws = p.splits > 1 && use_workspace((long)p.gx, SLOTS * 4, wsp, ws_bytes);
  if (ws) a.ws = (float*)wsp;
  hipLaunchKernelGGL(kernel, dim3(p.gx), dim3(WAVES * 64), 0, st, a);
  if (ws) hipLaunchKernelGGL((k_wgrad_reduce<WAVES, FR>), dim3((unsigned)(ntn * ntk * (SLOTS / 256))), dim3(256), 0, st, (const f32x4*)wsp, a.dw, a.scale,
                             ntn, ntk, p.splits, a.Cout, a.K, a.ldo);
}

void launch_wgrad(WgradArgs& a, const Plan& p, Operand op, hipStream_t st, void* ws, long ws_bytes) {
  switch (p.kernel) {
    case 12: launch_wgrad_split<8, 32>(k_wgrad256_f8, a, p, st, ws, ws_bytes); break;
    case 6: launch_wgrad_split<8, 32>(k_wgrad256, a, p, st, ws, ws_bytes); break;
    case 5:
      if (op == OP_BF16) launch_wgrad_split<4, 16>(k_conv_wgrad_dma<__bf16>, a, p, st, ws, ws_bytes);
      else hipLaunchKernelGGL(k_conv_wgrad_dma<float>, dim3(p.gx), dim3(256), 0, st, a);
      break;
    default:
      if (op == OP_BF16) hipLaunchKernelGGL(k_conv_wgrad<__bf16>, dim3(p.gx), dim3(256), 0, st, a);
      else hipLaunchKernelGGL(k_conv_wgrad<float>, dim3(p.gx), dim3(256), 0, st, a);
  }
}

void launch_gemm_tn(const WgradArgs& p, Operand op, const Plan& pl, int batch, int mode, hipStream_t st) {
  const dim3 grid(pl.gx, pl.gy);
  if (pl.kernel == 9) {
#define CDDMSL_TNS(NG)                                                                                              \
  case NG:                                                                                                          \
    if (mode == 0) hipLaunchKernelGGL((k_gemm_tn_small<NG, 0>), grid, dim3(256), 0, st, p, batch, pl.bpb);      \
    else if (mode == 1) hipLaunchKernelGGL((k_gemm_tn_small<NG, 1>), grid, dim3(256), 0, st, p, batch, pl.bpb); \
    else hipLaunchKernelGGL((k_gemm_tn_small<NG, 2>), grid, dim3(256), 0, st, p, batch, pl.bpb);                \
    break;
    switch (p.Cout / 8) { CDDMSL_TNS(1) CDDMSL_TNS(2) CDDMSL_TNS(3) CDDMSL_TNS(4) CDDMSL_TNS(5) CDDMSL_TNS(6) CDDMSL_TNS(7) CDDMSL_TNS(8) }
#undef CDDMSL_TNS
  } else if (pl.kernel == 7) {
    if (op == OP_BF16) hipLaunchKernelGGL(k_gemm_tn_stream<__bf16>, grid, dim3(256), 0, st, p, batch, pl.bpb);
    else hipLaunchKernelGGL(k_gemm_tn_stream<float>, grid, dim3(256), 0, st, p, batch, pl.bpb);
  } else {
    if (op == OP_BF16) hipLaunchKernelGGL(k_conv_wgrad_dma<__bf16>, grid, dim3(256), 0, st, p);
    else hipLaunchKernelGGL(k_conv_wgrad_dma<float>, grid, dim3(256), 0, st, p);
  }
}

void launch_attnpool_dx(const WgradArgs& p, unsigned gx, unsigned gy, int nbatch, int bpb, hipStream_t st) {
  hipLaunchKernelGGL((k_gemm_tn_small<7, 3, 49>), dim3(gx, gy), dim3(256), 0, st, p, nbatch, bpb);
}
