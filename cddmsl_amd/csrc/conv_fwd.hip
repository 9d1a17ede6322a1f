// Forward convolution / NT GEMM kernels on the 128x128 tile (kernel ids 1 and 2) and the streaming register-weight kernel of the
// few-channel layers (kernel id 8).  Tile geometry and data layout: see gemm_conv.hip.
#include "gemm_common.h"

namespace {

// 8 consecutive elements (16 B of bf16 / 32 B of f32) -> floats
template <typename T> __device__ __forceinline__ void load8(const char* p, float* f);
template <> __device__ __forceinline__ void load8<__bf16>(const char* p, float* f) {
  const u32x4 v = *(const u32x4*)p;
#pragma unroll
  for (int j = 0; j < 4; ++j) { f[2 * j] = bf2f(v[j] & 0xffff); f[2 * j + 1] = bf2f(v[j] >> 16); }
}
template <> __device__ __forceinline__ void load8<float>(const char* p, float* f) {
  const f32x4 a = ((const f32x4*)p)[0], b = ((const f32x4*)p)[1];
  f[0] = a[0]; f[1] = a[1]; f[2] = a[2]; f[3] = a[3]; f[4] = b[0]; f[5] = b[1]; f[6] = b[2]; f[7] = b[3];
}

__device__ __forceinline__ int swz(int row, int chunk) { return row * KCH + (chunk ^ ((row >> 1) & 7)); }

template <typename T>
__global__ __launch_bounds__(256, 2) void k_conv_fwd_reg(ConvArgs p) {
  __shared__ __attribute__((aligned(16))) u32x4 lds[2][BM * KCH];
  const int t = threadIdx.x;
  const int ntn = (p.Cout + BN - 1) / BN;
  const int tile_n = blockIdx.x % ntn, tile_m = blockIdx.x / ntn;
  const int m0 = tile_m * BM, n0 = tile_n * BN;
  const int cc = t & 7, rb = t >> 3;

  // per-thread A-row geometry (4 rows, fixed across K-tiles)
  long pix[4];
  int iy0[4], ix0[4];
  bool vm[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    int m = m0 + rb + 32 * i;
    vm[i] = m < p.M;
    int mm = vm[i] ? m : 0;
    int ox = mm % p.Wo, tq = mm / p.Wo;
    int oy = tq % p.Ho, img = tq / p.Ho;
    int s = p.pool ? 2 * p.stride : p.stride;
    iy0[i] = oy * s - p.pad;
    ix0[i] = ox * s - p.pad;
    pix[i] = ((long)img * p.Hi + iy0[i]) * p.Wi + ix0[i];
  }
  const int nkt = (p.Kc + KCH - 1) / KCH;
  u32x4 ra[4], rbv[4];
  const u32x4 zero = {0u, 0u, 0u, 0u};

  auto gload = [&](int kt) {
    int kc = kt * KCH + cc;
    bool vk = kc < p.Kc;
    int pp = vk ? kc / p.cpp : 0;
    int coff = vk ? kc - pp * p.cpp : 0;
    int ky = pp / p.KW, kx = pp - ky * p.KW;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      int iy = iy0[i] + ky, ix = ix0[i] + kx;
      if (!p.pool) {
        bool ok = vk && vm[i] && iy >= 0 && iy < p.Hi && ix >= 0 && ix < p.Wi;
        const u32x4* src = (const u32x4*)(p.x + ((pix[i] + (long)ky * p.Wi + kx) * p.cpp + coff) * 16);
        ra[i] = ok ? *src : zero;
      } else {  // 1x1 conv over a 2x2 average-pooled input (floor semantics: Ho = Hi/2)
        bool ok = vk && vm[i];
        if (ok) {
          const char* b0 = p.x + (pix[i] * p.cpp + coff) * 16;
          long rs = (long)p.Wi * p.cpp * 16, cs = (long)p.cpp * 16;
          ra[i] = avg4<T>(*(const u32x4*)b0, *(const u32x4*)(b0 + cs), *(const u32x4*)(b0 + rs), *(const u32x4*)(b0 + rs + cs));
        } else ra[i] = zero;
      }
      int n = n0 + rb + 32 * i;
      bool okb = vk && n < p.Cout;
      rbv[i] = okb ? *(const u32x4*)(p.w + ((long)n * p.Kc + kc) * 16) : zero;
    }
  };

  f32x16 acc[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;

  const int lane = t & 63, wv = t >> 6;
  const int wm = wv >> 1, wn = wv & 1;
  const int r = lane & 31, h = lane >> 5;

  gload(0);
  for (int kt = 0; kt < nkt; ++kt) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      int row = rb + 32 * i;
      lds[0][swz(row, cc)] = ra[i];
      lds[1][swz(row, cc)] = rbv[i];
    }
    __syncthreads();
    if (kt + 1 < nkt) gload(kt + 1);  // next tile's HBM loads fly under this tile's MFMAs
#pragma unroll
    for (int ks = 0; ks < KCH / 2; ++ks) {
      u32x4 fa[2], fb[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        fa[i] = lds[0][swz(wm * 64 + i * 32 + r, 2 * ks + h)];
        fb[i] = lds[1][swz(wn * 64 + i * 32 + r, 2 * ks + h)];
      }
#pragma unroll
      for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) Mma<T>::step(acc[a][b], fa[a], fb[b]);
    }
    __syncthreads();
  }

  // ---------------------------------------------------------------------------------------------
  // epilogue.  C/D map of the 32x32 MFMA: col = lane&31 (n), row = (reg&3) + 8*(reg>>2) + 4*(lane>>5) (m).
  // Vector path (all leading dims multiples of 8): each wave transposes its accumulators through LDS
  // (32 rows x 64 cols f32 per pass, 32-byte column groups XOR-swizzled by row) so that every lane owns
  // 8 consecutive channels of one pixel: residual / mask are read and y is written 16-32 B per lane,
  // whole 128-B lines per 8 lanes -- the scalar path issued 64 two-byte stores per lane instead.
  const bool vec_ok = (p.Cout % 8 == 0) && (p.ldy % 8 == 0) && (!p.residual || p.ldr % 8 == 0) && (!p.relu_mask || p.ldm % 8 == 0);
  if (vec_ok) {
    float* ep = (float*)&lds[0][0] + wv * 2048;      // 8 KB per wave; the K-loop's last barrier already passed
    const int cg = lane & 7, rr = lane >> 3;
    const int n = n0 + wn * 64 + cg * 8;
    float sc[8], bi[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      sc[j] = (p.scale && n + j < p.Cout) ? p.scale[n + j] : 1.f;
      bi[j] = (p.bias && n + j < p.Cout) ? p.bias[n + j] : 0.f;
    }
#pragma unroll
    for (int a = 0; a < 2; ++a) {
      __syncthreads();
#pragma unroll
      for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int g = 0; g < 16; ++g) {
          int row = (g & 3) + 8 * (g >> 2) + 4 * h, col = b * 32 + r;
          ep[row * 64 + ((((col >> 3) ^ (row & 7)) << 3) | (col & 7))] = acc[a][b][g];
        }
      __syncthreads();
      if (n < p.Cout) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          int row = rr + 8 * i;
          int m = m0 + wm * 64 + a * 32 + row;
          if (m >= p.M) continue;
          const f32x4* src = (const f32x4*)(ep + row * 64 + ((cg ^ (row & 7)) << 3));
          f32x4 v0 = src[0], v1 = src[1];
          float v[8] = {v0[0], v0[1], v0[2], v0[3], v1[0], v1[1], v1[2], v1[3]};
#pragma unroll
          for (int j = 0; j < 8; ++j) v[j] = affine<T>(v[j], sc[j], bi[j]);
          if (p.residual) {
            float rv[8];
            load8<T>(p.residual + ((long)m * p.ldr + n) * Mma<T>::ES, rv);
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] += rv[j];
          }
          if (p.relu) {
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = fmaxf(v[j], 0.f);
          }
          if (p.relu_mask) {
            float mv[8];
            load8<T>(p.relu_mask + ((long)m * p.ldm + n) * Mma<T>::ES, mv);
#pragma unroll
            for (int j = 0; j < 8; ++j) if (!(mv[j] > 0.f)) v[j] = 0.f;
          }
          if (p.out_f32 || Mma<T>::ES == 4) {
            f32x4* dst = (f32x4*)(p.y + ((long)m * p.ldy + n) * 4);
            f32x4 o0 = {v[0], v[1], v[2], v[3]}, o1 = {v[4], v[5], v[6], v[7]};
            dst[0] = o0; dst[1] = o1;
          } else {
            u32x4 o = {pack2bf(v[0], v[1]), pack2bf(v[2], v[3]), pack2bf(v[4], v[5]), pack2bf(v[6], v[7])};
            *(u32x4*)(p.y + ((long)m * p.ldy + n) * 2) = o;
          }
        }
      }
    }
    return;
  }
#pragma unroll
  for (int b = 0; b < 2; ++b) {
    int n = n0 + wn * 64 + b * 32 + r;
    if (n >= p.Cout) continue;
    float sc = p.scale ? p.scale[n] : 1.f;
    float bi = p.bias ? p.bias[n] : 0.f;
#pragma unroll
    for (int a = 0; a < 2; ++a) {
#pragma unroll
      for (int g = 0; g < 16; ++g) {
        int m = m0 + wm * 64 + a * 32 + (g & 3) + 8 * (g >> 2) + 4 * h;
        if (m >= p.M) continue;
        float v = affine<T>(acc[a][b][g], sc, bi);
        if (p.residual) v += Mma<T>::load(p.residual + ((long)m * p.ldr + n) * Mma<T>::ES);
        if (p.relu) v = fmaxf(v, 0.f);
        if (p.relu_mask && !(Mma<T>::load(p.relu_mask + ((long)m * p.ldm + n) * Mma<T>::ES) > 0.f)) v = 0.f;
        if (p.out_f32) *(float*)(p.y + ((long)m * p.ldy + n) * 4) = v;
        else Mma<T>::store(p.y + ((long)m * p.ldy + n) * Mma<T>::ES, v);
      }
    }
  }
}

// LDS-DMA variant (pool == 0): A and B tiles go global -> LDS directly (global_load_lds_dwordx4, 1 KiB per wave
// instruction = 8 rows x 128 B), double-buffered, with a counted vmcnt so the next tile's 8 DMAs per thread stay in
// flight across the barrier.  The VGPR -> LDS write path (ds_write_b128 ~13 cycles per wave-instruction) was the
// bottleneck of the register-staged loop at two blocks per CU.  LDS destination is lane-linear, so the XOR swizzle
// is applied to the per-lane SOURCE chunk; out-of-image / tail lanes read a 16-byte zero page.

// row of the 2x2-average-pooled tensor that output pixel m falls into (res_pool), or -1 on an odd size's last row / column
__device__ __forceinline__ long pooled_row(const ConvArgs& p, int m) {
  const unsigned tq = fdiv((unsigned)m, p.dWo), ox = m - tq * p.Wo;
  const unsigned img = fdiv(tq, p.dHo), oy = tq - img * p.Ho;
  const unsigned hp = p.Ho >> 1, wp = p.Wo >> 1;
  return ((oy >> 1) < hp && (ox >> 1) < wp) ? ((long)img * hp + (oy >> 1)) * wp + (ox >> 1) : -1L;
}

template <typename T>
__global__ __launch_bounds__(256, 2) void k_conv_fwd(ConvArgs p) {
  __shared__ __attribute__((aligned(16))) u32x4 lds[2][2][BM * KCH];   // [buffer][A|B]
  const int t = threadIdx.x;
  p.x += (long)blockIdx.y * p.bx; p.w += (long)blockIdx.y * p.bw; p.y += (long)blockIdx.y * p.by;   // batched GEMM
  const int wvu = __builtin_amdgcn_readfirstlane(t >> 6);     // wave index in an SGPR: LDS-DMA bases become scalar
  const int ntn = (p.Cout + BN - 1) / BN;
  const int lbid = xcd_remap(blockIdx.x, gridDim.x);
  const int tile_n = lbid % ntn, tile_m = lbid / ntn;
  const int m0 = tile_m * BM, n0 = tile_n * BN;
  const int cc = t & 7, rb = t >> 3;
  const int cl = cc ^ ((rb >> 1) & 7);        // logical K chunk this lane fetches (rows rb+32i share (row>>1)&7)

  // per-thread row geometry, fixed across K-tiles: byte offset of the (ky=kx=0) tap of each of the 4 rows
  long rowoff[4], wrow[4];
  int iy0[4], ix0[4];
  bool vm[4], vn[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    int m = m0 + rb + 32 * i;
    vm[i] = m < p.M;
    unsigned mm = vm[i] ? m : 0;
    unsigned tq = fdiv(mm, p.dWo), ox = mm - tq * p.Wo;
    unsigned img = fdiv(tq, p.dHo), oy = tq - img * p.Ho;
    iy0[i] = (int)oy * p.stride - p.pad;
    ix0[i] = (int)ox * p.stride - p.pad;
    rowoff[i] = ((((long)img * p.Hi + iy0[i]) * p.Wi + ix0[i]) * p.xrs) * 16;
    int n = n0 + rb + 32 * i;
    vn[i] = n < p.Cout;
    wrow[i] = (long)(vn[i] ? n : 0) * p.wrs * 16;
  }
  const int nkt = (p.Kc + KCH - 1) / KCH;
  const char* zp = (const char*)g_zero_page;
  const bool taps = !(p.KH == 1 && p.KW == 1 && p.pad == 0);   // 1x1 / linear: every tap is inside the image
  // running K position of this lane's logical chunk: kc -> (ky, kx, coff); advanced by KCH per tile without divisions
  int kc = cl;
  int pp0 = (int)fdiv((unsigned)kc, p.dcpp);
  int coff = kc - pp0 * p.cpp;
  int ky = (int)fdiv((unsigned)pp0, p.dKW), kx = pp0 - ky * p.KW;

  // Fast path (cpp % 8 == 0, i.e. a K-tile never straddles two filter taps -- every layer past the stem): per-row source
  // pointers are kept in registers and advanced by 128 B per tile (2 VALU each); tap validity / base addresses are
  // recomputed only when the (wave-uniform) tap changes.  The general path recomputes everything per tile.
  const bool fast = (p.cpp & 7) == 0;
  const char* pa[4];
  const char* pb[4];
  int inca[4], incb[4];
  int tiles_left_in_tap = 0;                    // K-tiles before (ky,kx) advances (fast path)
  auto retap = [&]() {                          // (re)build the A pointers for the current (ky, kx, coff)
    const int delta = ((ky * p.Wi + kx) * p.xrs + coff) * 16;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      bool ok = vm[i];
      if (taps) {
        int iy = iy0[i] + ky, ix = ix0[i] + kx;
        ok = ok && iy >= 0 && iy < p.Hi && ix >= 0 && ix < p.Wi;
      }
      pa[i] = ok ? p.x + rowoff[i] + delta : zp;
      inca[i] = ok ? KCH * 16 : 0;
    }
  };
  if (fast) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      pb[i] = vn[i] ? p.w + wrow[i] + (long)kc * 16 : zp;
      incb[i] = vn[i] ? KCH * 16 : 0;
    }
    retap();
    tiles_left_in_tap = p.cpp >> 3;
  }

  auto stage = [&](int buf) {
    if (fast) {
#pragma unroll
      for (int i = 0; i < 4; ++i) glds16(pa[i], &lds[buf][0][(8 * wvu + 32 * i) * KCH]);
#pragma unroll
      for (int i = 0; i < 4; ++i) glds16(pb[i], &lds[buf][1][(8 * wvu + 32 * i) * KCH]);
#pragma unroll
      for (int i = 0; i < 4; ++i) pb[i] += incb[i];
      if (--tiles_left_in_tap == 0) {          // wave-uniform: next tile starts a new filter tap
        tiles_left_in_tap = p.cpp >> 3;
        coff = cl;
        if (++kx == p.KW) { kx = 0; ++ky; }
        retap();
      } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) pa[i] += inca[i];
      }
      return;
    }
    const bool vk = kc < p.Kc;
    const int delta = ((ky * p.Wi + kx) * p.xrs + coff) * 16;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      bool ok = vk && vm[i];
      if (taps) {
        int iy = iy0[i] + ky, ix = ix0[i] + kx;
        ok = ok && iy >= 0 && iy < p.Hi && ix >= 0 && ix < p.Wi;
      }
      const char* src = ok ? p.x + rowoff[i] + delta : zp;
      glds16(src, &lds[buf][0][(8 * wvu + 32 * i) * KCH]);      // wave-uniform base; lane l lands at +16*l
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const char* src = (vk && vn[i]) ? p.w + wrow[i] + (long)kc * 16 : zp;
      glds16(src, &lds[buf][1][(8 * wvu + 32 * i) * KCH]);
    }
    kc += KCH;
    coff += KCH;
    while (coff >= p.cpp) {
      coff -= p.cpp;
      if (++kx == p.KW) { kx = 0; ++ky; }
    }
  };

  f32x16 acc[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;

  const int lane = t & 63, wv = t >> 6;
  const int wm = wv >> 1, wn = wv & 1;
  const int r = lane & 31, h = lane >> 5;

  // Epilogue operands (residual, ReLU mask) are fetched NOW, under the whole K loop, instead of inside the epilogue where
  // their HBM latency (~2 us per pass) was fully exposed on the small-K / wide-N layers (conv3 + residual, dgrad + mask).
  const bool vec_ok = (p.Cout % 8 == 0) && (p.ldy % 8 == 0) && (!p.residual || p.ldr % 8 == 0) && (!p.relu_mask || p.ldm % 8 == 0);
  constexpr bool PRE = Mma<T>::ES == 2;
  u32x4 rres[2][4], rmsk[2][4];
  const bool rf32 = PRE && p.res_f32;             // f32 residual rows on the bf16 kernel: read in the epilogue
  if (PRE && vec_ok && ((p.residual && !rf32) || p.relu_mask)) {
    const int n = n0 + wn * 64 + (lane & 7) * 8;
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        int m = m0 + wm * 64 + a * 32 + (lane >> 3) + 8 * i;
        bool ok = m < p.M && n < p.Cout;
        const u32x4 z = {0u, 0u, 0u, 0u};
        if (p.res_pool) {
          const long po = pooled_row(p, m);
          rres[a][i] = (ok && po >= 0) ? *(const u32x4*)(p.residual + (po * p.ldr + n) * 2) : z;
        } else
        rres[a][i] = (ok && p.residual && !rf32) ? *(const u32x4*)(p.residual + ((long)m * p.ldr + n) * 2) : z;
        rmsk[a][i] = (ok && p.relu_mask) ? *(const u32x4*)(p.relu_mask + ((long)m * p.ldm + n) * 2) : z;
      }
  }

  stage(0);
  for (int kt = 0; kt < nkt; ++kt) {
    const int cur = kt & 1;
    if (kt + 1 < nkt) {
      stage(cur ^ 1);
      asm volatile("s_waitcnt vmcnt(8)" ::: "memory");   // this tile's 8 DMAs done; the next tile's 8 stay in flight
    } else {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    __builtin_amdgcn_s_barrier();
    // fragments of k-step ks+1 are read while the MFMAs of k-step ks run (two named register sets, static indices)
    u32x4 fa[2][2], fb[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      fa[0][i] = lds[cur][0][swz(wm * 64 + i * 32 + r, h)];
      fb[0][i] = lds[cur][1][swz(wn * 64 + i * 32 + r, h)];
    }
#pragma unroll
    for (int ks = 0; ks < KCH / 2; ++ks) {
      if (ks + 1 < KCH / 2) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          fa[(ks + 1) & 1][i] = lds[cur][0][swz(wm * 64 + i * 32 + r, 2 * (ks + 1) + h)];
          fb[(ks + 1) & 1][i] = lds[cur][1][swz(wn * 64 + i * 32 + r, 2 * (ks + 1) + h)];
        }
      }
#pragma unroll
      for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) Mma<T>::step(acc[a][b], fa[ks & 1][a], fb[ks & 1][b]);
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();                          // everyone is done reading buffer `cur`
  }

  // ---------------------------------------------------------------------------------------------
  // epilogue.  C/D map of the 32x32 MFMA: col = lane&31 (n), row = (reg&3) + 8*(reg>>2) + 4*(lane>>5) (m).
  // Vector path (all leading dims multiples of 8): each wave transposes its accumulators through LDS
  // (32 rows x 64 cols f32 per pass, 32-byte column groups XOR-swizzled by row) so that every lane owns
  // 8 consecutive channels of one pixel: residual / mask are read and y is written 16-32 B per lane,
  // whole 128-B lines per 8 lanes -- the scalar path issued 64 two-byte stores per lane instead.
  if (vec_ok) {
    float* ep = (float*)&lds[0][0][0] + wv * 2048;      // 8 KB per wave; the K-loop's last barrier already passed
    const int cg = lane & 7, rr = lane >> 3;
    const int n = n0 + wn * 64 + cg * 8;
    float sc[8], bi[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      sc[j] = (p.scale && n + j < p.Cout) ? p.scale[n + j] : 1.f;
      bi[j] = (p.bias && n + j < p.Cout) ? p.bias[n + j] : 0.f;
    }
#pragma unroll
    for (int a = 0; a < 2; ++a) {
      __syncthreads();
#pragma unroll
      for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int g = 0; g < 16; ++g) {
          int row = (g & 3) + 8 * (g >> 2) + 4 * h, col = b * 32 + r;
          ep[row * 64 + ((((col >> 3) ^ (row & 7)) << 3) | (col & 7))] = acc[a][b][g];
        }
      __syncthreads();
      if (n < p.Cout) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          int row = rr + 8 * i;
          int m = m0 + wm * 64 + a * 32 + row;
          if (m >= p.M) continue;
          const f32x4* src = (const f32x4*)(ep + row * 64 + ((cg ^ (row & 7)) << 3));
          f32x4 v0 = src[0], v1 = src[1];
          float v[8] = {v0[0], v0[1], v0[2], v0[3], v1[0], v1[1], v1[2], v1[3]};
#pragma unroll
          for (int j = 0; j < 8; ++j) v[j] = affine<T>(v[j], sc[j], bi[j]);
          if (p.residual) {
            float rv[8];
            if (rf32) load8<float>(p.residual + ((long)m * p.ldr + n) * 4, rv);
            else if (PRE) {
#pragma unroll
              for (int j = 0; j < 4; ++j) { rv[2 * j] = bf2f(rres[a][i][j] & 0xffff); rv[2 * j + 1] = bf2f(rres[a][i][j] >> 16); }
            } else if (p.res_pool) {
              const long po = pooled_row(p, m);
#pragma unroll
              for (int j = 0; j < 8; ++j) rv[j] = 0.f;
              if (po >= 0) load8<T>(p.residual + (po * p.ldr + n) * Mma<T>::ES, rv);
            } else load8<T>(p.residual + ((long)m * p.ldr + n) * Mma<T>::ES, rv);
            if (p.res_pool) {
#pragma unroll
              for (int j = 0; j < 8; ++j) rv[j] *= 0.25f;
            }
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] += rv[j];
          }
          if (p.relu) {
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = fmaxf(v[j], 0.f);
          }
          if (p.relu_mask) {
            float mv[8];
            if (PRE) {
#pragma unroll
              for (int j = 0; j < 4; ++j) { mv[2 * j] = bf2f(rmsk[a][i][j] & 0xffff); mv[2 * j + 1] = bf2f(rmsk[a][i][j] >> 16); }
            } else load8<T>(p.relu_mask + ((long)m * p.ldm + n) * Mma<T>::ES, mv);
#pragma unroll
            for (int j = 0; j < 8; ++j) if (!(mv[j] > 0.f)) v[j] = 0.f;
          }
          if (p.out_f32 || Mma<T>::ES == 4) {
            f32x4* dst = (f32x4*)(p.y + ((long)m * p.ldy + n) * 4);
            f32x4 o0 = {v[0], v[1], v[2], v[3]}, o1 = {v[4], v[5], v[6], v[7]};
            dst[0] = o0; dst[1] = o1;
          } else {
            u32x4 o = {pack2bf(v[0], v[1]), pack2bf(v[2], v[3]), pack2bf(v[4], v[5]), pack2bf(v[6], v[7])};
            *(u32x4*)(p.y + ((long)m * p.ldy + n) * 2) = o;
          }
        }
      }
    }
    return;
  }
#pragma unroll
  for (int b = 0; b < 2; ++b) {
    int n = n0 + wn * 64 + b * 32 + r;
    if (n >= p.Cout) continue;
    float sc = p.scale ? p.scale[n] : 1.f;
    float bi = p.bias ? p.bias[n] : 0.f;
#pragma unroll
    for (int a = 0; a < 2; ++a) {
#pragma unroll
      for (int g = 0; g < 16; ++g) {
        int m = m0 + wm * 64 + a * 32 + (g & 3) + 8 * (g >> 2) + 4 * h;
        if (m >= p.M) continue;
        float v = affine<T>(acc[a][b][g], sc, bi);
        if (p.residual) v += Mma<T>::load(p.residual + ((long)m * p.ldr + n) * Mma<T>::ES);
        if (p.relu) v = fmaxf(v, 0.f);
        if (p.relu_mask && !(Mma<T>::load(p.relu_mask + ((long)m * p.ldm + n) * Mma<T>::ES) > 0.f)) v = 0.f;
        if (p.out_f32) *(float*)(p.y + ((long)m * p.ldy + n) * 4) = v;
        else Mma<T>::store(p.y + ((long)m * p.ldy + n) * Mma<T>::ES, v);
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------
// 3x3 convolutions with FEW input channels (the CLIP stem: 3(->8 padded)->32 stride 2, 32->32, 32->64; one or four
// 16-byte chunks per pixel), pad 1, FrozenBN + ReLU epilogue.  These layers are pure streaming work: K = 72 or 288,
// N = 32 or 64, M = millions of pixels.  On the tile kernel a block ran 2-5 K-tiles behind one DMA latency each and
// reached ~1 TB/s; here NOTHING goes through LDS: the whole weight matrix lives in registers as MFMA B fragments
// (<= 18 k-steps x NT tiles), each wave walks 32-pixel tiles with a grid stride, and a lane's A fragment of a k-step is
// ONE 16-byte global load (8 consecutive channels of one filter tap of its pixel; the 9 taps of neighbouring pixels hit
// L1/L2).  All loads of a tile are issued before its MFMAs.  Output: lanes = consecutive channels (64 contiguous bytes
// per pixel and tile).  Same accumulation order as k_conv_fwd (chunk pairs in K order) -> bit-identical results.
// ------------------------------------------------------------------------------------------------
//
// POOL (bf16, the ost_ok path only): the launch writes AvgPool2d(2) of its result and the full-resolution map never reaches memory.  A
// tile is then 8 POOLED pixels: tile row r stands for pixel (2 poy + ((r >> 1) & 1), 2 pox + (r & 1)) of pooled pixel tile * 8 + (r >> 2), so
// accumulator registers 4k .. 4k+3 of a lane are the 2x2 window of pooled pixel 2k + hh in k_avgpool2_fwd's order; the four values are
// rounded to bf16 as the unfused launch stores them, averaged in that kernel's order and rounded once more: bit-identical to the two
// launches.  An odd last row / column is never computed.  The pooled tile is 8 rows x NT * 64 bytes (NT = 2: one 1 KiB store).
template <typename T, int CPP, int NT, int NTAP = 9, bool POOL = false>     // NTAP = 1: the same streaming structure for a 1x1 layer with 32 / 64 output channels
__global__ __launch_bounds__(256) void k_conv3x3_small(ConvArgs p) {
  static_assert(!POOL || (Mma<T>::ES == 2 && NT == 2 && NTAP == 9 && CPP > 1), "pooled output: the bf16 3x3 instantiation with 64 output channels");
  constexpr int KC = NTAP * CPP, KS = (KC + 1) / 2;    // 16-byte chunks of a weight row; k-steps of two chunks
  constexpr int PAD = NTAP == 9 ? 1 : 0;
  constexpr int ES = Mma<T>::ES;
  const int lane = threadIdx.x & 63, r = lane & 31, hh = lane >> 5;
  // weights as MFMA B fragments: fragment (nt, ks) of a lane = chunk 2ks+hh of weight row nt*32 + r (zero past the row end).
  // One chunk per pixel (K = 72): 5 k-steps, kept in registers.  Four chunks per pixel (K = 288): 18 k-steps x NT tiles would
  // take up to 144 VGPRs and leave one wave per SIMD -- they sit in LDS in fragment order (lane-linear 16-byte reads).
  constexpr bool WLDS = CPP > 1;
  __shared__ __attribute__((aligned(16))) u32x4 wl[WLDS ? NT * KS * 64 : 1];
  u32x4 bw[WLDS ? 1 : NT][WLDS ? 1 : KS];
  {
    const int wv = threadIdx.x >> 6;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        if (WLDS && ((nt * KS + ks) & 3) != wv) continue;       // the four waves fill the image cooperatively
        const int q = 2 * ks + hh;
        u32x4 v = {0u, 0u, 0u, 0u};
        if (q < KC) v = *(const u32x4*)(p.w + ((long)(nt * 32 + r) * KC + q) * 16);
        if (WLDS) wl[(nt * KS + ks) * 64 + lane] = v;
        else bw[WLDS ? 0 : nt][WLDS ? 0 : ks] = v;
      }
    if (WLDS) __syncthreads();
  }
  float sc[NT], bi[NT];
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) { sc[nt] = p.scale ? p.scale[nt * 32 + r] : 1.f; bi[nt] = p.bias ? p.bias[nt * 32 + r] : 0.f; }
  const int wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, nwaves = (gridDim.x * blockDim.x) >> 6;
  const int Hp = p.Ho >> 1, Wp = p.Wo >> 1, Mp = POOL ? p.Nimg * Hp * Wp : 0;     // POOL: the pooled map, Mp rows
  const int ntiles = POOL ? (Mp + 7) >> 3 : (p.M + 31) >> 5;
  // Addressing.  An ablation of this kernel (round 2: loads, MFMAs and stores switched off one at a time) showed 40-50 % of its time
  // to be the per-tile INDEX ARITHMETIC alone -- per k-step a tap select, two range tests and a 64-bit address, per output element a
  // 64-bit address and a row test: ~530 vector-ALU instructions per 32-pixel tile against 36-72 MFMAs.  Now: buffer addressing
  // (32-bit lane offset from the tensor base; the k-step's tap / chunk offset is wave-uniform and rides in soffset), tap validity as
  // a 9-bit mask per tile whose bit sets bit 31 of the lane offset (out of range -> zeros), and buffer stores with the row offset in
  // soffset; rows past M fall outside num_records.  (One chunk per pixel, CPP = 1: a k-step's two chunks straddle taps -- lane halves
  // differ by more than a constant -- and that instantiation keeps its direct loads.)
  // (base one row and one pixel BEFORE the tensor: the lane offset of a pixel's tap (0,0) is then never negative -- the range check
  // sees the lane offset alone -- and the bytes in front of the tensor are only ever addressed by taps the mask removes)
  const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc((void*)(p.x - (long)(p.Wi + 1) * (CPP * 16)), 0, 0x7fffffff, 0x00020000);
  const long ybytes = (long)(POOL ? Mp : p.M) * p.ldy * ES, mbytes = (long)p.M * p.ldm * ES;
  const __amdgpu_buffer_rsrc_t ry = __builtin_amdgcn_make_buffer_rsrc((void*)p.y, 0, (int)(ybytes > 0x7fffffffL ? 0x7fffffffL : ybytes), 0x00020000);
  const __amdgpu_buffer_rsrc_t rm = __builtin_amdgcn_make_buffer_rsrc((void*)p.relu_mask, 0, p.relu_mask ? (int)(mbytes > 0x7fffffffL ? 0x7fffffffL : mbytes) : 0, 0x00020000);
  const float relu_floor = p.relu ? 0.f : -__builtin_inff();
  __shared__ __attribute__((aligned(16))) u32x4 ost[ES == 2 ? 4 * 32 * NT * 4 : 1];    // per wave: one output tile, 32 rows x NT * 64 bytes
  const bool ost_ok = !p.relu_mask && p.ldy == NT * 32 && (long)p.M * NT * 64 < 0x7fffffffL;
  for (int tile = wave; tile < ntiles; tile += nwaves) {
    bool vm;
    unsigned ox, oy, img;
    if (POOL) {
      const int q = tile * 8 + (r >> 2);
      vm = q < Mp;
      const unsigned qq = vm ? q : 0;
      const unsigned tq = fdiv(qq, p.dWp), pox = qq - tq * Wp;
      img = fdiv(tq, p.dHp);
      oy = 2 * (tq - img * Hp) + ((r >> 1) & 1); ox = 2 * pox + (r & 1);
    } else {
      const int m = tile * 32 + r;
      vm = m < p.M;
      const unsigned mm = vm ? m : 0;
      const unsigned tq = fdiv(mm, p.dWo);
      ox = mm - tq * p.Wo;
      img = fdiv(tq, p.dHo); oy = tq - img * p.Ho;
    }
    const int iy0 = (int)oy * p.stride - PAD, ix0 = (int)ox * p.stride - PAD;
    // byte offset of tap (0,0), chunk 0 of this lane's pixel (may be "negative": wraps, and is then masked by the tap test)
    const unsigned lbase = (unsigned)((((int)img * p.Hi + iy0 + 1) * p.Wi + ix0 + 1) * (CPP * 16)) + (CPP > 1 ? hh * 16 : 0);
    unsigned bad = vm ? 0u : 0x1ffu;                // bit (3 ky + kx): that tap of this pixel is outside the image
    if (NTAP == 9) {
#pragma unroll
      for (int ky = 0; ky < 3; ++ky)
#pragma unroll
        for (int kx = 0; kx < 3; ++kx)
          if ((unsigned)(iy0 + ky) >= (unsigned)p.Hi || (unsigned)(ix0 + kx) >= (unsigned)p.Wi) bad |= 1u << (3 * ky + kx);
    }
    u32x4 a[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const int q0 = 2 * ks, q1 = 2 * ks + 1;
      const int t0 = q0 / CPP, c0 = q0 % CPP, t1 = q1 / CPP, c1 = q1 % CPP;
      if (CPP > 1) {                                // both chunks in tap t0, the upper half-wave one chunk further (in lbase)
        const unsigned v = lbase | (__builtin_amdgcn_ubfe(bad, (unsigned)t0, 1u) << 31);
        a[ks] = __builtin_amdgcn_raw_buffer_load_b128(rx, v, ((t0 / 3) * p.Wi + (t0 % 3)) * (CPP * 16) + c0 * 16, 0);
      } else {                                      // (direct loads: measured faster than the buffer form here, 120 vs 144 us on the first stem layer)
        const int ky = hh ? t1 / 3 : t0 / 3, kx = hh ? t1 % 3 : t0 % 3, cc = hh ? c1 : c0;
        const bool inq = hh ? (q1 < KC) : (q0 < KC);
        const int iy = iy0 + ky, ix = ix0 + kx;
        const bool ok = vm && inq && (unsigned)iy < (unsigned)p.Hi && (unsigned)ix < (unsigned)p.Wi;
        u32x4 v = {0u, 0u, 0u, 0u};
        if (ok) v = *(const u32x4*)(p.x + ((((long)img * p.Hi + iy0) * p.Wi + ix0) + (long)ky * p.Wi + kx) * (CPP * 16) + cc * 16);
        a[ks] = v;
      }
    }
    f32x16 acc[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
      for (int g = 0; g < 16; ++g) acc[nt][g] = 0.f;
    int wlane = lane;
    asm volatile("" : "+v"(wlane));            // opaque per tile: keeps the fragment reads in the loop (hoisted, they are 144 VGPRs again)
#pragma unroll
    for (int ks = 0; ks < KS; ++ks)
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        if (WLDS) Mma<T>::step(acc[nt], a[ks], wl[(nt * KS + ks) * 64 + wlane]);
        else Mma<T>::step(acc[nt], a[ks], bw[WLDS ? 0 : nt][WLDS ? 0 : ks]);
      }
    // bf16 rows of exactly the tile's NT * 32 channels, no mask (every forward launch of the stem / layer1): the tile is 32 * NT * 64
    // contiguous bytes of y.  It goes through this wave's LDS slot (2-byte writes in the accumulator layout, 16-byte reads in memory
    // order; one wave's DS operations execute in order, no barrier) and leaves as 2 * NT wave-wide 1 KiB stores instead of 16 * NT
    // stores of 2 bytes per lane (two 64-byte pieces per instruction).
    if (POOL) {
      char* ob = (char*)ost + (threadIdx.x >> 6) * (32 * NT * 64);
#pragma unroll
      for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          float a4[4];
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            float v = affine<T>(acc[nt][4 * k + j], sc[nt], bi[nt]);
            asm("v_max_f32 %0, %1, %2" : "=v"(v) : "v"(v), "s"(relu_floor));
            a4[j] = bf2f(f2bf(v));
          }
          *(unsigned short*)(ob + (2 * k + hh) * (NT * 64) + (nt * 32 + r) * 2) = f2bf(((a4[0] + a4[1]) + (a4[2] + a4[3])) * 0.25f);
        }
      static_assert(!POOL || NT == 2, "one 1 KiB store per pooled tile");
      const u32x4 o = *(const u32x4*)(ob + lane * 16);
      __builtin_amdgcn_raw_buffer_store_b128(o, ry, (unsigned)(lane * 16), tile * (8 * NT * 64), 0);   // (rows past Mp: outside num_records)
      continue;
    }
    if (ES == 2 && ost_ok) {
      char* ob = (char*)ost + (threadIdx.x >> 6) * (32 * NT * 64);
#pragma unroll
      for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int g = 0; g < 16; ++g) {
          const int row = (g & 3) + 8 * (g >> 2) + 4 * hh;
          float v = affine<T>(acc[nt][g], sc[nt], bi[nt]);
          asm("v_max_f32 %0, %1, %2" : "=v"(v) : "v"(v), "s"(relu_floor));
          *(unsigned short*)(ob + row * (NT * 64) + (nt * 32 + r) * 2) = f2bf(v);
        }
#pragma unroll
      for (int i = 0; i < 2 * NT; ++i) {
        const u32x4 o = *(const u32x4*)(ob + (i * 64 + lane) * 16);
        __builtin_amdgcn_raw_buffer_store_b128(o, ry, (unsigned)((i * 64 + lane) * 16), tile * (32 * NT * 64), 0);   // (rows past M: outside num_records)
      }
      continue;
    }
    // element (row (g&3) + 8(g>>2) + 4hh of the tile, channel 32 nt + r): lane offset once, the row in soffset
    const unsigned vy = (unsigned)(((tile * 32 + 4 * hh) * p.ldy + r) * ES), vmk = (unsigned)(((tile * 32 + 4 * hh) * p.ldm + r) * ES);
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
      for (int g = 0; g < 16; ++g) {
        const int row = (g & 3) + 8 * (g >> 2);
        float v = affine<T>(acc[nt][g], sc[nt], bi[nt]);
        asm("v_max_f32 %0, %1, %2" : "=v"(v) : "v"(v), "s"(relu_floor));
        if (p.relu_mask) {
          float mv;
          if (ES == 2) mv = bf2f((unsigned)__builtin_amdgcn_raw_buffer_load_b16(rm, vmk, (row * p.ldm + nt * 32) * ES, 0));
          else mv = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rm, vmk, (row * p.ldm + nt * 32) * ES, 0));
          if (!(mv > 0.f)) v = 0.f;
        }
        if (ES == 2) __builtin_amdgcn_raw_buffer_store_b16((unsigned short)f2bf(v), ry, vy, (row * p.ldy + nt * 32) * ES, 0);
        else __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), ry, vy, (row * p.ldy + nt * 32) * ES, 0);
      }
  }
}

template <typename T> void launch_small(const ConvArgs& a, unsigned nb, hipStream_t st) {
  if (a.KH == 1 && a.cpp == 8) hipLaunchKernelGGL((k_conv3x3_small<T, 8, 2, 1>), dim3(nb), dim3(256), 0, st, a);
  else if (a.KH == 1) hipLaunchKernelGGL((k_conv3x3_small<T, 32, 2, 1>), dim3(nb), dim3(256), 0, st, a);
  else if (a.cpp == 1 && a.Cout == 32) hipLaunchKernelGGL((k_conv3x3_small<T, 1, 1>), dim3(nb), dim3(256), 0, st, a);
  else if (a.cpp == 1) hipLaunchKernelGGL((k_conv3x3_small<T, 1, 2>), dim3(nb), dim3(256), 0, st, a);
  else if (a.cpp == 8) hipLaunchKernelGGL((k_conv3x3_small<T, 8, 2>), dim3(nb), dim3(256), 0, st, a);
  else if (a.Cout == 32) hipLaunchKernelGGL((k_conv3x3_small<T, 4, 1>), dim3(nb), dim3(256), 0, st, a);
  else if (a.pool_out) {                            // (cddmsl_conv3x3_pool_fwd admits bf16 alone)
    if constexpr (sizeof(T) == 2) hipLaunchKernelGGL((k_conv3x3_small<T, 4, 2, 9, true>), dim3(nb), dim3(256), 0, st, a);
  }
  else hipLaunchKernelGGL((k_conv3x3_small<T, 4, 2>), dim3(nb), dim3(256), 0, st, a);
}

template <typename T> void launch_tile128(const ConvArgs& a, const Plan& p, hipStream_t st) {
  const dim3 grid(p.gx, p.gy);
  switch (p.kernel) {
    case 8: launch_small<T>(a, p.gx, st); break;
    case 2: hipLaunchKernelGGL(k_conv_fwd_reg<T>, grid, dim3(256), 0, st, a); break;
    default: hipLaunchKernelGGL(k_conv_fwd<T>, grid, dim3(256), 0, st, a); break;
  }
}

}  // namespace

void launch_fwd_tile128(const ConvArgs& a, const Plan& p, Operand op, hipStream_t st) {
  if (op == OP_BF16) launch_tile128<__bf16>(a, p, st);
  else launch_tile128<float>(a, p, st);
}
