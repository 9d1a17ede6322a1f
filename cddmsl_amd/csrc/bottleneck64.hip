// The fused frozen res2 bottleneck (kernel id 13): the kernel and its two C entry points.
#include "gemm_common.h"

namespace {

// ------------------------------------------------------------------------------------------------
// One frozen 64-plane CLIP Bottleneck of res2 behind its conv1, as ONE streaming launch (bf16, forward only, stride 1):
//     o2   = relu(bn2(conv2_3x3(o1)))                        never leaves the CU
//     out  = relu(bn3(conv3_1x1(o2)) + residual)             [M][256] -> HBM
//     o1'  = relu(bn1'(conv1'_1x1(out)))        (NEXT)       [M][64]  -> HBM: conv1 of the block that follows
//     residual = bn_d(conv_d_1x1(x0))           (DOWN)       computed from the block's 64-channel input instead of read
// A wave walks 32-pixel tiles with a grid stride, exactly as k_conv3x3_small<T, 8, 2> does for conv2 (same gather, tap mask and
// k-step order).  Every later GEMM takes its A fragments from the wave's 4 KiB LDS slot: a layer's bf16 output is written there
// in the accumulator layout (2-byte writes) and read back as 16-byte chunks -- chunk 2 ks + hh of pixel row r is the A fragment
// of k-step ks -- so each layer sees the operands, the k-step order and the zero accumulator of the separate launch it replaces,
// and every output is rounded to bf16 at the same point: results are bit-identical to those launches, and a row's result does
// not depend on the tile it falls in.  `out` goes through the slot in four column quarters of 64 channels (32 rows x 128 B, the
// slot's one geometry): the quarter's residual rows are staged there in memory order, every lane updates its own elements in
// place, and the finished quarter leaves as four wave-wide 16-byte stores and feeds k-steps 4q .. 4q+3 of conv1'.
// Slot rows are 128 B with chunk ^= (row >> 1) & 7 (16 consecutive rows of one chunk cover the 16 slots of 256 B).
// LDS: conv2's and conv3's weights in fragment order (72 + 32 KiB), conv3's / the downsample's scale and bias (4 KiB), 8 slots
// (32 KiB) = 140 KiB: one workgroup of 8 waves per CU, two waves per SIMD.  The weight fragments of conv1' and of the downsample
// convolution (32 KiB each) do not fit beside them and are read through L1 / L2.
// One wave's DS operations execute in order, so the slot needs no barrier; the compiler fences keep them in program order.
// ------------------------------------------------------------------------------------------------
struct BottleneckArgs {
  const char* o1;        // [M][64]   conv2's input (conv1's output)
  const char* w2;        // [64][3][3][64]
  const char* w3;        // [256][64]
  const char* wd;        // [256][64]  DOWN
  const char* w1n;       // [64][256]  NEXT
  const char* x0;        // [M][64]    DOWN: the block's input
  const char* residual;  // [M][256]   !DOWN
  char* out;             // [M][256]
  char* o1n;             // [M][64]    NEXT
  const float *s2, *b2, *s3, *b3, *sd, *bd, *s1n, *b1n;
  int H, W, M;
  FastDiv dW, dH;
};

template <bool DOWN, bool NEXT>
__global__ __launch_bounds__(512) void k_bottleneck64(BottleneckArgs p) {
  using T = __bf16;
  constexpr int KS2 = 36, WAVES = 8;
  const int lane = threadIdx.x & 63, r = lane & 31, hh = lane >> 5, wv = threadIdx.x >> 6;
  __shared__ __attribute__((aligned(16))) u32x4 wl2[2 * KS2 * 64];     // fragment (nt, ks) of a lane = chunk 2ks+hh of weight row nt*32 + r
  __shared__ __attribute__((aligned(16))) u32x4 wl3[8 * 4 * 64];
  __shared__ __attribute__((aligned(16))) u32x4 slots[WAVES * 256];
  __shared__ float sbl[4 * 256];                                       // s3 | b3 | sd | bd
  for (int f = wv; f < 2 * KS2; f += WAVES) {
    const int nt = f / KS2, ks = f - nt * KS2;
    wl2[f * 64 + lane] = *(const u32x4*)(p.w2 + ((long)(nt * 32 + r) * (2 * KS2) + 2 * ks + hh) * 16);
  }
  for (int f = wv; f < 32; f += WAVES)
    wl3[f * 64 + lane] = *(const u32x4*)(p.w3 + ((long)((f >> 2) * 32 + r) * 8 + 2 * (f & 3) + hh) * 16);
  if (threadIdx.x < 256) {
    sbl[threadIdx.x] = p.s3[threadIdx.x]; sbl[256 + threadIdx.x] = p.b3[threadIdx.x];
    if (DOWN) { sbl[512 + threadIdx.x] = p.sd[threadIdx.x]; sbl[768 + threadIdx.x] = p.bd[threadIdx.x]; }
  }
  __syncthreads();
  float sc2[2], bi2[2], sc1[2], bi1[2];
#pragma unroll
  for (int nt = 0; nt < 2; ++nt) {
    sc2[nt] = p.s2[nt * 32 + r]; bi2[nt] = p.b2[nt * 32 + r];
    sc1[nt] = NEXT ? p.s1n[nt * 32 + r] : 1.f; bi1[nt] = NEXT ? p.b1n[nt * 32 + r] : 0.f;
  }
  const int wave = blockIdx.x * WAVES + wv, nwaves = gridDim.x * WAVES;
  const int ntiles = (p.M + 31) >> 5;
  // (conv2's input is addressed as in k_conv3x3_small: base one row and one pixel before the tensor, tap / chunk in soffset, an
  // invalid tap sets bit 31 of the lane offset.  Everything else: lane offset inside the tile, the tile's base in soffset, and
  // bit 31 of the lane offset for rows past M -- loads give zeros, stores are dropped.)
  const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc((void*)(p.o1 - (long)(p.W + 1) * 128), 0, 0x7fffffff, 0x00020000);
  const __amdgpu_buffer_rsrc_t rx0 = __builtin_amdgcn_make_buffer_rsrc((void*)p.x0, 0, DOWN ? p.M * 128 : 0, 0x00020000);
  const __amdgpu_buffer_rsrc_t rres = __builtin_amdgcn_make_buffer_rsrc((void*)p.residual, 0, DOWN ? 0 : p.M * 512, 0x00020000);
  const __amdgpu_buffer_rsrc_t rout = __builtin_amdgcn_make_buffer_rsrc((void*)p.out, 0, p.M * 512, 0x00020000);
  const __amdgpu_buffer_rsrc_t ro1n = __builtin_amdgcn_make_buffer_rsrc((void*)p.o1n, 0, NEXT ? p.M * 128 : 0, 0x00020000);
  const float relu_floor = 0.f;
  char* const sb = (char*)slots + wv * 4096;
  // slot addresses.  Accumulator layout (element g of a lane = row (g&3) + 8(g>>2) + 4hh, channel 32 ntl + r): the swizzled chunk
  // splits into a lane part XOR the compile-time part (ntl << 2) ^ ((g & 3) >> 1) ^ (((g >> 2) & 1) << 2) -- eight bases.
  char* wbase[8];
#pragma unroll
  for (int c = 0; c < 8; ++c) wbase[c] = sb + 4 * hh * 128 + ((((r >> 3) ^ (hh << 1)) ^ c) << 4) + (r & 7) * 2;
  // A fragment of k-step ks: row r, chunk 2ks + hh
  const char* fbase = sb + r * 128;
  const int fsw = hh ^ ((r >> 1) & 7);
  // memory order: 16-byte piece i * 64 + lane of the 4 KiB = row 8i + (lane >> 3), chunk lane & 7
  const int mrow = lane >> 3;
  char* const mbase0 = sb + mrow * 128 + ((((lane & 7) ^ (lane >> 4))) << 4);      // i even
  char* const mbase1 = sb + mrow * 128 + ((((lane & 7) ^ (lane >> 4) ^ 4)) << 4);  // i odd
  auto maddr = [&](int i) -> char* { return ((i & 1) ? mbase1 : mbase0) + i * 1024; };
  auto put = [&](const f32x16 (&acc)[2], const float (&sc)[2], const float (&bi)[2]) {   // relu(affine) of a 32 x 64 tile -> the slot, bf16
#pragma unroll
    for (int nt = 0; nt < 2; ++nt)
#pragma unroll
      for (int g = 0; g < 16; ++g) {
        float v = affine<T>(acc[nt][g], sc[nt], bi[nt]);
        asm("v_max_f32 %0, %1, %2" : "=v"(v) : "v"(v), "s"(relu_floor));
        *(unsigned short*)(wbase[(nt << 2) ^ ((g & 3) >> 1) ^ (((g >> 2) & 1) << 2)] + ((g & 3) + 8 * (g >> 2)) * 128) = f2bf(v);
      }
  };
  auto frags = [&](u32x4 (&fa)[4]) {
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) fa[ks] = *(const u32x4*)(fbase + (((2 * ks) ^ fsw) << 4));
  };
  for (int tile = wave; tile < ntiles; tile += nwaves) {
    const int m = tile * 32 + r;
    const bool vm = m < p.M;
    const unsigned mm = vm ? m : 0;
    const unsigned tq = fdiv(mm, p.dW), ox = mm - tq * p.W;
    const unsigned img = fdiv(tq, p.dH), oy = tq - img * p.H;
    const int iy0 = (int)oy - 1, ix0 = (int)ox - 1;
    const unsigned lbase = (unsigned)((((int)img * p.H + iy0 + 1) * p.W + ix0 + 1) * 128) + hh * 16;
    unsigned bad = vm ? 0u : 0x1ffu;                // bit (3 ky + kx): that tap of this pixel is outside the image
#pragma unroll
    for (int ky = 0; ky < 3; ++ky)
#pragma unroll
      for (int kx = 0; kx < 3; ++kx)
        if ((unsigned)(iy0 + ky) >= (unsigned)p.H || (unsigned)(ix0 + kx) >= (unsigned)p.W) bad |= 1u << (3 * ky + kx);
    u32x4 a[KS2];
#pragma unroll
    for (int ks = 0; ks < KS2; ++ks) {
      const int t0 = (2 * ks) / 8, c0 = (2 * ks) % 8;
      const unsigned v = lbase | (__builtin_amdgcn_ubfe(bad, (unsigned)t0, 1u) << 31);
      a[ks] = __builtin_amdgcn_raw_buffer_load_b128(rx, v, ((t0 / 3) * p.W + (t0 % 3)) * 128 + c0 * 16, 0);
    }
    // rows of this tile in memory order: piece i of a lane is row 8i + mrow
    const unsigned rowbad[4] = {tile * 32 + mrow < p.M ? 0u : 0x80000000u, tile * 32 + 8 + mrow < p.M ? 0u : 0x80000000u,
                                tile * 32 + 16 + mrow < p.M ? 0u : 0x80000000u, tile * 32 + 24 + mrow < p.M ? 0u : 0x80000000u};
    const unsigned vq = (unsigned)(mrow * 512 + (lane & 7) * 16);      // lane offset of piece 0 in a [M][256] tensor's tile quarter
    u32x4 xa[4], rr[4];
    if (DOWN) {
#pragma unroll
      for (int ks = 0; ks < 4; ++ks)
        xa[ks] = __builtin_amdgcn_raw_buffer_load_b128(rx0, (unsigned)(r * 128 + hh * 16) | (vm ? 0u : 0x80000000u), tile * 4096 + ks * 32, 0);
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i) rr[i] = __builtin_amdgcn_raw_buffer_load_b128(rres, (vq + i * 4096) | rowbad[i], tile * 16384, 0);
    }
    f32x16 acc2[2];
#pragma unroll
    for (int nt = 0; nt < 2; ++nt)
#pragma unroll
      for (int g = 0; g < 16; ++g) acc2[nt][g] = 0.f;
    int wlane = lane;
    asm volatile("" : "+v"(wlane));            // opaque per tile: keeps the fragment reads in the loop (hoisted, they are hundreds of VGPRs)
    // this lane's fragment chunk of weight row r in the [256][64] downsample and the [64][256] next-conv1 weights
    const char* const wdp = p.wd + ((wlane & 31) * 8 + (wlane >> 5)) * 16;
    const char* const w1p = p.w1n + ((wlane & 31) * 32 + (wlane >> 5)) * 16;
#pragma unroll
    for (int ks = 0; ks < KS2; ++ks)
#pragma unroll
      for (int nt = 0; nt < 2; ++nt) Mma<T>::step(acc2[nt], a[ks], wl2[(nt * KS2 + ks) * 64 + wlane]);
    asm volatile("" ::: "memory");
    put(acc2, sc2, bi2);
    asm volatile("" ::: "memory");
    u32x4 fo2[4];
    frags(fo2);
    asm volatile("" ::: "memory");
    f32x16 acc1[2];
#pragma unroll
    for (int nt = 0; nt < 2; ++nt)
#pragma unroll
      for (int g = 0; g < 16; ++g) acc1[nt][g] = 0.f;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      f32x16 acc3[2], accd[2];
#pragma unroll
      for (int nt = 0; nt < 2; ++nt)
#pragma unroll
        for (int g = 0; g < 16; ++g) { acc3[nt][g] = 0.f; accd[nt][g] = 0.f; }
      u32x4 wdf[DOWN ? 2 : 1][DOWN ? 4 : 1], w1f[NEXT ? 2 : 1][NEXT ? 4 : 1];
      if (DOWN) {
#pragma unroll
        for (int nt = 0; nt < 2; ++nt)
#pragma unroll
          for (int ks = 0; ks < 4; ++ks)
            wdf[DOWN ? nt : 0][DOWN ? ks : 0] = *(const u32x4*)(wdp + ((q * 2 + nt) * 32 * 8 + 2 * ks) * 16);
      }
      if (!DOWN) {                                // the quarter's residual rows -> the slot, memory order; the next quarter's set off
#pragma unroll
        for (int i = 0; i < 4; ++i) *(u32x4*)maddr(i) = rr[i];
        if (q < 3) {
#pragma unroll
          for (int i = 0; i < 4; ++i) rr[i] = __builtin_amdgcn_raw_buffer_load_b128(rres, (vq + i * 4096) | rowbad[i], tile * 16384 + (q + 1) * 128, 0);
        }
      }
#pragma unroll
      for (int ks = 0; ks < 4; ++ks)
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) Mma<T>::step(acc3[nt], fo2[ks], wl3[(((q * 2 + nt) << 2) + ks) * 64 + wlane]);
      if (DOWN) {
#pragma unroll
        for (int ks = 0; ks < 4; ++ks)
#pragma unroll
          for (int nt = 0; nt < 2; ++nt) Mma<T>::step(accd[nt], xa[ks], wdf[DOWN ? nt : 0][DOWN ? ks : 0]);
      }
      if (NEXT) {                                 // (requested here: they arrive behind the epilogue's arithmetic)
#pragma unroll
        for (int nt = 0; nt < 2; ++nt)
#pragma unroll
          for (int ks = 0; ks < 4; ++ks)
            w1f[NEXT ? nt : 0][NEXT ? ks : 0] = *(const u32x4*)(w1p + (nt * 32 * 32 + 2 * (4 * q + ks)) * 16);
      }
      asm volatile("" ::: "memory");
#pragma unroll
      for (int nt = 0; nt < 2; ++nt) {
        const int ch = (q * 2 + nt) * 32 + r;
        const float s3 = sbl[ch], b3 = sbl[256 + ch];
        const float sd = DOWN ? sbl[512 + ch] : 1.f, bd = DOWN ? sbl[768 + ch] : 0.f;
#pragma unroll
        for (int g = 0; g < 16; ++g) {
          unsigned short* e = (unsigned short*)(wbase[(nt << 2) ^ ((g & 3) >> 1) ^ (((g >> 2) & 1) << 2)] + ((g & 3) + 8 * (g >> 2)) * 128);
          float v = affine<T>(acc3[nt][g], s3, b3);
          if (DOWN) v += bf2f(f2bf(affine<T>(accd[nt][g], sd, bd)));      // (the downsample launch's bf16 output)
          else v += bf2f(*e);
          asm("v_max_f32 %0, %1, %2" : "=v"(v) : "v"(v), "s"(relu_floor));
          *e = f2bf(v);
        }
      }
      asm volatile("" ::: "memory");
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const u32x4 o = *(const u32x4*)maddr(i);
        __builtin_amdgcn_raw_buffer_store_b128(o, rout, (vq + i * 4096) | rowbad[i], tile * 16384 + q * 128, CDDMSL_STORE_AUX);
        asm volatile("s_nop 4" ::: "memory");    // (store-data hazard, see tile_epilogue)
        asm volatile("" :: "v"(o));
      }
      if (NEXT) {
        u32x4 fo[4];
        frags(fo);
#pragma unroll
        for (int ks = 0; ks < 4; ++ks)
#pragma unroll
          for (int nt = 0; nt < 2; ++nt) Mma<T>::step(acc1[nt], fo[ks], w1f[NEXT ? nt : 0][NEXT ? ks : 0]);
      }
      asm volatile("" ::: "memory");
    }
    if (NEXT) {
      put(acc1, sc1, bi1);
      asm volatile("" ::: "memory");
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const u32x4 o = *(const u32x4*)maddr(i);
        __builtin_amdgcn_raw_buffer_store_b128(o, ro1n, (unsigned)((i * 64 + lane) * 16) | rowbad[i], tile * 4096, 0);
        asm volatile("s_nop 4" ::: "memory");
        asm volatile("" :: "v"(o));
      }
      asm volatile("" ::: "memory");
    }
  }
}

}  // namespace

// ---- the fused frozen 64-plane bottleneck (k_bottleneck64, kernel 13): bf16 only, every tensor addressed with 32-bit byte
// offsets from its base (the [M][256] ones bound M), M a count of whole images
extern "C" int cddmsl_bottleneck64_ok(int Nimg, int H, int W, int dtype) {
  if (dtype != 0 || Nimg <= 0 || H <= 0 || W <= 0) return 0;
  return (long)Nimg * H * W + W + 64 < (1L << 31) / 512 ? 1 : 0;
}

extern "C" int cddmsl_bottleneck64_fwd(const void* o1, const void* w2, const float* s2, const float* b2, const void* w3,
                                       const float* s3, const float* b3, const void* residual, const void* x0, const void* wd,
                                       const float* sd, const float* bd, const void* w1n, const float* s1n, const float* b1n,
                                       void* out, void* o1n, int Nimg, int H, int W, int dtype, void* stream) {
  if (!cddmsl_bottleneck64_ok(Nimg, H, W, dtype)) return CDDMSL_ERR_ARG;
  if (!o1 || !w2 || !s2 || !b2 || !w3 || !s3 || !b3 || !out) return CDDMSL_ERR_ARG;
  const bool down = wd != nullptr, next = w1n != nullptr;
  if (down ? (!x0 || !sd || !bd || residual) : (!residual || x0 || sd || bd)) return CDDMSL_ERR_ARG;   // exactly one source of the residual
  if (next ? (!s1n || !b1n || !o1n) : (s1n || b1n || o1n)) return CDDMSL_ERR_ARG;
  BottleneckArgs a;
  a.o1 = (const char*)o1; a.w2 = (const char*)w2; a.w3 = (const char*)w3; a.wd = (const char*)wd; a.w1n = (const char*)w1n;
  a.x0 = (const char*)x0; a.residual = (const char*)residual; a.out = (char*)out; a.o1n = (char*)o1n;
  a.s2 = s2; a.b2 = b2; a.s3 = s3; a.b3 = b3; a.sd = sd; a.bd = bd; a.s1n = s1n; a.b1n = b1n;
  a.H = H; a.W = W; a.M = Nimg * H * W;
  a.dW = make_fastdiv((unsigned)W); a.dH = make_fastdiv((unsigned)H);
  if (record_kernel(13)) return CDDMSL_OK;
  // one workgroup of 8 waves per CU (its LDS image is filled once), each wave walking 32-pixel tiles with a grid stride
  const int ncu = persistent_blocks_raw(), ntiles = (a.M + 31) / 32;
  const int want = (ntiles + 7) / 8, cap = ncu > 0 ? ncu : 256;
  const unsigned nb = (unsigned)(want < cap ? want : cap);
  const hipStream_t st = (hipStream_t)stream;
  if (down && next) hipLaunchKernelGGL((k_bottleneck64<true, true>), dim3(nb), dim3(512), 0, st, a);
  else if (down) hipLaunchKernelGGL((k_bottleneck64<true, false>), dim3(nb), dim3(512), 0, st, a);
  else if (next) hipLaunchKernelGGL((k_bottleneck64<false, true>), dim3(nb), dim3(512), 0, st, a);
  else hipLaunchKernelGGL((k_bottleneck64<false, false>), dim3(nb), dim3(512), 0, st, a);
  return launch_status();
}
