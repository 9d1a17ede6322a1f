// What the conv / GEMM translation units share: tile constants, kernel-argument structs, MFMA wrappers, the small device helpers
// more than one unit uses, the plan a planner hands to a launcher, and the launchers' declarations.
//   gemm_conv.hip     host dispatch (fill, plan, run) and every C entry point but the fused bottleneck's; weight-prep kernels
//   conv_fwd.hip      128x128 tile and few-channel streaming forward kernels            kernel ids 1, 2, 8
//   conv_fwd256.hip   256x256 and 256x128 tile forward kernels, split-K tail            kernel ids 3, 10, 11
//   conv_wgrad.hip    weight-gradient and batched TN GEMM kernels, split reduction      kernel ids 4, 5, 6, 7, 9, 12
//   bottleneck64.hip  fused frozen res2 bottleneck and its entry points                 kernel id 13
// Every kernel is defined in one unit and launched from that unit only.  The units are compiled without relocatable device code,
// so everything here has internal linkage (each unit gets its own copy) except the launch functions at the end.
// -DCDDMSL_TILE_STAMPS (tools/tile_stamps.py) adds a member to ConvArgs / WgradArgs: define it for all of these units or for none.
#pragma once
#include "common.h"
#include <cstdlib>

namespace {

constexpr int BM = 128, BN = 128, KCH = 8;  // KCH chunks of 16 B per K-tile row

// n / d for 0 <= n < 2^31 with a host-precomputed multiplier (round-up method): q = (umulhi(n, mul) + n) >> shr
struct FastDiv {
  unsigned mul, shr, d;
};
static inline FastDiv make_fastdiv(unsigned d) {
  FastDiv f;
  f.d = d;
  unsigned s = 0;
  while ((1ull << s) < d) ++s;
  f.shr = s;
  f.mul = (unsigned)(((1ull << 32) * ((1ull << s) - d)) / d + 1);
  return f;
}
__device__ __forceinline__ unsigned fdiv(unsigned n, const FastDiv& f) { return (__umulhi(n, f.mul) + n) >> f.shr; }

// FrozenBN / bias in the epilogues: v * scale + bias.  The exact-f32 instantiations round twice like the reference's separate
// multiply and add (the library is built with -ffp-contract=off); the bf16 ones use one fused multiply-add -- one vector-ALU
// operation less per output element in every epilogue, identical where scale = 1 and bias = 0 (input-gradient launches).
template <typename T> __device__ __forceinline__ float affine(float v, float sc, float bi) {
  return sizeof(T) <= 2 ? __builtin_fmaf(v, sc, bi) : v * sc + bi;
}

// Cache-policy bits (buffer instruction aux: 1 = sc0, 2 = nt, 16 = sc1) of the 256x256 kernel's output stores and of its residual /
// ReLU-mask loads.  The outputs are written once and read by a LATER launch, by which time they have left the caches anyway: stored
// non-temporal they stop evicting the operand tiles the other workgroups are re-reading -- measured on the training step, same box,
// rebuilt library (scratch A/B): nt stores -0.55 .. -0.95 ms per step, sc0|nt the same, sc0 alone nothing,
// nt|sc1 +0.4 ms, nt on the residual / mask loads nothing on top.
#ifndef CDDMSL_STORE_AUX
#define CDDMSL_STORE_AUX 2
#endif
#ifndef CDDMSL_LOAD_AUX
#define CDDMSL_LOAD_AUX 0
#endif

struct ConvArgs {
  const char* x;
  const char* w;
  char* y;
  const float* scale;
  const float* bias;
  const char* residual;
  const char* relu_mask;
  int Nimg, Hi, Wi, Cin, Ho, Wo, Cout, KH, KW, stride, pad;
  int ldy, ldr, ldm;
  int relu, out_f32, pool;
  int res_f32;     // residual rows are f32 although T is bf16 (f32 output only): the mapper's f32 residual stream
  int res_pool;    // residual is [Nimg][Ho/2][Wo/2][ldr]: row m adds 0.25 * residual[pooled pixel of m] (AvgPool2d(2) backward fused)
  int M, Kc, cpp;  // rows, total K chunks, chunks per pixel
  FastDiv dWo, dHo, dcpp, dKW;
  int xrs, wrs;    // row strides in 16-byte chunks: A pixel -> pixel (default cpp), B row -> row (default Kc)
  long bx, bw, by; // byte strides of the batch axis (gridDim.y); 0 for plain convolutions
  // fp8 configuration: a second, OCP e4m3 copy of the (bf16) output for the convolution that consumes it -- y8[m][n] =
  // sat(y * q8[0]) -- written by the 256x256 kernel's epilogue, which also max-es |y| into amax8[blockIdx & 63] (delayed scaling)
  char* y8 = nullptr;
  const float* q8 = nullptr;
  unsigned* amax8 = nullptr;
  // split-K form of the 256x256 kernel (the tail of a launch whose tile count leaves the last round of workgroups nearly empty):
  // block b computes K-tiles [kper * (b % ksplits), ...) of logical tile tile0 + b / ksplits and stores its raw accumulators, in
  // fragment order, at partial[b]; k_conv_split_reduce sums a tile's splits and applies the epilogue.  tile_limit: the main
  // launch stops at this logical tile (persistent form; the one-tile grid is simply shorter).
  float* partial = nullptr;
  int tile0 = 0, ksplits = 1, kper = 0, tile_limit = 0;
  // cddmsl_conv3x3_pool_fwd: y is AvgPool2d(2) of the result, [Nimg][Ho/2][Wo/2][ldy] (k_conv3x3_small POOL); divisors of the pooled map
  int pool_out = 0;
  FastDiv dWp = {}, dHp = {};
  int nt_out = 1;  // bf16 output stored non-temporal (CDDMSL_STORE_AUX): outputs too large to be found in the caches by their consumer
#ifdef CDDMSL_TILE_STAMPS
  unsigned long long* tstamps = nullptr;  // diagnostic build only (tools/tile_stamps.py): per wave, 100 MHz s_memrealtime stamps at entry / loop start / loop end / exit
#endif
};

template <typename T> struct Mma;
template <> struct Mma<__bf16> {
  static constexpr int ES = 2;
  __device__ static __forceinline__ void step(f32x16& acc, const u32x4& a, const u32x4& b) {
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), acc, 0, 0, 0);
  }
  __device__ static __forceinline__ float load(const char* p) { return bf2f(*(const unsigned short*)p); }
  __device__ static __forceinline__ void store(char* p, float v) { *(unsigned short*)p = f2bf(v); }
};
template <> struct Mma<float> {
  static constexpr int ES = 4;
  // lane half h holds k = 4h + j in element j; MFMA step j contracts k in {j, 4 + j}: the same
  // permutation on both operands, so the sum over the chunk pair is exact f32 fma accumulation.
  __device__ static __forceinline__ void step(f32x16& acc, const u32x4& a, const u32x4& b) {
    const f32x4 fa = __builtin_bit_cast(f32x4, a), fb = __builtin_bit_cast(f32x4, b);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[0], fb[0], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[1], fb[1], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[2], fb[2], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[3], fb[3], acc, 0, 0, 0);
  }
  __device__ static __forceinline__ float load(const char* p) { return *(const float*)p; }
  __device__ static __forceinline__ void store(char* p, float v) { *(float*)p = v; }
};
typedef __attribute__((ext_vector_type(8))) int i32x8;   // operand of v_mfma_scale_f32_32x32x64_f8f6f4 (e4m3: two 16-byte chunks)

// XCD-aware tile order (8 XCDs, blocks dealt round-robin): give each XCD a contiguous run of logical tiles so the
// tiles that share an A row-panel / weight panel hit the same 4 MiB L2.  Bijective for any grid size.
__device__ __forceinline__ int xcd_remap(int bid, int nblk) {
  const int q = nblk >> 3, rem = nblk & 7, x = bid & 7, j = bid >> 3;
  return (x < rem ? x * (q + 1) : rem * (q + 1) + (x - rem) * q) + j;
}

// average of 4 packed chunks (2x2 avg-pool fused into the A loader)
template <typename T> __device__ __forceinline__ u32x4 avg4(const u32x4& a, const u32x4& b, const u32x4& c, const u32x4& d);
template <> __device__ __forceinline__ u32x4 avg4<float>(const u32x4& a, const u32x4& b, const u32x4& c, const u32x4& d) {
  const f32x4 fa = __builtin_bit_cast(f32x4, a), fb = __builtin_bit_cast(f32x4, b);
  const f32x4 fc = __builtin_bit_cast(f32x4, c), fd = __builtin_bit_cast(f32x4, d);
  f32x4 r = ((fa + fb) + (fc + fd)) * 0.25f;
  return __builtin_bit_cast(u32x4, r);
}
template <> __device__ __forceinline__ u32x4 avg4<__bf16>(const u32x4& a, const u32x4& b, const u32x4& c, const u32x4& d) {
  u32x4 r;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    float lo = (bf2f(a[j] & 0xffff) + bf2f(b[j] & 0xffff)) + (bf2f(c[j] & 0xffff) + bf2f(d[j] & 0xffff));
    float hi = (bf2f(a[j] >> 16) + bf2f(b[j] >> 16)) + (bf2f(c[j] >> 16) + bf2f(d[j] >> 16));
    r[j] = pack2bf(lo * 0.25f, hi * 0.25f);
  }
  return r;
}

// 16 zero bytes for LDS-DMA lanes that have nothing to fetch (out-of-image taps, tails); one copy per translation unit
__device__ __attribute__((aligned(16))) unsigned int g_zero_page[4] = {0u, 0u, 0u, 0u};

__device__ __forceinline__ void glds16(const void* g, void* l) {
  __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)g,
                                   (__attribute__((address_space(3))) void*)l, 16, 0, 0);
}

// ------------------------------------------------------------------------------------------------
// wgrad:  dW[n][k] += scale[n] * sum_m dY[m][n] * A[m][k]
// ------------------------------------------------------------------------------------------------
struct WgradArgs {
  const char* x;    // NHWC input of the forward conv
  const char* dy;   // [M][ldd] T
  float* dw;        // [Cout][K] f32 (K = KH*KW*Cin), accumulated with atomics
  const float* scale;
  int Nimg, Hi, Wi, Cin, Ho, Wo, Cout, KH, KW, stride, pad, ldd, pool;
  int M, Kc, cpp, K, ncc;  // ncc = chunks per dY row that exist (Cout*ES/16)
  int mtiles_per_split;
  FastDiv dWo, dHo;
  int xrs;            // x row stride in chunks (default cpp)
  int ldo;            // output row stride in elements (default K)
  int direct;         // 0: f32 atomicAdd (split reductions); 1: plain f32 store; 2: plain T store (single split only)
  long bx, bd, bo;    // batch (gridDim.y) byte strides of x, dy, out
  // k_gemm_tn_small MODE 3 (cddmsl_attnpool_dx): per-batch row vector added to every output row, bit masks of the rows to keep,
  // f32 accumulator of the unmasked rows
  const float* g0 = nullptr;
  const unsigned long long* mbits = nullptr;
  float* gpos = nullptr;
  float* ws = nullptr;  // split reductions through a workspace: block (split, tile) stores its accumulators, in fragment order, at
                        // ws[(split * ntiles + tile) * tile_floats ...]; k_wgrad_reduce sums the splits into dw (see cddmsl_set_workspace)
#ifdef CDDMSL_TILE_STAMPS
  unsigned long long* tstamps = nullptr;   // diagnostic build only (tools/tile_stamps.py)
#endif
};

constexpr int WM = 64;                 // m rows per reduction tile
constexpr int WROW = 16 + 4;           // LDS row = 16 data chunks (256 B) + 4 pad chunks (64 B)

// chunk swizzle of the 256-byte LDS rows that are read transposed (conv_wgrad.hip, LDS-DMA variant): chunk ^= fsw(row)
__device__ __forceinline__ int fsw(int row) { return ((row & 3) << 2) | ((row >> 2) & 3); }

// raw accumulators of a wave's 128 x 64 tile (acc[4][2] of 32x32 blocks) in fragment order: 32 x 16 bytes per lane, 1 KiB per wave
// instruction.  `dst`: this lane's first slot (the split reductions: k_wgrad_reduce<8, 32>, k_conv_split_reduce)
__device__ __forceinline__ void store_frags(f32x4* dst, const f32x16 (&acc)[4][2]) {
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int g4 = 0; g4 < 4; ++g4) {
        const f32x4 v = {acc[a][b][4 * g4], acc[a][b][4 * g4 + 1], acc[a][b][4 * g4 + 2], acc[a][b][4 * g4 + 3]};
        dst[((a * 2 + b) * 4 + g4) * 64] = v;
      }
}

// The A/B knobs are integer environment variables, read where they are used -- per launch, so one process can A/B -- unless the
// caller keeps the value (CDDMSL_NT_MIN_MB).  `set`: whether the variable exists at all.
static long env_int(const char* name, long dflt, bool* set = nullptr) {
  const char* e = getenv(name);
  if (set) *set = e != nullptr;
  return e ? atol(e) : dflt;
}

// operand type of a launch: the C ABI's dtype (0 = bf16, 1 = f32), or OCP e4m3 bytes (the fp8 entry points)
enum Operand { OP_BF16 = 0, OP_F32 = 1, OP_FP8 = 2 };
static int elem_size(Operand op) { return op == OP_BF16 ? 2 : op == OP_F32 ? 4 : 1; }

// ---- plan: what the planners return (members a planner does not set are 0)
struct Plan {
  int kernel;              // id of cddmsl_last_kernel (hip.py _CONV_KERNEL); 0 = no kernel takes the launch (CDDMSL_ERR_ARG)
  unsigned gx, gy;         // grid
  int splits;              // weight gradient: blocks along the reduction (m) per output tile ...
  int mtiles_per_split;    // ... and reduction tiles of WM rows per block
  int bpb;                 // batched TN GEMM, kernels 9 and 7: batches per block
};

// CUs of the device rounded down to a multiple of 8 (dealt round-robin over the XCDs): workgroups of the persistent kernels
static int persistent_blocks_raw() {
  static int ncu = -1;
  if (ncu < 0) {
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) n = 0;
    ncu = (n / 8) * 8;
  }
  return ncu;
}

}  // namespace

// ---- launch: what crosses the units.  Each takes the filled kernel arguments and the plan and launches exactly what the plan says;
// ws / ws_bytes: the registered workspace (cddmsl_set_workspace), null / 0 without one.  C linkage because the argument structs
// have internal linkage (they are part of the kernels' names); hidden: the library exports none of them.
extern "C" {
__attribute__((visibility("hidden"))) void launch_fwd_tile128(const ConvArgs& a, const Plan& p, Operand op, hipStream_t st);                        // conv_fwd.hip: kernels 1, 2, 8
__attribute__((visibility("hidden"))) void launch_fwd_tile256(const ConvArgs& a, const Plan& p, Operand op, hipStream_t st, void* ws, long ws_bytes);  // conv_fwd256.hip: kernels 3, 10, 11
__attribute__((visibility("hidden"))) void launch_wgrad(WgradArgs& a, const Plan& p, Operand op, hipStream_t st, void* ws, long ws_bytes);             // conv_wgrad.hip: kernels 4, 5, 6, 12
__attribute__((visibility("hidden"))) void launch_gemm_tn(const WgradArgs& p, Operand op, const Plan& pl, int batch, int mode, hipStream_t st);        // conv_wgrad.hip: kernels 9, 7, 5
__attribute__((visibility("hidden"))) void launch_attnpool_dx(const WgradArgs& p, unsigned gx, unsigned gy, int nbatch, int bpb, hipStream_t st);      // conv_wgrad.hip: kernel 9, MODE 3
// gemm_conv.hip: records `id` as the thread's last kernel (cddmsl_last_kernel); true in plan-only mode = do not launch
__attribute__((visibility("hidden"))) bool record_kernel(int id);
}
