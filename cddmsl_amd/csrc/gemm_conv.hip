// Implicit-GEMM convolution / linear kernels for gfx950 (MI355X, CDNA4), wave64 + MFMA.
//
// Replaces on the hot path: ATen conv2d / F.linear as called from the reference's
//   ModifiedResNet / Bottleneck   detectron2/modeling/backbone/clip_backbone.py:57-70,193-219
//   FrozenBatchNorm2d             detectron2/layers/batch_norm.py:45-66   (fused epilogue)
//   StandardRPNHead               detectron2/modeling/proposal_generator/rpn.py:158-177
//   AttentionPool2d projections   clip_backbone.py:83-107
//   TransformerMapper linears     detectron2/modeling/backbone/clipcap/clipcap.py:39-163
//
// Data layout: activations NHWC (channels contiguous), weights [Cout][KH][KW][Cin] (= torch
// channels_last OIHW).  Everything is addressed in 16-byte "chunks" along the contraction axis, so
// one kernel template serves bf16 (8 elem/chunk, v_mfma_f32_32x32x16_bf16) and exact f32
// (4 elem/chunk, v_mfma_f32_32x32x2_f32, bitwise an fmaf chain) -- the f32 instantiation is the
// parity path, the bf16 one the throughput path.
//
//   conv_fwd  : Y[m,n] = epi( sum_k A[m,k] * W[n,k] ),  A gathered on the fly from NHWC input
//               (m = (img,oy,ox), k = (ky,kx,c)); epilogue = per-n scale/bias (FrozenBN), residual
//               add, ReLU, ReLU-backward mask, f32 or T store.  dgrad runs through the same kernel
//               with flipped/transposed weights (see weight_prep).
//   conv_wgrad: dW[n,k] += scale[n] * sum_m dY[m,n] * A[m,k]  (reduction over m = pixels), both
//               operands staged row-major and read transposed (ds_read_b64_tr_b16), split over m
//               with f32 atomics.
//
// Tile: 128x128 per 256-thread workgroup (4 waves, 2x2, 64x64 per wave = 2x2 MFMA 32x32 tiles),
// K-tile = 8 chunks (128 B per row).  LDS rows are 128 B with chunk ^= (row>>1)&7 so that every
// ds_read_b128 lane group hits 16 distinct 16-B slots (bank = (addr/4)%64).
//
// This file is the host side: the C entry points, their argument checks and the planners, plus the weight-prep kernels.  The
// kernels and their launchers are in conv_fwd.hip, conv_fwd256.hip, conv_wgrad.hip and bottleneck64.hip (map: gemm_common.h).
#include "gemm_common.h"

namespace {

template <typename T>
__device__ __forceinline__ void weight_prep_body(const float* w, const float* scale, char* wf, char* wd, int Cout, int KH, int KW, int Cin,
                                                 long first, long stride) {
  __shared__ float tile[32][33];
  const int taps = KH * KW, nit = (Cin + 31) / 32, nct = (Cout + 31) / 32;
  const long ntiles = (long)nct * taps * nit;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;          // 256 threads: 8 rows x 32 columns per sweep
  constexpr int ES = Mma<T>::ES;
  for (long tl = first; tl < ntiles; tl += stride) {
    const int it = (int)(tl % nit); const long q = tl / nit;
    const int tap = (int)(q % taps), ct = (int)(q / taps);
    const int ky = tap / KW, kx = tap % KW;
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int co = ct * 32 + ty + 8 * r, ci = it * 32 + tx;
      float v = 0.f;
      if (co < Cout && ci < Cin) {
        const long i = ((long)co * taps + tap) * Cin + ci;
        v = w[i];
        if (wf) Mma<T>::store(wf + i * ES, v);
        if (scale) v *= scale[co];
      }
      tile[ty + 8 * r][tx] = v;
    }
    __syncthreads();
    if (wd) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int ci = it * 32 + ty + 8 * r, co = ct * 32 + tx;
        if (ci < Cin && co < Cout) {
          const long j = (((long)ci * KH + (KH - 1 - ky)) * KW + (KW - 1 - kx)) * Cout + co;
          Mma<T>::store(wd + j * ES, tile[tx][ty + 8 * r]);
        }
      }
    }
  }
}
template <typename T>
__global__ __launch_bounds__(256) void k_weight_prep(const float* w, const float* scale, char* wf, char* wd, int Cout, int KH, int KW, int Cin) {
  weight_prep_body<T>(w, scale, wf, wd, Cout, KH, KW, Cin, (long)blockIdx.x, (long)gridDim.x);
}
// every trainable weight of the step in ONE launch: blockIdx.y = table row {w, scale, wf, wd, Cout, KH, KW, Cin} (8 x int64)
template <typename T>
__global__ __launch_bounds__(256) void k_weight_prep_multi(const long long* table) {
  const long long* e = table + 8 * (long)blockIdx.y;
  weight_prep_body<T>((const float*)e[0], (const float*)e[1], (char*)e[2], (char*)e[3], (int)e[4], (int)e[5], (int)e[6], (int)e[7],
                      (long)blockIdx.x, (long)gridDim.x);
}

static thread_local int g_last_kernel = 0;   // which kernel the last conv/GEMM entry point of this thread launched (cddmsl_last_kernel)
static thread_local int g_plan_only = 0;     // cddmsl_plan_only(1): entry points choose their kernel (g_last_kernel) and return without launching

// ================================================================================================
// Host side.  Every entry point below is three steps:
//   fill    fill_conv / fill_wgrad validate the C arguments and build the kernel arguments;
//   plan    plan_fwd / plan_wgrad / plan_gemm_tn choose the kernel (the ids of cddmsl_last_kernel), its grid and its split from the
//           filled arguments, the operand type and the batch count: no HIP call, nothing global touched but the A/B knobs read;
//   launch  run_fwd / run_wgrad record the choice, stop there in plan-only mode, and launch what the plan says.
// What needs the device (CU count, registered workspace) is decided in the launchers: the persistent form and the K-split
// tail of the 256x256 kernel, and whether a split reduction goes through the workspace.
// ================================================================================================

// Shapes the 256x256 kernel takes: whole 256-column tiles, K-tiles inside one filter tap, vector epilogue, <= 32 taps,
// and enough tiles to fill the chip.  Environment CDDMSL_GEMM256 (read per launch, so one process can A/B): 0 = always the
// 128x128 kernel, 2 = the 256x256 kernel wherever it is legal, unset/1 = the heuristic below.
static bool gemm256_legal(const ConvArgs& a) {
  const bool vec_ok = (a.ldy % 8 == 0) && (!a.residual || a.ldr % 8 == 0) && (!a.relu_mask || a.ldm % 8 == 0);
  if (a.pool || (a.cpp & 7) || (a.Cout & 255) || !vec_ok || a.KH * a.KW > 31) return false;
  if (2 * a.pad > a.KH - 1 || 2 * a.pad > a.KW - 1) return false;   // rows of a tile must ascend in memory (per-block buffer base)
  return true;
}

static bool use_gemm256(const ConvArgs& a, int batch) {
  const long mode = env_int("CDDMSL_GEMM256", 1);
  if (mode == 0) return false;
  if (!gemm256_legal(a)) return false;
  if (mode == 2) return true;                                   // forced (tests)
  // (per-shape A/B inside the training step: 196 tiles (M 25088, N 512) run 1.3-1.5x faster here, 100 tiles and fewer slower)
  const long tiles = (long)((a.M + 255) / 256) * (a.Cout / 256) * batch;
  return tiles >= 160;
}

// The 256x128 two-workgroup kernel: whole 128-column tiles, K-tiles of 4 chunks inside one filter tap, vector epilogue.
// CDDMSL_FWD2 (read per launch): 0 = never, 2 = wherever legal (tests, A/B), unset / 1 = the heuristic.
static bool fwd2_legal(const ConvArgs& a) {
  const bool vec_ok = (a.ldy % 8 == 0) && (!a.residual || a.ldr % 8 == 0) && (!a.relu_mask || a.ldm % 8 == 0);
  if (a.pool || a.res_pool || (a.cpp & 3) || (a.Cout & 127) || !vec_ok || a.KH * a.KW > 31) return false;
  if (2 * a.pad > a.KH - 1 || 2 * a.pad > a.KW - 1) return false;
  return true;
}
static bool use_fwd2(const ConvArgs& a, int batch) {
  const long mode = env_int("CDDMSL_FWD2", 1);
  if (mode == 0 || !fwd2_legal(a)) return false;
  if (mode == 2) return true;
  // What the 256x256 kernel does not take (Cout = 128, 384, ...; too few 256x256 tiles), when there are enough 256x128 tiles to
  // give every CU work: per shape (two dispatches in one process) 1.14-1.31x the 128x128 kernel on the 128-channel 3x3 layers,
  // 1.04-1.23x on their 1x1 layers; against the 256x256 kernel it loses (x0.72-0.99) on everything but K = 128.
  if (use_gemm256(a, batch) || batch != 1) return false;
  return (long)(a.Cout / 128) * ((a.M + 255) / 256) >= env_int("CDDMSL_FWD2_MIN", 256);      // (A/B knob)
}

static Plan plan_fwd(const ConvArgs& a, Operand op, int batch) {
  const long tiles256 = (long)(a.Cout / 256) * ((a.M + 255) / 256);
  if (op == OP_FP8) {                                           // e4m3 operands: the 256x256 kernel or nothing -- there is no fallback
    if (!gemm256_legal(a) || tiles256 > 0x7fffffffL) return {};
    return {10, (unsigned)tiles256, 1};
  }
  if (a.y8 && !use_gemm256(a, batch)) return {};               // e4m3 second output: only launches the 256x256 kernel takes (its epilogue writes it)
  const long tiles128 = (long)((a.Cout + BN - 1) / BN) * ((a.M + BM - 1) / BM);
  if (tiles128 > 0x7fffffffL) return {};
  const bool packed = batch == 1 && a.xrs == a.cpp && a.wrs == a.Kc;
  // few-channel 3x3 layers (the CLIP stem): streaming register-weight kernel
  // (8 chunks per pixel = the 64 -> 64 layers of res2 in bf16, forward and -- with the ReLU mask -- input gradient)
  if (!a.pool && a.KH == 3 && a.KW == 3 && a.pad == 1 && (a.cpp == 1 || a.cpp == 4 || (a.cpp == 8 && a.Cout == 64)) &&
      (a.Cout == 32 || a.Cout == 64) && !a.residual && !a.out_f32 && packed) {
    // grid-stride over 32-pixel tiles.  Register weights (one chunk per pixel): 8 blocks of 4 waves per CU.  LDS weights (up to
    // 72 KiB per block, two blocks fit a CU): exactly the resident blocks, so that the weight image is filled once per CU slot
    // (2048 blocks refilled it every 4 tiles: 2.9 -> 2.7 ms/step)
    return {8, a.cpp > 1 ? 256u * 2 : 256u * 8, 1};
  }
  // ... and the 1x1 layers of res2 with 64 output channels (64 -> 64, 256 -> 64: one 128-column tile of the GEMM kernels would be half
  // empty): the same kernel with one tap, bf16.  CDDMSL_SMALL_1X1=0: the 128x128 GEMM kernel (A/B)
  if (op == OP_BF16 && !a.pool && a.KH == 1 && a.KW == 1 && a.pad == 0 && a.stride == 1 && a.Cout == 64 && (a.cpp == 8 || a.cpp == 32) &&
      !a.residual && !a.out_f32 && !a.y8 && packed && a.ldy == 64 && env_int("CDDMSL_SMALL_1X1", 1) != 0) return {8, 512, 1};
  if (use_fwd2(a, batch)) return {11, (unsigned)((long)(a.Cout / 128) * ((a.M + 255) / 256)), (unsigned)batch};
  if (use_gemm256(a, batch)) return {3, (unsigned)tiles256, (unsigned)batch};
  if (a.pool) return {2, (unsigned)tiles128, 1};           // AvgPool2d(2) fused into the loader: the register-staged kernel
  return {1, (unsigned)tiles128, (unsigned)batch};
}

static void* g_ws = nullptr;       // device workspace for split reductions (cddmsl_set_workspace); process-wide: one device per process
static long g_ws_bytes = 0;

// ---- launch, forward: the kernels live in conv_fwd.hip (1, 2, 8) and conv_fwd256.hip (3, 10, 11)
static int run_fwd(const ConvArgs& a, Operand op, const Plan& p, void* stream) {
  if (p.kernel == 0) return CDDMSL_ERR_ARG;
  g_last_kernel = p.kernel;
  if (g_plan_only) return CDDMSL_OK;
  if (p.kernel == 3 || p.kernel == 10 || p.kernel == 11) launch_fwd_tile256(a, p, op, (hipStream_t)stream, g_ws, g_ws_bytes);
  else launch_fwd_tile128(a, p, op, (hipStream_t)stream);
  return launch_status();
}

}  // namespace

#ifdef CDDMSL_TILE_STAMPS
static unsigned long long* g_tile_stamps = nullptr;
extern "C" void cddmsl_debug_tile_stamps(unsigned long long* p) { g_tile_stamps = p; }
#endif
extern "C" int cddmsl_last_kernel(void) { return g_last_kernel; }
extern "C" int cddmsl_plan_only(int on) { const int was = g_plan_only; g_plan_only = on; return was; }
bool record_kernel(int id) { g_last_kernel = id; return g_plan_only != 0; }

// outputs up to CDDMSL_NT_MIN_MB MiB are stored with the default policy (their consumer may still find them in the 256 MiB last-level cache), larger
// ones non-temporal (same-box A/B of the training step, 3 runs each: never 102.38 ms, always 101.60, above 128 MiB 101.66; on another box 100 MiB was
// 0.4 ms ahead of always)
static int nt_out_for(long out_bytes) {
  static const long nt_min_mb = env_int("CDDMSL_NT_MIN_MB", 128);
  return out_bytes > (nt_min_mb << 20) ? 1 : 0;
}

// ---- fill, forward: validates the arguments of the convolution entry points and builds the kernel arguments (a.M == 0 with
// CDDMSL_OK: nothing to do).  x / w are `op`; with e4m3 operands everything else is as for bf16.  out_f32: bit 0 = f32 output, and
// for cddmsl_conv_fwd bits 1 and 2 (below).  y8 / q8 / amax8 (nullable): the e4m3 second output.
static int fill_conv(ConvArgs& a, Operand op, const void* x, const void* w, void* y, const float* scale, const float* bias,
                     const void* residual, const void* relu_mask, int Nimg, int Hi, int Wi, int Cin, int Cout, int KH, int KW,
                     int stride, int pad, int pool, int ldy, int ldr, int ldm, int relu, int out_f32, void* y8, const float* q8,
                     float* amax8) {
  const int es = elem_size(op);
  if (Nimg < 0 || Hi <= 0 || Wi <= 0 || Cin <= 0 || Cout <= 0 || KH <= 0 || KW <= 0 || stride <= 0) return CDDMSL_ERR_ARG;
  if ((Cin * es) % 16 != 0) return CDDMSL_ERR_ARG;            // channel rows must be whole 16-B chunks
  if (pool && (KH != 1 || KW != 1 || pad != 0 || stride != 1)) return CDDMSL_ERR_ARG;
  a.x = (const char*)x; a.w = (const char*)w; a.y = (char*)y; a.scale = scale; a.bias = bias;
  a.residual = (const char*)residual; a.relu_mask = (const char*)relu_mask;
  a.Nimg = Nimg; a.Hi = Hi; a.Wi = Wi; a.Cin = Cin; a.Cout = Cout; a.KH = KH; a.KW = KW; a.stride = stride; a.pad = pad;
  if (pool) { a.Ho = Hi / 2; a.Wo = Wi / 2; }
  else { a.Ho = (Hi + 2 * pad - KH) / stride + 1; a.Wo = (Wi + 2 * pad - KW) / stride + 1; }
  if (a.Ho <= 0 || a.Wo <= 0) return CDDMSL_ERR_ARG;
  // out_f32 bit 1: the residual rows are f32 (bf16 kernels, f32 output, no ReLU mask) -- the mapper's f32 residual stream
  if ((out_f32 & 2) && (!(out_f32 & 1) || !residual || relu_mask || pool)) return CDDMSL_ERR_ARG;
  a.ldy = ldy; a.ldr = ldr; a.ldm = ldm; a.relu = relu; a.out_f32 = out_f32 & 1; a.pool = pool;
  a.res_f32 = (op == OP_BF16 && (out_f32 & 2)) ? 1 : 0;
  // out_f32 bit 2: the residual is a 2x2-average-pooled gradient (the downsample path's input gradient at pooled resolution);
  // buffer-addressed from the tensor base, so the pooled tensor must stay below 2 GiB
  a.res_pool = (out_f32 & 4) ? 1 : 0;
  if (a.res_pool && (!residual || (out_f32 & 2) || pool || KH != 1 || KW != 1 || pad != 0 || (long)Nimg * (a.Ho / 2) * (a.Wo / 2) * ldr * es >= (1L << 31) ||
                     (Cout & 7) || (ldy & 7) || (ldr & 7) || (relu_mask && (ldm & 7)))) return CDDMSL_ERR_ARG;
  if (a.res_f32 && ((Cout & 7) || (ldy & 7) || (ldr & 7))) return CDDMSL_ERR_ARG;                // (vector epilogue only)
  long M = (long)Nimg * a.Ho * a.Wo;
  if (M > 0x7fffff00L) return CDDMSL_ERR_ARG;
  a.M = (int)M; a.cpp = Cin * es / 16; a.Kc = KH * KW * a.cpp;
  a.dWo = make_fastdiv((unsigned)a.Wo); a.dHo = make_fastdiv((unsigned)a.Ho);
  a.dcpp = make_fastdiv((unsigned)a.cpp); a.dKW = make_fastdiv((unsigned)KW);
  a.xrs = a.cpp; a.wrs = a.Kc; a.bx = a.bw = a.by = 0;
#ifdef CDDMSL_TILE_STAMPS
  a.tstamps = g_tile_stamps;
#endif
  if (a.M == 0) return CDDMSL_OK;
  a.nt_out = nt_out_for((long)a.M * Cout * 2);
  if (y8) {       // e4m3 second output: bf16 output of bf16 or e4m3 operands, dense rows
    if (op == OP_F32 || (out_f32 & 1) || ldy != Cout) return CDDMSL_ERR_ARG;
    a.y8 = (char*)y8; a.q8 = q8; a.amax8 = (unsigned*)amax8;
  }
  return CDDMSL_OK;
}

// fill, plan, launch of the three convolution entry points
static int conv_fwd_any(Operand op, const void* x, const void* w, void* y, const float* scale, const float* bias,
                        const void* residual, const void* relu_mask, int Nimg, int Hi, int Wi, int Cin,
                        int Cout, int KH, int KW, int stride, int pad, int pool, int ldy, int ldr, int ldm,
                        int relu, int out_f32, void* y8, const float* q8, float* amax8, void* stream) {
  ConvArgs a;
  const int st = fill_conv(a, op, x, w, y, scale, bias, residual, relu_mask, Nimg, Hi, Wi, Cin, Cout, KH, KW, stride, pad, pool, ldy, ldr, ldm,
                           relu, out_f32, y8, q8, amax8);
  if (st != CDDMSL_OK || a.M == 0) return st;
  return run_fwd(a, op, plan_fwd(a, op, 1), stream);
}

extern "C" int cddmsl_conv_fwd(const void* x, const void* w, void* y, const float* scale, const float* bias,
                               const void* residual, const void* relu_mask, int Nimg, int Hi, int Wi, int Cin,
                               int Cout, int KH, int KW, int stride, int pad, int pool, int ldy, int ldr, int ldm,
                               int relu, int out_f32, int dtype, void* stream) {
  if (dtype != 0 && dtype != 1) return CDDMSL_ERR_ARG;
  return conv_fwd_any((Operand)dtype, x, w, y, scale, bias, residual, relu_mask, Nimg, Hi, Wi, Cin, Cout, KH, KW, stride, pad, pool, ldy, ldr, ldm,
                      relu, out_f32, nullptr, nullptr, nullptr, stream);
}

// The stem's third convolution with the AvgPool2d(2) behind it in one launch: y [Nimg][Hi/2][Wi/2][64] = avgpool2(relu(bn(conv3x3(x)))),
// bit-identical to cddmsl_conv_fwd (pad 1, FrozenBN + ReLU) followed by cddmsl_avgpool2_fwd.  Only what that layer is: bf16, 32 -> 64
// channels, stride 1, scale and bias given, no mask (stride / relu_mask / dtype are arguments so that anything else is REFUSED here
// instead of silently computed another way).
extern "C" int cddmsl_conv3x3_pool_fwd(const void* x, const void* w, void* y, const float* scale, const float* bias, const void* relu_mask,
                                       int Nimg, int Hi, int Wi, int Cin, int Cout, int stride, int dtype, void* stream) {
  if (dtype != 0 || Cin != 32 || Cout != 64 || stride != 1 || relu_mask || !scale || !bias || Hi < 2 || Wi < 2) return CDDMSL_ERR_ARG;
  ConvArgs a;
  const int st = fill_conv(a, OP_BF16, x, w, y, scale, bias, nullptr, nullptr, Nimg, Hi, Wi, Cin, Cout, 3, 3, 1, 1, 0, Cout, 0, 0, 1, 0,
                           nullptr, nullptr, nullptr);
  if (st != CDDMSL_OK || a.M == 0) return st;
  // (buffer addressing: the input and the pooled output each below 2 GiB)
  if ((long)Nimg * Hi * Wi * Cin * 2 >= 0x7ffff000L || (long)Nimg * (a.Ho / 2) * (a.Wo / 2) * Cout * 2 >= 0x7fffffffL) return CDDMSL_ERR_ARG;
  a.pool_out = 1;
  a.dWp = make_fastdiv((unsigned)(a.Wo / 2)); a.dHp = make_fastdiv((unsigned)(a.Ho / 2));
  const Plan pl = plan_fwd(a, OP_BF16, 1);
  if (pl.kernel != 8) return CDDMSL_ERR_ARG;
  return run_fwd(a, OP_BF16, pl, stream);
}

// cddmsl_conv_fwd (bf16) that ALSO writes y8 [M][Cout] = OCP e4m3 of sat(y * q8[0]) and max-es |y| into amax8[0..63] (64 floats,
// spread by block to keep the atomics off one address): the producer side of the fp8 configuration -- the convolution that
// consumes y reads y8 instead of a separate quantisation pass.  Only launches the 256x256 kernel takes (CDDMSL_ERR_ARG otherwise:
// the caller asks cddmsl_conv_fwd_q8_ok first).
extern "C" int cddmsl_conv_fwd_q8(const void* x, const void* w, void* y, const float* scale, const float* bias,
                                  const void* residual, const void* relu_mask, int Nimg, int Hi, int Wi, int Cin,
                                  int Cout, int KH, int KW, int stride, int pad, int relu, void* y8, const float* q8, float* amax8,
                                  void* stream) {
  if (!y8) return CDDMSL_ERR_ARG;
  return conv_fwd_any(OP_BF16, x, w, y, scale, bias, residual, relu_mask, Nimg, Hi, Wi, Cin, Cout, KH, KW, stride, pad, 0, Cout, Cout, Cout,
                      relu, 0, y8, q8, amax8, stream);
}

// e4m3 x e4m3 -> bf16 (or f32) on the 256x256 kernel: x [Nimg][Hi][Wi][Cin] and w [Cout][KH][KW][Cin] hold OCP e4m3 bytes (Cin a
// multiple of 128), everything else as cddmsl_conv_fwd with dtype 0: scale / bias f32 per output channel (the caller folds the two
// per-tensor dequantisation factors into ``scale``), residual / relu_mask / y bf16 (y f32 with out_f32).  Only shapes the 256x256
// kernel takes (Cout % 256 == 0, <= 31 taps, "same" padding at most); anything else is CDDMSL_ERR_ARG -- there is no fallback.
extern "C" int cddmsl_conv_fwd_fp8(const void* x, const void* w, void* y, const float* scale, const float* bias,
                                   const void* residual, const void* relu_mask, int Nimg, int Hi, int Wi, int Cin, int Cout, int KH,
                                   int KW, int pad, int relu, int out_f32, void* y8, const float* q8, float* amax8, void* stream) {
  if (Cin % 128 != 0 || (out_f32 & ~1)) return CDDMSL_ERR_ARG;
  return conv_fwd_any(OP_FP8, x, w, y, scale, bias, residual, relu_mask, Nimg, Hi, Wi, Cin, Cout, KH, KW, 1, pad, 0, Cout, Cout, Cout,
                      relu, out_f32, y8, q8, amax8, stream);
}

// The 256x256 wgrad kernel takes bf16 "same" problems with whole 256-wide output tiles and 8-chunk-aligned pixels
// (so the two X halves of a lane share one filter tap).  CDDMSL_GEMM256 as for the forward kernel (0 = never, 2 = always).
static bool wgrad256_ok(const WgradArgs& a, int batch) {
  const long mode = env_int("CDDMSL_GEMM256", 1);
  if (mode == 0) return false;
  if ((a.Cout & 255) || (a.K & 255) || (a.cpp & 7) || (a.ldd & 7)) return false;
  if (mode == 2) return true;
  // long reductions only: each block ends with 64 Ki scalar atomics, which a short m range cannot amortise
  // (threshold from per-shape A/B inside the training step: 9342 (M 66400, 256 x 2304) and 14112 (M 25088, 512 x 4608) run
  // 1.6x faster here than on the 128x128 kernel, 8300 (M 265600, 512 x 256) and everything below run slower)
  return (long)(a.Cout / 256) * (a.K / 256) * batch * ((a.M + WM - 1) / WM) >= env_int("CDDMSL_WGRAD256_MIN", 4000);      // (A/B knob)
}
// buffer addressing of the 256x256 wgrad kernels: lane offset + soffset must stay below 2 GiB inside one block's reduction range
// (row_bytes: the longer of a dy row and an x pixel row)
static bool wgrad256_span_ok(int mtiles_per_split, int Wi, long row_bytes) {
  return ((long)mtiles_per_split * WM + WM + 2L * Wi + 2) * row_bytes + (1L << 20) < (1L << 31);
}

// ---- plan, weight gradient
// `*splits` blocks over total_mt reduction tiles -> tiles per block; *splits becomes the number of blocks that then have work
static int even_split(int total_mt, long* splits) {
  const int mps = (int)((total_mt + *splits - 1) / *splits);
  *splits = (total_mt + mps - 1) / mps;
  return mps;
}

// Split count of the 128x128 kernels: one round of blocks (2 per CU) for 1x1 layers, two for filters with taps, and at least 8 m-tiles
// per block.  Every block ends with 16 Ki f32 atomics; with 2048+ blocks the atomic traffic at L2, not the reduction, set the
// time of the short backbone layers (measured: 150 -> 67 us at M = 66 400, N = 1024, K = 256).
// ... and a WHOLE number of 512-block rounds (two resident blocks per CU): with 9 output tiles (128 x 1152) a target of 1024
// gave 114 splits = 1026 blocks, i.e. a third round for two blocks.  Candidates: the largest split count that stays inside
// r rounds, r = the target's rounds and one more; the one whose last round is fullest wins (fewer rounds on ties).
// (Not the search of split_256_rounds: the candidates are clamped to 1 instead of skipped, and the fill is that of the blocks
// left after even_split.)
static long split_512_rounds(long tiles, int total_mt, bool taps) {
  bool forced;
  const long target = env_int("CDDMSL_WGRAD_BLOCKS", taps ? 1024 : 512, &forced);   // tuning knob (A/B runs): target number of blocks
  const long maxs = (total_mt + 7) / 8;
  long splits = 1;
  const long r0 = (target + 511) / 512;
  double best = -1.0;
  for (long r = r0; r <= r0 + 1; ++r) {
    long c = (512 * r) / tiles;
    if (c < 1) c = 1;
    if (c > maxs) c = maxs;
    long real = c;
    even_split(total_mt, &real);
    const long blocks = tiles * real, rounds = (blocks + 511) / 512;
    const double eff = (double)blocks / (512.0 * rounds);
    if (eff > best + 0.03) { best = eff; splits = c; }
    if (c == maxs) break;
  }
  if (forced) { splits = (target + tiles - 1) / tiles; if (splits > maxs) splits = maxs; }
  return splits < 1 ? 1 : splits;
}

// Split count of the 256x256 ping-pong kernels: ONE block per CU, so the grid should be a whole number of 256-block rounds: take
// the split count whose grid fills its last round best (fewest rounds on ties: every block ends with 64 Ki atomics), with at
// least 16 reduction tiles per block.  Measured on N = 2048, K = 512: 256 blocks 683 us vs 640 blocks 894 us.
static long split_256_rounds(long tiles, int total_mt) {
  const long maxs = (total_mt + 15) / 16;
  long sp = 1;
  double best = -1.0;
  for (int r = 1; r <= 6; ++r) {
    long c = (256L * r) / tiles;
    if (c < 1) continue;
    if (c > maxs) c = maxs;
    const long blocks = tiles * c, rounds = (blocks + 255) / 256;
    const double eff = (double)blocks / (256.0 * rounds);
    if (eff > best + 0.02) { best = eff; sp = c; }
    if (c == maxs) break;
  }
  return sp;
}

static Plan plan_wgrad(const WgradArgs& a, Operand op, int batch) {
  const int es = elem_size(op), total_mt = (a.M + WM - 1) / WM;
  const long tiles256 = (long)(a.Cout / 256) * (a.K / 256);
  const long row_bytes = (long)a.ldd * es > a.xrs * 16L ? (long)a.ldd * es : a.xrs * 16L;
  if (op == OP_FP8) {                                           // k_wgrad256_f8 or nothing (the entry point has checked the shape)
    long sp = split_256_rounds(tiles256, total_mt);
    const int mps = even_split(total_mt, &sp);
    if (!wgrad256_span_ok(mps, a.Wi, row_bytes)) return {};
    return {12, (unsigned)(tiles256 * sp), 1, (int)sp, mps};
  }
  const int cols = 256 / es;
  const long tiles = (long)((a.Cout + cols - 1) / cols) * ((a.K + cols - 1) / cols);
  long splits = split_512_rounds(tiles, total_mt, !(a.KH == 1 && a.KW == 1));
  const int mps = even_split(total_mt, &splits);
  if (tiles * splits > 0x7fffffffL) return {};
  const bool same = !a.pool && a.stride == 1 && a.Ho == a.Hi && a.Wo == a.Wi;   // LDS-DMA kernel: output pixel == input pixel
  if (same && op == OP_BF16 && wgrad256_ok(a, batch)) {
    bool forced;
    const long want = env_int("CDDMSL_WGRAD256_BLOCKS", 0, &forced);            // tuning knob (A/B runs): force ~this many blocks
    const long maxs = (total_mt + 15) / 16;
    long sp = forced ? (want + tiles256 - 1) / tiles256 : split_256_rounds(tiles256, total_mt);
    if (sp > maxs) sp = maxs;
    if (sp < 1) sp = 1;
    const int mps256 = even_split(total_mt, &sp);
    if (wgrad256_span_ok(mps256, a.Wi, row_bytes)) return {6, (unsigned)(tiles256 * sp), 1, (int)sp, mps256};
  }
  return {same ? 5 : 4, (unsigned)(tiles * splits), 1, (int)splits, mps};
}

extern "C" int cddmsl_set_workspace(void* ptr, long bytes) {
  if (bytes < 0 || (ptr == nullptr && bytes != 0) || ((size_t)ptr & 15)) return CDDMSL_ERR_ARG;
  g_ws = ptr; g_ws_bytes = bytes;
  return CDDMSL_OK;
}

// ---- launch, weight gradient: the kernels live in conv_wgrad.hip (4, 5, 6, 12)
static int run_wgrad(WgradArgs& a, Operand op, const Plan& p, void* stream) {
  if (p.kernel == 0) return CDDMSL_ERR_ARG;
  g_last_kernel = p.kernel;
  if (g_plan_only) return CDDMSL_OK;
  a.mtiles_per_split = p.mtiles_per_split;
  launch_wgrad(a, p, op, (hipStream_t)stream, g_ws, g_ws_bytes);
  return launch_status();
}

// ---- fill, weight gradient: validates the arguments and builds the kernel arguments of a convolution's weight gradient (a.M == 0
// with CDDMSL_OK: nothing to do); x / dy are `op`.  The split (mtiles_per_split) is the plan's.
static int fill_wgrad(WgradArgs& a, Operand op, const void* x, const void* dy, float* dw, const float* scale, int Nimg, int Hi,
                      int Wi, int Cin, int Cout, int KH, int KW, int stride, int pad, int pool, int ldd) {
  const int es = elem_size(op);
  if (Nimg < 0 || Hi <= 0 || Wi <= 0 || Cin <= 0 || Cout <= 0 || KH <= 0 || KW <= 0 || stride <= 0) return CDDMSL_ERR_ARG;
  if ((Cin * es) % 16 != 0 || (Cout * es) % 16 != 0 || (ldd * es) % 16 != 0) return CDDMSL_ERR_ARG;
  if (pool && (KH != 1 || KW != 1 || pad != 0 || stride != 1)) return CDDMSL_ERR_ARG;
  a.x = (const char*)x; a.dy = (const char*)dy; a.dw = dw; a.scale = scale;
  a.Nimg = Nimg; a.Hi = Hi; a.Wi = Wi; a.Cin = Cin; a.Cout = Cout; a.KH = KH; a.KW = KW; a.stride = stride; a.pad = pad;
  a.ldd = ldd; a.pool = pool;
  if (pool) { a.Ho = Hi / 2; a.Wo = Wi / 2; }
  else { a.Ho = (Hi + 2 * pad - KH) / stride + 1; a.Wo = (Wi + 2 * pad - KW) / stride + 1; }
  if (a.Ho <= 0 || a.Wo <= 0) return CDDMSL_ERR_ARG;
  long M = (long)Nimg * a.Ho * a.Wo;
  if (M > 0x7fffff00L) return CDDMSL_ERR_ARG;
  a.M = (int)M; a.cpp = Cin * es / 16; a.Kc = KH * KW * a.cpp; a.K = KH * KW * Cin; a.ncc = Cout * es / 16;
  a.mtiles_per_split = 0;
  a.dWo = make_fastdiv((unsigned)a.Wo); a.dHo = make_fastdiv((unsigned)a.Ho);
  a.xrs = a.cpp; a.ldo = a.K; a.direct = 0; a.bx = a.bd = a.bo = 0;
#ifdef CDDMSL_TILE_STAMPS
  a.tstamps = g_tile_stamps;
#endif
  return CDDMSL_OK;
}

extern "C" int cddmsl_conv_wgrad(const void* x, const void* dy, float* dw, const float* scale, int Nimg, int Hi,
                                 int Wi, int Cin, int Cout, int KH, int KW, int stride, int pad, int pool, int ldd,
                                 int dtype, void* stream) {
  if (dtype != 0 && dtype != 1) return CDDMSL_ERR_ARG;
  WgradArgs a;
  const int st = fill_wgrad(a, (Operand)dtype, x, dy, dw, scale, Nimg, Hi, Wi, Cin, Cout, KH, KW, stride, pad, pool, ldd);
  if (st != CDDMSL_OK || a.M == 0) return st;
  return run_wgrad(a, (Operand)dtype, plan_wgrad(a, (Operand)dtype, 1), stream);
}

// fp8 configuration: dW[Cout][KH*KW*Cin] (f32) += scale[n] * sum_m dy8[m][n] * im2col(x8)[m][k], both operands OCP e4m3 bytes (NHWC, dy
// rows ldd bytes apart); ``scale`` must carry the two dequantisation factors (x the FrozenBN scale).  "Same" convolutions only
// (stride 1, 2 * pad == KH - 1), Cout, Cin multiples of 256.  cddmsl_conv_wgrad_fp8_ok tells whether a shape is taken.
extern "C" int cddmsl_conv_wgrad_fp8_ok(int Cin, int Cout, int KH, int KW, int pad, int ldd) {
  return (Cin % 256 == 0 && Cout % 256 == 0 && KH == KW && (KH & 1) && 2 * pad == KH - 1 && ldd % 16 == 0) ? 1 : 0;
}
extern "C" int cddmsl_conv_wgrad_fp8(const void* x8, const void* dy8, float* dw, const float* scale, int Nimg, int Hi, int Wi, int Cin,
                                     int Cout, int KH, int KW, int pad, int ldd, void* stream) {
  if (!cddmsl_conv_wgrad_fp8_ok(Cin, Cout, KH, KW, pad, ldd) || ldd < Cout) return CDDMSL_ERR_ARG;
  WgradArgs a;
  const int st = fill_wgrad(a, OP_FP8, x8, dy8, dw, scale, Nimg, Hi, Wi, Cin, Cout, KH, KW, 1, pad, 0, ldd);
  if (st != CDDMSL_OK || a.M == 0) return st;
  return run_wgrad(a, OP_FP8, plan_wgrad(a, OP_FP8, 1), stream);
}

// Batched "NT" GEMM on the conv kernel: for b in [0,batch): C_b[m][n] = sum_k A_b[m][k] * B_b[n][k] (+ bias[n]),
// A_b = a + b*sa, rows lda apart; B_b = w + b*sw, rows ldb apart; C_b = c + b*sc, rows ldc apart (strides in ELEMENTS).
// Used by the reassociated attention pool (per-head and per-region products).
extern "C" int cddmsl_gemm_nt_batched(const void* a, const void* w, void* c, const float* bias, int M, int N, int K, int lda,
                                      int ldb, int ldc, int batch, long sa, long sw, long sc, int out_f32, int dtype, void* stream) {
  int es = dtype == 0 ? 2 : 4;
  if (dtype != 0 && dtype != 1) return CDDMSL_ERR_ARG;
  if (M < 0 || N <= 0 || K <= 0 || batch < 0 || batch > 65535) return CDDMSL_ERR_ARG;
  if ((K * es) % 16 || (lda * es) % 16 || (ldb * es) % 16 || (sa * es) % 16 || (sw * es) % 16) return CDDMSL_ERR_ARG;
  if (M == 0 || batch == 0) return CDDMSL_OK;
  // a 1x1 convolution of one 1 x M image, K -> N channels, with the operand rows and the batches at the caller's strides.  Shares
  // fill_conv; what a convolution never has is set here.  (nt_out: batched outputs keep the default store policy.)
  const Operand op = (Operand)dtype;
  ConvArgs p;
  const int st = fill_conv(p, op, a, w, c, nullptr, bias, nullptr, nullptr, 1, 1, M, K, N, 1, 1, 1, 0, 0, ldc, 0, 0, 0, out_f32 ? 1 : 0,
                           nullptr, nullptr, nullptr);
  if (st != CDDMSL_OK) return st;
  p.xrs = lda * es / 16; p.wrs = ldb * es / 16;
  p.bx = sa * es; p.bw = sw * es; p.by = sc * (out_f32 ? 4 : es);
  p.nt_out = 1;
  return run_fwd(p, op, plan_fwd(p, op, batch), stream);
}

// ---- the batched TN GEMM: its own plan (kernels 9, 7, 5) and launch
// k_gemm_tn_small's grid over kt 128-column K-tiles and `batch` batches: -> gridDim.y, *bpb = batches per block
static unsigned tn_small_grid(long kt, long batch, int* bpb) {
  long b = (kt * batch + 4095) / 4096;
  if (b < 8) b = 8;
  if (b > batch) b = batch;
  *bpb = (int)b;
  return (unsigned)((batch + b - 1) / b);
}

static Plan plan_gemm_tn(const WgradArgs& p, Operand op, int batch, int mode) {
  const int cols = 256 / elem_size(op), M = p.M, N = p.Cout, K = p.K;
  const long tiles = (long)((N + cols - 1) / cols) * ((K + cols - 1) / cols);
  const int total_mt = (M + WM - 1) / WM;
  if (op == OP_BF16 && total_mt == 1 && N <= 64 && batch >= 64 && K % 128 == 0 && N % 8 == 0) {
    // one reduction tile, narrow output (the attention pool's per-region products): compact three-stage ring
    Plan p = {9, (unsigned)(K / 128), 0};
    p.gy = tn_small_grid(K / 128, batch, &p.bpb);
    return p;
  }
  if (total_mt <= 4 && batch >= 64) {
    // short reductions over many batches: stream runs of batches through one block (k_gemm_tn_stream)
    long bpb = (tiles * batch + 4095) / 4096, minb = (8 + total_mt - 1) / total_mt;
    if (bpb < minb) bpb = minb;
    if (bpb > batch) bpb = batch;
    return {7, (unsigned)tiles, (unsigned)((batch + bpb - 1) / bpb), 0, 0, (int)bpb};
  }
  long splits = 1;
  if (mode == 0) {                                              // (the stores of modes 1 / 2 need one block per tile)
    const long want = (2048 + tiles * batch - 1) / (tiles * batch), maxs = (total_mt + 7) / 8;
    splits = want < 1 ? 1 : (want > maxs ? maxs : want);
    if (splits < 1) splits = 1;
  }
  const int mps = even_split(total_mt, &splits);
  if (tiles * splits > 0x7fffffffL) return {};
  return {5, (unsigned)(tiles * splits), (unsigned)batch, (int)splits, mps};
}

// Batched "TN" GEMM on the LDS-DMA wgrad kernel: out_b[n][k] (+)= sum_m A_b[m][n] * B_b[m][k]; A rows lda apart (n contiguous),
// B rows ldb apart (k contiguous), out rows ldo apart.  mode 0: f32 atomic accumulate (large M is split over blocks),
// 1: f32 store, 2: `dtype` store (modes 1/2 need M <= 64*8 so one block owns a tile... enforced: single split).
extern "C" int cddmsl_gemm_tn_batched(const void* a, const void* b, void* out, int M, int N, int K, int lda, int ldb, int ldo,
                                      int batch, long sa, long sb, long so, int mode, int dtype, void* stream) {
  int es = dtype == 0 ? 2 : 4;
  if (dtype != 0 && dtype != 1) return CDDMSL_ERR_ARG;
  if (M <= 0 || N <= 0 || K <= 0 || batch <= 0 || batch > 65535 || mode < 0 || mode > 2) return CDDMSL_ERR_ARG;
  if ((K * es) % 16 || (N * es) % 16 || (lda * es) % 16 || (ldb * es) % 16 || (sa * es) % 16 || (sb * es) % 16) return CDDMSL_ERR_ARG;
  // the weight gradient of a 1x1 convolution of one 1 x M image (x = B, dy = A), with rows, batches and output at the caller's
  // strides.  Shares fill_wgrad; what a convolution never has is set here.
  const Operand op = (Operand)dtype;
  WgradArgs p;
  const int fs = fill_wgrad(p, op, b, a, (float*)out, nullptr, 1, 1, M, K, N, 1, 1, 1, 0, 0, lda);
  if (fs != CDDMSL_OK) return fs;
  p.xrs = ldb * es / 16; p.ldo = ldo; p.direct = mode;
  p.bx = sb * es; p.bd = sa * es; p.bo = so * (mode == 2 ? es : 4);
  const Plan pl = plan_gemm_tn(p, op, batch, mode);
  if (pl.kernel == 0) return CDDMSL_ERR_ARG;
  g_last_kernel = pl.kernel;
  if (g_plan_only) return CDDMSL_OK;
  p.mtiles_per_split = pl.mtiles_per_split;
  launch_gemm_tn(p, op, pl, batch, mode, (hipStream_t)stream);
  return launch_status();
}

// dx [K][P][C] (bf16) and gpos [P+1][C] (f32, accumulated; nullable) of the CLIP attention pool from  pds [K][2H][TP] = [p ; ds]
// and  zu [K][2H][C] = [dZ ; U]  (cddmsl_amd/layers.py AttnPoolFn.backward; clip_backbone.py:83-107):  one batched TN product whose
// epilogue finishes the token gradients (see k_gemm_tn_small MODE 3).  g0 [K][C] f32 = the query path's gradient of the mean token;
// mbits [K][C] = sign bits of the pooled map per column (bit t = pixel t kept), all ones when the map is not a ReLU output.
extern "C" int cddmsl_attnpool_dx(const void* pds, const void* zu, const float* g0, const unsigned long long* mbits, void* dx, float* gpos,
                                  int K, int H2, int P, int TP, int C, int dtype, void* stream) {
  if (dtype != 0 || K < 0 || P != 49 || TP != 56 || H2 <= 0 || H2 > 64 || (H2 & 7) || C <= 0 || (C & 127) || !g0 || !mbits || !dx) return CDDMSL_ERR_ARG;
  if (K == 0) return CDDMSL_OK;
  if (K > 65535 * 8) return CDDMSL_ERR_ARG;
  // the batched TN product of cddmsl_gemm_tn_batched's kernel 9 (M = H2, N = TP, K = C, dense operands) with the MODE 3 epilogue
  WgradArgs p;
  const int fs = fill_wgrad(p, OP_BF16, zu, pds, (float*)dx, nullptr, 1, 1, H2, C, TP, 1, 1, 1, 0, 0, TP);
  if (fs != CDDMSL_OK) return fs;
  p.direct = 3;
  p.bx = (long)H2 * C * 2; p.bd = (long)H2 * TP * 2; p.bo = (long)P * C * 2;
  p.g0 = g0; p.mbits = mbits; p.gpos = gpos;
  int bpb;
  const unsigned gy = tn_small_grid(C / 128, K, &bpb);
  launch_attnpool_dx(p, (unsigned)(C / 128), gy, K, bpb, (hipStream_t)stream);
  return launch_status();
}

extern "C" int cddmsl_weight_prep_multi(const long long* table, int count, int dtype, void* stream) {
  if ((dtype != 0 && dtype != 1) || count < 0 || count > 65535) return CDDMSL_ERR_ARG;
  if (count == 0) return CDDMSL_OK;
  if (dtype == 0) hipLaunchKernelGGL(k_weight_prep_multi<__bf16>, dim3(256, (unsigned)count), dim3(256), 0, (hipStream_t)stream, table);
  else hipLaunchKernelGGL(k_weight_prep_multi<float>, dim3(256, (unsigned)count), dim3(256), 0, (hipStream_t)stream, table);
  return launch_status();
}

extern "C" int cddmsl_weight_prep(const float* w, const float* scale, void* w_fwd, void* w_dgrad, int Cout, int KH,
                                  int KW, int Cin, int dtype, void* stream) {
  if (dtype != 0 && dtype != 1) return CDDMSL_ERR_ARG;
  long n = (long)Cout * KH * KW * Cin;
  if (n <= 0) return n == 0 ? CDDMSL_OK : CDDMSL_ERR_ARG;
  const long tiles = (long)((Cout + 31) / 32) * KH * KW * ((Cin + 31) / 32);         // 32 x 32 tiles per tap
  unsigned grid = (unsigned)(tiles > 4096 ? 4096 : tiles);
  if (dtype == 0) hipLaunchKernelGGL(k_weight_prep<__bf16>, dim3(grid), dim3(256), 0, (hipStream_t)stream, w, scale, (char*)w_fwd, (char*)w_dgrad, Cout, KH, KW, Cin);
  else hipLaunchKernelGGL(k_weight_prep<float>, dim3(grid), dim3(256), 0, (hipStream_t)stream, w, scale, (char*)w_fwd, (char*)w_dgrad, Cout, KH, KW, Cin);
  return launch_status();
}
