// Forward convolution / NT GEMM kernels on the 256x256 tile (kernel id 3; 10 with e4m3 operands), its split-K tail, and the 256x128
// two-workgroup kernel (kernel id 11).  Data layout: see gemm_conv.hip.
#include "gemm_common.h"
#include <type_traits>

namespace {

__device__ __forceinline__ unsigned pack4_e4m3(float a, float b, float c, float d) {
  a = __builtin_amdgcn_fmed3f(a, -448.f, 448.f); b = __builtin_amdgcn_fmed3f(b, -448.f, 448.f);       // e4m3fn has no infinity: saturate
  c = __builtin_amdgcn_fmed3f(c, -448.f, 448.f); d = __builtin_amdgcn_fmed3f(d, -448.f, 448.f);
  int w = __builtin_amdgcn_cvt_pk_fp8_f32(a, b, 0, false);
  w = __builtin_amdgcn_cvt_pk_fp8_f32(c, d, w, true);
  return (unsigned)w;
}

// OCP e4m3 operands (BASELINE.json configs[4]): a 16-byte chunk holds 16 elements, one block-scaled
// v_mfma_scale_f32_32x32x64_f8f6f4 (E8M0 scales fixed at 2^0: per-tensor scales are folded into the epilogue's per-channel scale by
// the host) consumes TWO chunks per lane = 64 elements of K: twice the K per matrix-pipe cycle of the bf16 form.  The epilogue
// (output, residual, ReLU mask) stays bf16: ES below is the epilogue's element size.  Lane half h of a step holds chunks
// (2s' + h) for s' in the step's pair -- the same bytes for A and B, which is all a dot product needs.
struct fp8e4 { unsigned char v; };
template <> struct Mma<fp8e4> {
  static constexpr int ES = 2;
  __device__ static __forceinline__ void step2(f32x16& acc, const u32x4& a0, const u32x4& a1, const u32x4& b0, const u32x4& b1) {
    const i32x8 a = {(int)a0[0], (int)a0[1], (int)a0[2], (int)a0[3], (int)a1[0], (int)a1[1], (int)a1[2], (int)a1[3]};
    const i32x8 b = {(int)b0[0], (int)b0[1], (int)b0[2], (int)b0[3], (int)b1[0], (int)b1[1], (int)b1[2], (int)b1[3]};
    acc = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a, b, acc, 0, 0, 0, 0x7f7f7f7f, 0, 0x7f7f7f7f);
  }
};
// one 64x32 quadrant of a K-tile (4 chunk pairs per row): two row tiles x the tile's k-steps
template <typename T> struct MmaQuad {
  __device__ static __forceinline__ void run(f32x16& c0, f32x16& c1, const u32x4 (*fa)[4], const u32x4* fb) {
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      Mma<T>::step(c0, fa[0][ks], fb[ks]);
      Mma<T>::step(c1, fa[1][ks], fb[ks]);
    }
  }
};
template <> struct MmaQuad<fp8e4> {
  __device__ static __forceinline__ void run(f32x16& c0, f32x16& c1, const u32x4 (*fa)[4], const u32x4* fb) {
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      Mma<fp8e4>::step2(c0, fa[0][2 * s], fa[0][2 * s + 1], fb[2 * s], fb[2 * s + 1]);
      Mma<fp8e4>::step2(c1, fa[1][2 * s], fa[1][2 * s + 1], fb[2 * s], fb[2 * s + 1]);
    }
  }
};

// ------------------------------------------------------------------------------------------------
// 256x256 tile, 8 waves (2 x 4; 128x64 per wave), two wave groups ping-ponging on each SIMD.
//
// The 128x128 kernel above tops out near 1 PFLOP/s: both of its blocks on a CU stall at the same two barriers per
// K-tile.  Here each SIMD hosts one wave of group 0 (wr = 0) and one of group 1 (wr = 1), group 1 running ONE barrier
// behind: between two consecutive barriers one group issues LDS reads + LDS-DMA for its next quadrant while the other
// runs that quadrant's MFMAs, so the matrix pipe always has a wave feeding it.  A K-tile (8 chunks) is four phases,
// one 64x32 quadrant of the wave's 128x64 output each:
//     phase 1  read B0            MFMA q00   stage A1 of the OTHER buffer with tile kt+1 (read in the previous phase 3)
//     phase 2  read B1            MFMA q01   stage A0 of this buffer with tile kt+2   (read in the previous phase 4)
//     phase 3  read A1            MFMA q11   stage B0 (read in phase 1), s_waitcnt vmcnt(4)
//     phase 4  read A0 of kt+1    MFMA q10   stage B1 (read in phase 2)
// Each half-tile (128 rows x 128 B: sub-tile i of both row groups / sub-tile j of all four column groups) is restaged
// TWO phases after its last read: a phase's reads are retired (lgkmcnt(0), placed after the barrier so the LDS latency
// overlaps the wait for the other group's MFMAs) before its MFMAs, i.e. before the barrier that opens the next phase,
// which every wave passes before the phase after that issues its DMA -- for both groups despite the one-barrier stagger.
// The phase-3 wait leaves the two youngest half-tiles (4 DMAs per thread) in flight and retires every older one: all
// of tile kt+1, whose first read (A0, phase 4) comes after that phase's barrier.
// LDS: [2 buffers][A|B][2 halves][128 rows x 8 chunks] = 128 KiB, swizzled like the 128x128 kernel.
// Sources are buffer-addressed (buffer_load_dwordx4 ... offen lds): per-block base in SGPRs, a per-lane byte offset that
// is constant over the K loop, and the running K / filter-tap position in the wave-uniform soffset -- the loop carries
// no per-lane address arithmetic.  Filter-tap validity is a per-row bit mask (KH*KW <= 31 bits): an out-of-image tap or
// an out-of-range row sets bit 31 of the lane's offset, which the range check turns into zeros written to LDS.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ void blds16(__amdgpu_buffer_rsrc_t r, unsigned voff, unsigned soff, void* l) {
  __builtin_amdgcn_raw_ptr_buffer_load_lds(r, (__attribute__((address_space(3))) void*)l, 16, (int)voff, (int)soff, 0, 0);
}

// ------------------------------------------------------------------------------------------------
// Epilogue of a wave's 128 x 64 accumulator tile (acc[4][2] of 32x32 blocks; rows m0 + 128 wr ..., columns n0 + 64 wc ...), shared by
// the 256x256 kernel and the 256x128 two-workgroup kernel.
// Per-wave LDS transpose (32 rows x 64 cols f32 per pass; DS ops of one wave execute in order, so no barrier
// is needed); a lane then owns 8 consecutive columns of a row: 16-byte residual / mask loads and y stores.  All of them are
// buffer-addressed -- rows past M fall outside num_records (loads give 0, stores are dropped), an absent residual / mask is
// a zero-sized buffer, per-lane offsets are computed once and the row / pass position is the wave-uniform soffset -- so the
// passes are straight-line code without per-row exec masks, zero fills or 64-bit address arithmetic.
// The transposition is double-buffered in the wave's private 16 KiB of the (now idle) operand ring: pass a+1's 32 scratch
// writes are issued right behind pass a's 8 scratch reads (all four rows at once), so the write drain and the read latency
// are each paid once per pass and overlap the arithmetic and stores of the pass before -- tools/tile_stamps.py measured the
// former row-at-a-time form (read two chunks, wait, compute, store, scheduling barrier) at 7.4 us per tile without and
// 11 us with a residual, against ~1 us of vector-ALU work.
// `ep`: 16 KiB of LDS private to the wave.
// ------------------------------------------------------------------------------------------------
// PRE: the rows of the first two passes of ONE operand (the residual if there is one, else the ReLU mask) were requested by the caller
// -- the 256x256 kernel issues them in phase 3 of the tile's last K-tile, into the registers the A0 fragments no longer need -- and
// arrive in `pre`.
// `sb` (optional): this lane's 8 scale and 8 bias values, requested by the caller ahead of time (phase 4 of the last K-tile).
template <typename T, bool RPOOL, int EPI, bool PRE = false>
__device__ __forceinline__ void tile_epilogue(const ConvArgs& p, f32x16 (&acc)[4][2], float* ep, int wr, int wc, int lane, int m0, int n0,
                                              const u32x4 (*pre)[4] = nullptr, const f32x4* sb = nullptr) {
  constexpr int ES = Mma<T>::ES;
  const int r32 = lane & 31, hh = lane >> 5;
  const int cg = lane & 7, rr = lane >> 3;
  const int n = n0 + wc * 64 + cg * 8;
  float sc[8], bi[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    if (sb) { sc[j] = sb[j >> 2][j & 3]; bi[j] = sb[2 + (j >> 2)][j & 3]; }
    else { sc[j] = p.scale ? p.scale[n + j] : 1.f; bi[j] = p.bias ? p.bias[n + j] : 0.f; }
  }
  const bool has_res = EPI < 0 ? p.residual != nullptr : (EPI & 1) != 0;
  const bool has_msk = EPI < 0 ? p.relu_mask != nullptr : (EPI & 2) != 0;
  const bool f32out = EPI < 0 && (ES == 4 || p.out_f32 != 0);
  const int eso = f32out ? 4 : 2;
  const float relu_floor = p.relu ? 0.f : -__builtin_inff();
  const long rows = p.M - m0;
  auto mk = [&](const char* base, long ld, int es) {
    long bytes = rows * ld * es;
    if (bytes > 0x7fffffffL) bytes = 0x7fffffffL;
    return __builtin_amdgcn_make_buffer_rsrc((void*)(base + (long)m0 * ld * es), 0, base ? (int)bytes : 0, 0x00020000);
  };
  const bool rf32 = EPI < 0 && ES == 2 && p.res_f32;         // f32 residual rows on the bf16 kernel (the mapper's f32 residual stream)
  const int esr = rf32 ? 4 : ES;
  // (pooled residual: addressed from the tensor base -- the pooled pixel of a row is not linear in the row)
  const __amdgpu_buffer_rsrc_t ry = mk(p.y, p.ldy, eso), rmsk = mk(p.relu_mask, p.ldm, ES);
  // RPOOL is a template parameter, not a run-time branch: with the pooled path compiled into the one kernel every launch
  // ran 5 % slower (more uniform branches per epilogue row), although three launches per step use it.
  const __amdgpu_buffer_rsrc_t rres = RPOOL ? __builtin_amdgcn_make_buffer_rsrc((void*)p.residual, 0, 0x7fffffff, 0x00020000)
                                            : mk(p.residual, p.ldr, esr);
  auto pooled_off = [&](int m) -> unsigned {      // byte offset of this lane's 8 columns in the pooled row of output pixel m
    const unsigned tq = fdiv((unsigned)m, p.dWo), ox = m - tq * p.Wo;
    const unsigned img = fdiv(tq, p.dHo), oy = tq - img * p.Ho;
    const unsigned hp = p.Ho >> 1, wp = p.Wo >> 1;
    const bool in = m < p.M && (oy >> 1) < hp && (ox >> 1) < wp;      // an odd size's last row / column has no pooled pixel
    return in ? (unsigned)((((img * hp + (oy >> 1)) * wp + (ox >> 1)) * (unsigned)p.ldr + (unsigned)n) * ES) : 0x80000000u;
  };
  const unsigned vy = (unsigned)(((wr * 128 + rr) * p.ldy + n) * eso);
  const unsigned vr = (unsigned)(((wr * 128 + rr) * p.ldr + n) * esr), vm = (unsigned)(((wr * 128 + rr) * p.ldm + n) * ES);
  const bool emit8 = EPI < 0 && ES == 2 && p.y8 != nullptr;
  const __amdgpu_buffer_rsrc_t ry8 = mk(p.y8, p.ldy, 1);
  const unsigned vy8 = (unsigned)((wr * 128 + rr) * p.ldy + n);
  const float q8s = emit8 && p.q8 ? p.q8[0] : 1.f;
  unsigned am8 = 0u;                                 // max |y| as a bit pattern (common.h absmax_bits): Inf / NaN are recorded, not dropped
  // bf16: residual / mask rows are fetched TWO passes ahead (two register sets, static indices): with one block per CU
  // nothing else hides their HBM latency.  The f32 parity instantiation (twice the registers per row) one pass ahead.
  constexpr int DEPTH = ES == 2 ? 2 : 1;
  // transposition writes: the swizzled chunk (col>>3) ^ (row&7) splits into a lane part ((r32>>3) ^ (hh<<2)) XOR a
  // compile-time part ((b<<2) ^ (g&3)): eight per-lane base addresses, the row of a register is an immediate offset
  char* wbase[8];
#pragma unroll
  for (int c = 0; c < 8; ++c)
    wbase[c] = (char*)ep + (hh * 4 * 64 + ((((r32 >> 3) ^ (hh << 2)) ^ c) << 3) + (r32 & 7)) * 4;
  u32x4 rresb[DEPTH][4][ES / 2], rmskb[DEPTH][4][ES / 2];
  auto fetch = [&](int a, u32x4 (*rres_)[ES / 2], u32x4 (*rmsk_)[ES / 2]) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int q = 0; q < ES / 2; ++q) {       // (an absent operand is not requested at all: even a zero-sized buffer returns its zeros through the vector memory path)
        if (RPOOL) rres_[i][q] = __builtin_amdgcn_raw_buffer_load_b128(rres, pooled_off(m0 + wr * 128 + a * 32 + rr + 8 * i), q * 16, 0);
        else if (has_res && !rf32) rres_[i][q] = __builtin_amdgcn_raw_buffer_load_b128(rres, vr, (a * 32 + 8 * i) * p.ldr * ES + q * 16, CDDMSL_LOAD_AUX);
        if (has_msk) rmsk_[i][q] = __builtin_amdgcn_raw_buffer_load_b128(rmsk, vm, (a * 32 + 8 * i) * p.ldm * ES + q * 16, CDDMSL_LOAD_AUX);
      }
  };
  if (PRE && DEPTH == 2) {
#pragma unroll
    for (int d = 0; d < 2; ++d)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        if (EPI & 1) {
          rresb[d % DEPTH][i][0] = pre[d][i];
          if (EPI & 2) rmskb[d % DEPTH][i][0] = __builtin_amdgcn_raw_buffer_load_b128(rmsk, vm, (d * 32 + 8 * i) * p.ldm * ES, CDDMSL_LOAD_AUX);
        } else rmskb[d % DEPTH][i][0] = pre[d][i];
      }
  } else if (DEPTH == 2 && !rf32) { fetch(0, rresb[0], rmskb[0]); fetch(1, rresb[DEPTH - 1], rmskb[DEPTH - 1]); }
  auto put = [&](auto A) {                          // accumulator rows 32a..32a+31 -> transposition buffer a & 1
    constexpr int a = decltype(A)::value;
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int g = 0; g < 16; ++g)                  // element (row rg + 4hh, col 32b + r32) -> ep[row*64 + ((col>>3 ^ row&7) << 3 | col&7)]
        *(float*)(wbase[(b << 2) ^ (g & 3)] + ((g & 3) + 8 * (g >> 2)) * 256 + (a & 1) * 8192) = acc[a][b][g];
  };
  auto pass = [&](auto A) {
    constexpr int a = decltype(A)::value;
    if (DEPTH == 1) fetch(a, rresb[0], rmskb[0]);
    if (rf32) {                                   // this pass's 4 rows x 32 B, in the two bf16 register sets taken together
#pragma unroll
      for (int f = 0; f < 8; ++f)
        rresb[(f >> 2) % DEPTH][f & 3][0] = __builtin_amdgcn_raw_buffer_load_b128(rres, vr, (a * 32 + 8 * (f >> 1)) * p.ldr * 4 + (f & 1) * 16, 0);
    }
    u32x4 (*rres_)[ES / 2] = rresb[a % DEPTH];
    u32x4 (*rmsk_)[ES / 2] = rmskb[a % DEPTH];
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");          // this pass's scratch writes have landed
    f32x4 val[4][2];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int row = rr + 8 * i;
      const f32x4* src = (const f32x4*)(ep + (a & 1) * 2048 + row * 64 + ((cg ^ (row & 7)) << 3));
      val[i][0] = src[0]; val[i][1] = src[1];
    }
    // (compiler fence: the next pass's float stores must stay behind these f32x4 loads -- type-based alias analysis treats them
    // as unrelated; they go to the OTHER buffer, but a hoisted store of pass a+2 would not)
    asm volatile("" ::: "memory");
    if constexpr (a + 1 < 4) put(std::integral_constant<int, a + 1>{});
    asm volatile("" ::: "memory");
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const f32x4 v0 = val[i][0], v1 = val[i][1];
      float v[8] = {v0[0], v0[1], v0[2], v0[3], v1[0], v1[1], v1[2], v1[3]};
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = affine<T>(v[j], sc[j], bi[j]);
      if (rf32) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          v[j] += __builtin_bit_cast(f32x4, rresb[((2 * i) >> 2) % DEPTH][(2 * i) & 3][0])[j];
          v[4 + j] += __builtin_bit_cast(f32x4, rresb[((2 * i + 1) >> 2) % DEPTH][(2 * i + 1) & 3][0])[j];
        }
      } else if (RPOOL) {                         // (x 0.25 is exact: the same value avgpool2_bwd would have stored)
        if (ES == 2) {
#pragma unroll
          for (int j = 0; j < 4; ++j) { v[2 * j] += 0.25f * bf2f(rres_[i][0][j] & 0xffff); v[2 * j + 1] += 0.25f * bf2f(rres_[i][0][j] >> 16); }
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            v[j] += 0.25f * __builtin_bit_cast(f32x4, rres_[i][0])[j]; v[4 + j] += 0.25f * __builtin_bit_cast(f32x4, rres_[i][ES / 2 - 1])[j];
          }
        }
      } else if (has_res) {
        if (ES == 2) {
#pragma unroll
          for (int j = 0; j < 4; ++j) { v[2 * j] += bf2f(rres_[i][0][j] & 0xffff); v[2 * j + 1] += bf2f(rres_[i][0][j] >> 16); }
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            v[j] += __builtin_bit_cast(f32x4, rres_[i][0])[j]; v[4 + j] += __builtin_bit_cast(f32x4, rres_[i][ES / 2 - 1])[j];
          }
        }
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) asm("v_max_f32 %0, %1, %2" : "=v"(v[j]) : "v"(v[j]), "s"(relu_floor));   // (fmaxf adds a canonicalising op per element)
      if (has_msk) {
        float mv[8];
        if (ES == 2) {
#pragma unroll
          for (int j = 0; j < 4; ++j) { mv[2 * j] = bf2f(rmsk_[i][0][j] & 0xffff); mv[2 * j + 1] = bf2f(rmsk_[i][0][j] >> 16); }
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            mv[j] = __builtin_bit_cast(f32x4, rmsk_[i][0])[j]; mv[4 + j] = __builtin_bit_cast(f32x4, rmsk_[i][ES / 2 - 1])[j];
          }
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) if (!(mv[j] > 0.f)) v[j] = 0.f;
      }
      const unsigned so = (unsigned)((a * 32 + 8 * i) * p.ldy * eso);
      // Store-data hazard (observed, gfx950): hipcc may put a vector-ALU write to the FIRST data register of a
      // buffer_store_dwordx4 ... soffset offen directly behind the store (it did: v_mul_hi_u32 of the next row's pooled-pixel
      // division), and lanes 12-15 of every 16 then stored that instruction's result instead of the output.  Nothing may
      // WRITE the data registers for a few cycles: a wait behind every store, and a use of the data behind the wait, which
      // keeps the registers allocated until then (the rows of a pass are otherwise free to interleave).
      if (emit8) {                                  // the e4m3 copy for the consuming convolution (fp8 configuration)
#pragma unroll
        for (int j = 0; j < 8; ++j) am8 = absmax_bits(am8, v[j]);
        const u32x2 o8 = {pack4_e4m3(v[0] * q8s, v[1] * q8s, v[2] * q8s, v[3] * q8s), pack4_e4m3(v[4] * q8s, v[5] * q8s, v[6] * q8s, v[7] * q8s)};
        __builtin_amdgcn_raw_buffer_store_b64(o8, ry8, vy8, (unsigned)((a * 32 + 8 * i) * p.ldy), CDDMSL_STORE_AUX);
        asm volatile("s_nop 4" ::: "memory");
        asm volatile("" :: "v"(o8));
      }
      if (f32out) {
        const u32x4 o0 = {__builtin_bit_cast(unsigned, v[0]), __builtin_bit_cast(unsigned, v[1]), __builtin_bit_cast(unsigned, v[2]), __builtin_bit_cast(unsigned, v[3])};
        const u32x4 o1 = {__builtin_bit_cast(unsigned, v[4]), __builtin_bit_cast(unsigned, v[5]), __builtin_bit_cast(unsigned, v[6]), __builtin_bit_cast(unsigned, v[7])};
        __builtin_amdgcn_raw_buffer_store_b128(o0, ry, vy, so, CDDMSL_STORE_AUX);
        __builtin_amdgcn_raw_buffer_store_b128(o1, ry, vy, so + 16, CDDMSL_STORE_AUX);
        asm volatile("s_nop 4" ::: "memory");
        asm volatile("" :: "v"(o0), "v"(o1));
      } else {
        const u32x4 o = {pack2bf(v[0], v[1]), pack2bf(v[2], v[3]), pack2bf(v[4], v[5]), pack2bf(v[6], v[7])};
        if (p.nt_out) __builtin_amdgcn_raw_buffer_store_b128(o, ry, vy, so, CDDMSL_STORE_AUX);
        else __builtin_amdgcn_raw_buffer_store_b128(o, ry, vy, so, 0);
        asm volatile("s_nop 4" ::: "memory");
        asm volatile("" :: "v"(o));
      }
    }
    if (DEPTH == 2 && a + 2 < 4 && !rf32) fetch(a + 2, rresb[a % DEPTH], rmskb[a % DEPTH]);
  };
  put(std::integral_constant<int, 0>{});
  pass(std::integral_constant<int, 0>{});
  pass(std::integral_constant<int, 1>{});
  pass(std::integral_constant<int, 2>{});
  pass(std::integral_constant<int, 3>{});
  if (emit8 && p.amax8) {                           // (rows past M contribute their bias-only values: an over-estimate at worst)
    am8 = wave_max_u(am8);
    if (lane == 0) atomicMax(p.amax8 + (blockIdx.x & 63), am8);
  }
}

// EPI: which optional epilogue operands exist, as a COMPILE-TIME fact (bit 0 residual rows, bit 1 ReLU-mask rows; bf16 output, no
// e4m3 copy, no f32 residual stream) or -1 = decided at run time (every other combination, and the exact-f32 instantiations).
// With run-time flags every row of a pass is a chain of uniform branches: hipcc then neither interleaves the rows nor counts
// its vmcnt waits across them -- passes 2 and 3 waited vmcnt(0) for their residual rows, i.e. for the previous pass's stores.
// PERSIST: one workgroup per CU walks the tiles  first + i * gridDim.x  (the XCD-contiguous order xcd_remap gives the one-tile grid)
// one after the other -- nothing is carried from tile to tile (tools/tile_stamps.py: ~2.4 us pass between a workgroup's end and
// its successor's first instruction on the CU, and ~1 us of the start-up is kernel-argument and index arithmetic).
template <typename T, bool TAPS, bool RPOOL = false, int EPI = -1, bool PERSIST = false, bool SPLITK = false>
__global__ __launch_bounds__(512) void k_conv_fwd256(ConvArgs p) {
  __shared__ __attribute__((aligned(16))) u32x4 lds[2 * 2 * 2 * 128 * KCH];   // byte address = buf<<16 | ab<<15 | half<<14 | row*128 + slot*16
  const int t_in = threadIdx.x;
  p.x += (long)blockIdx.y * p.bx; p.w += (long)blockIdx.y * p.bw; p.y += (long)blockIdx.y * p.by;
  const int ntn = p.Cout >> 8;
  const int ntiles = PERSIST ? (p.tile_limit ? p.tile_limit : ntn * ((p.M + 255) >> 8)) : 0;
  int lbid = PERSIST ? (int)((blockIdx.x & 7) * (gridDim.x >> 3) + (blockIdx.x >> 3))
           : SPLITK ? p.tile0 + (int)(blockIdx.x / (unsigned)p.ksplits) : xcd_remap(blockIdx.x, gridDim.x);
  const int kt0 = SPLITK ? (int)(blockIdx.x % (unsigned)p.ksplits) * p.kper : 0;      // first K-tile of this block's share
  if (PERSIST && lbid >= ntiles) return;
  for (;;) {
  int t = t_in;
  if (PERSIST) asm volatile("" : "+v"(t));       // per-lane values are recomputed per tile, not carried through the main loop
  const int lane = t & 63;
#ifdef CDDMSL_TILE_STAMPS
  const unsigned long long ts_entry = __builtin_amdgcn_s_memrealtime();
#endif
  const int wvu = __builtin_amdgcn_readfirstlane(t >> 6);
  const int wr = wvu >> 2, wc = wvu & 3;
  const int tile_n = lbid % ntn, tile_m = lbid / ntn;
  const int m0 = tile_m * 256, n0 = tile_n * 256;
  const int cl = (t & 7) ^ ((t >> 4) & 7);      // logical K chunk of this lane's LDS slot (slot ^ ((row>>1)&7))
  const int nkt = SPLITK ? min(p.kper, (p.Kc >> 3) - kt0) : (p.Kc >> 3);
  const int tpt = p.cpp >> 3;                   // K-tiles per filter tap

  // ---- staging state.  Sources are addressed as buffer base (per block, SGPRs) + per-lane byte offset (constant over
  // the K loop) + a wave-uniform running offset in the instruction's soffset: no per-lane pointer arithmetic in the loop.
  // A lane whose row is outside M, or whose current filter tap falls outside the image, sets bit 31 of its offset:
  // beyond num_records, the load then writes zeros into LDS.
  //   A half h, piece i -> tile row i*128 + h*64 + (t>>3);   B half j, piece i -> tile col (2i + (t>>8))*64 + j*32 + ((t>>3)&31)
  auto rowoff = [&](int m, int& iy0, int& ix0) {
    const unsigned tq = fdiv((unsigned)m, p.dWo), ox = m - tq * p.Wo;
    const unsigned img = fdiv(tq, p.dHo), oy = tq - img * p.Ho;
    iy0 = (int)oy * p.stride - p.pad; ix0 = (int)ox * p.stride - p.pad;
    return (((long)img * p.Hi + iy0) * p.Wi + ix0) * p.xrs * 16;
  };
  int iyb, ixb;
  const long base_a = rowoff(m0, iyb, ixb);      // rows of one tile ascend from here (2*pad <= K-1, checked by the host)
  const __amdgpu_buffer_rsrc_t ra_rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)(p.x + base_a), 0, 0x7fffffff, 0x00020000);
  const __amdgpu_buffer_rsrc_t rb_rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)(p.w + (long)n0 * p.wrs * 16), 0, 0x7fffffff, 0x00020000);
  unsigned va[2][2], vinv[2][2], vb[2][2];
  int iy0[2][2], ix0[2][2];
#pragma unroll
  for (int h = 0; h < 2; ++h)
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int m = m0 + i * 128 + h * 64 + (t >> 3);
      const bool vm = m < p.M;
      const long ro = rowoff(vm ? m : m0, iy0[h][i], ix0[h][i]);
      va[h][i] = (unsigned)(ro - base_a) + cl * 16;
      // rows past M: every tap invalid (TAPS) / bit 31 of the offset (no taps); also parks iy0 outside the image for the loops below
      if (!vm) { iy0[h][i] = -(1 << 20); if (!TAPS) va[h][i] |= 0x80000000u; }
      vinv[h][i] = 0;
      vb[h][i] = (unsigned)(((2 * i + (t >> 8)) * 64 + h * 32 + ((t >> 3) & 31)) * p.wrs + cl) * 16;
    }
  if (TAPS) {
    // tap (ky, kx) of a row is invalid when its input row OR its input column falls outside the image: one pass over the filter
    // columns builds the row's column mask, one over the filter rows places it (or an all-ones group) -- KH + KW iterations with
    // the lane's four rows side by side, where the former KH x KW loop per row took ~4 us of a 3x3 tile's start-up
    // (tools/tile_stamps.py: 5.0 us from kernel entry to the first operand request, 1.2 us for a 1x1 layer).
    unsigned xm[2][2] = {{0, 0}, {0, 0}};
    for (int kx = 0; kx < p.KW; ++kx)
#pragma unroll
      for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int i = 0; i < 2; ++i) xm[h][i] |= ((unsigned)(ix0[h][i] + kx) >= (unsigned)p.Wi ? 1u : 0u) << kx;
    const unsigned full = (1u << p.KW) - 1u;
    for (int ky = 0; ky < p.KH; ++ky)
#pragma unroll
      for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int i = 0; i < 2; ++i) vinv[h][i] |= ((unsigned)(iy0[h][i] + ky) >= (unsigned)p.Hi ? full : xm[h][i]) << (ky * p.KW);
  }
  const int step_col = (p.xrs - (p.cpp - KCH)) * 16;                               // next tap in the same filter row
  const int step_row = ((p.Wi - (p.KW - 1)) * p.xrs - (p.cpp - KCH)) * 16;         // first tap of the next filter row
  int left[2] = {tpt, tpt}, tap[2] = {0, 0}, kxs[2] = {0, 0};
  unsigned soa[2] = {0, 0}, sob[2] = {0, 0};
  if (SPLITK) {                                 // the streams start at K-tile kt0: inside filter tap kt0 / tpt
    const int tap0 = TAPS ? kt0 / tpt : 0, within = TAPS ? kt0 - tap0 * tpt : kt0;
    const int ky0 = TAPS ? tap0 / p.KW : 0, kx0 = tap0 - ky0 * p.KW;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      left[h] = tpt - (TAPS ? within : 0); tap[h] = tap0; kxs[h] = kx0;
      soa[h] = (unsigned)((ky0 * p.Wi + kx0) * p.xrs * 16 + within * KCH * 16);
      sob[h] = (unsigned)(kt0 * KCH * 16);
    }
  }

  char* const L = (char*)lds;
  auto stageA = [&](auto H, int buf) {
    constexpr int h = decltype(H)::value;
    char* dst = L + (buf << 16) + (h << 14) + wvu * 1024;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      unsigned v = va[h][i];
      if (TAPS) v |= __builtin_amdgcn_ubfe(vinv[h][i], (unsigned)tap[h], 1u) << 31;
      blds16(ra_rsrc, v, soa[h], dst + i * 8192);
    }
    if (TAPS) {
      int step = KCH * 16;
      if (--left[h] == 0) {
        left[h] = tpt; ++tap[h];
        if (++kxs[h] == p.KW) { kxs[h] = 0; step = step_row; } else step = step_col;
      }
      soa[h] += step;
    } else soa[h] += KCH * 16;
  };
  auto stageB = [&](auto J, int buf) {
    constexpr int j = decltype(J)::value;
    char* dst = L + (buf << 16) + (1 << 15) + (j << 14) + wvu * 1024;
#pragma unroll
    for (int i = 0; i < 2; ++i) blds16(rb_rsrc, vb[j][i], sob[j], dst + i * 8192);
    sob[j] += KCH * 16;
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

  // ---- fragment reads: per-lane byte addresses per k-step, buffer bit (1<<16) toggled by XOR; half / row-tile offsets are immediates
  const int r32 = lane & 31, hh = lane >> 5, sw = (r32 >> 1) & 7;
  unsigned ada[4], adb[4];
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) {
    ada[ks] = (unsigned)(((wr * 64 + r32) * KCH + ((2 * ks + hh) ^ sw)) * 16);
    adb[ks] = (unsigned)(((wc * 32 + r32) * KCH + ((2 * ks + hh) ^ sw)) * 16 + (1 << 15));
  }
  u32x4 fa0[2][4], fa1[2][4], fb0[4], fb1[4];
  auto readA = [&](auto I, u32x4 (*fa)[4]) {
    constexpr int i = decltype(I)::value;
#pragma unroll
    for (int rt = 0; rt < 2; ++rt)
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) fa[rt][ks] = *(const u32x4*)(L + ada[ks] + ((i << 14) + rt * 32 * KCH * 16));
  };
  auto readB = [&](auto J, u32x4* fb) {
    constexpr int j = decltype(J)::value;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) fb[ks] = *(const u32x4*)(L + adb[ks] + (j << 14));
  };
  auto flipA = [&]() {
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) ada[ks] ^= 1u << 16;
  };
  auto flipB = [&]() {
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) adb[ks] ^= 1u << 16;
  };
#define CDDMSL_MMA_QUAD(I, J, FA, FB) MmaQuad<T>::run(acc[2 * (I)][J], acc[2 * (I) + 1][J], FA, FB)
#define CDDMSL_PHASE_SYNC_IN()                                                      \
  __builtin_amdgcn_sched_barrier(0);                                                \
  __builtin_amdgcn_s_barrier();                                                     \
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                                \
  __builtin_amdgcn_sched_barrier(0);                                                \
  __builtin_amdgcn_s_setprio(1);
#define CDDMSL_PHASE_SYNC_OUT(I, J)                                                 \
  asm volatile("" : "+v"(acc[2 * (I)][J]), "+v"(acc[2 * (I) + 1][J]));   /* the MFMAs above cannot sink below the barrier */ \
  __builtin_amdgcn_s_setprio(0);                                                    \
  __builtin_amdgcn_sched_barrier(0);                                                \
  __builtin_amdgcn_s_barrier();                                                     \
  __builtin_amdgcn_sched_barrier(0);

  // ---- prologue: tile 0 complete, tile 1 without its A1 half (staged by phase 1 of tile 0); A0 of tile 0 is read ahead
  stageA(I0{}, 0); stageA(I1{}, 0); stageB(I0{}, 0); stageB(I1{}, 0);
  if (nkt > 1) {
    stageA(I0{}, 1); stageB(I0{}, 1); stageB(I1{}, 1);
    asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
  } else {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  }
  __builtin_amdgcn_s_barrier();
  readA(I0{}, fa0);
  if (wr == 1) __builtin_amdgcn_s_barrier();     // group 1 runs one barrier behind group 0
  __builtin_amdgcn_sched_barrier(0);
#ifdef CDDMSL_TILE_STAMPS
  const unsigned long long ts_loop = __builtin_amdgcn_s_memrealtime();
#endif

  // One K-tile = four phases.  LAST (compile time): the tile's final K-tile, peeled out of the loop -- nothing is left to stage and no
  // wait is due (it was retired by the K-tile before it, or by the prologue).
  // (Tried here and measured slower, +1 ms of kernel time per step: starting the epilogue's residual / mask rows on their way from HBM
  // with one dword load per 128-byte line -- a lane per row -- during this last K-tile.  The epilogue's first pass does wait ~2 us
  // for its operand rows, but 64 single-line requests per instruction cost the load path more than the wait.)
  // the epilogue's first operand rows ride in the A0 fragments' registers from phase 3 of the last K-tile on (see tile_epilogue PRE)
  constexpr bool PREF = EPI > 0 && !RPOOL && Mma<T>::ES == 2 && !SPLITK;
  u32x4 pre[2][4];
  f32x4 sb[4];
  auto ktile = [&](int kt, auto LAST) {
    constexpr bool last = decltype(LAST)::value;
    const int d = kt & 1;
    const bool more1 = !last, more2 = !last && kt + 2 < nkt;
    // phase 1
    readB(I0{}, fb0);
    if (more1) stageA(I1{}, d ^ 1);
    CDDMSL_PHASE_SYNC_IN();
    CDDMSL_MMA_QUAD(0, 0, fa0, fb0);
    CDDMSL_PHASE_SYNC_OUT(0, 0);
    // phase 2
    readB(I1{}, fb1);
    flipB();
    if (more2) stageA(I0{}, d);
    CDDMSL_PHASE_SYNC_IN();
    CDDMSL_MMA_QUAD(0, 1, fa0, fb1);
    CDDMSL_PHASE_SYNC_OUT(0, 1);
    // phase 3: the wait retires everything but the two youngest half-tiles, i.e. all of tile kt+1 (other buffer)
    readA(I1{}, fa1);
    flipA();
    if (more2) {
      stageB(I0{}, d);
      asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
    } else if (more1) {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    } else if (PREF) {
      const bool is_res = (EPI & 1) != 0;
      const char* base = is_res ? p.residual : p.relu_mask;
      const int ld = is_res ? p.ldr : p.ldm;
      long bytes = ((long)p.M - m0) * ld * 2;
      if (bytes > 0x7fffffffL) bytes = 0x7fffffffL;
      const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)(base + (long)m0 * ld * 2), 0, (int)bytes, 0x00020000);
      const unsigned vo = (unsigned)(((wr * 128 + (lane >> 3)) * ld + n0 + wc * 64 + (lane & 7) * 8) * 2);
#pragma unroll
      for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int i = 0; i < 4; ++i) pre[a][i] = __builtin_amdgcn_raw_buffer_load_b128(rs, vo, (a * 32 + 8 * i) * ld * 2, 0);
    }
    CDDMSL_PHASE_SYNC_IN();
    CDDMSL_MMA_QUAD(1, 1, fa1, fb1);
    CDDMSL_PHASE_SYNC_OUT(1, 1);
    // phase 4
    if (more1) readA(I0{}, fa0);
    if (more2) stageB(I1{}, d);
    if (last && !SPLITK) {                          // the epilogue's scale / bias values (fb1 is dead from here on)
      const int n = n0 + wc * 64 + (lane & 7) * 8;
      const f32x4 one = {1.f, 1.f, 1.f, 1.f}, zero = {0.f, 0.f, 0.f, 0.f};
      sb[0] = p.scale ? *(const f32x4*)(p.scale + n) : one; sb[1] = p.scale ? *(const f32x4*)(p.scale + n + 4) : one;
      sb[2] = p.bias ? *(const f32x4*)(p.bias + n) : zero; sb[3] = p.bias ? *(const f32x4*)(p.bias + n + 4) : zero;
    }
    CDDMSL_PHASE_SYNC_IN();
    CDDMSL_MMA_QUAD(1, 0, fa1, fb0);
    CDDMSL_PHASE_SYNC_OUT(1, 0);
  };
  for (int kt = 0; kt + 1 < nkt; ++kt) ktile(kt, std::false_type{});
  ktile(nkt - 1, std::true_type{});
  if (wr == 0) __builtin_amdgcn_s_barrier();     // re-align the two groups (every wave has now passed all reads)
#ifdef CDDMSL_TILE_STAMPS
  const unsigned long long ts_epi = __builtin_amdgcn_s_memrealtime();
#endif
#undef CDDMSL_MMA_QUAD
#undef CDDMSL_PHASE_SYNC_IN
#undef CDDMSL_PHASE_SYNC_OUT

  if (SPLITK) {                                   // raw accumulators, fragment order: 32 x 16 bytes per lane, 1 KiB per wave instruction
    store_frags((f32x4*)p.partial + (long)blockIdx.x * (8 * 32 * 64) + (wvu * 32) * 64 + lane, acc);
    return;
  }
  tile_epilogue<T, RPOOL, EPI, PREF>(p, acc, (float*)lds + wvu * 4096, wr, wc, lane, m0, n0, pre, sb);
#ifdef CDDMSL_TILE_STAMPS
  if (p.tstamps && lane == 0) {
    if (!PERSIST) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // (exit stamp = the wave's stores have left)
    unsigned long long* o = p.tstamps + ((long)(PERSIST ? lbid : (int)blockIdx.x) * 8 + wvu) * 4;
    o[0] = ts_entry; o[1] = ts_loop; o[2] = ts_epi; o[3] = __builtin_amdgcn_s_memrealtime();
  }
#endif
  if (!PERSIST) break;
  lbid += gridDim.x;
  if (lbid >= ntiles) break;
  __builtin_amdgcn_s_barrier();                    // the next tile's operand DMA overwrites the other waves' transposition scratch
  }
}

// ------------------------------------------------------------------------------------------------
// 256 x 128 tile, 4 waves (2 x 2; 128 x 64 per wave -- the 256x256 kernel's per-wave tile and operand reuse), TWO workgroups per CU.
//
// The 256x256 kernel owns its CU: its tile's start-up (operands' first trip from HBM), main loop and epilogue traffic run one
// after the other, which leaves the layers whose epilogue moves as many bytes as their main loop takes time at about half of
// either roofline (tools/tile_stamps.py).  Here two independent workgroups share the CU's matrix pipes and memory path: while
// one drains its tile the other multiplies.  No ping-pong between wave groups (each SIMD hosts one wave of each workgroup, not
// synchronised with each other); instead each wave pipelines itself: the LDS reads of K-tile kt+1 (12 x 16 bytes per lane) and
// the LDS-DMA of K-tile kt+3 are issued in front of K-tile kt's 16 MFMAs, one barrier per K-tile.
// K-tile = 4 chunks (32 bf16): LDS ring of 3 stages x (256 + 128 rows x 64 B) = 72 KiB per workgroup; 64-byte rows, chunk
// ^= (row >> 1) & 3 on the source side of the DMA and on the ds_read_b128 side (8 consecutive rows cover the 8 bank groups).
// One operand stream (all six DMAs of a K-tile share the filter-tap state).  Epilogue: tile_epilogue, scratch = the idle ring.
// ------------------------------------------------------------------------------------------------
template <typename T, bool TAPS, int EPI>
__global__ __launch_bounds__(256, 2) void k_conv_fwd2(ConvArgs p) {
  constexpr int SA = 256 * 64, SB = 128 * 64, SS = SA + SB, STAGES = 3;
  __shared__ __attribute__((aligned(16))) u32x4 lds[STAGES * SS / 16];
  const int t = threadIdx.x, lane = t & 63;
#ifdef CDDMSL_TILE_STAMPS
  const unsigned long long ts_entry = __builtin_amdgcn_s_memrealtime();
#endif
  p.x += (long)blockIdx.y * p.bx; p.w += (long)blockIdx.y * p.bw; p.y += (long)blockIdx.y * p.by;
  const int wvu = __builtin_amdgcn_readfirstlane(t >> 6);
  const int wr = wvu >> 1, wc = wvu & 1;
  const int ntn = p.Cout >> 7;
  const int lbid = xcd_remap(blockIdx.x, gridDim.x);
  const int tile_n = lbid % ntn, tile_m = lbid / ntn;
  const int m0 = tile_m * 256, n0 = tile_n * 128;
  const int cl = (t & 3) ^ ((t >> 3) & 3);      // logical K chunk of this lane's LDS slot (slot ^ ((row>>1)&3)); rows (t>>2) + 64 i
  const int nkt = p.Kc >> 2;
  const int tpt = p.cpp >> 2;                   // K-tiles per filter tap

  auto rowoff = [&](int m, int& iy0, int& ix0) {
    const unsigned tq = fdiv((unsigned)m, p.dWo), ox = m - tq * p.Wo;
    const unsigned img = fdiv(tq, p.dHo), oy = tq - img * p.Ho;
    iy0 = (int)oy * p.stride - p.pad; ix0 = (int)ox * p.stride - p.pad;
    return (((long)img * p.Hi + iy0) * p.Wi + ix0) * p.xrs * 16;
  };
  int iyb, ixb;
  const long base_a = rowoff(m0, iyb, ixb);
  const __amdgpu_buffer_rsrc_t ra_rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)(p.x + base_a), 0, 0x7fffffff, 0x00020000);
  const __amdgpu_buffer_rsrc_t rb_rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)(p.w + (long)n0 * p.wrs * 16), 0, 0x7fffffff, 0x00020000);
  unsigned va[4], vinv[4], vb[2];
  int iy0[4], ix0[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int m = m0 + (t >> 2) + 64 * i;
    const bool vm = m < p.M;
    const long ro = rowoff(vm ? m : m0, iy0[i], ix0[i]);
    va[i] = (unsigned)(ro - base_a) + cl * 16;
    if (!vm) { iy0[i] = -(1 << 20); if (!TAPS) va[i] |= 0x80000000u; }
    vinv[i] = 0;
  }
#pragma unroll
  for (int i = 0; i < 2; ++i) vb[i] = (unsigned)((((t >> 2) + 64 * i) * p.wrs + cl) * 16);
  if (TAPS) {                                   // (as in k_conv_fwd256: column mask, then one step per filter row)
    unsigned xm[4] = {0, 0, 0, 0};
    for (int kx = 0; kx < p.KW; ++kx)
#pragma unroll
      for (int i = 0; i < 4; ++i) xm[i] |= ((unsigned)(ix0[i] + kx) >= (unsigned)p.Wi ? 1u : 0u) << kx;
    const unsigned full = (1u << p.KW) - 1u;
    for (int ky = 0; ky < p.KH; ++ky)
#pragma unroll
      for (int i = 0; i < 4; ++i) vinv[i] |= ((unsigned)(iy0[i] + ky) >= (unsigned)p.Hi ? full : xm[i]) << (ky * p.KW);
  }
  const int step_col = (p.xrs - (p.cpp - 4)) * 16;
  const int step_row = ((p.Wi - (p.KW - 1)) * p.xrs - (p.cpp - 4)) * 16;
  int left = tpt, tap = 0, kxs = 0;
  unsigned soa = 0, sob = 0;

  char* const L = (char*)lds;
  auto stage = [&](int st) {                    // the next K-tile of the operand stream -> ring stage st
    char* dst = L + st * SS + wvu * 1024;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      unsigned v = va[i];
      if (TAPS) v |= __builtin_amdgcn_ubfe(vinv[i], (unsigned)tap, 1u) << 31;
      blds16(ra_rsrc, v, soa, dst + i * 4096);
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) blds16(rb_rsrc, vb[i], sob, dst + SA + i * 4096);
    sob += 64;
    if (TAPS) {
      int step = 64;
      if (--left == 0) {
        left = tpt; ++tap;
        if (++kxs == p.KW) { kxs = 0; step = step_row; } else step = step_col;
      }
      soa += step;
    } else soa += 64;
  };

  f32x16 acc[4][2];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;

  const int r32 = lane & 31, hh = lane >> 5, sw = (r32 >> 1) & 3;
  unsigned ada[2], adb[2];
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) {
    ada[ks] = (unsigned)(((wr * 128 + r32) * 4 + ((2 * ks + hh) ^ sw)) * 16);
    adb[ks] = (unsigned)(SA + ((wc * 64 + r32) * 4 + ((2 * ks + hh) ^ sw)) * 16);
  }
  u32x4 fa[2][4][2], fb[2][2][2];               // [register set][32-row / 32-column tile][k-step]
  auto readf = [&](auto SET, int st) {
    constexpr int set = decltype(SET)::value;
    const char* base = L + st * SS;
#pragma unroll
    for (int rt = 0; rt < 4; ++rt)
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) fa[set][rt][ks] = *(const u32x4*)(base + ada[ks] + rt * 32 * 64);
#pragma unroll
    for (int ct = 0; ct < 2; ++ct)
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) fb[set][ct][ks] = *(const u32x4*)(base + adb[ks] + ct * 32 * 64);
  };
  using S0 = std::integral_constant<int, 0>;
  using S1 = std::integral_constant<int, 1>;

  // ---- prologue: K-tiles 0..2 requested, K-tile 0 landed and read
  stage(0);
  if (nkt > 1) stage(1);
  if (nkt > 2) stage(2);
  if (nkt > 2) asm volatile("s_waitcnt vmcnt(12)" ::: "memory");
  else if (nkt > 1) asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
  else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  readf(S0{}, 0);
#ifdef CDDMSL_TILE_STAMPS
  const unsigned long long ts_loop = __builtin_amdgcn_s_memrealtime();
#endif
  int st_next = 1, st_free = 0;                 // ring stage of K-tile kt+1 / stage K-tile kt+3 goes to (= K-tile kt's)

  auto ktile = [&](int kt, auto SET) {
    constexpr int set = decltype(SET)::value;
    // K-tile kt+1 has landed (this lane's share; the barrier makes it everyone's), K-tile kt's fragments have been read
    if (kt + 2 < nkt) asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_waitcnt(0xc07f);          // lgkmcnt(0), as the builtin: hipcc's own wait insertion then knows the fragments
                                                 // of K-tile kt are in, and does not put a lgkmcnt(0) -- which would also wait for
                                                 // K-tile kt+1's reads -- in front of the MFMAs
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
    if (kt + 1 < nkt) readf(std::integral_constant<int, set ^ 1>{}, st_next);
    if (kt + 3 < nkt) stage(st_free);
    st_next = st_next == STAGES - 1 ? 0 : st_next + 1;
    st_free = st_free == STAGES - 1 ? 0 : st_free + 1;
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
#pragma unroll
      for (int rt = 0; rt < 4; ++rt)
#pragma unroll
        for (int ct = 0; ct < 2; ++ct) Mma<T>::step(acc[rt][ct], fa[set][rt][ks], fb[set][ct][ks]);
    __builtin_amdgcn_s_setprio(0);
    __builtin_amdgcn_sched_barrier(0);
  };
  for (int kt = 0; kt < nkt; kt += 2) {
    ktile(kt, S0{});
    if (kt + 1 < nkt) ktile(kt + 1, S1{});
  }
#ifdef CDDMSL_TILE_STAMPS
  asm volatile("" : "+v"(acc[3][1]));
  const unsigned long long ts_epi = __builtin_amdgcn_s_memrealtime();
#endif
  // every wave has passed the last K-tile's barrier with its reads retired and no DMA in flight: the ring is free
  tile_epilogue<T, false, EPI>(p, acc, (float*)lds + wvu * 4096, wr, wc, lane, m0, n0);
#ifdef CDDMSL_TILE_STAMPS
  if (p.tstamps && lane == 0) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    unsigned long long* o = p.tstamps + ((long)blockIdx.x * 4 + wvu) * 4;
    o[0] = ts_entry; o[1] = ts_loop; o[2] = ts_epi; o[3] = __builtin_amdgcn_s_memrealtime();
  }
#endif
}

// Sum of a tile's K-splits + the epilogue (bf16 output; scale / bias, residual, ReLU, ReLU mask): one thread per 16-byte slot of
// the fragment-ordered partials = four consecutive rows of one output column.  Only ever a handful of tiles per launch.
__global__ __launch_bounds__(256) void k_conv_split_reduce(ConvArgs p) {
  const int tile_rel = blockIdx.x >> 6, q = (blockIdx.x & 63) * 256 + threadIdx.x;
  const f32x4* src = (const f32x4*)p.partial + (long)tile_rel * p.ksplits * 16384 + q;
  f32x4 sum = src[0];
  for (int s = 1; s < p.ksplits; ++s) sum += src[(long)s * 16384];
  const int wvu = q >> 11, j = (q >> 6) & 31, lane = q & 63, r32 = lane & 31, hh = lane >> 5;
  const int a = j >> 3, b = (j >> 2) & 1, g4 = j & 3, wr = wvu >> 2, wc = wvu & 3;
  const int ntn = p.Cout >> 8, lbid = p.tile0 + tile_rel;
  const int tile_n = lbid % ntn, tile_m = lbid / ntn;
  const int n = tile_n * 256 + wc * 64 + b * 32 + r32;
  const int mrow = tile_m * 256 + wr * 128 + a * 32 + 8 * g4 + 4 * hh;
  const float sc = p.scale ? p.scale[n] : 1.f, bi = p.bias ? p.bias[n] : 0.f;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const long m = mrow + e;
    if (m >= p.M) break;
    float v = __builtin_fmaf(sum[e], sc, bi);
    if (p.residual) v += bf2f(*(const unsigned short*)(p.residual + (m * p.ldr + n) * 2));
    if (p.relu) v = fmaxf(v, 0.f);
    if (p.relu_mask && !(bf2f(*(const unsigned short*)(p.relu_mask + (m * p.ldm + n) * 2)) > 0.f)) v = 0.f;
    *(unsigned short*)(p.y + (m * p.ldy + n) * 2) = f2bf(v);
  }
}

// Workgroups of the persistent form of the 256x256 kernel: one per CU, or 0 = use the one-tile-per-workgroup grid (CDDMSL_PERSIST=0;
// read per launch, so one process can A/B).
static int persistent_blocks() { return env_int("CDDMSL_PERSIST", 1) ? persistent_blocks_raw() : 0; }

// ---- launch, forward
// The epilogue variant (template parameter EPI) of k_conv_fwd256 and k_conv_fwd2: for bf16 outputs the operand set (bit 0 residual,
// bit 1 ReLU mask) at compile time, otherwise -1 = run-time flags.  with_epi turns the run-time set into the template argument.
static int epi_of(const ConvArgs& a) { return (a.out_f32 || a.res_f32 || a.y8) ? -1 : (a.residual ? 1 : 0) | (a.relu_mask ? 2 : 0); }
template <typename F> void with_epi(int epi, F&& launch) {
  switch (epi) {
    case 0: launch(std::integral_constant<int, 0>()); break;
    case 1: launch(std::integral_constant<int, 1>()); break;
    case 2: launch(std::integral_constant<int, 2>()); break;
    default: launch(std::integral_constant<int, 3>()); break;
  }
}

template <typename T, bool TAPS> void launch_fwd2(const ConvArgs& a, dim3 grid, hipStream_t st) {
  const int epi = epi_of(a);
  if constexpr (sizeof(T) == 2) {
    if (epi >= 0) {
      with_epi(epi, [&](auto e) { hipLaunchKernelGGL((k_conv_fwd2<T, TAPS, decltype(e)::value>), grid, dim3(256), 0, st, a); });
      return;
    }
  }
  hipLaunchKernelGGL((k_conv_fwd2<T, TAPS, -1>), grid, dim3(256), 0, st, a);
}

// Tail of a badly quantised launch.  16 x 50 x 83 pixels are 260 row panels: a 256-column layer of res4 is 260 tiles for 256 CUs --
// two rounds of workgroups, the second with 4 of them (15 + 16 such launches per step, ~55 and ~30 us each wasted).  When the last
// round would be less than an eighth full, the main launch stops at the last full round and the leftover tiles are computed
// split along K (every CU takes a slice; raw accumulators to the workspace) and finished by k_conv_split_reduce.
// -> the `rem` leftover tiles in `splits` slices of `kper` K-tiles each; splits = 0: no tail split.
struct TailSplit { int rem, splits, kper; };
constexpr int TAIL_FRAC_DEFAULT = 8;
static TailSplit plan_tail_split(int tiles, int ncu, int nktot, long ws_bytes) {
  const int rem = ncu > 0 ? tiles % ncu : 0;
  long frac = env_int("CDDMSL_TAIL_FRAC", TAIL_FRAC_DEFAULT);  // the last round counts as "nearly empty" below 1 / FRAC of the CUs
  if (frac <= 0) frac = 8;
  if (env_int("CDDMSL_TAIL_SPLIT", 1) == 0 || tiles <= ncu || rem <= 0 || rem * frac > ncu || nktot < 16) return {};
  long S = ncu / rem;
  if (S > nktot / 2) S = nktot / 2;
  const long maxs = env_int("CDDMSL_TAIL_MAXS", S);             // (A/B knob)
  if (S > maxs) S = maxs;
  const int kper = (int)((nktot + S - 1) / S);
  S = (nktot + kper - 1) / kper;
  if (S < 2 || rem * S * 65536 * 4 > ws_bytes) return {};
  return {rem, (int)S, kper};
}

template <typename T, bool TAPS> void launch256_main(const ConvArgs& a, dim3 grid, hipStream_t st, int epi) {
  // Persistent form (bf16, no taps) for SHORT reductions only: per shape, two builds in one process, K <= 512 layers gain 4-6 %
  // (the ~2.4 us between workgroups is 10-20 % of such a tile), K >= 2048 layers lose 2-4 % against the hardware's dynamic
  // dispatch; in the step k_conv_fwd256 50.9 -> 50.4 ms.
  if constexpr (std::is_same<T, __bf16>::value && !TAPS) {
    const int nb = persistent_blocks();
    // (A/B knob) CDDMSL_PERSIST_MAXKT: longest reduction, in K-tiles, that takes the persistent form
    if (nb > 0 && grid.y == 1 && (int)grid.x > nb && (a.Kc >> 3) <= env_int("CDDMSL_PERSIST_MAXKT", 8)) {
      with_epi(epi, [&](auto e) { hipLaunchKernelGGL((k_conv_fwd256<T, false, false, decltype(e)::value, true>), dim3(nb), dim3(512), 0, st, a); });
      return;
    }
  }
  with_epi(epi, [&](auto e) { hipLaunchKernelGGL((k_conv_fwd256<T, TAPS, false, decltype(e)::value>), grid, dim3(512), 0, st, a); });
}

template <typename T, bool TAPS> void launch256(const ConvArgs& a, dim3 grid, hipStream_t st, void* ws, long ws_bytes) {
  const int epi = epi_of(a);
  if (sizeof(T) == 4 || epi < 0) { hipLaunchKernelGGL((k_conv_fwd256<T, TAPS, false, -1>), grid, dim3(512), 0, st, a); return; }
  if constexpr (sizeof(T) != 4) {
    if constexpr (std::is_same<T, __bf16>::value) {
      const int tiles = (int)grid.x;
      const TailSplit ts = grid.y == 1 ? plan_tail_split(tiles, persistent_blocks_raw(), a.Kc >> 3, ws ? ws_bytes : 0) : TailSplit{};
      if (ts.splits) {
        ConvArgs m = a, t = a;
        m.tile_limit = tiles - ts.rem;
        launch256_main<T, TAPS>(m, dim3((unsigned)(tiles - ts.rem), 1), st, epi);
        t.partial = (float*)ws; t.tile0 = tiles - ts.rem; t.ksplits = ts.splits; t.kper = ts.kper;
        hipLaunchKernelGGL((k_conv_fwd256<T, TAPS, false, -1, false, true>), dim3((unsigned)(ts.rem * ts.splits)), dim3(512), 0, st, t);
        hipLaunchKernelGGL(k_conv_split_reduce, dim3((unsigned)(ts.rem * 64)), dim3(256), 0, st, t);
        return;
      }
    }
    launch256_main<T, TAPS>(a, grid, st, epi);
  }
}

template <typename T> void launch_tile256(const ConvArgs& a, const Plan& p, hipStream_t st, void* ws, long ws_bytes) {
  const dim3 grid(p.gx, p.gy);
  const bool taps = !(a.KH == 1 && a.KW == 1 && a.pad == 0);
  if constexpr (std::is_same<T, fp8e4>::value) {                // (kernel 10: the only one with e4m3 operands)
    if (taps) launch256<T, true>(a, grid, st, ws, ws_bytes);
    else launch256<T, false>(a, grid, st, ws, ws_bytes);
  } else if (p.kernel == 11) {
    if (taps) launch_fwd2<T, true>(a, grid, st);
    else launch_fwd2<T, false>(a, grid, st);
  } else {
    if (a.res_pool) hipLaunchKernelGGL((k_conv_fwd256<T, false, true>), grid, dim3(512), 0, st, a);
    else if (taps) launch256<T, true>(a, grid, st, ws, ws_bytes);
    else launch256<T, false>(a, grid, st, ws, ws_bytes);
  }
}

}  // namespace

void launch_fwd_tile256(const ConvArgs& a, const Plan& p, Operand op, hipStream_t st, void* ws, long ws_bytes) {
  if (op == OP_BF16) launch_tile256<__bf16>(a, p, st, ws, ws_bytes);
  else if (op == OP_F32) launch_tile256<float>(a, p, st, ws, ws_bytes);
  else launch_tile256<fp8e4>(a, p, st, ws, ws_bytes);
}
