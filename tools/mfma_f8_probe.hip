// What one v_mfma_scale_f32_32x32x64_f8f6f4 (gfx950; OCP e4m3 operands, unit E8M0 scales) does to its 64-term dot product: the
// probe issues SINGLE instructions on operands it builds itself and compares every output with the float64 sum of the same
// products plus the accumulator, computed on the host (products of two e4m3 numbers and sums of 65 such terms are exact in
// float64).  Independent of the library's kernels: tests/exact_fp8.py takes its constant T_MFMA from the figures printed here.
//
//   ratio  = |got - exact| / max_k |a_k * b_k|                                (the unit of the bound's per-instruction term)
//   excess = max(0, |got - exact| - 2^-24 * |exact|) / max_k |a_k * b_k|      (what is left after the f32 rounding of the result
//                                                                              itself, which the accumulation term of the bound covers)
// Patterns:
//   (a)  random e4m3 bytes (every finite code, subnormals included) and Gaussian values quantised to a maximum of 448; accumulator 0
//   (b)  one product of 2^j (j = 0..16; j = 17: 448 * 320) among 63 products of 1, and among 63 products of 1.125^2
//   (c)  accumulator 2^j (j = 0..24) plus 64 products of 1, and plus 64 products of 2^-9 * 1
//   (d)  integer operands |v| <= vmax on an integer accumulator |c| <= cmax: bit-exact or not (the tier A regime is vmax 4, cmax 2^17)
// One wave per problem; lane (r, h) holds bytes [32 h, 32 h + 32) of row r of A and of row r of B (= column r of the product), as
// k_fp8_dot_nt does; output register g of lane (j, h) is row (g & 3) + 8 (g >> 2) + 4 h of column j.
// build + run (GPU box): hipcc --offload-arch=gfx950 -O2 tools/mfma_f8_probe.hip -o mfma_f8_probe && ./mfma_f8_probe
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

typedef __attribute__((ext_vector_type(8))) int i32x8;
typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(4))) unsigned u32x4;

__global__ __launch_bounds__(64) void k_probe(const unsigned char* a, const unsigned char* b, const float* c, float* d, int nprob) {
  const int p = blockIdx.x;
  if (p >= nprob) return;
  const int lane = threadIdx.x, r = lane & 31, h = lane >> 5;
  const unsigned char* pa = a + (size_t)p * 2048 + r * 64 + 32 * h;
  const unsigned char* pb = b + (size_t)p * 2048 + r * 64 + 32 * h;
  const u32x4 a0 = *(const u32x4*)pa, a1 = *(const u32x4*)(pa + 16), b0 = *(const u32x4*)pb, b1 = *(const u32x4*)(pb + 16);
  const i32x8 fa = {(int)a0[0], (int)a0[1], (int)a0[2], (int)a0[3], (int)a1[0], (int)a1[1], (int)a1[2], (int)a1[3]};
  const i32x8 fb = {(int)b0[0], (int)b0[1], (int)b0[2], (int)b0[3], (int)b1[0], (int)b1[1], (int)b1[2], (int)b1[3]};
  f32x16 acc;
#pragma unroll
  for (int g = 0; g < 16; ++g) acc[g] = c[(size_t)p * 1024 + ((g & 3) + 8 * (g >> 2) + 4 * h) * 32 + r];
  acc = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(fa, fb, acc, 0, 0, 0, 0x7f7f7f7f, 0, 0x7f7f7f7f);
#pragma unroll
  for (int g = 0; g < 16; ++g) d[(size_t)p * 1024 + ((g & 3) + 8 * (g >> 2) + 4 * h) * 32 + r] = acc[g];
}

static double deq(unsigned char v) {              // OCP e4m3fn: 1-4-3, bias 7, no infinity, 0x7f / 0xff are NaN
  const int e = (v >> 3) & 15, m = v & 7;
  const double mag = e == 0 ? std::ldexp((double)m, -9) : std::ldexp(1.0 + m / 8.0, e - 7);
  return (v & 0x80) ? -mag : mag;
}

static unsigned char enc(double x) {              // nearest e4m3 code (ties to even), saturating at 448
  unsigned char best = 0;
  double bd = 1e300;
  for (int v = 0; v < 256; ++v) {
    if ((v & 0x7f) == 0x7f) continue;
    const double dd = std::fabs(deq((unsigned char)v) - x);
    if (dd < bd || (dd == bd && !(v & 1) && (best & 1))) { bd = dd; best = (unsigned char)v; }
  }
  return best;
}

struct Batch {
  std::vector<unsigned char> a, b;
  std::vector<float> c, d;
  int n = 0;
  int add() { a.resize((size_t)(n + 1) * 2048, 0); b.resize((size_t)(n + 1) * 2048, 0); c.resize((size_t)(n + 1) * 1024, 0.f); return n++; }
};

#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { std::printf("HIP error %s at line %d\n", hipGetErrorString(e_), __LINE__); std::exit(2); } } while (0)

static void run(Batch& t) {
  unsigned char *da, *db; float *dc, *dd;
  CHECK(hipMalloc(&da, t.a.size())); CHECK(hipMalloc(&db, t.b.size()));
  CHECK(hipMalloc(&dc, t.c.size() * 4)); CHECK(hipMalloc(&dd, t.c.size() * 4));
  CHECK(hipMemcpy(da, t.a.data(), t.a.size(), hipMemcpyHostToDevice)); CHECK(hipMemcpy(db, t.b.data(), t.b.size(), hipMemcpyHostToDevice));
  CHECK(hipMemcpy(dc, t.c.data(), t.c.size() * 4, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(k_probe, dim3(t.n), dim3(64), 0, 0, da, db, dc, dd, t.n);
  CHECK(hipGetLastError()); CHECK(hipDeviceSynchronize());
  t.d.resize(t.c.size());
  CHECK(hipMemcpy(t.d.data(), dd, t.c.size() * 4, hipMemcpyDeviceToHost));
  CHECK(hipFree(da)); CHECK(hipFree(db)); CHECK(hipFree(dc)); CHECK(hipFree(dd));
}

struct Stat { double ratio = 0, excess = 0, err = 0, got = 0, exact = 0, pmax = 0; long n = 0, wrong = 0; };

// problems [p0, p1) of a batch against float64
static Stat judge(const Batch& t, int p0, int p1) {
  Stat s;
  for (int p = p0; p < p1; ++p)
    for (int i = 0; i < 32; ++i)
      for (int j = 0; j < 32; ++j) {
        double ex = t.c[(size_t)p * 1024 + i * 32 + j], pm = 0;
        for (int k = 0; k < 64; ++k) {
          const double pr = deq(t.a[(size_t)p * 2048 + i * 64 + k]) * deq(t.b[(size_t)p * 2048 + j * 64 + k]);
          ex += pr;
          if (std::fabs(pr) > pm) pm = std::fabs(pr);
        }
        const double got = t.d[(size_t)p * 1024 + i * 32 + j], err = std::fabs(got - ex);
        ++s.n;
        if (err != 0) ++s.wrong;
        if (pm == 0) continue;
        const double r = err / pm, x = std::fmax(0.0, err - std::ldexp(std::fabs(ex), -24)) / pm;
        if (x > s.excess) s.excess = x;
        if (r > s.ratio) { s.ratio = r; s.err = err; s.got = got; s.exact = ex; s.pmax = pm; }
      }
  return s;
}

static void show(const char* name, const Stat& s) {
  std::printf("%-34s outputs %8ld inexact %8ld  worst ratio %.6g (2^%.2f)  excess %.6g  [got %.10g exact %.10g pmax %.6g]\n", name, s.n, s.wrong,
              s.ratio, s.ratio > 0 ? std::log2(s.ratio) : -999.0, s.excess, s.got, s.exact, s.pmax);
}

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() { rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(rng_state >> 33); }
static double gauss() {
  double u1 = (rnd() + 1.0) / 2147483649.0, u2 = rnd() / 2147483648.0;
  return std::sqrt(-2.0 * std::log(u1)) * std::cos(6.283185307179586 * u2);
}

int main() {
  double fig[4] = {0, 0, 0, 0};      // worst figure per pattern: (a) ratio, (b) ratio, (c) excess, (d) inexact outputs at vmax 4
  // ---- (a) random operands, zero accumulator
  {
    Batch t;
    const int NR = 512;
    for (int p = 0; p < NR; ++p) {                     // every finite code equally likely
      const int q = t.add();
      for (int i = 0; i < 2048; ++i) {
        unsigned char v; do v = (unsigned char)rnd(); while ((v & 0x7f) == 0x7f); t.a[(size_t)q * 2048 + i] = v;
        do v = (unsigned char)rnd(); while ((v & 0x7f) == 0x7f); t.b[(size_t)q * 2048 + i] = v;
      }
    }
    for (int p = 0; p < NR; ++p) {
      const int q = t.add();
      for (int i = 0; i < 2048; ++i) {
        t.a[(size_t)q * 2048 + i] = enc(std::fmax(-448.0, std::fmin(448.0, gauss() * 112.0)));
        t.b[(size_t)q * 2048 + i] = enc(std::fmax(-448.0, std::fmin(448.0, gauss() * 112.0)));
      }
    }
    for (int p = 0; p < NR; ++p) {                     // small codes only (exponent field <= 3: subnormals and their neighbours) against Gaussian
      const int q = t.add();
      for (int i = 0; i < 2048; ++i) {
        t.a[(size_t)q * 2048 + i] = (unsigned char)((rnd() & 0x9f));
        t.b[(size_t)q * 2048 + i] = enc(std::fmax(-448.0, std::fmin(448.0, gauss() * 112.0)));
      }
    }
    run(t);
    Stat s0 = judge(t, 0, NR), s1 = judge(t, NR, 2 * NR), s2 = judge(t, 2 * NR, 3 * NR);
    show("(a) uniform codes", s0); show("(a) gaussian to 448", s1); show("(a) small codes x gaussian", s2);
    fig[0] = std::fmax(s0.ratio, std::fmax(s1.ratio, s2.ratio));
  }
  // ---- (b) one large product among 63 small ones
  for (int var = 0; var < 2; ++var) {
    const unsigned char small = enc(var ? 1.125 : 1.0);
    for (int j = 0; j <= 17; ++j) {
      Batch t;
      for (int k0 = 0; k0 < 64; k0 += 9) {
        const int q = t.add();
        for (int i = 0; i < 2048; ++i) t.a[(size_t)q * 2048 + i] = t.b[(size_t)q * 2048 + i] = small;
        const double big_a = j <= 16 ? std::ldexp(1.0, j / 2) : 448.0, big_b = j <= 16 ? std::ldexp(1.0, j - j / 2) : 320.0;
        for (int r = 0; r < 32; ++r) { t.a[(size_t)q * 2048 + r * 64 + k0] = enc(big_a); t.b[(size_t)q * 2048 + r * 64 + k0] = enc((r & 1) ? -big_b : big_b); }
      }
      run(t);
      const Stat s = judge(t, 0, t.n);
      char nm[64]; std::snprintf(nm, sizeof nm, "(b) 2^%d + 63 x %s", j, var ? "1.125^2" : "1");
      show(nm, s);
      // in units of the SMALL products too: how much of the 63 addends is lost
      std::printf("      error / small product: %.6g\n", s.err / (var ? 1.265625 : 1.0));
      if (s.ratio > fig[1]) fig[1] = s.ratio;
    }
  }
  // ---- (c) non-zero accumulator
  for (int var = 0; var < 2; ++var)
    for (int j = 0; j <= 24; ++j) {
      Batch t;
      const int q = t.add();
      for (int i = 0; i < 2048; ++i) { t.a[(size_t)q * 2048 + i] = var ? 0x01 : enc(1.0); t.b[(size_t)q * 2048 + i] = enc(1.0); }
      for (int i = 0; i < 1024; ++i) t.c[(size_t)q * 1024 + i] = (float)((i & 1) ? -std::ldexp(1.0, j) : std::ldexp(1.0, j));
      run(t);
      const Stat s = judge(t, 0, t.n);
      char nm[64]; std::snprintf(nm, sizeof nm, "(c) acc 2^%d + 64 x %s", j, var ? "2^-9" : "1");
      show(nm, s);
      if (s.excess > fig[2]) fig[2] = s.excess;
    }
  // ---- (d) integers on an integer accumulator
  {
    const int vmaxs[4] = {4, 8, 16, 16}, cexp[4] = {17, 20, 23, 24};
    for (int v = 0; v < 4; ++v) {
      Batch t;
      for (int p = 0; p < 256; ++p) {
        const int q = t.add(), vm = vmaxs[v];
        for (int i = 0; i < 2048; ++i) {
          t.a[(size_t)q * 2048 + i] = (rnd() & 7) == 0 ? 0 : enc((double)((int)(rnd() % (2 * vm + 1)) - vm));
          t.b[(size_t)q * 2048 + i] = (rnd() & 7) == 0 ? 0 : enc((double)((int)(rnd() % (2 * vm + 1)) - vm));
        }
        const long cm = (1L << cexp[v]) - 64L * vm * vm;          // |c| + 64 vmax^2 <= 2^cexp
        for (int i = 0; i < 1024; ++i) {
          long c = (long)(((uint64_t)rnd() << 16 ^ rnd()) % (uint64_t)(2 * cm + 1)) - cm;
          if ((i & 7) == 0) c = (i & 8) ? cm : -cm;                 // and the extremes
          t.c[(size_t)q * 1024 + i] = (float)c;
        }
      }
      run(t);
      const Stat s = judge(t, 0, t.n);
      char nm[64]; std::snprintf(nm, sizeof nm, "(d) |v| <= %d, |result| <= 2^%d", vmaxs[v], cexp[v]);
      show(nm, s);
      if (v == 0) fig[3] = (double)s.wrong;
    }
  }
  std::printf("FIGURES (a) worst ratio %.6g  (b) worst ratio %.6g  (c) worst excess %.6g  (d) inexact outputs at |v| <= 4, 2^17: %.0f\n", fig[0], fig[1],
              fig[2], fig[3]);
  return 0;
}
