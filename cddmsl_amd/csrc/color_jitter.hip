// Photometric augmentation of the training loader (INPUT.COLOR_JITTER with DATALOADER.DEVICE_RESIZE) on gfx950:
// cddmsl_color_jitter_batch_u8 -- the reference's RandomBrightness / RandomContrast / RandomSaturation / RandomLighting
// (data/transforms/augmentation_impl.py:493-600), each a BlendTransform on uint8, chained in that fixed order IN PLACE on the planar
// [3][h][w] images cddmsl_resize_batch_u8 has just made.  Linked into a library of its own (include/cddmsl_color_jitter.h says why).
//
// The arithmetic is the canonical one of cddmsl_amd/augment.py::color_jitter_u8, bit for bit: float32 with every product and sum
// rounded on its own (contraction is off for this file whatever the command line says), trunc(min(max(v, 0), 255)) after each blend.
//
// Two kernels, both flat ONE-SHOT grids over fixed-size chunks of all items of a batch that travels by value (the item of a
// workgroup: a short uniform scan of the chunk prefix, as in k_resize_batch_u8), so every branch on an item's operations is
// workgroup-uniform:
//   k_jitter_sum    items with contrast only: the integer sum of the item's 3 h w bytes after the brightness step (recomputed on the
//                   fly, nothing written), 16-byte loads over the item's flat byte range, per-thread u32 -> wave shuffle -> LDS ->
//                   ONE 64-bit integer atomic per workgroup.  Integer addition: exact in any order, so two calls give the same bytes.
//   k_jitter_apply  a thread takes the three channel bytes of a run of pixels (saturation needs all three), chains the active
//                   operations in registers and stores once.  The three planes of a pixel run lie h w bytes apart, so all three are
//                   16-byte (4-byte) aligned together only when h w is a multiple of 16 (4): such an item runs 16-byte (4-byte)
//                   accesses over its body, with a scalar head up to the first aligned address and a scalar tail; any other item runs
//                   byte accesses (still consecutive lanes on consecutive bytes).  The short edges the shipped configs sample are
//                   multiples of 16, so h w is one unless MAX_SIZE_TRAIN caps the long edge.
// Plain vector loads and stores and one integer atomic per workgroup; no floating-point atomics.
#include "common.h"
#include "cddmsl_color_jitter.h"   // the compiler checks the entry point's definition against its declaration

#pragma clang fp contract(off)

namespace {

constexpr int JT_MAX = 32;                     // items per launch (16 pairs), as RS_MAX
constexpr int JT_NT = 256;
constexpr int JT_PIX = JT_NT * 16;             // pixels of the body per apply workgroup: 12 KiB read, 12 KiB written
constexpr int JT_SUM = JT_NT * 16 * 4;         // bytes of the body per sum workgroup: four 16-byte loads a thread, one atomic per 16 KiB
enum { OP_B = 1, OP_C = 2, OP_S = 4, OP_L = 8 };

struct JtBatch { cddmsl_jitter_item it[JT_MAX]; int sum0[JT_MAX + 1]; int app0[JT_MAX + 1]; int count; };
static_assert(sizeof(cddmsl_jitter_item) == 64, "cddmsl_jitter_item is 64 bytes without implicit padding");
static_assert(sizeof(JtBatch) + 16 + 256 <= 4096, "JtBatch + two pointers + hidden arguments exceed the kernel-argument limit");

// access width of an item's apply pass (16, 4 or 1 bytes a plane) and the pixels in front of the first aligned one; host and device
__host__ __device__ inline void apply_split(size_t addr, long n, int& width, long& head) {
  width = n % 16 == 0 ? 16 : (n % 4 == 0 ? 4 : 1);
  head = (long)((width - (addr & (size_t)(width - 1))) & (size_t)(width - 1));
  if (head > n) head = n;
}
inline long chunks_of(long body, long per) { const long c = (body + per - 1) / per; return c > 0 ? c : 1; }   // (chunk 0 also takes the head)

__device__ __forceinline__ float f32_of(int bits) { return __builtin_bit_cast(float, bits); }

// one BlendTransform on a byte value held as a float: ss = fl32(sw * src); the result is an integer in [0, 255] again
__device__ __forceinline__ float blend(float ss, float dw, float x) {
  const float v = ss + dw * x;
  return (float)(int)fminf(fmaxf(v, 0.f), 255.f);
}

struct JtConst {
  int ops, bgr;
  float b_ss, b_dw, c_ss, c_dw, s_sw, s_dw, l0, l1, l2;   // l0..l2: fl32(1 * offset) of planes 0..2
};

__device__ __forceinline__ JtConst consts_of(const cddmsl_jitter_item& t, float mean) {
  JtConst k;
  k.ops = t.ops; k.bgr = t.bgr;
  k.b_dw = f32_of(t.b_dw); k.b_ss = f32_of(t.b_sw) * 0.f;
  k.c_dw = f32_of(t.c_dw); k.c_ss = f32_of(t.c_sw) * mean;
  k.s_dw = f32_of(t.s_dw); k.s_sw = f32_of(t.s_sw);
  k.l0 = 1.f * f32_of(t.bgr ? t.light_b : t.light_r); k.l1 = 1.f * f32_of(t.light_g); k.l2 = 1.f * f32_of(t.bgr ? t.light_r : t.light_b);
  return k;
}

__device__ __forceinline__ void jitter_px(const JtConst& k, float& x0, float& x1, float& x2) {
  if (k.ops & OP_B) { x0 = blend(k.b_ss, k.b_dw, x0); x1 = blend(k.b_ss, k.b_dw, x1); x2 = blend(k.b_ss, k.b_dw, x2); }
  if (k.ops & OP_C) { x0 = blend(k.c_ss, k.c_dw, x0); x1 = blend(k.c_ss, k.c_dw, x1); x2 = blend(k.c_ss, k.c_dw, x2); }
  if (k.ops & OP_S) {
    const float r = k.bgr ? x2 : x0, b = k.bgr ? x0 : x2;
    const float grey = (0.299f * r + 0.587f * x1) + 0.114f * b;
    const float ss = k.s_sw * grey;
    x0 = blend(ss, k.s_dw, x0); x1 = blend(ss, k.s_dw, x1); x2 = blend(ss, k.s_dw, x2);
  }
  if (k.ops & OP_L) { x0 = blend(k.l0, 1.f, x0); x1 = blend(k.l1, 1.f, x1); x2 = blend(k.l2, 1.f, x2); }
}

__device__ __forceinline__ void jitter_one(const JtConst& k, unsigned char* p, long n, long i) {
  float x0 = (float)p[i], x1 = (float)p[n + i], x2 = (float)p[2 * n + i];
  jitter_px(k, x0, x1, x2);
  p[i] = (unsigned char)x0; p[n + i] = (unsigned char)x1; p[2 * n + i] = (unsigned char)x2;
}

// four pixels: one 32-bit word of each plane in, one out
__device__ __forceinline__ void jitter_word(const JtConst& k, unsigned& w0, unsigned& w1, unsigned& w2) {
  unsigned o0 = 0, o1 = 0, o2 = 0;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    float x0 = (float)((w0 >> (8 * q)) & 255u), x1 = (float)((w1 >> (8 * q)) & 255u), x2 = (float)((w2 >> (8 * q)) & 255u);
    jitter_px(k, x0, x1, x2);
    o0 |= (unsigned)x0 << (8 * q); o1 |= (unsigned)x1 << (8 * q); o2 |= (unsigned)x2 << (8 * q);
  }
  w0 = o0; w1 = o1; w2 = o2;
}

// the groups [s, s + ng * W) of a chunk's body, W pixels a thread and step; p + i, p + n + i, p + 2 n + i are W-byte aligned
template <int W>
__device__ __forceinline__ void apply_groups(const JtConst& k, unsigned char* p, long n, long s, int ng) {
  for (int g = threadIdx.x; g < ng; g += JT_NT) {
    const long i = s + (long)g * W;
    if (W == 16) {
      u32x4 a = *(const u32x4*)(p + i), b = *(const u32x4*)(p + n + i), c = *(const u32x4*)(p + 2 * n + i);
#pragma unroll
      for (int q = 0; q < 4; ++q) { unsigned w0 = a[q], w1 = b[q], w2 = c[q]; jitter_word(k, w0, w1, w2); a[q] = w0; b[q] = w1; c[q] = w2; }
      *(u32x4*)(p + i) = a; *(u32x4*)(p + n + i) = b; *(u32x4*)(p + 2 * n + i) = c;
    } else if (W == 4) {
      unsigned w0 = *(const unsigned*)(p + i), w1 = *(const unsigned*)(p + n + i), w2 = *(const unsigned*)(p + 2 * n + i);
      jitter_word(k, w0, w1, w2);
      *(unsigned*)(p + i) = w0; *(unsigned*)(p + n + i) = w1; *(unsigned*)(p + 2 * n + i) = w2;
    } else {
      jitter_one(k, p, n, i);
    }
  }
}

__global__ void __launch_bounds__(JT_NT) k_jitter_apply(JtBatch b, unsigned char* __restrict__ buf, const unsigned long long* __restrict__ sums) {
  __shared__ float s_mean;
  const int bid = blockIdx.x;
  int j = 0;
  while (j + 1 < b.count && bid >= b.app0[j + 1]) ++j;      // workgroup-uniform; an item without work has an empty chunk range
  const cddmsl_jitter_item& t = b.it[j];
  const long n = (long)t.h * t.w;
  unsigned char* p = buf + t.off;
  if (t.ops & OP_C) {                                        // workgroup-uniform
    if (threadIdx.x == 0) s_mean = (float)((double)sums[j] / (double)(3 * n));
    __syncthreads();
  }
  const JtConst k = consts_of(t, (t.ops & OP_C) ? s_mean : 0.f);
  int width;
  long head;
  apply_split((size_t)p, n, width, head);
  const long c = bid - b.app0[j];
  const long s = head + c * JT_PIX;                          // this chunk's body [s, e), inside [head, n)
  const long e = s + JT_PIX < n ? s + JT_PIX : n;
  if (c == 0 && (long)threadIdx.x < head) jitter_one(k, p, n, threadIdx.x);          // head < 16 pixels
  if (s >= e) return;
  const int ng = (int)((e - s) / width);
  if (width == 16) apply_groups<16>(k, p, n, s, ng);
  else if (width == 4) apply_groups<4>(k, p, n, s, ng);
  else apply_groups<1>(k, p, n, s, ng);
  const long tail = s + (long)ng * width + threadIdx.x;      // fewer than `width` pixels, in the item's last chunk only
  if (tail < e) jitter_one(k, p, n, tail);
}

__device__ __forceinline__ unsigned sum_byte(bool bright, float b_ss, float b_dw, unsigned x) {
  return bright ? (unsigned)blend(b_ss, b_dw, (float)x) : x;
}

__global__ void __launch_bounds__(JT_NT) k_jitter_sum(JtBatch b, const unsigned char* __restrict__ buf, unsigned long long* __restrict__ sums) {
  __shared__ unsigned part[JT_NT / 64];
  const int bid = blockIdx.x;
  int j = 0;
  while (j + 1 < b.count && bid >= b.sum0[j + 1]) ++j;      // workgroup-uniform
  const cddmsl_jitter_item& t = b.it[j];
  const long m = 3L * t.h * t.w;                             // the item's bytes as one flat range
  const unsigned char* p = buf + t.off;
  const bool bright = t.ops & OP_B;
  const float b_dw = f32_of(t.b_dw), b_ss = f32_of(t.b_sw) * 0.f;
  long head = (long)((16 - ((size_t)p & 15)) & 15);
  if (head > m) head = m;
  const long c = bid - b.sum0[j];
  const long s = head + c * JT_SUM;
  const long e = s + JT_SUM < m ? s + JT_SUM : m;
  unsigned acc = 0;                                          // at most 66 bytes of 255 a thread
  if (c == 0 && (long)threadIdx.x < head) acc += sum_byte(bright, b_ss, b_dw, p[threadIdx.x]);
  if (s < e) {
    const int ng = (int)((e - s) >> 4);
    for (int g = threadIdx.x; g < ng; g += JT_NT) {
      const u32x4 v = *(const u32x4*)(p + s + (long)g * 16);
#pragma unroll
      for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int r = 0; r < 4; ++r) acc += sum_byte(bright, b_ss, b_dw, (v[q] >> (8 * r)) & 255u);
    }
    const long tail = s + (long)ng * 16 + threadIdx.x;
    if (tail < e) acc += sum_byte(bright, b_ss, b_dw, p[tail]);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc += (unsigned)__shfl_xor((int)acc, o, 64);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long tot = 0;
    for (int i = 0; i < JT_NT / 64; ++i) tot += part[i];
    atomicAdd(&sums[j], tot);
  }
}

inline bool finite_bits(int bits) { return ((unsigned)bits & 0x7f800000u) != 0x7f800000u; }

// positive sizes, a known operation set, the three planes inside the buffer, finite weights of the active operations
bool item_ok(const cddmsl_jitter_item& t, long buf_bytes) {
  if (t.h <= 0 || t.w <= 0 || t.ops < 0 || t.ops > 15) return false;
  const long n = (long)t.h * t.w;
  if (n > buf_bytes / 3) return false;
  if (t.off < 0 || t.off > buf_bytes || 3 * n > buf_bytes - t.off) return false;
  if ((t.ops & OP_B) && !(finite_bits(t.b_dw) && finite_bits(t.b_sw))) return false;
  if ((t.ops & OP_C) && !(finite_bits(t.c_dw) && finite_bits(t.c_sw))) return false;
  if ((t.ops & OP_S) && !(finite_bits(t.s_dw) && finite_bits(t.s_sw))) return false;
  if ((t.ops & OP_L) && !(finite_bits(t.light_r) && finite_bits(t.light_g) && finite_bits(t.light_b))) return false;
  return true;
}

long sum_chunks(const cddmsl_jitter_item& t, const unsigned char* buf) {
  if (!(t.ops & OP_C)) return 0;
  const long m = 3L * t.h * t.w;
  long head = (long)((16 - ((size_t)(buf + t.off) & 15)) & 15);
  if (head > m) head = m;
  return chunks_of(m - head, JT_SUM);
}

long apply_chunks(const cddmsl_jitter_item& t, const unsigned char* buf) {
  if (!t.ops) return 0;
  const long n = (long)t.h * t.w;
  int width;
  long head;
  apply_split((size_t)(buf + t.off), n, width, head);
  return chunks_of(n - head, JT_PIX);
}

}  // namespace

extern "C" int cddmsl_color_jitter_batch_u8(unsigned char* buf, long buf_bytes, const cddmsl_jitter_item* items, int count, long* sums,
                                            void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (count < 0 || buf_bytes < 0) return CDDMSL_ERR_ARG;
  if (count == 0) return CDDMSL_OK;
  if (!buf || !items) return CDDMSL_ERR_ARG;
  bool any = false, contrast = false;
  long ns = 0, na = 0;
  for (int i = 0; i < count; ++i) {                           // every item of every chunk BEFORE the first HIP call
    const cddmsl_jitter_item& t = items[i];
    if (!item_ok(t, buf_bytes)) return CDDMSL_ERR_ARG;
    any = any || t.ops;
    contrast = contrast || (t.ops & OP_C);
    if (i % JT_MAX == 0) ns = na = 0;
    ns += sum_chunks(t, buf);
    na += apply_chunks(t, buf);
    if (ns > 0x7fffffffL || na > 0x7fffffffL) return CDDMSL_ERR_ARG;   // a launch's flat grid
  }
  if (contrast && !sums) return CDDMSL_ERR_ARG;
  if (!any) return CDDMSL_OK;
  if (sums && hipMemsetAsync(sums, 0, (size_t)count * sizeof(long), st) != hipSuccess) return CDDMSL_ERR_LAUNCH;
  for (int base = 0; base < count; base += JT_MAX) {
    JtBatch b{};
    b.count = count - base < JT_MAX ? count - base : JT_MAX;
    int s = 0, a = 0;
    for (int i = 0; i < b.count; ++i) {
      b.it[i] = items[base + i];
      b.sum0[i] = s;
      b.app0[i] = a;
      s += (int)sum_chunks(b.it[i], buf);
      a += (int)apply_chunks(b.it[i], buf);
    }
    for (int i = b.count; i <= JT_MAX; ++i) { b.sum0[i] = s; b.app0[i] = a; }
    unsigned long long* sm = (unsigned long long*)sums + (sums ? base : 0);
    if (s) k_jitter_sum<<<dim3((unsigned)s), dim3(JT_NT), 0, st>>>(b, buf, sm);
    if (a) k_jitter_apply<<<dim3((unsigned)a), dim3(JT_NT), 0, st>>>(b, buf, sm);
  }
  return launch_status();
}
