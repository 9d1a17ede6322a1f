// Test-time-augmentation views (detectron2/modeling/test_time_augmentation.py:58-98, DatasetMapperTTA) made on the device:
// one u8 CHW image -> PIL-exact bilinear resize to (newh, neww) -> (x/div - mean)/std -> zero-padded NHWC slot, and the same view
// mirrored left-right into a second slot, in ONE launch.  The host never sees a view.
//
// The resize is Pillow's ImagingResample (bilinear, 8 bits per channel), reproduced bit for bit:
//   * two separable passes, horizontal first, with a uint8 intermediate between them;
//   * per output index a window [min, min + n) of the input axis and n <= ksize coefficients, int(0.5 + w * 2^22) of the normalised
//     triangle weights.  The tables are built on the HOST in double (cddmsl_amd/hip.py:_resample_table) in Pillow's order of
//     operations and only READ here: recomputing one on the device (contraction, another rounding) changes pixels;
//   * each pass is clip8((2^21 + sum k * pixel) >> 22).  The coefficients of one output sum to 2^22 up to rounding and are never
//     negative, so the sum stays below 255 * 2^22 + 2^21 + ksize * 255 < 2^31: the int32 accumulator is exact;
//   * a pass whose size does not change is skipped (the pixels are copied), as Pillow skips it: its table is not the identity.
// The normalisation is the expression of preprocess_px (elementwise.hip), so a slot is bit-equal to cddmsl_preprocess_batch of the
// resized uint8 view.
//
// One workgroup makes a TH x TW tile of the padded output: it resamples the input rows the tile's vertical windows cover
// horizontally into LDS (uint8, 3 planes), runs the vertical pass from LDS, and writes each pixel as one 16-byte store (Cp = 8
// bf16 / 4 f32) to the plain slot at column x and to the mirrored slot at column neww - 1 - x.  In the horizontal pass a thread owns
// one tile column (window and coefficients in registers across the rows); in the vertical pass a wave is one output row, so the
// window and coefficients are wave-uniform.  A tile whose rows do not fit the LDS buffer (vertical scale beyond ~4)
// recomputes the horizontal taps per vertical tap instead: slower, same values.
#include "common.h"

namespace {

constexpr int TH = 16, TW = 64, NT = 256;      // output tile, threads (4 pixels per thread)
constexpr int RMAX = 80;                       // horizontally resampled rows kept in LDS: TH * 4 + 2 * 4 + 1 = 73 at scale 4
constexpr int PREC = 22;                       // Pillow's PRECISION_BITS
constexpr int KREG = 5;                        // horizontal coefficients a thread keeps in registers
static_assert(NT % TW == 0, "a thread owns one tile column");

__device__ __forceinline__ int clip8(int v) {
  v >>= PREC;
  return v < 0 ? 0 : (v > 255 ? 255 : v);
}

struct Axis { const int* lo; const int* n; const int* k; int ks; };   // window start, length, coefficients [out][ks]; lo == null: copy

struct Dst { char* out; int n, Hp, Wp; };

// the horizontal pass for one (plane row, output column)
__device__ __forceinline__ int hpass(const unsigned char* row, int x, int w, const Axis& ax) {
  if (!ax.lo) return row[x];
  const int lo = ax.lo[x];
  int n = ax.n[x];
  n = n < ax.ks ? n : ax.ks;
  const int* k = ax.k + (long)x * ax.ks;
  int s = 1 << (PREC - 1);
  for (int t = 0; t < n; ++t) {
    int xi = lo + t;
    xi = xi < 0 ? 0 : (xi < w ? xi : w - 1);        // (a valid table never reaches the clamp: it keeps a bad one inside the image)
    s += (int)row[xi] * k[t];
  }
  return clip8(s);
}

template <typename T> struct Px;
template <> struct Px<__bf16> {
  static constexpr int ES = 2, VEC = 8;
  __device__ static __forceinline__ u32x4 pack(float a, float b, float c) { return u32x4{pack2bf(a, b), pack2bf(c, 0.f), 0u, 0u}; }
  __device__ static __forceinline__ void st(char* p, float v) { *(unsigned short*)p = f2bf(v); }
};
template <> struct Px<float> {
  static constexpr int ES = 4, VEC = 4;
  __device__ static __forceinline__ u32x4 pack(float a, float b, float c) { return __builtin_bit_cast(u32x4, f32x4{a, b, c, 0.f}); }
  __device__ static __forceinline__ void st(char* p, float v) { *(float*)p = v; }
};

template <typename T>
__device__ __forceinline__ void store_px(const Dst& d, int y, int x, int Cp, float a, float b, float c) {
  char* p = d.out + ((((long)d.n * d.Hp + y) * d.Wp + x) * Cp) * Px<T>::ES;
  if (Cp == Px<T>::VEC) {                      // a pixel is one 16-byte chunk; written once and read by a later launch: non-temporal
    __builtin_nontemporal_store(Px<T>::pack(a, b, c), (u32x4*)p);
    return;
  }
  Px<T>::st(p, a); Px<T>::st(p + Px<T>::ES, b); Px<T>::st(p + 2 * Px<T>::ES, c);
  for (int ch = 3; ch < Cp; ++ch) Px<T>::st(p + ch * Px<T>::ES, 0.f);
}

template <typename T>
__global__ void __launch_bounds__(NT) k_tta_view(const unsigned char* __restrict__ img, int h, int w, int newh, int neww, Axis ax, Axis ay,
                                                 Dst d0, Dst d1, int Cp, float m0, float m1, float m2, float s0, float s1, float s2,
                                                 float div) {
  __shared__ unsigned char hrow[3 * RMAX * TW];
  const int x0 = blockIdx.x * TW, y0 = blockIdx.y * TH;
  const bool inside = y0 < newh && x0 < neww;       // block-uniform: the tile holds view pixels, not padding only
  int r0 = 0, nrows = 0;
  if (inside) {
    const int yl = (y0 + TH < newh ? y0 + TH : newh) - 1;
    if (ay.lo) {
      r0 = ay.lo[y0];
      const int nl = ay.n[yl] < ay.ks ? ay.n[yl] : ay.ks;
      nrows = ay.lo[yl] + nl - r0;                  // windows move monotonically with y
    } else {
      r0 = y0;
      nrows = yl + 1 - y0;
    }
  }
  const bool staged = inside && nrows <= RMAX;      // block-uniform
  const long plane = (long)h * w;
  if (staged) {
    // a thread keeps ONE column of the tile (NT is a multiple of TW) and walks the staged rows: its window and its first KREG
    // coefficients are read once and stay in registers (ksize <= 5 up to a horizontal ratio of 2; longer windows read the rest)
    const int cx = threadIdx.x % TW, x = x0 + cx;
    if (x < neww) {
      int lo = x, n = 0, kr[KREG];
      const int* k = nullptr;
      if (ax.lo) {
        lo = ax.lo[x];
        n = ax.n[x] < ax.ks ? ax.n[x] : ax.ks;
        k = ax.k + (long)x * ax.ks;
      }
#pragma unroll
      for (int t = 0; t < KREG; ++t) kr[t] = t < n ? k[t] : 0;
      for (int r = threadIdx.x / TW; r < nrows; r += NT / TW) {
        int yi = r0 + r;
        yi = yi < 0 ? 0 : (yi < h ? yi : h - 1);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const unsigned char* row = img + c * plane + (long)yi * w;
          int v;
          if (!ax.lo) {
            v = row[x];
          } else {
            int s = 1 << (PREC - 1);
#pragma unroll
            for (int t = 0; t < KREG; ++t) {
              int xi = lo + t;
              xi = xi < 0 ? 0 : (xi < w ? xi : w - 1);     // (a valid table never reaches the clamp)
              if (t < n) s += (int)row[xi] * kr[t];
            }
            for (int t = KREG; t < n; ++t) {
              int xi = lo + t;
              xi = xi < 0 ? 0 : (xi < w ? xi : w - 1);
              s += (int)row[xi] * k[t];
            }
            v = clip8(s);
          }
          hrow[(c * RMAX + r) * TW + cx] = (unsigned char)v;
        }
      }
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < TH * TW; i += NT) {
    const int cx = i % TW, x = x0 + cx, y = y0 + i / TW;
    if (y < newh && x < neww) {
      int v[3];
      if (!ay.lo) {
#pragma unroll
        for (int c = 0; c < 3; ++c)
          v[c] = staged ? hrow[(c * RMAX + (y - r0)) * TW + cx] : hpass(img + c * plane + (long)y * w, x, w, ax);
      } else {
        const int lo = ay.lo[y];
        int n = ay.n[y];
        n = n < ay.ks ? n : ay.ks;
        const int* k = ay.k + (long)y * ay.ks;
        int s[3] = {1 << (PREC - 1), 1 << (PREC - 1), 1 << (PREC - 1)};
        for (int t = 0; t < n; ++t) {
          const int kt = k[t];
          int yi = lo + t;
          yi = yi < 0 ? 0 : (yi < h ? yi : h - 1);
          int rr = yi - r0;                          // staged: inside [0, nrows) for a valid table
          rr = rr < 0 ? 0 : (rr < RMAX ? rr : RMAX - 1);
#pragma unroll
          for (int c = 0; c < 3; ++c)
            s[c] += kt * (staged ? (int)hrow[(c * RMAX + rr) * TW + cx] : hpass(img + c * plane + (long)yi * w, x, w, ax));
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = clip8(s[c]);
      }
      const float a = ((float)v[0] / div - m0) / s0, b = ((float)v[1] / div - m1) / s1, c = ((float)v[2] / div - m2) / s2;
      if (y < d0.Hp && x < d0.Wp) store_px<T>(d0, y, x, Cp, a, b, c);
      if (d1.out && y < d1.Hp && neww - 1 - x < d1.Wp) store_px<T>(d1, y, neww - 1 - x, Cp, a, b, c);
    } else {                                         // padding: the same position in both slots
      if (y < d0.Hp && x < d0.Wp) store_px<T>(d0, y, x, Cp, 0.f, 0.f, 0.f);
      if (d1.out && y < d1.Hp && x < d1.Wp) store_px<T>(d1, y, x, Cp, 0.f, 0.f, 0.f);
    }
  }
}

}  // namespace

// One TTA view and (out1 != NULL) its horizontal mirror.  img: device u8 [3][h][w].  The view (newh, neww) is written to slot n0 of
// out0 [N][Hp0][Wp0][Cp] and its mirror to slot n1 of out1 [N][Hp1][Wp1][Cp] (the two may be the same tensor or differently padded
// ones); the padding up to (Hp, Wp) and the channels 3..Cp are zeroed.  xlo / xn / xk [neww][xks] and ylo / yn / yk [newh][yks] are
// DEVICE int32 tables of Pillow's bilinear coefficients (22-bit fixed point) for the horizontal and vertical pass; the tables of a
// pass whose size does not change (neww == w, newh == h) are not read and may be NULL.  dtype 0 = bf16, 1 = f32.
extern "C" int cddmsl_tta_view(const unsigned char* img, int h, int w, int newh, int neww, const int* xlo, const int* xn, const int* xk,
                               int xks, const int* ylo, const int* yn, const int* yk, int yks, void* out0, int n0, int Hp0, int Wp0,
                               void* out1, int n1, int Hp1, int Wp1, int Cp, const float* mean3, const float* std3, int div255, int dtype,
                               void* stream) {
  if (!img || !out0 || !mean3 || !std3 || h <= 0 || w <= 0 || newh <= 0 || neww <= 0 || Cp < 3 || n0 < 0) return CDDMSL_ERR_ARG;
  if (newh > Hp0 || neww > Wp0) return CDDMSL_ERR_ARG;
  if (out1 && (n1 < 0 || newh > Hp1 || neww > Wp1)) return CDDMSL_ERR_ARG;
  if (neww != w && (!xlo || !xn || !xk || xks <= 0)) return CDDMSL_ERR_ARG;
  if (newh != h && (!ylo || !yn || !yk || yks <= 0)) return CDDMSL_ERR_ARG;
  if (dtype != 0 && dtype != 1) return CDDMSL_ERR_ARG;
  const Axis ax = neww != w ? Axis{xlo, xn, xk, xks} : Axis{nullptr, nullptr, nullptr, 0};
  const Axis ay = newh != h ? Axis{ylo, yn, yk, yks} : Axis{nullptr, nullptr, nullptr, 0};
  const Dst d0{(char*)out0, n0, Hp0, Wp0};
  const Dst d1 = out1 ? Dst{(char*)out1, n1, Hp1, Wp1} : Dst{nullptr, 0, 0, 0};
  const int Hm = Hp0 > d1.Hp ? Hp0 : d1.Hp, Wm = Wp0 > d1.Wp ? Wp0 : d1.Wp;
  const dim3 grid((unsigned)((Wm + TW - 1) / TW), (unsigned)((Hm + TH - 1) / TH));
  if (grid.y > 65535u) return CDDMSL_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  const float div = div255 ? 255.0f : 1.0f;
  if (dtype == 0)
    k_tta_view<__bf16><<<grid, dim3(NT), 0, st>>>(img, h, w, newh, neww, ax, ay, d0, d1, Cp, mean3[0], mean3[1], mean3[2], std3[0],
                                                  std3[1], std3[2], div);
  else
    k_tta_view<float><<<grid, dim3(NT), 0, st>>>(img, h, w, newh, neww, ax, ay, d0, d1, Cp, mean3[0], mean3[1], mean3[2], std3[0],
                                                 std3[1], std3[2], div);
  return launch_status();
}
