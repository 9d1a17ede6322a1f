// Test-time-augmentation views (detectron2/modeling/test_time_augmentation.py:58-98, DatasetMapperTTA) made on the device:
// one u8 CHW image -> PIL-exact bilinear resize to (newh, neww) -> (x/div - mean)/std -> zero-padded NHWC slot, and the same view
// mirrored left-right into a second slot, in ONE launch.  The host never sees a view.
//
// The resize is Pillow's ImagingResample (bilinear, 8 bits per channel), reproduced bit for bit from host-built coefficient tables
// (cddmsl_amd/resample.py); its arithmetic, the tile geometry and the LDS staging are resample.h, shared with loader_resize.hip.
// The normalisation is the expression of preprocess_px (elementwise.hip), so a slot is bit-equal to cddmsl_preprocess_batch of the
// resized uint8 view.
//
// One workgroup makes a TH x TW tile of the padded output: it resamples the input rows the tile's vertical windows cover
// horizontally into LDS (uint8, 3 planes), runs the vertical pass from LDS, and writes each pixel as one 16-byte store (Cp = 8
// bf16 / 4 f32) to the plain slot at column x and to the mirrored slot at column neww - 1 - x.  In the horizontal pass a thread owns
// one tile column (window and coefficients in registers across the rows); in the vertical pass a wave is one output row, so the
// window and coefficients are wave-uniform.  A tile whose rows do not fit the LDS buffer (vertical scale beyond ~4)
// recomputes the horizontal taps per vertical tap instead: slower, same values.
#include "resample.h"

namespace {

using namespace resample;      // tile geometry, the two passes and their LDS staging: shared with loader_resize.hip

struct Dst { char* out; int n, Hp, Wp; };

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
  __shared__ unsigned char hrow[HROW_BYTES];
  const int x0 = blockIdx.x * TW, y0 = blockIdx.y * TH;
  const bool inside = y0 < newh && x0 < neww;       // block-uniform: the tile holds view pixels, not padding only
  const Src<1> src{img, (long)h * w, (long)w};
  int r0 = 0, nrows = 0;
  if (inside) tile_rows(ay, y0, newh, r0, nrows);
  const bool staged = inside && nrows <= RMAX;      // block-uniform
  if (staged) stage_rows<1>(hrow, src, h, w, neww, ax, x0, r0, nrows);
  __syncthreads();
  for (int i = threadIdx.x; i < TH * TW; i += NT) {
    const int cx = i % TW, x = x0 + cx, y = y0 + i / TW;
    if (y < newh && x < neww) {
      int v[3];
      vpass<1, 3>(hrow, staged, src, 0, h, w, ax, ay, x, y, cx, r0, v);
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
