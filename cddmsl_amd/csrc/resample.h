// Pillow's bilinear ImagingResample (8 bits per channel) as device code, shared by the test-time-augmentation views (tta_views.hip)
// and the loader's batched resize (loader_resize.hip).  Both reproduce Pillow bit for bit:
//   * two separable passes, horizontal first, with a uint8 intermediate between them;
//   * per output index a window [min, min + n) of the input axis and n <= ksize coefficients, int(0.5 + w * 2^22) of the normalised
//     triangle weights.  The tables are built on the HOST in double (cddmsl_amd/resample.py) in Pillow's order of operations and
//     only READ here: recomputing one on the device (contraction, another rounding) changes pixels;
//   * each pass is clip8((2^21 + sum k * pixel) >> 22).  The coefficients of one output sum to 2^22 up to rounding and are never
//     negative, so the sum stays below 255 * 2^22 + 2^21 + ksize * 255 < 2^31: the int32 accumulator is exact;
//   * a pass whose size does not change is skipped (the pixels are copied), as Pillow skips it: its table is not the identity.
//
// One workgroup makes a TH x TW tile of the output: it resamples the input rows the tile's vertical windows cover horizontally into
// LDS (uint8, 3 planes; stage_rows) and runs the vertical pass from LDS (vpass).  In the horizontal pass a thread owns one tile
// column (window and coefficients in registers across the rows).  A tile whose rows do not fit the LDS buffer (vertical scale beyond
// ~4) recomputes the horizontal taps per vertical tap instead: slower, same values.
//
// The source layout is a template parameter: XS is the distance in bytes between horizontally adjacent pixels of one channel (1 for a
// planar image, 3 for an interleaved one), and Src gives the channel and row strides.
#pragma once
#include "common.h"

namespace resample {

constexpr int TH = 16, TW = 64, NT = 256;      // output tile, threads
constexpr int RMAX = 80;                       // horizontally resampled rows kept in LDS: TH * 4 + 2 * 4 + 1 = 73 at scale 4
constexpr int PREC = 22;                       // Pillow's PRECISION_BITS
constexpr int KREG = 5;                        // horizontal coefficients a thread keeps in registers
constexpr int HROW_BYTES = 3 * RMAX * TW;      // the LDS buffer a kernel declares for stage_rows / vpass
static_assert(NT % TW == 0, "a thread owns one tile column");

__device__ __forceinline__ int clip8(int v) {
  v >>= PREC;
  return v < 0 ? 0 : (v > 255 ? 255 : v);
}

struct Axis { const int* lo; const int* n; const int* k; int ks; };   // window start, length, coefficients [out][ks]; lo == null: copy

template <int XS>
struct Src {
  const unsigned char* p; long cs, rs;         // first byte, channel stride, row stride
  __device__ __forceinline__ const unsigned char* row(int c, int y) const { return p + c * cs + (long)y * rs; }
};

// the horizontal pass for one (plane row, output column)
template <int XS>
__device__ __forceinline__ int hpass(const unsigned char* row, int x, int w, const Axis& ax) {
  if (!ax.lo) return row[x * XS];
  const int lo = ax.lo[x];
  int n = ax.n[x];
  n = n < ax.ks ? n : ax.ks;
  const int* k = ax.k + (long)x * ax.ks;
  int s = 1 << (PREC - 1);
  for (int t = 0; t < n; ++t) {
    int xi = lo + t;
    xi = xi < 0 ? 0 : (xi < w ? xi : w - 1);        // (a valid table never reaches the clamp: it keeps a bad one inside the image)
    s += (int)row[xi * XS] * k[t];
  }
  return clip8(s);
}

// the input rows [r0, r0 + nrows) that the vertical windows of output rows [y0, min(y0 + TH, newh)) cover
__device__ __forceinline__ void tile_rows(const Axis& ay, int y0, int newh, int& r0, int& nrows) {
  const int yl = (y0 + TH < newh ? y0 + TH : newh) - 1;
  if (ay.lo) {
    r0 = ay.lo[y0];
    const int nl = ay.n[yl] < ay.ks ? ay.n[yl] : ay.ks;
    nrows = ay.lo[yl] + nl - r0;                    // windows move monotonically with y
  } else {
    r0 = y0;
    nrows = yl + 1 - y0;
  }
}

// horizontal pass of the rows [r0, r0 + nrows) (nrows <= RMAX) for the columns [x0, x0 + TW) into hrow [3][RMAX][TW].  A thread keeps
// ONE column of the tile (NT is a multiple of TW) and walks the staged rows: its window and its first KREG coefficients are read once
// and stay in registers (ksize <= 5 up to a horizontal ratio of 2; longer windows read the rest)
template <int XS>
__device__ __forceinline__ void stage_rows(unsigned char* hrow, const Src<XS>& src, int h, int w, int neww, const Axis& ax, int x0, int r0,
                                           int nrows) {
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
        const unsigned char* row = src.row(c, yi);
        int v;
        if (!ax.lo) {
          v = row[x * XS];
        } else {
          int s = 1 << (PREC - 1);
#pragma unroll
          for (int t = 0; t < KREG; ++t) {
            int xi = lo + t;
            xi = xi < 0 ? 0 : (xi < w ? xi : w - 1);     // (a valid table never reaches the clamp)
            if (t < n) s += (int)row[xi * XS] * kr[t];
          }
          for (int t = KREG; t < n; ++t) {
            int xi = lo + t;
            xi = xi < 0 ? 0 : (xi < w ? xi : w - 1);
            s += (int)row[xi * XS] * k[t];
          }
          v = clip8(s);
        }
        hrow[(c * RMAX + r) * TW + cx] = (unsigned char)v;
      }
    }
  }
}

// the vertical pass for output pixel (y, x), tile column cx, channels c0 .. c0 + NC - 1 -> v[NC]: from the staged rows, or (staged
// false) with the horizontal taps recomputed per vertical tap
template <int XS, int NC>
__device__ __forceinline__ void vpass(const unsigned char* hrow, bool staged, const Src<XS>& src, int c0, int h, int w, const Axis& ax,
                                      const Axis& ay, int x, int y, int cx, int r0, int* v) {
  if (!ay.lo) {
#pragma unroll
    for (int c = 0; c < NC; ++c)
      v[c] = staged ? hrow[((c0 + c) * RMAX + (y - r0)) * TW + cx] : hpass<XS>(src.row(c0 + c, y), x, w, ax);
    return;
  }
  const int lo = ay.lo[y];
  int n = ay.n[y];
  n = n < ay.ks ? n : ay.ks;
  const int* k = ay.k + (long)y * ay.ks;
  int s[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) s[c] = 1 << (PREC - 1);
  for (int t = 0; t < n; ++t) {
    const int kt = k[t];
    int yi = lo + t;
    yi = yi < 0 ? 0 : (yi < h ? yi : h - 1);
    int rr = yi - r0;                          // staged: inside [0, nrows) for a valid table
    rr = rr < 0 ? 0 : (rr < RMAX ? rr : RMAX - 1);
#pragma unroll
    for (int c = 0; c < NC; ++c)
      s[c] += kt * (staged ? (int)hrow[((c0 + c) * RMAX + rr) * TW + cx] : hpass<XS>(src.row(c0 + c, yi), x, w, ax));
  }
#pragma unroll
  for (int c = 0; c < NC; ++c) v[c] = clip8(s[c]);
}

}  // namespace resample
