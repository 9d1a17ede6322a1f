// The loader's ResizeShortestEdge + RandomFlip (data/dataset_mapper.py:126-217, transforms/transform.py ResizeTransform / HFlipTransform)
// for a whole batch in ONE launch: 2N differently sized uint8 images, interleaved [h][w][3] as PIL decodes them -> Pillow's bilinear
// resize to (newh, neww), bit for bit (resample.h) -> planar [3][newh][neww] uint8, mirrored left-right and / or with the channel
// order reversed (INPUT.FORMAT BGR) per item.  The host only decodes; what the model receives is byte-identical to the host path.
// flip is a bit set: bit 0 mirrors the columns (RandomFlip horizontal), bit 1 the rows of each plane (vertical), 3 does both.
//
// Work decomposition: one flat grid over the TH x TW output tiles of all items (per-item tile prefix in the by-value descriptor
// block; a workgroup finds its item with a short uniform scan).  A workgroup stages the horizontally resampled rows of its tile in LDS
// and runs the vertical pass from there (resample.h), a tile whose rows do not fit recomputes.  Output: a row of a plane starts at an
// arbitrary byte (neww is arbitrary), so a lane makes one ADDRESS-aligned group of 4 bytes of one plane row: a group that lies
// inside the tile's span is one 4-byte store, the (at most two) groups at the span's ends are byte stores.  With flip the span is
// the mirrored column range and a group's bytes read the tile's columns backwards; with the row mirror output row y is written to
// row newh - 1 - y, and since the aligned-group / byte-edge split is taken from the row's destination ADDRESS, only the row index
// changes.  Plain vector stores only.
#include "resample.h"

namespace {

using namespace resample;

constexpr int RS_MAX = 32;                     // items per launch (16 pairs): 56-byte descriptors + the tile prefix stay below 2 KiB of kernarg
constexpr int NG = TW / 4 + 1;                 // aligned 4-byte groups a misaligned span of TW bytes touches
static_assert(3 * NG <= 64, "a wave holds one row of the three planes");

struct RsBatch { cddmsl_resize_item it[RS_MAX]; int tile0[RS_MAX + 1]; int count; };

__device__ __forceinline__ Axis axis_at(const int* tab, int off, int out, int ks) {
  if (off < 0) return Axis{nullptr, nullptr, nullptr, 0};
  const int* t = tab + off;                    // [lo [out] | n [out] | k [out][ks]]
  return Axis{t, t + out, t + 2 * (long)out, ks};
}

__global__ void __launch_bounds__(NT) k_resize_batch_u8(RsBatch b, const unsigned char* __restrict__ src, unsigned char* __restrict__ dst,
                                                        const int* __restrict__ tab) {
  __shared__ unsigned char hrow[HROW_BYTES];
  const int bid = blockIdx.x;
  int j = 0;
  while (j + 1 < b.count && bid >= b.tile0[j + 1]) ++j;      // block-uniform
  const cddmsl_resize_item& t = b.it[j];
  const int h = t.h, w = t.w, newh = t.newh, neww = t.neww;
  const int tl = bid - b.tile0[j], tx = (neww + TW - 1) / TW;
  const int x0 = (tl % tx) * TW, y0 = (tl / tx) * TH;
  if (y0 >= newh) return;                                     // (never: the grid is the tile prefix's total)
  const Axis ax = axis_at(tab, t.xtab, neww, t.xks), ay = axis_at(tab, t.ytab, newh, t.yks);
  // plane c of the output takes source channel c, or 2 - c with reverse_channels: the channel stride runs backwards from byte 2
  const Src<3> s{src + t.src_off + (t.reverse_channels ? 2 : 0), t.reverse_channels ? -1L : 1L, 3L * w};
  int r0, nrows;
  tile_rows(ay, y0, newh, r0, nrows);
  const bool staged = nrows <= RMAX;                          // block-uniform
  if (staged) stage_rows<3>(hrow, s, h, w, neww, ax, x0, r0, nrows);
  __syncthreads();
  const int len = (x0 + TW < neww ? x0 + TW : neww) - x0;    // the tile's columns [x0, x0 + len) land on [xd0, xd0 + len) of the output row
  const bool fx = t.flip & 1, fy = t.flip & 2;               // block-uniform
  const int xd0 = fx ? neww - x0 - len : x0;
  const int ny = y0 + TH < newh ? TH : newh - y0;
  unsigned char* out = dst + t.dst_off;
  // a wave makes one output row at a time, all three planes: lane = plane * NG + group (51 of 64 lanes), so the row's window and
  // coefficients are the same addresses across the wave and are read once per group, not once per pixel
  const int c = (threadIdx.x & 63) / NG, g = (threadIdx.x & 63) % NG;
  if (c >= 3) return;
  // output row y0 + ry of the tile lands on row y0 + ry of its plane, or with the row mirror on newh - 1 - (y0 + ry): the tile's rows
  // walked backwards from newh - 1 - y0 (ry < ny keeps y0 + ry < newh, so the destination row stays inside [0, newh))
  const long rstep = fy ? -(long)neww : (long)neww;
  unsigned char* span0 = out + ((long)c * newh + (fy ? newh - 1 - y0 : y0)) * neww + xd0;
  for (int ry = threadIdx.x >> 6; ry < ny; ry += NT / 64) {
    const int y = y0 + ry;
    unsigned char* span = span0 + ry * rstep;
    const int j0 = g * 4 - (int)((size_t)span & 3);           // span index of the group's first byte: -3 .. len + 2
    if (j0 >= len) continue;
    int v[4] = {0, 0, 0, 0};
    if (staged && ay.lo) {
      // vpass for the group's four pixels at once (the same sums in the same order); a byte outside the span computes a
      // neighbour's column and is not stored
      int cxq[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        int jj = j0 + q;
        jj = jj < 0 ? 0 : (jj < len ? jj : len - 1);
        cxq[q] = fx ? len - 1 - jj : jj;
      }
      const int lo = ay.lo[y];
      int n = ay.n[y];
      n = n < ay.ks ? n : ay.ks;
      const int* k = ay.k + (long)y * ay.ks;
      int s4[4] = {1 << (PREC - 1), 1 << (PREC - 1), 1 << (PREC - 1), 1 << (PREC - 1)};
      for (int tp = 0; tp < n; ++tp) {
        const int kt = k[tp];
        int yi = lo + tp;
        yi = yi < 0 ? 0 : (yi < h ? yi : h - 1);
        int rr = yi - r0;                                     // inside [0, nrows) for a valid table
        rr = rr < 0 ? 0 : (rr < RMAX ? rr : RMAX - 1);
        const unsigned char* hr = hrow + (c * RMAX + rr) * TW;
#pragma unroll
        for (int q = 0; q < 4; ++q) s4[q] += kt * (int)hr[cxq[q]];
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) v[q] = clip8(s4[q]);
    } else {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int jj = j0 + q;
        if (jj >= 0 && jj < len) {
          const int cx = fx ? len - 1 - jj : jj;
          vpass<3, 1>(hrow, staged, s, c, h, w, ax, ay, x0 + cx, y, cx, r0, &v[q]);
        }
      }
    }
    if (j0 >= 0 && j0 + 4 <= len) {
      *(unsigned*)(span + j0) = (unsigned)v[0] | ((unsigned)v[1] << 8) | ((unsigned)v[2] << 16) | ((unsigned)v[3] << 24);
    } else {
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if (j0 + q >= 0 && j0 + q < len) span[j0 + q] = (unsigned char)v[q];
    }
  }
}

// offsets + extents inside the buffers, positive sizes, a flip code of 0..3, a table exactly for a changed axis and inside the table buffer
bool item_ok(const cddmsl_resize_item& t, long src_bytes, long dst_bytes, long tab_len) {
  if (t.h <= 0 || t.w <= 0 || t.newh <= 0 || t.neww <= 0) return false;
  if (t.flip < 0 || t.flip > 3) return false;
  const long sb = 3L * t.h * t.w, db = 3L * t.newh * t.neww;
  if (t.src_off < 0 || t.src_off > src_bytes || sb > src_bytes - t.src_off) return false;
  if (t.dst_off < 0 || t.dst_off > dst_bytes || db > dst_bytes - t.dst_off) return false;
  const int out[2] = {t.neww, t.newh}, in[2] = {t.w, t.h}, off[2] = {t.xtab, t.ytab}, ks[2] = {t.xks, t.yks};
  for (int a = 0; a < 2; ++a) {
    if (out[a] == in[a]) {
      if (off[a] >= 0) return false;
    } else {
      if (off[a] < 0 || ks[a] <= 0) return false;
      if ((long)out[a] * (2L + ks[a]) > tab_len - off[a]) return false;
    }
  }
  return true;
}

}  // namespace

extern "C" int cddmsl_resize_batch_u8(const unsigned char* src, long src_bytes, unsigned char* dst, long dst_bytes, const int* tab,
                                      long tab_len, const cddmsl_resize_item* items, int count, void* stream) {
  if (count < 0 || src_bytes < 0 || dst_bytes < 0 || tab_len < 0) return CDDMSL_ERR_ARG;
  if (count == 0) return CDDMSL_OK;
  if (!src || !dst || !items) return CDDMSL_ERR_ARG;
  long tiles = 0;
  for (int i = 0; i < count; ++i) {                           // every item of every chunk BEFORE the first launch
    const cddmsl_resize_item& t = items[i];
    if (!item_ok(t, src_bytes, dst_bytes, tab_len)) return CDDMSL_ERR_ARG;
    if ((t.xtab >= 0 || t.ytab >= 0) && !tab) return CDDMSL_ERR_ARG;
    if (i % RS_MAX == 0) tiles = 0;
    tiles += (long)((t.neww + TW - 1) / TW) * ((t.newh + TH - 1) / TH);
    if (tiles > 0x7fffffffL) return CDDMSL_ERR_ARG;           // a chunk's flat grid
  }
  for (int base = 0; base < count; base += RS_MAX) {
    RsBatch b{};
    b.count = count - base < RS_MAX ? count - base : RS_MAX;
    int n = 0;
    for (int i = 0; i < b.count; ++i) {
      b.it[i] = items[base + i];
      b.tile0[i] = n;
      n += ((b.it[i].neww + TW - 1) / TW) * ((b.it[i].newh + TH - 1) / TH);
    }
    for (int i = b.count; i <= RS_MAX; ++i) b.tile0[i] = n;
    k_resize_batch_u8<<<dim3((unsigned)n), dim3(NT), 0, (hipStream_t)stream>>>(b, src, dst, tab);
  }
  return launch_status();
}
