/*
 * cddmsl_color_jitter.h -- C-ABI of libcddmsl_color_jitter.so, the photometric augmentation of the training loader under
 * INPUT.COLOR_JITTER with DATALOADER.DEVICE_RESIZE (brightness, contrast, saturation, lighting; gfx950).  A library of its own next to
 * libcddmsl_hip.so, with the conventions of cddmsl_hip.h: device pointers + sizes + the HIP stream (void*), 0 on success (1 = bad
 * argument, 2 = launch failure), never synchronises, owns no memory, no global state.  This header is the source of the library's
 * ctypes signatures (cddmsl_amd/_lib.py).
 * Why a library of its own: the route of cddmsl_weight_average.h -- tests/test_cabi_host.py pins cddmsl_hip.h to exactly 110
 * declarations and libcddmsl_hip.so to exactly those exports, and a feature leaves existing tests as they are.  It belongs next to
 * cddmsl_resize_batch_u8; fold it in when that count is next updated.
 */
#ifndef CDDMSL_COLOR_JITTER_H
#define CDDMSL_COLOR_JITTER_H

#ifdef __cplusplus
extern "C" {
#endif

/* One planar uint8 image [3][h][w] at byte `off` of the buffer and what to do with it.  `ops` is a bit set, applied in this fixed
 * order, each operation on the uint8 result of the one before: 1 brightness, 2 contrast, 4 saturation, 8 lighting.  A weight is the
 * BIT PATTERN of a float32: *_dw = fl32(w), *_sw = fl32(1 - w) with 1 - w formed in double.  light_r/g/b are the float32 bits of the
 * lighting offsets in RGB order.  bgr != 0: plane 0 is blue and plane 2 red (saturation's grey value and the lighting offsets follow
 * it).  Members of an operation whose bit is clear are ignored.  64 bytes, no implicit padding. */
typedef struct cddmsl_jitter_item {
  long off;
  int h, w, ops, bgr;
  int b_dw, b_sw, c_dw, c_sw, s_dw, s_sw;
  int light_r, light_g, light_b;
  int reserved;
} cddmsl_jitter_item;

/* In place, per item and per byte x of a plane, every product and sum rounded to float32 on its own (no fused multiply-add):
 *   out = trunc(min(max(fl32(fl32(sw * src) + fl32(dw * fl32(x))), 0), 255))
 *   brightness: src = 0.   contrast: src = fl32(S / (3 h w)), S the exact integer sum of the item's 3 h w bytes as they stand after the
 *   brightness step, the division in double.   saturation: src = fl32(fl32(fl32(0.299f R) + fl32(0.587f G)) + fl32(0.114f B)) of the
 *   pixel.   lighting: sw = dw = 1, src = the plane's offset.
 * Two launches on `stream`: the sums of the items with contrast (64-bit integer atomics into sums[i], zeroed first; exact, so a call
 * repeats bit for bit), then the apply pass.  `sums`: device array of `count` 64-bit integers, may be NULL when no item has contrast;
 * on return (in stream order) sums[i] holds S of item i with contrast and 0 of the others.  Bytes outside the items' planes are neither
 * read nor written; items must not overlap.  An item with ops == 0 is left alone; a batch of such items (or count == 0) launches
 * nothing.  CDDMSL_ERR_ARG (1) before any HIP call for: count < 0, a NULL buffer, h or w <= 0, ops outside 0..15, an item that does not
 * lie inside [0, buf_bytes), a non-finite weight or offset of an active operation, contrast without `sums`. */
int cddmsl_color_jitter_batch_u8(unsigned char* buf, long buf_bytes, const cddmsl_jitter_item* items, int count, long* sums, void* stream);

#ifdef __cplusplus
}
#endif

#endif
