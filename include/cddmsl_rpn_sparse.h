/*
 * cddmsl_rpn_sparse.h -- C-ABI of libcddmsl_rpn_sparse.so, the bookkeeping kernels of the RPN head's sparse backward pass (gfx950).
 * A library of its own next to libcddmsl_hip.so, with the conventions of cddmsl_hip.h: device pointers + sizes + the HIP stream
 * (void*), 0 on success (1 = bad argument, 2 = launch failure), never synchronises, owns no memory, no global state.
 * dtype 0 = bf16, 1 = f32.  This header is the source of the library's ctypes signatures (cddmsl_amd/_lib.py).
 * Why a second library: tests/test_cabi_host.py pins cddmsl_hip.h to exactly 104 declarations and libcddmsl_hip.so to exactly those
 * exports, so the main pair could not take these five.  Not a pattern to copy: fold them into cddmsl_hip.h when that count is next updated.
 */
#ifndef CDDMSL_RPN_SPARSE_H
#define CDDMSL_RPN_SPARSE_H

#ifdef __cplusplus
extern "C" {
#endif

/* Sparse backward pass of the RPN head (3x3 "same" conv + ReLU -> fused 1x1 heads): the sampled loss (rpn.py:365-429) leaves the
 * heads' output gradient non-zero on a few rows, and the convolution's two gradient GEMMs then run over those rows only, through
 * cddmsl_conv_fwd / cddmsl_conv_wgrad / cddmsl_gemm_nt_batched.  These five are the bookkeeping around them; none uses atomics.
 * rpn_mark_rows:    marks[r] (int) = 1 where row r of dy [rows][cols] holds anything but +-0 (a NaN marks its row), else 0.  dy is f32
 *                   (src_f32) or `dtype`; a row is whole 16-byte chunks.
 * rpn_compact_rows: rows_out[cap] = the marked positions in ascending order, -1 in the unused tail; slot[positions] = a position's
 *                   index in rows_out, -1 if unmarked or past cap.  More than cap marks: overflow[0] = 1 (never cleared here) and the
 *                   surplus rows are dropped -- the caller must read the flag and refuse the result.  One block; positions <= 2^30.
 * rpn_gather_rows:  dst [cap][cols] (`dtype`) = src[rows[s]] (f32 with src_f32, else `dtype`), zeros where rows[s] < 0.
 * rpn_im2col_rows:  out [cap][KH*KW][Cin] = x[n][h + kh - pad][w + kw - pad] of position rows[s] = (n*H + h)*W + w, zeros where the
 *                   tap leaves the image or rows[s] < 0; x NHWC [Nimg][H][W][Cin], 2 pad == KH - 1 == KW - 1.
 * rpn_dx_gather:    dx [Nimg][H][W][Cin] (`dtype`) = sum over taps (kh, kw), in that order, of P[kh*KW + kw][slot[q]], q = the
 *                   position at (h + kh - pad, w + kw - pad) of the same image, skipped where q leaves the image or slot[q] < 0;
 *                   P [KH*KW][cap][Cin] f32.  One f32 sum per element in a fixed order, rounded once: the same bits every call.
 * Rows of cols / Cin elements are whole 16-byte chunks and every pointer is 16-byte aligned; anything else is CDDMSL_ERR_ARG. */
int cddmsl_rpn_mark_rows(const void* dy, int* marks, long rows, int cols, int src_f32, int dtype, void* stream);
int cddmsl_rpn_compact_rows(const int* marks, int* rows_out, int* slot, int* overflow, long positions, int cap, void* stream);
int cddmsl_rpn_gather_rows(const void* src, const int* rows, void* dst, int cap, int cols, int src_f32, int dtype, void* stream);
int cddmsl_rpn_im2col_rows(const void* x, const int* rows, void* out, int cap, int Nimg, int H, int W, int Cin, int KH, int KW, int pad,
                           int dtype, void* stream);
int cddmsl_rpn_dx_gather(const float* P, const int* slot, void* dx, int cap, int Nimg, int H, int W, int Cin, int KH, int KW, int pad,
                         int dtype, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CDDMSL_RPN_SPARSE_H */
