/*
 * cddmsl_weight_average.h -- C-ABI of libcddmsl_weight_average.so, the weight averaging that follows the optimizer step under
 * MODEL_EMA (EMA / SWA; gfx950).  A library of its own next to libcddmsl_hip.so, with the conventions of cddmsl_hip.h: device
 * pointers + sizes + the HIP stream (void*), 0 on success (1 = bad argument, 2 = launch failure), never synchronises, owns no
 * memory, no global state.  This header is the source of the library's ctypes signatures (cddmsl_amd/_lib.py).
 * Why a second library: tests/test_cabi_host.py pins cddmsl_hip.h to exactly 110 declarations and libcddmsl_hip.so to exactly those
 * exports, and a feature leaves existing tests as they are, so the main pair could not take this entry point.  Not a pattern to copy:
 * fold it into cddmsl_hip.h (next to cddmsl_sgd_step_groups, whose family it belongs to) when that count is next updated.
 */
#ifndef CDDMSL_WEIGHT_AVERAGE_H
#define CDDMSL_WEIGHT_AVERAGE_H

#ifdef __cplusplus
extern "C" {
#endif

/* Weight averaging over `count` f32 tensors; avg / params are HOST arrays of `count` device pointers and sizes the element counts, as
 * in cddmsl_sgd_step_groups.  Per element, in f32:
 *   copy != 0: avg = params, bit for bit; w is ignored.
 *   copy == 0: avg += w (params - avg) -- one subtraction, then a multiply-add onto avg: torch.lerp's expression for w < 0.5, what
 *              torch.optim.swa_utils computes (EMA: w = 1 - decay; running mean of n + 1 snapshots: w = 1 / (n + 1)).
 * params is never written.  A NaN or Inf element of params makes that element of avg NaN or Inf and no other; w == 0 leaves a
 * finite avg equal as a value.  CDDMSL_ERR_ARG (1) for count < 0, a negative size (or one above 2^42 elements), or (copy == 0) w
 * NaN or outside [0, 1], all checked before any HIP call; count == 0 or all sizes 0 launches nothing and returns success. */
int cddmsl_weight_average(float** avg, const float** params, const long* sizes, int count, float w, int copy, void* stream);

#ifdef __cplusplus
}
#endif

#endif
