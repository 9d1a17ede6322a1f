/*
 * cddmsl_proposal_recall.h -- C-ABI of libcddmsl_proposal_recall.so, the greedy cover walk of the proposal-recall evaluation (gfx950).
 * A library of its own next to libcddmsl_hip.so, with the conventions of cddmsl_hip.h: device pointers + sizes + the HIP stream
 * (void*), 0 on success (1 = bad argument, 2 = launch failure), never synchronises, owns no memory, no global state.
 * This header is the source of the library's ctypes signatures (cddmsl_amd/_lib.py).
 * Why a second library: tests/test_cabi_host.py pins cddmsl_hip.h to exactly 109 declarations and libcddmsl_hip.so to exactly those
 * exports, and existing tests stay as they are, so the main pair could not take this entry point.  Not a pattern to copy: fold it
 * into cddmsl_hip.h (next to cddmsl_coco_match, whose family it belongs to) when that count is next updated.
 */
#ifndef CDDMSL_PROPOSAL_RECALL_H
#define CDDMSL_PROPOSAL_RECALL_H

#ifdef __cplusplus
extern "C" {
#endif

/* The per-image body of _evaluate_box_proposals (evaluation/coco_evaluation.py:
 * 517-571: sort by objectness, cut at the limit, then min(P', G') times take the best-covered unused ground-truth box and retire it
 * with its proposal) for every (image, limit, area range) of a batch in ONE launch, bit-identical to the package's host walk
 * (cddmsl_amd/evaluation.py proposal_cover_host).
 *   proposals    boxes [P_total][4] f32 XYXY (16-byte aligned), logits [P_total] f32, concatenated over the batch's B images with
 *                offsets off [B + 1] int64, in any order inside an image; img_idx [B] int64 = each image's index into
 *   ground truth gt_boxes [G_total][4] f32 XYXY (16-byte aligned), gt_rng [G_total] u8: bit a set = the box counts in area range a
 *                (decided on the host from the stored area; a crowd box has no bit), concatenated over the data set's n_images images
 *                with offsets gt_off [n_images + 1] int64
 *   limits [L] int32, L <= 4: proposals kept per image (a "no limit" run passes a value >= 2048); A <= 8 area ranges
 *   cover_off [B + 1] int64: where each batch image's ground-truth slots start in the output; Gb = the slots of one (limit, range)
 *                plane, the sum of the batch images' ground-truth counts (only cover_off[b] is read: the slot count is the image's)
 * -> cover [L][A][Gb] f32, per ground-truth box: -1 = not counted (bit a clear, or the image has NO proposals at all: the reference
 *    skips such an image before it adds to num_pos, and that is kept); otherwise the IoU at which the walk covered the box, 0.0
 *    when the walk ended before reaching it (fewer kept proposals than boxes);
 *    over [B] int32: 1 when the image has more than 2048 proposals or more than 512 ground-truth boxes, or its offsets are
 *    inconsistent -- none of its cover slots is written then and the caller walks the image on the host; else 0.
 * The walk: rank = the stable descending-logit order (equal logits by input index, NaN last); the first min(P, limit) ranks are kept;
 * a pick is the maximum IoU over all unused (proposal, box) pairs, among equal maxima the lowest box index and then the lowest rank
 * (overlaps.max(dim=0) followed by .max(dim=0), torch returning the first maximal index); the IoU is recorded on that box.
 * Arithmetic: f32, one IEEE operation per operation of pairwise_iou (structures/boxes.py:322-367) in its order, true division,
 * contraction off: area = (x1 - x0) * (y1 - y0), wh = max(min(hi) - max(lo), 0), inter = w * h, iou = inter > 0 ? inter / ((area_p +
 * area_g) - inter) : 0.  Inputs are finite by contract.  No atomics, every output slot has one writer: two runs give the same
 * bytes.  No allocation, no synchronisation, no global state.
 * CDDMSL_ERR_ARG, nothing written: a negative count, L outside 1..4, A outside 1..8, B * L * A >= 2^31, a missing or misaligned
 * pointer.  B == 0 writes nothing. */
int cddmsl_proposal_cover(const float* boxes, const float* logits, const long* off, const long* img_idx, int B, long P_total,
                          const float* gt_boxes, const unsigned char* gt_rng, const long* gt_off, long n_images, long G_total,
                          const int* limits, int L, int A, const long* cover_off, long Gb, float* cover, int* over, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CDDMSL_PROPOSAL_RECALL_H */
