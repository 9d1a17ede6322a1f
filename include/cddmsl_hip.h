/*
 * cddmsl_hip.h -- C-ABI of libcddmsl_hip.so, the MI355X (gfx950) kernels of the CDDMSL training hot path.
 *
 * Boundary: the reference reaches its native ops through torch.autograd.Function wrappers over
 * `_C.<op>_forward/_backward(Tensor..., scalars...)` (detectron2/layers/roi_align_rotated.py:11-47; the pybind
 * file csrc/vision.cpp is absent from the tree) and through torchvision/ATen for the hot path.  This header is
 * the plain-C equivalent: device pointers + sizes + the HIP stream to enqueue on, no torch types.  Every function
 * returns 0 on success (1 = bad argument, 2 = launch failure), never synchronises, owns no memory (the caller
 * allocates outputs and workspaces) and keeps no global mutable state (one thread-local diagnostic id excepted, see
 * cddmsl_last_kernel), so calls are re-entrant and stream-ordered.
 *
 * Conventions
 *   dtype      0 = bf16 (throughput path), 1 = f32 (exact-f32 MFMA parity path)
 *   activations NHWC [N][H][W][C] in `dtype`; C * sizeof(dtype) must be a multiple of 16 bytes
 *   weights    [Cout][KH][KW][Cin] (= torch channels_last OIHW); f32 masters, `dtype` prepared copies
 *   rois       [K][5] f32 (batch_idx, x0, y0, x1, y1), grouped by image
 *   stream     hipStream_t passed as void*
 * Paths below are relative to /root/reference/detectron2/.
 */
#ifndef CDDMSL_HIP_H
#define CDDMSL_HIP_H
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

int cddmsl_abi_version(void);

/* ---- implicit-GEMM convolution / linear (bf16 or exact-f32 MFMA) ----------------------------------------------
 * replaces ATen conv2d / F.linear + FrozenBatchNorm2d + ReLU (+ residual add, + AvgPool2d) as called from
 * modeling/backbone/clip_backbone.py:57-70,193-219, layers/batch_norm.py:45-66,
 * modeling/proposal_generator/rpn.py:158-177, modeling/backbone/clipcap/clipcap.py:39-163.
 * y[m][n] = relu?( acc*scale[n] + bias[n] + residual[m][n] ), zeroed where relu_mask[m][n] <= 0 (ReLU backward);
 * pool=1: 1x1 conv over the 2x2 average-pooled input.  dgrad = the same entry point on weight_prep's w_dgrad.
 * out_f32: bit 0 = y is f32; bit 1 (bf16 kernels, with bit 0, no relu_mask, leading dims multiples of 8) = the residual rows are
 * f32 -- the mapper's residual stream x + f(LN(x)) stays f32 (clipcap.py:88-100) and its add rides in the GEMM epilogue;
 * bit 2 (leading dims multiples of 8, pooled tensor < 2 GiB) = `residual` is [Nimg][Ho/2][Wo/2][ldr] and row m adds a quarter
 * of its pooled pixel: the backward of the Bottleneck's AvgPool2d(stride) on the downsample path (clip_backbone.py:45-52). */
int cddmsl_conv_fwd(const void* x, const void* w, void* y, const float* scale, const float* bias, const void* residual,
                    const void* relu_mask, int Nimg, int Hi, int Wi, int Cin, int Cout, int KH, int KW, int stride, int pad,
                    int pool, int ldy, int ldr, int ldm, int relu, int out_f32, int dtype, void* stream);
/* The CLIP stem's third convolution and the AvgPool2d(2) behind it (clip_backbone.py:139-147) as ONE launch:
 *   y [Nimg][Hi/2][Wi/2][64] = avgpool2(relu(conv3x3(x, pad 1) * scale + bias)), bit-identical to cddmsl_conv_fwd + cddmsl_avgpool2_fwd;
 * the full-resolution map is never written.  bf16 (dtype 0), Cin 32, Cout 64, stride 1, scale and bias given, relu_mask NULL:
 * anything else is CDDMSL_ERR_ARG.  Plan-only mode reports kernel 8. */
int cddmsl_conv3x3_pool_fwd(const void* x, const void* w, void* y, const float* scale, const float* bias, const void* relu_mask,
                            int Nimg, int Hi, int Wi, int Cin, int Cout, int stride, int dtype, void* stream);
/* One frozen 64-plane CLIP Bottleneck behind its conv1 as ONE launch (clip_backbone.py:57-70 at stride 1; bf16, forward only):
 *   o2  = relu(o1 (*) w2 * s2 + b2)                   3x3 pad 1, 64 -> 64, never written to memory
 *   out = relu(o2 . w3 * s3 + b3 + residual)          [Nimg][H][W][256]
 *   o1n = relu(out . w1n * s1n + b1n)                 [Nimg][H][W][64]: conv1 of the NEXT block, when w1n is given
 * The residual is either read (`residual`, [Nimg][H][W][256]) or, when wd is given, computed as x0 . wd * sd + bd from the
 * block's 64-channel input x0 (the downsample convolution, rounded to bf16 as its own launch would store it): exactly one of
 * the two.  Weights as cddmsl_conv_fwd takes them ([Cout][KH][KW][Cin] bf16), scale / bias f32 per output channel, required.
 * Results are bit-identical to the separate cddmsl_conv_fwd launches.  cddmsl_bottleneck64_ok: 1 when the shape / dtype is taken
 * (dtype 0, every tensor below 2 GiB); anything else is CDDMSL_ERR_ARG -- the caller keeps the separate launches. */
int cddmsl_bottleneck64_ok(int Nimg, int H, int W, int dtype);
int cddmsl_bottleneck64_fwd(const void* o1, const void* w2, const float* s2, const float* b2, const void* w3, const float* s3,
                            const float* b3, const void* residual, const void* x0, const void* wd, const float* sd,
                            const float* bd, const void* w1n, const float* s1n, const float* b1n, void* out, void* o1n,
                            int Nimg, int H, int W, int dtype, void* stream);
/* Device scratch for the weight-gradient kernels' split reductions (no counterpart in the reference: ATen's conv backward owns its
 * workspace, aten/src/ATen/native/cudnn).  With `bytes` of 16-byte-aligned device memory registered, a split reduction stores its
 * partial tiles there and a second kernel sums them into dW (deterministic; f32 atomics otherwise, and whenever the launch needs more
 * than `bytes`).  One workspace per process; launches that use it must be stream-ordered.  (nullptr, 0) unregisters. */
int cddmsl_set_workspace(void* ptr, long bytes);
/* dW[n][k] (f32, accumulated) += scale[n] * sum_m dY[m][n] * im2col(x)[m][k] */
int cddmsl_conv_wgrad(const void* x, const void* dy, float* dw, const float* scale, int Nimg, int Hi, int Wi, int Cin,
                      int Cout, int KH, int KW, int stride, int pad, int pool, int ldd, int dtype, void* stream);
/* batched GEMMs on the same kernels (strides in elements; used by the reassociated attention pool):
 *   nt: C_b[m][n] = sum_k A_b[m][k] B_b[n][k] (+ bias[n]);   tn: out_b[n][k] (+)= sum_m A_b[m][n] B_b[m][k]
 *   tn mode 0 = f32 atomic accumulate, 1 = f32 store, 2 = `dtype` store */
int cddmsl_gemm_nt_batched(const void* a, const void* w, void* c, const float* bias, int M, int N, int K, int lda, int ldb, int ldc,
                           int batch, long sa, long sw, long sc, int out_f32, int dtype, void* stream);
int cddmsl_gemm_tn_batched(const void* a, const void* b, void* out, int M, int N, int K, int lda, int ldb, int ldo, int batch, long sa,
                           long sb, long so, int mode, int dtype, void* stream);
/* diagnostic: the kernel the calling thread's last conv / GEMM entry point launched -- 1 k_conv_fwd (128x128 LDS-DMA),
 * 2 k_conv_fwd_reg (fused avg-pool loader), 3 k_conv_fwd256 (256x256 ping-pong), 4 k_conv_wgrad, 5 k_conv_wgrad_dma,
 * 6 k_wgrad256, 7 k_gemm_tn_stream, 8 k_conv3x3_small (few-channel 3x3 layers: the CLIP stem), 9 k_gemm_tn_small, 13 k_bottleneck64 (cddmsl_bottleneck64_fwd).  bench.py uses it to attribute HIP-event times to kernels. */
int cddmsl_last_kernel(void);
/* diagnostic: while on (per thread), the conv / GEMM entry points above choose their kernel (cddmsl_last_kernel) and return
 * without launching; bench.py asks this way BEFORE a launch whether it is the kernel whose launches it is timing, so only those
 * launches carry HIP events inside the timed region.  Returns the previous setting. */
int cddmsl_plan_only(int on);
/* f32 master -> `dtype` forward weights and flipped/transposed dgrad weights scaled by the FrozenBN scale */
int cddmsl_weight_prep(const float* w, const float* scale, void* w_fwd, void* w_dgrad, int Cout, int KH, int KW, int Cin,
                       int dtype, void* stream);
/* the same for `count` weights in one launch; device table of 8 x int64 per weight: {w, scale, w_fwd, w_dgrad (pointers, 0 = skip),
 * Cout, KH, KW, Cin}.  Used once per step after the optimizer update. */
int cddmsl_weight_prep_multi(const long long* table, int count, int dtype, void* stream);

/* ---- OCP e4m3 (fp8) configuration: BASELINE.json configs[4] ------------------------------------------------------------------
 * The reference has no fp8 path (AMP is off, config/defaults.py:697): these entry points have no counterpart there; they replace,
 * for the MFMA-bound forward convolutions of layer3 / layer4 / the RoI head's layer4 (clip_backbone.py:57-70) and for the region x
 * text-embedding contraction (roi_heads/fast_rcnn.py:546-572), the bf16 launches of cddmsl_conv_fwd / cddmsl_cosine_logits_fwd.
 *   cddmsl_quantize_fp8   x (src_dtype 0 bf16 / 1 f32, numel % 8 == 0) -> y e4m3 bytes = sat(x * scale[0]); scale (device, nullable = 1)
 *                         and amax (device, nullable): max|x| is recorded with an atomic max (delayed scaling, no host round trip)
 *   cddmsl_conv_fwd_fp8   e4m3 x [Nimg][Hi][Wi][Cin] * e4m3 w [Cout][KH][KW][Cin], stride 1 -> bf16 (f32 with out_f32) y with the
 *                         epilogue of cddmsl_conv_fwd (scale / bias f32 per channel -- the caller folds both dequantisation
 *                         factors into scale --, bf16 residual, ReLU, bf16 ReLU mask); v_mfma_scale_f32_32x32x64_f8f6f4, f32 accumulate.
 *                         Cin % 128 == 0, Cout % 256 == 0, <= 31 taps: other shapes are CDDMSL_ERR_ARG
 *   cddmsl_fp8_dot_nt     c [R][ldc] f32 (columns < N) = alpha[0] * a [R][K] . b [N][K]^T, N <= 32, K % 64 == 0
 *   y8 / q8 / amax8 (nullable together; cddmsl_conv_fwd_fp8 and cddmsl_conv_fwd_q8): a second output y8 [M][Cout] = e4m3 of
 *                         sat(y * q8[0]) for the NEXT convolution, written by the same epilogue (no separate quantisation pass);
 *                         max|y| goes to amax8.  Every amax buffer is 64 floats (atomics are spread by block; the owner takes the max).
 *   cddmsl_conv_fwd_q8    = cddmsl_conv_fwd for bf16 with that second output; only launches the 256x256 kernel takes
 *   cddmsl_conv_wgrad_fp8 dW[n][k] (f32, accumulated) += scale[n] * sum_m dy8[m][n] * im2col(x8)[m][k] on the e4m3 copies of both
 *                         operands (x8 [Nimg][Hi][Wi][Cin], dy8 rows ldd bytes apart); "same" convolutions (stride 1, 2 pad = KH - 1),
 *                         Cin % 256 == 0, Cout % 256 == 0 (cddmsl_conv_wgrad_fp8_ok returns 1), else CDDMSL_ERR_ARG; the caller folds
 *                         both dequantisation factors into scale.  Replaces, for the fp8 configuration, the weight-gradient half of
 *                         torch's conv2d backward behind modeling/backbone/clip_backbone.py:57-70 */
int cddmsl_quantize_fp8(const void* x, void* y, const float* scale, float* amax, long numel, int src_dtype, void* stream);
int cddmsl_conv_fwd_fp8(const void* x, const void* w, void* y, const float* scale, const float* bias, const void* residual,
                        const void* relu_mask, int Nimg, int Hi, int Wi, int Cin, int Cout, int KH, int KW, int pad, int relu,
                        int out_f32, void* y8, const float* q8, float* amax8, void* stream);
int cddmsl_conv_fwd_q8(const void* x, const void* w, void* y, const float* scale, const float* bias, const void* residual,
                       const void* relu_mask, int Nimg, int Hi, int Wi, int Cin, int Cout, int KH, int KW, int stride, int pad,
                       int relu, void* y8, const float* q8, float* amax8, void* stream);
int cddmsl_fp8_dot_nt(const void* a, const void* b, float* c, const float* alpha, int R, int N, int K, int ldc, void* stream);
int cddmsl_conv_wgrad_fp8_ok(int Cin, int Cout, int KH, int KW, int pad, int ldd);
int cddmsl_conv_wgrad_fp8(const void* x8, const void* dy8, float* dw, const float* scale, int Nimg, int Hi, int Wi, int Cin, int Cout,
                          int KH, int KW, int pad, int ldd, void* stream);

/* ---- RoIAlign  (layers/roi_align.py:49-65 -> torchvision.ops.roi_align; modeling/poolers.py:190-229) --------- */
/* y_pooled (nullable, [K][ph/2][pw/2][C], ph and pw even): AvgPool2d(2) of y, formed from the rounded outputs in the pooling
 * kernel's order -- what the first Bottleneck of the RoI head's layer4 reads on its downsample path (clip_backbone.py:45-52) */
int cddmsl_roi_align_forward(const void* x, const float* rois, void* y, void* y_pooled, int* dbg_grid, int N, int C, int H, int W,
                             int K, int ph, int pw, float spatial_scale, int sampling_ratio, int aligned, int dtype, void* stream);
int cddmsl_roi_align_backward(const void* dy, const float* rois, const int* roi_start, void* dx, float* ws_ay, float* ws_ax,
                              int* ws_fp, int N, int C, int H, int W, int K, int ph, int pw, float spatial_scale,
                              int sampling_ratio, int aligned, int dtype, void* stream);
/* The RoI head's entry (modeling/roi_heads/clip_roi_heads.py:113-115: pooler, then backbone.layer4, whose first Bottleneck
 * starts with a 1x1 conv and pools 2x2 on its downsample path, clip_backbone.py:45-52,57-70) with the 1x1 conv moved in FRONT of
 * the pooling -- RoIAlign is linear over pixels, a 1x1 conv over channels: roi_align(x) W = roi_align(x W) -- so the
 * [K][14][14][1024] crop tensor (3.3 GB at 8192 RoIs) is never formed:
 *   _affine:  y = relu?(scale[c] * roi_align(x)[.., c] + bias[c])  (FrozenBN + ReLU of that conv; scale / bias nullable),
 *             y nullable when only y_pooled (the downsample path's AvgPool2d(2) of the crops) is wanted: then
 *             y_pooled = scale[c] * avgpool2(roi_align(x))[.., c] + bias[c], the affine AFTER the average (the downsample conv
 *             moved in front of the pooling too: its FrozenBN bias cannot be pooled, bins at the border do not weigh 1), and
 *             relu != 0 returns CDDMSL_ERR_ARG (a ReLU does not commute with the average); with y given, y_pooled is
 *             avgpool2 of the stored y;
 *   _backward_pooled: dy is the gradient of the pooled map [K][ph][pw][C] (RoIAlign grid 2ph x 2pw): roi_align_backward of the
 *             AvgPool2d backward of dy, without forming it;
 *             y8 / q8 / amax8 (nullable, bf16 only): e4m3 copy of y for the consuming convolution, as cddmsl_conv_fwd_q8. */
int cddmsl_roi_align_forward_affine(const void* x, const float* rois, void* y, void* y_pooled, const float* scale,
                                    const float* bias, int relu, int N, int C, int H, int W, int K, int ph, int pw,
                                    float spatial_scale, int sampling_ratio, int aligned, int dtype, void* y8, const float* q8,
                                    float* amax8, void* stream);
int cddmsl_roi_align_backward_pooled(const void* dy, const float* rois, const int* roi_start, void* dx, float* ws_ay,
                                     float* ws_ax, int* ws_fp, int N, int C, int H, int W, int K, int ph, int pw,
                                     float spatial_scale, int sampling_ratio, int aligned, int dtype, void* stream);
/* torchvision.ops.roi_align with the signature the reference calls (layers/roi_align.py:58-65 -> roi_align(input, rois, output_size,
 * spatial_scale, sampling_ratio, aligned)): input [N][C][H][W] (NCHW, any C), rois [K][5] (batch_idx, x0, y0, x1, y1) in ANY order ->
 * output [K][C][ph][pw]; backward: grad [K][C][ph][pw] -> grad_input [N][C][H][W] (what torchvision's autograd Function hands back).
 * They re-lay the operands channels-last in caller-provided scratch (RoIs ranked stably by image for the gather backward) and run
 * the kernels above: same arithmetic.  Call with temp == NULL to get *temp_bytes.  The training path keeps the channels-last,
 * grouped-by-image entry points (poolers.py:68-95 emits RoIs in that order anyway). */
int cddmsl_roi_align_nchw_anyorder(const void* input, const float* rois, void* output, int N, int C, int H, int W, int K, int ph, int pw,
                                   float spatial_scale, int sampling_ratio, int aligned, int dtype, void* temp, size_t* temp_bytes,
                                   void* stream);
int cddmsl_roi_align_backward_nchw_anyorder(const void* grad, const float* rois, void* grad_input, int N, int C, int H, int W, int K,
                                            int ph, int pw, float spatial_scale, int sampling_ratio, int aligned, int dtype, void* temp,
                                            size_t* temp_bytes, void* stream);

/* ---- RPN / matcher index stages --------------------------------------------------------------------------------
 * modeling/anchor_generator.py:161-228, modeling/box_regression.py:77-115, modeling/proposal_generator/rpn.py:514-533,
 * modeling/proposal_generator/proposal_utils.py:22-130, layers/nms.py:19-39 (torchvision nms),
 * structures/boxes.py:322-367 + modeling/matcher.py:61-126 */
int cddmsl_anchors(const float* cell, float* out, int Hf, int Wf, int A, float stride, float offset, void* stream);
/* stable descending sort of every row of keys_in [N][total] (torch.sort(descending=True, stable=True) per image,
 * proposal_utils.py:66-70): one device-wide radix sort over (image, score) composite keys; `offsets` is unused (dense rows);
 * temp == NULL returns the workspace size in *temp_bytes.  +0.0 and -0.0 are equal scores (lower index first); a -0.0 key is
 * returned as +0.0 in keys_out, every other key bit for bit.  NaN keys have no defined order. */
int cddmsl_sort_desc(const float* keys_in, float* keys_out, int* idx_scratch, int* order_out, const int* offsets, int N,
                     int total, void* temp, size_t* temp_bytes, void* stream);
int cddmsl_rpn_decode(const int* order, const float* deltas, const float* cell, const int* img_hw, float* boxes,
                      unsigned char* valid, int N, int Hf, int Wf, int A, int topk, float stride, float offset, float wx,
                      float wy, float ww, float wh, float scale_clamp, float min_size, void* stream);
int cddmsl_nms(const float* boxes, const unsigned char* valid, unsigned long long* mask_ws, int* keep, int* nkeep, int N,
               int n, float thr, int max_keep, void* stream);
/* torchvision.ops.nms as the reference calls it (layers/nms.py:6-7,30,35): boxes [K][4] and scores [K] in ANY order ->
 * keep [K] int64 = indices of the kept boxes in descending-score order (entries past *nkeep are -1), nkeep [1] (device).
 * Scratch from the caller: call with temp == NULL to get *temp_bytes.  K <= 12288. */
int cddmsl_nms_anyorder(const float* boxes, const float* scores, long* keep, int* nkeep, int K, float iou_threshold, void* temp,
                        size_t* temp_bytes, void* stream);
/* batched_soft_nms + _soft_nms + pairwise_iou (layers/soft_nms.py:85-132,186-261, structures/boxes.py:322-367) as
 * fast_rcnn_inference_single_image calls them (modeling/roi_heads/fast_rcnn.py:186-194): boxes [K][4] f32 XYXY, scores [K] f32
 * (finite), idxs [K] int64 categories in ANY order (ids need not be contiguous).  method 0 gaussian (sigma > 0), 1 linear,
 * 2 hard; iou_threshold is the linear / hard threshold, prune_threshold the strict survival threshold.  max_keep -1: no cap;
 * >= 0: every category's walk stops after max_keep picks and the output holds at most max_keep entries -- exactly the first
 * max_keep entries of the uncapped result.
 * -> keep [K] int64 = input indices in pick order (rescored score descending, equal scores by input index; entries past *nkeep
 * are -1), keep_scores [K] f32 = the rescored scores (entries past *nkeep are not written), nkeep [1] int (device).
 * Arithmetic: coordinates are shifted by (float)cls * (max coordinate + 1) in f32 and the IoU is pairwise_iou's form on the
 * SHIFTED values, every operation one IEEE f32 operation in the reference's order: linear and hard are bit-exact, gaussian up to
 * expf's 1 ulp.  One workgroup walks one category with its state in LDS (up to 2048 candidates of a category; a larger category
 * walks in the scratch buffer, same result, slower: ONE workgroup walks it with its state in global memory, unmeasured, and a call
 * with thousands of picks in such a category can take seconds).  As in the reference's single walk, a candidate whose score starts
 * at or below prune_threshold is dropped after the first pick of all (the global arg-max) unless it is that pick or shares its
 * category, where the ordinary decay-and-prune test decides.
 * Caps: K <= 32768 per call (any split over categories).  K above that, an unknown method, sigma <= 0 with the gaussian method,
 * or max_keep < -1 return CDDMSL_ERR_ARG with nothing written.  K == 0 writes *nkeep = 0 and nothing else.
 * Scratch from the caller: call with temp == NULL to get *temp_bytes.  temp == NULL always means "size query": with K == 0 the
 * query returns 0 bytes and the run still needs a non-NULL temp (any address, never dereferenced) to write *nkeep = 0.
 * No allocation, no synchronisation, no global state. */
int cddmsl_soft_nms(const float* boxes, const float* scores, const long* idxs, long* keep, float* keep_scores, int* nkeep, int K,
                    int method, float sigma, float iou_threshold, float prune_threshold, int max_keep, void* temp,
                    size_t* temp_bytes, void* stream);
/* ---- COCO box matching (csrc/coco_match.hip): COCOeval.evaluateImg's greedy walk (pycocotools cocoeval.py, iouType "bbox", as
 * evaluation/coco_evaluation.py drives it) for every (image, class) of a batch in ONE launch, bit-identical to the package's host
 * matcher (cddmsl_amd/evaluation.py _coco_match + coco_box_iou) called per (image, class, area range).
 *   detections   dt_boxes [D_total][4] f32 XYXY (16-byte aligned), dt_scores [D_total] f32, dt_cls [D_total] int64, concatenated
 *                over the batch's B images with offsets dt_off [B + 1] int64; img_idx [B] int64 = each image's index into
 *   ground truth gt_xywh [.][4] f64, gt_area [.] f64 (the stored area: it decides "ignored" per range), gt_crowd [.] u8, gt_cls [.]
 *                int64, concatenated over the data set's n_images images with offsets gt_off [n_images + 1] int64
 *   thrs [T] f64 IoU thresholds as the walk uses them (min(t, 1 - 1e-10), from the host), area_rngs [A][2] f64 (lo, hi), K classes,
 *                max_dets kept detections per (image, class).  T * A <= 64, A <= 4, max_dets <= 128.
 * -> rank [D_total] int32: the detection's position in the stable descending-score order of its (image, class) (NaN scores last,
 *    equal scores by input index), -1 for a position >= max_dets or a class outside [0, K);
 *    matched / ignored [D_total] int64: bit a * T + t = the walk's dtm / dtIg flag at threshold t in range a (0 where rank is -1);
 *    over [B] int32: 1 when some class of the image exceeds a cap (1024 detections or 256 ground-truth boxes of one class in one
 *    image) or its offsets are inconsistent -- the image's outputs are then incomplete and the caller matches it on the host.
 * Arithmetic: f64, the host's operations in the host's order (boxes widened to f64 first; w = x2 - x1; IoU = inter / union with
 * union = da + ga - inter, or da against a crowd box); `iou < best` skips, so of equal IoUs the later box wins and a NaN IoU (0 / 0)
 * is taken.  No atomics, every output has one writer: two runs give the same bytes.  No allocation, no synchronisation. */
int cddmsl_coco_match(const float* dt_boxes, const float* dt_scores, const long* dt_cls, const long* dt_off, const long* img_idx,
                      int B, long D_total, const double* gt_xywh, const double* gt_area, const unsigned char* gt_crowd,
                      const long* gt_cls, const long* gt_off, long n_images, const double* thrs, int T, const double* area_rngs,
                      int A, int K, int max_dets, int* rank, long* matched, long* ignored, int* over, void* stream);
/* ---- Proposal recall (csrc/proposal_recall.hip): the per-image body of _evaluate_box_proposals (evaluation/coco_evaluation.py:
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
/* ---- Pascal VOC matching (csrc/voc_match.hip): the devkit's greedy walk (pascal_voc_evaluation.py voc_eval, restated by
 * cddmsl_amd/evaluation.py class_ap) for every (class, image) of a test set at T IoU thresholds in ONE launch, bit-identical to
 * class_ap called per (class, threshold) on detections that went through the reference's result-file text lines.
 *   detections   boxes [D][4] f32 XYXY as the model left them (16-byte aligned).  The kernel applies the text round trip itself:
 *                xmin = rint(double(x0 + 1.0f) * 10.0) / 10.0 (the + 1 in f32), xmax = rint(double(x1) * 10.0) / 10.0, y likewise.
 *   segments     perm [P] int64 lists detection indices segment by segment, a segment = one (class, image), inside it in the order
 *                class_ap visits them (argsort(-rounded score) of the class, from the host); seg_off [S + 1] int64 offsets into
 *                perm; seg_gt [S] int64 each segment's row of the ground-truth CSR.  perm lists a detection at most once and
 *                seg_gt a row at most once.
 *   ground truth gt_boxes [G][4] f64 (the 1-based integers of the XML), gt_difficult [G] u8, gt_off [R + 1] int64, R rows.
 *   thrs [T] f64, T <= 16, as the host compares them (t / 100.0 computed there).
 * -> tp / fp [D] u16: bit t = class_ap's tp / fp flag of the detection at thrs[t] (both 0: matched a difficult box, or listed by no
 *    segment); bad [S] int32: 1 when the segment's offsets or one of its perm entries are out of range (such entries are skipped,
 *    nothing is read or written out of bounds), else 0.
 * Arithmetic: f64, one IEEE operation per host operation in the host's order (built with contraction off): iw = max(min(g.x2, b.x2)
 * - max(g.x1, b.x1) + 1, 0), union = (b area) + (g area) - inter left to right, ov = inter / union; numpy's minimum / maximum NaN
 * conventions; argmax = the first maximum, a NaN counts as the maximum; `best > thr` strict.  No cap on boxes or detections per
 * segment.  temp: 2 * G bytes of scratch from the caller (the claimed bits, one u16 per box), 2-byte aligned; zeroed by the call.
 * No atomics, every output has one writer: two runs give the same bytes.  No allocation, no synchronisation.
 * CDDMSL_ERR_ARG, nothing written: a negative count, T outside 1..16, S >= 2^31, a missing or misaligned pointer. */
int cddmsl_voc_match(const float* boxes, long D, const long* perm, long P, const long* seg_off, const long* seg_gt, long S,
                     const double* gt_boxes, const unsigned char* gt_difficult, const long* gt_off, long R, long G, const double* thrs,
                     int T, unsigned short* tp, unsigned short* fp, int* bad, void* temp, void* stream);
/* ---- open-vocabulary inference (csrc/openset.hip): the test_cls_score branch of FastRCNNOutputLayers.forward, predict_probs,
 * the RPN-objectness product and fast_rcnn_inference_single_image up to its NMS (roi_heads/fast_rcnn.py:546-565, 793-810, 706-710,
 * 155-180).  Everything f32; no atomics: two runs give the same bits.
 *   cddmsl_openset_logits  x [R][D], wn [K][D] unit rows -> logits [R][ld]: logits[r][c] = (x_hat_r . wn_c) * (1/T) for c < K with
 *                          x_hat = x * (1 / max(||x||, eps)) rounded per element and the contraction accumulated in f32 on the
 *                          32x32x2 f32 MFMA; logits[r][K] = 0 (zero background embedding); columns beyond K are not touched.
 *                          stats [R][2] = (m_r, l_r): the maximum of the row's K+1 logits and sum exp(logit - m_r).
 *                          D % 4 == 0, 1 <= K <= 16384, ld >= K + 1, T > 0; R == 0 succeeds with nothing launched.
 *   cddmsl_openset_select  score = expf(logit - m) / l, with objectness (nullable, [R]) sqrtf(score * objectness[r]).  A row with a
 *                          non-finite value among its ldb box values or its K+1 scores gets valid[r] = 0 and contributes nothing.
 *                          Entries with score > score_thresh and c < K are written in (row, class) order -- mask.nonzero()'s --
 *                          as cand_row / cand_cls / cand_score / cand_box; the box is the row's box of that class (ldb == 4:
 *                          class-agnostic, ldb == 4K: class-specific) clipped to [0, img_w] x [0, img_h].  count[0] is the FULL
 *                          number of entries; only the first cap are written -- the caller compares.  Scratch from the caller:
 *                          temp == NULL returns *temp_bytes.  No allocation, no synchronisation.
 * Alignment: x, wn (logits call) and boxes, cand_box (select call) are accessed as 16-byte vectors and must be 16-byte aligned; the
 * other buffers need their element's alignment only.
 * Any other argument, a misaligned pointer included, returns CDDMSL_ERR_ARG with nothing written. */
int cddmsl_openset_logits(const float* x, const float* wn, float* logits, float* stats, int R, int D, int K, int ld,
                          float temperature, float eps, void* stream);
int cddmsl_openset_select(const float* logits, const float* stats, int ld, const float* boxes, int ldb, const float* objectness,
                          int R, int K, float img_h, float img_w, float score_thresh, int* cand_row, int* cand_cls,
                          float* cand_score, float* cand_box, unsigned char* valid, int* count, int cap, void* temp,
                          size_t* temp_bytes, void* stream);
int cddmsl_iou_match(const float* gt, int G, const float* preds, int P, long* matches, signed char* labels,
                     unsigned int* best_ws, int nthr, float t0, float t1, int l0, int l1, int l2, int allow_low_quality,
                     void* stream);

/* the same for all images of a batch in one launch pair: boxes concatenated with offsets gt_off[N+1]; predictions shared by all
 * images (pred_off NULL: the anchors, outputs [N][P]) or concatenated with offsets pred_off[N+1] (proposals, outputs [sum P]) */
int cddmsl_iou_match_batched(const float* gt, const int* gt_off, const float* preds, const int* pred_off, long* matches,
                             signed char* labels, unsigned int* best_ws, int N, int P, int maxG, int totalG, int nthr, float t0,
                             float t1, int l0, int l1, int l2, int allow_low_quality, void* stream);

/* ---- CLIP attention pool (modeling/backbone/clip_backbone.py:83-107): token build/backward; the query-0 attention itself is
 * reassociated into the batched GEMMs above (cddmsl_amd/layers.py::AttnPoolFn) ------------------------------------- */
int cddmsl_attn_tokens_fwd(const void* x, const float* pos, void* tok, int K, int P, int TP, int C, int dtype, void* stream);
/* the same, also writing mbits [K][C] (64-bit words, P <= 64): bit p = (x[k][p][col] > 0), the ReLU mask of the pooled map in the
 * form cddmsl_attnpool_dx reads */
int cddmsl_attn_tokens_fwd_mask(const void* x, const float* pos, void* tok, unsigned long long* mbits, int K, int P, int TP, int C,
                                int dtype, void* stream);
/* The pool's input gradient in ONE pass (bf16, P = 49, TP = 56, C % 128 == 0): the batched product  dtok[k] = [p ; ds][k]^T . [dZ ; U][k]
 * (pds [K][H2][TP], zu [K][H2][C], H2 = 2 x heads <= 64) with the epilogue  dx[k][t-1] = dtok[t] + (dtok[0] + g0[k]) / P  for t = 1..P,
 * zeroed where bit t-1 of mbits[k][col] is clear, and  gpos[t] += sum_k dtok[k][t]  (t = 0: + g0[k]; f32 atomics, nullable) --
 * replaces the stored token gradients + cddmsl_attn_tokens_bwd.  g0 [K][C] f32: the query path's gradient of the mean token. */
int cddmsl_attnpool_dx(const void* pds, const void* zu, const float* g0, const unsigned long long* mbits, void* dx, float* gpos, int K,
                       int H2, int P, int TP, int C, int dtype, void* stream);
/* relu_mask (nullable, [K][P][C]): dx is zeroed where it is <= 0 -- the pooled map when it is a ReLU output (layer4 -> attnpool,
 * clip_roi_heads.py:160-165), so the stage's ReLU backward needs no pass of its own.  gpos (nullable, f32 [P+1][C]) accumulates
 * (atomics) the positional embedding's gradient sum_k dtok[k][t][:] in the same pass; dx may be NULL when only gpos is wanted */
int cddmsl_attn_tokens_bwd(const void* dtok, const void* relu_mask, void* dx, float* gpos, int K, int P, int TP, int C, int dtype,
                           void* stream);
/* softmax of the query-0 scores (clip_backbone.py:95-105, F.multi_head_attention_forward's softmax over the 50 keys) between the
 * batched products: S [K][H][TP] f32 -> p [K][H][P1] f32 = softmax(S[..., :P1] * scale) and pT [K][TP][H] (dtype; zero rows past
 * P1).  Backward: ds = p * (dP - sum p dP) * scale -> dsT [K][TP][H] and pds [K][2H][TP] = [p ; ds] (dtype; zero columns past P1) */
int cddmsl_attnpool_softmax_fwd(const float* S, float* p, void* pT, long K, int H, int P1, int TP, float scale, int dtype, void* stream);
int cddmsl_attnpool_softmax_bwd(const float* p, const float* dP, void* dsT, void* pds, long K, int H, int P1, int TP, float scale,
                                int dtype, void* stream);

/* ---- fused multi-head attention for short sequences: the ClipCap mapper's softmax(QK^T * scale) V (no mask), 80 tokens x 8
 * heads of 96 (modeling/backbone/clipcap/clipcap.py:59-83).  bf16 only (dtype 0), dh == 96, t <= 96; element (s, i, h, c) of
 * q / k / v / o sits at ((s*t + i) * ld + h*dh + c); the backward recomputes the probabilities from q, k. */
int cddmsl_attn_small_fwd(const void* q, const void* k, const void* v, void* o, int nseq, int t, int heads, int dh, int ldq,
                          int ldk, int ldv, int ldo, float scale, int dtype, void* stream);
int cddmsl_attn_small_bwd(const void* q, const void* k, const void* v, const void* dout, void* dq, void* dk, void* dv, int nseq,
                          int t, int heads, int dh, int ldq, int ldk, int ldv, int ldo, float scale, int dtype, void* stream);
/* the mapper's LAST layer evaluated for the last token only (v2l keeps one of the mapped tokens, clipcap.py:714-719; attention of
 * clipcap.py:59-83 with ONE query row per sequence): p [n][heads][t] f32 = softmax(q . K^T * scale), o [n][ldo] = p . V.  q [n][ldq],
 * kv [n*t][ldkv] bf16 with K of head h at column h*dh and V at column voff + h*dh; bf16 only (dtype 0), t <= 128, dh <= 128, dh % 8 == 0.
 * Backward: dq [n][ldq], dkv [n*t][ldkv] (every element written) from dout [n][ldo] and the saved p. */
int cddmsl_attn_last_fwd(const void* q, const void* kv, void* o, float* p, int n, int t, int heads, int dh, int ldq, int ldkv, int voff,
                         int ldo, float scale, int dtype, void* stream);
int cddmsl_attn_last_bwd(const void* q, const void* kv, const void* dout, const float* p, void* dq, void* dkv, int n, int t, int heads,
                         int dh, int ldq, int ldkv, int voff, int ldo, float scale, int dtype, void* stream);

/* ---- CLIP text encoder (modeling/backbone/clip_backbone.py:273-317,732-877; forward only, the encoder is frozen).  The linears
 * run on cddmsl_conv_fwd (1x1 over n*t rows) and the per-layer LayerNorms on cddmsl_layernorm_fwd; these four cover the rest.
 * text_embed:  x [rows][W] f32 = tok[ids[r]] + pos[r % t]; ids [rows] int64 in [0, vocab), tok [vocab][W] in `dtype`, pos [>= t][W] f32;
 *              W % 8 == 0, tok / pos / x 16-byte aligned.
 * attn_causal_fwd: qkv [nseq*t][ldqkv] bf16 = the in-projection as it comes (q | k | v column blocks of W = heads*dh, head h at
 *              column h*dh of its block, nn.MultiheadAttention order) -> o [nseq*t][ldo] bf16 = softmax(q k^T * scale + mask) v per
 *              (sequence, head), the mask keeping keys j <= query i.  bf16 only (dtype 0), dh == 64, t <= 128, ld % 8 == 0.
 * quick_gelu:  x = x * sigmoid(1.702 x) in place, numel % 8 == 0 (bf16) / % 4 == 0 (f32), 16-byte aligned.
 * text_pool:   y [nout][W] (`dtype`) row r = (1/group) sum_{p < group} LayerNorm(x[rows[r*group + p]]) with gamma / beta, eps;
 *              x [R][W] f32, rows int64 in [0, R), W % 64 == 0, W <= 1024. */
int cddmsl_text_embed(const long* ids, const void* tok, const float* pos, float* x, long rows, int t, int W, int vocab, int dtype,
                      void* stream);
int cddmsl_attn_causal_fwd(const void* qkv, void* o, int nseq, int t, int heads, int dh, int ldqkv, int ldo, float scale, int dtype,
                           void* stream);
int cddmsl_quick_gelu(void* x, long numel, int dtype, void* stream);
int cddmsl_text_pool(const float* x, const long* rows, const float* gamma, const float* beta, void* y, long R, int nout, int group,
                     int W, float eps, int dtype, void* stream);

/* ---- GPT-2 decoder for ClipCap captioning (gen_captions.py, clipcap.py generate2; forward only).  The prefill runs on
 * cddmsl_conv_fwd, cddmsl_layernorm_fwd and cddmsl_attn_causal_fwd; these cover the rest and the decode step.
 * skinny_gemm: y [M][N] = x [M][K] bf16 @ w [N][K]^T bf16 + bias [N] f32 (optional), f32 accumulation, 1 <= M <= 64, N % 8 == 0,
 *              K % 64 == 0, all pointers 16-byte aligned.  epi 0: y bf16; 1: y f32 (+ residual [M][N] f32 if given; y may be
 *              residual); 2: y bf16 = gelu_new (tanh form).  A fixed split of K that depends on (N, K) only goes through ws
 *              (ws_bytes >= cddmsl_skinny_gemm_workspace(M, N, K)): a row's result does not depend on M or the other rows.
 * skinny_gemm_workspace: the bytes skinny_gemm needs in ws, -1 outside the contract.
 * lm_head_argmax: ids[m * ld_ids] (int64) = argmax_v (h [M][K] bf16 @ wte [V][K]^T bf16)[m][v], the lowest index among equal
 *              maxima; 1 <= M <= 64, K % 64 == 0; logits [M][V] f32 written only when non-NULL; ws_bytes >=
 *              cddmsl_lm_head_workspace(M, V).
 * decode_attn: per (sequence s, head h), dh == 64: o [nseq][heads*64] bf16 = softmax(q k^T * scale) v over positions 0..L-1;
 *              qkv [nseq][ldqkv] bf16 = this step's c_attn output (q | k | v blocks of heads*64 columns), kc / vc [nseq][Lmax][heads*64]
 *              bf16 hold positions 0..L-2; this step's k / v (position L-1) are read from qkv and written to kc / vc.
 *              1 <= L <= min(Lmax, 1024), bf16 only (dtype 0).
 * pos_embed:   x [rows][W] f32 = row value + wpe[pos0 + r % t]; the row value is tab[ids[r * ld_ids]] (tab [vocab][W] in `dtype`)
 *              when ids is given, else src [rows][W] f32 (exactly one of ids / src); pos0 + t <= npos, W % 8 == 0.
 * gelu_new:    x = 0.5 x (1 + tanh(sqrt(2/pi) (x + 0.044715 x^3))) in place, numel % 8 == 0 (bf16) / % 4 == 0 (f32).
 * Beam search (length-normalised, beam width 1 <= B <= 8; row = caption * B + beam):
 * lm_head_topk: per row m of h [M][K] bf16 @ wte [V][K]^T bf16: vals [M][B] f32 / idx [M][B] int32 = the B largest logits in the order
 *              "larger value, then lower index" (lm_head_argmax's), logZ [M] f32 = max + log(sum exp(logit - max)).  The f32 logits
 *              go to `logits` [M][V] when non-NULL, else to ws (ws_bytes >= cddmsl_lm_head_topk_workspace(M, V)).  1 <= M <= 64,
 *              K % 64 == 0, B <= V.  No atomics; a row's outputs do not depend on M or on the other rows.
 * beam_step:   one selection step for n captions.  step >= 1: vals / idx [n*B][B] and logZ [n*B] of the rows' logits; the state
 *              sum [n*B] f32, len [n*B] int32, stop [n*B] uint8, hist [n*B][T] int32 (tokens, -1 past the length) and the ancestry
 *              table anc [n*B][T-1] uint8 are read from *_in and written to *_out (distinct buffers).  A live beam offers its B
 *              tokens with key (sum + (logit - logZ)) / (len + 1), a stopped beam itself with key sum / len; the B largest keys
 *              survive, ties to the lower (beam, token); new beam j = the j-th survivor: src [n*B] int32 its source beam, next_tok
 *              [n*B] int64 the token it appended (stop_id once stopped), hist_out its source's tokens plus that token at `step`,
 *              anc_out its source's ancestry plus the source beam at step - 1.  step == 0: vals / idx [n][B], logZ [n]; beam j
 *              takes the j-th pair (the *_in tables may be NULL).  stop_id -1: none.  0 <= step < T.
 * decode_attn_beam: decode_attn with indirect keys / values: positions j < P from the caption's prefix cache pk / pv
 *              [rows/B][P][heads*64], P <= j < L-1 from the generated cache gk / gv [rows][Tg][heads*64] at row
 *              (r / B) * B + anc[r * ldanc + j - P], position j - P; position L-1 from qkv, written to gk / gv at row r, position
 *              L-1-P.  P + 1 <= L <= min(P + Tg, 1024).  The summation orders are decode_attn's. */
int cddmsl_skinny_gemm_workspace(int M, int N, int K);
int cddmsl_skinny_gemm(const void* x, const void* w, const float* bias, const float* residual, void* y, float* ws, long ws_bytes, int M,
                       int N, int K, int epi, void* stream);
int cddmsl_lm_head_workspace(int M, int V);
int cddmsl_lm_head_argmax(const void* h, const void* wte, long* ids, int ld_ids, float* logits, void* ws, long ws_bytes, int M, int V,
                          int K, void* stream);
int cddmsl_decode_attn(const void* qkv, void* kc, void* vc, void* o, int nseq, int heads, int dh, int L, int Lmax, int ldqkv, float scale,
                       int dtype, void* stream);
int cddmsl_pos_embed(const long* ids, int ld_ids, const void* tab, const float* src, const float* wpe, float* x, long rows, int t, int pos0,
                     int W, int vocab, int npos, int dtype, void* stream);
int cddmsl_gelu_new(void* x, long numel, int dtype, void* stream);
int cddmsl_lm_head_topk_workspace(int M, int V);
int cddmsl_lm_head_topk(const void* h, const void* wte, float* vals, int* idx, float* logZ, float* logits, void* ws, long ws_bytes, int M,
                        int V, int K, int B, void* stream);
int cddmsl_beam_step(const float* vals, const int* idx, const float* logZ, const float* sum_in, const int* len_in,
                     const unsigned char* stop_in, const int* hist_in, const unsigned char* anc_in, float* sum_out, int* len_out,
                     unsigned char* stop_out, int* hist_out, unsigned char* anc_out, int* src, long* next_tok, int n, int B, int T, int step,
                     int stop_id, void* stream);
int cddmsl_decode_attn_beam(const void* qkv, const void* pk, const void* pv, void* gk, void* gv, const unsigned char* anc, void* o, int rows,
                            int B, int heads, int dh, int P, int L, int Tg, int ldanc, int ldqkv, float scale, int dtype, void* stream);

/* ---- fp32 heads: cosine-logit classifier (modeling/roi_heads/fast_rcnn.py:546-572) and the contrastive loss over
 * the cosine-similarity matrix (modeling/meta_arch/rcnn.py:308-317,458-468) ------------------------------------ */
int cddmsl_l2norm_fwd(const float* x, float* y, float* inv, long R, int D, float eps, void* stream);
int cddmsl_l2norm_bwd(const float* dy, const float* y, const float* inv, float* dx, long R, int D, void* stream);
int cddmsl_cosine_logits_fwd(const float* x, const float* wn, float* scores, float* inv, long R, int D, int Kc,
                             float temperature, float eps, void* stream);
int cddmsl_cosine_logits_bwd(const float* ds, const float* x, const float* wn, const float* inv, float* dx, long R, int D,
                             int Kc, float temperature, int accumulate, void* stream);
/* mapper LayerNorm (modeling/backbone/clipcap/clipcap.py:97-100; frozen affine) and the focal-scaled, background-weighted
 * classification loss (modeling/roi_heads/fast_rcnn.py:624-644): row_loss = CE * (1-p_t)^gamma * w; probs saved for backward */
int cddmsl_layernorm_fwd(const float* x, const float* gamma, const float* beta, void* y, float* mean, float* rstd, long R, int D,
                         float eps, int dtype, void* stream);
int cddmsl_layernorm_bwd(const void* dy, const float* x, const float* gamma, const float* mean, const float* rstd, float* dx,
                         long R, int D, int accumulate, int dtype, void* stream);
/* the same on the vector kernel (D 256/512/768/1024, 16-byte aligned) with a second output dx_bf16 [R][D] = bf16(dx), nearest even;
 * *emitted = 1 when it was written, 0 when the rows took the scalar kernel (dx alone is written then) */
int cddmsl_layernorm_bwd_emit(const void* dy, const float* x, const float* gamma, const float* mean, const float* rstd, float* dx,
                              void* dx_bf16, long R, int D, int accumulate, int dtype, int* emitted, void* stream);
int cddmsl_focal_ce_fwd(const float* logits, const long* target, float* row_loss, float* probs, long R, int C, float gamma,
                        int bg_class, float bg_weight, void* stream);
int cddmsl_focal_ce_bwd(const float* logits, const long* target, const float* probs, const float* gscale, float* dlogits, long R,
                        int C, float gamma, int bg_class, float bg_weight, void* stream);
int cddmsl_contrastive_fwd(const float* S, float* rlse, float* clse, float* loss, int n, int ld, void* stream);
int cddmsl_contrastive_bwd(const float* S, const float* rlse, const float* clse, const float* gloss, float* dS, int n, int ld,
                           void* stream);
/* Losses over SAMPLED rows with known index lists (no dense pass, no boolean-mask gathers):
 *   cddmsl_rpn_losses: RPN.losses (modeling/proposal_generator/rpn.py:365-429; _dense_box_regression_loss box_regression.py:229-270, smooth-L1 beta 0):
 *     out2 = (sum_{sampled} BCE-with-logits, sum_{positives} |delta - get_deltas(anchor, matched gt)|) * inv_norm.  logits [N*A], deltas [N*A][4],
 *     pos / neg = global anchor indices (image * A + anchor), midx [N*A] matched gt index within the image, gt [G][4], gt_off [N], anchors [A][4].
 *   cddmsl_box_l1: FastRCNNOutputLayers.box_reg_loss (modeling/roi_heads/fast_rcnn.py:646-689): out1 = sum_{fg rows} |delta[4 cls[r] ..] - get_deltas(src, tgt)| * inv_norm;
 *     cls nullable (class-agnostic).  Backward = the same entry point with gout given: gradients are scattered into CALLER-ZEROED tensors. */
int cddmsl_rpn_losses(const float* logits, const float* deltas, const long* pos, int npos, const long* neg, int nneg, const long* midx,
                      const float* gt, const long* gt_off, const float* anchors, long A, float wx, float wy, float ww, float wh, float inv_norm,
                      float* out2, const float* gout2, float* dlogits, float* ddeltas, void* stream);
int cddmsl_box_l1(const float* deltas, int ld, const long* fg, int nfg, const long* cls, const float* src, const float* tgt, float wx, float wy,
                  float ww, float wh, float inv_norm, float* out1, const float* gout1, float* ddeltas, void* stream);
/* The same pair with the reference's other box-regression terms (MODEL.RPN / ROI_BOX_HEAD .BBOX_REG_LOSS_TYPE, .SMOOTH_L1_BETA;
 * box_regression.py:229-270, fast_rcnn.py:646-689): three scalars in front of the outputs, every other argument and convention as above.
 *   loc_type 0: smooth-L1 with beta (fvcore smooth_l1_loss): n = |delta - get_deltas(..)|; beta < 1e-5: n; else n < beta ? 0.5 n n / beta : n - 0.5 beta,
 *     gradient n < beta ? e / beta : sgn(e).  loc_type 0 with beta 0 returns the bytes of cddmsl_rpn_losses / cddmsl_box_l1.
 *   loc_type 1: GIoU (fvcore giou_loss, reduction sum, eps 1e-7) of Box2BoxTransform.apply_deltas(the row's 4 deltas, anchor / src) (box_regression.py:77-115,
 *     dw / dh clamped from above at scale_clamp) against the gt box / tgt; beta is ignored.  Backward = the analytic gradient with torch autograd's
 *     conventions: max / min of EQUAL operands hands the prediction HALF the gradient, the clamp passes it at dw == scale_clamp and blocks it above,
 *     a row whose intersection test (both comparisons strict) fails has no gradient through the intersection.
 * CDDMSL_ERR_ARG, nothing written: loc_type not 0 / 1, beta < 0 or NaN, scale_clamp not finite at loc_type 1, and what the pair above refuses. */
int cddmsl_rpn_losses_reg(const float* logits, const float* deltas, const long* pos, int npos, const long* neg, int nneg, const long* midx,
                          const float* gt, const long* gt_off, const float* anchors, long A, float wx, float wy, float ww, float wh, float inv_norm,
                          int loc_type, float beta, float scale_clamp, float* out2, const float* gout2, float* dlogits, float* ddeltas, void* stream);
int cddmsl_box_reg_loss(const float* deltas, int ld, const long* fg, int nfg, const long* cls, const float* src, const float* tgt, float wx, float wy,
                        float ww, float wh, float inv_norm, int loc_type, float beta, float scale_clamp, float* out1, const float* gout1, float* ddeltas,
                        void* stream);

/* ---- elementwise: preprocessing (modeling/meta_arch/rcnn.py:161-179,758-768, structures/image_list.py:72-124),
 * AvgPool2d(2) (clip_backbone.py:36,46,147), ReLU backward, column sums, fused clip+SGD (solver/build.py:59-130) -- */
int cddmsl_preprocess(const unsigned char* img, void* out, int n, int h, int w, int Hp, int Wp, int Cp, const float* mean3,
                      const float* std3, int div255, int dtype, void* stream);
int cddmsl_preprocess224(const unsigned char* img, void* out, int n, int h, int w, int Hp, int Wp, int RH, int RW, int top,
                         int left, int S, int Cp, const float* mean3, const float* std3, int dtype, void* stream);
/* the same two for a whole batch in one launch: imgs / hs / ws are HOST arrays of N device pointers / heights / widths (the images are
 * separate tensors of different sizes: ImageList.from_tensors, structures/image_list.py:72-124); image j is written to out[j] */
int cddmsl_preprocess_batch(const unsigned char* const* imgs, const int* hs, const int* ws, int N, void* out, int Hp, int Wp, int Cp,
                            const float* mean3, const float* std3, int div255, int dtype, void* stream);
int cddmsl_preprocess224_batch(const unsigned char* const* imgs, const int* hs, const int* ws, int N, void* out, int Hp, int Wp, int RH,
                               int RW, int top, int left, int S, int Cp, const float* mean3, const float* std3, int dtype, void* stream);
/* test-time-augmentation views (modeling/test_time_augmentation.py:58-98) made on the device (tta_views.hip): img u8 [3][h][w] ->
 * Pillow's bilinear resize to (newh, neww), bit for bit (two separable passes, 22-bit fixed-point coefficients, uint8 between the
 * passes, a pass whose size does not change skipped) -> the normalisation of cddmsl_preprocess -> slot n0 of out0 [N][Hp0][Wp0][Cp],
 * and, with out1 != NULL, the left-right mirror of the view -> slot n1 of out1 [N][Hp1][Wp1][Cp].  Padding and channels 3..Cp are
 * zeroed; other slots are not touched.  xlo / xn [neww], xk [neww][xks] (horizontal pass) and ylo / yn [newh], yk [newh][yks]
 * (vertical pass) are DEVICE int32 tables: window start, window length, coefficients int(0.5 + w * 2^22), computed on the host in
 * double in Pillow's order (cddmsl_amd/hip.py); NULL is allowed for a pass that is skipped (neww == w / newh == h). */
int cddmsl_tta_view(const unsigned char* img, int h, int w, int newh, int neww, const int* xlo, const int* xn, const int* xk, int xks,
                    const int* ylo, const int* yn, const int* yk, int yks, void* out0, int n0, int Hp0, int Wp0, void* out1, int n1,
                    int Hp1, int Wp1, int Cp, const float* mean3, const float* std3, int div255, int dtype, void* stream);
/* the loader's ResizeShortestEdge + RandomFlip for a whole batch in ONE launch (loader_resize.hip; a launch per 32 items beyond that):
 * item i reads the uint8 image [h][w][3] (interleaved, as PIL decodes it) at byte src_off of src and writes Pillow's bilinear resize
 * to (newh, neww) -- the arithmetic of cddmsl_tta_view, bit for bit -- as planar uint8 [3][newh][neww] at byte dst_off of dst; with
 * reverse_channels plane c takes source channel 2 - c (INPUT.FORMAT BGR).  flip is a bit set: with bit 0 column x is written to
 * column neww - 1 - x (RandomFlip horizontal), with bit 1 row y of each plane is written to row newh - 1 - y (vertical), 3 does
 * both; a value outside 0..3 is CDDMSL_ERR_ARG.  (Before bit 1 had a meaning the kernel tested flip for truth only, so 2 happened to
 * mirror the columns; no caller passed it.)
 * xtab / ytab: position (in int32 elements) of the axis' table in tab [tab_len], laid out lo [out] | n [out] | k [out][ks] with
 * ks = xks / yks (cddmsl_amd/resample.py); -1 for an axis whose size does not change, which is copied.  Items may share tables (an
 * image and its twin do).  The descriptors are a HOST array.  Every item is checked before the first launch: positive sizes, a flip code of 0..3,
 * offset + extent inside src_bytes / dst_bytes, a table exactly where an axis changes and inside tab_len; anything else is
 * CDDMSL_ERR_ARG with nothing launched.  count == 0 succeeds with nothing launched.  Bytes of dst outside the items' extents are
 * not written. */
typedef struct cddmsl_resize_item {
  long src_off, dst_off;
  int h, w, newh, neww, flip, reverse_channels, xtab, xks, ytab, yks;
} cddmsl_resize_item;
int cddmsl_resize_batch_u8(const unsigned char* src, long src_bytes, unsigned char* dst, long dst_bytes, const int* tab, long tab_len,
                           const cddmsl_resize_item* items, int count, void* stream);
int cddmsl_avgpool2_fwd(const void* x, void* y, int N, int H, int W, int C, int dtype, void* stream);
int cddmsl_avgpool2_bwd(const void* dy, const void* mask, const void* add, void* dx, int N, int H, int W, int C, int dtype,
                        void* stream);
/* bf16 only: the forward also writes the ReLU mask of x, bits [N][H/2][W/2][C/8] u32 -- byte (dy*2+dx) of a word = (x[2oy+dy][2ox+dx][8c+j] > 0)
 * in bit j; the backward reads that word instead of the full-resolution mask: dx = (bit ? dy/4 : 0), zero on a floor-dropped row / column */
int cddmsl_avgpool2_fwd_bits(const void* x, void* y, void* bits, int N, int H, int W, int C, int dtype, void* stream);
int cddmsl_avgpool2_bwd_bits(const void* dy, const void* bits, void* dx, int N, int H, int W, int C, int dtype, void* stream);
/* fp8 configuration: the same pass (bf16 only) with a second output, y8 = e4m3 of sat(dx * q8[0]), max|dx| recorded in amax8 (64 floats) */
int cddmsl_avgpool2_bwd_q8(const void* dy, const void* mask, const void* add, void* dx, int N, int H, int W, int C, void* y8,
                           const float* q8, float* amax8, void* stream);
/* stock Detectron2 R50-C4 pieces (config #1): BasicStem max-pool (modeling/backbone/resnet.py:355-358), the input-gradient
 * scatter of stride-2 1x1 convs (STRIDE_IN_1X1 bottlenecks, resnet.py:100-210), Res5ROIHeads mean pool (roi_heads.py:487) */
int cddmsl_maxpool3s2_fwd(const void* x, void* y, int N, int H, int W, int C, int dtype, void* stream);
int cddmsl_upsample_zero2(const void* t, const void* mask, const void* add, void* dx, int N, int H, int W, int C, int dtype,
                          void* stream);
int cddmsl_meanpool_fwd(const void* x, float* y, long K, int P, int C, int dtype, void* stream);
int cddmsl_meanpool_bwd(const float* dy, void* dx, long K, int P, int C, int dtype, void* stream);
int cddmsl_relu_bwd(const void* g, const void* y, void* dx, long numel, int g_f32, int dtype, void* stream);
int cddmsl_colsum(const void* x, float* out, long rows, int cols, int period, int dtype, void* stream);
int cddmsl_sgd_clip_step(float** params, const float** grads, float** moms, const long* sizes, int count, float* norm_ws,
                         float lr, float momentum, float wd, float clip, int first_step, void* stream);
/* torch.optim.SGD (dampening 0) with one lr and one weight decay PER TENSOR (host arrays lrs / wds of `count` entries, like the
 * pointer arrays), optional Nesterov momentum and the per-parameter gradient clipping of solver/build.py:23-40.
 * clip_mode 0: none; 1: value, g clamped to [-clip_value, clip_value] (clip_grad_value_); 2 / 3 / 4: L2 / L1 / inf norm of the
 * tensor, g *= min(clip_value / (norm + 1e-6), 1) (clip_grad_norm_ on the single tensor).  Per element, in f32:
 *   d = clip(g) + wd_i p;  buf = first_step ? d : momentum buf + d;  p -= lr_i (nesterov ? d + momentum buf : buf)
 * buf is always written and not read on the first step.  Modes 2-4 leave sum g^2, sum |g| or max |g| in norm_ws[i], i < count;
 * modes 0 and 1 do not touch norm_ws.  A NaN gradient element is kept: under every norm (the inf norm included) it makes the
 * tensor's norm_ws entry, coefficient and parameters NaN, as torch does; other tensors are unaffected.
 * CDDMSL_ERR_ARG for count < 0, clip_mode outside 0..4 or nesterov outside {0, 1}; count == 0 launches nothing. */
int cddmsl_sgd_step_groups(float** params, const float** grads, float** moms, const long* sizes, const float* lrs, const float* wds,
                           int count, float* norm_ws, float momentum, int nesterov, int clip_mode, float clip_value, int first_step,
                           void* stream);

/* ---- Training the ClipCap mapper against the frozen GPT-2 (the reference's clipcap.py: ClipCaptionModel.forward, train with
 * --only_prefix).  No floating-point atomics: reductions have a fixed order, one call gives the same bits twice.
 * attn_causal_bwd: backward of attn_causal_fwd, same layouts and contract (bf16, dh == 64, t <= 128, ld % 8 == 0, 16-byte
 *              aligned): qkv [nseq*t][ldqkv] (q | k | v), dout [nseq*t][ldo] -> dqkv [nseq*t][ldqkv] (dq | dk | dv).  The
 *              probabilities are recomputed from q, k.  All three blocks are written in full; columns >= 3*heads*dh are not touched.
 * gelu_new_bwd: dx = dy * gelu_new'(x_pre), x_pre the value from before the activation; any numel, 16-byte aligned pointers.
 * token_ce_fwd: logits [R][ld] f32, classes are columns < V <= ld (the rest is padding, never read as a class), ld % 8 == 0,
 *              target [R] int64.  lse [R], row_loss [R] (0 on rows whose target is ignore_index; NaN where a target that is not
 *              ignore_index lies outside [0, V)), sum_count[0] = sum of row_loss, sum_count[1] = number of rows that count.
 *              The mean is sum / count, the caller's division (count may be 0).
 * token_ce_bwd: dlogits [R][ld] (dtype_out 0: bf16, 1: f32) = (softmax - onehot) * gscale on rows that count and columns < V,
 *              zero elsewhere.  With dtype_out 1 dlogits may be logits.
 * layernorm_bwd_params: dgamma [D] = sum_r dy (x - mean) rstd, dbeta [D] = sum_r dy, what cddmsl_layernorm_bwd leaves out;
 *              dy [R][D] in `dtype`, x f32; accumulate 1 adds to dgamma / dbeta.  ws holds the per-chunk partial sums,
 *              ws_bytes >= cddmsl_layernorm_bwd_params_workspace(R, D) (-1 outside the contract).
 * adamw_step:  torch.optim.AdamW (amsgrad off) over `count` f32 tensors, host pointer arrays as in sgd_step_groups; step >= 1 is
 *              the step being taken (bias corrections 1 - beta^step).  Per element:
 *                p *= 1 - lr wd;  m += (g - m)(1 - beta1);  v = beta2 v + (1 - beta2) g g;
 *                p -= lr / (1 - beta1^step) * m / (sqrt(v) / sqrt(1 - beta2^step) + eps)
 *              A NaN gradient element makes that element of m, v and p NaN, as torch does; other tensors are unaffected. */
int cddmsl_attn_causal_bwd(const void* qkv, const void* dout, void* dqkv, int nseq, int t, int heads, int dh, int ldqkv, int ldo,
                           float scale, int dtype, void* stream);
int cddmsl_gelu_new_bwd(const void* x_pre, const void* dy, void* dx, long numel, int dtype, void* stream);
int cddmsl_token_ce_fwd(const float* logits, int ld, const long* target, long R, int V, long ignore_index, float* lse, float* row_loss,
                        float* sum_count, void* stream);
int cddmsl_token_ce_bwd(const float* logits, int ld, const long* target, const float* lse, float gscale, void* dlogits, long R, int V,
                        long ignore_index, int dtype_out, void* stream);
int cddmsl_layernorm_bwd_params_workspace(long R, int D);
int cddmsl_layernorm_bwd_params(const void* dy, const float* x, const float* mean, const float* rstd, float* dgamma, float* dbeta,
                                float* ws, long ws_bytes, long R, int D, int accumulate, int dtype, void* stream);
int cddmsl_adamw_step(float** params, const float** grads, float** exp_avg, float** exp_avg_sq, const long* sizes, int count, float lr,
                      float beta1, float beta2, float eps, float weight_decay, long step, void* stream);

/* ---- Sparse backward pass of the RPN head (3x3 "same" conv + ReLU -> fused 1x1 heads) ------------------------------------
 * The sampled loss (rpn.py:365-429) leaves the heads' output gradient non-zero on a few rows, and the convolution's two gradient
 * GEMMs then run over those rows only, through cddmsl_conv_fwd / cddmsl_conv_wgrad / cddmsl_gemm_nt_batched.  These five
 * (csrc/rpn_sparse.hip) are the bookkeeping around them; none uses atomics.
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

/* ---- Cityscapes instance boxes (input side, not the training step) -------------------------------------------------------
 * replaces the per-id `inst_image == instance_id` + np.nonzero loop of data/datasets/cityscapes.py:501-540 (from_json=False).
 * maps [B][H][W] instance ids, dtype 0 = uint16, 1 = int32.  For every map b, one record per id in [24, 34000) that occurs in it,
 * in ascending id order: records[b][r][6] int32 = (id, xmin, ymin, xmax, ymax, npixels), the box being the inclusive pixel-index
 * extent; counts[b] = number of records, or -1 if the map holds an id >= 34000 (no Cityscapes label: the reference's id2label
 * raises; the device reports it here and the caller raises CDDMSL_ERR_ARG after its readback).  Ids below 24 are stuff and skipped.
 * max_records >= min(H * W, 33976).  Workspace: call with ws == NULL to get *ws_bytes; it is zeroed on the stream by every call.
 * Integer atomics only: the output is bit-identical from run to run. */
int cddmsl_instance_boxes(const void* maps, int B, int H, int W, int dtype, int* records, int max_records, int* counts, void* ws,
                          size_t* ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CDDMSL_HIP_H */
