"""Case table of tests/test_gpu_gemm_exact.py, plain data (the host test imports it to check that every launch recorded in
tests/golden/bench_gemm_launches.json -- the CLIP benchmark step -- and in tests/golden/stock_gemm_launches.json -- the stock R50-C4
configuration's step --, in their f32 twins bench_gemm_launches_f32.json and stock_gemm_launches_f32.json -- the same steps in f32 on one
image -- and every kernel instantiation, bf16 and f32, has a Tier A and a Tier B case).

A case: entry point, the kernel id dispatch must pick (cddmsl_last_kernel; hip.py _CONV_KERNEL), the per-call switches that force
it, the geometry (the keys tools/record_gemm_launches.py writes), the epilogue flags, the tiers it runs in, the variants it covers
and -- ``why`` -- which variant it targets and which function of the dispatch selects it (plan_* in cddmsl_amd/csrc/gemm_conv.hip choose the
kernel, launch_* in the kernel's own file -- conv_fwd.hip, conv_fwd256.hip, conv_wgrad.hip -- its instantiation).
Tier A: small-integer operands, every partial sum exact in f32, output bit-equal to the exact value rounded once.
Tier B: Gaussian operands, held to exact_gemm.check_bound and exact_gemm.rounding_bias."""

AB = ("A", "B")
F256 = {"CDDMSL_GEMM256": "2", "CDDMSL_FWD2": "0"}          # forces k_conv_fwd256 / k_wgrad256 wherever legal
F128 = {"CDDMSL_GEMM256": "0", "CDDMSL_FWD2": "0"}          # the 128x128 kernels (k_conv_fwd / k_conv_wgrad_dma)
FWD2 = {"CDDMSL_FWD2": "2"}


def conv(N, H, W, Cin, Cout, K=1, stride=1, pad=0, pool=False):
    return dict(N=N, H=H, W=W, Cin=Cin, Cout=Cout, KH=K, KW=K, stride=stride, pad=pad, pool=pool, dtype="bf16")


def fwd(scale=False, bias=False, residual=None, relu=False, relu_mask=False, out_f32=False):
    return dict(scale=scale, bias=bias, residual=residual, relu=relu, relu_mask=relu_mask, out_f32=out_f32, emit8=False)


def wg(scale=False, accumulate=False):
    return dict(scale=scale, accumulate=accumulate)


def case(id, entry, kid, geom, epi, env, why, variants=(), tiers=AB):
    return dict(id=id, entry=entry, kid=kid, geom=geom, epi=epi, env=env, why=why, variants=tuple(variants), tiers=tiers)


# every epilogue operand set the step launches, per kernel (bench_gemm_launches.json)
_FWD_SETS_1X1 = {
    "plain": fwd(), "bn": fwd(True, True), "bn_relu": fwd(True, True, relu=True), "bias_relu": fwd(bias=True, relu=True),
    "bn_res_relu": fwd(True, True, "bf16", True), "res": fwd(residual="bf16"), "mask": fwd(relu_mask=True),
    "mask_res": fwd(residual="bf16", relu_mask=True), "f32": fwd(out_f32=True), "bias_f32": fwd(bias=True, out_f32=True),
    "bias_relu_f32": fwd(bias=True, relu=True, out_f32=True), "bias_resf32_f32": fwd(bias=True, residual="f32", out_f32=True),
}

CASES = []
# ---- k_conv_fwd (id 1): the 128x128 kernel, plan_fwd's default (gemm_conv.hip) when neither k_conv_fwd256
# (use_gemm256) nor k_conv_fwd2 (use_fwd2) is taken.  Ragged M (666 rows) and N (136 columns).
for k, e in _FWD_SETS_1X1.items():
    CASES.append(case(f"fwd_1x1_{k}", "conv_fwd", 1, conv(2, 9, 37, 64, 136), e, F128, "k_conv_fwd 1x1, plan_fwd's default", ["fwd"]))
CASES += [
    case("fwd_3x3_bn_relu", "conv_fwd", 1, conv(2, 9, 13, 64, 96, 3, 1, 1), fwd(True, True, relu=True), F128, "k_conv_fwd taps, plan_fwd's default", ["fwd"]),
    case("fwd_3x3_mask", "conv_fwd", 1, conv(2, 9, 13, 64, 96, 3, 1, 1), fwd(relu_mask=True), F128,
         "k_conv_fwd taps, ReLU-mask input gradient, plan_fwd's default", ["fwd", "relu_mask"]),
    case("fwd_s56_bias", "conv_fwd", 1, conv(37, 1, 56, 128, 136, 1, 56), fwd(bias=True), F128,
         "k_conv_fwd, the attention pool's strided query projection (one row of every 56), plan_fwd's default", ["fwd"]),
    case("fwd_reg_pool", "conv_fwd", 2, conv(2, 15, 21, 64, 160, pool=True), fwd(), F128,
         "k_conv_fwd_reg: AvgPool2d(2) fused into the loader, odd sizes floor, plan_fwd (pool)", ["fwd_reg_pool"]),
    case("fwd_reg_pool_bn_relu", "conv_fwd", 2, conv(3, 14, 14, 128, 256, pool=True), fwd(True, True, relu=True), {},
         "k_conv_fwd_reg (pool is never legal on the 256 kernels: gemm256_legal), plan_fwd (pool)", ["fwd_reg_pool"]),
    case("fwd_full_m_rpn_1x1", "conv_fwd", 1, conv(32, 14, 14, 1024, 256), fwd(True, True, relu=True), {},
         "k_conv_fwd at a bench launch (res5 head, 6272 rows; too few 256x256 tiles for use_gemm256), plan_fwd's default", ["fwd", "full_m"]),
]
CASES += [
    case("fwd_f32_1x1", "conv_fwd", 1, dict(conv(1, 1, 300, 256, 136), dtype="f32"), fwd(), {},
         "k_conv_fwd<float> (the step's f32 1x1 launches: too few 256x256 tiles, Cout 136 not a fwd2 width), plan_fwd's default", ["fwd_f32"]),
    case("fwd_f32_1x1_narrow", "conv_fwd", 1, dict(conv(1, 1, 16, 256, 16), dtype="f32"), fwd(), {},
         "k_conv_fwd<float> at the step's 16 x 256 -> 16 launch, plan_fwd's default", ["fwd_f32"]),
]
# ---- k_conv_fwd2 (id 11): the 256x128 two-workgroup kernel, use_fwd2 in plan_fwd; launch_fwd / launch_fwd2 pick TAPS / EPI
for k in ("plain", "bn_relu", "mask", "bias_f32"):
    CASES.append(case(f"fwd2_1x1_{k}", "conv_fwd", 11, conv(2, 19, 23, 96, 384), _FWD_SETS_1X1[k], FWD2,
                      "k_conv_fwd2<bf16, false, EPI> (EPI -1 for f32 output), launch_fwd2", ["fwd2_1x1"]))
for k in ("bn_relu", "mask"):
    CASES.append(case(f"fwd2_3x3_{k}", "conv_fwd", 11, conv(2, 19, 23, 32, 128, 3, 1, 1), _FWD_SETS_1X1[k], FWD2,
                      "k_conv_fwd2<bf16, true, EPI>, launch_fwd2", ["fwd2_taps"]))
CASES += [
    case("fwd2_full_m_res2_3x3", "conv_fwd", 11, conv(16, 200, 333, 128, 128, 3, 1, 1), fwd(True, True, relu=True), {},
         "k_conv_fwd2 at the bench's (1065600, 128, 1152) launch, use_fwd2's heuristic", ["fwd2_taps", "full_m"]),
    case("fwd2_full_m_res2_3x3_mask", "conv_fwd", 11, conv(16, 200, 333, 128, 128, 3, 1, 1), fwd(relu_mask=True), {},
         "k_conv_fwd2 input-gradient form at the bench's (1065600, 128, 1152) launch, use_fwd2's heuristic", ["fwd2_taps", "full_m", "relu_mask"]),
]
# ---- k_conv_fwd256 (id 3): use_gemm256 in plan_fwd; launch_fwd / launch256 / launch256_main pick the instantiation
for k, e in _FWD_SETS_1X1.items():
    CASES.append(case(f"fwd256_1x1_{k}", "conv_fwd", 3, conv(2, 19, 23, 128, 512), e, F256,
                      "k_conv_fwd256<bf16, false, false, EPI> (EPI -1: f32 output / f32 residual, launch256), launch256_main",
                      ["fwd256_1x1"] + (["fwd256_out_f32"] if e["out_f32"] else []) + (["fwd256_res_f32"] if e["residual"] == "f32" else [])))
for k in ("plain", "bias_relu", "bn_relu", "mask"):
    CASES.append(case(f"fwd256_3x3_{k}", "conv_fwd", 3, conv(2, 19, 23, 64, 256, 3, 1, 1), _FWD_SETS_1X1[k], F256,
                      "k_conv_fwd256<bf16, true, false, EPI>, launch256_main", ["fwd256_taps"]))
CASES += [
    case("fwd256_s56_bias", "conv_fwd", 3, conv(37, 1, 56, 128, 256, 1, 56), fwd(bias=True), F256,
         "k_conv_fwd256 on the strided query projection (stride is legal on the 256 kernel: gemm256_legal), launch256_main", ["fwd256_1x1"]),
    case("fwd256_res_pool", "conv_fwd", 3, conv(3, 15, 21, 128, 256), fwd(residual="pooled"), F256,
         "k_conv_fwd256<bf16, false, true>: AvgPool2d(2)-backward residual, odd sizes, launch_fwd (res_pool)", ["fwd256_res_pool"]),
    case("fwd256_res_pool_mask", "conv_fwd", 3, conv(2, 50, 84, 64, 512), fwd(residual="pooled", relu_mask=True), F256,
         "k_conv_fwd256<bf16, false, true> with the ReLU mask, launch_fwd (res_pool)", ["fwd256_res_pool", "relu_mask"]),
    case("fwd256_persistent", "conv_fwd", 3, conv(1, 83003, 1, 128, 1024), fwd(True, True, "bf16", True), F256,
         "persistent form (K <= 512, 1 300 tiles > CUs, ragged last panel): launch256_main's persistent form", ["fwd256_persistent"]),
    case("fwd256_persistent_mask", "conv_fwd", 3, conv(1, 83003, 1, 128, 1024), fwd(residual="bf16", relu_mask=True), F256,
         "persistent form, EPI 3, launch256_main", ["fwd256_persistent", "relu_mask"]),
    case("fwd256_tail_split_3x3", "conv_fwd", 3, conv(13, 64, 80, 320, 256, 3, 1, 1), fwd(True, True, "bf16", True),
         dict(F256, CDDMSL_TAIL_SPLIT="1"),
         "K-split tail (260 tiles on 256 CUs, K slices starting inside taps) + k_conv_split_reduce epilogue: plan_tail_split in launch256", ["fwd256_tail_split"]),
    case("fwd256_tail_split_mask", "conv_fwd", 3, conv(13, 64, 80, 320, 256, 3, 1, 1), fwd(relu_mask=True), dict(F256, CDDMSL_TAIL_SPLIT="1"),
         "K-split tail, the ReLU-mask form of k_conv_split_reduce, plan_tail_split in launch256", ["fwd256_tail_split", "relu_mask"]),
    case("fwd256_dgrad_wd", "conv_fwd", 3, conv(2, 19, 23, 256, 256, 3, 1, 1), fwd(relu_mask=True), F256,
         "input gradient through weight_prep's flipped / transposed / scaled wd (read back as the operand), launch256_main", ["dgrad_wd", "relu_mask"]),
    # bench launch shapes, full M, row-sampled references (16 images)
    case("fwd256_full_m_roi_3x3", "conv_fwd", 3, conv(8192, 14, 14, 512, 512, 3, 1, 1), fwd(True, True, relu=True), {},
         "the bench's (1605632, 512, 4608) RoI-head 3x3, use_gemm256's heuristic, non-temporal stores (1.5 GiB out)", ["fwd256_taps", "full_m"]),
    case("fwd256_full_m_roi_3x3_mask", "conv_fwd", 3, conv(8192, 14, 14, 512, 512, 3, 1, 1), fwd(relu_mask=True), {},
         "its input gradient at full M, use_gemm256's heuristic", ["fwd256_taps", "full_m", "relu_mask"]),
    case("fwd256_full_m_roi_expand", "conv_fwd", 3, conv(8192, 7, 7, 512, 2048), fwd(True, True, "bf16", True), {},
         "the bench's (401408, 2048, 512) res5 expand with residual: persistent form, launch256_main", ["fwd256_persistent", "full_m"]),
    case("fwd256_full_m_res2_expand", "conv_fwd", 3, conv(16, 200, 333, 64, 256), fwd(True, True, "bf16", True), {},
         "the bench's (1065600, 256, 64) res2 expand with residual: persistent, one K-tile, launch256_main", ["fwd256_persistent", "full_m"]),
    case("fwd256_full_m_res4_3x3", "conv_fwd", 3, conv(16, 50, 83, 1024, 1024, 3, 1, 1), fwd(bias=True, relu=True), {},
         "the bench's (66400, 1024, 9216) 3x3: 1 040 tiles, K-split tail, plan_tail_split in launch256", ["fwd256_tail_split", "full_m"]),
    # 32-image geometry: input and output 3.06 GiB, sampled rows past byte 2^31 (per-block buffer bases of tile_epilogue and k_conv_fwd256)
    case("fwd256_over_2gib_roi_3x3", "conv_fwd", 3, conv(16384, 14, 14, 512, 512, 3, 1, 1), fwd(True, True, relu=True), {},
         "32 images' RoI-head 3x3: operands over 2 GiB, use_gemm256's heuristic", ["fwd256_taps", "full_m", "over_2gib"]),
]
# ---- k_conv3x3_small (id 8): plan_fwd's two small-layer branches (3x3; 1x1, 64 outputs); launch_small picks the instantiation by chunks per pixel / Cout
CASES += [
    case("small_1_1", "conv_fwd", 8, conv(2, 37, 53, 8, 32, 3, 2, 1), fwd(True, True, relu=True), {},
         "k_conv3x3_small<bf16, 1, 1>: the stem's padded 3-channel pixel, 32 outputs, stride 2, launch_small", ["small<1,1>"]),
    case("small_1_2", "conv_fwd", 8, conv(1, 40, 61, 8, 64, 3, 1, 1), fwd(True, True, relu=True), {},
         "k_conv3x3_small<bf16, 1, 2>, launch_small", ["small<1,2>"]),
    case("small_8_2", "conv_fwd", 8, conv(2, 37, 53, 64, 64, 3, 1, 1), fwd(True, True, relu=True), {},
         "k_conv3x3_small<bf16, 8, 2>: res2's 64 -> 64 3x3, launch_small", ["small<8,2>"]),
    case("small_8_2_mask", "conv_fwd", 8, conv(1, 50, 83, 64, 64, 3, 1, 1), fwd(relu_mask=True), {},
         "k_conv3x3_small<bf16, 8, 2> input-gradient form, launch_small", ["small<8,2>", "relu_mask"]),
    case("small_4_1", "conv_fwd", 8, conv(3, 21, 30, 32, 32, 3, 1, 1), fwd(True, True, relu=True), {},
         "k_conv3x3_small<bf16, 4, 1>, launch_small", ["small<4,1>"]),
    case("small_4_2", "conv_fwd", 8, conv(3, 21, 30, 32, 64, 3, 1, 1), fwd(True, True, relu=True), {},
         "k_conv3x3_small<bf16, 4, 2>, launch_small", ["small<4,2>"]),
    case("small_8_2_1", "conv_fwd", 8, conv(2, 37, 53, 64, 64), fwd(True, True, relu=True), {},
         "k_conv3x3_small<bf16, 8, 2, 1>: 1x1 64 -> 64, plan_fwd's one-tap branch, launch_small", ["small<8,2,1>"]),
    case("small_32_2_1", "conv_fwd", 8, conv(3, 5, 7, 256, 64), fwd(True, True, relu=True), {},
         "k_conv3x3_small<bf16, 32, 2, 1>: 1x1 256 -> 64, plan_fwd's one-tap branch, launch_small", ["small<32,2,1>"]),
    case("small_full_m_stem2", "conv_fwd", 8, conv(16, 400, 667, 32, 64, 3, 1, 1), fwd(True, True, relu=True), {},
         "the bench's (4268800, 64, 288) stem conv, launch_small", ["small<4,2>", "full_m"]),
]
# ---- weight gradients: cddmsl_conv_wgrad (plan_wgrad chooses kernel and split, run_wgrad / launch_wgrad_split launch)
CASES += [
    case("wgrad256_3x3_ws", "conv_wgrad", 6, conv(9, 14, 14, 256, 256, 3, 1, 1), wg(True, True), F256,
         "k_wgrad256 + k_wgrad_reduce<8, 32>: M = 1764 is 28 reduction tiles, two splits through the workspace, into a non-zero dW, launch_wgrad_split",
         ["wgrad256_ws"]),
    case("wgrad256_3x3_atomics", "conv_wgrad", 6, conv(9, 14, 14, 512, 512, 3, 1, 1), wg(False, True), dict(F256, CDDMSL_WGRAD_WS="0"),
         "k_wgrad256 with f32 atomics (CDDMSL_WGRAD_WS=0: use_workspace), launch_wgrad_split", ["wgrad256_atomics"]),
    case("wgrad256_1x1_ws", "conv_wgrad", 6, conv(4, 40, 37, 256, 512), wg(True, True), F256, "k_wgrad256 1x1, launch_wgrad_split", ["wgrad256_ws"]),
    case("wgrad256_1x1_atomics", "conv_wgrad", 6, conv(2, 9, 11, 256, 512), wg(False, True), dict(F256, CDDMSL_WGRAD_WS="0"),
         "k_wgrad256 1x1, atomics, launch_wgrad_split", ["wgrad256_atomics"]),
    case("wgrad_dma_1x1_ws", "conv_wgrad", 5, conv(4, 40, 37, 128, 192), wg(True, True), F128,
         "k_conv_wgrad_dma<bf16> + k_wgrad_reduce<4, 16>, launch_wgrad_split", ["wgrad_dma"]),
    case("wgrad_dma_1x1_acc", "conv_wgrad", 5, conv(4, 40, 37, 128, 192), wg(False, True), dict(F128, CDDMSL_WGRAD_WS="0"),
         "k_conv_wgrad_dma<bf16> with atomics, launch_wgrad_split", ["wgrad_dma"]),
    case("wgrad_dma_1x1_new", "conv_wgrad", 5, conv(1, 1, 300, 128, 64), wg(), F128,
         "k_conv_wgrad_dma<bf16> into a fresh dW (the mapper's linear layers), launch_wgrad_split", ["wgrad_dma"]),
    case("wgrad_dma_3x3", "conv_wgrad", 5, conv(3, 14, 14, 64, 128, 3, 1, 1), wg(True, True), F128, "k_conv_wgrad_dma<bf16> taps, launch_wgrad_split", ["wgrad_dma"]),
    case("wgrad_s56", "conv_wgrad", 4, conv(37, 1, 56, 128, 136, 1, 56), wg(False, True), {},
         "k_conv_wgrad: the stride-56 1x1 query projection (not 'same' in plan_wgrad), run_wgrad", ["wgrad_s56"]),
    case("wgrad_full_m_s56", "conv_wgrad", 4, conv(8192, 1, 56, 2048, 2048, 1, 56), wg(False, True), {},
         "k_conv_wgrad at the bench's (8192, 2048, 2048) stride-56 launch, plan_wgrad (not 'same')", ["wgrad_s56", "full_m"]),
    case("wgrad256_full_m_roi_3x3", "conv_wgrad", 6, conv(8192, 14, 14, 512, 512, 3, 1, 1), wg(True, True), {},
         "k_wgrad256 at the bench's (1605632, 512, 4608) launch, wgrad256_ok's heuristic", ["wgrad256_ws", "full_m"]),
    case("wgrad256_full_m_res4_3x3", "conv_wgrad", 6, conv(16, 50, 83, 1024, 1024, 3, 1, 1), wg(False, True), {},
         "k_wgrad256 at the bench's (66400, 1024, 9216) launch, wgrad256_ok's heuristic", ["wgrad256_ws", "full_m"]),
    case("wgrad_dma_full_m_res2_3x3", "conv_wgrad", 5, conv(16, 200, 333, 128, 128, 3, 1, 1), wg(True, True), {},
         "k_conv_wgrad_dma at the bench's (1065600, 128, 1152) launch, plan_wgrad, launch_wgrad_split", ["wgrad_dma", "full_m"]),
    case("wgrad256_over_2gib_roi_3x3", "conv_wgrad", 6, conv(16384, 14, 14, 512, 512, 3, 1, 1), wg(True, True), {},
         "32 images' RoI-head 3x3 weight gradient: operands over 2 GiB (wgrad256_span_ok in plan_wgrad)", ["wgrad256_ws", "full_m", "over_2gib"]),
]
# ---- batched entry points (the attention pool): cddmsl_gemm_nt_batched on plan_fwd / run_fwd, cddmsl_gemm_tn_batched on plan_gemm_tn.
# Geometry = the full layout (element strides; a_off / b_off / c_off: element offsets of the operand views, as layers.py passes them).
def nt(M, N, K, batch, lda=None, ldb=None, ldc=None, sa=None, sw=None, sc=None, a_off=0, b_off=0, c_off=0):
    return dict(M=M, N=N, K=K, batch=batch, lda=lda or K, ldb=ldb or K, ldc=ldc or N, sa=sa or M * K, sw=sw or N * K, sc=sc or M * N,
                a_off=a_off, b_off=b_off, c_off=c_off, dtype="bf16")


def tn(M, N, K, batch, lda=None, ldb=None, ldo=None, sa=None, sb=None, so=None, a_off=0, b_off=0, c_off=0):
    return dict(M=M, N=N, K=K, batch=batch, lda=lda or N, ldb=ldb or K, ldo=ldo or K, sa=sa or M * N, sb=sb or M * K, so=so or N * K,
                a_off=a_off, b_off=b_off, c_off=c_off, dtype="bf16")


for out in (False, True):
    s = "_f32" if out else ""
    CASES.append(case(f"nt_128{s}", "gemm_nt_batched", 1, nt(70, 40, 64, 3), dict(bias=False, out_f32=out), F128,
                      "k_conv_fwd over gridDim.y batches, packed operands, plan_fwd's default", ["fwd"]))
    CASES.append(case(f"nt_256{s}", "gemm_nt_batched", 3, nt(300, 256, 64, 2), dict(bias=False, out_f32=out), F256,
                      "k_conv_fwd256 batched (batch > 1: no persistent / split forms), packed operands, plan_fwd (use_gemm256 with the batch count)", ["fwd256_batched"]))
CASES += [
    case("tn_small", "gemm_tn_batched", 9, tn(56, 32, 256, 70), dict(accumulate=False, out="bf16"), {},
         "k_gemm_tn_small<4, 2> (one reduction tile, N <= 64, >= 64 batches), plan_gemm_tn", ["tn_small"]),
    case("tn_small_f32", "gemm_tn_batched", 9, tn(33, 24, 128, 90), dict(accumulate=False, out="f32"), {},
         "k_gemm_tn_small<3, 1> (f32 store, 33-row reduction), plan_gemm_tn", ["tn_small"]),
    case("tn_stream", "gemm_tn_batched", 7, tn(100, 32, 256, 77), dict(accumulate=False, out="bf16"), {},
         "k_gemm_tn_stream<bf16> (two reduction tiles, runs of batches per block), plan_gemm_tn", ["tn_stream"]),
    case("tn_dma_acc", "gemm_tn_batched", 5, tn(1500, 64, 128, 3), dict(accumulate=True, out="f32"), {},
         "k_conv_wgrad_dma<bf16> batched, f32 atomics into a non-zero out, plan_gemm_tn's last branch", ["wgrad_dma"]),
]
# The attention pool's strided layouts at the bench's sizes (layers.py AttnPoolFn, K regions, H = 32 heads, C = 2048, D = 64, TP = 56):
# 16 images = 8192 regions, 32 images = 16384 (operand views reaching 2 and 4 GiB through the per-batch bases)
_ATTN = [  # (id, entry, kid, geometry, epilogue, why)
    ("nt_heads", "gemm_nt_batched", 1, nt(8192, 64, 2048, 32, 65536, 2048, 2048, 2048, 131072, 64), dict(bias=False, out_f32=False),
     "o = Z @ Wv^T per head: A rows H*C apart, k_conv_fwd (64 columns), plan_fwd's default"),
    ("nt_regions", "gemm_nt_batched", 1, nt(32, 56, 2048, 8192, 2048, 2048, 56, 131072, 114688, 1792, a_off=65536), dict(bias=False, out_f32=True),
     "S = U . tok^T per region, U = the second half of zu, f32 out, k_conv_fwd, plan_fwd's default"),
    ("nt_qk", "gemm_nt_batched", 3, nt(8192, 2048, 64, 32, 2048, 2048, 131072, 64, 64, 2048, c_off=65536), dict(bias=False, out_f32=False),
     "U = q0 @ Wk per head into the second half of zu (rows 2*H*C apart), k_conv_fwd256, plan_fwd (use_gemm256 with the batch count)"),
    ("tn_dwv", "gemm_tn_batched", 5, tn(8192, 64, 2048, 32, 2048, 65536, 2048, 64, 2048, 131072), dict(accumulate=True, out="f32"),
     "dWv += dO^T Z per head: f32 atomics, B rows H*C apart, k_conv_wgrad_dma, plan_gemm_tn's last branch"),
    ("tn_z", "gemm_tn_batched", 9, tn(56, 32, 2048, 8192, 32, 2048, 2048, 1792, 114688, 65536), dict(accumulate=False, out="bf16"),
     "Z = P^T tok per region: k_gemm_tn_small<4, 2>, 32 batches per block, plan_gemm_tn"),
]
for id_, entry, kid, geom, epi, why in _ATTN:
    CASES.append(case(id_, entry, kid, geom, epi, {}, why + " (the bench's 16-image launch)",
                      ["full_m", "batched_strided"] + (["tn_small"] if kid == 9 else [])))
    big = dict(geom, M=16384) if geom["batch"] == 32 else dict(geom, batch=16384)
    CASES.append(case(id_ + "_32img", entry, kid, big, epi, {}, why + " (32 images: operands past 2 GiB)",
                      ["full_m", "batched_strided", "over_2gib"]))
CASES.append(case("nt_mapper", "gemm_nt_batched", 3, nt(544, 1024, 1920, 16, 30720, 30720, 1024, 1920, 1920, 557056),
                  dict(bias=False, out_f32=True), {}, "the mapper's per-head product (A, B rows 30720 apart), k_conv_fwd256, plan_fwd (use_gemm256 with the batch count)",
                  ["batched_strided"]))

# ---- the stock ResNet-50 path (cddmsl_amd/modeling/resnet.py): the stride lives in the first 1x1 of a block and in its shortcut, the stem
# is a 7x7 stride-2 pad-3 convolution.  plan_fwd puts no condition on the stride, so a stride-2 1x1 lands on every forward GEMM kernel
# by size; each of them addresses a tile from a per-block base plus lane offsets, and with stride 2 in H and W a tile's rows skip every
# other pixel and every other image row.  Odd and even maps ((H - 1) // 2 + 1 floors or not), two images and more (an image boundary
# inside a tile), more than one row tile.  tests/golden/stock_gemm_launches.json records which of these the stock step launches.
_BN, _BN_RELU = _FWD_SETS_1X1["bn"], _FWD_SETS_1X1["bn_relu"]
CASES += [
    case("stem_7x7_s2_bf16", "conv_fwd", 1, conv(2, 37, 53, 8, 64, 7, 2, 3), _BN_RELU, {},
         "k_conv_fwd on BasicStem's 7x7 stride 2 pad 3, one 16-byte chunk per pixel (all 8 channels non-zero here): 49 taps are above the "
         "31 of gemm256_legal / fwd2_legal and 64 outputs no whole 128 columns, plan_fwd's default", ["stem_7x7_s2", "fwd"]),
    case("stem_7x7_s2_bf16_even", "conv_fwd", 1, conv(2, 38, 54, 8, 64, 7, 2, 3), _BN_RELU, {},
         "k_conv_fwd, the stem on an even map (the last tap row and column lie in the padding), plan_fwd's default", ["stem_7x7_s2", "fwd"]),
    case("stem_7x7_s2_f32", "conv_fwd", 1, dict(conv(2, 37, 53, 4, 64, 7, 2, 3), dtype="f32"), _BN_RELU, {},
         "k_conv_fwd<float> on the stem (4 f32 channels are one chunk), plan_fwd's default", ["stem_7x7_s2", "fwd_f32"]),
    case("stem_7x7_s2_f32_even", "conv_fwd", 1, dict(conv(2, 38, 54, 4, 64, 7, 2, 3), dtype="f32"), _BN_RELU, {},
         "k_conv_fwd<float> on the stem, even map, plan_fwd's default", ["stem_7x7_s2", "fwd_f32"]),
    case("fwd_1x1_s2_bn_relu", "conv_fwd", 1, conv(2, 9, 37, 64, 136, 1, 2), _BN_RELU, F128,
         "k_conv_fwd 1x1 stride 2 (conv1 of a stock block): 190 rows are two tiles, the image boundary inside the first; plan_fwd's default", ["fwd_1x1_s2"]),
    case("fwd_1x1_s2_bn", "conv_fwd", 1, conv(2, 9, 37, 64, 136, 1, 2), _BN, F128,
         "k_conv_fwd 1x1 stride 2 without ReLU (the shortcut of a stock block), plan_fwd's default", ["fwd_1x1_s2"]),
    case("fwd_1x1_s2_bn_relu_even", "conv_fwd", 1, conv(2, 10, 38, 64, 136, 1, 2), _BN_RELU, F128,
         "k_conv_fwd 1x1 stride 2 on an even map: the last row and column are never read; plan_fwd's default", ["fwd_1x1_s2"]),
    case("fwd_1x1_s2_bn_even", "conv_fwd", 1, conv(2, 10, 38, 64, 136, 1, 2), _BN, F128,
         "k_conv_fwd 1x1 stride 2, shortcut epilogue, even map; plan_fwd's default", ["fwd_1x1_s2"]),
    case("fwd2_1x1_s2_bn_relu", "conv_fwd", 11, conv(3, 19, 23, 96, 384, 1, 2), _BN_RELU, FWD2,
         "k_conv_fwd2<bf16, false, 0> 1x1 stride 2 (stride is legal there: fwd2_legal): 360 rows are two row tiles, two image boundaries "
         "inside the first; launch_fwd2", ["fwd2_1x1_s2"]),
    case("fwd2_1x1_s2_bn_even", "conv_fwd", 11, conv(3, 20, 24, 96, 384, 1, 2), _BN, FWD2,
         "k_conv_fwd2 1x1 stride 2, shortcut epilogue, even map; launch_fwd2", ["fwd2_1x1_s2"]),
    case("fwd256_1x1_s2_bn_relu", "conv_fwd", 3, conv(3, 19, 23, 128, 512, 1, 2), _BN_RELU, F256,
         "k_conv_fwd256<bf16, false, false, 0> 1x1 stride 2, the plain tile form (4 tiles): two row panels, image boundaries inside the "
         "first; launch256_main", ["fwd256_1x1_s2"]),
    case("fwd256_1x1_s2_bn_even", "conv_fwd", 3, conv(3, 20, 24, 128, 512, 1, 2), _BN, F256,
         "k_conv_fwd256 1x1 stride 2, shortcut epilogue, even map; launch256_main", ["fwd256_1x1_s2"]),
    case("fwd256_roi_crops_s2", "conv_fwd", 3, conv(37, 14, 14, 256, 512, 1, 2), _BN_RELU, F256,
         "k_conv_fwd256 on the RoI head's geometry, 14 x 14 crops to 7 x 7: 49 rows per crop, a 256-row tile spans more than five crops; "
         "launch256_main", ["fwd256_1x1_s2"]),
    case("fwd256_persistent_s2", "conv_fwd", 3, conv(2, 181, 181, 128, 1024, 1, 2), _BN_RELU, F256,
         "persistent form under stride 2 (K = 128 <= 512; 2 x 91 x 91 = 16 562 rows are 65 panels, 260 tiles > 256 CUs, the ragged last panel "
         "in the second round): launch256_main's persistent form", ["fwd256_persistent_s2", "fwd256_persistent"]),
    case("fwd256_persistent_s2_bn", "conv_fwd", 3, conv(2, 181, 181, 128, 1024, 1, 2), _BN, F256,
         "persistent form under stride 2, shortcut epilogue: launch256_main", ["fwd256_persistent_s2", "fwd256_persistent"]),
    case("fwd256_tail_split_s2", "conv_fwd", 3, conv(169, 14, 14, 1024, 2048, 1, 2), _BN, dict(F256, CDDMSL_TAIL_SPLIT="1"),
         "K-split tail under stride 2 at Res5ROIHeads' 1024 -> 2048 shortcut on 14 x 14 crops (8 281 rows are 33 panels, 264 tiles on 256 "
         "CUs, 16 K-tiles in 8 slices) + k_conv_split_reduce: plan_tail_split in launch256", ["fwd256_tail_split_s2", "fwd256_tail_split"]),
    case("wgrad_1x1_s2", "conv_wgrad", 4, conv(4, 41, 37, 128, 192, 1, 2), wg(True, True), {},
         "k_conv_wgrad 1x1 stride 2 with the FrozenBN scale into a non-zero dW (conv1 / shortcut of a stock block; not 'same' in plan_wgrad), "
         "odd map: 4 x 21 x 19 rows; run_wgrad", ["wgrad_1x1_s2"]),
    case("wgrad_1x1_s2_even", "conv_wgrad", 4, conv(4, 40, 38, 128, 192, 1, 2), wg(True, True), {},
         "k_conv_wgrad 1x1 stride 2, even map (the last row and column are never read), plan_wgrad (not 'same')", ["wgrad_1x1_s2"]),
    case("wgrad_1x1_s2_one_row", "conv_wgrad", 4, conv(1, 1, 37, 128, 192, 1, 2), wg(True, True), {},
         "k_conv_wgrad 1x1 stride 2, degenerate: one image of one row, 19 output pixels (Ho == Hi, Wo != Wi: still not 'same'), plan_wgrad",
         ["wgrad_1x1_s2"]),
]

# ---- what the stock step's record (tests/golden/stock_gemm_launches.json) holds beyond the strided convolutions
CASES += [
    case("nt_rpn_sparse_dx", "gemm_nt_batched", 3, dict(nt(4096, 1024, 1024, 9, 1024, 9216, 1024, None, 1024, 4194304), sa=0),
         dict(bias=False, out_f32=True), {},
         "the RPN head's sparse input gradient (layers.py RpnHeadFn.backward): one product per filter tap, the 4 096 gathered rows shared by "
         "all nine (sa = 0), B the tap's 1 024 columns of rows 9 216 apart, f32 out; k_conv_fwd256, plan_fwd (use_gemm256 with the batch "
         "count) (the stock step's 16-image launch)", ["batched_strided", "nt_shared_a"]),
]
N_BF16_TABLE = len(CASES)          # the cases above keep their place: a case's seed is its index (tests/test_gpu_gemm_exact.py)

# ================================================================================================ f32 operands
# The f32 instantiations are their own index math -- 4 elements per 16-byte chunk, a 32-element K-tile, Mma<float>'s k-to-lane layout
# (four 32x32x2f32 steps per chunk), TrFrag<float> / TrFragS<float> in the weight gradient, 64x64 weight-gradient tiles that only ever
# finish with atomics, b32 mask loads and stores in the epilogues -- and every oracle-parity step runs on them.  One case per
# instantiation and epilogue set, each at the smallest shape that still has a ragged last tile in M and N, a reduction that ends
# inside a K-tile where the kernel allows one (Cin 36 = 9 chunks, a K-tile holds 8) and, for the strided cases, an image boundary
# inside a tile.  Residuals and masks of an f32 launch are f32; its output is f32 without the out_f32 flag.
# tests/golden/bench_gemm_launches_f32.json and stock_gemm_launches_f32.json record which classes the f32 steps launch.


def conv32(*a, **k):
    return dict(conv(*a, **k), dtype="f32")


_F32_SETS = {k: dict(_FWD_SETS_1X1[k], residual="f32" if _FWD_SETS_1X1[k]["residual"] else None)
             for k in ("plain", "bn", "bn_relu", "bias_relu", "bn_res_relu", "res", "mask", "mask_res")}
_BN32, _BN_RELU32, _MASK32 = _F32_SETS["bn"], _F32_SETS["bn_relu"], _F32_SETS["mask"]


def _tags(k, *base):
    return list(base) + (["relu_mask_f32"] if "mask" in k else [])


# ---- k_conv_fwd<float> (id 1), plan_fwd's default
for k, e in _F32_SETS.items():
    CASES.append(case(f"f32_fwd_1x1_{k}", "conv_fwd", 1, conv32(2, 9, 37, 36, 136), e, F128,
                      "k_conv_fwd<float> 1x1, 666 x 136 outputs, K = 36 is 9 chunks: the second K-tile holds one; plan_fwd's default",
                      _tags(k, "fwd_f32", "fwd_f32_ragged_k")))
CASES += [
    case("f32_fwd_3x3_bn_relu", "conv_fwd", 1, conv32(2, 9, 13, 32, 96, 3, 1, 1), _BN_RELU32, F128,
         "k_conv_fwd<float> taps: 32 channels are one K-tile per tap, plan_fwd's default", ["fwd_f32_taps"]),
    case("f32_fwd_3x3_mask", "conv_fwd", 1, conv32(2, 9, 13, 32, 96, 3, 1, 1), _MASK32, F128,
         "k_conv_fwd<float> taps, ReLU-mask input gradient (b32 mask loads), plan_fwd's default", ["fwd_f32_taps", "relu_mask_f32"]),
    case("f32_fwd_1x1_s2_bn_relu", "conv_fwd", 1, conv32(2, 9, 37, 32, 136, 1, 2), _BN_RELU32, F128,
         "k_conv_fwd<float> 1x1 stride 2 (conv1 of a stock block): 190 rows are two tiles, the image boundary inside the first; plan_fwd's default",
         ["fwd_1x1_s2_f32"]),
    case("f32_fwd_1x1_s2_bn", "conv_fwd", 1, conv32(2, 9, 37, 32, 136, 1, 2), _BN32, F128,
         "k_conv_fwd<float> 1x1 stride 2, the shortcut's epilogue, plan_fwd's default", ["fwd_1x1_s2_f32"]),
    case("f32_fwd_1x1_s2_bn_relu_even", "conv_fwd", 1, conv32(2, 10, 38, 32, 136, 1, 2), _BN_RELU32, F128,
         "k_conv_fwd<float> 1x1 stride 2 on an even map: the last row and column are never read; plan_fwd's default", ["fwd_1x1_s2_f32"]),
    case("f32_fwd_1x1_s2_bn_even", "conv_fwd", 1, conv32(2, 10, 38, 32, 136, 1, 2), _BN32, F128,
         "k_conv_fwd<float> 1x1 stride 2, shortcut epilogue, even map; plan_fwd's default", ["fwd_1x1_s2_f32"]),
    case("f32_fwd_s56_bias", "conv_fwd", 1, conv32(37, 1, 56, 64, 136, 1, 56), fwd(bias=True), F128,
         "k_conv_fwd<float>, the attention pool's strided query projection (one row of every 56), plan_fwd's default", ["fwd_f32_s56"]),
    case("f32_fwd_1x1_64_not_small", "conv_fwd", 1, conv32(2, 37, 53, 32, 64), _BN_RELU32, {},
         "k_conv_fwd<float>: plan_fwd's one-tap branch to k_conv3x3_small is bf16 only (op == OP_BF16), so the f32 1x1 with 64 outputs "
         "stays on plan_fwd's default -- a change of that rule shows here", ["fwd_f32_one_tap_rule"]),
    # ---- k_conv_fwd_reg<float> (id 2)
    case("f32_fwd_reg_pool", "conv_fwd", 2, conv32(2, 15, 21, 32, 160, pool=True), _F32_SETS["plain"], F128,
         "k_conv_fwd_reg<float>: AvgPool2d(2) fused into the loader, odd sizes floor, plan_fwd (pool)", ["fwd_reg_pool_f32"]),
    case("f32_fwd_reg_pool_bn_relu", "conv_fwd", 2, conv32(3, 14, 14, 64, 256, pool=True), _BN_RELU32, {},
         "k_conv_fwd_reg<float> (pool is never legal on the 256 kernels: gemm256_legal), plan_fwd (pool)", ["fwd_reg_pool_f32"]),
]
# ---- k_conv_fwd256<float, TAPS, false, -1> (id 3): use_gemm256 in plan_fwd; launch256 gives f32 operands EPI -1
for k, e in _F32_SETS.items():
    CASES.append(case(f"f32_fwd256_1x1_{k}", "conv_fwd", 3, conv32(2, 19, 23, 64, 512), e, F256,
                      "k_conv_fwd256<float, false, false, -1>: 874 rows are four row panels, the last ragged; two K-tiles; launch256_main",
                      _tags(k, "fwd256_1x1_f32")))
CASES += [
    case("f32_fwd256_3x3_bn_relu", "conv_fwd", 3, conv32(2, 19, 23, 32, 256, 3, 1, 1), _BN_RELU32, F256,
         "k_conv_fwd256<float, true, false, -1>, launch256_main", ["fwd256_taps_f32"]),
    case("f32_fwd256_3x3_mask", "conv_fwd", 3, conv32(2, 19, 23, 32, 256, 3, 1, 1), _MASK32, F256,
         "k_conv_fwd256<float, true, false, -1>, ReLU-mask input gradient, launch256_main", ["fwd256_taps_f32", "relu_mask_f32"]),
    case("f32_fwd256_1x1_s2_bn_relu", "conv_fwd", 3, conv32(3, 19, 23, 64, 512, 1, 2), _BN_RELU32, F256,
         "k_conv_fwd256<float, false, false, -1> 1x1 stride 2: 360 rows are two row panels, image boundaries inside the first; launch256_main",
         ["fwd256_1x1_s2_f32"]),
    case("f32_fwd256_1x1_s2_bn_even", "conv_fwd", 3, conv32(3, 20, 24, 64, 512, 1, 2), _BN32, F256,
         "k_conv_fwd256<float> 1x1 stride 2, shortcut epilogue, even map; launch256_main", ["fwd256_1x1_s2_f32"]),
    case("f32_fwd256_res_pool", "conv_fwd", 3, conv32(3, 15, 21, 64, 256), fwd(residual="pooled"), F256,
         "k_conv_fwd256<float, false, true>: AvgPool2d(2)-backward residual (f32), odd sizes, launch_fwd (res_pool)", ["fwd256_res_pool_f32"]),
    case("f32_fwd256_res_pool_mask", "conv_fwd", 3, conv32(3, 15, 21, 64, 256), fwd(residual="pooled", relu_mask=True), F256,
         "k_conv_fwd256<float, false, true> with the ReLU mask, launch_fwd (res_pool)", ["fwd256_res_pool_f32", "relu_mask_f32"]),
]
# ---- k_conv_fwd2<float, TAPS, -1> (id 11): use_fwd2 in plan_fwd; launch_fwd2
for k in ("plain", "bn_relu", "mask"):
    CASES.append(case(f"f32_fwd2_1x1_{k}", "conv_fwd", 11, conv32(2, 19, 23, 48, 384), _F32_SETS[k], FWD2,
                      "k_conv_fwd2<float, false, -1>: K = 48 is 12 chunks, three K-tiles of 4; launch_fwd2", _tags(k, "fwd2_1x1_f32")))
for k in ("bn_relu", "mask"):
    CASES.append(case(f"f32_fwd2_3x3_{k}", "conv_fwd", 11, conv32(2, 19, 23, 16, 128, 3, 1, 1), _F32_SETS[k], FWD2,
                      "k_conv_fwd2<float, true, -1>: one K-tile per tap, launch_fwd2", _tags(k, "fwd2_taps_f32")))
CASES.append(case("f32_fwd2_1x1_s2_bn", "conv_fwd", 11, conv32(3, 19, 23, 48, 384, 1, 2), _BN32, FWD2,
                  "k_conv_fwd2<float, false, -1> 1x1 stride 2: 360 rows are two row tiles, two image boundaries inside the first; launch_fwd2",
                  ["fwd2_1x1_s2_f32"]))
# ---- k_conv3x3_small<float, CPP, NB> (id 8): plan_fwd's 3x3 branch (its one-tap branch is bf16 only: f32_fwd_1x1_64_not_small above);
# launch_small picks the instantiation by chunks per pixel / Cout.  A chunk is 4 f32 channels: <4,.> is 16 channels, <8,2> is 32.
CASES += [
    case("f32_small_1_1", "conv_fwd", 8, conv32(2, 37, 53, 4, 32, 3, 2, 1), _BN_RELU32, {},
         "k_conv3x3_small<float, 1, 1>: one chunk per pixel, 32 outputs, stride 2, launch_small", ["small_f32<1,1>"]),
    case("f32_small_1_2", "conv_fwd", 8, conv32(1, 40, 61, 4, 64, 3, 1, 1), _BN_RELU32, {},
         "k_conv3x3_small<float, 1, 2>, launch_small", ["small_f32<1,2>"]),
    case("f32_small_4_1", "conv_fwd", 8, conv32(3, 21, 30, 16, 32, 3, 1, 1), _BN_RELU32, {},
         "k_conv3x3_small<float, 4, 1>, launch_small", ["small_f32<4,1>"]),
    case("f32_small_4_2", "conv_fwd", 8, conv32(3, 21, 30, 16, 64, 3, 1, 1), _BN_RELU32, {},
         "k_conv3x3_small<float, 4, 2>, launch_small", ["small_f32<4,2>"]),
    case("f32_small_8_2", "conv_fwd", 8, conv32(2, 37, 53, 32, 64, 3, 1, 1), _BN_RELU32, {},
         "k_conv3x3_small<float, 8, 2>: 32 -> 64 3x3, launch_small", ["small_f32<8,2>"]),
    case("f32_small_8_2_mask", "conv_fwd", 8, conv32(1, 50, 83, 32, 64, 3, 1, 1), _MASK32, {},
         "k_conv3x3_small<float, 8, 2> input-gradient form, launch_small", ["small_f32<8,2>_mask", "relu_mask_f32"]),
]
# ---- weight gradients: f32 operands take 64x64 tiles and always finish with f32 atomics (launch_wgrad); k_wgrad256 is bf16 only
CASES += [
    case("f32_wgrad_dma_1x1_acc", "conv_wgrad", 5, conv32(4, 40, 37, 64, 96), wg(True, True), F128,
         "k_conv_wgrad_dma<float>: 64x64 tiles (Cout 96: a ragged second), atomics, scale, into a non-zero dW; plan_wgrad, launch_wgrad",
         ["wgrad_dma_f32"]),
    case("f32_wgrad_dma_1x1_new", "conv_wgrad", 5, conv32(4, 40, 37, 64, 96), wg(), F128,
         "k_conv_wgrad_dma<float> into a fresh dW, plan_wgrad, launch_wgrad", ["wgrad_dma_f32_new"]),
    case("f32_wgrad_dma_3x3", "conv_wgrad", 5, conv32(3, 14, 14, 32, 64, 3, 1, 1), wg(True, True), F128,
         "k_conv_wgrad_dma<float> taps, plan_wgrad, launch_wgrad", ["wgrad_dma_f32_taps"]),
    case("f32_wgrad_dma_under_f256", "conv_wgrad", 5, conv32(4, 40, 37, 256, 512), wg(True, True), F256,
         "k_conv_wgrad_dma<float> where bf16 takes k_wgrad256 (wgrad256_ok: bf16 only, so CDDMSL_GEMM256=2 must not move it); plan_wgrad",
         ["wgrad_f32_not_256"]),
    case("f32_wgrad_1x1_s2", "conv_wgrad", 4, conv32(4, 41, 37, 64, 96, 1, 2), wg(True, True), {},
         "k_conv_wgrad<float> 1x1 stride 2 with the FrozenBN scale into a non-zero dW (not 'same' in plan_wgrad), odd map: 4 x 21 x 19 rows; "
         "run_wgrad", ["wgrad_1x1_s2_f32"]),
    case("f32_wgrad_1x1_s2_even", "conv_wgrad", 4, conv32(4, 40, 38, 64, 96, 1, 2), wg(True, True), {},
         "k_conv_wgrad<float> 1x1 stride 2, even map (the last row and column are never read), plan_wgrad (not 'same')", ["wgrad_1x1_s2_f32_even"]),
    case("f32_wgrad_1x1_s2_one_row", "conv_wgrad", 4, conv32(1, 1, 37, 64, 96, 1, 2), wg(True, True), {},
         "k_conv_wgrad<float> 1x1 stride 2, degenerate: one image of one row, 19 output pixels, plan_wgrad", ["wgrad_1x1_s2_f32_one_row"]),
    case("f32_wgrad_s56", "conv_wgrad", 4, conv32(37, 1, 56, 64, 136, 1, 56), wg(False, True), {},
         "k_conv_wgrad<float>: the stride-56 1x1 query projection (not 'same' in plan_wgrad), run_wgrad", ["wgrad_s56_f32"]),
]
# ---- batched products on f32 operands (f32 stores: the out_f32 flag is for bf16 operands)
_NT32 = dict(bias=False, out_f32=False)
CASES += [
    case("f32_nt_128", "gemm_nt_batched", 1, dict(nt(70, 40, 32, 3), dtype="f32"), _NT32, F128,
         "k_conv_fwd<float> over gridDim.y batches, packed operands, plan_fwd's default", ["nt_f32"]),
    case("f32_nt_256", "gemm_nt_batched", 3, dict(nt(300, 256, 32, 2), dtype="f32"), _NT32, F256,
         "k_conv_fwd256<float> batched, packed operands, plan_fwd (use_gemm256 with the batch count)", ["fwd256_batched_f32"]),
    case("f32_nt_regions", "gemm_nt_batched", 1, dict(nt(32, 56, 64, 5, sa=4096, sw=3584, sc=1792, a_off=2048), dtype="f32"), _NT32, {},
         "k_conv_fwd<float> on the attention pool's per-region layout: A the second half of a two-part buffer (batches 2 * M * K apart, "
         "operand offset M * K), plan_fwd's default", ["nt_f32_strided"]),
    case("f32_nt_shared_a", "gemm_nt_batched", 1, dict(nt(70, 40, 32, 9, ldb=288, sw=32), sa=0, dtype="f32"), _NT32, {},
         "k_conv_fwd<float> on the RPN head's sparse input-gradient layout: one A for all nine batches (sa = 0), B the tap's 32 columns of "
         "rows 288 apart, plan_fwd's default", ["nt_f32_shared_a"]),
    case("f32_tn_stream", "gemm_tn_batched", 7, dict(tn(56, 32, 256, 70), dtype="f32"), dict(accumulate=False, out="f32"), {},
         "k_gemm_tn_stream<float> where bf16 takes k_gemm_tn_small (bf16 only): one reduction tile, 70 batches, plan_gemm_tn", ["tn_stream_f32"]),
    case("f32_tn_stream_2", "gemm_tn_batched", 7, dict(tn(100, 32, 128, 77), dtype="f32"), dict(accumulate=False, out="f32"), {},
         "k_gemm_tn_stream<float>, two reduction tiles, runs of batches per block, plan_gemm_tn", ["tn_stream_f32_two_tiles"]),
    case("f32_tn_dma_acc", "gemm_tn_batched", 5, dict(tn(700, 64, 96, 3), dtype="f32"), dict(accumulate=True, out="f32"), {},
         "k_conv_wgrad_dma<float> batched, f32 atomics into a non-zero out, plan_gemm_tn's last branch", ["wgrad_dma_f32_batched"]),
]
# ---- what the f32 records hold beyond the instantiations above (bench_gemm_launches_f32.json, stock_gemm_launches_f32.json: the records
# decide): epilogue sets -- the out_f32 flag on f32 operands (layers.linear(..., out_f32=True) passes it in either dtype; the store is
# f32 anyway), a pooled residual on the 128x128 kernel (too few tiles for use_gemm256 on one image), the bottleneck's residual sets on
# k_conv_fwd2, a weight gradient accumulated without a scale -- a store-mode k_conv_wgrad_dma<float> product (fewer than 64 batches),
# and the attention pool's, the mapper's and the RPN head's strided layouts, which only a case with the same strides covers
# (batched_layout), at the one-image sizes recorded: 34 regions, 32 heads, 256 gathered rows.
_SETS32_MORE = {"f32": fwd(out_f32=True), "bias_f32": fwd(bias=True, out_f32=True), "bias_relu_f32": fwd(bias=True, relu=True, out_f32=True)}
for k, e in _SETS32_MORE.items():
    CASES.append(case(f"f32_fwd_1x1_{k}", "conv_fwd", 1, conv32(2, 9, 37, 36, 136), e, F128,
                      "k_conv_fwd<float> 1x1 with the out_f32 flag set on f32 operands (heads and linear layers), plan_fwd's default",
                      ["f32_recorded", "fwd_f32_out_flag"]))
CASES += [
    case("f32_fwd_3x3_bias_relu", "conv_fwd", 1, conv32(2, 9, 13, 32, 96, 3, 1, 1), _F32_SETS["bias_relu"], F128,
         "k_conv_fwd<float> taps, the RPN head's 3x3 epilogue (bias, ReLU, no scale), plan_fwd's default", ["f32_recorded", "fwd_f32_taps"]),
    case("f32_fwd_res_pool", "conv_fwd", 1, conv32(3, 15, 21, 36, 136), fwd(residual="pooled"), F128,
         "k_conv_fwd<float> with the AvgPool2d(2)-backward residual (res_pool is legal on the 128x128 kernel; not on k_conv_fwd2: fwd2_legal), "
         "odd sizes, plan_fwd's default", ["f32_recorded", "fwd_res_pool_f32"]),
]
for k in ("bn", "bn_res_relu", "mask_res"):
    CASES.append(case(f"f32_fwd2_1x1_{k}", "conv_fwd", 11, conv32(2, 19, 23, 48, 384), _F32_SETS[k], FWD2,
                      "k_conv_fwd2<float, false, -1> under a bottleneck's residual / shortcut epilogues, launch_fwd2",
                      _tags(k, "f32_recorded", "fwd2_1x1_f32")))
CASES += [
    case("f32_wgrad_dma_1x1_acc_noscale", "conv_wgrad", 5, conv32(4, 40, 37, 64, 96), wg(False, True), F128,
         "k_conv_wgrad_dma<float> into a non-zero dW without a scale (linear layers), plan_wgrad, launch_wgrad", ["f32_recorded", "wgrad_dma_f32_noscale"]),
    case("f32_tn_dma_store", "gemm_tn_batched", 5, dict(tn(56, 32, 96, 34), dtype="f32"), dict(accumulate=False, out="f32"), {},
         "k_conv_wgrad_dma<float> batched in store mode (fewer than 64 batches: neither k_gemm_tn_small nor k_gemm_tn_stream), one block "
         "per 64x64 tile, ragged in N and K, plan_gemm_tn's last branch", ["f32_recorded", "tn_dma_store_f32"]),
]
_ATTN32 = [  # (id, entry, kid, geometry, epilogue, why): the layouts of _ATTN, nt_mapper and nt_rpn_sparse_dx at the f32 records' one-image sizes
    ("f32_nt_heads", "gemm_nt_batched", 1, nt(34, 64, 2048, 32, 65536, 2048, 2048, 2048, 131072, 64), _NT32,
     "o = Z @ Wv^T per head: A rows H*C apart, k_conv_fwd<float> (64 columns), plan_fwd's default"),
    ("f32_nt_regions_full", "gemm_nt_batched", 1, nt(32, 56, 2048, 34, 2048, 2048, 56, 131072, 114688, 1792, a_off=65536), _NT32,
     "S = U . tok^T per region, U = the second half of zu, k_conv_fwd<float>, plan_fwd's default"),
    ("f32_nt_qk", "gemm_nt_batched", 3, nt(34, 2048, 64, 32, 2048, 2048, 131072, 64, 64, 2048, c_off=65536), _NT32,
     "U = q0 @ Wk per head into the second half of zu (rows 2*H*C apart): 34 rows of a 256-row tile, k_conv_fwd256<float>, plan_fwd "
     "(use_gemm256 with the batch count)"),
    ("f32_tn_dwv", "gemm_tn_batched", 5, tn(34, 64, 2048, 32, 2048, 65536, 2048, 64, 2048, 131072), dict(accumulate=True, out="f32"),
     "dWv += dO^T Z per head: f32 atomics, B rows H*C apart, k_conv_wgrad_dma<float>, plan_gemm_tn's last branch"),
    ("f32_nt_mapper", "gemm_nt_batched", 1, nt(34, 1024, 1920, 16, 30720, 30720, 1024, 1920, 1920, 34816), _NT32,
     "the mapper's per-head product (A, B rows 30720 apart): too few 256x256 tiles on one image, k_conv_fwd<float>, plan_fwd's default"),
    ("f32_nt_rpn_sparse_dx", "gemm_nt_batched", 1, dict(nt(256, 1024, 1024, 9, 1024, 9216, 1024, None, 1024, 262144), sa=0), _NT32,
     "the RPN head's sparse input gradient: 256 gathered rows shared by the nine taps (sa = 0), B the tap's 1 024 columns of rows 9 216 "
     "apart; k_conv_fwd<float>, plan_fwd's default"),
]
for id_, entry, kid, geom, epi, why in _ATTN32:
    CASES.append(case(id_, entry, kid, dict(geom, dtype="f32"), epi, {}, why + " (the f32 step's one-image launch)", ["f32_recorded", "batched_strided_f32"]))

REQUIRED_VARIANTS = [
    "fwd", "fwd_reg_pool", "fwd2_1x1", "fwd2_taps", "fwd256_1x1", "fwd256_taps", "fwd256_res_pool", "fwd256_persistent",
    "fwd256_tail_split", "fwd256_batched", "fwd256_res_f32", "fwd256_out_f32", "small<1,1>", "small<1,2>", "small<8,2>", "small<4,1>",
    "small<4,2>", "small<8,2,1>", "small<32,2,1>", "wgrad256_ws", "wgrad256_atomics", "wgrad_dma", "wgrad_s56", "tn_small", "tn_stream",
    "relu_mask", "dgrad_wd", "full_m", "over_2gib", "batched_strided", "fwd_f32",
    "stem_7x7_s2", "fwd_1x1_s2", "fwd2_1x1_s2", "fwd256_1x1_s2", "fwd256_persistent_s2", "fwd256_tail_split_s2", "wgrad_1x1_s2", "nt_shared_a",
    # the f32 instantiations (and what only f32 dispatch does: the one-tap rule, no k_wgrad256, no k_gemm_tn_small)
    "fwd_f32_ragged_k", "fwd_f32_taps", "fwd_1x1_s2_f32", "fwd_f32_s56", "fwd_f32_one_tap_rule", "fwd_reg_pool_f32", "fwd256_1x1_f32",
    "fwd256_taps_f32", "fwd256_1x1_s2_f32", "fwd256_res_pool_f32", "fwd2_1x1_f32", "fwd2_taps_f32", "fwd2_1x1_s2_f32", "small_f32<1,1>",
    "small_f32<1,2>", "small_f32<4,1>", "small_f32<4,2>", "small_f32<8,2>", "small_f32<8,2>_mask", "relu_mask_f32", "wgrad_dma_f32",
    "wgrad_dma_f32_new", "wgrad_dma_f32_taps", "wgrad_f32_not_256", "wgrad_1x1_s2_f32", "wgrad_1x1_s2_f32_even", "wgrad_1x1_s2_f32_one_row",
    "wgrad_s56_f32", "nt_f32", "fwd256_batched_f32", "nt_f32_strided", "nt_f32_shared_a", "tn_stream_f32", "tn_stream_f32_two_tiles",
    "wgrad_dma_f32_batched",
    # what the f32 records added
    "f32_recorded", "fwd_f32_out_flag", "fwd_res_pool_f32", "wgrad_dma_f32_noscale", "tn_dma_store_f32", "batched_strided_f32",
]
# (kernel id, M, N, K) bench launches the issue names: each has a full-M case
BENCH_SHAPES = [(3, 1605632, 512, 4608), (3, 401408, 2048, 512), (3, 1065600, 256, 64), (3, 66400, 1024, 9216), (11, 1065600, 128, 1152),
                (8, 4268800, 64, 288), (9, 56, 32, 2048)]
# kernels the bench launches: each has at least one case at a bench launch shape with its full M
BENCH_KERNELS = {1, 3, 4, 5, 6, 8, 9, 11}


def mnk(c):
    """(M, N, K) of a convolution case as the profiler counts them (output rows, output channels, reduction length)"""
    g = c["geom"]
    if "H" not in g:
        return (g["M"], g["N"], g["K"])
    if g["pool"]:
        Ho, Wo = g["H"] // 2, g["W"] // 2
    else:
        Ho, Wo = (g["H"] + 2 * g["pad"] - g["KH"]) // g["stride"] + 1, (g["W"] + 2 * g["pad"] - g["KW"]) // g["stride"] + 1
    return (g["N"] * Ho * Wo, g["Cout"], g["KH"] * g["KW"] * g["Cin"])


def batched_layout(entry, geom):
    """'packed' when every operand of a batched call is dense and batch after batch, else the strides themselves (element units) --
    a strided layout is only covered by a case with the same strides"""
    if entry == "gemm_nt_batched":
        M, N, K = geom["M"], geom["N"], geom["K"]
        st = (geom["lda"], geom["ldb"], geom["ldc"], geom["sa"], geom["sw"], geom["sc"])
        packed = st == (K, K, N, M * K, N * K, M * N)
    else:
        M, N, K = geom["M"], geom["N"], geom["K"]
        st = (geom["lda"], geom["ldb"], geom["ldo"], geom["sa"], geom["sb"], geom["so"])
        packed = st == (N, K, K, M * N, M * K, N * K)
    return ("packed",) if packed else ("strided",) + st


def launch_class(entry, kid, geom, epi):
    """what the coverage check groups launches by: entry point, kernel id, operand dtype, geometry class (taps or 1x1, strided,
    pooled; for the batched entry points the layout) and the set of epilogue flags"""
    flags = tuple(sorted(k if v is True else f"{k}={v}" for k, v in epi.items() if v))
    if "H" in geom:
        geo = ("taps" if geom["KH"] * geom["KW"] > 1 else "1x1", "strided" if geom["stride"] > 1 else "", "pool" if geom["pool"] else "")
    else:
        geo = ("batched",) + batched_layout(entry, geom)
    return (entry, kid, geom["dtype"], geo, flags)
