"""Case table of tests/test_gpu_fp8_exact.py, plain data in the format of tests/gemm_exact_cases.py (the host test
tests/test_fp8_bound_host.py imports it to check that every instantiation of k_conv_fwd256<fp8e4>, every required variant and
every launch class of tests/golden/bench_fp8_launches.json has a Tier A and a Tier B case).

A case: entry point, the kernel id the dispatch must report (cddmsl_last_kernel; None for fp8_dot_nt, which has one kernel and
does not go through the dispatch), per-call environment switches, geometry, epilogue flags, tiers, variants and ``why``.
Tier A: integer operands |v| <= exact_fp8.TIER_A_VMAX as e4m3 bytes, output bit-equal to the exact value rounded once.
Tier B: Gaussian operands quantised to a maximum of 448, held to exact_fp8.check_bound and the rounding-bias check."""

AB = ("A", "B")
F256 = {"CDDMSL_GEMM256": "2", "CDDMSL_FWD2": "0"}          # the bf16 256x256 kernel wherever legal (the e4m3 second output needs it)


def conv8(N, H, W, Cin, Cout, K=1, pad=0, dtype="e4m3"):
    return dict(N=N, H=H, W=W, Cin=Cin, Cout=Cout, KH=K, KW=K, stride=1, pad=pad, pool=False, dtype=dtype)


def fwd(scale=False, bias=False, residual=None, relu=False, relu_mask=False, out_f32=False, emit8=False):
    return dict(scale=scale, bias=bias, residual=residual, relu=relu, relu_mask=relu_mask, out_f32=out_f32, emit8=emit8)


def wg(scale=False, accumulate=True, ldd_extra=0):
    """scale False: a vector of ones (the entry point always takes one); ldd_extra: bytes between dy rows beyond Cout"""
    return dict(scale=scale, accumulate=accumulate, ldd_extra=ldd_extra)


def case(id, entry, kid, geom, epi, env, why, variants=(), tiers=AB):
    return dict(id=id, entry=entry, kid=kid, geom=geom, epi=epi, env=env, why=why, variants=tuple(variants), tiers=tiers)


# the operand sets conv_fwd_auto / dgrad_auto (cddmsl_amd/layers.py) launch kernel 10 with, each with and without the e4m3 second output
PRODUCTION = {"bn_relu": fwd(True, True, relu=True), "bn_res_relu": fwd(True, True, "bf16", True),
              "mask": fwd(True, relu_mask=True), "mask_res": fwd(True, residual="bf16", relu_mask=True)}
SETS = {"plain": fwd(), "dq": fwd(True), "f32": fwd(True, True, out_f32=True), **PRODUCTION,
        **{k + "_emit8": dict(v, emit8=True) for k, v in PRODUCTION.items()}}


def epi_template(e):
    """EPI template argument of k_conv_fwd256 for an epilogue set: epi_of in conv_fwd256.hip"""
    if e["out_f32"] or e["emit8"] or e["residual"] == "f32":
        return -1
    return (1 if e["residual"] else 0) | (2 if e["relu_mask"] else 0)


def taps_template(g):
    """TAPS template argument: launch_tile256 in conv_fwd256.hip"""
    return not (g["KH"] == 1 and g["KW"] == 1 and g["pad"] == 0)


def fwd8_variants(g, e):
    v = [f"k10<{'taps' if taps_template(g) else '1x1'},{epi_template(e)}>"]
    key = [k for k, s in PRODUCTION.items() if {**s, "emit8": False} == {**e, "emit8": False}]
    if key:
        v.append("prod_" + key[0] + ("_emit8" if e["emit8"] else ""))
    return v


CASES = []
# ---- k_conv_fwd256<fp8e4> (id 10): plan_fwd takes it for every legal e4m3 launch; launch_tile256 / launch256 / launch256_main pick
# TAPS and EPI.  M = 2 * 19 * 23 = 874: three full 256-row panels and a ragged one; Cout 512: two column tiles.
_G1 = conv8(2, 19, 23, 256, 512)
_G3 = conv8(2, 19, 23, 128, 512, 3, 1)
for k, e in SETS.items():
    CASES.append(case(f"fp8_1x1_{k}", "conv_fwd_fp8", 10, _G1, e, {}, f"k_conv_fwd256<fp8e4, false, EPI {epi_template(e)}>, two K-tiles, launch256_main",
                      ["fp8_1x1"] + fwd8_variants(_G1, e)))
for k, e in SETS.items():
    CASES.append(case(f"fp8_taps_{k}", "conv_fwd_fp8", 10, _G3, e, {}, f"k_conv_fwd256<fp8e4, true, EPI {epi_template(e)}>: border taps of every row panel, launch256_main",
                      ["fp8_taps"] + fwd8_variants(_G3, e)))
_ONE = [
    ("fp8_one_ktile", conv8(2, 19, 23, 128, 512), "bn_relu", "one 128-element K-tile: shorter than the two-tile prefetch"),
    ("fp8_odd_ktiles", conv8(2, 19, 23, 384, 512), "mask_res", "three K-tiles: an odd count through the two-set loop"),
    ("fp8_valid_3x3", conv8(2, 19, 23, 128, 512, 3, 0), "bn_res_relu", "3x3 without padding (legal by gemm256_legal: 2 pad <= KH - 1): Ho x Wo = 17 x 21"),
    ("fp8_5x5", conv8(2, 19, 23, 128, 512, 5, 2), "mask", "25 taps (<= 31 bits of the per-row tap mask)"),
    ("fp8_short_m", conv8(1, 5, 8, 256, 256), "bn_relu_emit8", "M = 40 < 256: one ragged panel, one tile; e4m3 second output of a ragged panel"),
    ("fp8_short_m_f32", conv8(1, 5, 8, 256, 256), "f32", "M = 40 < 256, f32 output"),
]
for id_, g, k, why in _ONE:
    CASES.append(case(id_, "conv_fwd_fp8", 10, g, SETS[k], {}, "k_conv_fwd256<fp8e4>: " + why, [id_.replace("_f32", "")] + fwd8_variants(g, SETS[k])))

# ---- k_wgrad256_f8 (id 12): plan_wgrad's OP_FP8 branch; always into a non-zero dW, with a scale of ones and with a real one
_W = [
    ("wgrad8_1x1_a", conv8(2, 19, 23, 512, 256), {}, "1x1 (the RoI head's conv1 / conv3: the taps == false staging path), 512 -> 256, M = 874", ["wgrad8_1x1"]),
    ("wgrad8_1x1_b", conv8(2, 19, 23, 256, 512), {}, "1x1, 256 -> 512", ["wgrad8_1x1"]),
    ("wgrad8_3x3", conv8(9, 14, 14, 256, 256, 3, 1), {}, "3x3, M = 1764: 28 reduction tiles, two splits through the workspace", ["wgrad8_3x3"]),
    ("wgrad8_atomics", conv8(9, 14, 14, 256, 256, 3, 1), {"CDDMSL_WGRAD_WS": "0"}, "the split reduction on f32 atomics (use_workspace)", ["wgrad8_atomics"]),
    ("wgrad8_short_m", conv8(1, 5, 3, 256, 256, 3, 1), {}, "M = 15: one reduction tile, fewer than the ring is deep, odd count", ["wgrad8_short_m"]),
    ("wgrad8_narrow_w", conv8(2, 50, 3, 256, 256, 3, 1), {}, "W = 3: every tap's border inside every reduction tile", ["wgrad8_narrow_w"]),
]
for id_, g, env, why, var in _W:
    for sc in (False, True):
        CASES.append(case(id_ + ("_scale" if sc else "_ones"), "conv_wgrad_fp8", 12, g, wg(sc), env, "k_wgrad256_f8: " + why, var + ["wgrad8_scale" if sc else "wgrad8_ones"]))
CASES.append(case("wgrad8_ldd", "conv_wgrad_fp8", 12, conv8(2, 19, 23, 256, 256, 3, 1), wg(True, True, 256), {},
                  "k_wgrad256_f8: dy rows ldd = Cout + 256 bytes apart (C ABI), the gap filled with NaN codes", ["wgrad8_ldd", "wgrad8_scale"]))

# ---- k_conv_fwd256<bf16> with the e4m3 second output (id 3, cddmsl_conv_fwd_q8): bf16 operands at the kernel-10 geometries
for gname, g in (("1x1", conv8(2, 19, 23, 256, 512, dtype="bf16")), ("3x3", conv8(2, 19, 23, 128, 512, 3, 1, dtype="bf16"))):
    for k in ("bn_relu", "bn_res_relu", "mask", "mask_res"):      # (the bf16 input-gradient launches carry no scale)
        e = dict(PRODUCTION[k], emit8=True, scale=not k.startswith("mask"))
        CASES.append(case(f"q8_{gname}_{k}", "conv_fwd_q8", 3, g, e, F256, "k_conv_fwd256<bf16, EPI -1> writing y8 / amax8 (cddmsl_conv_fwd_q8)",
                          ["q8_" + gname, "q8_" + k]))

# ---- k_fp8_dot_nt: one wave per 32 rows; c rows ldc = N + 3 apart with sentinel columns; alpha null and non-null inside each case
for R in (1, 31, 32, 33, 1000):
    for N in (1, 20, 32):
        for K in (64, 128, 1024):
            CASES.append(case(f"dot_{R}_{N}_{K}", "fp8_dot_nt", None, dict(R=R, N=N, K=K, ldc=N + 3, dtype="e4m3"), dict(alpha="both"), {},
                              "k_fp8_dot_nt: ragged last wave, partial columns, one and many K steps", ["dot_nt"]))

# ---- one bench launch per kernel, row-sampled (tier B only): the RoI head's 3x3 at 16 images
FULL_M = conv8(8192, 14, 14, 512, 512, 3, 1)
CASES += [
    case("fp8_full_m_roi_3x3", "conv_fwd_fp8", 10, FULL_M, SETS["bn_relu"], {}, "k_conv_fwd256<fp8e4> at the bench's (1605632, 512, 4608) launch", ["full_m", "fp8_taps"] + fwd8_variants(FULL_M, SETS["bn_relu"]), ("B",)),
    case("wgrad8_full_m_roi_3x3", "conv_wgrad_fp8", 12, FULL_M, wg(True), {}, "k_wgrad256_f8 at the bench's (1605632, 512, 4608) launch", ["full_m", "wgrad8_3x3", "wgrad8_scale"], ("B",)),
]

K10_INSTANCES = [f"k10<{t},{e}>" for t in ("1x1", "taps") for e in (0, 1, 2, 3, -1)]
REQUIRED_VARIANTS = K10_INSTANCES + [
    "fp8_1x1", "fp8_taps", "fp8_one_ktile", "fp8_odd_ktiles", "fp8_valid_3x3", "fp8_5x5", "fp8_short_m",
    *["prod_" + k for k in PRODUCTION], *["prod_" + k + "_emit8" for k in PRODUCTION],
    "wgrad8_1x1", "wgrad8_3x3", "wgrad8_atomics", "wgrad8_ldd", "wgrad8_short_m", "wgrad8_narrow_w", "wgrad8_scale", "wgrad8_ones",
    "q8_1x1", "q8_3x3", "q8_bn_relu", "q8_bn_res_relu", "q8_mask", "q8_mask_res", "dot_nt",
]
# variants only Tier B can carry (bench shapes: integer operands over 1.6 M rows say nothing the small cases do not)
TIER_B_ONLY = ["full_m"]


def reduction_length(c):
    """longest reduction of a case (what the Tier A generator must keep exact)"""
    g = c["geom"]
    if c["entry"] == "fp8_dot_nt":
        return g["K"]
    if c["entry"] == "conv_wgrad_fp8":
        return g["N"] * g["H"] * g["W"]
    return g["KH"] * g["KW"] * g["Cin"]


def launch_class(entry, kid, geom, epi):
    """what the coverage check groups launches by: entry point, kernel id, operand dtype, taps or 1x1, and the epilogue flags that are set"""
    flags = tuple(sorted(k if v is True else f"{k}={v}" for k, v in epi.items() if v and k not in ("ldd_extra", "alpha")))
    entry = "conv_fwd_q8" if entry == "conv_fwd" else entry          # (the recorder notes the bf16 launch under hip.conv_fwd)
    geo = ("dot",) if entry == "fp8_dot_nt" else ("taps" if geom["KH"] * geom["KW"] > 1 else "1x1",)
    return (entry, kid or 0, geom["dtype"], geo, flags)
