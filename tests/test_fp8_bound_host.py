"""CPU only: the e4m3 oracle (tests/exact_fp8.py) can tell right from wrong before it meets a kernel.  e4m3_rne against torch's
conversion; the tier A generator's range; a CPU emulation of what the kernels do (f32 accumulation of the dequantised products in
64-element groups, groups in a shuffled order, f32 epilogue, round-to-nearest stores) passes both tiers at three shapes of the case
table; seven defects each fail at least one tier, and pass again with the defect switched off; the case table covers every required
variant, every instantiation of k_conv_fwd256<fp8e4> and every launch class of tests/golden/bench_fp8_launches.json."""
import json
import os

import pytest
import torch

import exact_fp8 as F
import exact_gemm as X
import exact_roi as XR
import fp8_exact_cases as T

CASE = {c["id"]: c for c in T.CASES}


# ------------------------------------------------------------------------------------------------ the reference rounding
def test_e4m3_rne_is_torchs_conversion_on_every_bf16_pattern_and_every_tie():
    bits = torch.arange(65536, dtype=torch.int32).to(torch.int16).view(torch.bfloat16)
    x = bits[torch.isfinite(bits.float())].double()
    ties = F.midpoints_f32().double()
    for t in (x, x * 0.37, x * (448.0 / 3.0), ties):
        want = t.clamp(-448.0, 448.0).float().to(torch.float8_e4m3fn)        # (torch does not saturate: clamp first, as the kernels do)
        assert F.same_codes(F.e4m3_encode(t), want.view(torch.uint8)) == 0
        assert torch.equal(F.e4m3_rne(t).abs(), want.float().double().abs())
    # ties go to the even code, 464 (the tie between 448 and the absent 480) saturates, subnormals are multiples of 2^-9
    assert float(F.e4m3_rne(torch.tensor(2.0 ** -10))) == 0.0 and float(F.e4m3_rne(torch.tensor(3 * 2.0 ** -10))) == 2.0 ** -8
    assert float(F.e4m3_rne(torch.tensor(464.0))) == 448.0 and float(F.e4m3_rne(torch.tensor(-1e9))) == -448.0
    assert torch.equal(F.deq(F.e4m3_encode(torch.arange(-16, 17).double())), torch.arange(-16, 17).double())   # every |v| <= 16 is exact
    assert torch.equal(XR.e4m3_decode(torch.arange(0, 127, dtype=torch.uint8)), F.deq(torch.arange(0, 127, dtype=torch.uint8)))


def test_tier_a_sums_stay_exact_for_every_case():
    for c in T.CASES:
        if "A" not in c["tiers"]:
            continue
        vmax = 3 if c["geom"]["dtype"] == "bf16" else F.TIER_A_VMAX
        assert T.reduction_length(c) * vmax ** 2 < 2 ** 24, c["id"]
        if c["geom"]["dtype"] == "e4m3" and c["entry"] != "conv_wgrad_fp8":
            assert T.reduction_length(c) * vmax ** 2 <= 2 ** 17, c["id"]        # (what pattern (d) of the probe covered)
    with pytest.raises(AssertionError):
        F.tier_a_operand((8,), 2 ** 20 + 1, torch.Generator().manual_seed(0), "cpu", vmax=4)


# ------------------------------------------------------------------------------------------------ the emulation
def _grouped(a, b, seed, drop_last=False, swap_chunks=False, splits=1):
    """a [R, G, 64], b [N, G, 64] float64 (e4m3 numbers) -> ``splits`` f32 partial sums [R, N]: every group's 64 products summed in
    f32, the groups added in a shuffled order.  drop_last: the last group is never added; swap_chunks: elements 0..15 and 16..31 of
    every group of a trade places (b's stay)."""
    a32, b32 = a.float(), b.float()
    if swap_chunks:
        a32 = torch.cat([a32[..., 16:32], a32[..., :16], a32[..., 32:]], -1)
    G = a.shape[1]
    order = torch.randperm(G - 1 if drop_last else G, generator=torch.Generator().manual_seed(seed)).tolist()
    parts = [torch.zeros(a.shape[0], b.shape[0]) for _ in range(splits)]
    for i, g in enumerate(order):
        parts[i % splits] += a32[:, g] @ b32[:, g].t()
    return parts


def _store(v32, odt, truncate=False):
    if odt == torch.float32:
        return v32
    return X.truncate_bf16(v32).to(torch.bfloat16) if truncate else v32.to(torch.bfloat16)


def _conv_problem(c, tier, seed):
    g, e = c["geom"], c["epi"]
    N, H, W, Cin, Cout, KH, KW, pad = (g[k] for k in ("N", "H", "W", "Cin", "Cout", "KH", "KW", "pad"))
    Ho, Wo = X.out_geometry(H, W, KH, KW, 1, pad, False)
    M, K = N * Ho * Wo, KH * KW * Cin
    gen = torch.Generator().manual_seed(seed)
    mk = (lambda s: F.tier_a_operand(s, K, gen, "cpu")) if tier == "A" else (lambda s: F.tier_b_operand(s, gen, "cpu"))
    x, w = F.deq(mk((N, H, W, Cin))), F.deq(mk((Cout, KH, KW, Cin)))
    if tier == "A":
        scale = torch.pow(2.0, torch.randint(-2, 2, (Cout,), generator=gen).float())
        bias = torch.randint(-64, 65, (Cout,), generator=gen).float() / 8
    else:
        scale = (torch.rand(Cout, generator=gen) + 0.5) * (K ** -0.5 / 1e4)
        bias = torch.randn(Cout, generator=gen) * 0.1
    return dict(x=x, w=w, scale=scale, bias=bias, M=M, Ho=Ho, Wo=Wo, pad=pad, relu=e["relu"], odt=torch.float32 if e["out_f32"] else torch.bfloat16)


def _conv_emulate(p, seed, unmasked_border=False, scale_before_sum=False, truncate=False, e4m3_toward_zero=False, q8=None, **defect):
    """-> (y, y8 values or None): the forward kernel's arithmetic on the CPU"""
    x, w = p["x"], p["w"]
    N, H, W, Cin = x.shape
    Cout, KH, KW, _ = w.shape
    rows = torch.arange(p["M"])
    a, b = [], []
    for kh in range(KH):
        for kw in range(KW):
            if unmasked_border:               # the clamped pixel itself instead of the zero padding
                n, r = rows // (p["Ho"] * p["Wo"]), rows % (p["Ho"] * p["Wo"])
                ih = ((r // p["Wo"]) - p["pad"] + kh).clamp(0, H - 1)
                iw = ((r % p["Wo"]) - p["pad"] + kw).clamp(0, W - 1)
                a.append(x.reshape(-1, Cin)[(n * H + ih) * W + iw])
            else:
                a.append(X._tap_rows(x, rows, p["Ho"], p["Wo"], kh, kw, 1, p["pad"]))
            b.append(w[:, kh, kw])
    a, b = torch.cat(a, 1).reshape(p["M"], -1, 64), torch.cat(b, 1).reshape(Cout, -1, 64)
    s, bi = p["scale"], p["bias"]
    if scale_before_sum:                          # the epilogue applied to each of two splits, then the sum: the bias counts twice
        p1, p2 = _grouped(a, b, seed, splits=2, **defect)
        v = (p1 * s + bi) + (p2 * s + bi)
    else:
        p1, p2 = _grouped(a, b, seed, splits=2, **defect)
        v = (p1 + p2) * s + bi
    if p["relu"]:
        v = v.clamp_min(0)
    y8 = None
    if q8 is not None:
        t = (v * q8).double()
        y8 = F.round_e4m3_toward_zero(t) if e4m3_toward_zero else F.e4m3_rne(t)
    return _store(v, p["odt"], truncate), y8


def _conv_verdict(c, tier, seed, **defect):
    """does the emulation (with a defect) pass the tier's checks?"""
    p = _conv_problem(c, tier, seed)
    q8 = 0.5 if tier == "A" else 100.0
    y, y8 = _conv_emulate(p, seed, q8=q8, **defect)
    acc, absp = X.conv_exact(p["x"], p["w"], 1, p["pad"])
    gterm = F.conv_group_term(p["x"], p["w"], p["pad"])
    exact = X.epilogue_exact(acc, p["scale"], p["bias"], None, p["relu"])
    codes = F.e4m3_encode(y8)
    if tier == "A":
        want = X.round_bf16(exact) if p["odt"] == torch.bfloat16 else exact.float().double()
        return torch.equal(y.double(), want) and F.same_codes(codes, F.e4m3_encode(exact * q8)) == 0
    ok, _, _ = F.check_bound(y, exact, absp, gterm, p["odt"], p["scale"], p["bias"])
    if p["odt"] == torch.bfloat16:
        rb, n = X.rounding_bias(y, exact, absp, p["scale"])
        ok = ok and n >= 1000 and abs(rb) <= 0.05
    ok8, _, _ = XR.check_e4m3(codes, exact, F.pre_bound(absp, gterm, p["scale"], p["bias"]), q8)
    return ok and ok8


def _wgrad_verdict(c, tier, seed, overwrite=False, **defect):
    g = c["geom"]
    N, H, W, Cin, Cout, KH, KW, pad = (g[k] for k in ("N", "H", "W", "Cin", "Cout", "KH", "KW", "pad"))
    M = N * H * W
    gen = torch.Generator().manual_seed(seed)
    mk = (lambda s: F.tier_a_operand(s, M, gen, "cpu")) if tier == "A" else (lambda s: F.tier_b_operand(s, gen, "cpu"))
    x, d = F.deq(mk((N, H, W, Cin))), F.deq(mk((N, H, W, Cout)))
    if tier == "A":
        scale, base = torch.pow(2.0, torch.randint(-2, 2, (Cout,), generator=gen).float()), torch.randint(-100, 101, (Cout, KH * KW, Cin), generator=gen).float()
    else:
        scale, base = (torch.rand(Cout, generator=gen) + 0.5) * (M ** -0.5 / 1e4), torch.randn(Cout, KH * KW, Cin, generator=gen)
    T64 = (M + 63) // 64
    dp = torch.zeros(T64 * 64, Cout, dtype=torch.float64)
    dp[:M] = d.reshape(M, Cout)
    dp = dp.view(T64, 64, Cout).permute(2, 0, 1)
    got = torch.empty(Cout, KH * KW, Cin)
    rows = torch.arange(M)
    for t in range(KH * KW):
        ap = torch.zeros(T64 * 64, Cin, dtype=torch.float64)
        ap[:M] = X._tap_rows(x, rows, H, W, t // KW, t % KW, 1, pad)
        p1, p2 = _grouped(dp, ap.view(T64, 64, Cin).permute(2, 0, 1), seed + t, splits=2, **defect)
        upd = (p1 + p2) * scale.view(-1, 1)
        got[:, t] = upd if overwrite else base[:, t] + upd
    acc, absp = X.wgrad_exact(x, d, KH, KW, 1, pad)
    gterm = F.wgrad_group_term(x, d, KH, KW, pad)
    sc = scale.view(-1, 1, 1)
    exact = acc * sc.double() + base.double()
    if tier == "A":
        return torch.equal(got.double(), exact)
    return F.check_bound(got, exact, absp, gterm, torch.float32, sc, None, None, base.abs())[0]


def _dot_verdict(c, tier, seed, **defect):
    g = c["geom"]
    gen = torch.Generator().manual_seed(seed)
    mk = (lambda s: F.tier_a_operand(s, g["K"], gen, "cpu")) if tier == "A" else (lambda s: F.tier_b_operand(s, gen, "cpu"))
    a, b = F.deq(mk((g["R"], g["K"]))), F.deq(mk((g["N"], g["K"])))
    alpha = 0.125
    p1, p2 = _grouped(a.reshape(g["R"], -1, 64), b.reshape(g["N"], -1, 64), seed, splits=2, **defect)
    got = (p1 + p2) * alpha
    exact = (a @ b.t()) * alpha
    if tier == "A":
        return torch.equal(got.double(), exact)
    return F.check_bound(got, exact, a.abs() @ b.abs().t(), F.dot_group_term(a, b), torch.float32, torch.tensor([[alpha]]))[0]


_TAPS = T.case("host_taps", "conv_fwd_fp8", 10, T.conv8(1, 5, 8, 128, 256, 3, 1), T.SETS["bn_relu_emit8"], {}, "a 3x3 small enough for the CPU")


def test_emulation_passes_both_tiers_at_three_table_shapes():
    for tier in T.AB:
        assert _conv_verdict(CASE["fp8_short_m"], tier, 1), tier
        assert _conv_verdict(CASE["fp8_short_m_f32"], tier, 2), tier
        assert _wgrad_verdict(CASE["wgrad8_short_m_scale"], tier, 3), tier
        assert _dot_verdict(CASE["dot_33_20_1024"], tier, 4), tier


_CONTROLS = [
    ("the last 64-group dropped", _conv_verdict, CASE["fp8_short_m"], dict(drop_last=True)),
    ("the last 64-group dropped (dot)", _dot_verdict, CASE["dot_33_20_1024"], dict(drop_last=True)),
    ("two 16-byte chunks of A swapped without B", _conv_verdict, CASE["fp8_short_m"], dict(swap_chunks=True)),
    ("two 16-byte chunks of A swapped without B (weight gradient)", _wgrad_verdict, CASE["wgrad8_short_m_scale"], dict(swap_chunks=True)),
    ("a border tap read unmasked", _conv_verdict, _TAPS, dict(unmasked_border=True)),
    ("dW overwritten instead of accumulated", _wgrad_verdict, CASE["wgrad8_short_m_scale"], dict(overwrite=True)),
    ("scale and bias applied to each of two splits before their sum", _conv_verdict, CASE["fp8_short_m"], dict(scale_before_sum=True)),
    ("a truncating bf16 store", _conv_verdict, CASE["fp8_short_m"], dict(truncate=True)),
    ("e4m3 rounding toward zero", _conv_verdict, CASE["fp8_short_m"], dict(e4m3_toward_zero=True)),
]


@pytest.mark.parametrize("name,verdict,c,defect", _CONTROLS, ids=[k[0] for k in _CONTROLS])
def test_negative_control_fails_a_tier_and_passes_without_its_defect(name, verdict, c, defect):
    off = {k: False for k in defect}
    clean = [verdict(c, tier, 11, **off) for tier in T.AB]
    broken = [verdict(c, tier, 11, **defect) for tier in T.AB]
    assert all(clean), (name, "the emulation without the defect must pass", clean)
    assert not all(broken), (name, "passed both tiers", broken)


# ------------------------------------------------------------------------------------------------ coverage
def _covered(pred):
    return {t for c in T.CASES if pred(c) for t in c["tiers"]}


def test_every_required_variant_has_both_tiers():
    for v in T.REQUIRED_VARIANTS:
        assert _covered(lambda c: v in c["variants"]) == {"A", "B"}, v
    for v in T.TIER_B_ONLY:
        assert "B" in _covered(lambda c: v in c["variants"]), v
    assert len({c["id"] for c in T.CASES}) == len(T.CASES)


def test_every_instantiation_of_the_e4m3_forward_kernel_is_reached():
    want = {(taps, epi) for taps in (False, True) for epi in (0, 1, 2, 3, -1)}
    for tier in T.AB:
        got = {(T.taps_template(c["geom"]), T.epi_template(c["epi"])) for c in T.CASES if c["entry"] == "conv_fwd_fp8" and tier in c["tiers"]}
        assert got == want, (tier, want - got)
    # -1 is reached both ways: f32 output and the e4m3 second output
    for taps in (False, True):
        m1 = [c["epi"] for c in T.CASES if c["entry"] == "conv_fwd_fp8" and T.taps_template(c["geom"]) == taps and T.epi_template(c["epi"]) == -1]
        assert any(e["out_f32"] for e in m1) and any(e["emit8"] for e in m1)


def test_every_recorded_fp8_launch_class_has_a_case(golden_dir):
    with open(os.path.join(golden_dir, "bench_fp8_launches.json")) as fh:
        rec = json.load(fh)["entries"]
    assert {e["entry"] for e in rec} == {"conv_fwd", "conv_fwd_fp8", "conv_wgrad_fp8", "fp8_dot_nt"}
    have = {}
    for c in T.CASES:
        have.setdefault(T.launch_class(c["entry"], c["kid"], c["geom"], c["epi"]), set()).update(c["tiers"])
    for e in rec:
        k = T.launch_class(e["entry"], e["kernel_id"], e["geometry"], e["epilogue"])
        assert have.get(k) == {"A", "B"}, (k, e["geometry"])
    # the bench's RoI-head 3x3 at 16 images has a full-M case for each of the two GEMM kernels
    for entry in ("conv_fwd_fp8", "conv_wgrad_fp8"):
        geoms = [{k: e["geometry"][k] for k in ("N", "H", "W", "Cin", "Cout", "KH")} for e in rec if e["entry"] == entry]
        full = {k: T.FULL_M[k] for k in ("N", "H", "W", "Cin", "Cout", "KH")}
        assert full in geoms and any(c["entry"] == entry and "full_m" in c["variants"] and c["geom"] == T.FULL_M for c in T.CASES)
