"""The exact-product checker itself (tests/exact_gemm.py), on the CPU: the float64 reference against ATen, the bound against an f32
convolution in another summation order, negative controls the bound must reject -- with the verdict of the old 2e-2 * max criterion
printed next to it --, the same for f32 operands, and the coverage of the recorded launches (the bench step's and the stock R50-C4 step's,
in bf16 and in f32) by the GPU case table."""
import json
import os

import pytest
import torch
import torch.nn.functional as F

import exact_gemm as X
import gemm_exact_cases as CASES

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _g(seed):
    return torch.Generator().manual_seed(seed)


@pytest.mark.parametrize("K,stride,pad,pool", [(1, 1, 0, False), (3, 1, 1, False), (3, 2, 1, False), (1, 2, 0, False),
                                               (3, 1, 0, False), (1, 56, 0, False), (3, 2, 0, False), (1, 1, 0, True)])
def test_conv_exact_equals_aten_float64(K, stride, pad, pool):
    N, H, W, Cin, Cout = 2, 9, 113 if stride == 56 else 13, 24, 16
    if pool:
        H, W = 11, 15
    x = torch.randn(N, H, W, Cin, generator=_g(1), dtype=torch.float64)
    w = torch.randn(Cout, K, K, Cin, generator=_g(2), dtype=torch.float64)
    xin = x.permute(0, 3, 1, 2)
    ref = F.conv2d(F.avg_pool2d(xin, 2) if pool else xin, w.permute(0, 3, 1, 2), stride=1 if pool else stride, padding=pad)
    ref = ref.permute(0, 2, 3, 1).reshape(-1, Cout)
    got, absp = X.conv_exact(x, w, stride, pad, pool)
    assert got.shape == ref.shape
    assert (got - ref).abs().max() <= 1e-12 * ref.abs().max()
    ref_abs = F.conv2d(F.avg_pool2d(xin.abs(), 2) if pool else xin.abs(), w.abs().permute(0, 3, 1, 2), stride=1 if pool else stride,
                       padding=pad).permute(0, 2, 3, 1).reshape(-1, Cout)
    if not pool:           # (|mean| <= mean|.|: the pooled absprod is the product of the pooled operand's magnitude)
        assert (absp - ref_abs).abs().max() <= 1e-12 * ref_abs.abs().max()
    rows = X.sample_rows(got.shape[0], tile=16)
    g2, a2 = X.conv_exact(x, w, stride, pad, pool, rows=rows)
    assert torch.equal(g2, got[rows]) and torch.equal(a2, absp[rows])


def test_wgrad_and_gemm_exact_equal_aten_float64():
    N, H, W, Cin, Cout = 2, 7, 9, 16, 8
    x = torch.randn(N, H, W, Cin, generator=_g(3), dtype=torch.float64)
    dy = torch.randn(N, H, W, Cout, generator=_g(4), dtype=torch.float64)
    w = torch.zeros(Cout, Cin, 3, 3, dtype=torch.float64, requires_grad=True)
    F.conv2d(x.permute(0, 3, 1, 2), w, padding=1).backward(dy.permute(0, 3, 1, 2))
    got, _ = X.wgrad_exact(x, dy, 3, 3, 1, 1, chunk=37)
    assert (got - w.grad.permute(0, 2, 3, 1).reshape(Cout, 9, Cin)).abs().max() <= 1e-12 * w.grad.abs().max()
    got1, _ = X.wgrad_exact(x, dy, 3, 3, 1, 1, taps=[(2, 0)])
    assert (got1[:, 0] - got[:, 6]).abs().max() <= 1e-12 * got.abs().max()
    a = torch.randn(3, 20, 16, generator=_g(5), dtype=torch.float64)
    b = torch.randn(3, 12, 16, generator=_g(6), dtype=torch.float64)
    assert torch.allclose(X.gemm_exact(a, b)[0], torch.bmm(a, b.transpose(1, 2)), rtol=0, atol=1e-12)
    c = torch.randn(3, 20, 12, generator=_g(7), dtype=torch.float64)
    assert torch.allclose(X.gemm_exact(c, a, transpose_a=True)[0], torch.bmm(c.transpose(1, 2), a), rtol=0, atol=1e-12)


def test_round_bf16_is_round_to_nearest_even():
    v = torch.randn(200000, generator=_g(8), dtype=torch.float64) * 37
    r = X.round_bf16(v)
    lo = X.truncate_bf16(v)
    hi = lo + torch.sign(v) * X.ulp_bf16(lo)
    d_lo, d_hi = (v - lo).abs(), (hi - v).abs()
    assert bool(((r == lo) | (r == hi)).all())
    assert bool(torch.where(d_lo < d_hi, r == lo, torch.ones_like(r, dtype=torch.bool)).all())
    assert bool(torch.where(d_hi < d_lo, r == hi, torch.ones_like(r, dtype=torch.bool)).all())
    # ties go to the even neighbour; a value just past a tie in float64 (but a tie once in f32) goes away from the tie
    t = torch.tensor([257.0, 259.0, -257.0, 257.0 + 2 ** -30], dtype=torch.float64)
    assert X.round_bf16(t).tolist() == [256.0, 260.0, -256.0, 258.0]


def test_sample_rows_covers_tiles_edges_and_2gib_crossings():
    M, rb = 3211264, 1024                      # 3.06 GiB of 1 KiB rows
    r = X.sample_rows(M, rb)
    assert int(r[0]) == 0 and int(r[-1]) == M - 1
    assert torch.equal(torch.unique(r // 256), torch.arange((M + 255) // 256))
    assert bool((torch.bincount(r // 256) >= 1).all())
    assert (2 ** 31) // rb in r.tolist() and (2 ** 31) // rb - 1 in r.tolist()
    r2 = X.sample_rows(1000, 6)                # ragged last tile: every row
    assert set(range(768, 1000)) <= set(r2.tolist())


def _case_fwd(M=600, K=1024, Cout=512, seed=11):
    x = torch.randn(M, K, generator=_g(seed)).bfloat16()
    w = (torch.randn(Cout, K, generator=_g(seed + 1)) * K ** -0.5).bfloat16()
    exact, absp = X.conv_exact(x.view(1, 1, M, K), w.view(Cout, 1, 1, K))
    return x, w, exact, absp


def test_bound_accepts_an_f32_convolution_in_another_order():
    """ATen's CPU f32 convolution of the same bf16 operands (blocked, its own summation order), rounded RNE to bf16 -- and its
    f32 result as an f32 output: both inside the bound, no rounding bias"""
    N, H, W, Cin, Cout = 4, 31, 37, 64, 96
    x = torch.randn(N, H, W, Cin, generator=_g(21)).bfloat16()
    w = (torch.randn(Cout, 3, 3, Cin, generator=_g(22)) * (9 * Cin) ** -0.5).bfloat16()
    scale = torch.rand(Cout, generator=_g(23)) + 0.5
    bias = torch.randn(Cout, generator=_g(24)) * 0.1
    f32 = F.conv2d(x.float().permute(0, 3, 1, 2), w.float().permute(0, 3, 1, 2), padding=1).permute(0, 2, 3, 1).reshape(-1, Cout)
    acc, absp = X.conv_exact(x, w, 1, 1)
    exact = X.epilogue_exact(acc, scale, bias)
    got = (f32 * scale + bias).bfloat16()
    ok, ratio, _ = X.check_bound(got, exact, absp, torch.bfloat16, scale, bias)
    assert ok, ratio
    ok32, ratio32, _ = X.check_bound(f32, acc, absp, torch.float32)
    assert ok32, ratio32
    rb, n = X.rounding_bias(got, exact, absp, scale)
    assert n >= 100000 and abs(rb) <= 0.02, (rb, n)
    print(f"\nf32 conv (other order) -> bf16: worst |err|/bound {ratio:.3f}, f32 output {ratio32:.3f}, rounding bias {rb:+.4f} over {n}")


def _mutants():
    """(name, got, exact, absprod, out dtype, epilogue operands for the bound, reference of the old criterion)"""
    out = []
    # 1. one 32-wide K chunk dropped in one 256x256 tile
    x, w, acc, absp = _case_fwd()
    xa, wa = x.double(), w.double()
    drop = xa[256:512, 64:96] @ wa[256:512, 64:96].t()
    mut = acc.clone()
    mut[256:512, 256:512] -= drop
    out.append(("k-chunk dropped in one 256x256 tile", X.round_bf16(mut), acc, absp, torch.bfloat16, {}, acc))
    # 2. one 32-row chunk dropped from a weight-gradient reduction at M = 66 400 (f32 output)
    M, Cin, Cout = 66400, 64, 64
    xg = torch.randn(1, 1, M, Cin, generator=_g(31)).bfloat16()
    dy = torch.randn(1, 1, M, Cout, generator=_g(32)).bfloat16()
    dw, dabs = X.wgrad_exact(xg, dy, 1, 1)
    dw, dabs = dw[:, 0], dabs[:, 0]
    part = dy.view(M, Cout)[40000:40032].double().t() @ xg.view(M, Cin)[40000:40032].double()
    out.append(("32-row chunk dropped from a wgrad reduction (M=66400)", (dw - part).float(), dw, dabs, torch.float32, {}, dw))
    # 3. truncation instead of round-to-nearest-even on the store
    out.append(("truncating bf16 store", X.truncate_bf16(acc), acc, absp, torch.bfloat16, {}, acc))
    # 4. the bias omitted from one column tile
    bias = torch.randn(512, generator=_g(41)) * 0.1
    ex = X.epilogue_exact(acc, None, bias)
    mut = ex.clone()
    mut[:, 256:512] -= bias[256:512].double()
    out.append(("bias omitted from one column tile", X.round_bf16(mut), ex, absp, torch.bfloat16, {"bias": bias}, ex))
    # 5. the residual read from the neighbouring row in the last ragged tile (M = 600: rows 512..599)
    res = torch.randn(600, 512, generator=_g(51)).bfloat16().double()
    ex = X.epilogue_exact(acc, None, None, res)
    mut = ex.clone()
    mut[512:599] += res[513:600] - res[512:599]
    out.append(("residual from the neighbouring row in the ragged tile", X.round_bf16(mut), ex, absp, torch.bfloat16, {"residual": res}, ex))
    return out


def test_negative_controls_are_rejected_and_the_old_criterion_misses_some(capsys):
    lines = ["", "negative controls (each must be rejected by the exact-product bound):"]
    missed_by_old = 0
    for name, got, exact, absp, odt, epi, ref in _mutants():
        ok, ratio, _ = X.check_bound(got, exact, absp, odt, **epi)
        rb = X.rounding_bias(got, exact, absp)[0] if odt == torch.bfloat16 else 0.0
        rejected = not ok or abs(rb) > 0.02
        old_ok = X.old_criterion(got, ref)
        lines.append(f"  {name:55s} old 2e-2*max: {'ACCEPTS' if old_ok else 'rejects'}   new bound: {'rejects' if rejected else 'ACCEPTS'}"
              f"  (worst |err|/bound {ratio:.3g}, rounding bias {rb:+.3f})")
        assert rejected, name
        missed_by_old += old_ok
    with capsys.disabled():                 # (the verdicts are the point of this test: shown without -s)
        print("\n".join(lines))
    assert missed_by_old >= 1


def test_rounding_bias_separates_rne_from_truncation():
    _, _, acc, absp = _case_fwd(M=400, seed=61)
    rne, n = X.rounding_bias(X.round_bf16(acc), acc, absp)
    tr, _ = X.rounding_bias(X.truncate_bf16(acc), acc, absp)
    assert n >= 100000 and abs(rne) <= 0.02 and -0.55 < tr < -0.45, (rne, tr, n)


# ------------------------------------------------------------------------------------------------ f32 operands
def test_bound_accepts_atens_f32_convolution_of_f32_operands(capsys):
    """f32 operands: the products are rounded too (one more 2^-24 |a*b| each).  ATen's CPU f32 convolution of f32 Gaussian operands
    at the shape of the table's f32_fwd256_3x3 cases (K = 288) stays inside the bound with u_out = 2^-24 and the same C_ACC"""
    g = CASES.conv32(2, 19, 23, 32, 256, 3, 1, 1)
    assert any(c["geom"] == g for c in CASES.CASES)
    x = torch.randn(g["N"], g["H"], g["W"], g["Cin"], generator=_g(71))
    w = torch.randn(g["Cout"], 3, 3, g["Cin"], generator=_g(72)) * (9 * g["Cin"]) ** -0.5
    f32 = F.conv2d(x.permute(0, 3, 1, 2), w.permute(0, 3, 1, 2), padding=1).permute(0, 2, 3, 1).reshape(-1, g["Cout"])
    assert f32.dtype == torch.float32
    acc, absp = X.conv_exact(x, w, 1, 1)
    ok, ratio, _ = X.check_bound(f32, acc, absp, torch.float32)
    ar = X.acc_ratio(f32, acc, absp)
    with capsys.disabled():
        print(f"\nATen f32 conv of f32 operands (K = 288): worst |err|/bound {ratio:.3f}, acc_ratio {ar:.3g} (C_ACC = {X.C_ACC:g})")
    assert ok, ratio
    assert ar < X.C_ACC


def _f32_data(tier, shape, seed, lim=3, scale=1.0):
    if tier == "A":
        return torch.randint(-lim, lim + 1, shape, generator=_g(seed)).float()
    return torch.randn(shape, generator=_g(seed)) * scale


def _mutants_f32(tier):
    """(name, mutant, exact, absprod, operands of the bound) on f32 operands at shapes of the table's f32 cases; tier A data
    (small integers, power-of-two scales, dyadic bias / residual / dW) or tier B (Gaussian); mutant and exact in float64"""
    out = []
    N, H, W, Cin, Cout = 2, 9, 37, 36, 136                      # f32_fwd_1x1_*: 9 chunks of 4 elements
    x = _f32_data(tier, (N, H, W, Cin), 81)
    w = _f32_data(tier, (Cout, 1, 1, Cin), 82, scale=Cin ** -0.5)
    M = N * H * W
    if tier == "A":
        scale = torch.pow(2.0, torch.randint(-2, 2, (Cout,), generator=_g(83)).float())
        bias = torch.randint(-64, 65, (Cout,), generator=_g(84)).float() / 8
        res = torch.randint(-16, 17, (M, Cout), generator=_g(85)).float() / 4
        msk = torch.randint(-1, 2, (M, Cout), generator=_g(86)).float()
    else:
        scale = torch.rand(Cout, generator=_g(83)) + 0.5
        bias = torch.randn(Cout, generator=_g(84)) * 0.1
        res = torch.randn(M, Cout, generator=_g(85)) * 3.0
        msk = torch.randn(M, Cout, generator=_g(86))
    acc, absp = X.conv_exact(x, w)
    # 1. the last 4-element chunk of the reduction dropped (the one chunk of the second K-tile)
    short, _ = X.conv_exact(x[..., :Cin - 4].contiguous(), w[..., :Cin - 4].contiguous())
    out.append(("last 4-element chunk of the reduction dropped", short, acc, absp, {}))
    # 2. stride 2: the tap of the second row tile (rows 128..189 of 190) read one pixel to the right (f32_fwd_1x1_s2_*)
    x2, w2 = x[..., :32].contiguous(), w[..., :32].contiguous()
    ex2, ab2 = X.conv_exact(x2, w2, 2, 0)
    off, _ = X.conv_exact(torch.roll(x2, -1, dims=2), w2, 2, 0)
    mut = ex2.clone()
    mut[128:] = off[128:]
    out.append(("one tap read one pixel off under stride 2", mut, ex2, ab2, {}))
    # 3. the ReLU mask taken from the neighbouring channel
    ex = X.epilogue_exact(acc, relu_mask=msk)
    out.append(("mask taken from the neighbouring channel", X.epilogue_exact(acc, relu_mask=torch.roll(msk, -1, dims=1)), ex, absp, {}))
    # 4. the scale of channel n + 1 applied to channel n
    ex = X.epilogue_exact(acc, scale, bias, relu=True)
    out.append(("scale of channel n+1 applied to channel n", X.epilogue_exact(acc, torch.roll(scale, -1), bias, relu=True), ex, absp,
                {"scale": scale, "bias": bias}))
    # 5. the residual added twice
    ex = X.epilogue_exact(acc, None, None, res)
    out.append(("residual added twice", ex + res.double(), ex, absp, {"residual": res}))
    # weight gradient at f32_wgrad_dma_1x1_acc: M = 5920 rows, scale and a non-zero dW
    N, H, W, Cin, Cout = 4, 40, 37, 64, 96
    M = N * H * W
    xg, dy = _f32_data(tier, (N, H, W, Cin), 91), _f32_data(tier, (N, H, W, Cout), 92)
    base = (torch.randint(-100, 101, (Cout, Cin), generator=_g(93)).float() if tier == "A" else torch.randn(Cout, Cin, generator=_g(93))).double()
    sc = (torch.pow(2.0, torch.randint(-2, 2, (Cout,), generator=_g(94)).float()) if tier == "A" else torch.rand(Cout, generator=_g(94)) + 0.5).view(-1, 1)
    dw, dabs = X.wgrad_exact(xg, dy, 1, 1)
    dw, dabs = dw[:, 0], dabs[:, 0]
    ex = dw * sc.double() + base
    # 6. one of eight splits of the reduction lost (its atomics never land)
    rows = slice(2 * (M // 8), 3 * (M // 8))
    part = dy.view(M, Cout)[rows].double().t() @ xg.view(M, Cin)[rows].double()
    out.append(("one split's contribution to dW lost", (dw - part) * sc.double() + base, ex, dabs, {"scale": sc, "base": base.abs()}))
    # 7. dW overwritten instead of accumulated
    out.append(("dW overwritten instead of accumulated", dw * sc.double(), ex, dabs, {"scale": sc, "base": base.abs()}))
    return out


def test_f32_negative_controls_break_tier_a_and_the_tier_b_bound(capsys):
    """each mutant of an f32 launch, stored as a correctly rounded f32: tier A data -- not bit-equal to the exact value rounded once;
    tier B data -- outside check_bound with u_out = 2^-24 (the unmutated value, rounded once, passes both).  Next to it the verdict of
    the criterion tests/test_gpu_conv.py applies to f32 results, max|got - ref| < 2e-5 * max|ref|."""
    lines = ["", "f32 negative controls (tier A: must not be bit-equal; tier B: must be rejected by the bound):"]
    a, b = _mutants_f32("A"), _mutants_f32("B")
    assert [m[0] for m in a] == [m[0] for m in b] and len(a) == 7
    missed = []
    for (name, mut_a, ex_a, absp_a, _), (_, mut_b, ex_b, absp_b, epi) in zip(a, b):
        assert float(absp_a.max()) < 2 ** 24 and torch.equal(ex_a, ex_a.float().double()), name       # tier A's premise
        same = torch.equal(mut_a.float(), ex_a.float())
        ok0, r0, _ = X.check_bound(ex_b.float(), ex_b, absp_b, torch.float32, **epi)
        ok, ratio, _ = X.check_bound(mut_b.float(), ex_b, absp_b, torch.float32, **epi)
        old_ok = X.old_criterion(mut_b.float(), ex_b, tol=2e-5)
        missed += [name] if old_ok else []
        lines.append(f"  {name:48s} tier A bit-equal: {'YES' if same else 'no'}   old 2e-5*max: {'ACCEPTS' if old_ok else 'rejects'}   "
                     f"bound: {'ACCEPTS' if ok else 'rejects'} (worst |err|/bound {ratio:.3g}; unmutated {r0:.3g})")
        assert ok0 and r0 <= 1.0, (name, r0)
        assert not same, name
        assert not ok, name
    lines.append(f"  the 2e-5 * max criterion would have missed: {', '.join(missed) if missed else 'none of these, had it run them'}")
    with capsys.disabled():
        print("\n".join(lines))


# ------------------------------------------------------------------------------------------------ coverage of the recorded launches
BF16_RECORDS = ("bench_gemm_launches.json", "stock_gemm_launches.json")     # the CLIP benchmark step; the stock R50-C4 configuration's step
# ... and the same two configurations' f32 steps on one 800x1333 image (the oracle-parity path: tests/test_gpu_e2e.py test_full_size_step_matches_oracle)
F32_RECORDS = ("bench_gemm_launches_f32.json", "stock_gemm_launches_f32.json")
RECORDS = BF16_RECORDS + F32_RECORDS


def _recorded(name):
    with open(os.path.join(GOLDEN, name)) as fh:
        return json.load(fh)["entries"]


def test_case_table_covers_every_recorded_launch_class_in_both_tiers():
    rec = [e for record in RECORDS for e in _recorded(record)]
    assert all(_recorded(record) for record in RECORDS)
    have = {}
    for c in CASES.CASES:
        for tier in c["tiers"]:
            have.setdefault(CASES.launch_class(c["entry"], c["kid"], c["geom"], c["epi"]), set()).add(tier)
    missing = []
    for e in rec:
        cls = CASES.launch_class(e["entry"], e["kernel_id"], e["geometry"], e["epilogue"])
        if have.get(cls, set()) != {"A", "B"}:        # (the batched classes carry their strides: see launch_class)
            missing.append((cls, sorted(have.get(cls, ()))))
    assert not missing, missing


def test_case_table_covers_every_instantiation_and_bench_shape():
    variants = {v for c in CASES.CASES for v in c.get("variants", ())}
    assert not set(CASES.REQUIRED_VARIANTS) - variants, sorted(set(CASES.REQUIRED_VARIANTS) - variants)
    full = {(c["kid"]) for c in CASES.CASES if "full_m" in c.get("variants", ())}
    assert CASES.BENCH_KERNELS <= full, CASES.BENCH_KERNELS - full
    for record in BF16_RECORDS:
        launched = {e["kernel_id"] for e in _recorded(record)}
        assert launched <= CASES.BENCH_KERNELS, (record, launched - CASES.BENCH_KERNELS)
    f32_kernels = {(c["entry"], c["kid"]) for c in CASES.CASES if c["geom"]["dtype"] == "f32"}
    for record in F32_RECORDS:         # (one image: no full-M cases; every kernel an f32 step launches has f32 cases)
        rec = _recorded(record)
        assert all(e["geometry"]["dtype"] == "f32" for e in rec), record
        launched = {(e["entry"], e["kernel_id"]) for e in rec}
        assert launched <= f32_kernels, (record, launched - f32_kernels)
    # the stock step's strided launches (7x7 stem, stride-2 1x1 forward and weight gradient): each kernel that takes one has a strided case
    strided = {(e["entry"], e["kernel_id"]) for e in _recorded("stock_gemm_launches.json") if e["geometry"].get("stride", 1) > 1}
    assert strided == {("conv_fwd", 1), ("conv_fwd", 3), ("conv_fwd", 11), ("conv_wgrad", 4)}, strided
    assert strided <= {(c["entry"], c["kid"]) for c in CASES.CASES if c["geom"].get("stride", 1) == 2}
    for shape in CASES.BENCH_SHAPES:
        assert any(CASES.mnk(c) == shape[1:] and c["kid"] == shape[0] and "full_m" in c["variants"] for c in CASES.CASES), shape
    big = [c for c in CASES.CASES if "over_2gib" in c.get("variants", ())]
    assert {c["kid"] for c in big} >= {1, 3, 5, 6, 9}
    for c in CASES.CASES:          # every case says what it targets and where dispatch selects it
        assert c.get("why"), c["id"]


N_F32_CASES = 75       # the f32-operand block of the table: 59 cases, one per instantiation and epilogue set, and 16 more that the f32 records
                       # demanded; none may go without this changing


def test_f32_block_is_complete_and_leaves_the_bf16_table_in_place():
    """The cases before the f32 block keep their index (their seeds are 1000 + 2 * index + tier); the f32 block is all f32, runs in both
    tiers, adds no full-M and no over-2-GiB case, holds no two cases alike -- so that with the count above and REQUIRED_VARIANTS
    (one entry per f32 instantiation) a dropped case shows -- and covers each forward kernel under each epilogue set an f32 launch has."""
    n0 = CASES.N_BF16_TABLE
    assert n0 == 120 and CASES.CASES[0]["id"] == "fwd_1x1_plain" and CASES.CASES[n0 - 1]["id"] == "nt_rpn_sparse_dx"
    assert [c["id"] for c in CASES.CASES[:n0] if c["geom"]["dtype"] == "f32"] == ["fwd_f32_1x1", "fwd_f32_1x1_narrow", "stem_7x7_s2_f32",
                                                                                 "stem_7x7_s2_f32_even"]
    new = CASES.CASES[n0:]
    assert len(new) == N_F32_CASES
    seen = set()
    for c in new:
        assert c["geom"]["dtype"] == "f32" and c["tiers"] == CASES.AB and c["id"].startswith("f32_"), c["id"]
        assert not {"full_m", "over_2gib"} & set(c["variants"]), c["id"]
        assert c["variants"] and set(c["variants"]) <= set(CASES.REQUIRED_VARIANTS), c["id"]
        key = json.dumps([c["entry"], c["kid"], c["geom"], c["epi"], c["env"]], sort_keys=True)
        assert key not in seen, c["id"]
        seen.add(key)
        M, N, K = CASES.mnk(c)
        assert M * N * K * c["geom"].get("batch", 1) <= 1 << 32, (c["id"], "a new GPU test takes seconds: its float64 reference too")
        if c["entry"] == "conv_fwd":         # residuals and masks of an f32 launch are f32
            assert c["epi"]["residual"] in (None, "f32", "pooled"), c["id"]
    sets = {}
    for c in new:
        if c["entry"] == "conv_fwd" and c["geom"]["KH"] == 1 and c["geom"]["stride"] == 1 and not c["geom"]["pool"]:
            sets.setdefault(c["kid"], set()).add(CASES.launch_class(c["entry"], c["kid"], c["geom"], c["epi"])[-1])
    eight = {CASES.launch_class("conv_fwd", 1, CASES.conv32(1, 1, 1, 4, 4), e)[-1] for e in CASES._F32_SETS.values()}
    assert len(eight) == 8 and eight <= sets[1] and eight <= sets[3], (eight - sets[1], eight - sets[3])


# ------------------------------------------------------------------------------------------------ the dispatch, replayed on the CPU
SWITCHES = ("CDDMSL_GEMM256", "CDDMSL_FWD2", "CDDMSL_PERSIST", "CDDMSL_TAIL_SPLIT", "CDDMSL_SMALL_1X1", "CDDMSL_WGRAD_WS")
_PTR = 1 << 20          # stands for an operand: in plan-only mode the entry points validate, plan and return -- nothing reads it


def _plan_raw(L, entry, g, epi):
    """one entry point of the raw C ABI, with the arguments hip.py's wrapper would pass for this geometry and epilogue
    -> (status, cddmsl_last_kernel)"""
    dt = {"bf16": 0, "f32": 1}[g["dtype"]]
    es = 2 if dt == 0 else 4
    if entry in ("conv_fwd", "conv_wgrad"):
        N, H, W, Cin, Cout, KH, KW, s, p, pool = (g[k] for k in ("N", "H", "W", "Cin", "Cout", "KH", "KW", "stride", "pad", "pool"))
    if entry == "conv_fwd":
        opt = lambda on: _PTR if on else None
        if epi["emit8"]:
            st = L.cddmsl_conv_fwd_q8(_PTR, _PTR, _PTR, opt(epi["scale"]), opt(epi["bias"]), opt(epi["residual"]), opt(epi["relu_mask"]),
                                      N, H, W, Cin, Cout, KH, KW, s, p, int(epi["relu"]), _PTR, _PTR, _PTR, None)
        else:
            bits = int(epi["out_f32"]) | (2 if epi["residual"] == "f32" and dt == 0 else 0) | (4 if epi["residual"] == "pooled" else 0)
            st = L.cddmsl_conv_fwd(_PTR, _PTR, _PTR, opt(epi["scale"]), opt(epi["bias"]), opt(epi["residual"]), opt(epi["relu_mask"]),
                                   N, H, W, Cin, Cout, KH, KW, s, p, int(pool), Cout, Cout, Cout, int(epi["relu"]), bits, dt, None)
    elif entry == "conv_wgrad":
        st = L.cddmsl_conv_wgrad(_PTR, _PTR, _PTR, _PTR if epi["scale"] else None, N, H, W, Cin, Cout, KH, KW, s, p, int(pool), Cout, dt, None)
    elif entry == "gemm_nt_batched":
        off = lambda k: _PTR + g.get(k, 0) * es
        st = L.cddmsl_gemm_nt_batched(off("a_off"), off("b_off"), off("c_off"), None, g["M"], g["N"], g["K"], g["lda"], g["ldb"], g["ldc"],
                                      g["batch"], g["sa"], g["sw"], g["sc"], int(epi["out_f32"] and dt == 0), dt, None)
    elif entry == "gemm_tn_batched":
        mode = 0 if epi["accumulate"] else 1 if epi["out"] == "f32" else 2
        st = L.cddmsl_gemm_tn_batched(_PTR, _PTR, _PTR, g["M"], g["N"], g["K"], g["lda"], g["ldb"], g["ldo"], g["batch"], g["sa"], g["sb"],
                                      g["so"], mode, dt, None)
    else:
        raise AssertionError(f"the raw replay has no call for entry point {entry!r}")
    return st, L.cddmsl_last_kernel()


def test_dispatch_replayed_through_the_raw_abi_in_plan_only_mode(monkeypatch):
    """every launch recorded from the bench step, the stock step and their f32 twins, and every case of the GPU table -- under the case's switches, the others cleared --
    goes through the raw C ABI in plan-only mode (no GPU: validate, plan, return): status CDDMSL_OK and the recorded / expected
    kernel id.  Every entry point of the two tables has a raw call in _plan_raw (an unknown one fails there, it is not skipped)."""
    import __graft_entry__ as ge
    ge.build()
    from cddmsl_amd import hip
    L = hip._L()
    rec = _recorded("bench_gemm_launches.json")
    stock = _recorded("stock_gemm_launches.json")
    todo = [(f"recorded launch {i}", e["entry"], e["geometry"], e["epilogue"], {}, e["kernel_id"]) for i, e in enumerate(rec)]
    todo += [(f"recorded stock launch {i}", e["entry"], e["geometry"], e["epilogue"], {}, e["kernel_id"]) for i, e in enumerate(stock)]
    for record in F32_RECORDS:
        assert len(_recorded(record)) >= 40, record
        todo += [(f"{record} launch {i}", e["entry"], e["geometry"], e["epilogue"], {}, e["kernel_id"]) for i, e in enumerate(_recorded(record))]
    todo += [(c["id"], c["entry"], c["geom"], dict({"emit8": False}, **c["epi"]), c["env"], c["kid"]) for c in CASES.CASES]
    assert len(rec) >= 367 and len(stock) >= 58 and len(CASES.CASES) >= 120 + N_F32_CASES
    bad = []
    was = L.cddmsl_plan_only(1)
    try:
        for name, entry, g, epi, env, kid in todo:
            for k in SWITCHES:
                monkeypatch.delenv(k, raising=False)
            for k, v in env.items():
                monkeypatch.setenv(k, v)
            st, got = _plan_raw(L, entry, g, epi)
            if (st, got) != (0, kid):
                bad.append((name, entry, g, epi, env, f"status {st}, kernel {got}, expected {kid}"))
    finally:
        L.cddmsl_plan_only(was)
    assert not bad, bad
