"""The OCP e4m3 (fp8) kernels against the exact float64 product of the bytes they were given (tests/exact_fp8.py), for every case
of tests/fp8_exact_cases.py -- every instantiation of k_conv_fwd256<fp8e4> (kernel id 10), k_wgrad256_f8 (12) on its 1x1 / 3x3 /
atomics / strided-dy paths, the e4m3 second output of the bf16 256x256 kernel (cddmsl_conv_fwd_q8), k_fp8_dot_nt -- in two tiers:

  A  integer operands |v| <= 4 as e4m3 bytes, power-of-two scales, dyadic bias / residual / dW: every partial sum is exact in f32
     (and in the instruction: tools/mfma_f8_probe.hip pattern (d)), so the output must equal the exact value rounded once.
  B  Gaussian operands quantised to a maximum of 448: every element inside exact_fp8.check_bound, a bf16 store without bias.

Every case asserts the dispatched kernel id, keeps sentinels behind every output, and runs twice for identical bits (the f32
atomics of CDDMSL_WGRAD_WS=0 excepted).  Then the quantiser on every bf16 bit pattern and every e4m3 tie, the non-finite policy of
every e4m3 emitter, the single-instruction patterns of the probe through k_fp8_dot_nt, and what the entry points refuse."""
import math

import pytest
import torch

import exact_fp8 as F
import exact_gemm as X
import exact_roi as XR
import fp8_exact_cases as T

pytestmark = pytest.mark.gpu

DEV = "cuda"
PAD = 4096                           # sentinel elements behind every output
ROW_SAMPLE_ABOVE = 200_000
SWITCHES = ("CDDMSL_GEMM256", "CDDMSL_FWD2", "CDDMSL_PERSIST", "CDDMSL_TAIL_SPLIT", "CDDMSL_SMALL_1X1", "CDDMSL_WGRAD_WS")
KNAME = {10: "k_conv_fwd256<fp8e4>", 12: "k_wgrad256_f8", 3: "k_conv_fwd256<bf16> + y8", None: "k_fp8_dot_nt"}
WORST, ACC, MFMA = {}, {}, {}
ERR_ARG = 1


def _table_lines():
    """per kernel the worst |err| / bound, and over the f32 outputs the worst acc_ratio (exact_fp8.acc_ratio: what C_ACC covers) and
    the worst error in units of |s| sum_g max|a b| (what T_MFMA covers)"""
    lines = ["", f"worst |err| / bound per kernel (T_MFMA {F.T_MFMA:.4g}, C_ACC {F.C_ACC:g}):"]
    for k in sorted(WORST):
        lines.append(f"  {k:28s} err/bound {WORST[k]:.3f}   acc_ratio {ACC.get(k, float('nan')):.4g}   mfma_ratio {MFMA.get(k, float('nan')):.4g}")
    return lines


@pytest.fixture(scope="module", autouse=True)
def _worst_ratio_table():
    """collects the worst figures of this module's tier B cases; test_worst_ratio_table, the module's last test, prints them
    (shown without -s); this fixture prints them again at teardown for a run with -s that selected cases only"""
    WORST.clear(), ACC.clear(), MFMA.clear()
    yield
    if WORST:
        print("\n".join(_table_lines()))


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def _hip():
    from cddmsl_amd import hip
    hip.ensure_workspace(DEV)
    return hip


def _set_env(monkeypatch, env):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _kid():
    return int(_hip()._L().cddmsl_last_kernel())


def _ints(shape, lo, hi, g, dtype=torch.float32):
    return torch.randint(lo, hi + 1, shape, device=DEV, generator=g, dtype=torch.int16).to(dtype)


def _pow2(n, g):
    return torch.pow(2.0, torch.randint(-2, 2, (n,), device=DEV, generator=g).float())


_SENT = {torch.bfloat16: (torch.int16, 0x7FC1), torch.float32: (torch.int32, 0x7FC00001), torch.uint8: (torch.uint8, 0xA5)}


def _buffer(n, dtype):
    """n elements + PAD behind them, all set to a sentinel bit pattern"""
    b = torch.empty(n + PAD, device=DEV, dtype=dtype)
    it, v = _SENT[dtype]
    b.view(it).fill_(v)
    return b


def _tail_ok(b, n):
    it, v = _SENT[b.dtype]
    return bool((b.view(it)[n:] == v).all())


def _bits(t):
    return t.view(_SENT[t.dtype][0])


def _note(c, ratio, acc=None, mf=None):
    k = KNAME[c["kid"]]
    WORST[k] = max(WORST.get(k, 0.0), ratio)
    if acc is not None:
        ACC[k] = max(ACC.get(k, 0.0), acc)
    if mf is not None:
        MFMA[k] = max(MFMA.get(k, 0.0), mf)


def _report(c, tier, **kv):
    return f"[{c['id']} tier {tier}] {KNAME[c['kid']]} ({c['why']}): " + ", ".join(f"{k} {v}" for k, v in kv.items())


def _judge(c, tier, got, exact, absp, gterm, odt, scale=None, bias=None, residual=None, base=None):
    """tier A: bit-equal to the exact value rounded once; tier B: inside the bound, unbiased bf16 rounding.  gterm None: bf16
    operands (exact_gemm's bound).  -> (report line, pre-rounding bound)"""
    if gterm is None:
        pre = X.bound(torch.zeros_like(exact), absp, torch.float32, scale, bias, residual, base) / (1.0 + X.U_F32)
    else:
        pre = F.pre_bound(absp, gterm, scale, bias, residual, base)
    if tier == "A":
        assert float(absp.max()) < 2 ** 24, "tier A data must keep every partial sum exact in f32"
        assert torch.equal(X._f64(exact), X._f64(X._f64(exact).float())), "tier A exact value must be an f32 number"
        want = X.round_bf16(exact) if odt == torch.bfloat16 else X._f64(X._f64(exact).float())
        nbad = int((X._f64(got) != want).sum())
        line = _report(c, tier, bit_exact=nbad == 0, elements=got.numel(), mismatches=nbad)
        assert nbad == 0, f"{nbad} of {got.numel()} elements differ from the exact result rounded once"
        return line, pre
    if gterm is None:
        ok, ratio, worst = X.check_bound(got, exact, absp, odt, scale, bias, residual, base)
    else:
        ok, ratio, worst = F.check_bound(got, exact, absp, gterm, odt, scale, bias, residual, base)
    kv = dict(worst_err_over_bound=f"{ratio:.3g}", elements=got.numel())
    acc = mf = None
    if odt == torch.bfloat16:
        rb, n = X.rounding_bias(got, exact, absp, scale)
        kv.update(rounding_bias=f"{rb:+.4f}", bias_elements=n)
    else:
        if gterm is None:
            acc = X.acc_ratio(got, exact, absp, scale, bias, residual, base)
        else:
            acc, mf = F.acc_ratio(got, exact, absp, gterm, scale, bias, residual, base), F.mfma_ratio(got, exact, gterm, scale)
            kv.update(mfma_ratio=f"{mf:.4g}", raw_acc_ratio=f"{X.acc_ratio(got, exact, absp, scale, bias, residual, base):.4g}")
        kv.update(acc_ratio=f"{acc:.4g}")
    _note(c, ratio, acc, mf)
    line = _report(c, tier, **kv)
    g, e = X._f64(got).reshape(-1)[worst], X._f64(exact).reshape(-1)[worst]
    assert ok, f"element {worst}: got {float(g)!r}, exact {float(e)!r}, |err| / bound = {ratio:.3g}"
    if odt == torch.bfloat16:
        assert n >= 1000, f"rounding bias counted over {n} elements only"
        assert abs(rb) <= 0.05, f"bf16 rounding bias {rb:+.4f} ulp over {n} elements (RNE gives ~0, truncation -0.5)"
    return line, pre


def _check_emit8(c, tier, y8, amax, exact, pre, q8, rows=None):
    """the e4m3 second output and the recorded maximum against the UNROUNDED value"""
    if tier == "A":
        want = F.e4m3_encode(X._f64(exact) * float(q8))
        nbad = F.same_codes(y8, want)
        bad = (y8 != want).reshape(-1).nonzero().reshape(-1)[:6]
        show = [(float(exact.reshape(-1)[i]) * float(q8), hex(int(y8.reshape(-1)[i])), hex(int(want.reshape(-1)[i]))) for i in bad] if nbad else []
        assert nbad == 0, f"{nbad} e4m3 bytes differ from e4m3_rne(exact * q8): (value, got, want) {show}"
        if rows is None:
            assert float(amax.max()) == float(X._f64(exact).abs().max()), (float(amax.max()), float(X._f64(exact).abs().max()))
        return
    ok, ratio, worst = XR.check_e4m3(y8.reshape(exact.shape), exact, pre, float(q8))
    assert ok, f"y8 element {worst}: |err| / bound = {ratio:.3g}"
    if rows is None:
        ok, got, lo, hi = XR.check_amax(amax, exact, pre)
        assert ok, f"amax8 {got!r} outside [{lo!r}, {hi!r}]"


# ------------------------------------------------------------------------------------------------ forward convolutions
def _epilogue_operands(tier, e, M, Cout, K, gen, sigma2=1e4):
    """scale / bias / residual / mask of a forward case.  Tier B scales put the outputs near 1 (operands have sigma ~ 100)."""
    scale = bias = res = msk = None
    if tier == "A":
        scale = _pow2(Cout, gen) if e["scale"] else None
        bias = (_ints((Cout,), -64, 64, gen) / 8) if e["bias"] else None
        if e["residual"]:
            res = (_ints((M, Cout), -16, 16, gen) / 4).to(torch.bfloat16)
        if e["relu_mask"]:
            msk = _ints((M, Cout), -1, 1, gen, torch.bfloat16)
    else:
        scale = ((torch.rand(Cout, device=DEV, generator=gen) + 0.5) * (K ** -0.5 / sigma2)) if e["scale"] else None
        bias = (torch.randn(Cout, device=DEV, generator=gen) * 0.1) if e["bias"] else None
        if e["residual"]:
            res = torch.randn(M, Cout, device=DEV, generator=gen).to(torch.bfloat16)
        if e["relu_mask"]:
            msk = torch.randn(M, Cout, device=DEV, generator=gen).to(torch.bfloat16)
    return scale, bias, res, msk


def _launch_fwd(entry, x, w, scale, bias, res, msk, g, e, q8, M):
    """one launch through the C ABI into sentinel-backed buffers -> (y buffer, y8 buffer or None, amax or None)"""
    hip = _hip()
    from cddmsl_amd.hip import ptr, stream_ptr
    L = hip._L()
    N, H, W, Cin, Cout, KH, KW, pad = (g[k] for k in ("N", "H", "W", "Cin", "Cout", "KH", "KW", "pad"))
    y = _buffer(M * Cout, torch.float32 if e["out_f32"] else torch.bfloat16)
    y8 = _buffer(M * Cout, torch.uint8) if e["emit8"] else None
    amax = torch.zeros(64, device=DEV) if e["emit8"] else None
    if entry == "conv_fwd_fp8":
        st = L.cddmsl_conv_fwd_fp8(ptr(x), ptr(w), ptr(y), ptr(scale), ptr(bias), ptr(res), ptr(msk), N, H, W, Cin, Cout, KH, KW, pad,
                                   int(e["relu"]), int(e["out_f32"]), ptr(y8), ptr(q8 if e["emit8"] else None), ptr(amax), stream_ptr())
    else:
        st = L.cddmsl_conv_fwd_q8(ptr(x), ptr(w), ptr(y), ptr(scale), ptr(bias), ptr(res), ptr(msk), N, H, W, Cin, Cout, KH, KW, 1, pad,
                                  int(e["relu"]), ptr(y8), ptr(q8), ptr(amax), stream_ptr())
    assert st == 0, st
    return y, y8, amax


def _run_fwd(c, tier, seed):
    g, e = c["geom"], c["epi"]
    N, H, W, Cin, Cout, KH, KW, pad = (g[k] for k in ("N", "H", "W", "Cin", "Cout", "KH", "KW", "pad"))
    Ho, Wo = X.out_geometry(H, W, KH, KW, 1, pad, False)
    M, K = N * Ho * Wo, KH * KW * Cin
    gen = _gen(seed)
    fp8 = c["entry"] == "conv_fwd_fp8"
    if fp8:
        mk = (lambda s: F.tier_a_operand(s, K, gen, DEV)) if tier == "A" else (lambda s: F.tier_b_operand(s, gen, DEV))
        x, w = mk((N, H, W, Cin)), mk((Cout, KH, KW, Cin))
        big = M > ROW_SAMPLE_ABOVE
        xd, wd = F.deq(x, torch.float32 if big else torch.float64), F.deq(w)
        scale, bias, res, msk = _epilogue_operands(tier, e, M, Cout, K, gen)
    else:                     # bf16 operands (the e4m3 second output of the bf16 kernel)
        if tier == "A":
            x, w = _ints((N, H, W, Cin), -3, 3, gen, torch.bfloat16), _ints((Cout, KH, KW, Cin), -3, 3, gen, torch.bfloat16)
        else:
            x = torch.randn(N, H, W, Cin, device=DEV, generator=gen).to(torch.bfloat16)
            w = (torch.randn(Cout, KH, KW, Cin, device=DEV, generator=gen) * K ** -0.5).to(torch.bfloat16)
        xd, wd = x, w
        scale, bias, res, msk = _epilogue_operands(tier, e, M, Cout, K, gen, sigma2=K ** -0.5)      # (scale ~ 1: the outputs already are)
    q8 = torch.tensor([0.5 if tier == "A" else 100.0], device=DEV)
    y, y8, amax = _launch_fwd(c["entry"], x, w, scale, bias, res, msk, g, e, q8, M)
    assert _kid() == c["kid"], (_kid(), c["kid"])
    y2, y82, amax2 = _launch_fwd(c["entry"], x, w, scale, bias, res, msk, g, e, q8, M)
    torch.cuda.synchronize()
    assert _tail_ok(y, M * Cout) and (y8 is None or _tail_ok(y8, M * Cout)), "bytes behind the output were written"
    assert torch.equal(_bits(y), _bits(y2)), "two runs differ"
    if y8 is not None:
        assert torch.equal(y8, y82) and torch.equal(amax.max(), amax2.max()), "two runs differ in y8 / amax8"
    del y2, y82
    if not fp8:               # y bit-equal to the launch without the second output
        hip = _hip()
        plain = hip.conv_fwd(x, w, scale, bias, None if res is None else res.view(N, Ho, Wo, Cout), e["relu"],
                             None if msk is None else msk.view(N, Ho, Wo, Cout), 1, pad)
        assert _kid() == 3 and torch.equal(_bits(plain.reshape(-1)), _bits(y[:M * Cout])), "y differs from the launch without emit8"
    rows = X.sample_rows(M, [Cout * y.element_size(), Cin], device=DEV, seed=seed) if M > ROW_SAMPLE_ABOVE else None
    acc, absp = X.conv_exact(xd, wd, 1, pad, rows=rows)
    gterm = F.conv_group_term(xd, wd, pad, rows) if fp8 else None
    sel = (lambda t: t[:M * Cout].view(M, Cout)) if rows is None else (lambda t: t[:M * Cout].view(M, Cout)[rows])
    r_rows = None if res is None else X._f64(sel(res.reshape(-1)))
    m_rows = None if msk is None else sel(msk.reshape(-1))
    exact = X.epilogue_exact(acc, scale, bias, r_rows, e["relu"], m_rows)
    line, pre = _judge(c, tier, sel(y), exact, absp, gterm, y.dtype, scale, bias, None if r_rows is None else r_rows.abs())
    if y8 is not None:
        _check_emit8(c, tier, sel(y8), amax, exact, pre, q8, rows)
    return line


# ------------------------------------------------------------------------------------------------ weight gradient
def _run_wgrad(c, tier, seed):
    hip = _hip()
    from cddmsl_amd.hip import ptr, stream_ptr
    L = hip._L()
    g, e = c["geom"], c["epi"]
    N, H, W, Cin, Cout, KH, KW, pad = (g[k] for k in ("N", "H", "W", "Cin", "Cout", "KH", "KW", "pad"))
    M, ldd = N * H * W, Cout + e["ldd_extra"]
    gen = _gen(seed)
    big = M > ROW_SAMPLE_ABOVE
    mk = (lambda s: F.tier_a_operand(s, M, gen, DEV)) if tier == "A" else (lambda s: F.tier_b_operand(s, gen, DEV))
    x, d = mk((N, H, W, Cin)), mk((M, Cout))
    dbuf = torch.full((M, ldd), 0x7F, device=DEV, dtype=torch.uint8)          # the gap between rows: NaN codes
    dbuf[:, :Cout] = d
    if tier == "A":
        scale = _pow2(Cout, gen) if e["scale"] else torch.ones(Cout, device=DEV)
        base = _ints((Cout, KH * KW, Cin), -100, 100, gen)
    else:
        scale = ((torch.rand(Cout, device=DEV, generator=gen) + 0.5) * (M ** -0.5 / 1e4)) if e["scale"] else torch.ones(Cout, device=DEV)
        base = torch.randn(Cout, KH * KW, Cin, device=DEV, generator=gen) * (1.0 if e["scale"] else 1e4 * M ** 0.5)
    n = base.numel()

    def launch():
        out = _buffer(n, torch.float32)
        out[:n] = base.reshape(-1)
        st = L.cddmsl_conv_wgrad_fp8(ptr(x), ptr(dbuf), ptr(out), ptr(scale), N, H, W, Cin, Cout, KH, KW, pad, ldd, stream_ptr())
        assert st == 0, st
        return out
    out = launch()
    assert _kid() == c["kid"], (_kid(), c["kid"])
    out2 = launch()
    torch.cuda.synchronize()
    assert _tail_ok(out, n), "floats behind dW were written"
    atomics = c["env"].get("CDDMSL_WGRAD_WS") == "0"
    if not atomics:
        assert torch.equal(_bits(out), _bits(out2)), "two runs differ"
    del out2
    taps = [(kh, kw) for kh in range(KH) for kw in range(KW)]
    nsel = torch.arange(Cout, device=DEV)
    if big:                   # a bench launch: corner and centre taps, 16 of the output channels, every input channel -- each the full reduction
        taps = [taps[0], taps[len(taps) // 2], taps[-1]]
        nsel = torch.randperm(Cout, device=DEV, generator=gen)[:16].sort().values
    xd, dd = F.deq(x, torch.float32), F.deq(d[:, nsel], torch.float32).view(N, H, W, len(nsel))
    acc, absp = X.wgrad_exact(xd, dd, KH, KW, 1, pad, taps=taps)
    gterm = F.wgrad_group_term(xd, dd, KH, KW, pad, taps=taps)
    ti = torch.tensor([kh * KW + kw for kh, kw in taps], device=DEV)
    got = out[:n].view(Cout, KH * KW, Cin)[nsel][:, ti]
    sc = scale[nsel].view(-1, 1, 1)
    bsel = X._f64(base[nsel][:, ti])
    exact = acc * X._f64(sc) + bsel
    line, _ = _judge(c, tier, got, exact, absp, gterm, torch.float32, sc, None, None, bsel.abs())
    return line


# ------------------------------------------------------------------------------------------------ fp8_dot_nt
def _dot(a8, b8, alpha, ldc):
    """c [R, ldc] (+ PAD) through the C ABI; the columns >= N and the tail keep their sentinel"""
    hip = _hip()
    from cddmsl_amd.hip import ptr, stream_ptr
    R, K = a8.shape
    N = b8.shape[0]
    c = _buffer(R * ldc, torch.float32)
    st = hip._L().cddmsl_fp8_dot_nt(ptr(a8), ptr(b8), ptr(c), ptr(alpha), R, N, K, ldc, stream_ptr())
    assert st == 0, st
    torch.cuda.synchronize()
    body = c[:R * ldc].view(R, ldc)
    assert _tail_ok(c, R * ldc) and bool((_bits(body[:, N:]) == _SENT[torch.float32][1]).all()), "sentinel columns were written"
    return body[:, :N]


def _run_dot(c, tier, seed):
    g = c["geom"]
    R, N, K, ldc = g["R"], g["N"], g["K"], g["ldc"]
    gen = _gen(seed)
    mk = (lambda s: F.tier_a_operand(s, K, gen, DEV)) if tier == "A" else (lambda s: F.tier_b_operand(s, gen, DEV))
    a8, b8 = mk((R, K)), mk((N, K))
    ad, bd = F.deq(a8), F.deq(b8)
    acc, absp, gterm = ad @ bd.t(), ad.abs() @ bd.abs().t(), F.dot_group_term(ad, bd)
    line = None
    for alpha in (None, torch.tensor([0.125 if tier == "A" else 0.37 / 1e4], device=DEV)):
        got = _dot(a8, b8, alpha, ldc)
        assert torch.equal(_bits(got.contiguous()), _bits(_dot(a8, b8, alpha, ldc).contiguous())), "two runs differ"
        s = None if alpha is None else alpha.view(1, 1)
        exact = acc if alpha is None else acc * X._f64(alpha)
        line, _ = _judge(c, tier, got, exact, absp, gterm, torch.float32, s)
    return line


_RUN = {"conv_fwd_fp8": _run_fwd, "conv_fwd_q8": _run_fwd, "conv_wgrad_fp8": _run_wgrad, "fp8_dot_nt": _run_dot}
_PARAMS = [pytest.param(c, t, id=f"{c['id']}-{t}") for c in T.CASES for t in c["tiers"]]


@pytest.mark.parametrize("c,tier", _PARAMS)
def test_exact_product(c, tier, monkeypatch, capsys):
    _set_env(monkeypatch, c["env"])
    try:
        line = _RUN[c["entry"]](c, tier, seed=5000 + T.CASES.index(c) * 2 + (tier == "B"))
    finally:
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
    if c["kid"] is not None:
        with capsys.disabled():
            print("\n" + line)


def test_recorded_fp8_launches_keep_their_kernels(monkeypatch, golden_dir, capsys):
    """every distinct e4m3 launch of the bench step (tests/golden/bench_fp8_launches.json, tools/record_gemm_launches.py --dtype fp8)
    still dispatches to the kernel recorded for it: replayed in plan-only mode on right-sized, uninitialised tensors"""
    import json
    import os
    hip = _hip()
    _set_env(monkeypatch, {})
    with open(os.path.join(golden_dir, "bench_fp8_launches.json")) as fh:
        rec = [e for e in json.load(fh)["entries"] if e["entry"] != "fp8_dot_nt"]        # (one kernel, no dispatch)
    L = hip._L()
    bad = []
    for e in rec:
        g, epi = e["geometry"], e["epilogue"]
        N, H, W, Cin, Cout, KH, KW, pad = (g[k] for k in ("N", "H", "W", "Cin", "Cout", "KH", "KW", "pad"))
        op = torch.uint8 if g["dtype"] == "e4m3" else torch.bfloat16
        x, vec = torch.empty(N, H, W, Cin, device=DEV, dtype=op), torch.ones(Cout, device=DEV)
        L.cddmsl_plan_only(1)
        try:
            if e["entry"] == "conv_wgrad_fp8":
                hip.conv_wgrad_fp8(x, torch.empty(N, H, W, Cout, device=DEV, dtype=op), (Cout, KH, KW, Cin), vec, pad,
                                   out=torch.empty(Cout, KH, KW, Cin, device=DEV))
            else:
                w = torch.empty(Cout, KH, KW, Cin, device=DEV, dtype=op)
                Ho, Wo = X.out_geometry(H, W, KH, KW, 1, pad, False)
                side = lambda on: torch.empty(N, Ho, Wo, Cout, device=DEV, dtype=torch.bfloat16) if on else None
                e8 = (torch.ones(1, device=DEV), torch.zeros(64, device=DEV)) if epi["emit8"] else None
                args = (x, w, vec if epi["scale"] else None, vec if epi["bias"] else None, side(epi["residual"]), epi["relu"], side(epi["relu_mask"]))
                if e["entry"] == "conv_fwd_fp8":
                    hip.conv_fwd_fp8(*args, pad=pad, emit8=e8)
                else:
                    hip.conv_fwd(*args, stride=1, pad=pad, emit8=e8)
        finally:
            L.cddmsl_plan_only(0)
        if _kid() != e["kernel_id"]:
            bad.append((e["entry"], g, epi, e["kernel_id"], _kid()))
        del x
        torch.cuda.empty_cache()
    with capsys.disabled():
        print(f"\n{len(rec)} recorded e4m3 launches replayed in plan-only mode, {len(bad)} changed kernel")
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ the instruction, through the library
def _codes(values):
    return F.e4m3_encode(torch.as_tensor(values, dtype=torch.float64, device=DEV))


def test_mfma_patterns_through_fp8_dot_nt(capsys):
    """the patterns of tools/mfma_f8_probe.hip through k_fp8_dot_nt: with K = 64 every output is ONE instruction on a zero
    accumulator, and its error must stay within T_MFMA of the largest product (plus the f32 rounding of the result); with
    K = 128 the second instruction adds to the first one's result.  A different chip or compiler shows up here."""
    gen = _gen(77)
    worst = {}

    def run(name, a8, b8, exact_only=False):
        ad, bd = F.deq(a8), F.deq(b8)
        exact, gterm = ad @ bd.t(), F.dot_group_term(ad, bd)
        got = X._f64(_dot(a8, b8, None, b8.shape[0] + 3))
        err = (got - exact).abs()
        if exact_only:
            assert float(err.max()) == 0.0, (name, float(err.max()))
            return
        r = F.mfma_ratio(got, exact, gterm)
        worst[name] = max(worst.get(name, 0.0), r)
        assert r <= F.T_MFMA, (name, r, F.T_MFMA)

    for K in (64, 128):
        # (a) random finite codes, and Gaussian operands
        ra = torch.randint(0, 256, (4096, K), device=DEV, generator=gen, dtype=torch.int16)
        rb = torch.randint(0, 256, (32, K), device=DEV, generator=gen, dtype=torch.int16)
        fix = lambda t: torch.where((t & 0x7F) == 0x7F, t & 0x80, t).to(torch.uint8)
        run(f"(a) codes K={K}", fix(ra), fix(rb))
        run(f"(a) gauss K={K}", F.tier_b_operand((4096, K), gen, DEV), F.tier_b_operand((32, K), gen, DEV))
        # (b) one product of 2^j among products of 1 and of 1.125^2, the large one at k0
        for small in (1.0, 1.125):
            for j in range(17):
                a = torch.full((32, K), small, dtype=torch.float64, device=DEV)
                b = torch.full((32, K), small, dtype=torch.float64, device=DEV)
                k0 = (7 * j) % K
                a[:, k0], b[:, k0] = 2.0 ** (j // 2), 2.0 ** (j - j // 2)
                b[1::2, k0] *= -1
                run(f"(b) small {small} K={K}", _codes(a), _codes(b))
        # (d) the tier A regime
        run(f"(d) K={K}", F.tier_a_operand((4096, K), K, gen, DEV), F.tier_a_operand((32, K), K, gen, DEV), exact_only=True)
    # (c) K = 128: the first instruction leaves 2^j in the accumulator, the second adds 64 products of 1 / of 2^-9
    for small in (1.0, 2.0 ** -9):
        for j in range(17):
            a = torch.zeros(32, 128, dtype=torch.float64, device=DEV)
            b = torch.ones(32, 128, dtype=torch.float64, device=DEV)
            a[:, 5], b[:, 5] = 2.0 ** (j // 2), 2.0 ** (j - j // 2)
            a[:, 64:] = small
            a8, b8 = _codes(a), _codes(b)
            ad, bd = F.deq(a8), F.deq(b8)
            exact = ad @ bd.t()
            got = _dot(a8, b8, None, 35)
            ok, ratio, _ = F.check_bound(got, exact, ad.abs() @ bd.abs().t(), F.dot_group_term(ad, bd), torch.float32)
            worst["(c) err/bound"] = max(worst.get("(c) err/bound", 0.0), ratio)
            assert ok, (small, j, ratio)
    with capsys.disabled():
        print("\nsingle-instruction patterns through k_fp8_dot_nt, worst error / largest product (T_MFMA %.4g):" % F.T_MFMA)
        for k in sorted(worst):
            print(f"  {k:28s} {worst[k]:.4g}")


# ------------------------------------------------------------------------------------------------ the quantiser
def _quantize(x, scale=None, amax=True):
    """-> (codes [numel], amax slots or None), through the C ABI into a sentinel-backed buffer"""
    hip = _hip()
    from cddmsl_amd.hip import ptr, stream_ptr
    n = x.numel()
    y = _buffer(n, torch.uint8)
    am = torch.zeros(64, device=DEV) if amax else None
    s = None if scale is None else torch.tensor([scale], device=DEV, dtype=torch.float32)
    st = hip._L().cddmsl_quantize_fp8(ptr(x), ptr(y), ptr(s), ptr(am), n, 0 if x.dtype == torch.bfloat16 else 1, stream_ptr())
    assert st == 0, st
    torch.cuda.synchronize()
    assert _tail_ok(y, n), "bytes behind the output were written"
    return y[:n], am


def _want_codes(x, scale):
    """e4m3_rne of the f32 product the kernel forms (x * scale in f32), with the non-finite policy: NaN and -Inf -> the code of
    -448, +Inf -> the code of +448 (pack4_e4m3 clamps with fmaxf / fminf, which return the operand that is not NaN)"""
    t = x.float() * torch.tensor(1.0 if scale is None else scale, dtype=torch.float32, device=x.device)
    want = F.e4m3_encode(t.double())
    return torch.where(torch.isnan(t), torch.full_like(want, 0xFE), want)


@pytest.mark.parametrize("scale", [None, 0.37, 448.0 / 3.0])
def test_quantiser_on_every_bf16_bit_pattern(scale):
    bits = torch.arange(65536, dtype=torch.int32, device=DEV).to(torch.int16)
    x = bits.view(torch.bfloat16)
    got, am = _quantize(x, scale)
    want = _want_codes(x, scale)
    assert F.same_codes(got, want) == 0, F.same_codes(got, want)
    assert not bool(torch.isfinite(am.max()))              # (the patterns hold NaN and Inf: the record says so)
    fin = x[torch.isfinite(x.float())]
    fin = fin[:fin.numel() // 8 * 8]
    got, am = _quantize(fin, scale)
    assert F.same_codes(got, _want_codes(fin, scale)) == 0
    assert float(am.max()) == float(fin.float().abs().max())


def test_quantiser_ties_to_even_on_f32_midpoints():
    m = F.midpoints_f32().to(DEV)
    m = torch.cat([m, torch.zeros((-m.numel()) % 8, device=DEV)])
    got, am = _quantize(m, None)
    assert F.same_codes(got, F.e4m3_encode(m.double())) == 0
    assert float(am.max()) == float(m.abs().max())


@pytest.mark.parametrize("numel", [8, 2048 * 256 * 8 + 8 * 300])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_quantiser_sizes(numel, dtype):
    """one chunk; and more than 2048 blocks' worth, so the grid-stride loop runs a second round (its last chunk included)"""
    x = (torch.randn(numel, device=DEV, generator=_gen(numel)) * 40.0).to(dtype)
    x[-1], x[-8] = 300.0, -2.0 ** -9
    got, am = _quantize(x, 1.7)
    want = _want_codes(x, 1.7)
    assert F.same_codes(got, want) == 0
    assert F.same_codes(got[-8:], want[-8:]) == 0
    assert float(am.max()) == float(x.float().abs().max())


def test_non_finite_policy_of_every_emitter(monkeypatch):
    """NaN and -Inf become the code of -448 (0xFE), +Inf the code of +448 (0x7E) -- what pack4_e4m3's clamp makes of them in fp8.hip
    (fminf(fmaxf(x, -448), 448)) and in conv_fwd256.hip (v_med3_f32, which returns the smallest operand when one is NaN) -- and the
    recorded maximum is non-finite.  Produced by a NaN / Inf in the input or the bias, never by a fault."""
    hip = _hip()
    x = torch.randn(4096, device=DEV)
    x[77], x[99], x[1234] = float("nan"), float("inf"), float("-inf")
    for src in (x, x.bfloat16()):
        got, am = _quantize(src, 0.5)
        assert (int(got[77]), int(got[99]), int(got[1234])) == (0xFE, 0x7E, 0xFE), [hex(int(got[i])) for i in (77, 99, 1234)]
        assert not bool(torch.isfinite(am.max()))
        keep = torch.isfinite(x)
        assert F.same_codes(got[keep], _want_codes(src, 0.5)[keep]) == 0
    gen = _gen(9)
    g8, gb = T.conv8(1, 5, 8, 256, 256), T.conv8(1, 5, 8, 256, 256, dtype="bf16")
    e = T.fwd(True, True, emit8=True)
    bias = torch.randn(256, device=DEV, generator=gen)
    bias[3], bias[5], bias[7] = float("nan"), float("inf"), float("-inf")
    scale = torch.full((256,), 1e-6, device=DEV)
    q8 = torch.tensor([2.0], device=DEV)
    _set_env(monkeypatch, T.F256)
    for entry, g, x_, w_ in (("conv_fwd_fp8", g8, F.tier_b_operand((1, 5, 8, 256), gen, DEV), F.tier_b_operand((256, 1, 1, 256), gen, DEV)),
                             ("conv_fwd_q8", gb, torch.randn(1, 5, 8, 256, device=DEV, generator=gen).bfloat16(),
                              torch.randn(256, 1, 1, 256, device=DEV, generator=gen).bfloat16())):
        y, y8, am = _launch_fwd(entry, x_, w_, scale, bias, None, None, g, e, q8, 40)
        torch.cuda.synchronize()
        assert _kid() == (10 if entry == "conv_fwd_fp8" else 3)
        y8 = y8[:40 * 256].view(40, 256)
        assert bool((y8[:, 3] == 0xFE).all()) and bool((y8[:, 5] == 0x7E).all()) and bool((y8[:, 7] == 0xFE).all()), \
            (entry, [hex(int(v)) for v in y8[0, :8]])
        assert not bool(torch.isfinite(am.max())), entry
        yv = y[:40 * 256].view(40, 256).float()
        # (y itself: the ReLU floor is a v_max_f32 against -Inf when there is no ReLU, which returns the operand that is not NaN,
        # so today the NaN column is stored as -Inf; what is pinned is that it is not finite)
        assert not bool(torch.isfinite(yv[:, 3]).any()) and bool((yv[:, 5] == math.inf).all()) and bool((yv[:, 7] == -math.inf).all())
        cols = torch.tensor([c for c in range(256) if c not in (3, 5, 7)], device=DEV)
        assert bool(torch.isfinite(yv[:, cols]).all()) and bool(((y8[:, cols] & 0x7F) != 0x7F).all())
    # a NaN code among the e4m3 operands reaches every output of its row, unless the ReLU mask zeroes it
    x8 = F.tier_b_operand((1, 5, 8, 256), gen, DEV)
    x8.view(40, 256)[11, 100] = 0x7F
    msk = torch.randn(40, 256, device=DEV, generator=gen).bfloat16()
    y, y8, am = _launch_fwd("conv_fwd_fp8", x8, F.tier_b_operand((256, 1, 1, 256), gen, DEV), scale, None, None, msk, g8,
                            T.fwd(True, relu_mask=True, emit8=True), q8, 40)
    torch.cuda.synchronize()
    row = y8[:40 * 256].view(40, 256)[11]
    on = msk[11].float() > 0
    assert bool((row[on] == 0xFE).all()) and bool(((row[~on] & 0x7F) == 0).all()) and not bool(torch.isfinite(am.max()))


@pytest.mark.parametrize("entry", ["conv_fwd_fp8", "conv_fwd_q8"])
def test_amax8_of_a_ragged_panel(entry, monkeypatch):
    """M = 40 of a 256-row tile: the epilogue also runs on the 216 rows past M, whose accumulators, residual and mask read as zero.
    tile_epilogue documents that these rows "contribute their bias-only values: an over-estimate at worst" -- pinned here as
    exactly that and no more: with a bias that outweighs every real output, amax8 is max(max|y|, max_n |relu?(bias_n)|); with a
    ReLU mask (rows past M read a zero mask) it is max|y| alone.  Nothing past row M is written either way."""
    _set_env(monkeypatch, T.F256)
    gen = _gen(31)
    fp8 = entry == "conv_fwd_fp8"
    g = T.conv8(1, 5, 8, 256, 256, dtype="e4m3" if fp8 else "bf16")
    if fp8:
        x, w = F.tier_a_operand((1, 5, 8, 256), 256, gen, DEV), F.tier_a_operand((256, 1, 1, 256), 256, gen, DEV)
        xd, wd = F.deq(x), F.deq(w)
    else:
        x, w = _ints((1, 5, 8, 256), -3, 3, gen, torch.bfloat16), _ints((256, 1, 1, 256), -3, 3, gen, torch.bfloat16)
        xd, wd = x, w
    acc, _ = X.conv_exact(xd, wd)
    scale = torch.full((256,), 2.0 ** -6, device=DEV)
    bias = _ints((256,), -8, 8, gen)
    bias[0], bias[1] = 4096.0, -8192.0                    # channel 0 outweighs every output; channel 1 is negative: the ReLU takes it out
    res = torch.zeros(40, 256, device=DEV)
    res[:, 0], res[:, 1] = -4096.0, 8192.0                # ... and the real rows cancel both
    res = res.to(torch.bfloat16)
    q8 = torch.tensor([1.0], device=DEV)
    y, y8, am = _launch_fwd(entry, x, w, scale, bias, res, None, g, T.fwd(True, True, "bf16", True, emit8=True), q8, 40)
    torch.cuda.synchronize()
    assert _tail_ok(y, 40 * 256) and _tail_ok(y8, 40 * 256)
    exact = X.epilogue_exact(acc, scale, bias, X._f64(res), True)
    assert float(exact.abs().max()) < 4096.0
    assert float(am.max()) == 4096.0, float(am.max())
    msk = _ints((40, 256), -1, 1, gen, torch.bfloat16)
    y, y8, am = _launch_fwd(entry, x, w, scale, bias, res, msk, g, T.fwd(True, True, "bf16", True, relu_mask=True, emit8=True), q8, 40)
    torch.cuda.synchronize()
    exact = X.epilogue_exact(acc, scale, bias, X._f64(res), True, msk)
    assert float(am.max()) == float(exact.abs().max()), (float(am.max()), float(exact.abs().max()))


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_write_nothing(monkeypatch):
    """what the entry points do not take is CDDMSL_ERR_ARG with every output byte untouched"""
    hip = _hip()
    from cddmsl_amd.hip import ptr, stream_ptr
    L = hip._L()
    _set_env(monkeypatch, {})
    sp = stream_ptr

    def untouched(*bufs):
        torch.cuda.synchronize()
        return all(_tail_ok(b, 0) for b in bufs)

    # quantiser: numel % 8 != 0, a source dtype that does not exist
    x, y, am = torch.randn(64, device=DEV), _buffer(0, torch.uint8), _buffer(0, torch.float32)
    assert L.cddmsl_quantize_fp8(ptr(x), ptr(y), None, ptr(am), 60, 1, sp()) == ERR_ARG
    assert L.cddmsl_quantize_fp8(ptr(x), ptr(y), None, ptr(am), 64, 2, sp()) == ERR_ARG
    assert untouched(y, am)
    # fp8_dot_nt: N = 33, K = 96, ldc < N
    a8, b8, c = torch.zeros(64, 128, dtype=torch.uint8, device=DEV), torch.zeros(64, 128, dtype=torch.uint8, device=DEV), _buffer(0, torch.float32)
    assert L.cddmsl_fp8_dot_nt(ptr(a8), ptr(b8), ptr(c), None, 64, 33, 128, 33, sp()) == ERR_ARG
    assert L.cddmsl_fp8_dot_nt(ptr(a8), ptr(b8), ptr(c), None, 64, 20, 96, 20, sp()) == ERR_ARG
    assert L.cddmsl_fp8_dot_nt(ptr(a8), ptr(b8), ptr(c), None, 64, 20, 128, 19, sp()) == ERR_ARG
    assert untouched(c)
    # conv_fwd_fp8: Cin = 64, Cout = 128, pad 2 on a 3x3, out_f32 together with y8
    x8, w8 = torch.zeros(1 << 16, dtype=torch.uint8, device=DEV), torch.zeros(1 << 20, dtype=torch.uint8, device=DEV)
    yb, yf, y8 = _buffer(0, torch.bfloat16), _buffer(0, torch.float32), _buffer(0, torch.uint8)
    q8 = torch.ones(1, device=DEV)
    fwd8 = lambda y, Cin, Cout, K, pad, f32, e8: L.cddmsl_conv_fwd_fp8(ptr(x8), ptr(w8), ptr(y), None, None, None, None, 1, 4, 4, Cin, Cout, K, K, pad, 0, f32,
                                                                         ptr(y8) if e8 else None, ptr(q8) if e8 else None, ptr(am) if e8 else None, sp())
    assert fwd8(yb, 64, 256, 1, 0, 0, False) == ERR_ARG
    assert fwd8(yb, 128, 128, 1, 0, 0, False) == ERR_ARG
    assert fwd8(yb, 128, 256, 3, 2, 0, False) == ERR_ARG
    assert fwd8(yf, 128, 256, 1, 0, 1, True) == ERR_ARG
    assert untouched(yb, yf, y8, am)
    # conv_fwd_q8: a shape the 256x256 kernel does not take (Cout = 128), and one it takes but does not pick (too few tiles, nothing forced)
    xb, wb = torch.zeros(1 << 16, dtype=torch.bfloat16, device=DEV), torch.zeros(1 << 20, dtype=torch.bfloat16, device=DEV)
    q = lambda Cin, Cout: L.cddmsl_conv_fwd_q8(ptr(xb), ptr(wb), ptr(yb), None, None, None, None, 1, 4, 4, Cin, Cout, 1, 1, 1, 0, 0, ptr(y8), ptr(q8), ptr(am), sp())
    assert q(128, 128) == ERR_ARG and q(128, 256) == ERR_ARG
    monkeypatch.setenv("CDDMSL_GEMM256", "2")
    assert q(128, 128) == ERR_ARG
    assert untouched(yb, y8, am)
    # conv_wgrad_fp8: ldd < Cout
    dw = _buffer(0, torch.float32)
    sc = torch.ones(256, device=DEV)
    assert L.cddmsl_conv_wgrad_fp8(ptr(x8), ptr(w8), ptr(dw), ptr(sc), 1, 4, 4, 256, 256, 3, 3, 1, 240, sp()) == ERR_ARG
    assert L.cddmsl_conv_wgrad_fp8(ptr(x8), ptr(w8), ptr(dw), ptr(sc), 1, 4, 4, 256, 512, 1, 1, 0, 256, sp()) == ERR_ARG
    assert untouched(dw)


# ------------------------------------------------------------------------------------------------ the table (last test of the module)
def test_worst_ratio_table(capsys):
    """prints what the tier B cases above measured, per kernel, and holds every worst |err| / bound below 1 once more; says nothing
    when a selection ran none of them"""
    if not WORST:
        return
    with capsys.disabled():
        print("\n".join(_table_lines()))
    assert all(v < 1.0 for v in WORST.values()), WORST
