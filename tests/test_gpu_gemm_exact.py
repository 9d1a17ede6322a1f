"""bf16 convolution / GEMM kernels against the exact float64 product of the operands they were given (tests/exact_gemm.py), for
every case of tests/gemm_exact_cases.py -- every kernel family and instantiation, the bench's own launch shapes at full M and
the 32-image geometry past 2 GiB -- in two tiers:

  A  small-integer operands, power-of-two scales, dyadic bias / residual / dW: every partial sum is exact in f32 in any order
     (split-K, atomics, workspace reductions), so the output must equal the exact value rounded once -- torch.equal.
  B  Gaussian operands: every element inside exact_gemm.check_bound, and a bf16 store without rounding bias.

Plus the launch record (tests/golden/bench_gemm_launches.json) replayed in plan-only mode: dispatch still picks the recorded kernel."""
import json
import os

import pytest
import torch

import exact_gemm as X
import gemm_exact_cases as T

pytestmark = pytest.mark.gpu

DEV = "cuda"
ROW_SAMPLE_ABOVE = 200_000          # outputs with more rows are checked on exact_gemm.sample_rows
SWITCHES = ("CDDMSL_GEMM256", "CDDMSL_FWD2", "CDDMSL_PERSIST", "CDDMSL_TAIL_SPLIT", "CDDMSL_SMALL_1X1", "CDDMSL_WGRAD_WS")


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def _ints(shape, lo, hi, g, dtype=torch.bfloat16):
    return torch.randint(lo, hi + 1, shape, device=DEV, generator=g, dtype=torch.int16).to(dtype)


def _gauss(shape, g, dtype=torch.bfloat16, scale=1.0):
    out = torch.empty(shape, device=DEV, dtype=dtype)
    flat = out.view(-1)
    step = 1 << 28
    for i in range(0, flat.numel(), step):          # (in slices: the f32 temporary of a 3 GiB bf16 tensor stays small)
        n = min(step, flat.numel() - i)
        flat[i:i + n] = (torch.randn(n, device=DEV, generator=g) * scale).to(dtype)
    return out


def _pow2(n, g):
    return torch.pow(2.0, torch.randint(-2, 2, (n,), device=DEV, generator=g).float())


def _set_env(monkeypatch, env):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _kid():
    from cddmsl_amd import hip
    return int(hip._L().cddmsl_last_kernel())


def _report(c, tier, **kv):
    line = f"[{c['id']} tier {tier}] kernel {c['kid']} ({c['why']}): " + ", ".join(f"{k} {v}" for k, v in kv.items())
    print(line)
    return line


def _judge(c, tier, got, exact, absp, odt, scale=None, bias=None, residual=None, base=None):
    """tier A: bit-equal to the exact value rounded once; tier B: inside the bound, unbiased bf16 rounding"""
    if tier == "A":
        assert float(absp.max()) < 2 ** 24, "tier A data must keep every partial sum exact in f32"
        want = X.round_bf16(exact) if odt == torch.bfloat16 else X._f64(X._f64(exact).float())
        assert torch.equal(X._f64(exact), X._f64(X._f64(exact).float())), "tier A exact value must be an f32 number"
        same = torch.equal(X._f64(got), want)
        nbad = int((X._f64(got) != want).sum())
        line = _report(c, tier, bit_exact=same, elements=got.numel(), mismatches=nbad)
        assert same, f"{nbad} of {got.numel()} elements differ from the exact result rounded once"
        return line
    ok, ratio, worst = X.check_bound(got, exact, absp, odt, scale, bias, residual, base)
    kv = dict(worst_err_over_bound=f"{ratio:.3g}", elements=got.numel())
    if odt == torch.bfloat16:
        rb, n = X.rounding_bias(got, exact, absp, scale)
        kv.update(rounding_bias=f"{rb:+.4f}", bias_elements=n)
    else:
        kv.update(acc_ratio=f"{X.acc_ratio(got, exact, absp, scale, bias, residual, base):.4g}")
    line = _report(c, tier, **kv)
    g, e = X._f64(got).reshape(-1)[worst], X._f64(exact).reshape(-1)[worst]
    assert ok, f"element {worst}: got {float(g)!r}, exact {float(e)!r}, |err| / bound = {ratio:.3g}"
    if odt == torch.bfloat16 and n >= 100_000:
        assert abs(rb) <= 0.02, f"bf16 rounding bias {rb:+.4f} ulp over {n} elements (RNE gives ~0, truncation -0.5)"
    return line


def _run_conv_fwd(c, tier, seed):
    from cddmsl_amd import hip
    g, e = c["geom"], c["epi"]
    N, H, W, Cin, Cout, KH, KW, s, p, pool = (g[k] for k in ("N", "H", "W", "Cin", "Cout", "KH", "KW", "stride", "pad", "pool"))
    Ho, Wo = X.out_geometry(H, W, KH, KW, s, p, pool)
    M = N * Ho * Wo
    gen = _gen(seed)
    K = KH * KW * Cin
    dt = {"bf16": torch.bfloat16, "f32": torch.float32}[g["dtype"]]
    if tier == "A":
        xa = _ints((N, H, W, Cin), -3 if K <= 4608 else -2, 3 if K <= 4608 else 2, gen, dt)
        wm = _ints((Cout, KH, KW, Cin), -3, 3, gen, torch.float32)
        scale = _pow2(Cout, gen) if e["scale"] else None
        bias = (_ints((Cout,), -64, 64, gen, torch.float32) / 8) if e["bias"] else None
    else:
        xa = _gauss((N, H, W, Cin), gen, dt)
        wm = _gauss((Cout, KH, KW, Cin), gen, torch.float32, K ** -0.5)
        scale = (torch.rand(Cout, device=DEV, generator=gen) + 0.5) if e["scale"] else None
        bias = (torch.randn(Cout, device=DEV, generator=gen) * 0.1) if e["bias"] else None
    if "dgrad_wd" in c["variants"]:
        # the weights the input gradient runs on: weight_prep's flipped / transposed copy of a master [Cin', KH, KW, Cout'],
        # scaled by the forward layer's FrozenBN scale -- its own rounding checked here, then read back as the operand
        master = wm.permute(3, 1, 2, 0).contiguous()                       # forward layer: Cout' = Cin, Cin' = Cout
        fscale = _pow2(Cin, gen) if tier == "A" else torch.rand(Cin, device=DEV, generator=gen) + 0.5
        _, w = hip.weight_prep(master, fscale, torch.bfloat16, want_fwd=False)
        want = (master * fscale.view(-1, 1, 1, 1)).to(torch.bfloat16).flip(1, 2).permute(3, 1, 2, 0)
        assert torch.equal(w, want), "weight_prep's dgrad weights: not the flipped, transposed, scaled weights rounded once"
    else:
        w = wm.to(dt)
    res = rp = msk = None
    if e["residual"] == "pooled":
        rp = (_ints((N, Ho // 2, Wo // 2, Cout), -16, 16, gen) / 4 if tier == "A" else _gauss((N, Ho // 2, Wo // 2, Cout), gen)).to(torch.bfloat16)
    elif e["residual"] in ("bf16", "f32"):
        rdt = torch.bfloat16 if e["residual"] == "bf16" else torch.float32
        res = (_ints((N, Ho, Wo, Cout), -16, 16, gen, torch.float32) / 4).to(rdt) if tier == "A" else _gauss((N, Ho, Wo, Cout), gen, rdt, 3.0)
    if e["relu_mask"]:
        msk = _ints((N, Ho, Wo, Cout), -1, 1, gen) if tier == "A" else _gauss((N, Ho, Wo, Cout), gen)
    y = hip.conv_fwd(xa, w, scale, bias, rp if rp is not None else res, e["relu"], msk, s, p, pool, e["out_f32"], rp is not None)
    assert _kid() == c["kid"], (_kid(), c["kid"])
    odt = y.dtype
    rows = None
    if M > ROW_SAMPLE_ABOVE:
        rows = X.sample_rows(M, [Cout * y.element_size(), Cin * xa.element_size()], device=DEV, seed=seed)
    acc, absp = X.conv_exact(xa, w, s, p, pool, rows=rows)
    sel = (lambda t: t.reshape(M, -1)) if rows is None else (lambda t: t.reshape(M, -1)[rows])
    r_rows = None
    if rp is not None:
        r_rows = X.pooled_residual_rows(rp, rows if rows is not None else torch.arange(M, device=DEV), Ho, Wo)
    elif res is not None:
        r_rows = X._f64(sel(res))
    m_rows = None if msk is None else sel(msk)
    exact = X.epilogue_exact(acc, scale, bias, r_rows, e["relu"], m_rows, rp is not None)
    got = sel(y)
    del y
    return _judge(c, tier, got, exact, absp, odt, scale, bias, None if r_rows is None else (0.25 if rp is not None else 1.0) * r_rows.abs())


def _run_conv_wgrad(c, tier, seed):
    from cddmsl_amd import hip
    g, e = c["geom"], c["epi"]
    N, H, W, Cin, Cout, KH, KW, s, p, pool = (g[k] for k in ("N", "H", "W", "Cin", "Cout", "KH", "KW", "stride", "pad", "pool"))
    Ho, Wo = X.out_geometry(H, W, KH, KW, s, p, pool)
    M = N * Ho * Wo
    gen = _gen(seed)
    if tier == "A":
        lim = 1 if M * 9 >= 2 ** 20 else 3              # bench M: {-1, 0, 1} keeps sums over millions of rows exact
        x = _ints((N, H, W, Cin), -lim, lim, gen)
        dy = _ints((N, Ho, Wo, Cout), -lim, lim, gen)
        scale = _pow2(Cout, gen) if e["scale"] else None
        base = _ints((Cout, KH, KW, Cin), -100, 100, gen, torch.float32) if e["accumulate"] else None
    else:
        x = _gauss((N, H, W, Cin), gen)
        dy = _gauss((N, Ho, Wo, Cout), gen)
        scale = (torch.rand(Cout, device=DEV, generator=gen) + 0.5) if e["scale"] else None
        base = torch.randn(Cout, KH, KW, Cin, device=DEV, generator=gen) if e["accumulate"] else None
    out = hip.conv_wgrad(x, dy, (Cout, KH, KW, Cin), scale, s, p, pool, out=None if base is None else base.clone())
    assert _kid() == c["kid"], (_kid(), c["kid"])
    taps = [(kh, kw) for kh in range(KH) for kw in range(KW)]
    if M > ROW_SAMPLE_ABOVE and len(taps) > 3:
        taps = [taps[0], taps[len(taps) // 2], taps[-1]]       # (corner taps read the padding, the centre tap does not)
    acc, absp = X.wgrad_exact(x, dy, KH, KW, s, p, pool, taps=taps)
    del x, dy
    ti = torch.tensor([kh * KW + kw for kh, kw in taps], device=DEV)
    got = out.view(Cout, KH * KW, Cin)[:, ti]
    sc = None if scale is None else scale.view(-1, 1, 1)
    exact = acc * (1.0 if sc is None else X._f64(sc))
    bsel = None
    if base is not None:
        bsel = X._f64(base.view(Cout, KH * KW, Cin)[:, ti])
        exact = exact + bsel
    return _judge(c, tier, got, exact, absp, torch.float32, sc, None, None, None if bsel is None else bsel.abs())


def _extent(shape, strides, off):
    return off + sum((n - 1) * st for n, st in zip(shape, strides)) + 1


def _run_gemm(c, tier, seed):
    """the batched entry points on the case's own layout: operand views of flat buffers (element strides and offsets as the
    attention pool passes them); the output buffer outside the view must come back untouched"""
    from cddmsl_amd import hip
    g, e = c["geom"], c["epi"]
    M, N, K, B = g["M"], g["N"], g["K"], g["batch"]
    gen = _gen(seed)
    is_nt = c["entry"] == "gemm_nt_batched"
    if is_nt:
        va = ((B, M, K), (g["sa"], g["lda"], 1), g["a_off"])
        vb = ((B, N, K), (g["sw"], g["ldb"], 1), g["b_off"])
        vo = ((B, M, N), (g["sc"], g["ldc"], 1), g["c_off"])
        odt, acc_out = (torch.float32 if e["out_f32"] else torch.bfloat16), False
    else:
        va = ((B, M, N), (g["sa"], g["lda"], 1), g["a_off"])
        vb = ((B, M, K), (g["sb"], g["ldb"], 1), g["b_off"])
        vo = ((B, N, K), (g["so"], g["ldo"], 1), g["c_off"])
        odt, acc_out = (torch.float32 if e["out"] == "f32" else torch.bfloat16), e["accumulate"]
    mk = (lambda n: _ints((n,), -3, 3, gen)) if tier == "A" else (lambda n: _gauss((n,), gen))
    abuf, bbuf = mk(_extent(*va)), mk(_extent(*vb))
    no = _extent(*vo)
    if acc_out:
        obuf = _ints((no,), -100, 100, gen, torch.float32) if tier == "A" else torch.randn(no, device=DEV, generator=gen)
    else:
        obuf = torch.full((no,), float("nan"), device=DEV, dtype=odt)
    before = obuf.clone()
    if is_nt:
        hip.gemm_nt_batched(abuf, bbuf, obuf, M, N, K, g["lda"], g["ldb"], g["ldc"], B, g["sa"], g["sw"], g["sc"],
                            a_off=g["a_off"], w_off=g["b_off"], c_off=g["c_off"])
    else:
        hip.gemm_tn_batched(abuf, bbuf, obuf, M, N, K, g["lda"], g["ldb"], g["ldo"], B, g["sa"], g["sb"], g["so"],
                            a_off=g["a_off"], b_off=g["b_off"], o_off=g["c_off"], accumulate=acc_out)
    assert _kid() == c["kid"], (_kid(), c["kid"])
    torch.cuda.synchronize()
    inview = torch.zeros(no, device=DEV, dtype=torch.bool)
    inview.as_strided(*vo).fill_(True)
    ibits = torch.int32 if odt == torch.float32 else torch.int16
    stray = int(((obuf.view(ibits) != before.view(ibits)) & ~inview).sum())      # (no boolean indexing: > 2^31 elements)
    del inview
    assert stray == 0, f"{stray} elements outside the output view changed"
    # the batches checked: all of a few; of many, two of every 64, the first and last, those whose base crosses a 2 GiB multiple
    if B <= 64:
        bsel = torch.arange(B, device=DEV)
    else:
        bsel = X.sample_rows(B, [va[1][0] * 2, vb[1][0] * 2, vo[1][0] * obuf.element_size()], tile=64, seed=seed, device=DEV)
    parts = []
    for i in range(0, len(bsel), 4):           # (float64 copies of a few batches at a time)
        bi = bsel[i:i + 4]
        parts.append(X.gemm_exact(abuf.as_strided(*va)[bi], bbuf.as_strided(*vb)[bi], transpose_a=not is_nt))
    exact, absp = torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts])
    base = X._f64(before.as_strided(*vo)[bsel]) if acc_out else None
    if base is not None:
        exact = exact + base
    got = obuf.as_strided(*vo)[bsel]
    return _judge(c, tier, got, exact, absp, odt, None, None, None, None if base is None else base.abs())


_RUN = {"conv_fwd": _run_conv_fwd, "conv_wgrad": _run_conv_wgrad, "gemm_nt_batched": _run_gemm, "gemm_tn_batched": _run_gemm}
_PARAMS = [pytest.param(c, t, id=f"{c['id']}-{t}") for c in T.CASES for t in c["tiers"]]


@pytest.mark.parametrize("c,tier", _PARAMS)
def test_exact_product(c, tier, monkeypatch, capsys):
    from cddmsl_amd import hip
    hip.ensure_workspace(DEV)
    _set_env(monkeypatch, c["env"])
    try:
        line = _RUN[c["entry"]](c, tier, seed=1000 + T.CASES.index(c) * 2 + (tier == "B"))
    finally:
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
    with capsys.disabled():                 # (kernel id, bit-exactness / worst ratio and rounding bias: shown without -s)
        print("\n" + line)


# ------------------------------------------------------------------------------------------------ the recorded dispatch
def _plan(entry, g, epi):
    """run the entry point on right-sized (uninitialised) tensors with the library in plan-only mode: it chooses its kernel and
    returns without launching; -> the kernel id"""
    from cddmsl_amd import hip
    bf = {"bf16": torch.bfloat16, "f32": torch.float32}[g["dtype"]]      # (the operand dtype of the recorded launch)
    L = hip._L()
    L.cddmsl_plan_only(1)
    try:
        if entry == "conv_fwd":
            N, H, W, Cin, Cout, KH, KW, s, p, pool = (g[k] for k in ("N", "H", "W", "Cin", "Cout", "KH", "KW", "stride", "pad", "pool"))
            Ho, Wo = X.out_geometry(H, W, KH, KW, s, p, pool)
            x, w = torch.empty(N, H, W, Cin, device=DEV, dtype=bf), torch.empty(Cout, KH, KW, Cin, device=DEV, dtype=bf)
            vec = torch.ones(Cout, device=DEV)
            res = None
            if epi["residual"] == "pooled":
                res = torch.empty(N, Ho // 2, Wo // 2, Cout, device=DEV, dtype=bf)
            elif epi["residual"]:
                res = torch.empty(N, Ho, Wo, Cout, device=DEV, dtype=torch.bfloat16 if epi["residual"] == "bf16" else torch.float32)
            msk = torch.empty(N, Ho, Wo, Cout, device=DEV, dtype=bf) if epi["relu_mask"] else None
            hip.conv_fwd(x, w, vec if epi["scale"] else None, vec if epi["bias"] else None, res, epi["relu"], msk, s, p, pool,
                         epi["out_f32"], epi["residual"] == "pooled")
        elif entry == "conv_wgrad":
            N, H, W, Cin, Cout, KH, KW, s, p, pool = (g[k] for k in ("N", "H", "W", "Cin", "Cout", "KH", "KW", "stride", "pad", "pool"))
            Ho, Wo = X.out_geometry(H, W, KH, KW, s, p, pool)
            x, dy = torch.empty(N, H, W, Cin, device=DEV, dtype=bf), torch.empty(N, Ho, Wo, Cout, device=DEV, dtype=bf)
            out = torch.empty(Cout, KH, KW, Cin, device=DEV)
            hip.conv_wgrad(x, dy, (Cout, KH, KW, Cin), torch.ones(Cout, device=DEV) if epi["scale"] else None, s, p, pool, out=out)
        elif entry == "gemm_nt_batched":
            na = (g["batch"] - 1) * g["sa"] + (g["M"] - 1) * g["lda"] + g["K"]
            nw = (g["batch"] - 1) * g["sw"] + (g["N"] - 1) * g["ldb"] + g["K"]
            nc = (g["batch"] - 1) * g["sc"] + (g["M"] - 1) * g["ldc"] + g["N"]
            hip.gemm_nt_batched(torch.empty(na, device=DEV, dtype=bf), torch.empty(nw, device=DEV, dtype=bf),
                                torch.empty(nc, device=DEV, dtype=torch.float32 if epi["out_f32"] else bf), g["M"], g["N"], g["K"], g["lda"],
                                g["ldb"], g["ldc"], g["batch"], g["sa"], g["sw"], g["sc"])
        else:
            na = (g["batch"] - 1) * g["sa"] + (g["M"] - 1) * g["lda"] + g["N"]
            nb = (g["batch"] - 1) * g["sb"] + (g["M"] - 1) * g["ldb"] + g["K"]
            no = (g["batch"] - 1) * g["so"] + (g["N"] - 1) * g["ldo"] + g["K"]
            hip.gemm_tn_batched(torch.empty(na, device=DEV, dtype=bf), torch.empty(nb, device=DEV, dtype=bf),
                                torch.empty(no, device=DEV, dtype=torch.float32 if epi["out"] == "f32" else bf), g["M"], g["N"], g["K"],
                                g["lda"], g["ldb"], g["ldo"], g["batch"], g["sa"], g["sb"], g["so"], accumulate=epi["accumulate"])
    finally:
        L.cddmsl_plan_only(0)
    return _kid()


def test_recorded_bench_launches_keep_their_kernels(monkeypatch, golden_dir, capsys):
    """every distinct GEMM launch of the bench step (16 and 32 images) still dispatches to the kernel recorded for it; a change of
    dispatch must re-record tests/golden/bench_gemm_launches.json (tools/record_gemm_launches.py) -- and the case table follows"""
    from cddmsl_amd import hip
    hip.ensure_workspace(DEV)
    _set_env(monkeypatch, {})
    with open(os.path.join(golden_dir, "bench_gemm_launches.json")) as fh:
        rec = json.load(fh)["entries"]
    bad = []
    for e in rec:
        kid = _plan(e["entry"], e["geometry"], e["epilogue"])
        if kid != e["kernel_id"]:
            bad.append((e["images"], e["entry"], e["geometry"], e["epilogue"], e["kernel_id"], kid))
        torch.cuda.empty_cache()
    with capsys.disabled():
        print(f"\n{len(rec)} recorded launches replayed in plan-only mode, {len(bad)} changed kernel")
    assert not bad, bad
