"""bf16 and f32 convolution / GEMM kernels against the exact float64 product of the operands they were given (tests/exact_gemm.py),
for every case of tests/gemm_exact_cases.py -- every kernel family and instantiation in either operand type, the bench's own launch
shapes at full M and the 32-image geometry past 2 GiB -- in two tiers:

  A  small-integer operands, power-of-two scales, dyadic bias / residual / dW: every partial sum is exact in f32 in any order
     (split-K, atomics, workspace reductions), so the output must equal the exact value rounded once -- torch.equal.
  B  Gaussian operands: every element inside exact_gemm.check_bound, and a bf16 store without rounding bias.

Plus the launch records (tests/golden/bench_gemm_launches.json, stock_gemm_launches.json of the stock R50-C4 step, and the f32 steps
of both in bench_gemm_launches_f32.json and stock_gemm_launches_f32.json) replayed in plan-only mode: dispatch still picks the
recorded kernel.  And the stock stem as the model calls it (BasicStem.forward_nhwc).

Measured on one MI355X, the strided cases of the stock ResNet path and what else its record added; tier A bit-equal in all of them,
tier B worst |err| / bound (0.99 is a correctly rounded bf16 store of a value just above a power of two; none below 0.05, the mark of
a loose bound -- the two lowest, the accumulating weight gradients, are dominated by the 2^-24 |dW before| term of the bound), then
the bf16 store's rounding bias in ulp or, for f32 outputs, the accumulation ratio C_ACC = 8 must cover:
  stem_7x7_s2_bf16 0.993 -0.0004         stem_7x7_s2_bf16_even 0.992 -0.0027     stem_7x7_s2_f32 0.467 acc 3.18
  stem_7x7_s2_f32_even 0.445 acc 3.06    fwd_1x1_s2_bn_relu 0.986 -0.0064        fwd_1x1_s2_bn 0.990 -0.0002
  fwd_1x1_s2_bn_relu_even 0.993 -0.0016  fwd_1x1_s2_bn_even 0.995 -0.0000        fwd2_1x1_s2_bn_relu 0.994 +0.0017
  fwd2_1x1_s2_bn_even 0.995 -0.0001      fwd256_1x1_s2_bn_relu 0.992 +0.0006     fwd256_1x1_s2_bn_even 0.995 -0.0001
  fwd256_roi_crops_s2 0.995 -0.0001      fwd256_persistent_s2 0.996 -0.0003      fwd256_persistent_s2_bn 0.996 -0.0002
  fwd256_tail_split_s2 0.995 -0.0003     wgrad_1x1_s2 0.055 acc 0.43             wgrad_1x1_s2_even 0.068 acc 0.43
  wgrad_1x1_s2_one_row 0.244 acc 0.43    nt_rpn_sparse_dx 0.283 acc 2.03
  test_stock_stem_against_float64, worst |err| / limit: f32 0.470 (37 x 53), 0.589 (38 x 54); bf16 0.992, 0.986

The f32-operand block (the f32_* cases: operands, residuals, masks and output f32; u_out = 2^-24, the same C_ACC = 8), measured on one
MI355X: tier A bit-equal in all 75, no kernel fix needed; tier B worst |err| / bound, then acc_ratio.  Worst acc_ratio per kernel:
k_conv_fwd<float> 5.52 (f32_nt_rpn_sparse_dx, K = 1024, 2.4 M outputs), k_conv_fwd_reg<float> 3.58, k_conv_fwd256<float> 5.01
(f32_nt_qk), k_conv_fwd2<float> 4.25, k_conv3x3_small<float> 4.91, k_conv_wgrad<float> 2.46, k_conv_wgrad_dma<float> 4.27
(f32_tn_dwv), k_gemm_tn_stream<float> 3.55 -- above the bf16-operand figures because the products are rounded too, and in line with
ATen's CPU f32 convolution of f32 operands (4.07 at K = 288, tests/test_exact_bound_host.py); none reaches 8.
  f32_fwd_1x1_plain 0.526 acc 3.43              f32_fwd_1x1_bn 0.500 acc 2.88                 f32_fwd_1x1_bn_relu 0.458 acc 2.56
  f32_fwd_1x1_bias_relu 0.497 acc 2.93          f32_fwd_1x1_bn_res_relu 0.538 acc 3.11        f32_fwd_1x1_res 0.428 acc 2.31
  f32_fwd_1x1_mask 0.458 acc 2.68               f32_fwd_1x1_mask_res 0.434 acc 2.63           f32_fwd_3x3_bn_relu 0.538 acc 3.85
  f32_fwd_3x3_mask 0.550 acc 4.05               f32_fwd_1x1_s2_bn_relu 0.505 acc 3.29         f32_fwd_1x1_s2_bn 0.424 acc 2.61
  f32_fwd_1x1_s2_bn_relu_even 0.542 acc 3.35    f32_fwd_1x1_s2_bn_even 0.481 acc 2.68         f32_fwd_s56_bias 0.408 acc 2.50
  f32_fwd_1x1_64_not_small 0.478 acc 2.73       f32_fwd_reg_pool 0.414 acc 2.21               f32_fwd_reg_pool_bn_relu 0.566 acc 3.58
  f32_fwd256_1x1_plain 0.669 acc 4.85           f32_fwd256_1x1_bn 0.572 acc 3.85              f32_fwd256_1x1_bn_relu 0.535 acc 3.66
  f32_fwd256_1x1_bias_relu 0.550 acc 3.86       f32_fwd256_1x1_bn_res_relu 0.504 acc 3.29     f32_fwd256_1x1_res 0.536 acc 3.26
  f32_fwd256_1x1_mask 0.654 acc 4.33            f32_fwd256_1x1_mask_res 0.510 acc 3.37        f32_fwd256_3x3_bn_relu 0.615 acc 4.55
  f32_fwd256_3x3_mask 0.496 acc 3.60            f32_fwd256_1x1_s2_bn_relu 0.573 acc 3.99      f32_fwd256_1x1_s2_bn_even 0.507 acc 3.53
  f32_fwd256_res_pool 0.516 acc 3.55            f32_fwd256_res_pool_mask 0.628 acc 4.26       f32_fwd2_1x1_plain 0.555 acc 3.35
  f32_fwd2_1x1_bn_relu 0.571 acc 3.92           f32_fwd2_1x1_mask 0.547 acc 3.50              f32_fwd2_3x3_bn_relu 0.532 acc 3.88
  f32_fwd2_3x3_mask 0.501 acc 3.64              f32_fwd2_1x1_s2_bn 0.487 acc 2.98             f32_small_1_1 0.547 acc 3.22
  f32_small_1_2 0.482 acc 3.32                  f32_small_4_1 0.417 acc 2.93                  f32_small_4_2 0.542 acc 3.88
  f32_small_8_2 0.650 acc 4.91                  f32_small_8_2_mask 0.568 acc 4.26             f32_wgrad_dma_1x1_acc 0.067 acc 0.53
  f32_wgrad_dma_1x1_new 0.082 acc 0.58          f32_wgrad_dma_3x3 0.405 acc 2.94              f32_wgrad_dma_under_f256 0.105 acc 0.80
  f32_wgrad_1x1_s2 0.180 acc 1.23               f32_wgrad_1x1_s2_even 0.172 acc 1.25          f32_wgrad_1x1_s2_one_row 0.393 acc 1.86
  f32_wgrad_s56 0.455 acc 2.46                  f32_nt_128 0.405 acc 2.45                     f32_nt_256 0.485 acc 2.71
  f32_nt_regions 0.565 acc 3.89                 f32_nt_shared_a 0.416 acc 2.52                f32_tn_stream 0.418 acc 2.58
  f32_tn_stream_2 0.479 acc 3.55                f32_tn_dma_acc 0.277 acc 2.21                 f32_fwd_1x1_f32 0.502 acc 3.06
  f32_fwd_1x1_bias_f32 0.526 acc 3.28           f32_fwd_1x1_bias_relu_f32 0.564 acc 3.41      f32_fwd_3x3_bias_relu 0.461 acc 3.32
  f32_fwd_res_pool 0.517 acc 2.91               f32_fwd2_1x1_bn 0.628 acc 4.25                f32_fwd2_1x1_bn_res_relu 0.492 acc 2.90
  f32_fwd2_1x1_mask_res 0.499 acc 2.59          f32_wgrad_dma_1x1_acc_noscale 0.075 acc 0.59  f32_tn_dma_store 0.589 acc 3.90
  f32_nt_heads 0.546 acc 4.21                   f32_nt_regions_full 0.579 acc 4.48            f32_nt_qk 0.684 acc 5.01
  f32_tn_dwv 0.646 acc 4.27                     f32_nt_mapper 0.618 acc 4.83                  f32_nt_rpn_sparse_dx 0.707 acc 5.52"""
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
        rp = (_ints((N, Ho // 2, Wo // 2, Cout), -16, 16, gen) / 4 if tier == "A" else _gauss((N, Ho // 2, Wo // 2, Cout), gen, dt)).to(dt)
    elif e["residual"] in ("bf16", "f32"):
        rdt = torch.bfloat16 if e["residual"] == "bf16" else torch.float32
        res = (_ints((N, Ho, Wo, Cout), -16, 16, gen, torch.float32) / 4).to(rdt) if tier == "A" else _gauss((N, Ho, Wo, Cout), gen, rdt, 3.0)
    if e["relu_mask"]:
        msk = _ints((N, Ho, Wo, Cout), -1, 1, gen, dt) if tier == "A" else _gauss((N, Ho, Wo, Cout), gen, dt)     # (the operand dtype: b32 mask loads in f32)
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
    dt = {"bf16": torch.bfloat16, "f32": torch.float32}[g["dtype"]]      # (x and dy; dW and its master are f32 in either)
    if tier == "A":
        lim = 1 if M * 9 >= 2 ** 20 else 3              # bench M: {-1, 0, 1} keeps sums over millions of rows exact
        x = _ints((N, H, W, Cin), -lim, lim, gen, dt)
        dy = _ints((N, Ho, Wo, Cout), -lim, lim, gen, dt)
        scale = _pow2(Cout, gen) if e["scale"] else None
        base = _ints((Cout, KH, KW, Cin), -100, 100, gen, torch.float32) if e["accumulate"] else None
    else:
        x = _gauss((N, H, W, Cin), gen, dt)
        dy = _gauss((N, Ho, Wo, Cout), gen, dt)
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
    dt = {"bf16": torch.bfloat16, "f32": torch.float32}[g["dtype"]]      # (both operands; an f32 product stores f32)
    is_nt = c["entry"] == "gemm_nt_batched"
    if is_nt:
        va = ((B, M, K), (g["sa"], g["lda"], 1), g["a_off"])
        vb = ((B, N, K), (g["sw"], g["ldb"], 1), g["b_off"])
        vo = ((B, M, N), (g["sc"], g["ldc"], 1), g["c_off"])
        odt, acc_out = (torch.float32 if e["out_f32"] else dt), False
    else:
        va = ((B, M, N), (g["sa"], g["lda"], 1), g["a_off"])
        vb = ((B, M, K), (g["sb"], g["ldb"], 1), g["b_off"])
        vo = ((B, N, K), (g["so"], g["ldo"], 1), g["c_off"])
        odt, acc_out = (torch.float32 if e["out"] == "f32" else torch.bfloat16), e["accumulate"]
        assert odt == torch.float32 or dt == torch.bfloat16, "an f32 product has no bf16 store"
    mk = (lambda n: _ints((n,), -3, 3, gen, dt)) if tier == "A" else (lambda n: _gauss((n,), gen, dt))
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
        es = abuf.element_size()
        bsel = X.sample_rows(B, [va[1][0] * es, vb[1][0] * es, vo[1][0] * obuf.element_size()], tile=64, seed=seed, device=DEV)
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


def _replay(monkeypatch, golden_dir, capsys, record):
    from cddmsl_amd import hip
    hip.ensure_workspace(DEV)
    _set_env(monkeypatch, {})
    with open(os.path.join(golden_dir, record)) as fh:
        rec = json.load(fh)["entries"]
    bad = []
    for e in rec:
        kid = _plan(e["entry"], e["geometry"], e["epilogue"])
        if kid != e["kernel_id"]:
            bad.append((e["images"], e["entry"], e["geometry"], e["epilogue"], e["kernel_id"], kid))
        torch.cuda.empty_cache()
    with capsys.disabled():
        print(f"\n{record}: {len(rec)} recorded launches replayed in plan-only mode, {len(bad)} changed kernel")
    assert rec and not bad, bad


def test_recorded_bench_launches_keep_their_kernels(monkeypatch, golden_dir, capsys):
    """every distinct GEMM launch of the bench step (16 and 32 images) still dispatches to the kernel recorded for it; a change of
    dispatch must re-record tests/golden/bench_gemm_launches.json (tools/record_gemm_launches.py) -- and the case table follows"""
    _replay(monkeypatch, golden_dir, capsys, "bench_gemm_launches.json")


def test_recorded_stock_launches_keep_their_kernels(monkeypatch, golden_dir, capsys):
    """the same for the stock R50-C4 configuration's step (16 images; tests/golden/stock_gemm_launches.json, recorded with
    tools/record_gemm_launches.py --stock): the 7x7 stem, the stride-2 1x1 convolutions and their weight gradients among them"""
    _replay(monkeypatch, golden_dir, capsys, "stock_gemm_launches.json")


@pytest.mark.parametrize("record", ["bench_gemm_launches_f32.json", "stock_gemm_launches_f32.json"])
def test_recorded_f32_launches_keep_their_kernels(record, monkeypatch, golden_dir, capsys):
    """the same for the f32 steps of the two configurations on one 800x1333 image -- the instantiations every oracle-parity test runs
    on (tools/record_gemm_launches.py --dtype f32, with and without --stock)"""
    _replay(monkeypatch, golden_dir, capsys, record)


# ------------------------------------------------------------------------------------------------ the stock stem, as the model calls it
@pytest.mark.parametrize("H,W", [(37, 53), (38, 54)])
@pytest.mark.parametrize("tname", ["f32", "bf16"])
def test_stock_stem_against_float64(tname, H, W, capsys):
    """BasicStem.forward_nhwc (7x7 stride 2 pad 3 on k_conv_fwd, FrozenBN, ReLU, then hip.maxpool3s2_fwd) on 2 x H x W pixels padded
    to one 16-byte chunk, the padding channels holding garbage (the stem's padded weights are zero there), non-trivial FrozenBN
    buffers -- against F.conv2d on the 3 real channels in float64, the folded affine, ReLU and F.max_pool2d(3, 2, 1).

    Limit, per pooled element: the largest exact_gemm.bound of the convolution outputs in its 3 x 3 window.  Reasoning, as in
    tests/test_gpu_fused_bottleneck.py test_against_float64_chain: the chain has ONE rounded layer.  A stored convolution output
    differs from the exact relu(scale * sum + bias) by at most the bound of the exact-product cases above (accumulation: C_ACC * 2^-24
    * |scale| * sum|a*b|, plus 2^-24 |bias|, plus one rounding of the output, u_out * |exact|; ReLU does not increase a difference);
    the pooling kernel selects one of the stored values and rounds nothing, and |max a_i - max b_i| <= max |a_i - b_i|."""
    import torch.nn.functional as F
    from cddmsl_amd.modeling import resnet
    T = {"f32": torch.float32, "bf16": torch.bfloat16}[tname]
    cp = 16 // torch.empty((), dtype=T).element_size()
    gen = _gen(4100 + H + (T == torch.bfloat16))
    stem = resnet.BasicStem(3, 64).to(DEV)
    w = torch.randn(64, 3, 7, 7, device=DEV, generator=gen) * 147 ** -0.5
    stem.conv1.weight.data.copy_(w.to(T).float())                  # (values the compute dtype holds: weight_prep rounds nothing)
    n = stem.conv1.norm
    for buf, v in (("weight", torch.rand(64, device=DEV, generator=gen) + 0.5), ("bias", torch.randn(64, device=DEV, generator=gen) * 0.3),
                   ("running_mean", torch.randn(64, device=DEV, generator=gen) * 0.3), ("running_var", torch.rand(64, device=DEV, generator=gen) + 0.5)):
        getattr(n, buf).copy_(v)
    x = _gauss((2, H, W, cp), gen, T)
    x[..., 3:] = _gauss((2, H, W, cp - 3), gen, T, 100.0)           # garbage where the model writes zeros
    assert float(x[..., 3:].abs().min()) > 0
    with torch.no_grad():
        got = stem.forward_nhwc(x)
    assert _kid() == 1, _kid()
    torch.cuda.synchronize()
    scale, bias = (X._f64(v) for v in n.affine())
    xr, wr = X._f64(x[..., :3]).permute(0, 3, 1, 2), X._f64(stem.conv1.weight.detach())
    acc = F.conv2d(xr, wr, stride=2, padding=3)
    absp = F.conv2d(xr.abs(), wr.abs(), stride=2, padding=3)
    sc, bi = scale.view(1, -1, 1, 1), bias.view(1, -1, 1, 1)
    exact = (acc * sc + bi).clamp_min(0)
    b = X.bound(exact, absp, T, sc, bi.expand_as(exact))
    ref = F.max_pool2d(exact, 3, 2, 1).permute(0, 2, 3, 1)
    lim = F.max_pool2d(b, 3, 2, 1).permute(0, 2, 3, 1)
    Hc, Wc = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    assert got.dtype == T and tuple(got.shape) == tuple(ref.shape) == (2, (Hc - 1) // 2 + 1, (Wc - 1) // 2 + 1, 64)
    err = (X._f64(got) - ref).abs()
    ratio = float((err / lim).max())
    with capsys.disabled():
        print(f"\n[stock stem {tname} 2 x {H} x {W}] kernel 1 + maxpool3s2: worst |err| / limit {ratio:.3g}, elements {got.numel()}, "
              f"non-zero {int((ref > 0).sum())}")
    assert int((ref > 0).sum()) > got.numel() // 2
    assert bool((err <= lim).all()), ratio
