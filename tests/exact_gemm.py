"""Exact references and an error bound for the bf16 convolution / GEMM kernels (imported by the exact-product tests; not a conftest).

Every kernel behind the dispatch of cddmsl_amd/csrc/gemm_conv.hip (conv_fwd.hip, conv_fwd256.hip, conv_wgrad.hip, bottleneck64.hip) multiplies bf16 operands exactly and sums the products in f32, so its result can be
held to the float64 product of the operands it was given -- not to another library's f32 convolution:

  |got - exact| <= u_out * |exact| + C_ACC * 2^-24 * |scale| * sum|a*b| + 2^-24 * (|bias| + |residual| + |dW before|)

u_out is the unit roundoff of the stored output (2^-8 bf16, 2^-24 f32).  Everything here runs on the CPU or on the GPU, in float64.

The f32 instantiations of the same kernels (Mma<float>: 32x32x2f32 steps) are held to the same bound: their products are rounded to
f32 as well, one more 2^-24 |a*b| each, which C_ACC covers (figures below).  Small-integer operands stay exact in f32, so tier A of
tests/test_gpu_gemm_exact.py asks of them what it asks of bf16: the exact value, rounded once.
"""
import math

import torch

U_F32 = 2.0 ** -24
U_BF16 = 2.0 ** -8

# Accumulation constant of the bound, in units of 2^-24 * sum|a*b|.  Measured on one MI355X over the f32-output cases of
# tests/test_gpu_gemm_exact.py (tier B, the acc_ratio it prints): worst 3.48 on the f32-operand k_conv_fwd case (its products are
# rounded to f32 too); of the bf16-operand kernels, 2.05 (k_conv_fwd256, the mapper's batched product, K = 1920), 1.90
# (k_conv_fwd, the attention pool's per-region product at 16384 regions) and 1.30 (k_conv_wgrad, stride 56, M = 8192); the
# weight-gradient reductions through the workspace stay below 0.9.  The bf16 MFMA chains thus accumulate like plain f32 sums --
# nowhere near the 64 that would call for probing the instruction's internal accumulation.  ATen's CPU f32 convolution
# (tests/test_exact_bound_host.py, K = 576) measures 2.4.  8 keeps a margin of 2.3x over the worst of these.
# The f32-operand cases (f32_*: every f32 instantiation, products rounded to f32 as well), worst per kernel: k_conv_fwd<float> 5.52
# (the RPN head's shared-A batched product, K = 1024, the maximum over 2.4 M outputs), k_conv_fwd256<float> 5.01 (K = 64 on 2.2 M
# outputs), k_conv3x3_small<float> 4.91, k_conv_fwd2<float> 4.25, k_conv_wgrad_dma<float> 4.27, k_conv_fwd_reg<float> 3.58,
# k_gemm_tn_stream<float> 3.55, k_conv_wgrad<float> 2.46.  ATen's CPU f32 convolution of f32 operands measures 4.07 at K = 288
# on 0.2 M outputs (the same file), so this is what a plain f32 sum of rounded products gives; none exceeds 8 (margin 1.45x), and the
# bf16 constant stays as it is.  Should an f32 case pass 8 with its tier A twin bit-equal, it gets a constant of its own.
C_ACC = 8.0


def _f64(t):
    return t.to(torch.float64)


def out_geometry(H, W, KH, KW, stride, pad, pool):
    if pool:
        return H // 2, W // 2
    return (H + 2 * pad - KH) // stride + 1, (W + 2 * pad - KW) // stride + 1


def _tap_rows(x, rows, Ho, Wo, kh, kw, stride, pad):
    """[R, Cin] input pixels tap (kh, kw) of output rows ``rows`` reads (zeros in the padding), x's dtype"""
    N, H, W, Cin = x.shape
    n, r = rows // (Ho * Wo), rows % (Ho * Wo)
    ih, iw = (r // Wo) * stride - pad + kh, (r % Wo) * stride - pad + kw
    ok = (ih >= 0) & (ih < H) & (iw >= 0) & (iw < W)
    idx = ((n * H + ih.clamp(0, H - 1)) * W + iw.clamp(0, W - 1))
    a = x.reshape(-1, Cin)[idx]
    return a * ok.unsqueeze(1).to(a.dtype)


def _pool_rows(x, rows, Ho, Wo):
    """[R, Cin] 2x2-average-pooled input pixels of output rows ``rows``: the operand the pooled loader forms -- the f32 mean
    rounded to x's dtype (bf16 or f32); kept exact for a float64 x"""
    N, H, W, Cin = x.shape
    n, r = rows // (Ho * Wo), rows % (Ho * Wo)
    oh, ow = r // Wo, r % Wo
    xf = x.reshape(-1, Cin)
    s = 0
    for dy in (0, 1):
        for dx in (0, 1):
            s = s + _f64(xf[(n * H + 2 * oh + dy) * W + 2 * ow + dx])
    s = s * 0.25
    return s if x.dtype == torch.float64 else _f64(s.to(x.dtype))


def conv_exact(x, w, stride=1, pad=0, pool=False, rows=None, chunk=1 << 16):
    """NHWC convolution in float64 from explicit tap shifts and float64 matmuls.  x [N,H,W,Cin], w [Cout,KH,KW,Cin] (any dtype,
    any device).  Returns (exact [R, Cout], absprod [R, Cout]) for the flattened output rows ``rows`` (all rows if None);
    absprod = sum |a*b| per output, the same computation on |x| and |w|.  pool: 1x1 over the 2x2 average-pooled input."""
    N, H, W, Cin = x.shape
    Cout, KH, KW, _ = w.shape
    Ho, Wo = out_geometry(H, W, KH, KW, stride, pad, pool)
    if rows is None:
        rows = torch.arange(N * Ho * Wo, device=x.device)
    rows = rows.to(x.device, torch.int64)
    wf = _f64(w)
    out = torch.zeros(len(rows), Cout, dtype=torch.float64, device=x.device)
    absp = torch.zeros_like(out)
    for c0 in range(0, len(rows), chunk):
        rr = rows[c0:c0 + chunk]
        for kh in range(KH):
            for kw in range(KW):
                a = _pool_rows(x, rr, Ho, Wo) if pool else _f64(_tap_rows(x, rr, Ho, Wo, kh, kw, stride, pad))
                b = wf[:, kh, kw, :]
                out[c0:c0 + chunk] += a @ b.t()
                absp[c0:c0 + chunk] += a.abs() @ b.abs().t()
    return out, absp


def wgrad_exact(x, dy, KH, KW, stride=1, pad=0, pool=False, taps=None, chunk=1 << 18):
    """dW[n, tap, c] = sum_m dy[m, n] * im2col(x)[m, tap, c] in float64 (reduction over every output row, chunked).  Returns
    (exact, absprod), each [Cout, len(taps), Cin]; ``taps`` = list of (kh, kw), all taps if None."""
    N, H, W, Cin = x.shape
    Ho, Wo = out_geometry(H, W, KH, KW, stride, pad, pool)
    M = N * Ho * Wo
    Cout = dy.shape[-1]
    taps = [(kh, kw) for kh in range(KH) for kw in range(KW)] if taps is None else list(taps)
    d2 = dy.reshape(M, Cout)
    out = torch.zeros(Cout, len(taps), Cin, dtype=torch.float64, device=x.device)
    absp = torch.zeros_like(out)
    for c0 in range(0, M, chunk):
        rr = torch.arange(c0, min(M, c0 + chunk), device=x.device)
        g = _f64(d2[c0:c0 + chunk])
        for t, (kh, kw) in enumerate(taps):
            a = _pool_rows(x, rr, Ho, Wo) if pool else _f64(_tap_rows(x, rr, Ho, Wo, kh, kw, stride, pad))
            out[:, t] += g.t() @ a
            absp[:, t] += g.abs().t() @ a.abs()
    return out, absp


def gemm_exact(a, b, transpose_a=False):
    """float64 (exact, absprod) of the batched products: NT  C_b = A_b @ B_b^T  (a [B,M,K], b [B,N,K]), or with transpose_a the
    TN form  out_b = A_b^T @ B_b  (a [B,M,N], b [B,M,K])"""
    a, b = _f64(a), _f64(b)
    if transpose_a:
        return a.transpose(1, 2) @ b, a.abs().transpose(1, 2) @ b.abs()
    return a @ b.transpose(1, 2), a.abs() @ b.abs().transpose(1, 2)


def pooled_residual_rows(res, rows, Ho, Wo):
    """[R, C] residual the pooled-residual epilogue adds to output rows ``rows``: the pooled pixel (Ho//2 x Wo//2 map) each output
    pixel falls in, zero where an odd size leaves it without one (the 0.25 is applied by epilogue_exact)"""
    N, Hp, Wp, C = res.shape
    n, r = rows // (Ho * Wo), rows % (Ho * Wo)
    oh, ow = r // Wo, r % Wo
    ok = (oh // 2 < Hp) & (ow // 2 < Wp)
    idx = (n * Hp + (oh // 2).clamp(max=Hp - 1)) * Wp + (ow // 2).clamp(max=Wp - 1)
    return _f64(res.reshape(-1, C)[idx]) * ok.unsqueeze(1).to(torch.float64)


def epilogue_exact(acc, scale=None, bias=None, residual=None, relu=False, relu_mask=None, residual_pooled=False):
    """The conv epilogue in float64: relu?(acc * scale[n] + bias[n] + residual), zeroed where relu_mask <= 0.  ``residual`` /
    ``relu_mask`` are row-aligned with acc ([R, Cout]; a pooled residual as pooled_residual_rows gives it)."""
    v = _f64(acc)
    if scale is not None:
        v = v * _f64(scale)
    if bias is not None:
        v = v + _f64(bias)
    if residual is not None:
        v = v + (0.25 if residual_pooled else 1.0) * _f64(residual)
    if relu:
        v = v.clamp_min(0.0)
    if relu_mask is not None:
        v = torch.where(_f64(relu_mask) > 0, v, torch.zeros_like(v))
    return v


def round_bf16(t):
    """float64 -> the nearest bf16 (ties to even), as float64: what a correctly rounded store of the exact value gives"""
    t = _f64(t)
    f = t.to(torch.float32)
    # correct the rare double rounding: when f64 -> f32 rounded onto a bf16 tie point, step toward the f64 value
    bits = f.view(torch.int32)
    tie = (bits & 0xFFFF) == 0x8000
    fix = tie & (_f64(f) != t)
    if bool(fix.any()):
        nxt = torch.where(t > _f64(f), torch.nextafter(f, torch.full_like(f, math.inf)), torch.nextafter(f, torch.full_like(f, -math.inf)))
        f = torch.where(fix, nxt, f)
    return _f64(f.to(torch.bfloat16))


def truncate_bf16(t):
    """float64 -> bf16 rounded toward zero (a negative control: what a truncating store would give), as float64"""
    f = _f64(t).to(torch.float32)
    return _f64((f.view(torch.int32) & ~0xFFFF).view(torch.float32))


def sample_rows(M, row_bytes=(), per_tile=2, tile=256, seed=0, device="cpu"):
    """Output rows (flattened M index) a row-sampled check computes: ``per_tile`` random rows of every ``tile``-row tile, the first
    and last rows, every row of the last ragged tile, and -- for each row size in ``row_bytes`` -- the rows around every
    multiple of 2^31 bytes (the row that crosses it, its neighbours).  Sorted, unique, int64."""
    g = torch.Generator().manual_seed(seed)
    nt = (M + tile - 1) // tile
    r = (torch.arange(nt).repeat_interleave(per_tile) * tile + torch.randint(0, tile, (nt * per_tile,), generator=g)).clamp(max=M - 1)
    parts = [r, torch.tensor([0, M - 1])]
    if M % tile:
        parts.append(torch.arange((M // tile) * tile, M))
    for rb in ([row_bytes] if isinstance(row_bytes, int) else row_bytes):
        k = 1
        while k * 2 ** 31 < M * rb:
            m = (k * 2 ** 31) // rb
            parts.append(torch.arange(max(0, m - 1), min(M, m + 2)))
            k += 1
    return torch.unique(torch.cat(parts)).to(device)


def bound(exact, absprod, out_dtype, scale=None, bias=None, residual=None, base=None, c_acc=None):
    """per-element error bound (float64, exact's shape).  scale / bias broadcast over the last axis; residual / base (the dW an
    accumulating launch adds to) elementwise."""
    u = U_BF16 if out_dtype == torch.bfloat16 else U_F32
    c = C_ACC if c_acc is None else c_acc
    s = 1.0 if scale is None else _f64(scale).abs()
    acc = c * U_F32 * s * _f64(absprod)
    small = 0.0
    for t in (bias, residual, base):
        if t is not None:
            small = small + _f64(t).abs()
    return u * _f64(exact).abs() + (1.0 + u) * (acc + U_F32 * small)


def check_bound(got, exact, absprod, out_dtype, scale=None, bias=None, residual=None, base=None, c_acc=None):
    """-> (ok, worst |err| / bound, flat index of the worst element)"""
    err = (_f64(got) - _f64(exact)).abs()
    b = bound(exact, absprod, out_dtype, scale, bias, residual, base, c_acc)
    ratio = err / b.clamp_min(1e-300)
    ratio = torch.where(err == 0, torch.zeros_like(ratio), ratio)
    worst = int(ratio.argmax())
    return bool((err <= b).all()), float(ratio.reshape(-1)[worst]), worst


def acc_ratio(got, exact, absprod, scale=None, bias=None, residual=None, base=None):
    """worst accumulation error of an f32 output in units of 2^-24 * |scale| * sum|a*b| (what C_ACC must cover), after taking
    off the f32 rounding of the stored value and of the epilogue's adds"""
    err = (_f64(got) - _f64(exact)).abs()
    small = _f64(exact).abs()
    for t in (bias, residual, base):
        if t is not None:
            small = small + _f64(t).abs()
    s = 1.0 if scale is None else _f64(scale).abs()
    den = U_F32 * s * _f64(absprod)
    r = (err - 2 * U_F32 * small).clamp_min(0) / den.clamp_min(1e-300)
    return float(torch.where(den > 0, r, torch.zeros_like(r)).max())


def ulp_bf16(t):
    """spacing of bf16 numbers at |t| (float64; t != 0)"""
    e = torch.floor(torch.log2(_f64(t).abs()))
    return torch.pow(2.0, e - 7)


def rounding_bias(got, exact, absprod=None, scale=None):
    """-> (bias, n): mean of sign(exact) * (got - exact) / ulp_bf16(exact) over the elements with exact != 0 -- the signed store
    error in ulps of the output, measured toward zero.  Round-to-nearest-even gives ~0, truncation about -0.5.  With absprod,
    only elements whose accumulation bound is below 1/16 ulp count (the rounding, not the sum, decides them)."""
    g, e = _f64(got).reshape(-1), _f64(exact).reshape(-1)
    keep = e != 0
    if absprod is not None:
        s = 1.0 if scale is None else _f64(scale).abs()
        acc = (C_ACC * U_F32 * s * _f64(absprod)).reshape(-1)
        keep = keep & (acc < ulp_bf16(torch.where(keep, e, torch.ones_like(e))) / 16)
    g, e = g[keep], e[keep]
    if e.numel() == 0:
        return 0.0, 0
    return float((torch.sign(e) * (g - e) / ulp_bf16(e)).mean()), int(e.numel())


def old_criterion(got, ref, tol=2e-2):
    """the criterion tests/test_gpu_conv.py applies to bf16 results: max|got - ref| / max|ref| < tol"""
    return float((_f64(got) - _f64(ref)).abs().max() / _f64(ref).abs().max()) < tol
