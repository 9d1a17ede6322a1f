"""Exact references and an error bound for the OCP e4m3 (fp8) kernels: k_conv_fwd256<fp8e4> (kernel id 10), k_wgrad256_f8 (12),
k_fp8_dot_nt, the quantiser and the e4m3 second output of the 256x256 kernels (imported by the fp8 exact-product tests; not a
conftest).  Built on tests/exact_gemm.py: the float64 references are the same functions on the dequantised bytes.

An e4m3 x e4m3 product has 8 significant bits and is exact in f32; what is not exact is the sum.  One
v_mfma_scale_f32_32x32x64_f8f6f4 adds 64 products and the accumulator in a fixed-point adder aligned to the largest of them, and
cuts what falls below it -- measured by tools/mfma_f8_probe.hip, which issues single instructions on operands of its own against
float64 (figures below).  Per output element

  |got - exact| <= u_out |exact| + (1 + u_out) ( C_ACC 2^-24 |s| sum|a b| + |s| T_MFMA sum_g max_{k in g} |a_k b_k|
                                                   + 2^-24 (|bias| + |residual| + |dW before|) )

g runs over the 64-element groups one instruction consumes: kernel 10, 64 consecutive channels of one filter tap; kernel 12, the 64
output rows of one reduction tile; fp8_dot_nt, 64 consecutive k (conv_group_term / wgrad_group_term / dot_group_term compute the
sum from the dequantised operands)."""
import math

import torch

import exact_gemm as X
from exact_gemm import U_BF16, U_F32, _f64

# ---- T_MFMA: what one instruction loses of its own 64 products, in units of the largest |product| of the instruction.
# tools/mfma_f8_probe.hip on one MI355X (gfx950), worst |got - exact| / max|product| over every output:
#   (a) random operands, zero accumulator: 4.93e-4 (every finite code equally likely, 524 288 outputs, all inexact), 2.64e-4
#       (Gaussian quantised to a maximum of 448, 70 % inexact), 2.01e-4 (subnormal-range codes x Gaussian)
#   (b) one product of 2^j among 63 of 1: exact up to j = 13; from j = 14 seven of the 63 ones are lost (ratio 4.27e-4 at j = 14,
#       halving per j); among 63 products of 1.125^2: exact up to j = 7, worst 5.41e-4 = 2^-10.85 at j = 14
#   (c) accumulator 2^j + 64 products of 1: exact for every j <= 24; + 64 products of 2^-9: exact up to j = 18, from j = 19 the
#       whole 0.125 is dropped although 2^19 + 0.125 is an f32 number: the accumulator takes part in the alignment, and what lies
#       more than ~21 bits below it is cut, not rounded.  Relative to the products this is unbounded (64 at every j >= 19, 48 after
#       taking off the f32 rounding of the result); relative to the accumulator it is <= 2^-21 |acc|, an accumulation rounding:
#       it belongs to the C_ACC term (|acc| <= sum|a b|) and is measured there (acc_ratio), not here
#   (d) integers |v| <= 4 on an integer accumulator, |result| <= 2^17: 262 144 outputs, all exact; likewise |v| <= 8 up to 2^20
#       and |v| <= 16 up to 2^23 and 2^24
# T_MFMA = twice the worst zero-accumulator ratio, 2 x 5.41e-4 (the probe samples operand patterns, it does not enumerate them).
T_MFMA = 2 * 5.40733e-4
# Tier A operand range: (d) is exact, so tier A demands bit-equality on integers |v| <= 4 (every |v| <= 16 is an e4m3 number; 4
# keeps the longest reduction of the table, K = 9 * 512 = 4608, at partial sums <= 73 728 < 2^17, inside what (d) covered).
TIER_A_VMAX = 4
# C_ACC: exact_gemm's 8.  Measured on one MI355X over the f32-output tier B cases of tests/test_gpu_fp8_exact.py (the table it
# prints): acc_ratio -- the error left after the instruction term at the probe's own worst ratio, T_MFMA / 2, in units of
# 2^-24 |s| sum|a b| -- is 0 for k_conv_fwd256<fp8e4>, k_wgrad256_f8 and k_fp8_dot_nt alike: the instruction's cut explains every
# error seen, with room (worst error / (|s| sum_g max|a b|): 3.34e-4 on the one-tile weight gradient, M = 15; 2.85e-4 on
# fp8_dot_nt; 1.30e-4 on the forward kernel -- all below the probe's 5.41e-4).  The whole error in units of 2^-24 |s| sum|a b|
# (exact_gemm.acc_ratio, printed as raw_acc_ratio) is 50 to 3 500 on these short reductions -- the cut, not the accumulation --
# and 1.41 on the bench's weight gradient (1 605 632 rows = 25 088 chained instructions per element), where accumulation
# dominates and pattern (c)'s alignment to the accumulator would show: below 3.5, so C_ACC stays 8.
C_ACC = X.C_ACC

E4M3_MAX = 448.0


def deq(u8, dtype=torch.float64):
    """e4m3 bytes -> float64 (or f32: every e4m3 number is one), through torch.float8_e4m3fn (torch defines the format here;
    e4m3_rne below does not use it)"""
    return u8.contiguous().view(torch.float8_e4m3fn).to(torch.float32).to(dtype)


def _two_to(e):
    """2^e as float64 for an integer tensor e, built from the exponent field: exact on every device (a pow evaluated through
    exp / log need not be)"""
    return ((e.to(torch.int64) + 1023) << 52).view(torch.float64)


def e4m3_rne(t):
    """float64 -> the nearest e4m3fn number (ties to even), as float64: plain arithmetic, independent of torch's conversion.
    Saturates at +-448 (the kernels clamp first: e4m3fn has no infinity); subnormals are the multiples of 2^-9 below 2^-6.
    NaN stays NaN (what byte a kernel makes of it is a policy the tests pin separately)."""
    t = _f64(t)
    a = t.abs().clamp(max=E4M3_MAX)
    _, e = torch.frexp(a)                                    # a = m 2^e, m in [0.5, 1): floor(log2 a) = e - 1
    q = _two_to((e - 1).clamp(min=-6) - 3)                  # spacing of the grid at a: 3 mantissa bits, 2^-9 at the bottom
    v = torch.round(a / q) * q                               # torch.round: half to even; a / q and the product are exact
    v = torch.where(torch.isnan(t), t, v.clamp(max=E4M3_MAX))
    return torch.copysign(v, t)


def e4m3_encode(t):
    """float64 -> uint8 codes of e4m3_rne(t) (sign bit from t's sign; NaN -> 0x7f)"""
    v = e4m3_rne(t)
    a = v.abs()
    a0 = torch.where(torch.isnan(a), torch.zeros_like(a), a)
    _, e = torch.frexp(a0)
    e = (e - 1).clamp(min=-6)
    m = a0 / _two_to(e)                                      # [1, 2) for normals, [0, 1) for subnormals
    normal = a0 >= 2.0 ** -6
    code = torch.where(normal, ((e + 7) << 3) + ((m - 1.0) * 8.0).to(torch.int64), (a0 * 512.0).to(torch.int64))
    code = torch.where(torch.isnan(a), torch.full_like(code, 0x7F), code)
    code = code | torch.where(torch.signbit(v), 0x80, 0).to(torch.int64)
    return code.to(torch.uint8)


def same_codes(got, want):
    """number of bytes that differ, the sign of zero being free"""
    g, w = got.reshape(-1), want.reshape(-1)
    return int(((g != w) & ~(((g & 0x7F) == 0) & ((w & 0x7F) == 0))).sum())


# ---------------------------------------------------------------------------------------------------------------- operands
def tier_a_operand(shape, K, gen, device, vmax=TIER_A_VMAX):
    """integers in [-vmax, vmax] (an eighth forced to zero) as e4m3 bytes, for a reduction of length K: every partial sum of
    K products stays below 2^24 in magnitude, so any order of f32 additions is exact"""
    assert K * vmax ** 2 < 2 ** 24, (K, vmax)
    assert vmax <= 16, "integers above 16 are not all e4m3 numbers"
    v = torch.randint(-vmax, vmax + 1, shape, device=device, generator=gen, dtype=torch.int16)
    v = torch.where(torch.randint(0, 8, shape, device=device, generator=gen, dtype=torch.int16) == 0, torch.zeros_like(v), v)
    codes = e4m3_encode(v.to(torch.float64))
    assert torch.equal(deq(codes), v.to(torch.float64))
    return codes


def tier_b_operand(shape, gen, device, chunk=1 << 24):
    """Gaussian values scaled so that the largest magnitude lands on 448, as e4m3 bytes: the whole code range, subnormals included"""
    n = math.prod(shape)
    g = torch.randn(n, device=device, generator=gen)
    g = g * (E4M3_MAX / float(g.abs().max()))
    out = torch.empty(n, device=device, dtype=torch.uint8)
    for i in range(0, n, chunk):
        out[i:i + chunk] = e4m3_encode(g[i:i + chunk])
    return out.view(shape)


# ---------------------------------------------------------------------------------------------------------------- group term
def group_sum(a, b, budget=1 << 25):
    """a [R, G, 64], b [N, G, 64] (dequantised operands, zeros where a kernel reads padding) -> [R, N] float64:
    sum over g of max_k |a[r, g, k] b[n, g, k]| -- the largest product of every instruction that feeds the element"""
    a, b = a.abs().to(torch.float32), b.abs().to(torch.float32)          # (|products| of e4m3 numbers are exact in f32)
    R, G, L = a.shape
    N = b.shape[0]
    out = torch.zeros(R, N, dtype=torch.float64, device=a.device)
    rs = max(1, min(R, budget // max(1, N * L)))                          # rows, then groups, per slice of at most ``budget`` products
    gs = max(1, budget // (rs * N * L))
    for r0 in range(0, R, rs):
        for g0 in range(0, G, gs):
            p = a[r0:r0 + rs, g0:g0 + gs].unsqueeze(1) * b[:, g0:g0 + gs].unsqueeze(0)      # [rs, N, gs, 64]
            out[r0:r0 + rs] += p.amax(-1).to(torch.float64).sum(-1)
    return out


def conv_group_term(x, w, pad=0, rows=None):
    """kernel 10: x [N,H,W,Cin], w [Cout,KH,KW,Cin] dequantised (stride 1) -> [R, Cout]; groups = 64 consecutive channels of a tap"""
    N, H, W, Cin = x.shape
    Cout, KH, KW, _ = w.shape
    Ho, Wo = X.out_geometry(H, W, KH, KW, 1, pad, False)
    if rows is None:
        rows = torch.arange(N * Ho * Wo, device=x.device)
    rows = rows.to(x.device, torch.int64)
    out = torch.zeros(len(rows), Cout, dtype=torch.float64, device=x.device)
    for kh in range(KH):
        for kw in range(KW):
            a = X._tap_rows(x, rows, Ho, Wo, kh, kw, 1, pad)
            out += group_sum(a.reshape(len(rows), Cin // 64, 64), w[:, kh, kw].reshape(Cout, Cin // 64, 64))
    return out


def wgrad_group_term(x, dy, KH, KW, pad, taps=None, tile=64):
    """kernel 12: x [N,H,W,Cin], dy [N,H,W,Cout] dequantised ("same" convolution) -> [Cout, taps, Cin]; groups = the ``tile`` output
    rows of one reduction tile (tiles start at row 0: a split owns whole tiles)"""
    N, H, W, Cin = x.shape
    Cout = dy.shape[-1]
    M = N * H * W
    T = (M + tile - 1) // tile
    taps = [(kh, kw) for kh in range(KH) for kw in range(KW)] if taps is None else list(taps)
    rows = torch.arange(M, device=x.device)
    d = torch.zeros(T * tile, Cout, dtype=torch.float32, device=x.device)       # (e4m3 numbers: exact in f32)
    d[:M] = dy.reshape(M, Cout).to(torch.float32)
    d = d.view(T, tile, Cout).permute(2, 0, 1).contiguous()
    out = torch.zeros(Cout, len(taps), Cin, dtype=torch.float64, device=x.device)
    for t, (kh, kw) in enumerate(taps):
        a = torch.zeros(T * tile, Cin, dtype=torch.float32, device=x.device)
        a[:M] = X._tap_rows(x, rows, H, W, kh, kw, 1, pad).to(torch.float32)
        out[:, t] = group_sum(d, a.view(T, tile, Cin).permute(2, 0, 1).contiguous())
    return out


def dot_group_term(a, b):
    """fp8_dot_nt: a [R, K], b [N, K] dequantised -> [R, N]; groups = 64 consecutive k"""
    return group_sum(a.reshape(a.shape[0], -1, 64), b.reshape(b.shape[0], -1, 64))


# ---------------------------------------------------------------------------------------------------------------- the bound
def pre_bound(absprod, gterm, scale=None, bias=None, residual=None, base=None, c_acc=None, t_mfma=None):
    """error of the unrounded value (before the store): the accumulation term, the instruction term, the epilogue's adds"""
    c = C_ACC if c_acc is None else c_acc
    t = T_MFMA if t_mfma is None else t_mfma
    s = 1.0 if scale is None else _f64(scale).abs()
    small = 0.0
    for v in (bias, residual, base):
        if v is not None:
            small = small + _f64(v).abs()
    return c * U_F32 * s * _f64(absprod) + s * t * _f64(gterm) + U_F32 * small


def bound(exact, absprod, gterm, out_dtype, scale=None, bias=None, residual=None, base=None, c_acc=None, t_mfma=None):
    u = U_BF16 if out_dtype == torch.bfloat16 else U_F32
    return u * _f64(exact).abs() + (1.0 + u) * pre_bound(absprod, gterm, scale, bias, residual, base, c_acc, t_mfma)


def check_bound(got, exact, absprod, gterm, out_dtype, scale=None, bias=None, residual=None, base=None, c_acc=None, t_mfma=None):
    """-> (ok, worst |err| / bound, flat index of the worst element)"""
    err = (_f64(got) - _f64(exact)).abs()
    b = bound(exact, absprod, gterm, out_dtype, scale, bias, residual, base, c_acc, t_mfma)
    ratio = err / b.clamp_min(1e-300)
    ratio = torch.where(err == 0, torch.zeros_like(ratio), ratio)
    ratio = torch.where(torch.isnan(err), torch.full_like(ratio, math.inf), ratio)
    worst = int(ratio.argmax())
    return bool((err <= b).all()), float(ratio.reshape(-1)[worst]), worst


def acc_ratio(got, exact, absprod, gterm, scale=None, bias=None, residual=None, base=None):
    """worst error of an f32 output BEYOND the instruction term at the probe's own worst ratio (T_MFMA / 2), in units of
    2^-24 |s| sum|a b| -- what C_ACC must cover -- after taking off the f32 rounding of the stored value and of the epilogue's adds
    (exact_gemm.acc_ratio with the instruction's cut taken off first: on e4m3 operands that cut is hundreds of such units)"""
    err = (_f64(got) - _f64(exact)).abs()
    small = _f64(exact).abs()
    for t in (bias, residual, base):
        if t is not None:
            small = small + _f64(t).abs()
    s = 1.0 if scale is None else _f64(scale).abs()
    den = U_F32 * s * _f64(absprod)
    r = (err - 2 * U_F32 * small - s * (T_MFMA / 2) * _f64(gterm)).clamp_min(0) / den.clamp_min(1e-300)
    return float(torch.where(den > 0, r, torch.zeros_like(r)).max())


def mfma_ratio(got, exact, gterm, scale=None):
    """worst error of an f32 output in units of |s| sum_g max|a b| (what T_MFMA must cover), the f32 rounding of the stored value taken off"""
    err = ((_f64(got) - _f64(exact)).abs() - U_F32 * _f64(exact).abs()).clamp_min(0)
    s = 1.0 if scale is None else _f64(scale).abs()
    den = s * _f64(gterm)
    return float(torch.where(den > 0, err / den.clamp_min(1e-300), torch.zeros_like(err)).max())


def round_e4m3_toward_zero(t):
    """negative control: float64 -> e4m3 grid, magnitude truncated (as float64)"""
    t = _f64(t)
    a = t.abs().clamp(max=E4M3_MAX)
    _, e = torch.frexp(a)
    q = _two_to((e - 1).clamp(min=-6) - 3)
    return torch.copysign(torch.floor(a / q) * q, t)


def midpoints_f32():
    """every midpoint between two neighbouring non-negative e4m3 numbers (and 448 | 480, the edge of saturation) with its two f32
    neighbours, both signs: [n] float32 -- where round-to-nearest-even is decided"""
    grid = deq(torch.arange(0, 0x7F, dtype=torch.uint8))                      # 0 .. 448, ascending
    mid = torch.cat([(grid[:-1] + grid[1:]) / 2, torch.tensor([464.0], dtype=torch.float64)]).to(torch.float32)
    inf = torch.full_like(mid, math.inf)
    pts = torch.cat([mid, torch.nextafter(mid, inf), torch.nextafter(mid, -inf)])
    return torch.cat([pts, -pts])
