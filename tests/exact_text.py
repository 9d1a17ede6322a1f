"""Checker of the CLIP text tower's kernels (cddmsl_amd/csrc/text_encoder.hip) and of the GPT-2 decoder's (csrc/gpt2.hip): float64
references of the operands the kernels were given, the bounds their outputs are held to, and float32 emulations (and mutants) that
tests/test_text_bound_host.py runs against the same references and bounds.  Imports without a GPU; every function takes tensors
of any device.  u = 2^-24 (f32).  One round-to-nearest store of y in a format of p bits is off by at most half_ulp(y) =
2^(floor(log2 |y|) - p), which lies between 2^-(p+1) |y| and 2^-p |y| (p = 8 for bf16: a relative 2^-9 |y| is NOT a bound of a
correctly rounded bf16 store, 1.0039 -> 1.0 is off by 2^-8; the half ulp is the exact statement and the one used here).

attn_causal   |got - ref| <= 2^-8 (|ref| + max_{j<=i} |v_j|) + 1e-6.  P is rounded to bf16 before P V: each weight moves by at most
              2^-8 relative, the output by at most 2^-8 max_j |v_j| since the weights sum to 1; the output store is at most 2^-8 |o|.
              The roundings rarely all reach half an ulp, which leaves room for the f32 softmax and accumulation (a few hundred u);
              the host emulation measures 0.63 of the bound.  (The bound and the reference are those of tests/test_gpu_text.py.)
text_pool     y = (x - mean) rstd gamma + beta per gathered row, nk = W / 64 registers per lane.  The f32 mean is a sum of depth
              nk + 6 (registers, then the wave butterfly) and one division: |dmean| <= (nk + 7) u max|x|.  d = x - mean adds u |d|.
              The variance sums d^2 at the same depth (a shifted mean enters only in second order), then / W, + eps, rsqrtf (2 ulp):
              rstd carries ((nk + 10) / 2 + 4) u relative.  Two products and the sum with beta: 3 u |y - beta| + u |y|.  Together
                |dy| <= [(nk + 7) max|x| + (nk / 2 + 13) |x - mean|] u rstd |gamma| + u |y|
              which scales with u max|x| rstd |gamma|: a row of mean 1e3 and unit spread loses three digits to the cancellation in
              x - mean, and the bound says so.  The group mean adds group roundings of the running sum and two of the final product:
              (group + 2) u mean_p |y_p|.  bf16 output: + half_ulp(out), and the GPU test also requires it bit-equal to the
              rounding of the f32 output.
activations   g = F(x) on the STORED operand (the bf16 value for bf16).  |got - g| <= C_ACT u |x| + output rounding.  The bound is
              absolute in |x| and must not be relative to |g|: gelu_new's 1 + tanh(..) and QuickGELU's 1 / (1 + e^y) lose all relative
              accuracy where g ~ 0 (x ~ -4 and below; once f32 tanh returns -1 the result is -0) while the absolute
              error stays a few u |x|.  C_ACT = 8: QuickGELU's fast exponential takes its argument through two products (x 1.702f,
              x log2 e), a relative (3 y + 2) u of e^-y with y e^-y <= 0.37, so <= 3.1 u on the sum, + the reciprocal, the sum and
              the product <= 6 u |x|; gelu_new's inner polynomial (4 u relative, times |z| sech^2 z <= 0.45), tanhf (2 ulp), the sum
              and two products <= 4.5 u |x|.  Output rounding: half_ulp(g) of the output format.
skinny_gemm   tier A: integer operands |x|, |w| <= 4, so every partial sum is an integer below 2^24 and exact in any order; the f32
              output (epi 1) is the exact value and the bf16 output (epi 0) its single rounding.  Tier B: the existing bound
              (K + S + 4) u sum|x||w| + .. of tests/test_gpu_caption.py."""
import numpy as np
import torch

U = 2.0 ** -24
EPS_BF16 = 2.0 ** -8                 # twice bf16's unit roundoff
C_ACT = 8.0
PREC = {torch.float32: 24, torch.bfloat16: 8}                           # significand bits of the output formats
GELU_C = 0.7978845608028654


def bits_equal(a, b):
    it = {torch.float32: torch.int32, torch.bfloat16: torch.int16, torch.float64: torch.int64}[a.dtype]
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(it), b.contiguous().view(it))


def half_ulp(y, dtype):
    """half the spacing of ``dtype`` at |y|: 2^(floor(log2 |y|) - p), the largest error of one round-to-nearest store (between
    2^-(p+1) |y| and 2^-p |y|; the subnormal spacing below 2^-126)"""
    e = torch.frexp(y.double().abs())[1].double() - 1
    e = torch.where(y == 0, torch.full_like(e, -126.0), e).clamp_min(-126.0)
    return torch.pow(torch.full_like(e, 2.0), e - PREC[dtype])


def ratio(err, bound):
    """worst err / bound; an exceeded zero bound is infinite, a met one 0; a NaN error is infinite"""
    err, bound = torch.nan_to_num(err.double(), nan=float("inf"), posinf=float("inf")), bound.double()
    r = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    return float(r.max()) if r.numel() else 0.0


# ------------------------------------------------------------------------------------------------ causal attention
def attn_ref(qkv, n, t, heads, scale=0.125):
    """float64 causal attention of the bf16 operands: ([n*t, W], v [n, heads, t, 64])"""
    W = qkv.shape[1] // 3
    q, k, v = qkv.double().view(n, t, 3, heads, 64).permute(2, 0, 3, 1, 4)
    mask = torch.full((t, t), float("-inf"), dtype=torch.float64, device=qkv.device).triu(1)
    p = torch.softmax(q @ k.transpose(-1, -2) * scale + mask, dim=-1)
    return (p @ v).permute(0, 2, 1, 3).reshape(n * t, W), v


def attn_bound(ref, v, n, t, heads):
    """2^-8 (|ref| + max_{j <= i} |v_j|) + 1e-6 (module docstring), [n*t, W]"""
    vmax = v.abs().cummax(dim=2).values                                  # [n, heads, t, 64]: max over keys j <= i, per channel
    vmax = vmax.amax(dim=-1, keepdim=True).expand(-1, -1, -1, 64).permute(0, 2, 1, 3).reshape(n * t, heads * 64)
    return EPS_BF16 * (ref.abs() + vmax) + 1e-6


def check_attn_bound(got, ref, v, n, t, heads):
    err = (got.double() - ref).abs()
    bound = attn_bound(ref, v, n, t, heads)
    assert bool((err <= bound).all()), (float((err / bound).max()), t, heads)
    return float((err / bound).max())


def attn_emulate(qkv, n, t, heads, scale=0.125):
    """the kernel's arithmetic in torch f32 (another summation order): f32 scores and softmax, P rounded to bf16, f32 P V, the
    output rounded to bf16"""
    W = qkv.shape[1] // 3
    q, k, v = qkv.float().view(n, t, 3, heads, 64).permute(2, 0, 3, 1, 4)
    s = (q @ k.transpose(-1, -2)) * np.float32(scale)
    s = s.masked_fill(torch.ones(t, t, dtype=torch.bool).triu(1), float("-inf"))
    e = torch.exp(s - s.amax(-1, keepdim=True))
    p = (e * (1.0 / e.sum(-1, keepdim=True))).bfloat16().float()
    return (p @ v).permute(0, 2, 1, 3).reshape(n * t, W).bfloat16()


def attn_case(n, t, heads, seed=0):
    """random qkv [n*t, 3 W] bf16 on the CPU"""
    g = torch.Generator().manual_seed(1000 * t + 10 * heads + n + seed)
    return (torch.randn(n * t, 3 * heads * 64, generator=g) * 1.5).bfloat16()


def attn_dominant_case(n, t, heads):
    """for scale = 0.125: q_i = 64 e_0 and k_j = 4 (j + 1) e_0 (exact in bf16), so the logit of key j is 32 (j + 1), 32 above every
    earlier key's and up to 32 t >= 60: row i's softmax is its own key's to 1e-14 and the output row is v_i within the bound"""
    qkv = torch.zeros(n, t, 3, heads, 64)
    qkv[:, :, 0, :, 0] = 64.0
    qkv[:, :, 1, :, 0] = (torch.arange(t, dtype=torch.float32) + 1).view(1, t, 1) * 4.0
    g = torch.Generator().manual_seed(t)
    qkv[:, :, 2] = torch.randn(n, t, heads, 64, generator=g) * 2
    return qkv.view(n * t, 3 * heads * 64).bfloat16()


# ------------------------------------------------------------------------------------------------ text_pool
def pool_ref(x, rows, gamma, beta, group, eps=1e-5, out_dtype=torch.float32):
    """(float64 LayerNorm + group mean [nout, W], bound [nout, W]) of the f32 operands"""
    W = x.shape[1]
    nk = W // 64
    xs, g, b = x.double()[rows], gamma.double(), beta.double()
    mean = xs.mean(1, keepdim=True)
    d = xs - mean
    rstd = 1.0 / torch.sqrt((d * d).mean(1, keepdim=True) + eps)
    y = d * rstd * g + b
    xmax = xs.abs().amax(1, keepdim=True)
    dy = ((nk + 7) * xmax + (nk / 2 + 13) * d.abs()) * U * rstd * g.abs() + U * y.abs()
    nout = rows.numel() // group
    out = y.view(nout, group, W).mean(1)
    bound = dy.view(nout, group, W).mean(1) + (group + 2) * U * y.abs().view(nout, group, W).mean(1)
    if out_dtype == torch.bfloat16:
        bound = bound + half_ulp(out.abs() + bound, torch.bfloat16)
    return out, bound + 1e-30


POOL_MUTANTS = ("unbiased variance", "eps omitted", "group mean before LN")


def pool_emulate(x, rows, gamma, beta, group, eps=1e-5, out_dtype=torch.float32, mutant=None):
    """f32 torch emulation of k_text_pool with torch's (pairwise) sums instead of the kernel's register-then-butterfly order"""
    assert mutant is None or mutant in POOL_MUTANTS
    W = x.shape[1]
    nout = rows.numel() // group
    xs = x.float()[rows]
    if mutant == "group mean before LN":
        xs = xs.view(nout, group, W).mean(1, keepdim=True).expand(nout, group, W).reshape(nout * group, W)
    mean = xs.sum(1, keepdim=True) / W
    d = xs - mean
    var = (d * d).sum(1, keepdim=True) / (W - 1 if mutant == "unbiased variance" else W)
    rstd = torch.rsqrt(var + (0.0 if mutant == "eps omitted" else np.float32(eps)))
    y = d * rstd * gamma.float() + beta.float()
    acc = torch.zeros(nout, W)
    for p in range(group):
        acc = acc + y.view(nout, group, W)[:, p]
    return (acc * np.float32(np.float32(1.0) / np.float32(group))).to(out_dtype)


POOL_R = 12


def pool_case(W, nout, group, seed=0):
    """(x [R, W], rows [nout * group], gamma, beta) f32 on the CPU.  Row 0 is the constant 1.5 (variance 0: LayerNorm returns beta
    exactly), row 1 has variance 1e-6 (below eps: rstd is set by eps), row R - 1 has mean 1e3 and unit spread (cancellation in
    x - mean); the indices start R - 1, 1, 3, 3 (a repeat inside a group) and, with more than one output, the last group is row 0
    throughout (both ends of x; at group = 1 that output is exactly beta); every index is in range"""
    g = torch.Generator().manual_seed(1000 * W + 10 * group + nout + seed)
    x = torch.randn(POOL_R, W, generator=g) * 3 + 1
    x[0] = 1.5
    x[1] = 0.5 + 1e-3 * torch.randn(W, generator=g)
    x[POOL_R - 1] = 1000.0 + torch.randn(W, generator=g)
    gamma, beta = 1 + 0.1 * torch.randn(W, generator=g), 0.1 * torch.randn(W, generator=g)
    rows = torch.randint(1, POOL_R, (nout * group,), generator=g)
    for i, r in enumerate([POOL_R - 1, 1, 3, 3][:rows.numel()]):
        rows[i] = r
    if nout > 1:
        rows[-group:] = 0
    return x, rows, gamma, beta


# ------------------------------------------------------------------------------------------------ activations
def quick_gelu_ref(x):
    x = x.double()
    return x * (1.0 / (1.0 + torch.exp(-1.702 * x)))


def gelu_new_ref(x):
    x = x.double()
    return 0.5 * x * (1.0 + torch.tanh(GELU_C * (x + 0.044715 * x * x * x)))


ACT_REF = {"quick_gelu": quick_gelu_ref, "gelu_new": gelu_new_ref}


def act_bound(x, g, dtype):
    """C_ACT u |x| + the output rounding (module docstring); g = the float64 formula on the stored operand"""
    b = C_ACT * U * x.double().abs()
    return b + half_ulp(g.abs() + b, dtype)


def act_check(got, x, name):
    """-> worst err / bound over the finite entries.  Entries where the float64 formula is NaN must be NaN and no others; where it is
    infinite the result is that infinity"""
    g = ACT_REF[name](x)
    gd = got.double()
    assert torch.equal(torch.isnan(gd), torch.isnan(g)), (name, "NaN exactly where the formula is NaN")
    inf = torch.isinf(g)
    assert torch.equal(gd[inf], g[inf]), (name, "infinite entries")
    fin = torch.isfinite(g)
    assert bool(torch.isfinite(gd[fin]).all())
    return ratio((gd[fin] - g[fin]).abs(), act_bound(x[fin], g[fin], got.dtype))


def act_emulate(x, name):
    """f32 torch evaluation (torch's exp / tanh, the f32 constants), stored in x's dtype"""
    v = x.float()
    if name == "quick_gelu":
        g = v * (1.0 / (1.0 + torch.exp(np.float32(-1.702) * v)))
    else:
        g = np.float32(0.5) * v * (1.0 + torch.tanh(np.float32(GELU_C) * (v + np.float32(0.044715) * v * v * v)))
    return g.to(x.dtype)


BF16_MAX = float(torch.finfo(torch.bfloat16).max)
SPECIALS = [0.0, -0.0, 1e-40, -1e-40, 1e-3, -1e-3, 4.0, -4.0, 20.0, -20.0, 60.0, -60.0, 1e4, -1e4, BF16_MAX, -BF16_MAX,
            float("inf"), float("-inf"), float("nan")]


def specials(dtype):
    """the table of special operands, padded with 1.0 to a multiple of the kernel's 16-byte chunk"""
    per = 8 if dtype == torch.bfloat16 else 4
    vals = SPECIALS + [1.0] * (-len(SPECIALS) % per)
    return torch.tensor(vals, dtype=torch.float32).to(dtype)


# ------------------------------------------------------------------------------------------------ skinny GEMM, LM head
def skinny_bound(x, w, bias, S):
    """(K + S + 4) u (sum |x||w| + |bias|): the accumulation term of tests/test_gpu_caption.py's bound"""
    K = x.shape[1]
    a = x.double().abs() @ w.double().abs().t()
    return (K + S + 4) * U * (a + (bias.double().abs() if bias is not None else 0.0))


def small_ints(shape, seed, lim=4, zero_frac=0.5):
    """integers in [-lim, lim], about half of them zero (f32 tensor)"""
    g = torch.Generator().manual_seed(seed)
    v = torch.randint(-lim, lim + 1, shape, generator=g).float()
    return v * (torch.rand(shape, generator=g) >= zero_frac).float()


def topk_order(logits, B):
    """(values, indices) of the B best per row under 'larger value first, lower index among equal values'"""
    s = torch.sort(logits, dim=1, descending=True, stable=True)
    return s.values[:, :B], s.indices[:, :B]


def lse_chain(V):
    """the longest chain of additions in k_lm_head_topk's sum of exponentials (as tests/test_gpu_beam.py counts it)"""
    return -(-V // 512) + 6 + 7 + 8


# ------------------------------------------------------------------------------------------------ decode attention
def decode_ref(q, k, v, scale):
    """q [n, H, 64], k / v [n, L, H, 64] float64 -> (o [n, H * 64], vmax [n, H * 64])"""
    n, H = q.shape[:2]
    p = torch.softmax(torch.einsum("nhd,nlhd->nhl", q, k) * scale, dim=-1)
    ref = torch.einsum("nhl,nlhd->nhd", p, v).reshape(n, H * 64)
    return ref, v.abs().amax(dim=(1, 3)).repeat_interleave(64, dim=1)


def decode_bound(ref, vmax):
    """tests/test_gpu_caption.py's: the bf16 store 2^-8 |ref|, the f32 softmax and sum 1e-4 max |v|"""
    return EPS_BF16 * ref.abs() + 1e-4 * vmax

