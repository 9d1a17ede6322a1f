"""Exact references, per-element error bounds and the shared case list for the loss-side kernels (imported by
test_losses_bound_host.py and test_gpu_losses_exact.py; not a conftest): all of cddmsl_amd/csrc/losses.hip and the multi-tensor
clip-and-SGD step (k_sqnorm / k_sgd of elementwise.hip).

Every reference takes the operands a kernel was given, as stored (f32, or bf16 for LayerNorm's y / dy), and computes in float64.
Scalars are rounded to f32 first (they cross the C-ABI as float); invT = f32(1 / f32(T)) as the host computes it.  A backward
kernel works from saved forward results (inv, mean / rstd, probs, rlse / clse): its reference works from the values it was given,
so the error of a stage is attributed to that stage.  Units: u = 2^-24.  A sum of depth d is off by at most d u sum|terms|:
  wave_sum      6 levels + the per-lane terms                      wave_depth(n)  = ceil(n / 64) + 6
  block_sum     a wave sum of ceil(n / 256) terms per lane + 4     block_depth(n) = ceil(n / 256) + 10
  k_sqnorm      per-lane terms + 6 + 3 (the four waves) + one atomic per block, in any order
Factor 1.01 covers the second-order terms throughout; TINY (exact_attn) the results below the normal range.

Math-function constants, relative error in units of u (1 ulp = 2 u):
  C_EXP0 / C_EXP1   expf at x: (C_EXP0 + C_EXP1 |x|) u -- fixed by exact_attn.py (c_exp)
  C_DIV  = 1        f32 division: correctly rounded.  The build (HIPFLAGS of __graft_entry__.py: -O3 -ffp-contract=off; _lib.py only
                    loads the library) sets no fast-math, approximate-function or approximate-division flag, and hipcc's default is
                    -fhip-fp32-correctly-rounded-divide-sqrt (its --help lists the -fno- form as the opt-out).
  C_SQRT = 1        sqrtf: correctly rounded, same flag.
  C_LOG  = 2        logf:   1 ulp  } ASSUMPTION: the figure of the HIP math-API accuracy table for the device library without
  C_LOG1P = 2       log1pf: 1 ulp  } fast-math; the table is not available where this was written, so these four are marked as
  C_POW  = 2        powf:   1 ulp  } assumptions (logf, log1pf, powf, rsqrtf) rather than derived.  None is fitted to a kernel's
  C_RSQRT = 2       rsqrtf: 1 ulp  } output.

L2 (256 threads per row):  ss = sum x^2 (block_depth + 1 for the product, all terms positive: relative), iv = 1 / max(sqrt ss, eps):
  r_iv = (d/2 + C_SQRT + C_DIV) u (max is 1-Lipschitz);  y = x iv: (r_iv + u) |y|.
  backward from the given y, inv:  dx = inv (dy - y dot), dot = sum dy y: cancels, so ABSOLUTE terms |inv| (|y| e_dot + u |y dot|)
  stand next to the relative 2 u |dx|.
Cosine logits (one wave per row):  iv as above at wave depth; dot_c = sum (x iv) w: (r_iv + (depth + 2) u) sum|x w| iv; times invT.
  The background column is +0.0 bit for bit.  Backward from the given inv: g_d = sum_c (ds_c invT) w_cd ((Kc + 2) u sum|.|),
  dot = sum g xh, v = inv (g - xh dot): ABSOLUTE |inv| (e_g + |xh| e_dot + 2 u |xh dot|); accumulate adds u |dx0 + v|.  Both branches
  (registers for D <= 1024, two passes above) form the same sums.
Contrastive:  lse = m + logf(sum expf(s - m)): the rounded argument adds u |x| to c_exp(x); r_se = sum p (c_exp + u |x|) + depth u;
  |err| <= r_se + C_LOG u |log se| + u |lse|.  loss from the given rlse / clse: (3 + depth) u sum(|rl - s_ii| + |cl - s_ii|) / 2n.
  dS from the given rlse / clse: g = e^(s - rl) + e^(s - cl) - 2 [i = j] cancels on the diagonal: ABSOLUTE
  scale (p_r (c_exp + u |a_r|) + p_c (c_exp + u |a_c|) + u (p_r + p_c)), scale = |gloss| / 2n.
LayerNorm (one wave per row, both the register form and the generic one bounded at the generic depth):
  e_mu = depth u sum|x| / D + C_DIV u |mu|;  var = sum (x - mu~)^2 / D: a shifted mean adds exactly e_mu^2 (sum (x - mu) = 0), the
  roundings (depth + 3) u var;  rstd: r_rs = e_var / 2(var + eps) + (C_RSQRT + 1) u;  y before its store:
  |rs g| (e_mu + u |c|) + |c rs g| (r_rs + 2 u) + u |y|;  a bf16 y gets store_bound of that (a truncating store is off by up to 2 u_b |y|
  and already leaves it at some element) and store_bias, the signed store error, pooled over all the cases of a run and judged where
  at least 20000 elements have been seen (one R = 37 case at D >= 768 alone, or the whole case list together).
  backward from the given mean, rstd:  v = rs (g - sg - xh sgx) cancels: ABSOLUTE |rs| (u |g| + e_sg + |xh| e_sgx + |sgx| e_xh + ...).
Focal CE (one lane per class):  p = e / se: (c_exp(x) + u |x| + r_se + C_DIV u) p;  ce = (m + logf se) - z_t: ABSOLUTE
  r_se + C_LOG u |log se| + u |m + log se|;  1 - pt cancels: e_omp = e_pt + u (1 - pt), carried through powf by evaluating the power at
  both ends of the interval (its slope is unbounded at 0 for gamma < 1).  gamma = 0: mod = 1 exactly.
  backward from the given probs (the kernel reads nothing else): ce = -logf(max(pt, 1e-38)); omp = 0 gives mod = dmod = 0.
RPN / box L1 (one block):  get_deltas in f32 (divisions, logf) bounded term by term (deltas_ref); BCE term
  max(x, 0) - x y + log1pf(expf(-|x|)): c_exp e + (C_LOG1P + 2) u t;  block sums at block_depth.  The delta gradient is
  sgn(delta - target) f32(gout inv_norm): compared BIT FOR BIT wherever the bound of the target decides the sign, exactly 0 at
  exact equality; unsampled entries stay exactly 0.
SGD:  norm^2 relative (depth + 1) u;  coef = min(clip / (sqrt + 1e-6), 1): r = r_ss / 2 + (C_SQRT + 1 + C_DIV) u;
  g' = g coef + wd p, m' = g' or momentum m + g', p' = p - lr m': each rounding counted once.
"""
import torch

import exact_gemm as X
from exact_attn import TINY, c_exp, check, store_bias, store_bound  # noqa: F401  (re-exported to the two test modules)
from exact_gemm import C_ACC, U_BF16, U_F32, rounding_bias  # noqa: F401

_f64 = X._f64
U = U_F32
S2 = 1.01
C_DIV, C_SQRT = 1.0, 1.0
C_LOG, C_LOG1P, C_POW, C_RSQRT = 2.0, 2.0, 2.0, 2.0      # assumptions: see the docstring
SGD_MAX = 96


def f32(v):
    return float(torch.tensor(float(v), dtype=torch.float32))


def inv_t(T):
    return float(torch.tensor(1.0, dtype=torch.float32) / torch.tensor(float(T), dtype=torch.float32))


def wave_depth(n):
    return (n + 63) // 64 + 6


def block_depth(n):
    return (n + 255) // 256 + 10


# ================================================================================================== references and bounds
def _inv_norm(x, eps, depth):
    ss = (x * x).sum(-1)
    iv = 1.0 / torch.clamp(ss.sqrt(), min=f32(eps))
    r = S2 * ((depth + 1) / 2 + C_SQRT + C_DIV) * U
    return iv, r


def l2_fwd(x, eps):
    x = _f64(x)
    iv, r = _inv_norm(x, eps, block_depth(x.shape[1]))
    y = x * iv[:, None]
    return dict(y=(y, S2 * (r + U) * y.abs() + TINY), inv=(iv, r * iv))


def l2_bwd(dy, y, inv):
    dy, y, iv = _f64(dy), _f64(y), _f64(inv)[:, None]
    d = block_depth(y.shape[1]) + 1
    dot = (dy * y).sum(-1, keepdim=True)
    e_dot = S2 * d * U * (dy * y).abs().sum(-1, keepdim=True)
    s = dy - y * dot
    dx = iv * s
    b = S2 * iv.abs() * (y.abs() * e_dot + U * (y * dot).abs() + U * s.abs()) + U * dx.abs() + TINY
    return dict(dx=(dx, b))


def cos_fwd(x, wn, T, eps):
    x, wn = _f64(x), _f64(wn)
    D = x.shape[1]
    it = inv_t(T)
    iv, r = _inv_norm(x, eps, wave_depth(D))
    sc = (x @ wn.t()) * iv[:, None] * it
    ab = (x.abs() @ wn.abs().t()) * iv[:, None] * it
    b = S2 * (r + (wave_depth(D) + 2) * U) * ab + U * sc.abs() + TINY
    return dict(scores=(sc, b), inv=(iv, r * iv))


def cos_bwd(ds, x, wn, inv, T, dx0=None):
    ds, x, wn, iv = _f64(ds), _f64(x), _f64(wn), _f64(inv)[:, None]
    D, Kc = x.shape[1], wn.shape[0]
    it = inv_t(T)
    dsv = ds[:, :Kc] * it
    g = dsv @ wn
    e_g = S2 * (Kc + 2) * U * (dsv.abs() @ wn.abs())
    xh = x * iv
    dot = (g * xh).sum(-1, keepdim=True)
    e_dot = S2 * ((e_g * xh.abs()).sum(-1, keepdim=True) + (wave_depth(D) + 2) * U * (g * xh).abs().sum(-1, keepdim=True))
    s = g - xh * dot
    v = iv * s
    b = S2 * iv.abs() * (e_g + xh.abs() * e_dot + 2 * U * (xh * dot).abs() + U * s.abs()) + U * v.abs() + TINY
    if dx0 is not None:
        v = _f64(dx0) + v
        b = b + U * v.abs()
    return dict(dx=(v, b))


def _lse(s, depth):
    """s [m, n] float64 -> (lse over the last axis, bound)"""
    mx = s.amax(-1, keepdim=True)
    x = s - mx
    e = torch.exp(x)
    se = e.sum(-1, keepdim=True)
    r_se = S2 * ((e * (c_exp(x) + U * x.abs())).sum(-1, keepdim=True) / se + depth * U)
    lse = mx + se.log()
    b = S2 * (r_se + C_LOG * U * se.log().abs()) + U * lse.abs() + s.shape[-1] * TINY
    return lse[:, 0], b[:, 0], r_se[:, 0]


def con_fwd(S, n):
    s = _f64(S)[:n, :n]
    rl, rb, _ = _lse(s, block_depth(n))
    cl, cb, _ = _lse(s.t(), block_depth(n))
    return dict(rlse=(rl, rb), clse=(cl, cb))


def con_loss(S, rl, cl, n):
    s = _f64(S)[:n, :n].diagonal()
    a, b = _f64(rl) - s, _f64(cl) - s
    loss = 0.5 * (a + b).sum() / n
    bd = S2 * (3 + block_depth(n)) * U * (a.abs() + b.abs()).sum() * 0.5 / n + (1 + C_DIV) * U * loss.abs() + TINY
    return dict(loss=(loss.reshape(1), bd.reshape(1)))


def con_bwd(S, rl, cl, gloss, n):
    s = _f64(S)[:n, :n]
    ar, ac = s - _f64(rl)[:, None], s - _f64(cl)[None, :]
    pr, pc = torch.exp(ar), torch.exp(ac)
    g = pr + pc - 2.0 * torch.eye(n, dtype=torch.float64)
    sc = _f64(gloss).reshape(()) * 0.5 / n
    dS = g * sc
    b = S2 * sc.abs() * (pr * (c_exp(ar) + U * ar.abs()) + pc * (c_exp(ac) + U * ac.abs()) + U * (pr + pc)) + (3 + C_DIV) * U * dS.abs() + TINY
    return dict(dS=(dS, b))


def ln_fwd(x, gamma, beta, eps, out_dtype):
    x, ga, be = _f64(x), _f64(gamma), _f64(beta)
    D = x.shape[1]
    d = wave_depth(D)
    ep = f32(eps)
    mu = x.mean(-1, keepdim=True)
    e_mu = S2 * (d * U * x.abs().sum(-1, keepdim=True) / D + C_DIV * U * mu.abs())
    c = x - mu
    var = (c * c).mean(-1, keepdim=True)
    e_var = S2 * ((d + 3 + C_DIV) * U * var + e_mu * e_mu + U * (var + ep))
    rs = (var + ep).rsqrt()
    r_rs = S2 * (0.5 * e_var / (var + ep) + C_RSQRT * U)
    y = c * rs * ga + be
    pre = S2 * ((rs * ga).abs() * (e_mu + U * c.abs()) + (c * rs * ga).abs() * (r_rs + 2 * U)) + TINY
    if out_dtype == torch.bfloat16:
        pre = pre + U * y.abs()
        yb = store_bound(y, pre)
    else:
        yb = pre + U * y.abs()
    return dict(y=(y, yb), y_pre=pre, mean=(mu[:, 0], e_mu[:, 0] + TINY), rstd=(rs[:, 0], (r_rs * rs)[:, 0]))


def ln_bwd(dy, x, gamma, mean, rstd, dx0=None):
    dy, x, ga = _f64(dy), _f64(x), _f64(gamma)
    mu, rs = _f64(mean)[:, None], _f64(rstd)[:, None]
    D = x.shape[1]
    d = wave_depth(D)
    g = dy * ga
    xh = (x - mu) * rs
    e_xh = S2 * 2 * U * xh.abs()
    sg = g.mean(-1, keepdim=True)
    e_sg = S2 * ((d + 1) * U * g.abs().sum(-1, keepdim=True) / D + C_DIV * U * sg.abs())
    sgx = (g * xh).mean(-1, keepdim=True)
    e_sgx = S2 * ((d + 4) * U * (g * xh).abs().sum(-1, keepdim=True) / D + C_DIV * U * sgx.abs())
    s = g - sg - xh * sgx
    v = rs * s
    b = S2 * rs.abs() * (U * g.abs() + e_sg + xh.abs() * e_sgx + sgx.abs() * e_xh + U * (xh * sgx).abs() + U * (g - sg).abs() + U * s.abs()) + U * v.abs() + TINY
    if dx0 is not None:
        v = _f64(dx0) + v
        b = b + U * v.abs()
    return dict(dx=(v, b))


def focal_fwd(z, t, gamma, bg_class, bg_weight):
    z = _f64(z)
    R, C = z.shape
    ga, bw = f32(gamma), f32(bg_weight)
    ar = torch.arange(R)
    mx = z.amax(-1, keepdim=True)
    x = z - mx
    e = torch.exp(x)
    se = e.sum(-1, keepdim=True)
    dl = c_exp(x) + U * x.abs()
    r_se = S2 * ((e * dl).sum(-1, keepdim=True) / se + 7 * U)
    p = e / se
    pb = S2 * p * (dl + r_se + C_DIV * U) + TINY
    lse = mx + se.log()
    ce = (lse - z[ar, t][:, None])[:, 0]
    e_ce = (S2 * (r_se + C_LOG * U * se.log().abs()) + U * lse.abs())[:, 0] + U * ce.abs()
    pt, e_pt = p[ar, t], pb[ar, t]
    w = torch.where(t == bg_class, torch.full_like(ce, bw), torch.ones_like(ce))
    if ga > 0:
        omp = (1 - pt).clamp_min(0)
        e_omp = e_pt + U * omp
        mod = omp ** ga
        hi, lo = (omp + e_omp) ** ga, (omp - e_omp).clamp_min(0) ** ga
        e_mod = torch.maximum(hi - mod, mod - lo) + C_POW * U * hi
    else:
        mod, e_mod = torch.ones_like(ce), torch.zeros_like(ce)
    row = ce * mod * w
    rb = S2 * w * (mod * e_ce + (ce.abs() + e_ce) * e_mod) + 2 * U * row.abs() + TINY
    return dict(row_loss=(row, rb), probs=(p, pb))


def focal_bwd(t, probs, gscale, gamma, bg_class, bg_weight):
    p = _f64(probs)
    R, C = p.shape
    ga, bw = f32(gamma), f32(bg_weight)
    gs = _f64(gscale).reshape(())
    ar = torch.arange(R)
    pt = p[ar, t][:, None]
    one = torch.zeros_like(p)
    one[ar, t] = 1.0
    w = torch.where(t == bg_class, torch.full_like(pt[:, 0], bw), torch.ones_like(pt[:, 0]))[:, None]
    if ga > 0:
        ce = -torch.log(pt.clamp_min(f32(1e-38)))
        omp = (1 - pt).clamp_min(0)
        pos = omp > 0
        safe = torch.where(pos, omp, torch.ones_like(omp))
        mod = torch.where(pos, safe ** ga, torch.zeros_like(omp))
        dmod = torch.where(pos, -ga * safe ** (ga - 1.0) * pt * (one - p), torch.zeros_like(p))
        A, B = mod * (p - one), ce * dmod
        rA, rB = (ga + C_POW + 2) * U, (C_LOG + abs(ga - 1.0) + C_POW + 5) * U
    else:
        A, B = p - one, torch.zeros_like(p)
        rA, rB = U, 0.0
    g = w * (A + B) * gs
    b = S2 * (w * gs).abs() * (rA * A.abs() + rB * B.abs() + U * (A + B).abs()) + 2 * U * g.abs() + 16 * TINY * (1 + gs.abs())
    return dict(dlogits=(g, b))


def deltas_ref(s, t, w):
    """get_deltas4 of losses.hip: s, t [n, 4] -> (d [n, 4] float64, bound of the f32 result)"""
    s, t = _f64(s), _f64(t)
    w = [f32(v) for v in w]

    def cw(b, i):
        sz = b[:, i + 2] - b[:, i]
        e_sz = U * sz.abs()
        c = b[:, i] + 0.5 * sz
        return sz, e_sz, c, 0.5 * e_sz + U * c.abs()

    d, e = [None] * 4, [None] * 4
    for i in (0, 1):
        sw, e_sw, sx, e_sx = cw(s, i)
        tw, e_tw, tx, e_tx = cw(t, i)
        num = tx - sx
        e_num = e_tx + e_sx + U * num.abs()
        d[i] = w[i] * num / sw
        e[i] = S2 * (abs(w[i]) * e_num / sw.abs() + d[i].abs() * (3 + C_DIV) * U) + TINY
        lg = torch.log(tw / sw)
        d[i + 2] = w[i + 2] * lg
        e[i + 2] = S2 * (abs(w[i + 2]) * ((2 + C_DIV) * U + C_LOG * U * lg.abs()) + U * d[i + 2].abs()) + TINY
    return torch.stack(d, 1), torch.stack(e, 1)


def _l1_parts(delta, tgt, e_tgt):
    e = _f64(delta) - tgt
    eb = e_tgt + U * e.abs()
    return e, eb


def _sgn_expect(e, eb, gl):
    """expected gradient sgn(e) * gl as f32 (bit-exact) and the mask of elements whose sign the target's bound leaves open"""
    decided = (e.abs() > eb) | (e == 0)
    return (torch.sign(e) * gl).to(torch.float32), decided


def rpn_ref(logits, deltas, pos, neg, midx, gt, gt_off, anchors, A, w, inv_norm, gout=None):
    lg, inn = _f64(logits), f32(inv_norm)
    n = pos.numel() + neg.numel()
    d = block_depth(n)
    rows = torch.cat([pos, neg])
    x = lg[rows]
    y = torch.cat([torch.ones(pos.numel()), torch.zeros(neg.numel())]).double()
    img = torch.div(pos, A, rounding_mode="floor")
    tgt, e_tgt = deltas_ref(anchors[pos - img * A], gt[midx[pos] + gt_off[img]], w)
    e, eb = _l1_parts(deltas[pos], tgt, e_tgt)
    if gout is None:
        ex = torch.exp(-x.abs())
        t = x.clamp_min(0) - x * y + torch.log1p(ex)
        e_t = c_exp(x) * ex + (C_LOG1P + 2) * U * t
        cls = t.sum() * inn
        cb = S2 * inn * (e_t.sum() + d * U * t.sum()) + U * cls.abs() + TINY
        loc = e.abs().sum() * inn
        lb = S2 * inn * (eb.sum() + d * U * e.abs().sum()) + U * loc.abs() + TINY
        return dict(out2=(torch.stack([cls, loc]), torch.stack([cb, lb])))
    g32 = gout.float() * torch.tensor(inn, dtype=torch.float32)          # gc, gl as the kernel forms them
    gc, gl = _f64(g32[0]), g32[1]
    ex = torch.exp(-x)
    sig = 1 / (1 + ex)
    r_sig = S2 * (ex / (1 + ex) * c_exp(x) + (1 + C_DIV) * U)
    dl = torch.zeros_like(lg)
    db = torch.zeros_like(lg)
    dl[rows] = (sig - y) * gc
    db[rows] = gc.abs() * sig * r_sig + 3 * U * dl[rows].abs() + TINY
    dd = torch.zeros(deltas.shape, dtype=torch.float32)
    ok = torch.ones(deltas.shape, dtype=torch.bool)
    dd[pos], ok[pos] = _sgn_expect(e, eb, gl)
    return dict(dlogits=(dl, db), ddeltas=dd, decided=ok)


def box_ref(deltas, fg, cls, src, tgt, w, inv_norm, gout=None):
    inn = f32(inv_norm)
    c0 = 4 * cls[fg] if cls is not None else torch.zeros_like(fg)
    cols = c0[:, None] + torch.arange(4)[None, :]
    tg, e_tg = deltas_ref(src[fg], tgt[fg], w)
    e, eb = _l1_parts(deltas[fg[:, None], cols], tg, e_tg)
    if gout is None:
        loss = e.abs().sum() * inn
        b = S2 * inn * (eb.sum() + block_depth(fg.numel()) * U * e.abs().sum()) + U * loss.abs() + TINY
        return dict(out1=(loss.reshape(1), b.reshape(1)))
    g = (gout.float().reshape(()) * torch.tensor(inn, dtype=torch.float32))
    dd = torch.zeros(deltas.shape, dtype=torch.float32)
    ok = torch.ones(deltas.shape, dtype=torch.bool)
    dd[fg[:, None], cols], ok[fg[:, None], cols] = _sgn_expect(e, eb, g)
    return dict(ddeltas=dd, decided=ok)


def sgd_grid(sizes):
    """grid.x of each tensor's launch pair: gsz(max size of its batch of SGD_MAX, 2048 elements per block, cap 256)"""
    out = []
    for b0 in range(0, len(sizes), SGD_MAX):
        mx = max(sizes[b0:b0 + SGD_MAX])
        out += [min(256, max(1, (mx + 2047) // 2048))] * len(sizes[b0:b0 + SGD_MAX])
    return out


def sgd_ref(ps, gs, ms, lr, momentum, wd, clip, first_step, exact_scalars=False):
    """lists of 1-D tensors (as stored before the step) -> list of dict(norm=(e, b), p=(e, b), m=(e, b)).  exact_scalars: take the
    scalars and the 1e-6 as the doubles given (for the comparison with the float64 oracle), not rounded to f32 as the kernel gets them"""
    r32 = (lambda v: v) if exact_scalars else f32
    lr, mo, wd, clip = r32(lr), r32(momentum), r32(wd), r32(clip)
    grid = sgd_grid([p.numel() for p in ps])
    out = []
    for p, g, m, gx in zip(ps, gs, ms, grid):
        p, g = _f64(p), _f64(g)
        n = p.numel()
        depth = (n + gx * 256 - 1) // (gx * 256) + 3 + 6 + 3 + gx + 1
        ss = (g * g).sum()
        r_ss = S2 * depth * U
        c = clip / (ss.sqrt() + r32(1e-6))
        coef = c.clamp(max=1.0)
        e_coef = S2 * (r_ss / 2 + (C_SQRT + 1 + C_DIV) * U) * coef
        g2 = g * coef + wd * p
        e_g = g.abs() * e_coef + U * ((g * coef).abs() + (wd * p).abs() + g2.abs())
        if first_step:
            m2, e_m = g2, e_g
        else:
            m2 = mo * _f64(m) + g2
            e_m = e_g + U * ((mo * _f64(m)).abs() + m2.abs())
        p2 = p - lr * m2
        e_p = lr * e_m + U * ((lr * m2).abs() + p2.abs())
        out.append(dict(norm=(ss.reshape(1), (r_ss * ss + TINY).reshape(1)), m=(m2, S2 * e_m + TINY), p=(p2, S2 * e_p + TINY)))
    return out


# ================================================================================================== judging
class Report:
    """collects the checks of one implementation (a kernel, its emulation or a mutant): bound checks keep the worst ratio per
    output, bit-exact checks and store-bias checks add a failure line.  The signed store error is judged per case where the case
    has 20000 elements, and pooled over every case seen (``pool``: output -> [sum of ulps, elements]) by finish()"""

    def __init__(self):
        self.worst, self.fail, self.bias, self.pool = {}, [], {}, {}

    def bound(self, name, case, got, eb, bias=None):
        ok, r, w = check(got, eb[0], eb[1])
        self.worst[name] = max(self.worst.get(name, 0.0), r)
        if not ok:
            self.fail.append(f"{name} [{case}]: worst |err|/bound {r:.3g} at element {w}: got {float(_f64(got).reshape(-1)[w])!r}, "
                             f"exact {float(_f64(eb[0]).reshape(-1)[w])!r}")
        if bias is not None:
            rb, n = store_bias(got, *bias)
            acc = self.pool.setdefault(name, [0.0, 0])
            acc[0] += rb * n
            acc[1] += n
            if n >= 20000:
                self.bias[name] = max(self.bias.get(name, 0.0), abs(rb))
                if abs(rb) > 0.02:
                    self.fail.append(f"{name} [{case}]: store bias {rb:+.4f} ulp over {n} elements")

    def exact(self, name, case, ok, what):
        if not ok:
            self.fail.append(f"{name} [{case}]: {what}")

    def finish(self):
        """judge the pooled store bias of every output"""
        for name, (sm, n) in self.pool.items():
            if n >= 20000:
                self.bias[name] = max(self.bias.get(name, 0.0), abs(sm / n))
                if abs(sm / n) > 0.02:
                    self.fail.append(f"{name} [all cases]: store bias {sm / n:+.4f} ulp over {n} elements")
        return self

    @property
    def rejected(self):
        return bool(self.fail)


def bits_equal(a, b):
    """same bit patterns (NaN payloads and the sign of zero included)"""
    iv = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(iv[a.element_size()]), b.contiguous().view(iv[b.element_size()]))


def pos_zero(t):
    return bool((t == 0).all()) and not bool(torch.signbit(t).any())


# ================================================================================================== the shared case list
def _g(seed):
    return torch.Generator().manual_seed(seed)


def _randn(shape, seed, s=1.0):
    return torch.randn(shape, generator=_g(seed)) * s


def l2_cases():
    return [dict(R=R, D=D, eps=eps) for R in (1, 5) for D in (1, 63, 256, 257, 1024) for eps in (0.0, 1e-12)]


def cos_cases():
    return [dict(R=R, D=D, Kc=Kc, T=0.01, acc=acc) for D in (64, 200, 1024, 1030, 1088) for R, Kc in ((1, 1), (5, 8), (6, 20), (5, 20))
            for acc in (0, 1)]


def con_cases():
    return [dict(n=n, pad=pad, scale=sc, gloss=1.0 if (pad == 0 and sc == 1.0) else -0.37)
            for n in (1, 3, 48, 257, 300) for pad in (0, 5) for sc in (1.0, 100.0)]


def ln_cases():
    out = [dict(R=R, D=D, bf16=bf, acc=acc, mis=None) for D in (256, 512, 768, 1024, 1, 65, 200) for R in (1, 5, 37) for bf in (0, 1)
           for acc in (0, 1)]
    out += [dict(R=5, D=768, bf16=bf, acc=bf, mis=mis) for mis in ("x", "y", "gamma", "dx") for bf in (0, 1)]
    return out


def focal_cases():
    out = []
    for C in (1, 9, 21, 64):
        for R in (1, 61):
            for gi, ga in enumerate((0.0, 0.5, 2.0)):
                for si, spread in enumerate((1.0, 100.0)):
                    # rotated per (C, R) block: every (gamma, spread) meets every (bg_weight, bg_class)
                    bw, bg = ((1.0, C - 1), (0.2, C - 1), (0.2, 0))[(gi + 2 * si + len(out) // 6) % 3]
                    out.append(dict(R=R, C=C, gamma=ga, spread=spread, bgw=bw, bg=bg, gscale=0.37))
    return out


def rpn_cases():
    return [dict(npos=a, nneg=b) for a, b in ((0, 0), (1, 0), (0, 1), (100, 155), (100, 156), (101, 156), (300, 700), (0, 256), (257, 0))]


def box_cases():
    return [dict(nfg=nfg, form=form) for nfg in (0, 1, 300) for form in ("specific", "specific_padded", "agnostic")]


def sgd_cases():
    return [dict(count=1, wd=0.0, big=False), dict(count=4, wd=1e-4, big=True), dict(count=97, wd=1e-4, big=False),
            dict(count=193, wd=0.0, big=False), dict(count=193, wd=1e-4, big=False)]


def tag(case):
    return " ".join(f"{k}={v}" for k, v in case.items())


# ================================================================================================== drivers
# ``impl`` supplies the kernels (the C-ABI on the GPU, the f32 emulation or one of its mutants on the CPU) with CPU tensors in and out;
# a driver builds a case's operands, calls the implementation and records every check in a Report.
def run_l2(c, impl, rep):
    R, D, t = c["R"], c["D"], tag(c)
    x = _randn((R, D), 11 + R + D)
    if c["eps"] > 0 and R > 2:
        x[2] *= 1e-15                                            # a row of norm below eps
    y, inv = impl.l2_fwd(x, c["eps"])
    ref = l2_fwd(x, c["eps"])
    rep.bound("l2norm_fwd y", t, y, ref["y"])
    rep.bound("l2norm_fwd inv", t, inv, ref["inv"])
    dy = _randn((R, D), 12 + R + D)
    dx = impl.l2_bwd(dy, y, inv)
    rep.bound("l2norm_bwd dx", t, dx, l2_bwd(dy, y, inv)["dx"])


def run_cos(c, impl, rep):
    R, D, Kc, T, t = c["R"], c["D"], c["Kc"], c["T"], tag(c)
    x = _randn((R, D), 21 + R + D + Kc)
    wn = torch.nn.functional.normalize(_randn((Kc, D), 22 + D + Kc), dim=1)
    sc, inv = impl.cos_fwd(x, wn, T, 1e-12)
    ref = cos_fwd(x, wn, T, 1e-12)
    rep.bound("cosine_logits_fwd scores", t, sc[:, :Kc], ref["scores"])
    rep.exact("cosine_logits_fwd background column", t, pos_zero(sc[:, Kc]), "not +0.0")
    rep.bound("cosine_logits_fwd inv", t, inv, ref["inv"])
    ds = _randn((R, Kc + 1), 23 + R + Kc)                        # the background column's gradient is non-zero and must be ignored
    dx0 = _randn((R, D), 24 + R + D) if c["acc"] else None
    dx = impl.cos_bwd(ds, x, wn, inv, T, dx0)
    rep.bound("cosine_logits_bwd dx" + (" (accumulate)" if c["acc"] else ""), t, dx, cos_bwd(ds, x, wn, inv, T, dx0)["dx"])


def run_con(c, impl, rep):
    n, ld, t = c["n"], c["n"] + c["pad"], tag(c)
    S = torch.full((n, ld), float("nan"))
    S[:, :n] = (torch.rand((n, n), generator=_g(31 + n)) * 2 - 1) * c["scale"]
    rl, cl, loss = impl.con_fwd(S, n)
    ref = con_fwd(S, n)
    rep.bound("contrastive_fwd rlse", t, rl, ref["rlse"])
    rep.bound("contrastive_fwd clse", t, cl, ref["clse"])
    rep.bound("contrastive_fwd loss", t, loss, con_loss(S, rl, cl, n)["loss"])
    gl = torch.tensor([c["gloss"]])
    dS = impl.con_bwd(S, rl, cl, gl, n)
    rep.bound("contrastive_bwd dS", t, dS, con_bwd(S, rl, cl, gl, n)["dS"])


def ln_inputs(c):
    R, D = c["R"], c["D"]
    x = _randn((R, D), 41 + R + D)
    if R >= 5:
        x[1] = 0.37                                              # variance 0: rstd = eps^-1/2
        x[2] = 1e3 + _randn((D,), 42 + D)                        # mean 1e3, spread 1
    ga, be = 1.0 + 0.1 * _randn((D,), 43 + D), 0.1 * _randn((D,), 44 + D)
    dy = _randn((R, D), 45 + R + D)
    dx0 = _randn((R, D), 46 + R + D) if c["acc"] else None
    return x, ga, be, (dy.bfloat16() if c["bf16"] else dy), dx0


def run_ln(c, impl, rep):
    t = tag(c)
    x, ga, be, dy, dx0 = ln_inputs(c)
    dt = torch.bfloat16 if c["bf16"] else torch.float32
    y, mean, rstd = impl.ln_fwd(x, ga, be, 1e-5, dt, c["mis"])
    ref = ln_fwd(x, ga, be, 1e-5, dt)
    sfx = " bf16" if c["bf16"] else " f32"
    rep.bound("layernorm_fwd y" + sfx, t, y, ref["y"], (ref["y"][0], ref["y_pre"]) if c["bf16"] else None)
    rep.bound("layernorm_fwd mean", t, mean, ref["mean"])
    rep.bound("layernorm_fwd rstd", t, rstd, ref["rstd"])
    dx = impl.ln_bwd(dy, x, ga, mean, rstd, dx0, c["mis"])
    rep.bound("layernorm_bwd dx" + (" (accumulate)" if c["acc"] else ""), t, dx, ln_bwd(dy, x, ga, mean, rstd, dx0)["dx"])


def focal_inputs(c):
    R, C = c["R"], c["C"]
    z = _randn((R, C), 51 + R + C, c["spread"])
    t = torch.randint(0, C, (R,), generator=_g(52 + R + C))
    if R > 16:
        t[12:16] = c["bg"]
        z[0:4] = -z[0:4].abs() - 1.0                             # every logit negative
        ar = torch.arange(R)
        z[ar[4:8], t[4:8]] = z[4:8].amax(-1) + 25.0              # the target wins by more than 20: 1 - pt == 0 in f32
        if C > 1:
            z[ar[8:12], t[8:12]] = z[8:12].amax(-1) - 95.0       # the target loses by more than 90: pt subnormal or flushed
    return z, t


def run_focal(c, impl, rep):
    tg = tag(c)
    z, t = focal_inputs(c)
    row, probs = impl.focal_fwd(z, t, c["gamma"], c["bg"], c["bgw"])
    ref = focal_fwd(z, t, c["gamma"], c["bg"], c["bgw"])
    rep.bound("focal_ce_fwd row_loss", tg, row, ref["row_loss"])
    rep.bound("focal_ce_fwd probs", tg, probs, ref["probs"])
    gs = torch.tensor([c["gscale"]])
    dl = impl.focal_bwd(z, t, probs, gs, c["gamma"], c["bg"], c["bgw"])
    rep.bound("focal_ce_bwd dlogits", tg, dl, focal_bwd(t, probs, gs, c["gamma"], c["bg"], c["bgw"])["dlogits"])


RPN_N, RPN_A = 3, 400
RPN_W = (2.0, 1.5, 0.5, 3.0)
N_EQ = 3                                                         # positives / foreground rows made exactly equal to their target


def _boxes(n, seed, size=200.0):
    b = torch.rand((n, 4), generator=_g(seed)) * size
    b[:, 2:] += b[:, :2] + 8
    return b


def rpn_inputs(c):
    N, A, npos, nneg = RPN_N, RPN_A, c["npos"], c["nneg"]
    g = _g(61 + npos + nneg)
    anchors = _boxes(A, 62)
    gt = _boxes(5, 63)
    gt_off = torch.tensor([0, 3, 3])                             # image 1 has no ground truth
    midx = torch.zeros(N, A, dtype=torch.int64)
    midx[0] = torch.randint(0, 3, (A,), generator=g)
    midx[2] = torch.randint(0, 2, (A,), generator=g)
    forced = torch.tensor([7, 2 * A + 11])                       # one positive in each image that has boxes
    cand = torch.cat([torch.arange(A), 2 * A + torch.arange(A)])
    cand = cand[~torch.isin(cand, forced)][torch.randperm(2 * A - 2, generator=g)]
    pos = torch.cat([forced, cand])[:npos]
    rest = torch.arange(N * A)
    rest = rest[~torch.isin(rest, pos)]
    neg = rest[torch.randperm(rest.numel(), generator=g)[:nneg]]
    logits = _randn((N * A,), 64, 3.0)
    deltas = _randn((N * A, 4), 65)
    eq = pos[pos < A][:N_EQ]                                     # anchor == matched box, delta 0: loss term and gradient exactly 0
    for r in eq.tolist():
        anchors[r] = gt[midx.view(-1)[r]]
        deltas[r] = 0.0
    return dict(logits=logits, deltas=deltas, pos=pos, neg=neg, midx=midx.view(-1), gt=gt, gt_off=gt_off, anchors=anchors, A=A, w=RPN_W,
                inv_norm=1.0 / (256.0 * N)), eq


def _grad_checks(rep, name, t, dd, ref):
    ok = ref["decided"]
    rep.exact(name, t, bool((dd[ok] == ref["ddeltas"][ok]).all()), "not sgn(delta - target) * f32(gout * inv_norm) bit for bit")
    rep.exact(name, t, bool(((dd[~ok] == 0) | (dd[~ok].abs() == ref["ddeltas"][~ok].abs())).all()), "an undecided element is neither +-g nor 0")


def run_rpn(c, impl, rep):
    t = tag(c)
    a, eq = rpn_inputs(c)
    out2 = impl.rpn(**a)
    rep.bound("rpn_losses out2", t, out2, rpn_ref(**a)["out2"])
    gout = torch.tensor([1.5, 0.7])
    dl, dd = impl.rpn(**a, gout=gout)
    ref = rpn_ref(**a, gout=gout)
    rep.bound("rpn_losses dlogits", t, dl, ref["dlogits"])
    samp = torch.zeros(a["logits"].numel(), dtype=torch.bool)
    samp[a["pos"]] = True
    samp[a["neg"]] = True
    rep.exact("rpn_losses dlogits", t, pos_zero(dl[~samp]), "an unsampled entry is not exactly 0")
    _grad_checks(rep, "rpn_losses ddeltas", t, dd, ref)
    isp = torch.zeros_like(samp)
    isp[a["pos"]] = True
    rep.exact("rpn_losses ddeltas", t, pos_zero(dd[~isp]), "an entry outside the positives is not exactly 0")
    rep.exact("rpn_losses ddeltas", t, bool((dd[eq] == 0).all()), "gradient at delta == target is not 0")


BOX_R, BOX_KC = 320, 5
BOX_W = (10.0, 10.0, 5.0, 5.0)


def box_inputs(c):
    R, Kc, nfg = BOX_R, BOX_KC, c["nfg"]
    ld = {"specific": 4 * Kc, "specific_padded": 4 * Kc + 4, "agnostic": 4}[c["form"]]
    g = _g(71 + nfg)
    deltas = _randn((R, ld), 72 + ld)
    cls = None if c["form"] == "agnostic" else torch.randint(0, Kc, (R,), generator=g)
    fg = torch.randperm(R, generator=g)[:nfg].sort().values
    src, tgt = _boxes(R, 73, 100.0), _boxes(R, 74, 100.0)
    eq = fg[:N_EQ if nfg > N_EQ else 0]
    for r in eq.tolist():
        tgt[r] = src[r]
        c0 = 0 if cls is None else 4 * int(cls[r])
        deltas[r, c0:c0 + 4] = 0.0
    return dict(deltas=deltas, fg=fg, cls=cls, src=src, tgt=tgt, w=BOX_W, inv_norm=1.0 / R), eq


def run_box(c, impl, rep):
    t = tag(c)
    a, eq = box_inputs(c)
    out1 = impl.box(**a)
    rep.bound("box_l1 out1", t, out1, box_ref(**a)["out1"])
    gout = torch.tensor([0.7])
    dd = impl.box(**a, gout=gout)
    ref = box_ref(**a, gout=gout)
    _grad_checks(rep, "box_l1 ddeltas", t, dd, ref)
    touched = torch.zeros(a["deltas"].shape, dtype=torch.bool)
    c0 = 4 * a["cls"][a["fg"]] if a["cls"] is not None else torch.zeros_like(a["fg"])
    touched[a["fg"][:, None], c0[:, None] + torch.arange(4)[None, :]] = True
    rep.exact("box_l1 ddeltas", t, pos_zero(dd[~touched]), "an entry outside the foreground rows' class columns is not exactly 0")
    if eq.numel():
        rep.exact("box_l1 ddeltas", t, bool((dd[eq] == 0).all()), "gradient at delta == target is not 0")


SGD_SIZES = (1, 3, 4, 5, 35, 1000)
SGD_BIG = 2 ** 20 + 3
SGD_CLIP = 1e-2


def sgd_layout(c):
    """per tensor: (size, start in the p, g, m flat buffers).  Tensor i's alignment pattern is i % 4: all three 16-byte aligned, only
    g misaligned, only p, only m (by 1..3 elements); >= 4 guard elements between tensors"""
    g = _g(81 + c["count"])
    sizes = [SGD_SIZES[int(k)] for k in torch.randint(0, len(SGD_SIZES), (c["count"],), generator=g)]
    if c["big"]:                                                 # one per alignment pattern, n % 4 = 3, 2, 1, 0: every loop wraps
        sizes[:4] = [SGD_BIG - k for k in range(4)]
    lay, cur = [], 4
    for i, n in enumerate(sizes):
        off = 1 + (i // 4) % 3
        o = [off if i % 4 == k else 0 for k in (2, 1, 3)]         # p, g, m
        lay.append((n, cur + o[0], cur + o[1], cur + o[2]))
        cur = (cur + n + 3 + 4 + 3) // 4 * 4
    return lay, cur + 4


def sgd_buffers(c, lay, total):
    """p, g flat buffers with NaN between the tensors; gradient norms far above the clip, around it (twice), below it, and zero"""
    p = torch.full((total,), float("nan"))
    g = torch.full((total,), float("nan"))
    for i, (n, op, og, om) in enumerate(lay):
        p[op:op + n] = _randn((n,), 82 + i)
        gi = _randn((n,), 83 + i)
        target = (3.0, 2 * SGD_CLIP, 0.3 * SGD_CLIP, 0.0, 7 * SGD_CLIP)[i % 5]     # (5 does not divide SGD_MAX)
        if i == 0 and target == 0.0:
            target = 3.0
        g[og:og + n] = gi / gi.norm().clamp_min(1e-30) * target if n > 1 or target == 0 else gi.sign() * target
    return p, g


def sgd_views(buf, lay, which):
    return [buf[l[which]:l[which] + l[0]] for l in lay]


def run_sgd(c, impl, rep):
    t = tag(c)
    lay, total = sgd_layout(c)
    p, g = sgd_buffers(c, lay, total)
    m = torch.full((total,), float("nan"))                       # first_step = 1 must not read the momentum
    ws = torch.full((c["count"] + 4,), 12345.0)                  # garbage: the step zeroes what it uses
    lr, mo = 0.02, 0.9
    for step, first in ((1, 1), (2, 0)):
        p2, m2, ws2 = impl.sgd(lay, p, g, m, ws, lr, mo, c["wd"], SGD_CLIP, first)
        ref = sgd_ref(sgd_views(p, lay, 1), sgd_views(g, lay, 2), sgd_views(m, lay, 3), lr, mo, c["wd"], SGD_CLIP, first)
        inside_p, inside_m = torch.zeros(total, dtype=torch.bool), torch.zeros(total, dtype=torch.bool)
        for i, (n, op, og, om) in enumerate(lay):
            inside_p[op:op + n] = True
            inside_m[om:om + n] = True
        rep.exact("sgd_clip_step p", t, bits_equal(p2[~inside_p], p[~inside_p]), f"step {step}: an element between the tensors was written")
        rep.exact("sgd_clip_step m", t, bits_equal(m2[~inside_m], m[~inside_m]), f"step {step}: an element between the tensors was written")
        rep.exact("sgd_clip_step norm_ws", t, bits_equal(ws2[c["count"]:], ws[c["count"]:]), f"step {step}: norm_ws written past count")
        cat = lambda k: (torch.cat([r[k][0] for r in ref]), torch.cat([r[k][1] for r in ref]))
        rep.bound("sgd_clip_step norm_ws", f"{t} step {step}", ws2[:c["count"]], cat("norm"))
        rep.bound("sgd_clip_step p", f"{t} step {step}", torch.cat(sgd_views(p2, lay, 1)), cat("p"))
        rep.bound("sgd_clip_step m", f"{t} step {step}", torch.cat(sgd_views(m2, lay, 3)), cat("m"))
        p, m, ws = p2, m2, ws2


FAMILIES = (("l2", l2_cases, run_l2), ("cos", cos_cases, run_cos), ("con", con_cases, run_con), ("ln", ln_cases, run_ln),
            ("focal", focal_cases, run_focal), ("rpn", rpn_cases, run_rpn), ("box", box_cases, run_box), ("sgd", sgd_cases, run_sgd))
