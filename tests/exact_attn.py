"""Exact references and per-element error bounds for the attention kernels (imported by the attention tests; not a conftest).

Every reference takes the operands a kernel was given, as stored (bf16 or f32), and computes in float64.  Every bound follows the
kernel's own rounding points (cddmsl_amd/csrc/attn_small.hip, elementwise.hip, conv_wgrad.hip k_gemm_tn_small MODE 3).  Units:
u = 2^-24 (f32), u_b = 2^-8 (the unit roundoff of a round-to-nearest-even bf16 store), C_ACC the f32 accumulation constant of
tests/exact_gemm.py (a sum of products is off by at most C_ACC u sum|a b|).

cddmsl_attn_small (ClipCap mapper, bf16 in and out):
  S = scale Q K^T          products exact, f32 sum, f32 multiply:   eps_S[i,j] = (C_ACC + 1) u scale sum_c |q_ic k_jc|
  p = softmax_j(S)         f32, __expf at x = S - m (relative error c_exp(x) = (C_EXP0 + C_EXP1 |x|) u: the argument's
                           rounding grows with |x|), normalised by a sum of NORM_DEPTH_SMALL levels and one reciprocal: a
                           weight's relative error is  r_ij = 2 max_j eps_S + c_exp(x_ij) + (depth + 2) u  (a score shift of
                           eps moves a softmax weight by a factor within exp(+-2 eps))
  P~ = bf16(p)             put_tile: relative u_b more per weight
  O = P~ V                 f32 sum (C_ACC u sum_j P~ |v|), stored bf16:
      |got - o| <= u_b |o| + (1 + u_b) [ sum_j (u_b + (1 + u_b) r_ij) p_ij |v_jc| + C_ACC u sum_j p_ij |v_jc| + TINY sum_j |v_jc| ]
  backward (recomputes p as the forward does):
      dV = bf16(P~^T dO)                                  as O, with dO for V
      dP = dO V^T (f32), rs = sum_j dP p (f32 p, not P~)  |dP - dp| <= C_ACC u sum_c |do v| ;  rs: the same per term + (depth + 1) u
      dS = bf16(p (dP - rs) scale)                         cancels where dp ~ rs: the f32 errors of dP and rs enter as an ABSOLUTE
                                                           term  scale p (|dP - dp| + |rs~ - rs|), next to u_b |ds|
      dQ = bf16(dS~ K), dK = bf16(dS~^T Q)                sum_j |dS~ - ds| |k| + C_ACC u sum_j |dS~| |k|, stored bf16
cddmsl_attn_last (one query row; f32 FMA chains on bf16 operands, p kept in f32): the same with no bf16 P; the backward works
  from the p it is given (the forward's), so its reference does too, and the dV half of dkv is bit-exact: bf16(f32(p_j dO_c)).
Attention-pool glue (elementwise.hip):
  tokens_fwd   rows 1..P bit-exact bf16(f32(x + pos)); row 0 = mean_p x + pos[0]: a (P - 1)-term f32 sum, a division, an add,
               (P + 2) u (sum_p |x| / P + |pos0|) before the store; mbits bit-exact; pad rows P+1..TP-1 exactly zero
  softmax_fwd  p (f32) from the given f32 S: relative delta_t + sum_k p_k delta_k + (depth + 3) u, delta_t = c_exp(x_t) + u |s_t|
               (the product s * scale is rounded too); pT = bf16(p) bit for bit, zero rows past P1
  softmax_bwd  ds = bf16(p (dP - sum p dP) scale) from the given p, dP: u_b |ds| + scale p (3 u |dP - dot| + (depth + 1) u
               sum p |dP|); the p half of pds = bf16(p), dsT = the ds half transposed, zero past P1 -- all bit for bit
  attnpool_dx  dtok[t] = sum_h pds[h,t] zu[h,:] (products exact, f32), dx[t-1] = bf16(dtok[t] + (dtok[0] + g0) / P):
               u_b |dx| + (1 + u_b) [C_ACC u (A_t + (A_0 + |g0|) / P) + 4 u (|dtok_t| + |dtok_0 + g0| / P)],  A_t = sum_h |pds zu|;
               masked elements exactly 0; gpos += sum_k dtok[k] (f32: a run of bpb regions per block, then one atomic per block):
               C_ACC u sum_k A_k + (bpb + blocks + 2) u (|gpos0| + sum_k |dtok_k|)
TINY covers values below the normal range -- weights whose exp underflows, f32 intermediates and bf16 stores that land among the
subnormals or are flushed to zero: their absolute error is below 2^-126.

A bound does not see a store that rounds the wrong way inside it (a truncating store stays within u_b; for dQ / dK of attn_small the
bound carries u_b sum_j |ds_j| |k_j| >= u_b |dq| from dS~ as well, so even a whole ulp fits); store_bias measures the signed store
error in ulps against the exact value of what the store rounds, computed from the kernel's bf16 intermediates (P~, dS~) rounded
correctly, as exact_gemm.rounding_bias does for the GEMMs -- so a truncated intermediate shows up as well as a truncated output.
Every bf16 output of the kernels above is checked by one or the other: bit for bit, or bound + store_bias.
"""
import math

import torch

import exact_gemm as X
from exact_gemm import C_ACC, U_BF16, U_F32

_f64 = X._f64

C_EXP0, C_EXP1 = 4.0, 3.0          # __expf / expf: (C_EXP0 + C_EXP1 |x|) u relative (exp2 of a rounded x log2e, 1-ulp v_exp_f32)
TINY = 2.0 ** -126
NORM_DEPTH_SMALL = 8               # attn_small: 3 columns per lane + 5 reduction steps over 32 lanes
NORM_DEPTH_WAVE = 8                # 64-lane wave sums (attn_last, the wave form of the pool softmax): 2 per lane + 6 steps
SMALL_T = 96                       # attn_small's padded tile (t <= 96, dh == 96)


def c_exp(x):
    return (C_EXP0 + C_EXP1 * _f64(x).abs()) * U_F32


def softmax_depth(H, TP, P1):
    """summation depth of cddmsl_attnpool_softmax_fwd/bwd: the wave form for H <= 32, TP <= 64, else one thread per row (P1 terms)"""
    return NORM_DEPTH_WAVE if (H <= 32 and TP <= 64) else P1 + 1


def heads_first(x, n, t, heads, dh, col0=0):
    """[n*t, ld] rows (head h at columns col0 + h*dh) -> [n*heads, t, dh] float64"""
    return _f64(x[:, col0:col0 + heads * dh]).reshape(n, t, heads, dh).permute(0, 2, 1, 3).reshape(n * heads, t, dh)


def rows_first(y, n, t, heads, dh):
    """inverse of heads_first: [n*heads, t, dh] -> [n*t, heads*dh]"""
    return y.reshape(n, heads, t, dh).permute(0, 2, 1, 3).reshape(n * t, heads * dh)


def store_bound(exact, pre, u=U_BF16):
    """bound of a value whose pre-store error is bounded by ``pre``, stored with unit roundoff u: u |exact| + (1 + u) pre, and
    TINY for a result below the normal range (bf16 subnormals are 2^-133 apart; a flushed one is off by less than 2^-126)"""
    return u * _f64(exact).abs() + (1 + u) * pre + TINY


def _softmax(s):
    m = s.amax(-1, keepdim=True)
    e = torch.exp(s - m)
    return e / e.sum(-1, keepdim=True), s - m


def _p_rel(x, eps, depth):
    """relative error bound of a kernel's f32 softmax weight: scores off by <= eps (absolute, per row max), exp at x, normalisation"""
    return 2.0 * eps * (1.0 + 2.0 * eps) + c_exp(x) + (depth + 2) * U_F32


# ---------------------------------------------------------------------------------------------------------------- forward
def attn_fwd(q, k, v, scale, depth=NORM_DEPTH_SMALL, p_bf16=True):
    """q [B, tq, dh], k / v [B, t, dh] (any dtype; exact as float64), scale the f32 value the kernel got.  Returns a dict:
    o (exact), bound (per element), p (exact weights), pre (the error bound before the output store: what store_bias filters on),
    o_rw (o with the weights rounded once to bf16 -- what a correct kernel's f32 sum approximates, for store_bias; p_bf16 only),
    p_bound (per weight, attn_last's f32 p)."""
    q, k, v = _f64(q), _f64(k), _f64(v)
    sc = float(torch.tensor(scale, dtype=torch.float32))
    s = sc * (q @ k.transpose(1, 2))
    eps = (C_ACC + 1) * U_F32 * sc * (q.abs() @ k.abs().transpose(1, 2))
    p, x = _softmax(s)
    r = _p_rel(x, eps.amax(-1, keepdim=True), depth)
    va = v.abs()
    ub = U_BF16 if p_bf16 else 0.0
    pre = ((ub + (1 + ub) * r) * p) @ va + C_ACC * U_F32 * (1 + ub) * 1.01 * (p @ va) + TINY * va.sum(1, keepdim=True)
    o = p @ v
    out = dict(o=o, p=p, pre=pre, bound=store_bound(o, pre), p_bound=r * p * 1.01 + TINY)
    if p_bf16:
        out["o_rw"] = X.round_bf16(p) @ v
        out["pre_rw"] = C_ACC * U_F32 * (X.round_bf16(p) @ va)
    return out


# ---------------------------------------------------------------------------------------------------------------- backward
def attn_small_bwd(q, k, v, do, scale, depth=NORM_DEPTH_SMALL):
    """cddmsl_attn_small_bwd: q, k, v, do [B, t, dh] -> dict of (exact, bound) pairs dq, dk, dv, and ds (the bf16 intermediate)"""
    q, k, v, do = _f64(q), _f64(k), _f64(v), _f64(do)
    sc = float(torch.tensor(scale, dtype=torch.float32))
    s = sc * (q @ k.transpose(1, 2))
    eps = (C_ACC + 1) * U_F32 * sc * (q.abs() @ k.abs().transpose(1, 2))
    p, x = _softmax(s)
    r = _p_rel(x, eps.amax(-1, keepdim=True), depth)
    dp = do @ v.transpose(1, 2)
    bdp = C_ACC * U_F32 * (do.abs() @ v.abs().transpose(1, 2))
    rs = (p * dp).sum(-1, keepdim=True)
    ds = p * (dp - rs) * sc
    e_rs = 1.01 * (p * (r * dp.abs() + (1 + r) * bdp + (depth + 1) * U_F32 * dp.abs())).sum(-1, keepdim=True)
    e_d = bdp + e_rs
    e_ds = sc * (p * ((r + 3 * U_F32) * (dp - rs).abs() + (1 + r) * (1 + 3 * U_F32) * e_d) + TINY * (dp.abs() + rs.abs()))
    b_ds = store_bound(ds, e_ds)
    dsa = ds.abs() + b_ds
    dq = ds @ k
    dk = ds.transpose(1, 2) @ q
    pre_dq = b_ds @ k.abs() + C_ACC * U_F32 * (dsa @ k.abs())
    pre_dk = b_ds.transpose(1, 2) @ q.abs() + C_ACC * U_F32 * (dsa.transpose(1, 2) @ q.abs())
    dv = p.transpose(1, 2) @ do
    pre_dv = (((U_BF16 + (1 + U_BF16) * r) * p).transpose(1, 2) @ do.abs() + C_ACC * U_F32 * (1 + U_BF16) * 1.01 * (p.transpose(1, 2) @ do.abs())
              + TINY * do.abs().sum(1, keepdim=True))
    pr = X.round_bf16(p)
    out = {}
    for name, e, pre in (("dq", dq, pre_dq), ("dk", dk, pre_dk), ("dv", dv, pre_dv)):
        out[name] = (e, store_bound(e, pre))
    out["ds"] = (ds, b_ds)
    # for store_bias: each output with the kernel's bf16 intermediate (P~ for dV, dS~ for dQ / dK) rounded once, and the f32 sum's
    # bound -- a truncating dS~ store shifts dQ and dK toward zero just as a truncating store of dQ / dK itself does
    dsr = X.round_bf16(ds)
    out["dv_rw"] = (pr.transpose(1, 2) @ do, C_ACC * U_F32 * (pr.transpose(1, 2) @ do.abs()))
    out["dq_rw"] = (dsr @ k, C_ACC * U_F32 * (dsr.abs() @ k.abs()))
    out["dk_rw"] = (dsr.transpose(1, 2) @ q, C_ACC * U_F32 * (dsr.abs().transpose(1, 2) @ q.abs()))
    return out


def attn_last_bwd(q, k, v, do, p, scale, depth=NORM_DEPTH_WAVE):
    """cddmsl_attn_last_bwd from the p it is given: q / do [B, dh], k / v [B, t, dh], p [B, t] f32 -> dict of (exact, bound):
    dq [B, dh], dk [B, t, dh]; dq_pre / dk_pre, their bounds before the bf16 store (for store_bias); and dv [B, t, dh] =
    bf16(f32(p * dO)), the bit-exact expectation"""
    q, k, v, do, pp = _f64(q), _f64(k), _f64(v), _f64(do), _f64(p)
    sc = float(torch.tensor(scale, dtype=torch.float32))
    dp = (v @ do.unsqueeze(-1)).squeeze(-1)
    bdp = C_ACC * U_F32 * (v.abs() @ do.abs().unsqueeze(-1)).squeeze(-1)
    rs = (pp * dp).sum(-1, keepdim=True)
    ds = pp * (dp - rs) * sc
    e_rs = 1.01 * (pp * (bdp + (depth + 1) * U_F32 * dp.abs())).sum(-1, keepdim=True)
    e_ds = sc * pp * (3 * U_F32 * (dp - rs).abs() + (1 + 3 * U_F32) * (bdp + e_rs)) + TINY
    dsa = ds.abs() + e_ds
    dq = (ds.unsqueeze(1) @ k).squeeze(1)
    pre_dq = (e_ds.unsqueeze(1) @ k.abs()).squeeze(1) + C_ACC * U_F32 * (dsa.unsqueeze(1) @ k.abs()).squeeze(1)
    dk = ds.unsqueeze(-1) * q.unsqueeze(1)
    pre_dk = (e_ds.unsqueeze(-1) + U_F32 * dsa.unsqueeze(-1)) * q.abs().unsqueeze(1)
    dv = _f64((p.float().unsqueeze(-1) * do.float().unsqueeze(1)).bfloat16())
    return dict(dq=(dq, store_bound(dq, pre_dq)), dk=(dk, store_bound(dk, pre_dk)), dv=dv,
                dq_pre=pre_dq, dk_pre=pre_dk)


# ---------------------------------------------------------------------------------------------------------------- pool glue
def tokens_fwd(x, pos, TP):
    """cddmsl_attn_tokens_fwd(_mask): x [K, P, C], pos [P+1, C] f32 -> dict: rows (bf16 rows 1..P, bit-exact), row0 (exact mean +
    pos[0]), row0_bound, mbits [K, C] int64 (bit-exact), TP"""
    K, P, C = x.shape
    xf = x.float()
    rows = (xf + pos[1:].unsqueeze(0)).to(x.dtype)
    xd = _f64(x)
    row0 = xd.mean(1) + _f64(pos[0])
    pre = (P + 2) * U_F32 * (xd.abs().sum(1) / P + _f64(pos[0]).abs())
    u = U_BF16 if x.dtype == torch.bfloat16 else U_F32
    bits = ((x > 0).long() << torch.arange(P, device=x.device).view(1, P, 1)).sum(1)
    return dict(rows=rows, row0=row0, row0_bound=store_bound(row0, pre, u), row0_pre=pre, mbits=bits)


def softmax_fwd(S, P1, scale, depth):
    """cddmsl_attnpool_softmax_fwd: S [R, TP] f32 -> (p exact [R, P1], bound)"""
    sc = float(torch.tensor(scale, dtype=torch.float32))
    s = _f64(S[:, :P1]) * sc
    p, x = _softmax(s)
    d = c_exp(x) + U_F32 * s.abs()
    b = 1.01 * p * (d + (p * d).sum(-1, keepdim=True) + (depth + 3) * U_F32) + TINY
    return p, b


def softmax_bwd(p, dP, scale, depth):
    """cddmsl_attnpool_softmax_bwd from the given p [R, P1], dP [R, TP] (f32) -> (ds exact [R, P1], bound of its bf16 store,
    pre: the bound before the store)"""
    P1 = p.shape[1]
    sc = float(torch.tensor(scale, dtype=torch.float32))
    pp, dp = _f64(p), _f64(dP[:, :P1])
    dot = (pp * dp).sum(-1, keepdim=True)
    ds = pp * (dp - dot) * sc
    e_dot = (depth + 1) * U_F32 * (pp * dp.abs()).sum(-1, keepdim=True)
    pre = 1.01 * sc * pp * (3 * U_F32 * (dp - dot).abs() + e_dot) + TINY
    return ds, store_bound(ds, pre), pre


def attnpool_dtok(pds, zu, P):
    """[K, TP, C] exact token gradients dtok = pds^T zu and A = |pds|^T |zu| (float64), rows 0..P"""
    a, b = _f64(pds[:, :, :P + 1]), _f64(zu)
    return a.transpose(1, 2) @ b, a.abs().transpose(1, 2) @ b.abs()


def attnpool_dx(pds, zu, g0, mbits, P):
    """cddmsl_attnpool_dx for the regions given: -> (dx exact [K, P, C] (masked), bound, keep mask [K, P, C] bool, pre)"""
    dt, A = attnpool_dtok(pds, zu, P)
    g = _f64(g0)
    t0 = dt[:, 0] + g
    dx = dt[:, 1:] + (t0 / P).unsqueeze(1)
    pre = C_ACC * U_F32 * (A[:, 1:] + ((A[:, 0] + g.abs()) / P).unsqueeze(1)) + 4 * U_F32 * (dt[:, 1:].abs() + (t0.abs() / P).unsqueeze(1))
    keep = ((mbits.unsqueeze(1) >> torch.arange(P, device=mbits.device).view(1, P, 1)) & 1).bool()
    dx = torch.where(keep, dx, torch.zeros_like(dx))
    return dx, store_bound(dx, pre), keep, pre


def attnpool_gpos(pds, zu, g0, gpos0, P, run, blocks, chunk=256):
    """gpos0 + sum_k dtok[k][0..P] (+ g0 in row 0), all K regions, float64, and its bound (f32 sums over a run of ``run`` regions
    per block, then ``blocks`` atomics per element)"""
    K = pds.shape[0]
    tot = _f64(gpos0).clone()
    absum = _f64(gpos0).abs()
    acc = torch.zeros_like(tot)
    for c0 in range(0, K, chunk):
        dt, A = attnpool_dtok(pds[c0:c0 + chunk], zu[c0:c0 + chunk], P)
        dt[:, 0] += _f64(g0[c0:c0 + chunk])
        tot += dt.sum(0)
        absum += dt.abs().sum(0)
        acc += A.sum(0)
        acc[0] += _f64(g0[c0:c0 + chunk]).abs().sum(0)
    return tot, U_F32 * tot.abs() + C_ACC * U_F32 * acc + (run + blocks + 2) * U_F32 * absum


# ---------------------------------------------------------------------------------------------------------------- judging
def check(got, exact, bound):
    """-> (ok, worst |err| / bound, flat index of the worst element); NaN in got fails"""
    err = (_f64(got) - _f64(exact)).abs()
    ratio = err / _f64(bound).clamp_min(1e-300)
    ratio = torch.where(err == 0, torch.zeros_like(ratio), ratio)
    ratio = torch.where(torch.isnan(err), torch.full_like(ratio, math.inf), ratio)
    worst = int(ratio.reshape(-1).argmax()) if ratio.numel() else 0
    w = float(ratio.reshape(-1)[worst]) if ratio.numel() else 0.0
    return bool(w <= 1.0), w, worst


def store_bias(got, exact_rounded_in, pre):
    """signed error of a bf16 store in ulps of the output, measured toward zero, over the elements whose pre-store error bound
    ``pre`` is below 1/16 ulp (exact_gemm.rounding_bias): RNE ~0, truncation ~-0.5.  ``exact_rounded_in`` is the exact value of
    what the store rounds -- with the kernel's own bf16 intermediates (P~) rounded correctly -- so that a truncated intermediate
    shows up here too.  -> (bias, elements)"""
    return X.rounding_bias(got, exact_rounded_in, _f64(pre) / (C_ACC * U_F32))


def old_criterion(got, ref, tol=2e-2):
    return X.old_criterion(got, ref, tol)
