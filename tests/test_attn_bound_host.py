"""The attention checker itself (tests/exact_attn.py), on the CPU: the float64 references against torch's float64 attention, softmax
and autograd; every bound against an f32 emulation of its kernel that rounds at the same points but sums in another order; and
mutants every bound must reject -- with the verdict of the old  max|got - ref| / max|ref| < 2e-2  criterion printed next to each."""
import torch

import exact_attn as A
import exact_gemm as X

MAPPER_SCALE = 96 ** -0.5


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _bf(shape, seed, s=1.0):
    return (torch.randn(*shape, generator=_g(seed)) * s).bfloat16()


def _qkv(B=24, t=80, dh=96, seed=0, s=0.56):
    return _bf((B, t, dh), seed, s), _bf((B, t, dh), seed + 1, s), _bf((B, t, dh), seed + 2, s)


def _close(a, b):
    a, b = A._f64(a).detach(), A._f64(b).detach()
    return float((a - b).abs().max()) <= 1e-12 * max(float(b.abs().max()), 1e-300)


# -------------------------------------------------------------------------------------------------- references = torch float64
def test_references_equal_torch_float64_attention_and_autograd():
    q, k, v = (x.double().requires_grad_(True) for x in _qkv(B=6, t=33, dh=96, seed=3))
    do = torch.randn(6, 33, 96, generator=_g(9), dtype=torch.float64)
    sc = float(torch.tensor(MAPPER_SCALE, dtype=torch.float32))
    o = torch.softmax((q @ k.transpose(1, 2)) * sc, -1) @ v
    dq, dk, dv = torch.autograd.grad(o, (q, k, v), do)
    f = A.attn_fwd(q.detach(), k.detach(), v.detach(), MAPPER_SCALE)
    assert _close(f["o"], o)
    b = A.attn_small_bwd(q.detach(), k.detach(), v.detach(), do, MAPPER_SCALE)
    assert _close(b["dq"][0], dq) and _close(b["dk"][0], dk) and _close(b["dv"][0], dv)
    # the last-token backward from the (exact) p: the same gradients for one query row
    ql = q.detach()[:, -1:].clone().requires_grad_(True)
    kk, vv = k.detach().clone().requires_grad_(True), v.detach().clone().requires_grad_(True)
    pl = torch.softmax((ql @ kk.transpose(1, 2)) * sc, -1)
    ol = pl @ vv
    gl = torch.autograd.grad(ol, (ql, kk, vv), do[:, -1:])
    lb = A.attn_last_bwd(ql.detach()[:, 0], kk.detach(), vv.detach(), do[:, -1], pl.detach()[:, 0], MAPPER_SCALE)
    assert _close(lb["dq"][0], gl[0][:, 0]) and _close(lb["dk"][0], gl[1])
    # pool glue: softmax and its backward, the token gradient product with the mean token's share
    S = torch.randn(40, 56, generator=_g(4), dtype=torch.float64) * 8
    Sg = S.clone().requires_grad_(True)
    p = torch.softmax(Sg[:, :50] * 0.125, -1)
    dP = torch.randn(40, 56, generator=_g(5), dtype=torch.float64)
    (gS,) = torch.autograd.grad(p, Sg, dP[:, :50])
    assert _close(A.softmax_fwd(S, 50, 0.125, 8)[0], p)
    assert _close(A.softmax_bwd(p.detach(), dP, 0.125, 8)[0], gS[:, :50])
    K, H2, P, C = 5, 16, 49, 24
    pds = torch.randn(K, H2, 56, generator=_g(6), dtype=torch.float64)
    zu = torch.randn(K, H2, C, generator=_g(7), dtype=torch.float64)
    g0 = torch.randn(K, C, generator=_g(8), dtype=torch.float64)
    x = torch.randn(K, P, C, generator=_g(10), dtype=torch.float64, requires_grad=True)
    tok = torch.cat([x.mean(1, keepdim=True), x], 1)                      # the token build (positional embedding: a constant)
    dtok = torch.einsum("kht,khc->ktc", pds[:, :, :P + 1], zu)
    (gx,) = torch.autograd.grad((tok * dtok).sum() + (x.mean(1) * g0).sum(), x)
    all_bits = torch.full((K, C), (1 << P) - 1, dtype=torch.int64)
    assert _close(A.attnpool_dx(pds, zu, g0, all_bits, P)[0], gx)


# -------------------------------------------------------------------------------------------------- f32 emulations
def _emu_small_fwd(q, k, v, sc, truncate_p=False, truncate_o=False, extra_key=False):
    s = (q.float() @ k.float().transpose(1, 2)) * torch.tensor(sc, dtype=torch.float32)
    if extra_key:                                                         # the first padded key: score 0, V = 0
        s = torch.cat([s, torch.zeros_like(s[:, :, :1])], -1)
    p = torch.softmax(s, -1)
    if extra_key:
        p = p[:, :, :-1]
    P = X.truncate_bf16(p).float() if truncate_p else p.bfloat16().float()
    o = P @ v.float()
    return X.truncate_bf16(o) if truncate_o else o.bfloat16()


def _emu_small_bwd(q, k, v, do, sc, truncate_ds=False, truncate_dq=False):
    scf = torch.tensor(sc, dtype=torch.float32)
    p = torch.softmax((q.float() @ k.float().transpose(1, 2)) * scf, -1)
    dP = do.float() @ v.float().transpose(1, 2)
    pr = p.bfloat16().float()
    rs = (dP * p).sum(-1, keepdim=True)
    ds32 = p * (dP - rs) * scf
    ds = X.truncate_bf16(ds32).float() if truncate_ds else ds32.bfloat16().float()
    dq = ds @ k.float()
    dq = X.truncate_bf16(dq).bfloat16() if truncate_dq else dq.bfloat16()
    return dq, (ds.transpose(1, 2) @ q.float()).bfloat16(), (pr.transpose(1, 2) @ do.float()).bfloat16()


def _emu_last(q, k, v, sc, exp_err=0.0, head_shift=0):
    """q [B, dh], k / v [B, t, dh] -> (o bf16, p f32).  exp_err: relative error of exp on every other key; head_shift: V of the
    next (sequence, head) block"""
    s = (k.float() @ q.float().unsqueeze(-1)).squeeze(-1) * torch.tensor(sc, dtype=torch.float32)
    e = torch.exp(s - s.amax(-1, keepdim=True))
    if exp_err:
        e = e * (1 + exp_err * (torch.arange(e.shape[-1]) % 2))
    p = e / e.sum(-1, keepdim=True)
    vv = v.roll(-head_shift, 0) if head_shift else v
    return (p.unsqueeze(1) @ vv.float()).squeeze(1).bfloat16(), p


def _verdict(ok, ratio, bias):
    return (not ok) or (bias is not None and abs(bias) > 0.02)


def test_bounds_accept_f32_emulations_in_another_order():
    lines = []
    q, k, v = _qkv(seed=20)
    f = A.attn_fwd(q, k, v, MAPPER_SCALE)
    got = _emu_small_fwd(q, k, v, MAPPER_SCALE)
    ok, r, _ = A.check(got, f["o"], f["bound"])
    rb, n = A.store_bias(got, f["o_rw"], f["pre_rw"])
    assert ok and abs(rb) <= 0.02 and n > 50000, (r, rb, n)
    lines.append(f"attn_small fwd: worst |err|/bound {r:.3f}, store bias {rb:+.4f} over {n}")
    do = _bf(q.shape, 23, 0.5)
    b = A.attn_small_bwd(q, k, v, do, MAPPER_SCALE)
    for name, g in zip(("dq", "dk", "dv"), _emu_small_bwd(q, k, v, do, MAPPER_SCALE)):
        ok, r, _ = A.check(g, *b[name])
        rb, n = A.store_bias(g, *b[name + "_rw"])
        assert ok and abs(rb) <= 0.02 and n > 50000, (name, r, rb, n)
        lines.append(f"attn_small bwd {name}: worst |err|/bound {r:.3f}, store bias {rb:+.4f} over {n}")
    # attn_last: the one query row, p in f32; the backward from that p
    ql, kl, vl = q[:, -1], k, v
    o, p = _emu_last(ql, kl, vl, MAPPER_SCALE)
    fl = A.attn_fwd(ql.unsqueeze(1), kl, vl, MAPPER_SCALE, depth=A.NORM_DEPTH_WAVE, p_bf16=False)
    for name, g, e, bd in (("o", o, fl["o"][:, 0], fl["bound"][:, 0]), ("p", p, fl["p"][:, 0], fl["p_bound"][:, 0])):
        ok, r, _ = A.check(g, e, bd)
        assert ok, (name, r)
        lines.append(f"attn_last fwd {name}: worst |err|/bound {r:.3f}")
    dol = do[:, -1]
    lb = A.attn_last_bwd(ql, kl, vl, dol, p, MAPPER_SCALE)
    scf = torch.tensor(MAPPER_SCALE, dtype=torch.float32)
    dp = (vl.float() @ dol.float().unsqueeze(-1)).squeeze(-1)
    ds = p * (dp - (p * dp).sum(-1, keepdim=True)) * scf
    for name, g in (("dq", (ds.unsqueeze(1) @ kl.float()).squeeze(1).bfloat16()), ("dk", (ds.unsqueeze(-1) * ql.float().unsqueeze(1)).bfloat16())):
        ok, r, _ = A.check(g, *lb[name])
        rb, n = A.store_bias(g, lb[name][0], lb[name + "_pre"])
        assert ok and abs(rb) <= 0.05, (name, r, rb, n)
        lines.append(f"attn_last bwd {name}: worst |err|/bound {r:.3f}, store bias {rb:+.4f} over {n}")
    # pool glue
    S = torch.randn(3000, 56, generator=_g(30)) * 8.2
    pe, pb = A.softmax_fwd(S, 50, 0.125, 51)
    ps = torch.softmax(S[:, :50] * 0.125, -1)
    ok, r, _ = A.check(ps, pe, pb)
    assert ok, r
    lines.append(f"pool softmax fwd p: worst |err|/bound {r:.3f}")
    dP = torch.randn(3000, 56, generator=_g(31)) * 1e-3
    dse, dsb, dspre = A.softmax_bwd(ps, dP, 0.125, 51)
    dsg = (ps * (dP[:, :50] - (ps * dP[:, :50]).flip(-1).sum(-1, keepdim=True)) * 0.125).bfloat16()
    ok, r, _ = A.check(dsg, dse, dsb)
    rb, n = A.store_bias(dsg, dse, dspre)
    assert ok and abs(rb) <= 0.02, (r, rb)
    lines.append(f"pool softmax bwd ds: worst |err|/bound {r:.3f}, store bias {rb:+.4f} over {n}")
    K, H2, P, C = 40, 64, 49, 256
    pds = (torch.randn(K, H2, 56, generator=_g(32)) * 0.05).bfloat16()
    pds[:, :, P + 1:] = 0
    zu = _bf((K, H2, C), 33, 0.2)
    g0 = torch.randn(K, C, generator=_g(34)) * 0.01
    bits = torch.randint(0, 2 ** 62, (K, C), generator=_g(35))
    dt = torch.einsum("kht,khc->ktc", pds.float().flip(1), zu.float().flip(1))
    dxf = dt[:, 1:P + 1] + ((dt[:, 0] + g0) * (1.0 / P)).unsqueeze(1)
    dxe, dxb, keep, pre = A.attnpool_dx(pds, zu, g0, bits, P)
    got = torch.where(keep, dxf, torch.zeros_like(dxf)).bfloat16()
    ok, r, _ = A.check(got, dxe, dxb)
    rb, n = A.store_bias(got[keep], dxe[keep], pre[keep])
    assert ok and abs(rb) <= 0.02, (r, rb)
    lines.append(f"attnpool_dx: worst |err|/bound {r:.3f}, store bias {rb:+.4f} over {n}")
    gp0 = torch.full((P + 1, C), 0.25)
    gpe, gpb = A.attnpool_gpos(pds, zu, g0, gp0, P, run=8, blocks=5)
    dt0 = dt[:, :P + 1].clone()
    dt0[:, 0] += g0
    ok, r, _ = A.check(gp0 + dt0.flip(0).sum(0), gpe, gpb)
    assert ok, r
    lines.append(f"attnpool gpos: worst |err|/bound {r:.3f}")
    x = _bf((K, P, C), 36, 0.86)
    pos = torch.randn(P + 1, C, generator=_g(37)) * 0.022
    te = A.tokens_fwd(x, pos, 56)
    r0 = ((x.float().flip(1).sum(1) / P) + pos[0]).bfloat16()
    ok, r, _ = A.check(r0, te["row0"], te["row0_bound"])
    assert ok, r
    lines.append(f"tokens row 0: worst |err|/bound {r:.3f}")
    print("\n" + "\n".join(lines))


# -------------------------------------------------------------------------------------------------- mutants
def _mutants():
    """(name, got, exact, bound, bias (got, exact_rounded_in, pre) or None, reference of the old criterion)"""
    out = []
    q, k, v = _qkv(seed=40)
    f = A.attn_fwd(q, k, v, MAPPER_SCALE)
    for name, kw in (("truncating bf16 store of P (attn_small)", dict(truncate_p=True)),
                     ("truncating bf16 store of O (attn_small)", dict(truncate_o=True)),
                     ("mask off by one: first padded key in (score 0, V 0), t = 80", dict(extra_key=True))):
        g = _emu_small_fwd(q, k, v, MAPPER_SCALE, **kw)
        out.append((name, g, f["o"], f["bound"], (g, f["o_rw"], f["pre_rw"]), f["o"]))
    # attn_small's backward: a truncating dQ store, and a truncating store of the bf16 intermediate dS~ (both inside the dQ / dK
    # bound: it carries u_b sum_j |ds_j| |k_j| for dS~ next to u_b |dq| for the store)
    do = _bf(q.shape, 44, 0.5)
    b = A.attn_small_bwd(q, k, v, do, MAPPER_SCALE)
    g = _emu_small_bwd(q, k, v, do, MAPPER_SCALE, truncate_dq=True)[0]
    out.append(("truncating bf16 store of dQ (attn_small bwd)", g, b["dq"][0], b["dq"][1], (g, *b["dq_rw"]), b["dq"][0]))
    g = _emu_small_bwd(q, k, v, do, MAPPER_SCALE, truncate_ds=True)
    out.append(("truncating bf16 store of dS~, seen in dQ (attn_small bwd)", g[0], b["dq"][0], b["dq"][1], (g[0], *b["dq_rw"]), b["dq"][0]))
    out.append(("truncating bf16 store of dS~, seen in dK (attn_small bwd)", g[1], b["dk"][0], b["dk"][1], (g[1], *b["dk_rw"]), b["dk"][0]))
    # exp with a relative error of 2^-12 (every other key): the pool softmax's f32 p, and attn_last's
    S = torch.randn(3000, 56, generator=_g(41)) * 8.2
    pe, pb = A.softmax_fwd(S, 50, 0.125, 51)
    e = torch.exp(S[:, :50] * 0.125 - (S[:, :50] * 0.125).amax(-1, keepdim=True)) * (1 + 2.0 ** -12 * (torch.arange(50) % 2))
    out.append(("exp with relative error 2^-12 (pool softmax p)", e / e.sum(-1, keepdim=True), pe, pb, None, pe))
    fl = A.attn_fwd(q[:, -1:], k, v, MAPPER_SCALE, depth=A.NORM_DEPTH_WAVE, p_bf16=False)
    _, pm = _emu_last(q[:, -1], k, v, MAPPER_SCALE, exp_err=2.0 ** -12)
    out.append(("exp with relative error 2^-12 (attn_last p)", pm, fl["p"][:, 0], fl["p_bound"][:, 0], None, fl["p"][:, 0]))
    # rs = sum dP P~ with the bf16 P: the pool softmax backward, whose output is ds itself (inside attn_small the same slip moves
    # dQ / dK by less than their own bf16 budget: no bound on them can see it)
    ps = torch.softmax(S[:, :50] * 0.125, -1)
    dP = torch.randn(3000, 56, generator=_g(42)) * 1e-3
    dse, dsb, dspre = A.softmax_bwd(ps, dP, 0.125, 51)
    rs = (dP[:, :50] * ps.bfloat16().float()).sum(-1, keepdim=True)
    g = (ps * (dP[:, :50] - rs) * 0.125).bfloat16()
    out.append(("rs from the bf16 P (pool softmax bwd ds)", g, dse, dsb, (g, dse, dspre), dse))
    # attn_last reading V of the wrong head
    o, _ = _emu_last(q[:, -1], k, v, MAPPER_SCALE, head_shift=1)
    out.append(("wrong head offset (attn_last V)", o, fl["o"][:, 0], fl["bound"][:, 0], None, fl["o"][:, 0]))
    return out


def test_mutants_are_rejected_and_the_old_criterion_misses_some(capsys):
    lines = ["", "mutants (each must be rejected by the exact bound or the store-bias measure):"]
    missed_by_old = 0
    for name, got, exact, bound, bias, ref in _mutants():
        ok, ratio, _ = A.check(got, exact, bound)
        rb = A.store_bias(*bias)[0] if bias is not None else None
        rejected = _verdict(ok, ratio, rb)
        old_ok = A.old_criterion(got, ref)
        lines.append(f"  {name:62s} old 2e-2*max: {'ACCEPTS' if old_ok else 'rejects'}   new: {'rejects' if rejected else 'ACCEPTS'}"
                     f"  (worst |err|/bound {ratio:.3g}" + (f", store bias {rb:+.3f})" if rb is not None else ")"))
        assert rejected, name
        missed_by_old += old_ok
    with capsys.disabled():
        print("\n".join(lines))
    assert missed_by_old >= 6


def test_store_bias_separates_rne_from_truncation():
    q, k, v = _qkv(seed=50)
    f = A.attn_fwd(q, k, v, MAPPER_SCALE)
    rne, n = A.store_bias(X.round_bf16(f["o_rw"]), f["o_rw"], f["pre_rw"])
    tr, _ = A.store_bias(X.truncate_bf16(f["o_rw"]), f["o_rw"], f["pre_rw"])
    assert n > 50000 and abs(rne) <= 0.02 and -0.55 < tr < -0.45, (rne, tr, n)
