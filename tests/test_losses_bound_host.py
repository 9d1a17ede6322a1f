"""The loss checker itself (tests/exact_losses.py), on the CPU: the float64 references against torch's float64 forward and autograd
of the plain expressions (and the float64 oracle); every bound against an f32 emulation of its kernel that rounds at the same points
but sums in another order, at every case of the list the GPU test runs; and mutants of the emulation every one of which some case
must reject -- with the verdict of the old criterion of tests/test_gpu_ops.py (its tolerance, at its single shape) next to each.

Mutants the old criterion accepts (14 of 27): the L2 dot-product tail, the cosine D % 64 tail, cosine accumulate overwriting, the
cosine D > 1024 branch without iv, contrastive ld / n swapped, LayerNorm accumulate ignored, the truncated bf16 LayerNorm store, focal
padding lanes at exp(0), focal gamma = 0 down the unguarded gamma > 0 path, sgn(0) = 1, box L1 columns without ld, SGD without the
1e-6, SGD second-batch norms read from the first, SGD first_step reading the old momentum.

"gamma = 0 treated as gamma > 0" with the kernel's omp > 0 guard kept computes the same numbers (powf(x, 0) = 1, dmod = -0 * ...): no
test can tell it apart.  The mutant here drops the guards as well, so that a saturated row forms 0 * powf(0, -1)."""
import torch
import torch.nn.functional as F

import exact_gemm as X
import exact_losses as E

f64 = E._f64


def _close(a, b, tol=1e-12):
    a, b = f64(a).detach(), f64(b).detach()
    return float((a - b).abs().max()) <= tol * max(float(b.abs().max()), 1e-300) if b.numel() else True


G = torch.Generator()              # the reference tests' operands: re-seeded at the start of each


def _rn(*shape):
    return torch.randn(*shape, generator=G, dtype=torch.float64)


def _t32(v):
    return torch.tensor(float(v), dtype=torch.float32)


# ================================================================================================== the f32 emulation and its mutants
class Emu:
    """every kernel in f32 torch on the CPU: the kernel's rounding points, torch's summation order.  ``mut`` names one mutant"""

    def __init__(self, mut=None):
        self.mut = mut

    # ---- L2
    def l2_fwd(self, x, eps):
        iv = 1.0 / torch.clamp((x * x).sum(1).sqrt(), min=_t32(eps))
        return x * iv[:, None], iv

    def l2_bwd(self, dy, y, inv):
        D = y.shape[1]
        k = D - D % 256 if self.mut == "l2_dot_tail" else D
        dot = (dy[:, :k] * y[:, :k]).sum(1, keepdim=True)
        return inv[:, None] * (dy - y * dot)

    # ---- cosine logits
    def cos_fwd(self, x, wn, T, eps):
        D, Kc = x.shape[1], wn.shape[0]
        iv = 1.0 / torch.clamp((x * x).sum(1).sqrt(), min=_t32(eps))
        k = D - D % 64 if self.mut == "cos_tail" else D
        dot = ((x * iv[:, None])[:, None, :k] * wn[None, :, :k]).sum(-1)
        sc = torch.zeros(x.shape[0], Kc + 1)
        sc[:, :Kc] = dot * (_t32(1.0) / _t32(T))
        if self.mut == "cos_bg":
            sc[:, Kc] = 1e-3
        return sc, iv

    def cos_bwd(self, ds, x, wn, inv, T, dx0):
        Kc = wn.shape[0]
        g = ((ds[:, :Kc] * (_t32(1.0) / _t32(T)))[:, :, None] * wn[None]).sum(1)
        iv = inv[:, None]
        xv = x * iv
        dot = (g * (x if (self.mut == "cos_big_noiv" and x.shape[1] > 1024) else xv)).sum(1, keepdim=True)
        v = iv * (g - xv * dot)
        return v if (dx0 is None or self.mut == "cos_acc_overwrite") else dx0 + v

    # ---- contrastive
    def _S(self, S, n, column_pass):
        if self.mut == "con_swap" and column_pass:                # the row stride taken as n
            return S.reshape(-1)[:n * n].view(n, n)
        return S[:n, :n]

    def con_fwd(self, S, n):
        def lse(s):
            m = s.amax(1, keepdim=True)
            return (m + torch.log(torch.exp(s - m).sum(1, keepdim=True)))[:, 0]
        rl, cl = lse(self._S(S, n, False)), lse(self._S(S, n, True).t())
        d = S[:n, :n].diagonal()
        s = ((rl - d) + (cl - d)).sum()
        loss = (s if self.mut == "con_scale" else 0.5 * s) / _t32(n)
        return rl, cl, loss.reshape(1)

    def con_bwd(self, S, rl, cl, gloss, n):
        s = self._S(S, n, True)
        g = torch.exp(s - rl[:, None]) + torch.exp(s - cl[None, :]) - (1.0 if self.mut == "con_diag1" else 2.0) * torch.eye(n)
        return g * gloss[0] * (1.0 if self.mut == "con_scale" else 0.5) / _t32(n)

    # ---- LayerNorm
    def ln_fwd(self, x, ga, be, eps, dt, mis=None):
        D = x.shape[1]
        mu = x.sum(1, keepdim=True) / _t32(D)
        c = x - mu
        var = (c * c).sum(1, keepdim=True) / _t32(D - 1 if (self.mut == "ln_var_dm1" and D > 1) else D)
        rs = 1.0 / (var.sqrt() + _t32(eps)) if self.mut == "ln_eps_outside" else torch.rsqrt(var + _t32(eps))
        y = c * rs * ga + be
        if dt == torch.bfloat16:
            y = X.truncate_bf16(y).bfloat16() if self.mut == "ln_trunc" else y.bfloat16()
        return y, mu[:, 0], rs[:, 0]

    def ln_bwd(self, dy, x, ga, mean, rstd, dx0, mis=None):
        D = x.shape[1]
        g = dy.float() * ga
        xh = (x - mean[:, None]) * rstd[:, None]
        sg = g.sum(1, keepdim=True) / _t32(D)
        sgx = (g * xh).sum(1, keepdim=True) / _t32(D)
        v = rstd[:, None] * ((g if self.mut == "ln_no_sg" else g - sg) - xh * sgx)
        return v if (dx0 is None or self.mut == "ln_acc_ignored") else dx0 + v

    # ---- focal CE
    def focal_fwd(self, z, t, gamma, bg, bgw):
        R, C = z.shape
        ar = torch.arange(R)
        zz = torch.cat([z, torch.zeros(R, 64 - C)], 1) if (self.mut == "focal_pad" and C < 64) else z
        mx = zz.amax(1, keepdim=True)
        e = torch.exp(zz - mx)
        se = e.sum(1, keepdim=True)
        p = (e / se)[:, :C]
        ce = (mx + torch.log(se))[:, 0] - z[ar, t]
        w = torch.where(t == (0 if self.mut == "focal_bg0" else bg), _t32(bgw), _t32(1.0))
        ga = _t32(gamma)
        mod = torch.pow(torch.clamp(1.0 - p[ar, t], min=0.0), ga) if (ga > 0 or self.mut == "focal_gamma0") else torch.ones(R)
        return ce * mod * w, p

    def focal_bwd(self, z, t, p, gs, gamma, bg, bgw):
        R, C = p.shape
        ar = torch.arange(R)
        pt = p[ar, t][:, None]
        one = torch.zeros_like(p)
        one[ar, t] = 1.0
        w = torch.where(t == (0 if self.mut == "focal_bg0" else bg), _t32(bgw), _t32(1.0))[:, None]
        ga = _t32(gamma)
        ce = -torch.log(torch.clamp(pt, min=1e-38))
        omp = torch.clamp(1.0 - pt, min=0.0)
        if self.mut == "focal_gamma0":                            # no guards: gamma = 0 goes down the gamma > 0 path
            mod, dmod = torch.pow(omp, ga), -ga * torch.pow(omp, ga - 1.0) * pt * (one - p)
        elif ga > 0:
            mod = torch.pow(omp, ga)
            dmod = torch.where(omp > 0, -ga * torch.pow(omp, ga - 1.0) * pt * (one - p), torch.zeros_like(p))
        else:
            mod, dmod = torch.ones_like(pt), torch.zeros_like(p)
        if self.mut == "focal_no_dmod":
            dmod = torch.zeros_like(p)
        return w * (mod * (p - one) + ce * dmod) * gs[0]

    # ---- sampled losses
    @staticmethod
    def _deltas(s, t, w):
        sw, sh = s[:, 2] - s[:, 0], s[:, 3] - s[:, 1]
        sx, sy = s[:, 0] + 0.5 * sw, s[:, 1] + 0.5 * sh
        tw, th = t[:, 2] - t[:, 0], t[:, 3] - t[:, 1]
        tx, ty = t[:, 0] + 0.5 * tw, t[:, 1] + 0.5 * th
        w = [_t32(v) for v in w]
        return torch.stack([w[0] * (tx - sx) / sw, w[1] * (ty - sy) / sh, w[2] * torch.log(tw / sw), w[3] * torch.log(th / sh)], 1)

    def _sgn(self, e):
        s = torch.sign(e)
        return torch.where(e == 0, torch.ones_like(s), s) if self.mut == "sgn0" else s

    def rpn(self, logits, deltas, pos, neg, midx, gt, gt_off, anchors, A, w, inv_norm, gout=None):
        inn = _t32(inv_norm)
        rows = torch.cat([pos, neg])
        x = logits[rows]
        y = torch.cat([torch.zeros(pos.numel()) if self.mut == "rpn_pos0" else torch.ones(pos.numel()), torch.zeros(neg.numel())])
        img = torch.div(pos, A, rounding_mode="floor")
        a = pos.clamp(max=A - 1) if self.mut == "rpn_anchor_r" else pos - img * A
        gi = midx[pos] if self.mut == "rpn_gtoff" else midx[pos] + gt_off[img]
        e = deltas[pos] - self._deltas(anchors[a], gt[gi], w)
        if gout is None:
            cls = (torch.clamp(x, min=0) - x * y + torch.log1p(torch.exp(-x.abs()))).sum()
            return torch.stack([cls * inn, e.abs().sum() * inn])
        gc, gl = gout[0] * inn, gout[1] * inn
        dl, dd = torch.zeros_like(logits), torch.zeros_like(deltas)
        dl[rows] = (1.0 / (1.0 + torch.exp(-x)) - y) * gc
        dd[pos] = self._sgn(e) * gl
        return dl, dd

    def box(self, deltas, fg, cls, src, tgt, w, inv_norm, gout=None):
        inn = _t32(inv_norm)
        R, ld = deltas.shape
        c0 = 4 * cls[fg] if cls is not None else torch.zeros_like(fg)
        cols = c0[:, None] + torch.arange(4)[None, :]
        if self.mut == "box_no_ld" and cls is not None:           # rows taken as 4 Kc wide whatever ld is
            flat = fg[:, None] * (4 * E.BOX_KC) + cols
        else:
            flat = fg[:, None] * ld + cols
        e = deltas.reshape(-1)[flat] - self._deltas(src[fg], tgt[fg], w)
        if gout is None:
            return (e.abs().sum() * inn).reshape(1)
        dd = torch.zeros_like(deltas)
        dd.view(-1)[flat] = self._sgn(e) * (gout[0] * inn)
        return dd

    # ---- SGD
    def sgd(self, lay, p, g, m, ws, lr, mo, wd, clip, first):
        p2, m2, ws2 = p.clone(), m.clone(), ws.clone()
        lr, mo, wd, clip = _t32(lr), _t32(mo), _t32(wd), _t32(clip)
        for i, (n, op, og, om) in enumerate(lay):
            gi = g[og:og + n]
            ws2[i] = (gi * gi).sum()
        for i, (n, op, og, om) in enumerate(lay):
            nrm = torch.sqrt(ws2[i % E.SGD_MAX if self.mut == "sgd_batch_norm" else i])
            coef = torch.clamp(clip / (nrm if self.mut == "sgd_no_eps" else nrm + _t32(1e-6)), max=1.0)
            k = n - n % 4 if self.mut == "sgd_tail" else n
            pi, gi, mi = p[op:op + k], g[og:og + k], m[om:om + k]
            gg = (gi + wd * pi) * coef if self.mut == "sgd_wd_before" else gi * coef + wd * pi
            mm = gg if (first and self.mut != "sgd_first_reads_m") else mo * mi + gg
            m2[om:om + k] = mm
            p2[op:op + k] = pi - lr * mm
        return p2, m2, ws2


def _run_all(impl, families=None):
    rep = E.Report()
    for name, cases, run in E.FAMILIES:
        if families is None or name in families:
            for c in cases():
                run(c, impl, rep)
    return rep.finish()


# ================================================================================================== a. references = torch float64
def test_l2_cosine_contrastive_references_equal_torch_float64():
    G.manual_seed(101)
    from oracle import model as om
    x = _rn(7, 200).requires_grad_(True)
    dy = _rn(7, 200)
    y = F.normalize(x, dim=1, eps=1e-12)
    (gx,) = torch.autograd.grad(y, x, dy)
    r = E.l2_fwd(x.detach(), 1e-12)
    assert _close(r["y"][0], y) and _close(r["inv"][0], 1 / x.detach().norm(dim=1))
    assert _close(E.l2_bwd(dy, r["y"][0], r["inv"][0])["dx"][0], gx)
    # cosine logits: x/|x| . wn * invT with a zero background column, and its input gradient (accumulated into dx0)
    wn = F.normalize(_rn(9, 200), dim=1)
    ds = _rn(7, 10)
    s = torch.cat([F.normalize(x, dim=1) @ wn.t() * E.inv_t(0.01), torch.zeros(7, 1, dtype=torch.float64)], 1)
    (gx,) = torch.autograd.grad(s, x, ds)
    c = E.cos_fwd(x.detach(), wn, 0.01, 1e-12)
    assert _close(c["scores"][0], s[:, :9])
    dx0 = _rn(7, 200)
    assert _close(E.cos_bwd(ds, x.detach(), wn, c["inv"][0], 0.01)["dx"][0], gx)
    assert _close(E.cos_bwd(ds, x.detach(), wn, c["inv"][0], 0.01, dx0)["dx"][0], dx0 + gx)
    # symmetric contrastive CE: the oracle's loss, and dS by autograd, from a padded S
    a, b = _rn(11, 40), _rn(11, 40)
    an, bn = E.l2_fwd(a, 0.0)["y"][0], E.l2_fwd(b, 0.0)["y"][0]
    St = (an @ bn.t() * 7.0).requires_grad_(True)
    gt = torch.arange(11)
    loss = (F.cross_entropy(St, gt) + F.cross_entropy(St.t(), gt)) / 2
    (gS,) = torch.autograd.grad(loss, St, torch.tensor(-0.37, dtype=torch.float64))
    Sp = torch.full((11, 16), float("nan"), dtype=torch.float64)
    Sp[:, :11] = St.detach()
    f = E.con_fwd(Sp, 11)
    assert _close(f["rlse"][0], torch.logsumexp(St.detach(), 1)) and _close(f["clse"][0], torch.logsumexp(St.detach(), 0))
    assert _close(E.con_loss(Sp, f["rlse"][0], f["clse"][0], 11)["loss"][0], loss)
    assert _close(E.con_bwd(Sp, f["rlse"][0], f["clse"][0], torch.tensor([-0.37], dtype=torch.float64), 11)["dS"][0], gS)
    S1 = an @ bn.t()
    f1 = E.con_fwd(S1, 11)
    assert _close(E.con_loss(S1, f1["rlse"][0], f1["clse"][0], 11)["loss"][0], om.symmetric_ce(a, b))


def test_layernorm_and_focal_references_equal_torch_float64():
    G.manual_seed(102)
    from oracle import model as om
    x = (_rn(6, 65) + 3.0).requires_grad_(True)
    ga, be = 1 + 0.1 * _rn(65), 0.1 * _rn(65)
    dy = _rn(6, 65)
    eps = E.f32(1e-5)
    y = F.layer_norm(x, (65,), ga, be, eps)
    (gx,) = torch.autograd.grad(y, x, dy)
    r = E.ln_fwd(x.detach(), ga, be, 1e-5, torch.float32)
    assert _close(r["y"][0], y) and _close(r["mean"][0], x.detach().mean(1))
    assert _close(r["rstd"][0], (x.detach().var(1, unbiased=False) + eps).rsqrt())
    dx0 = _rn(6, 65)
    assert _close(E.ln_bwd(dy, x.detach(), ga, r["mean"][0], r["rstd"][0])["dx"][0], gx)
    assert _close(E.ln_bwd(dy, x.detach(), ga, r["mean"][0], r["rstd"][0], dx0)["dx"][0], dx0 + gx)
    # focal CE: oracle.model.focal_loss (background = the last class, weight and gamma from its Cfg), and gamma = 0, 2
    for gamma in (0.5, 0.0, 2.0):
        cfg = om.Cfg()
        cfg.focal_gamma = gamma
        C = cfg.num_classes + 1
        z = (_rn(40, C) * 3).requires_grad_(True)
        t = torch.randint(0, C, (40,), generator=G)
        t[:5] = C - 1
        loss = om.focal_loss(cfg, z, t)
        (gz,) = torch.autograd.grad(loss, z)
        f = E.focal_fwd(z.detach(), t, gamma, C - 1, cfg.bg_cls_loss_weight)
        assert _close(f["row_loss"][0].mean(), loss) and _close(f["probs"][0], torch.softmax(z.detach(), 1))
        b = E.focal_bwd(t, f["probs"][0], torch.tensor([1.0 / 40], dtype=torch.float64), gamma, C - 1, cfg.bg_cls_loss_weight)
        assert _close(b["dlogits"][0], gz)


def test_sampled_loss_and_sgd_references_equal_torch_float64():
    G.manual_seed(103)
    from oracle import model as om
    from oracle import ops
    a, _ = E.rpn_inputs(dict(npos=40, nneg=90))
    a = {k: (v.double() if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in a.items()}
    lg, dl = a["logits"].clone().requires_grad_(True), a["deltas"].clone().requires_grad_(True)
    inn = E.f32(a["inv_norm"])
    rows = torch.cat([a["pos"], a["neg"]])
    lab = torch.cat([torch.ones(40), torch.zeros(90)]).double()
    cls = F.binary_cross_entropy_with_logits(lg[rows], lab, reduction="sum") * inn
    img = a["pos"] // a["A"]
    tg = ops.get_deltas(a["anchors"][a["pos"] % a["A"]], a["gt"][a["midx"][a["pos"]] + a["gt_off"][img]], [E.f32(w) for w in a["w"]])
    loc = (dl[a["pos"]] - tg).abs().sum() * inn
    gout = torch.tensor([1.5, 0.7])
    g32 = gout * torch.tensor(inn, dtype=torch.float32)             # the kernel forms f32(gout * inv_norm): scale the autograd loss by it
    glg, gdl = torch.autograd.grad(cls * (float(g32[0]) / inn) + loc * (float(g32[1]) / inn), (lg, dl))
    assert _close(E.rpn_ref(**a)["out2"][0], torch.stack([cls, loc]))
    rb = E.rpn_ref(**a, gout=gout)
    assert _close(rb["dlogits"][0], glg) and _close(rb["ddeltas"], gdl)
    b, _ = E.box_inputs(dict(nfg=50, form="specific_padded"))
    b = {k: (v.double() if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in b.items()}
    d2 = b["deltas"].clone().requires_grad_(True)
    fg = b["fg"]
    ref = (d2[:, :4 * E.BOX_KC].reshape(E.BOX_R, E.BOX_KC, 4)[fg, b["cls"][fg]] - ops.get_deltas(b["src"][fg], b["tgt"][fg], list(b["w"]))).abs().sum() * E.f32(b["inv_norm"])
    (gd,) = torch.autograd.grad(ref, d2)
    assert _close(E.box_ref(**b)["out1"][0], ref)
    assert torch.equal(torch.sign(E.box_ref(**b, gout=torch.tensor([1.0]))["ddeltas"]).double(), torch.sign(gd))
    # SGD: oracle.model.sgd_step in float64, two steps
    cfg = om.Cfg()
    ps = [_rn(n) for n in (1, 5, 35, 1000)]
    gs = [_rn(n) * s for n, s in zip((1, 5, 35, 1000), (10.0, 0.001, 3.0, 0.0))]
    sd, mom, ms = {str(i): p.clone() for i, p in enumerate(ps)}, {}, [torch.zeros_like(p) for p in ps]
    for it in (150, 151):
        lr = om.sgd_step(sd, {str(i): g for i, g in enumerate(gs)}, mom, cfg, it)
        out = E.sgd_ref(ps, gs, ms, lr, cfg.momentum, cfg.weight_decay, cfg.clip_value, it == 150, exact_scalars=True)
        ps, ms = [o["p"][0] for o in out], [o["m"][0] for o in out]
        for i in range(4):
            assert _close(ps[i], sd[str(i)]) and _close(ms[i], mom[str(i)])


# ================================================================================================== b. the emulation inside every bound
def test_bounds_accept_the_f32_emulation_at_every_case(capsys):
    rep = _run_all(Emu())
    lines = ["", "f32 emulation, worst |err| / bound per output over the shared case list:"]
    lines += [f"  {k:44s} {v:.3f}" + (f"   store bias {rep.bias[k]:.4f} ulp" if k in rep.bias else "") for k, v in sorted(rep.worst.items())]
    with capsys.disabled():
        print("\n".join(lines))
    assert not rep.fail, "\n".join(rep.fail)
    assert all(v <= 1.0 for v in rep.worst.values())
    assert "layernorm_fwd y bf16" in rep.bias


# ================================================================================================== c. mutants
def _rel_ok(got, ref, tol, floor=0.0):
    got, ref = f64(got), f64(ref)
    return bool(float((got - ref).abs().max()) < tol * max(float(ref.abs().max()), floor))


def _old_cos_l2_con(emu):
    """test_cosine_logits_and_contrastive: R = 37, D = 1024, Kc = 20, no accumulate, < 1e-4 max|ref|; n = 48, D = 256, ld = n,
    |loss - ref| < 1e-5 |ref|, the input gradients < 1e-4 max|ref|"""
    x, wn, ds = E._randn((37, 1024), 1), F.normalize(E._randn((20, 1024), 2), dim=1), E._randn((37, 21), 3)
    sc, inv = emu.cos_fwd(x, wn, 0.01, 1e-12)
    ok = _rel_ok(sc[:, :20], E.cos_fwd(x, wn, 0.01, 1e-12)["scores"][0], 1e-4) and bool((sc[:, -1] == 0).all())
    ok &= _rel_ok(emu.cos_bwd(ds, x, wn, inv, 0.01, None), E.cos_bwd(ds, x, wn, inv, 0.01)["dx"][0], 1e-4)
    a, b = E._randn((48, 256), 4), E._randn((48, 256), 5)
    an, ia = emu.l2_fwd(a, 0.0)
    bn, _ = emu.l2_fwd(b, 0.0)
    S = an @ bn.t()
    rl, cl, loss = emu.con_fwd(S, 48)
    ad = a.double().requires_grad_(True)
    from oracle import model as om
    ref = om.symmetric_ce(ad, b.double())
    (ga,) = torch.autograd.grad(ref, ad)
    ok &= abs(float(loss) - float(ref.detach())) < 1e-5 * abs(float(ref.detach()))
    dS = emu.con_bwd(S, rl, cl, torch.ones(1), 48)
    ok &= _rel_ok(emu.l2_bwd(dS @ bn, an, ia), ga, 1e-4)
    return bool(ok)


def _old_ln_focal(emu):
    """test_layernorm_and_focal_ce: R = 37, D = 768, aligned, no accumulate: |y - ref| < 1e-5 (bf16 3e-2), dx < 1e-5 max(1, max|ref|);
    R = 61, C = 21, gamma 0.5, spread 30, background = class 20 at weight 0.2: loss 1e-5 relative, gradient 1e-5 max|ref| + 1e-9"""
    x, ga, be, dy = E._randn((37, 768), 1), 1 + 0.1 * E._randn((768,), 2), 0.1 * E._randn((768,), 3), E._randn((37, 768), 4)
    ref = E.ln_fwd(x, ga, be, 1e-5, torch.float32)
    y, mean, rstd = emu.ln_fwd(x, ga, be, 1e-5, torch.float32)
    ok = float((f64(y) - ref["y"][0]).abs().max()) < 1e-5
    ok &= float((f64(emu.ln_fwd(x, ga, be, 1e-5, torch.bfloat16)[0]) - ref["y"][0]).abs().max()) < 3e-2
    ok &= _rel_ok(emu.ln_bwd(dy, x, ga, mean, rstd, None), E.ln_bwd(dy, x, ga, ref["mean"][0], ref["rstd"][0])["dx"][0], 1e-5, 1.0)
    z = E._randn((61, 21), 5, 30.0)
    t = torch.randint(0, 21, (61,), generator=E._g(6))
    t[:7] = 20
    row, p = emu.focal_fwd(z, t, 0.5, 20, 0.2)
    fr = E.focal_fwd(z, t, 0.5, 20, 0.2)
    lref = float(fr["row_loss"][0].mean())
    ok &= abs(float(row.double().mean()) - lref) < 1e-5 * abs(lref)
    gs = torch.tensor([1.0 / 61])
    gref = E.focal_bwd(t, fr["probs"][0], gs, 0.5, 20, 0.2)["dlogits"][0]
    ok &= float((f64(emu.focal_bwd(z, t, p, gs, 0.5, 20, 0.2)) - gref).abs().max()) < 1e-5 * float(gref.abs().max()) + 1e-9
    return bool(ok)


def _allclose(got, ref, rtol=1e-5, atol=0.0):
    return bool(torch.allclose(f64(got), f64(ref), rtol=rtol, atol=atol))


def _old_sampled(emu):
    """test_sampled_loss_kernels_match_torch: 5 positives, ~90 negatives, no delta equal to its target, class-specific ld = 4 Kc
    and the class-agnostic form: allclose(rtol 1e-5) on the sums, allclose(rtol 1e-5, atol 1e-9) on the gradients"""
    a, eq = E.rpn_inputs(dict(npos=5, nneg=90))
    a["deltas"][eq] = E._randn((eq.numel(), 4), 7)
    gout = torch.tensor([1.5, 0.7])
    ok = _allclose(emu.rpn(**a), E.rpn_ref(**a)["out2"][0])
    dl, dd = emu.rpn(**a, gout=gout)
    r = E.rpn_ref(**a, gout=gout)
    ok &= _allclose(dl, r["dlogits"][0], atol=1e-9) and _allclose(dd, r["ddeltas"], atol=1e-9)
    for form in ("specific", "agnostic"):
        b, eq = E.box_inputs(dict(nfg=50, form=form))
        b["deltas"][eq] = E._randn((eq.numel(), b["deltas"].shape[1]), 8)
        ok &= _allclose(emu.box(**b), E.box_ref(**b)["out1"][0])
        if form == "specific":
            ok &= _allclose(emu.box(**b, gout=torch.ones(1)), E.box_ref(**b, gout=torch.ones(1))["ddeltas"], atol=1e-9)
    return bool(ok)


def _old_sgd(emu):
    """test_sgd_clip_step: four separately allocated (aligned) tensors, momentum zero-filled, clip 5, wd 1e-4, two steps:
    |p - ref| < 1e-6, |m - ref| < 1e-5"""
    sizes = [64 * 3 * 3 * 32, 1000, 35, 2048 * 512]
    lay, cur = [], 0
    for n in sizes:
        lay.append((n, cur, cur, cur))
        cur = (cur + n + 3) // 4 * 4
    p, g, m = torch.zeros(cur), torch.zeros(cur), torch.zeros(cur)
    for i, (n, o, _, _) in enumerate(lay):
        p[o:o + n] = E._randn((n,), i)
        g[o:o + n] = E._randn((n,), 10 + i, 3.0 if i % 2 else 0.01)
    ws = torch.zeros(4)
    ok = True
    for first in (1, 0):
        ref = E.sgd_ref(E.sgd_views(p, lay, 1), E.sgd_views(g, lay, 2), E.sgd_views(m, lay, 3), 0.02, 0.9, 1e-4, 5.0, first)
        p, m, ws = emu.sgd(lay, p, g, m, ws, 0.02, 0.9, 1e-4, 5.0, first)
        for i, (n, o, _, _) in enumerate(lay):
            ok &= float((f64(p[o:o + n]) - ref[i]["p"][0]).abs().max()) < 1e-6 and float((f64(m[o:o + n]) - ref[i]["m"][0]).abs().max()) < 1e-5
    return bool(ok)


MUTANTS = (
    ("L2 backward: the projection's dot product misses its last D % 256 elements", "l2_dot_tail", ("l2",), _old_cos_l2_con),
    ("cosine forward: the last D % 64 elements of a row dropped", "cos_tail", ("cos",), _old_cos_l2_con),
    ("cosine forward: background column non-zero", "cos_bg", ("cos",), _old_cos_l2_con),
    ("cosine backward: accumulate overwrites", "cos_acc_overwrite", ("cos",), _old_cos_l2_con),
    ("cosine backward: the D > 1024 branch forms dot without iv", "cos_big_noiv", ("cos",), _old_cos_l2_con),
    ("contrastive: ld and n swapped in the column pass", "con_swap", ("con",), _old_cos_l2_con),
    ("contrastive: diagonal term 1 instead of 2", "con_diag1", ("con",), _old_cos_l2_con),
    ("contrastive: scale 1/n instead of 1/(2n)", "con_scale", ("con",), _old_cos_l2_con),
    ("LayerNorm: variance over D - 1", "ln_var_dm1", ("ln",), _old_ln_focal),
    ("LayerNorm: eps added outside the root", "ln_eps_outside", ("ln",), _old_ln_focal),
    ("LayerNorm backward: without the sg term", "ln_no_sg", ("ln",), _old_ln_focal),
    ("LayerNorm backward: accumulate ignored", "ln_acc_ignored", ("ln",), _old_ln_focal),
    ("LayerNorm: bf16 store truncated (store_bias)", "ln_trunc", ("ln",), _old_ln_focal),
    ("focal: padding lanes contribute exp(0)", "focal_pad", ("focal",), _old_ln_focal),
    ("focal: background weight applied to class 0 instead of bg_class", "focal_bg0", ("focal",), _old_ln_focal),
    ("focal backward: without the ce * dmod term", "focal_no_dmod", ("focal",), _old_ln_focal),
    ("focal: gamma = 0 sent down the gamma > 0 path, unguarded (0 * powf(0, -1))", "focal_gamma0", ("focal",), _old_ln_focal),
    ("RPN: positives labelled 0", "rpn_pos0", ("rpn",), _old_sampled),
    ("RPN: gt_off ignored", "rpn_gtoff", ("rpn",), _old_sampled),
    ("RPN: anchor taken as r instead of r % A", "rpn_anchor_r", ("rpn",), _old_sampled),
    ("RPN / box L1: sgn(0) = 1", "sgn0", ("rpn", "box"), _old_sampled),
    ("box L1: class columns indexed without ld", "box_no_ld", ("box",), _old_sampled),
    ("SGD: weight decay added before the clip coefficient", "sgd_wd_before", ("sgd",), _old_sgd),
    ("SGD: 1e-6 missing in the coefficient", "sgd_no_eps", ("sgd",), _old_sgd),
    ("SGD: the n % 4 tail skipped", "sgd_tail", ("sgd",), _old_sgd),
    ("SGD: norms of the second batch (tensor 97 onward) read from the first", "sgd_batch_norm", ("sgd",), _old_sgd),
    ("SGD: first_step reads the old momentum", "sgd_first_reads_m", ("sgd",), _old_sgd),
)


def test_mutants_are_rejected_and_the_old_criterion_misses_some(capsys):
    lines = ["", "mutants of the emulation (each must be rejected at some case of the shared list):"]
    missed_by_old, survivors = [], []
    for name, key, fams, old in MUTANTS:
        rep = _run_all(Emu(key), fams)
        old_ok = old(Emu(key))
        w = max(rep.worst.values())
        lines.append(f"  {name:80s} old: {'ACCEPTS' if old_ok else 'rejects'}   new: {'rejects' if rep.rejected else 'ACCEPTS'}"
                     f"  ({len(rep.fail)} checks fail, worst |err|/bound {w:.3g})")
        if not rep.rejected:
            survivors.append(name)
        if old_ok:
            missed_by_old.append(name)
    with capsys.disabled():
        print("\n".join(lines))
    assert not survivors, survivors
    assert len(missed_by_old) >= 10, missed_by_old


def test_old_criteria_accept_the_unmutated_emulation():
    """the old-criterion restatements above are not stricter than the tests they restate: the plain emulation passes all four"""
    assert _old_cos_l2_con(Emu()) and _old_ln_focal(Emu()) and _old_sampled(Emu()) and _old_sgd(Emu())
