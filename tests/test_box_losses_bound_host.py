"""Host-side checks of tests/exact_box_losses.py (no GPU): (a) its references equal torch float64 autograd of the published
formulation -- Box2BoxTransform.apply_deltas + fvcore giou_loss, fvcore smooth_l1_loss -- losses and gradients, the constructed tie
rows included; (b) the reference's own f32 evaluation (tests/golden/ref_box_losses.npz, written by make_golden_box_losses.py) lies
inside the bounds; (c) an f32 emulation of the kernels, torch f32 operations one at a time, is accepted at every case of the list
the GPU test runs; (d) mutants of the emulation are each rejected at some case; (e) the config keys construct the model, an
unknown type raises the reference's ValueError, CLS_AGNOSTIC_BBOX_REG still refuses."""
import os

import numpy as np
import pytest
import torch

import exact_box_losses as B
import exact_losses as E
import test_losses_bound_host as H

f64 = E._f64
_t32 = H._t32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_box_losses.npz")


# ================================================================================================== the published formulation
def pub_apply_deltas(d, b, w, clamp):
    bw, bh = b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]
    cx, cy = b[:, 0] + 0.5 * bw, b[:, 1] + 0.5 * bh
    dx, dy = d[:, 0] / w[0], d[:, 1] / w[1]
    dw, dh = torch.clamp(d[:, 2] / w[2], max=clamp), torch.clamp(d[:, 3] / w[3], max=clamp)
    pcx, pcy = dx * bw + cx, dy * bh + cy
    pw, ph = torch.exp(dw) * bw, torch.exp(dh) * bh
    return torch.stack((pcx - 0.5 * pw, pcy - 0.5 * ph, pcx + 0.5 * pw, pcy + 0.5 * ph), dim=-1)


def pub_giou(boxes1, boxes2, eps):
    """fvcore.nn.giou_loss, reduction "none", statement by statement"""
    x1, y1, x2, y2 = boxes1.unbind(dim=-1)
    x1g, y1g, x2g, y2g = boxes2.unbind(dim=-1)
    xkis1, ykis1, xkis2, ykis2 = torch.max(x1, x1g), torch.max(y1, y1g), torch.min(x2, x2g), torch.min(y2, y2g)
    intsctk = torch.zeros_like(x1)
    mask = (ykis2 > ykis1) & (xkis2 > xkis1)
    intsctk[mask] = (xkis2[mask] - xkis1[mask]) * (ykis2[mask] - ykis1[mask])
    unionk = (x2 - x1) * (y2 - y1) + (x2g - x1g) * (y2g - y1g) - intsctk
    iouk = intsctk / (unionk + eps)
    xc1, yc1, xc2, yc2 = torch.min(x1, x1g), torch.min(y1, y1g), torch.max(x2, x2g), torch.max(y2, y2g)
    area_c = (xc2 - xc1) * (yc2 - yc1)
    return 1 - (iouk - ((area_c - unionk) / (area_c + eps)))


def pub_smooth_l1(inp, tgt, beta):
    n = torch.abs(inp - tgt)
    return n if beta < 1e-5 else torch.where(n < beta, 0.5 * n ** 2 / beta, n - 0.5 * beta)


def pub_get_deltas(s, t, w):
    sw, sh = s[:, 2] - s[:, 0], s[:, 3] - s[:, 1]
    sx, sy = s[:, 0] + 0.5 * sw, s[:, 1] + 0.5 * sh
    tw, th = t[:, 2] - t[:, 0], t[:, 3] - t[:, 1]
    tx, ty = t[:, 0] + 0.5 * tw, t[:, 1] + 0.5 * th
    return torch.stack([w[0] * (tx - sx) / sw, w[1] * (ty - sy) / sh, w[2] * torch.log(tw / sw), w[3] * torch.log(th / sh)], 1)


def _rows(n, seed, w):
    """the constructed rows followed by random ones: (box, gt, deltas, constructed mask)"""
    cb, cg, cd = B.constructed_rows(w)
    b, g, d = E._boxes(n, seed), E._boxes(n, seed + 1), B._deltas(n, w, seed + 2)
    con = torch.zeros(n + B.NCON, dtype=torch.bool)
    con[:B.NCON] = True
    return torch.cat([cb, b]), torch.cat([cg, g]), torch.cat([cd, d]), con


@pytest.mark.parametrize("w", [B.RPN_W, B.BOX_W])
def test_giou_reference_equals_torch_float64_autograd(w):
    """loss and gradient of every row, the tie rows with autograd's half shares, the clamp passing at equality; and the random rows of
    the reference alone are all decided with the mix wanted (disjoint and overlapping)"""
    b, g, d, con = _rows(2000, 301, w)
    ref = B.giou_ref(b, d, g, w, B.CLAMP_T, con)
    dd = f64(d).requires_grad_(True)
    w64 = [E.f32(x) for x in w]
    loss = pub_giou(pub_apply_deltas(dd, f64(b), w64, B.CLAMP_T), f64(g), B.GIOU_EPS)
    loss.sum().backward()
    assert float((loss.detach() - ref["loss"][0]).abs().max()) <= 1e-13
    scale = ref["grad"][0].abs().amax(1, keepdim=True).clamp_min(1e-30)
    # (float64's own cancellation at the matching row leaves 1e-16 of the O(1) intermediates next to a gradient of 1e-10)
    assert bool(((dd.grad - ref["grad"][0]).abs() <= 1e-10 * scale + 1e-13).all())
    assert bool(ref["decided"].all()), "the reference alone leaves a row undecided: change the seed"
    hit = ref["hit"][B.NCON:]                                             # overlapping rows; the others are disjoint
    assert 0.25 < float(hit.double().mean()) < 0.75
    # the conventions, stated directly
    gr = ref["grad"][0]
    assert bool((gr[B.ROW_MATCH, :2] == 0).all()) and bool((gr[B.ROW_MATCH, 2:].abs() < 1e-6).all()) and bool((gr[B.ROW_MATCH, 2:] != 0).all())
    assert bool((gr[B.ROW_CLAMP_OVER, 2:] == 0).all()) and bool(gr[B.ROW_CLAMP_EQ, 2] != 0)
    assert float(ref["loss"][0][B.ROW_TOUCH]) > 1.0                       # no intersection


@pytest.mark.parametrize("beta", [1.0 / 9, 1.0])
def test_smooth_l1_reference_equals_torch_float64_autograd(beta):
    b, g, d, _ = _rows(500, 311, B.BOX_W)
    d[::3] = B._f32_get_deltas(b, g, B.BOX_W)[::3] + E._randn((d[::3].shape[0], 4), 312, 0.05)
    ref = B.sl1_ref(d, b, g, B.BOX_W, beta)
    dd = f64(d).requires_grad_(True)
    t = pub_smooth_l1(dd, pub_get_deltas(f64(b), f64(g), [E.f32(x) for x in B.BOX_W]), E.f32(beta))
    t.sum().backward()
    assert float((t.detach() - ref["term"][0]).abs().max()) <= 1e-12
    assert float((dd.grad - ref["grad"][0]).abs().max()) <= 1e-12
    quad = ref["term"][0] < 0.5 * beta
    assert 0.05 < float(quad.double().mean()) < 0.95                      # both branches are met


# ================================================================================================== b. the reference's f32 evaluation
def _fixture_case(z, name):
    g = lambda k: torch.from_numpy(z[f"{name}/{k}"])
    return g


@pytest.mark.parametrize("name", ["rpn_giou", "rpn_sl1_b0.111", "rpn_sl1_b1", "box_giou", "box_sl1_b0.111", "box_sl1_b1"])
def test_reference_f32_evaluation_lies_inside_the_bounds(name):
    """the committed fixture: the reference's _dense_box_regression_loss / FastRCNNOutputLayers.box_reg_loss in f32 with torch
    autograd.  Its sum runs in torch's order, so the depth of the sum is the row count (any order stays inside that)"""
    z = np.load(GOLDEN)
    g = _fixture_case(z, name)
    loc = "giou" if "giou" in name else "smooth_l1"
    beta = float(z[f"{name}/beta"])
    w = tuple(float(x) for x in z[f"{name}/weights"])
    ncon = int(z[f"{name}/ncon"])
    c = dict(loc=loc, beta=beta)
    rep = E.Report()
    if name.startswith("rpn"):
        fgm, deltas, gtb = g("fg"), g("deltas"), g("gt")                    # [N, R], [N, R, 4], [N, R, 4]
        N, R = fgm.shape
        pos = torch.nonzero(fgm.reshape(-1))[:, 0]
        a = dict(logits=torch.zeros(N * R), deltas=deltas.reshape(-1, 4), pos=pos, neg=pos[:0], midx=torch.arange(N * R) % R,
                 gt=gtb.reshape(-1, 4), gt_off=torch.arange(N) * R, anchors=g("anchors"), A=R, w=w, inv_norm=1.0)
        assert not bool(fgm[1].any())                                       # the image without ground truth
        n = pos.numel()
        rep.bound(name + " loss", name, g("loss").reshape(1), tuple(x.reshape(1) for x in B.rpn_reg_ref(a, loc, beta, B.SCALE_CLAMP, depth=n)))
        ref = B.rpn_reg_ref(a, loc, beta, B.SCALE_CLAMP, gout=torch.tensor([0.0, 1.0]), ncon=ncon)
        grad = g("grad").reshape(-1, 4)
        B._loc_checks(rep, name + " grad", name, grad[pos], ref, c, ncon, own_zero=False)
        isp = torch.zeros(N * R, dtype=torch.bool)
        isp[pos] = True
        assert bool((grad[~isp] == 0).all())
    else:
        cls, deltas = g("classes"), g("deltas")
        K = deltas.shape[1] // 4
        R = cls.numel()
        fg = torch.nonzero((cls >= 0) & (cls < K))[:, 0]
        a = dict(deltas=deltas, fg=fg, cls=cls.clamp(max=K - 1), src=g("proposals"), tgt=g("gt"), w=w, inv_norm=1.0 / R)
        n = fg.numel()
        rep.bound(name + " loss", name, g("loss").reshape(1), tuple(x.reshape(1) for x in B.box_reg_ref(a, loc, beta, B.SCALE_CLAMP, depth=n)))
        ref = B.box_reg_ref(a, loc, beta, B.SCALE_CLAMP, gout=torch.tensor([1.0]), ncon=ncon)
        grad = g("grad")
        cols = B.box_cols(a)
        B._loc_checks(rep, name + " grad", name, grad[fg[:, None], cols], ref, c, ncon, own_zero=False)
        touched = torch.zeros(deltas.shape, dtype=torch.bool)
        touched[fg[:, None], cols] = True
        assert bool((grad[~touched] == 0).all())
    print({k: round(v, 3) for k, v in rep.worst.items()})
    assert not rep.fail, "\n".join(rep.fail)


# ================================================================================================== c. the f32 emulation, d. its mutants
class EmuBox(H.Emu):
    """cddmsl_rpn_losses_reg / cddmsl_box_reg_loss in f32 torch on the CPU, one operation at a time in the kernel's order (torch's
    summation order); ``mut`` names one mutant"""

    def _giou(self, b, d, t, w, clamp, want_grad):
        w = [_t32(v) for v in w]
        cl = _t32(clamp)
        eps = _t32(0.0 if self.mut == "giou_no_eps" else 1e-7)
        bw, bh = b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]
        cx, cy = b[:, 0] + 0.5 * bw, b[:, 1] + 0.5 * bh
        dx, dy, dw0, dh0 = d[:, 0] / w[0], d[:, 1] / w[1], d[:, 2] / w[2], d[:, 3] / w[3]
        if self.mut == "giou_no_clamp":
            dw, dh = dw0, dh0
        else:
            dw, dh = torch.where(dw0 > cl, cl, dw0), torch.where(dh0 > cl, cl, dh0)
        pcx, pcy = dx * bw + cx, dy * bh + cy
        pw, ph = torch.exp(dw) * bw, torch.exp(dh) * bh
        x1, y1, x2, y2 = pcx - 0.5 * pw, pcy - 0.5 * ph, pcx + 0.5 * pw, pcy + 0.5 * ph
        x1g, y1g, x2g, y2g = t.unbind(1)
        xk1, yk1, xk2, yk2 = torch.max(x1, x1g), torch.max(y1, y1g), torch.min(x2, x2g), torch.min(y2, y2g)
        hit = ((yk2 >= yk1) & (xk2 >= xk1)) if self.mut == "giou_ge" else ((yk2 > yk1) & (xk2 > xk1))
        iw, ih = xk2 - xk1, yk2 - yk1
        zero = torch.zeros_like(x1)
        inter = torch.where(hit, iw * ih, zero)
        sw, sh = x2 - x1, y2 - y1
        uni = sw * sh + (x2g - x1g) * (y2g - y1g) - inter
        ue = uni + eps
        iou = inter / ue
        xc1, yc1, xc2, yc2 = torch.min(x1, x1g), torch.min(y1, y1g), torch.max(x2, x2g), torch.max(y2, y2g)
        cw, ch = xc2 - xc1, yc2 - yc1
        ac = cw * ch
        ce = ac + eps
        loss = 1.0 - (iou - (ac - uni) / ce)
        if not want_grad:
            return loss, None
        g_u = inter / (ue * ue) - 1.0 / ce
        g_i = torch.where(hit, -(1.0 / ue) - g_u, zero)
        g_c = ue / (ce * ce)
        tie = 1.0 if self.mut == "giou_full_tie" else 0.5

        def share(p, g, hi):
            return torch.where(p == g, torch.full_like(p, tie), ((p > g) if hi else (p < g)).float())

        kx1, ky1, kx2, ky2 = share(x1, x1g, True), share(y1, y1g, True), share(x2, x2g, False), share(y2, y2g, False)
        ex1, ey1, ex2, ey2 = share(x1, x1g, False), share(y1, y1g, False), share(x2, x2g, True), share(y2, y2g, True)
        gx1 = -(g_u * sh) - (g_i * ih) * kx1 - (g_c * ch) * ex1
        gx2 = (g_u * sh) + (g_i * ih) * kx2 + (g_c * ch) * ex2
        gy1 = -(g_u * sw) - (g_i * iw) * ky1 - (g_c * cw) * ey1
        gy2 = (g_u * sw) + (g_i * iw) * ky2 + (g_c * cw) * ey2
        passes = (lambda v: v < cl) if self.mut == "giou_clamp_eq" else (lambda v: v <= cl)
        if self.mut == "giou_no_clamp":
            passes = lambda v: torch.ones_like(v, dtype=torch.bool)
        g0, g1 = (gx1 + gx2) * bw / w[0], (gy1 + gy2) * bh / w[1]
        g2 = torch.where(passes(dw0), 0.5 * (gx2 - gx1) * pw / w[2], zero)
        g3 = torch.where(passes(dh0), 0.5 * (gy2 - gy1) * ph / w[3], zero)
        return loss, torch.stack([g0, g1, g2, g3], 1)

    def _sl1(self, e, beta, want_grad):
        be = _t32(beta)
        n = e.abs()
        quad = n < be
        if self.mut == "sl1_no_div":
            term, grad = torch.where(quad, 0.5 * n * n, n - 0.5 * be), torch.where(quad, e, torch.sign(e))
        else:
            term, grad = torch.where(quad, 0.5 * n * n / be, n - 0.5 * be), torch.where(quad, e / be, torch.sign(e))
        return term, grad

    def _rows(self, dsel, src, tgt, w, loc, beta, clamp, want_grad):
        if loc == "giou":
            return self._giou(src, dsel, tgt, w, clamp, want_grad)
        e = dsel - self._deltas(src, tgt, w)
        if beta < 1e-5:
            return e.abs(), self._sgn(e)
        return self._sl1(e, beta, want_grad)

    def rpn_reg(self, logits, deltas, pos, neg, midx, gt, gt_off, anchors, A, w, inv_norm, loc, beta, clamp, gout=None):
        base = H.Emu.rpn(self, logits, deltas, pos, neg, midx, gt, gt_off, anchors, A, w, inv_norm, gout)
        inn = _t32(inv_norm)
        img = torch.div(pos, A, rounding_mode="floor")
        term, grad = self._rows(deltas[pos], anchors[pos - img * A], gt[midx[pos] + gt_off[img]], w, loc, beta, clamp, gout is not None)
        if gout is None:
            return torch.stack([base[0], term.sum() * inn])
        gl = gout[1] if self.mut == "grad_no_inv_norm" else gout[1] * inn
        dd = torch.zeros_like(deltas)
        dd[pos] = grad * gl
        return base[0], dd

    def box_reg(self, deltas, fg, cls, src, tgt, w, inv_norm, loc, beta, clamp, gout=None):
        inn = _t32(inv_norm)
        c0 = 4 * cls[fg] if (cls is not None and self.mut != "box_col0") else torch.zeros_like(fg)
        cols = c0[:, None] + torch.arange(4)[None, :]
        term, grad = self._rows(deltas[fg[:, None], cols], src[fg], tgt[fg], w, loc, beta, clamp, gout is not None)
        if gout is None:
            return (term.sum() * inn).reshape(1)
        gl = gout[0] if self.mut == "grad_no_inv_norm" else gout[0] * inn
        dd = torch.zeros_like(deltas)
        dd[fg[:, None], cols] = grad * gl
        return dd


def _run_all(impl, families=None):
    rep = E.Report()
    for name, cases, run in B.FAMILIES:
        if families is None or name in families:
            for c in cases():
                run(c, impl, rep)
    return rep


def test_bounds_accept_the_f32_emulation_at_every_case(capsys):
    rep = _run_all(EmuBox())
    with capsys.disabled():
        print("\n" + "\n".join(f"  {k:44s} {v:.3f}" for k, v in sorted(rep.worst.items())))
    assert not rep.fail, "\n".join(rep.fail[:20])


MUTANTS = [
    ("GIoU: eps dropped", "giou_no_eps", None),
    ("GIoU: the full gradient instead of half at a tie", "giou_full_tie", None),
    ("GIoU: >= in the intersection test (the touching row)", "giou_ge", None),
    ("GIoU: the clamp of dw / dh not applied", "giou_no_clamp", None),
    ("GIoU: the clamp blocks the gradient at equality", "giou_clamp_eq", None),
    ("smooth-L1: the quadratic branch without / beta", "sl1_no_div", None),
    ("inv_norm missing from the gradient", "grad_no_inv_norm", None),
    ("box head: class column 0 instead of the row's class", "box_col0", ("box_reg",)),
]


@pytest.mark.parametrize("what,mut,families", MUTANTS, ids=[m[1] for m in MUTANTS])
def test_mutants_are_rejected(what, mut, families):
    rep = _run_all(EmuBox(mut), families)
    assert rep.fail, f"accepted: {what}"


# ================================================================================================== e. the config keys
def _build(opts):
    from cddmsl_amd.config import get_cfg
    from cddmsl_amd.modeling import build_model
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cfg = get_cfg()
    cfg.merge_from_file(os.path.join(root, "configs", "VOC-Experiments", "faster_rcnn_CLIP_R_50_C4.yaml"))
    cfg.merge_from_list(list(opts) + ["MODEL.DEVICE", "cpu"])
    return build_model(cfg)


def test_config_keys_construct_the_model():
    m = _build(["MODEL.RPN.BBOX_REG_LOSS_TYPE", "giou"])
    assert m.proposal_generator.box_reg_loss_type == "giou" and m.roi_heads.box_predictor.box_reg_loss_type == "smooth_l1"
    m = _build(["MODEL.RPN.SMOOTH_L1_BETA", 0.111])
    assert m.proposal_generator.smooth_l1_beta == 0.111
    m = _build(["MODEL.ROI_BOX_HEAD.BBOX_REG_LOSS_TYPE", "giou", "MODEL.ROI_BOX_HEAD.SMOOTH_L1_BETA", 0.5])
    assert m.roi_heads.box_predictor.box_reg_loss_type == "giou" and m.roi_heads.box_predictor.smooth_l1_beta == 0.5
    assert m.proposal_generator.box_reg_loss_type == "smooth_l1" and m.proposal_generator.smooth_l1_beta == 0.0


def test_unknown_loss_type_and_class_agnostic_regression_are_refused():
    with pytest.raises(ValueError, match="Invalid dense box regression loss type 'diou'"):
        _build(["MODEL.RPN.BBOX_REG_LOSS_TYPE", "diou"])
    with pytest.raises(ValueError, match="Invalid bbox reg loss type 'ciou'"):
        _build(["MODEL.ROI_BOX_HEAD.BBOX_REG_LOSS_TYPE", "ciou"])
    with pytest.raises(AssertionError, match="CLS_AGNOSTIC_BBOX_REG"):
        _build(["MODEL.ROI_BOX_HEAD.CLS_AGNOSTIC_BBOX_REG", True])


def test_torch_branch_of_the_model_losses_equals_the_published_formulation():
    """modeling.rpn.box_reg_loss_terms (the torch branch of RPN.losses and FastRCNNOutputLayers.losses) against the statement-by-
    statement fvcore definitions above, float64"""
    from cddmsl_amd.modeling.rpn import box_reg_loss_terms
    b, g, d, _ = _rows(300, 321, B.BOX_W)
    w = B.BOX_W
    got = box_reg_loss_terms(d, b, g, w, "giou", 0.0)                    # (apply_deltas decodes in f32, as the reference's does)
    want = pub_giou(pub_apply_deltas(f64(d), f64(b), w, B.SCALE_CLAMP), f64(g), 1e-7).sum()
    assert got.dtype == torch.float32 and abs(float(got) - float(want)) <= 1e-5 * abs(float(want))
    b, g, d = f64(b), f64(g), f64(d)
    for beta in (0.0, 1.0 / 9, 1.0):
        got = box_reg_loss_terms(d, b, g, w, "smooth_l1", beta)
        want = pub_smooth_l1(d, pub_get_deltas(b, g, w), beta).sum()
        assert abs(float(got - want)) <= 1e-12 * abs(float(want))
