"""cddmsl_rpn_losses_reg / cddmsl_box_reg_loss (cddmsl_amd/csrc/losses.hip) against the float64 references and derived bounds of
tests/exact_box_losses.py, through the raw C-ABI with sentinel-filled, over-long outputs (the helpers of test_gpu_losses_exact.py),
at the case list the host test shares (tests/test_box_losses_bound_host.py runs the same drivers on an f32 emulation and its
mutants); then RPN.losses and FastRCNNOutputLayers.losses under the new config values, kernel branch against torch branch; then one
reduced-size f32 training step with smooth-L1 beta > 0 against the oracle (which has no GIoU).

  test_rpn_losses_reg    N = 3 images of A = 400 anchors, image 1 without boxes; npos + nneg = 0, 1, 7 (npos = 0), 255, 256, 257, 1000
                         around the 256-thread stride; GIoU, smooth-L1 beta 1/9 and 1.0, and beta 0 (array_equal to cddmsl_rpn_losses)
  test_box_reg_loss      R = 320, Kc = 5 at ld = 4 Kc (nfg = 0, 1, 255, 256, 257, 300), 4 Kc + 4 and 4 with cls null (nfg = 300); R = 1200
                         with nfg = 1000; the same four losses (beta 0: array_equal to cddmsl_box_l1)
  every case             the constructed rows first (exact match, shared edge, touching boxes, dw == scale_clamp, dw / dh above it, a
                         tiny box, gt inside the prediction); gradients outside the touched columns exactly +0; the forward
                         repeated and bit-equal; the classification half bit-equal to cddmsl_rpn_losses'
  test_argument_errors   loc_type not 0 / 1, beta < 0 and NaN, scale_clamp inf / NaN at loc_type 1, and the conditions the old pair
                         checks: CDDMSL_ERR_ARG with nothing written

Measured on one MI355X, worst |err| / bound over all cases (test_worst_ratio_table prints them; 73 tests in 11.5 s).  The GIoU
ratios are low because a running bound counts every rounding of the chain at its worst; the f32 emulation of the host test gives the
same figures (0.122 / 0.112), so they are the bound's, not slack fitted to the kernel.  The smooth-L1 gradient ratios are the
quadratic branch e / beta, dominated by the error of the target (exact_losses.deltas_ref):
  rpn_losses_reg giou loss 0.040                 rpn_losses_reg giou ddeltas 0.122
  rpn_losses_reg smooth_l1 beta 0.111 loss 0.086 rpn_losses_reg smooth_l1 beta 0.111 ddeltas 0.623
  rpn_losses_reg smooth_l1 beta 1 loss 0.121     rpn_losses_reg smooth_l1 beta 1 ddeltas 0.620
  box_reg_loss giou loss 0.048                   box_reg_loss giou ddeltas 0.112
  box_reg_loss smooth_l1 beta 0.111 loss 0.048   box_reg_loss smooth_l1 beta 0.111 ddeltas 0.737
  box_reg_loss smooth_l1 beta 1 loss 0.050       box_reg_loss smooth_l1 beta 1 ddeltas 0.738
  RPN.losses (kernel | torch): giou loss_loc 0.007 | 0.005, ddeltas 0.150 | 0.094; beta 0.111 loss_loc 0.018 | 0.002, ddeltas 0.517 |
    0.517; beta 1 loss_loc 0.020 | 0.002, ddeltas 0.528 | 0.528; dlogits 0.460 | 0.460; loss_cls 0.067 | 0.000
  box head losses (kernel | torch): giou loss 0.023 | 0.001, ddeltas 0.135 | 0.135; beta 0.111 loss 0.029 | 0.008, ddeltas 0.421 | 0.421;
    beta 1 loss 0.011 | 0.003, ddeltas 0.478 | 0.478
  (where the two columns agree, the worst element is one whose error is the f32 forward chain's, which both sides evaluate alike)
  oracle step with beta 1/9 (RPN) and 0.5 (box head): every loss within 1e-3, worst gradient 9.1e-4 of its tensor's max (5e-3 allowed)
"""
import os

import pytest
import torch

import exact_box_losses as B
import exact_losses as E
import test_gpu_losses_exact as T

pytestmark = pytest.mark.gpu

DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORST = {}
_L, _p, _dev, _Out, _ok, _stream = T._L, T._p, T._dev, T._Out, T._ok, T._stream
LOC = {"smooth_l1": 0, "giou": 1}


_bind = _L                                                      # (cddmsl_amd.hip declares the argument types when it loads the library)


class Gpu(T.Gpu):
    """exact_box_losses' implementation interface on the C-ABI: CPU tensors in, CPU tensors out"""

    def rpn_reg(self, logits, deltas, pos, neg, midx, gt, gt_off, anchors, A, w, inv_norm, loc, beta, clamp, gout=None):
        args = (_p(_dev(logits)), _p(_dev(deltas)), _p(_dev(pos)), pos.numel(), _p(_dev(neg)), neg.numel(), _p(_dev(midx)), _p(_dev(gt)),
                _p(_dev(gt_off)), _p(_dev(anchors)), A, *w, inv_norm, LOC[loc], beta, clamp)
        if gout is None:
            out = _Out(2)
            _ok(_bind().cddmsl_rpn_losses_reg(*args, out.ptr, None, None, None, _stream()))
            return out.get()
        dl, dd = _Out(logits.numel(), fill=0.0), _Out(logits.numel(), 4, fill=0.0)      # zero-filled by the caller: the contract
        _ok(_bind().cddmsl_rpn_losses_reg(*args, None, _p(_dev(gout)), dl.ptr, dd.ptr, _stream()))
        return dl.get(), dd.get()

    def box_reg(self, deltas, fg, cls, src, tgt, w, inv_norm, loc, beta, clamp, gout=None):
        R, ld = deltas.shape
        args = (_p(_dev(deltas)), ld, _p(_dev(fg)), fg.numel(), _p(_dev(cls)), _p(_dev(src)), _p(_dev(tgt)), *w, inv_norm, LOC[loc], beta, clamp)
        if gout is None:
            out = _Out(1)
            _ok(_bind().cddmsl_box_reg_loss(*args, out.ptr, None, None, _stream()))
            return out.get()
        dd = _Out(R, ld, fill=0.0)
        _ok(_bind().cddmsl_box_reg_loss(*args, None, _p(_dev(gout)), dd.ptr, _stream()))
        return dd.get()


def _note(rep, label=""):
    for k, v in rep.worst.items():
        WORST[k] = max(WORST.get(k, 0.0), v)
        print(f"{k} [{label}]: worst |err|/bound {v:.3g}")
    assert not rep.fail, "\n".join(rep.fail)


def _run(run, case):
    rep = E.Report()
    run(case, Gpu(), rep)
    torch.cuda.synchronize()
    T.LIVE.clear()
    _note(rep, E.tag(case))


def _cases(fn):
    return dict(argvalues=fn(), ids=[E.tag(c).replace(" ", ",") for c in fn()])


@pytest.mark.parametrize("case", **_cases(B.rpn_cases))
def test_rpn_losses_reg(case):
    _run(B.run_rpn_reg, case)


@pytest.mark.parametrize("case", **_cases(B.box_cases))
def test_box_reg_loss(case):
    _run(B.run_box_reg, case)


def test_argument_errors_write_nothing():
    L, st = _bind(), _stream()
    x = _dev(torch.randn(8, 16))
    lng = _dev(torch.zeros(8, dtype=torch.int64))
    o = [_Out(8, 16) for _ in range(3)]
    nan, inf = float("nan"), float("inf")

    def rpn(npos=1, A=4, loc=0, beta=0.0, clamp=4.0, out=o[0].ptr, gout=None, dl=None, dd=None):
        return L.cddmsl_rpn_losses_reg(_p(x), _p(x), _p(lng), npos, _p(lng), 1, _p(lng), _p(x), _p(lng), _p(x), A, 1.0, 1.0, 1.0, 1.0, 1.0,
                                       loc, beta, clamp, out, gout, dl, dd, st)

    def box(ld=4, nfg=1, loc=0, beta=0.0, clamp=4.0, out=o[0].ptr, gout=None, dd=None):
        return L.cddmsl_box_reg_loss(_p(x), ld, _p(lng), nfg, None, _p(x), _p(x), 1.0, 1.0, 1.0, 1.0, 1.0, loc, beta, clamp, out, gout, dd, st)

    calls = [
        lambda: rpn(loc=2), lambda: rpn(loc=-1), lambda: rpn(beta=-1.0), lambda: rpn(beta=nan), lambda: rpn(loc=1, beta=nan),
        lambda: rpn(loc=1, clamp=inf), lambda: rpn(loc=1, clamp=-inf), lambda: rpn(loc=1, clamp=nan),
        lambda: rpn(out=None), lambda: rpn(out=None, gout=_p(x), dl=o[1].ptr, dd=None), lambda: rpn(out=None, gout=_p(x), dl=None, dd=o[2].ptr),
        lambda: rpn(npos=-1), lambda: rpn(A=0),
        lambda: box(loc=2), lambda: box(loc=-1), lambda: box(beta=-0.5), lambda: box(beta=nan), lambda: box(loc=1, clamp=inf),
        lambda: box(loc=1, clamp=nan), lambda: box(ld=3), lambda: box(nfg=-1), lambda: box(out=None), lambda: box(out=None, gout=_p(x), dd=None),
    ]
    for i, call in enumerate(calls):
        assert call() == 1, f"call {i}"
    for b in o:
        b.get(written=False)
    T.LIVE.clear()


# ================================================================================================== the model level
def _model(opts):
    from cddmsl_amd.config import get_cfg
    from cddmsl_amd.modeling import build_model
    cfg = get_cfg()
    cfg.merge_from_file(os.path.join(ROOT, "configs", "VOC-Experiments", "faster_rcnn_CLIP_R_50_C4.yaml"))
    cfg.merge_from_list(list(opts) + ["MODEL.COMPUTE_DTYPE", "f32", "MODEL.DEVICE", "cuda:0"])
    return build_model(cfg)


MODEL_LOSSES = [("giou", 0.0), ("smooth_l1", 1.0 / 9), ("smooth_l1", 1.0)]


@pytest.mark.parametrize("loc,beta", MODEL_LOSSES, ids=["giou", "beta0.111", "beta1"])
def test_rpn_losses_kernel_branch_against_torch_branch(loc, beta):
    """RPN.losses with MODEL.RPN.BBOX_REG_LOSS_TYPE / SMOOTH_L1_BETA set: the kernel branch and the torch branch (the one taken when
    the sampled index lists are not at hand) on the same device tensors.  Both must lie inside the bounds around the float64
    reference (the torch branch sums in torch's order: depth = the row count), losses and the gradients of logits and deltas.
    N = 2 images: the normaliser 256 N is a power of two, so dividing by it (torch) and multiplying by its inverse (kernel) agree"""
    rpn = _model(["MODEL.RPN.BBOX_REG_LOSS_TYPE", loc, "MODEL.RPN.SMOOTH_L1_BETA", beta]).proposal_generator
    N, A, npos, nneg = 2, 300, 90, 160
    g = E._g(501)
    w = rpn.weights
    anchors = E._boxes(A, 502)
    gts = [E._boxes(3, 503), E._boxes(2, 504)]
    midx = torch.stack([torch.randint(0, 3, (A,), generator=g), torch.randint(0, 2, (A,), generator=g)])
    perm = torch.randperm(N * A, generator=g)
    pos, neg = perm[:npos], perm[npos:npos + nneg]
    labels = torch.full((N * A,), -1, dtype=torch.int8)
    labels[pos], labels[neg] = 1, 0
    logits = E._randn((N, A), 505, 3.0)
    deltas = B._deltas(N * A, w, 506).view(N, A, 4)
    if loc == "smooth_l1":
        img = torch.div(pos, A, rounding_mode="floor")
        gt_cat = torch.cat(gts)
        tg = B._f32_get_deltas(anchors[pos - img * A], gt_cat[midx.view(-1)[pos] + 3 * img], w)
        deltas.view(-1, 4)[pos[::3]] = (tg + E._randn(tuple(tg.shape), 507, 0.05))[::3]
    a = dict(logits=logits.view(-1), deltas=deltas.view(-1, 4), pos=pos, neg=neg, midx=midx.view(-1), gt=torch.cat(gts),
             gt_off=torch.tensor([0, 3]), anchors=anchors, A=A, w=w, inv_norm=1.0 / (rpn.batch_size_per_image * N))
    gout = torch.tensor([1.5, 0.7])
    got = {}
    for branch in ("kernel", "torch"):
        rpn.last_pos_global = pos.to(DEV)
        rpn.last_neg_global = neg.to(DEV) if branch == "kernel" else None
        lg, dl = logits.to(DEV).requires_grad_(True), deltas.to(DEV).requires_grad_(True)
        out = rpn.losses(anchors.to(DEV), lg, labels.view(N, A).to(DEV), dl, (midx.to(DEV), [t.to(DEV) for t in gts]))
        (gout[0] * out["loss_rpn_cls"] + gout[1] * out["loss_rpn_loc"]).backward()
        got[branch] = (torch.stack([out["loss_rpn_cls"], out["loss_rpn_loc"]]).detach().cpu(), lg.grad.cpu().view(-1), dl.grad.cpu().view(-1, 4))
    c = dict(loc=loc, beta=beta)
    for branch, (out2, dlg, dd) in got.items():
        rep = E.Report()
        depth = None if branch == "kernel" else npos + nneg
        name = f"RPN.losses {loc}" + (f" beta {beta:.3g}" if loc == "smooth_l1" else "") + f" ({branch})"
        cls_ref = E.rpn_ref(**a)["out2"]
        if branch == "torch":                                           # the dense BCE sums N A terms (the unsampled ones are exact zeros)
            cls_ref = (cls_ref[0], cls_ref[1] + E.S2 * E.U * (N * A) * cls_ref[0].abs())
        rep.bound(name + " loss_cls", branch, out2[:1], (cls_ref[0][:1], cls_ref[1][:1]))
        rep.bound(name + " loss_loc", branch, out2[1:], tuple(x.reshape(1) for x in B.rpn_reg_ref(a, loc, beta, B.SCALE_CLAMP, depth=depth)))
        rep.bound(name + " dlogits", branch, dlg, E.rpn_ref(**a, gout=gout)["dlogits"])
        isp = torch.zeros(N * A, dtype=torch.bool)
        isp[pos] = True
        rep.exact(name + " ddeltas", branch, bool((dd[~isp] == 0).all()), "a gradient outside the positives")
        B._loc_checks(rep, name + " ddeltas", branch, dd[pos], B.rpn_reg_ref(a, loc, beta, B.SCALE_CLAMP, gout=gout), c, 0)
        _note(rep, branch)


@pytest.mark.parametrize("loc,beta", MODEL_LOSSES, ids=["giou", "beta0.111", "beta1"])
def test_box_head_losses_kernel_branch_against_torch_formulation(loc, beta):
    """FastRCNNOutputLayers.losses with MODEL.ROI_BOX_HEAD.BBOX_REG_LOSS_TYPE / SMOOTH_L1_BETA set (the kernel branch) and
    box_reg_loss_terms, the torch formulation its other branch calls, on the same device tensors: both inside the bounds around
    the float64 reference.  R = 128 rows: the normaliser is a power of two"""
    from cddmsl_amd.modeling.rpn import box_reg_loss_terms
    from cddmsl_amd.structures import Boxes, Instances
    head = _model(["MODEL.ROI_BOX_HEAD.BBOX_REG_LOSS_TYPE", loc, "MODEL.ROI_BOX_HEAD.SMOOTH_L1_BETA", beta]).roi_heads.box_predictor
    K, R = head.num_classes, 128
    w = head.box_weights
    g = E._g(511)
    cls = torch.randint(0, K, (R,), generator=g)
    cls[torch.rand(R, generator=g) < 0.4] = K
    fg = torch.nonzero(cls < K)[:, 0]
    src, tgt = E._boxes(R, 512), E._boxes(R, 513)
    deltas = E._randn((R, 4 * K), 514)
    own = B._deltas(R, w, 515)
    if loc == "smooth_l1":
        own[::3] = (B._f32_get_deltas(src, tgt, w) + E._randn((R, 4), 516, 0.05))[::3]
    cols = 4 * cls[fg][:, None] + torch.arange(4)[None, :]
    deltas[fg[:, None], cols] = own[fg]
    scores = E._randn((R, K + 1), 517)
    a = dict(deltas=deltas, fg=fg, cls=cls.clamp(max=K - 1), src=src, tgt=tgt, w=w, inv_norm=1.0 / R)
    gout = torch.tensor([0.7])
    halves = [slice(0, R // 2), slice(R // 2, R)]
    props = []
    for h in halves:
        p = Instances((480, 640))
        p.proposal_boxes, p.gt_boxes, p.gt_classes = Boxes(src[h].to(DEV)), Boxes(tgt[h].to(DEV)), cls[h].to(DEV)
        props.append(p)
    d1 = deltas.to(DEV).requires_grad_(True)
    out = head.losses((scores.to(DEV), d1), props)
    (gout[0] * out["loss_box_reg"]).backward()
    d2 = deltas.to(DEV).requires_grad_(True)
    fgd = fg.to(DEV)
    lt = box_reg_loss_terms(d2.view(-1, K, 4)[fgd, cls.to(DEV)[fgd]], src.to(DEV)[fgd], tgt.to(DEV)[fgd], w, loc, beta) / max(R, 1.0)
    (gout[0] * lt).backward()
    c = dict(loc=loc, beta=beta)
    for branch, loss, grad in (("kernel", out["loss_box_reg"], d1.grad), ("torch", lt, d2.grad)):
        rep = E.Report()
        name = f"box head losses {loc}" + (f" beta {beta:.3g}" if loc == "smooth_l1" else "") + f" ({branch})"
        depth = None if branch == "kernel" else fg.numel()
        rep.bound(name + " loss", branch, loss.detach().cpu().reshape(1),
                  tuple(x.reshape(1) for x in B.box_reg_ref(a, loc, beta, B.SCALE_CLAMP, depth=depth)))
        dd = grad.cpu()
        touched = torch.zeros(deltas.shape, dtype=torch.bool)
        touched[fg[:, None], cols] = True
        rep.exact(name + " ddeltas", branch, bool((dd[~touched] == 0).all()), "a gradient outside the foreground rows' class columns")
        B._loc_checks(rep, name + " ddeltas", branch, dd[fg[:, None], cols], B.box_reg_ref(a, loc, beta, B.SCALE_CLAMP, gout=gout), c, 0)
        _note(rep, branch)


def test_step_with_smooth_l1_beta_matches_oracle():
    """one reduced-size f32 training step with MODEL.RPN.SMOOTH_L1_BETA = 1/9 and MODEL.ROI_BOX_HEAD.SMOOTH_L1_BETA = 0.5 against the
    oracle with rpn_smooth_l1_beta / roi_smooth_l1_beta set: the shape and the tolerances of
    test_gpu_e2e.test_step_losses_and_grads_match_oracle (losses 1e-3, gradients 5e-3 of each tensor's max)"""
    import test_gpu_e2e as G
    from cddmsl_amd import synthetic
    from cddmsl_amd.engine import SimpleTrainer
    from cddmsl_amd.solver import build_optimizer
    from oracle import model as om
    torch.set_num_threads(min(32, os.cpu_count() or 8))
    rb, hb = 1.0 / 9, 0.5
    cfg = G._cfg("f32")
    cfg.merge_from_list(["MODEL.RPN.SMOOTH_L1_BETA", rb, "MODEL.ROI_BOX_HEAD.SMOOTH_L1_BETA", hb])
    model, mapper, sd, msd = G._build(cfg, seed=5)
    assert model.proposal_generator.smooth_l1_beta == rb and model.roi_heads.box_predictor.smooth_l1_beta == hb
    batch = synthetic.make_batch(2, 160, 224, num_gt=3)
    tr = SimpleTrainer(model, iter([batch]), build_optimizer(cfg, model), cfg, clipcap_model=mapper, metrics_period=0)
    tr.iter = 20000
    tr.buckets.zero()
    ld = tr.compute_losses(batch)
    sum(ld.values()).backward()
    got = {k: float(v.detach()) for k, v in ld.items()}
    ocfg = G._oracle_cfg(cfg, False)
    ocfg.rpn_smooth_l1_beta, ocfg.roi_smooth_l1_beta = rb, hb
    keys = om.trainable_keys(sd, ocfg)
    for k in keys:
        sd[k].requires_grad_(True)
    ref = om.run_step_losses(sd, msd, ocfg, batch, 20000, torch.Generator().manual_seed(5))
    sum(ref.values()).backward()
    want = {k: float(v.detach()) for k, v in ref.items()}
    assert set(got) == set(want)
    for k in want:
        assert abs(got[k] - want[k]) <= 1e-3 * abs(want[k]) + 1e-6, (k, got[k], want[k])
    params = dict(model.named_parameters())
    worst = 0.0
    for k in keys:
        gk, r = params[k].grad.detach().float().cpu(), sd[k].grad
        err = float((gk - r).abs().max() / max(float(r.abs().max()), 1e-5))
        worst = max(worst, err)
        assert err < 5e-3, (k, err)
    print("losses", got, "worst grad rel err", worst)


def test_worst_ratio_table(capsys):
    """the module's last test: the worst |err| / bound of every output the tests before it checked, one line each; every ratio is at
    most 1"""
    lines = ["", "worst |err| / bound per output:"] + [f"  {k:56s} {WORST[k]:.3f}" for k in sorted(WORST)]
    with capsys.disabled():
        print("\n".join(lines))
    assert all(v <= 1.0 for v in WORST.values())
