"""cddmsl_sgd_step_groups (k_gnorm / k_sgd_groups of cddmsl_amd/csrc/elementwise.hip) against the float64 reference of
tests/exact_solver.py, called through the C-ABI at the case list the host test shares (tests/test_solver_host.py runs the same
driver on an f32 emulation and on its mutants), and one training step end to end through ClippedSGD.

The case that reaches each branch:
  k_sgd_groups<0 / 1 / 2>   clip mode none / value / the three norms; per-tensor lr and weight decay (some 0); Nesterov on and off,
                            momentum 0.9 and 0; first_step 1 on a NaN momentum, then two more steps; the vector path and the scalar
                            path for each of p, g, m one to three elements off 16-byte alignment; the n % 4 tail; NaN between tensors
  k_gnorm<L2 / L1 / INF>    its vector path and its scalar path (g misaligned); norm_ws pre-filled, entries past count untouched;
                            modes none / value leave norm_ws untouched altogether; the inf norm bit for bit
  batches                   count = 1, 4, B, B + 1, 2 B + 1 for B = 80 tensors per launch; four tensors of about 2^20 elements
                            (n % 4 = 3, 2, 1, 0), one per alignment pattern, so every grid-stride loop wraps
  clipping                  gradient norms 300, 7 and 2 times the clip, 0.3 times, and zero: coefficient below 1 and clamped to 1;
                            value clamp on both sides, inside it, and on a zero gradient
  NaN                       one NaN gradient element under the inf norm and under the L1 norm: norm_ws, p and buf of that tensor are
                            NaN, its neighbours pass their bounds

Measured on one MI355X, worst |err| / bound over all cases (the inf norm, the value clamp and every guard element are checked bit
for bit and have no ratio):
  sgd_step_groups m 0.988           sgd_step_groups p 0.990           sgd_step_groups norm_ws l1 0.119
  sgd_step_groups norm_ws l2 0.113  trainer step m 0.989              trainer step p 0.990
(0.99 is a correctly rounded store of a value just above a power of two: half an ulp is u |value| there.  The two norm sums are
bounded at the depth of the longest chain of additions a lane, a wave, a block and the atomics can form, which random signs do not
reach; cddmsl_sgd_clip_step's norm_ws sits at 0.119 under the same bound.)"""
import ctypes
import os

import pytest
import torch

import exact_solver as S

pytestmark = pytest.mark.gpu

DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORST = {}


def _L():
    from cddmsl_amd import hip
    return hip._L()


def _stream():
    from cddmsl_amd import hip
    return hip.stream_ptr()


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


class Gpu:
    """exact_solver's implementation interface on the C-ABI: CPU tensors in, CPU tensors out"""

    def sgd_groups(self, lay, p, g, m, ws, lrs, wds, mo, nesterov, mode, clip, first):
        pd, gd, md, wsd = p.to(DEV), g.to(DEV), m.to(DEV), ws.to(DEV)
        n = len(lay)
        at = lambda buf, k: (ctypes.c_void_p * n)(*[buf.data_ptr() + 4 * l[k] for l in lay])
        sizes = (ctypes.c_long * n)(*[l[0] for l in lay])
        status = _L().cddmsl_sgd_step_groups(at(pd, 1), at(gd, 2), at(md, 3), sizes, (ctypes.c_float * n)(*lrs), (ctypes.c_float * n)(*wds),
                                             n, _p(wsd), mo, int(nesterov), mode, clip, int(first), _stream())
        assert status == 0, f"status {status}"
        torch.cuda.synchronize()
        assert S.bits_equal(gd.cpu(), g), "the gradient buffer was written"
        return pd.cpu(), md.cpu(), wsd.cpu()


_CASES = S.groups_cases()


@pytest.mark.parametrize("case", _CASES, ids=[S.groups_tag(c).replace(" ", ",") for c in _CASES])
def test_sgd_step_groups(case):
    rep = S.Report()
    S.run_groups(case, Gpu(), rep)
    for k, v in rep.worst.items():
        WORST[k] = max(WORST.get(k, 0.0), v)
        print(f"{k} [{S.groups_tag(case)}]: worst |err|/bound {v:.3g}")
    assert not rep.fail, "\n".join(rep.fail[:20])


def test_argument_errors_and_empty_launch_write_nothing():
    """the returns before any launch: CDDMSL_ERR_ARG (1) for count < 0, a clip mode outside 0..4, nesterov outside {0, 1}; 0 for count == 0"""
    L, st = _L(), _stream()
    bufs = [torch.full((24,), float("nan"), device=DEV) for _ in range(4)]
    before = [b.clone() for b in bufs]
    one = lambda b: (ctypes.c_void_p * 1)(b.data_ptr() + 16)
    sizes, lrs, wds = (ctypes.c_long * 1)(8), (ctypes.c_float * 1)(0.1), (ctypes.c_float * 1)(1e-4)
    call = lambda count, nest, mode: L.cddmsl_sgd_step_groups(one(bufs[0]), one(bufs[1]), one(bufs[2]), sizes, lrs, wds, count, _p(bufs[3]),
                                                             0.9, nest, mode, 1.0, 1, st)
    assert call(-1, 0, 2) == 1 and call(1, 0, 5) == 1 and call(1, 0, -1) == 1 and call(1, 2, 0) == 1 and call(1, -1, 0) == 1
    for mode in range(5):
        assert call(0, 1, mode) == 0
    assert L.cddmsl_sgd_step_groups(None, None, None, None, None, None, 0, _p(bufs[3]), 0.9, 0, 4, 1.0, 0, st) == 0
    torch.cuda.synchronize()
    assert all(S.bits_equal(a.cpu(), b.cpu()) for a, b in zip(bufs, before))


def test_wrapper_refusals():
    """hip.sgd_step_groups passes raw pointers: it refuses what sgd_clip_step refuses, and lr / weight-decay lists of another length"""
    from cddmsl_amd import hip
    from cddmsl_amd._lib import HipLibraryError
    sq = torch.randn(8, 8, device=DEV)
    ws = torch.zeros(2, device=DEV)
    ok = dict(params=[sq.clone(), sq.clone()], grads=[sq, sq], moms=[sq.clone(), sq.clone()], norm_ws=ws, lrs=[0.1, 0.2], wds=[0.0, 1e-4],
              momentum=0.9, nesterov=True, clip_mode=hip.SGD_CLIP_MODES["inf"], clip_value=1.0, first_step=True)
    bad = [dict(lrs=[0.1]), dict(wds=[0.0, 0.0, 0.0]), dict(norm_ws=torch.zeros(1, device=DEV)), dict(norm_ws=torch.zeros(4, device=DEV)[::2]),
           dict(norm_ws=torch.zeros(2, device=DEV, dtype=torch.float64)), dict(grads=[sq, sq.t()]), dict(moms=[sq.clone(), sq.clone().t()]),
           dict(grads=[sq]), dict(moms=[sq.clone()]), dict(params=[sq.clone(), sq.clone().bfloat16()]), dict(grads=[sq, sq.double()])]
    for change in bad:
        with pytest.raises(AssertionError):
            hip.sgd_step_groups(**dict(ok, **change))
    with pytest.raises(HipLibraryError):
        hip.sgd_step_groups(**dict(ok, grads=[sq, sq.cpu()]))
    with pytest.raises(HipLibraryError):                           # the library's own CDDMSL_ERR_ARG
        hip.sgd_step_groups(**dict(ok, clip_mode=7))
    p0 = ok["params"][0].clone()
    hip.sgd_step_groups(**ok)
    hip.sgd_step_groups([], [], [], ws, [], [], 0.9, False, 0, 1.0, True)
    torch.cuda.synchronize()
    assert float(ws[0]) == float(sq.abs().max()) and not torch.equal(ok["params"][0], p0)


def test_trainer_steps_with_reference_solver_options():
    """two SimpleTrainer steps of the tiny synthetic model with NESTEROV, BIAS_LR_FACTOR 2, WEIGHT_DECAY_BIAS 0 and value clipping,
    against torch.optim.SGD in float64 fed the gradients the steps produced, with the bound of exact_solver.groups_ref (whose
    reference is chained through both steps and compared with torch's result as well)"""
    from cddmsl_amd import hip, synthetic
    from cddmsl_amd.config import get_cfg
    from cddmsl_amd.engine import SimpleTrainer
    from cddmsl_amd.modeling import TransformerMapper, build_model
    from cddmsl_amd.solver import build_optimizer, lr_multiplier
    cfg = get_cfg()
    cfg.merge_from_file(os.path.join(ROOT, "configs", "VOC-Experiments", "faster_rcnn_CLIP_R_50_C4.yaml"))
    cfg.merge_from_list(["MODEL.COMPUTE_DTYPE", "f32", "MODEL.ROI_HEADS.BATCH_SIZE_PER_IMAGE", 16, "MODEL.RPN.PRE_NMS_TOPK_TRAIN", 300,
                         "MODEL.RPN.POST_NMS_TOPK_TRAIN", 100, "SOLVER.NESTEROV", True, "SOLVER.BIAS_LR_FACTOR", 2.0,
                         "SOLVER.WEIGHT_DECAY_BIAS", 0.0, "SOLVER.CLIP_GRADIENTS.ENABLED", True, "SOLVER.CLIP_GRADIENTS.CLIP_TYPE", "value",
                         "SOLVER.CLIP_GRADIENTS.CLIP_VALUE", 1e-3])
    model = build_model(cfg)
    model.load_state_dict(synthetic.make_state_dict(0), strict=False)
    mapper = TransformerMapper(compute_dtype=model.compute_dtype)
    mapper.load_state_dict(synthetic.make_mapper_state_dict(1))
    mapper.to(model.device)
    g = torch.Generator().manual_seed(3)
    model.proposal_generator.sample_generator = model.roi_heads.sample_generator = model.region_generator = g
    batch = synthetic.make_batch(1, 128, 160, num_gt=2)
    opt = build_optimizer(cfg, model)
    assert not opt.uniform
    names = {p.data_ptr(): k for k, p in model.named_parameters()}
    record = []                                                   # per step: what the grouped entry point was given, copied before it runs
    inner = hip.sgd_step_groups

    def recording(params, grads, moms, norm_ws, lrs, wds, *rest):
        record.append(dict(p=[p.detach().cpu().clone() for p in params], g=[x.detach().cpu().clone() for x in grads],
                           m=[x.detach().cpu().clone() for x in moms], lrs=list(lrs), wds=list(wds), rest=rest, live=list(params), moms=list(moms)))
        inner(params, grads, moms, norm_ws, lrs, wds, *rest)
        torch.cuda.synchronize()
        record[-1]["p2"] = [p.detach().cpu().clone() for p in params]
        record[-1]["m2"] = [x.detach().cpu().clone() for x in moms]

    hip.sgd_step_groups = recording
    try:
        tr = SimpleTrainer(model, iter([batch, batch]), opt, cfg, clipcap_model=mapper, metrics_period=0)
        tr.iter = opt.iteration = 20000
        tr.run_step()
        tr.run_step()
    finally:
        hip.sgd_step_groups = inner
    assert len(record) == 2
    s = cfg.SOLVER
    for step, r in enumerate(record):
        mo, nest, mode, clip, first = r["rest"]
        assert (mo, nest, mode, clip, bool(first)) == (s.MOMENTUM, True, hip.SGD_CLIP_MODES["value"], 1e-3, step == 0)
        mult = lr_multiplier(cfg, 20000 + step)
        bias = [names[p.data_ptr()].endswith(".bias") for p in r["live"]]
        assert any(bias) and not all(bias)
        assert r["lrs"] == [s.BASE_LR * (2.0 if b else 1.0) * mult for b in bias] and r["wds"] == [0.0 if b else s.WEIGHT_DECAY for b in bias]
        assert any(bool((x.abs() > clip).any()) for x in r["g"]) and any(bool(((x.abs() < clip) & (x != 0)).any()) for x in r["g"])
    assert [p.data_ptr() for p in record[0]["live"]] == [p.data_ptr() for p in record[1]["live"]]
    # torch.optim.SGD in float64 on the recorded gradients (f32 scalars, as the kernel gets them)
    r0 = record[0]
    qs = [torch.nn.Parameter(p.double().reshape(-1).clone()) for p in r0["p"]]
    ref_opt = torch.optim.SGD([{"params": [q], "weight_decay": S.f32(wd)} for q, wd in zip(qs, r0["wds"])], lr=1.0, momentum=S.f32(s.MOMENTUM),
                              nesterov=True)
    rep = S.Report()
    for step, r in enumerate(record):
        for grp, lr in zip(ref_opt.param_groups, r["lrs"]):
            grp["lr"] = S.f32(lr)
        for q, x in zip(qs, r["g"]):
            q.grad = x.double().reshape(-1).clone()
            torch.nn.utils.clip_grad_value_(q, S.f32(1e-3))
        flat = lambda ts: [t.reshape(-1) for t in ts]
        if step == 1:                                             # the second step starts from what the first one left, bit for bit
            assert all(S.bits_equal(a, b) for a, b in zip(r["p"], record[0]["p2"])) and all(S.bits_equal(a, b) for a, b in zip(r["m"], record[0]["m2"]))
            for q, p in zip(qs, r["p"]):                          # each step is judged from the operands the kernel was given
                q.data.copy_(p.double().reshape(-1))
            for q, m in zip(qs, r["m"]):
                ref_opt.state[q]["momentum_buffer"].copy_(m.double().reshape(-1))
        ref_opt.step()
        ref = S.groups_ref(flat(r["p"]), flat(r["g"]), flat(r["m"]), r["lrs"], r["wds"], s.MOMENTUM, 1, S.VALUE, 1e-3, step == 0)
        for i, q in enumerate(qs):
            assert torch.allclose(q.detach(), ref[i]["p"][0], rtol=1e-12, atol=1e-300)
            assert torch.allclose(ref_opt.state[q]["momentum_buffer"], ref[i]["m"][0], rtol=1e-12, atol=1e-300)
        for k, got in (("p", r["p2"]), ("m", r["m2"])):
            rep.bound(f"trainer step {k}", f"step {step + 1}", torch.cat(flat(got)), (torch.cat([x[k][0] for x in ref]), torch.cat([x[k][1] for x in ref])))
    for k, v in rep.worst.items():
        WORST[k] = max(WORST.get(k, 0.0), v)
    assert not rep.fail, "\n".join(rep.fail)


def test_worst_ratio_table(capsys):
    """the module's last test: the worst |err| / bound of every output the tests before it checked (shown without -s)"""
    with capsys.disabled():
        print("\n".join(["", "worst |err| / bound per output:"] + [f"  {k:44s} {WORST[k]:.3f}" for k in sorted(WORST)]))
    assert all(v <= 1.0 for v in WORST.values())
