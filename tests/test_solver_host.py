"""The solver without a GPU (tests/exact_solver.py holds the cases, the float64 reference and its bounds):
  a. groups_ref equals torch.optim.SGD(per-parameter groups, momentum, nesterov) after clip_grad_value_ / clip_grad_norm_ per
     parameter, in float64, over three steps; torch's own NaN convention under the inf norm
  b. an f32 emulation of cddmsl_sgd_step_groups stays within the bounds at the whole case list, and each mutant of it is rejected
  c. get_default_optimizer_params: the reference's groups, its two ValueErrors, model.parameters() order
  d. schedule known answers (the reference's tests/test_scheduler.py:14-68) and the two ValueErrors
  e. construction errors of ClippedSGD
  f. the dispatch rule: which entry point a configuration calls, and with which arguments
  g. state_dict / load_state_dict round trip with unchanged keys"""
import math
import os

import pytest
import torch
from torch import nn

import exact_solver as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
YAMLS = ("PascalVOC-Detection/faster_rcnn_R_50_C4.yaml", "VOC-Experiments/faster_rcnn_CLIP_R_50_C4.yaml",
         "AdverseWeather-Experiments/faster_rcnn_CLIP_R_50_C4.yaml")


def _t32(v):
    return torch.tensor(float(v), dtype=torch.float32)


# ================================================================================================== a. reference = torch float64
@pytest.mark.parametrize("mode", range(5), ids=S.NAMES)
@pytest.mark.parametrize("mo,nest", S.COMBOS)
def test_reference_equals_torch_sgd_float64(mode, mo, nest):
    c = dict(mode=mode, count=9, big=False, nan=False)
    lay, total = S.sgd_layout(c)
    p, g = S.groups_buffers(c, lay, total)
    gs = [v.double() for v in S.sgd_views(g, lay, 2)]
    qs = [nn.Parameter(v.double().clone()) for v in S.sgd_views(p, lay, 1)]
    _, wds = S.groups_scalars(c, 0)
    opt = torch.optim.SGD([{"params": [q], "weight_decay": wd} for q, wd in zip(qs, wds)], lr=1.0, momentum=mo, nesterov=bool(nest))
    cur_p, cur_m = [q.detach().clone() for q in qs], [torch.zeros_like(q) for q in qs]
    for step in range(3):
        lrs, _ = S.groups_scalars(c, step)
        for grp, lr in zip(opt.param_groups, lrs):
            grp["lr"] = lr
        for q, gi in zip(qs, gs):
            q.grad = gi.clone()
            if mode == S.VALUE:
                nn.utils.clip_grad_value_(q, S.CLIP)
            elif mode >= S.L2:
                nn.utils.clip_grad_norm_(q, S.CLIP, {S.L2: 2.0, S.L1: 1.0, S.INF: float("inf")}[mode])
        opt.step()
        ref = S.groups_ref(cur_p, gs, cur_m, lrs, wds, mo, nest, mode, S.CLIP, step == 0, exact_scalars=True)
        for i, q in enumerate(qs):
            assert torch.allclose(q.detach(), ref[i]["p"][0], rtol=1e-12, atol=1e-300), (step, i)
            if mo:
                assert torch.allclose(opt.state[q]["momentum_buffer"], ref[i]["m"][0], rtol=1e-12, atol=1e-300), (step, i)
        cur_p, cur_m = [r["p"][0] for r in ref], [r["m"][0] for r in ref]


def test_torch_keeps_a_nan_gradient_under_every_norm():
    """the convention the kernels follow: one NaN element makes the tensor's norm, coefficient and clipped gradient NaN"""
    for nt in (1.0, 2.0, float("inf")):
        q = nn.Parameter(torch.zeros(5, dtype=torch.float64))
        q.grad = torch.tensor([1.0, -3.0, float("nan"), 0.5, 0.0], dtype=torch.float64)
        assert torch.isnan(nn.utils.clip_grad_norm_(q, 1.0, nt)) and bool(torch.isnan(q.grad).all())
    q.grad = torch.tensor([1.0, -3.0, float("nan"), 0.5, 0.0], dtype=torch.float64)
    nn.utils.clip_grad_value_(q, 1.0)
    assert torch.isnan(q.grad).tolist() == [False, False, True, False, False] and q.grad[1] == -1.0


# ================================================================================================== b. emulation and mutants
class Emu:
    """cddmsl_sgd_step_groups in f32 torch operations on the CPU; ``mut`` names one deliberate mistake"""

    def __init__(self, mut=None):
        self.mut = mut

    def sgd_groups(self, lay, p, g, m, ws, lrs, wds, mo, nesterov, mode, clip, first):
        mut = self.mut
        p2, m2, ws2 = p.clone(), m.clone(), ws.clone()
        mo, clip = _t32(mo), _t32(clip)
        for i, (n, op, og, om) in enumerate(lay):
            pi, gi, mi = p[op:op + n], g[og:og + n], m[om:om + n]
            lr, wd = _t32(lrs[0 if mut == "lr_of_tensor0" else i]), _t32(wds[0 if mut == "wd_of_tensor0" else i])
            if mode >= S.L2:
                a = gi.abs()
                if mode == S.L2:
                    s = (gi * gi).sum()
                elif mode == S.L1:
                    s = (gi if mut == "l1_no_abs" else a).sum()
                elif mut == "inf_as_sum":
                    s = a.sum()
                elif mut == "inf_drops_nan":                      # fmaxf returns the operand that is a number
                    s = a[~torch.isnan(a)].max() if bool((~torch.isnan(a)).any()) else _t32(0.0)
                else:
                    s = a.max()
                ws2[i] = s
                nrm = torch.sqrt(s) if mode == S.L2 else s
                coef = clip / (nrm if mut == "no_eps" else nrm + _t32(1e-6))
                if mut != "coef_unclamped":
                    coef = torch.clamp(coef, max=1.0)
                gc = gi * coef
            elif mode == S.VALUE and mut != "clamp_after_wd":
                gc = torch.clamp(gi, max=clip) if mut == "clamp_one_sided" else torch.clamp(gi, -clip, clip)
            else:
                gc = gi
            d = gc + wd * pi
            if mode == S.VALUE and mut == "clamp_after_wd":
                d = torch.clamp(d, -clip, clip)
            buf = d if first else mo * mi + d
            ahead = nesterov and mut != "nesterov_ignored" and not (first and mut == "nesterov_dropped_on_first_step")
            m2[om:om + n] = buf
            p2[op:op + n] = pi - lr * (d + mo * buf if ahead else buf)
        return p2, m2, ws2


def _run_all(impl, keep=lambda c: True):
    rep = S.Report()
    for c in S.groups_cases():
        if keep(c):
            S.run_groups(c, impl, rep)
    return rep


def test_emulation_stays_within_the_bounds(capsys):
    rep = _run_all(Emu())
    with capsys.disabled():
        print("\n" + "\n".join(f"  {k:44s} {v:.3f}" for k, v in sorted(rep.worst.items())))
    assert not rep.fail, "\n".join(rep.fail[:20])


_small = lambda c: not c["big"]
MUTANTS = (
    ("Nesterov ignored", "nesterov_ignored", lambda c: _small(c) and c["nesterov"]),
    ("Nesterov's look-ahead dropped on the first step", "nesterov_dropped_on_first_step", lambda c: _small(c) and c["nesterov"]),
    ("lr taken from tensor 0", "lr_of_tensor0", _small),
    ("weight decay taken from tensor 0", "wd_of_tensor0", _small),
    ("value clamp after the weight-decay add", "clamp_after_wd", lambda c: _small(c) and c["mode"] == S.VALUE),
    ("one-sided value clamp", "clamp_one_sided", lambda c: _small(c) and c["mode"] == S.VALUE),
    ("L1 norm without abs", "l1_no_abs", lambda c: _small(c) and c["mode"] == S.L1),
    ("inf norm as a sum", "inf_as_sum", lambda c: _small(c) and c["mode"] == S.INF),
    ("coefficient not clamped to 1", "coef_unclamped", lambda c: _small(c) and c["mode"] >= S.L2),
    ("1e-6 missing in the coefficient", "no_eps", lambda c: _small(c) and c["mode"] >= S.L2),
    ("inf-norm max that drops a NaN", "inf_drops_nan", lambda c: _small(c) and c["mode"] == S.INF),
)


@pytest.mark.parametrize("name,key,keep", MUTANTS, ids=[m[1] for m in MUTANTS])
def test_mutant_is_rejected(name, key, keep):
    assert not _run_all(Emu(), keep).fail, "the plain emulation fails at the mutant's cases"
    rep = _run_all(Emu(key), keep)
    assert rep.rejected, f"{name}: accepted at every case"


# ================================================================================================== c. parameter groups
class Toy(nn.Module):
    def __init__(self, norm=True):
        super().__init__()
        self.frozen = nn.Parameter(torch.zeros(2), requires_grad=False)
        self.embedding = nn.Parameter(torch.zeros(5))
        self.fc = nn.Linear(4, 3)
        self.norm = nn.LayerNorm(3) if norm else nn.Identity()
        self.head = nn.Linear(3, 3, bias=False)
        self.tied = nn.Linear(3, 3, bias=False)
        self.tied.weight = self.head.weight                      # one parameter in two modules


def _groups(model, **kw):
    from cddmsl_amd.solver import get_default_optimizer_params
    return get_default_optimizer_params(model, **kw)


def test_default_optimizer_params_follow_the_reference_rules():
    m = Toy()
    gs = _groups(m, base_lr=0.1, weight_decay=1e-4, weight_decay_norm=0.0, bias_lr_factor=2.0, weight_decay_bias=5e-4)
    want = [(m.embedding, 0.1, 1e-4), (m.fc.weight, 0.1, 1e-4), (m.fc.bias, 0.2, 5e-4), (m.norm.weight, 0.1, 0.0),
            (m.norm.bias, 0.2, 5e-4), (m.head.weight, 0.1, 1e-4)]
    assert len(gs) == len(want)
    for grp, (p, lr, wd) in zip(gs, want):
        assert set(grp) == {"params", "lr", "weight_decay"} and len(grp["params"]) == 1 and grp["params"][0] is p
        assert grp["lr"] == lr and grp["weight_decay"] == wd
    # the order is model.parameters() without the frozen one: the checkpoint's momentum_buffers list depends on it
    assert [id(grp["params"][0]) for grp in gs] == [id(p) for p in m.parameters() if p.requires_grad]
    # no overrides: only the defaults given; bias_lr_factor 1.0 and no weight_decay_bias leave the biases alone
    assert all(set(grp) == {"params"} for grp in _groups(m))
    plain = _groups(m, base_lr=0.1, weight_decay=1e-4)
    assert all(grp["lr"] == 0.1 and grp["weight_decay"] == 1e-4 for grp in plain) and len(plain) == 6
    # overrides by the parameter's name inside its module, applied after weight_decay_norm
    ov = {"embedding": {"lr": 0.01, "weight_decay": 0.1}, "weight": {"weight_decay": 0.3}}
    by = {id(grp["params"][0]): grp for grp in _groups(m, base_lr=0.1, weight_decay=1e-4, weight_decay_norm=0.0, overrides=ov)}
    assert by[id(m.embedding)]["lr"] == 0.01 and by[id(m.embedding)]["weight_decay"] == 0.1
    assert by[id(m.norm.weight)]["weight_decay"] == 0.3 and by[id(m.norm.bias)]["weight_decay"] == 0.0
    assert ov == {"embedding": {"lr": 0.01, "weight_decay": 0.1}, "weight": {"weight_decay": 0.3}}
    with pytest.raises(ValueError, match="bias_lr_factor requires base_lr"):
        _groups(m, bias_lr_factor=2.0)
    with pytest.raises(ValueError, match="Conflicting overrides for 'bias'"):
        _groups(m, weight_decay_bias=0.0, overrides={"bias": {"lr": 1.0}})


# ================================================================================================== d. schedules
def _sched_cfg(*extra):
    from cddmsl_amd.config import get_cfg
    cfg = get_cfg()
    cfg.merge_from_list(["SOLVER.BASE_LR", 5.0, "SOLVER.STEPS", (10, 15, 20), "SOLVER.GAMMA", 0.1, "SOLVER.WARMUP_FACTOR", 0.001,
                         "SOLVER.WARMUP_ITERS", 5, "SOLVER.MAX_ITER", 30, *extra])
    return cfg


def test_schedule_known_answers():
    from cddmsl_amd.config import get_cfg
    from cddmsl_amd.solver import lr_at
    assert get_cfg().SOLVER.LR_SCHEDULER_NAME == "WarmupMultiStepLR"
    lrs = [lr_at(_sched_cfg(), i) for i in range(31)]             # the multistep default: tests/test_scheduler.py:14-43
    want = [0.005, 1.004, 2.003, 3.002, 4.001] + [5.0] * 5 + [0.5] * 5 + [0.05] * 5 + [0.005] * 11
    assert all(abs(a - b) < 1e-9 for a, b in zip(lrs, want)), lrs
    cos = [lr_at(_sched_cfg("SOLVER.LR_SCHEDULER_NAME", "WarmupCosineLR"), i) for i in range(31)]      # :45-68
    end = 2.5 * (1 + math.cos(math.pi / 6))
    for i, v in enumerate(cos):
        want_i = 2.5 * (1 + math.cos(math.pi * i / 30)) if i >= 5 else 0.005 + (end - 0.005) * i / 5
        assert abs(v - want_i) < 1e-9, (i, v, want_i)
    const = [lr_at(_sched_cfg("SOLVER.LR_SCHEDULER_NAME", "WarmupCosineLR", "SOLVER.WARMUP_METHOD", "constant"), i) for i in range(31)]
    assert all(abs(v - 0.005) < 1e-12 for v in const[:5]) and all(abs(a - b) < 1e-12 for a, b in zip(const[5:], cos[5:]))
    mconst = [lr_at(_sched_cfg("SOLVER.WARMUP_METHOD", "constant"), i) for i in range(31)]
    assert all(abs(v - 0.005) < 1e-12 for v in mconst[:5]) and mconst[5:] == lrs[5:]
    # a warm-up longer than the run ends with the run: it reaches sched(1) at MAX_ITER (solver/build.py:259)
    long = _sched_cfg("SOLVER.WARMUP_ITERS", 60)
    assert abs(lr_at(long, 15) - 5.0 * (0.001 * 0.5 + 0.001 * 0.5)) < 1e-12
    for bad in ("WarmupTwoStageMultiStepLR", "StepLR"):
        with pytest.raises(ValueError, match="Unknown LR scheduler: " + bad):
            lr_at(_sched_cfg("SOLVER.LR_SCHEDULER_NAME", bad), 0)
    with pytest.raises(ValueError, match="Unknown warmup method: burnin"):
        lr_at(_sched_cfg("SOLVER.WARMUP_METHOD", "burnin"), 0)


# ================================================================================================== e. - g. ClippedSGD on the host
def _cfg(*extra, yaml=None):
    from cddmsl_amd.config import get_cfg
    cfg = get_cfg()
    if yaml:
        cfg.merge_from_file(os.path.join(ROOT, "configs", yaml))
    cfg.merge_from_list(list(extra))
    return cfg


def test_construction_errors():
    from cddmsl_amd.solver import build_optimizer
    m = Toy()
    with pytest.raises(ValueError, match="'both' is not a valid GradientClipType"):
        build_optimizer(_cfg("SOLVER.CLIP_GRADIENTS.ENABLED", True, "SOLVER.CLIP_GRADIENTS.CLIP_TYPE", "both"), m)
    for nt in (3.0, 0.0, "two"):
        with pytest.raises(ValueError, match="1.0, 2.0 and inf"):
            build_optimizer(_cfg("SOLVER.CLIP_GRADIENTS.ENABLED", True, "SOLVER.CLIP_GRADIENTS.CLIP_TYPE", "norm",
                                 "SOLVER.CLIP_GRADIENTS.NORM_TYPE", nt), m)
    with pytest.raises(ValueError, match="Nesterov momentum requires a momentum and zero dampening"):
        build_optimizer(_cfg("SOLVER.NESTEROV", True, "SOLVER.MOMENTUM", 0.0), m)
    # a disabled clipper is not looked at (solver/build.py:94-95), and the reference's default CLIP_TYPE "value" constructs
    build_optimizer(_cfg("SOLVER.CLIP_GRADIENTS.CLIP_TYPE", "both"), m)
    build_optimizer(_cfg("SOLVER.CLIP_GRADIENTS.ENABLED", True), m)


class _Recorder:
    def __init__(self, monkeypatch):
        from cddmsl_amd import hip
        self.calls = []
        monkeypatch.setattr(hip, "sgd_clip_step", lambda *a: self.calls.append(("sgd_clip_step", a)))
        monkeypatch.setattr(hip, "sgd_step_groups", lambda *a: self.calls.append(("sgd_step_groups", a)))

    def step(self, opt, params, iteration):
        """give every parameter of ``params`` a gradient as the backward pass does, take one step, return the recorded call"""
        from cddmsl_amd import layers
        for p in params:
            p.grad = torch.zeros_like(p)
            layers._TOUCHED.add(id(p))
        opt.iteration = iteration
        n = len(self.calls)
        lr = opt.step()
        assert len(self.calls) == n + 1
        return lr, self.calls[-1]


def _same(tensors, want):
    return len(tensors) == len(want) and all(a.data_ptr() == b.data_ptr() for a, b in zip(tensors, want))


def _assert_old_call(opt, call, ps, lr, cfg, clip, first):
    name, (P, G, M, ws, a_lr, mo, wd, a_clip, a_first) = call
    assert name == "sgd_clip_step"
    assert _same(P, ps) and _same(G, [p.grad for p in ps]) and _same(M, [opt.moms[id(p)] for p in ps]) and ws is opt.norm_ws
    assert (a_lr, mo, wd, a_clip, bool(a_first)) == (lr, cfg.SOLVER.MOMENTUM, cfg.SOLVER.WEIGHT_DECAY, clip, first)


def test_default_and_shipped_configs_call_the_old_entry_point(monkeypatch):
    from cddmsl_amd.modeling.rcnn import GeneralizedRCNN
    from cddmsl_amd.solver import build_optimizer, lr_at
    rec = _Recorder(monkeypatch)
    toy = Toy(norm=False)                                        # (with a torch.nn normalisation layer: OPTIONS' last entry)
    ps = [p for p in toy.parameters() if p.requires_grad]
    cfg = _cfg()
    opt = build_optimizer(cfg, toy)
    lr, call = rec.step(opt, ps, 0)
    assert lr == lr_at(cfg, 0) == cfg.SOLVER.BASE_LR * cfg.SOLVER.WARMUP_FACTOR
    _assert_old_call(opt, call, ps, lr, cfg, float("inf"), True)
    lr, call = rec.step(opt, ps[1:3], 2000)                      # only the parameters that received a gradient this step
    _assert_old_call(opt, call, ps[1:3], cfg.SOLVER.BASE_LR, cfg, float("inf"), False)
    for y in YAMLS:
        cfg = _cfg(yaml=y)
        model = GeneralizedRCNN(cfg)
        opt = build_optimizer(cfg, model)
        all_ps = [p for p in model.parameters() if p.requires_grad]
        assert opt.uniform and _same(opt.params, all_ps), y
        some = all_ps[:7] + all_ps[-5:]
        lr, call = rec.step(opt, some, 50)
        clip = cfg.SOLVER.CLIP_GRADIENTS.CLIP_VALUE if cfg.SOLVER.CLIP_GRADIENTS.ENABLED else float("inf")
        _assert_old_call(opt, call, some, lr_at(cfg, 50), cfg, clip, True)
        del model, opt


OPTIONS = (
    # (config options, expected clip mode, expected clip value, nesterov, lr factor of (weight, bias), weight decay of (weight, norm weight, bias))
    (("SOLVER.NESTEROV", True), 0, float("inf"), True, (1.0, 1.0), (1e-4, 0.0, 1e-4)),
    (("SOLVER.BIAS_LR_FACTOR", 2.0), 0, float("inf"), False, (1.0, 2.0), (1e-4, 0.0, 1e-4)),
    (("SOLVER.WEIGHT_DECAY_BIAS", 0.0), 0, float("inf"), False, (1.0, 1.0), (1e-4, 0.0, 0.0)),
    (("SOLVER.WEIGHT_DECAY_NORM", 1e-4, "SOLVER.CLIP_GRADIENTS.ENABLED", True), 1, 1.0, False, (1.0, 1.0), (1e-4, 1e-4, 1e-4)),
    (("SOLVER.WEIGHT_DECAY_NORM", 1e-4, "SOLVER.CLIP_GRADIENTS.ENABLED", True, "SOLVER.CLIP_GRADIENTS.CLIP_TYPE", "norm",
      "SOLVER.CLIP_GRADIENTS.NORM_TYPE", 1.0, "SOLVER.CLIP_GRADIENTS.CLIP_VALUE", 5.0), 3, 5.0, False, (1.0, 1.0), (1e-4, 1e-4, 1e-4)),
    (("SOLVER.WEIGHT_DECAY_NORM", 1e-4, "SOLVER.CLIP_GRADIENTS.ENABLED", True, "SOLVER.CLIP_GRADIENTS.CLIP_TYPE", "norm",
      "SOLVER.CLIP_GRADIENTS.NORM_TYPE", "inf"), 4, 1.0, False, (1.0, 1.0), (1e-4, 1e-4, 1e-4)),
    (("SOLVER.WEIGHT_DECAY_NORM", 1e-4, "SOLVER.CLIP_GRADIENTS.ENABLED", True, "SOLVER.CLIP_GRADIENTS.CLIP_TYPE", "norm",
      "SOLVER.CLIP_GRADIENTS.NORM_TYPE", float("inf")), 4, 1.0, False, (1.0, 1.0), (1e-4, 1e-4, 1e-4)),
    # WEIGHT_DECAY_NORM's default 0.0 differs from WEIGHT_DECAY on a model with a torch.nn normalisation layer, as in the reference
    ((), 0, float("inf"), False, (1.0, 1.0), (1e-4, 0.0, 1e-4)),
)


@pytest.mark.parametrize("opts,mode,clip,nest,lrf,wdv", OPTIONS, ids=[str(i) for i in range(len(OPTIONS))])
def test_each_other_option_calls_the_grouped_entry_point(opts, mode, clip, nest, lrf, wdv, monkeypatch):
    from cddmsl_amd.solver import build_optimizer, lr_at, lr_multiplier
    rec = _Recorder(monkeypatch)
    m = Toy()
    cfg = _cfg(*opts)
    opt = build_optimizer(cfg, m)
    assert not opt.uniform
    ps = [p for p in m.parameters() if p.requires_grad]
    is_bias = [p is m.fc.bias or p is m.norm.bias for p in ps]
    want_wd = [wdv[2] if b else (wdv[1] if p is m.norm.weight else wdv[0]) for p, b in zip(ps, is_bias)]
    for it, first in ((0, True), (700, False)):
        lr, (name, a) = rec.step(opt, ps, it)
        P, G, M, ws, lrs, wds, mo, a_nest, a_mode, a_clip, a_first = a
        assert name == "sgd_step_groups" and lr == lr_at(cfg, it)
        assert _same(P, ps) and _same(G, [p.grad for p in ps]) and _same(M, [opt.moms[id(p)] for p in ps]) and ws is opt.norm_ws
        mult = lr_multiplier(cfg, it)
        assert lrs == [cfg.SOLVER.BASE_LR * lrf[1 if b else 0] * mult for b in is_bias] and wds == want_wd
        assert (mo, a_nest, a_mode, a_clip, bool(a_first)) == (cfg.SOLVER.MOMENTUM, nest, mode, clip, first)
    # the view the reference's hooks read
    opt.iteration = 700
    groups = opt.param_groups
    assert [g["params"][0] for g in groups] == ps and all(set(g) == {"params", "lr", "initial_lr", "weight_decay", "momentum", "nesterov"} for g in groups)
    assert [g["lr"] for g in groups] == lrs and [g["weight_decay"] for g in groups] == want_wd
    assert all(g["initial_lr"] == cfg.SOLVER.BASE_LR * lrf[1 if b else 0] and g["nesterov"] is nest for g, b in zip(groups, is_bias))


def test_l2_norm_clipping_without_groups_keeps_the_old_entry_point(monkeypatch):
    from cddmsl_amd.solver import build_optimizer
    rec = _Recorder(monkeypatch)
    m = Toy()
    ps = [p for p in m.parameters() if p.requires_grad]
    cfg = _cfg("SOLVER.WEIGHT_DECAY_NORM", 1e-4, "SOLVER.CLIP_GRADIENTS.ENABLED", True, "SOLVER.CLIP_GRADIENTS.CLIP_TYPE", "norm",
               "SOLVER.CLIP_GRADIENTS.CLIP_VALUE", 5.0)
    opt = build_optimizer(cfg, m)
    lr, call = rec.step(opt, ps, 3000)
    _assert_old_call(opt, call, ps, lr, cfg, 5.0, True)


def test_state_dict_round_trip_keeps_its_keys(monkeypatch):
    from cddmsl_amd.solver import build_optimizer
    rec = _Recorder(monkeypatch)
    m = Toy()
    ps = [p for p in m.parameters() if p.requires_grad]
    cfg = _cfg("SOLVER.NESTEROV", True, "SOLVER.BIAS_LR_FACTOR", 2.0)
    opt = build_optimizer(cfg, m)
    assert opt.state_dict() == {"momentum_buffers": None, "steps_done": 0, "iteration": 0}
    rec.step(opt, ps, 41)
    for i, p in enumerate(ps):
        opt.moms[id(p)].fill_(float(i + 1))
    sd = opt.state_dict()
    assert set(sd) == {"momentum_buffers", "steps_done", "iteration"} and (sd["steps_done"], sd["iteration"]) == (1, 42)
    assert [tuple(b.shape) for b in sd["momentum_buffers"]] == [tuple(p.shape) for p in ps]          # model.parameters() order
    new = build_optimizer(cfg, m)
    new.load_state_dict(sd)
    assert (new.steps_done, new.iteration) == (1, 42) and new.norm_ws.numel() == len(ps)
    assert all(torch.equal(new.moms[id(p)], torch.full_like(p, float(i + 1))) for i, p in enumerate(ps))
    _, (name, a) = rec.step(new, ps, 42)
    assert name == "sgd_step_groups" and not a[-1]               # a restored optimizer does not take a first step again
