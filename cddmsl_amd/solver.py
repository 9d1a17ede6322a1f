"""Optimizer / LR schedule of the hot path -- detectron2/solver/build.py:23-262, solver/lr_scheduler.py:17-116.

``ClippedSGD`` = torch.optim.SGD over one param group per parameter (``get_default_optimizer_params``) with the reference's
*per-parameter* gradient clipping (solver/build.py:23-110), run as ONE fused multi-tensor HIP launch family instead of ~120
tensors x (norm + clip + update).  The configuration every shipped YAML uses -- one lr and one weight decay for all parameters, no
Nesterov, clipping off or by L2 norm -- runs through ``hip.sgd_clip_step``; every other one through ``hip.sgd_step_groups``.
"""
import contextlib
import math

import torch

from . import hip, layers

# the torch.nn normalisation layers whose parameters take SOLVER.WEIGHT_DECAY_NORM (solver/build.py:188-200)
NORM_MODULE_TYPES = (torch.nn.BatchNorm1d, torch.nn.BatchNorm2d, torch.nn.BatchNorm3d, torch.nn.SyncBatchNorm, torch.nn.GroupNorm,
                     torch.nn.InstanceNorm1d, torch.nn.InstanceNorm2d, torch.nn.InstanceNorm3d, torch.nn.LayerNorm,
                     torch.nn.LocalResponseNorm)
LR_SCHEDULERS = ("WarmupMultiStepLR", "WarmupCosineLR")


def _sched(s, name, it):
    """the schedule below the warm-up at iteration ``it``: MultiStepParamScheduler / CosineParamScheduler(1, 0)"""
    if name == "WarmupCosineLR":
        return 0.5 * (1.0 + math.cos(math.pi * it / s.MAX_ITER))
    steps = [x for x in s.STEPS if x <= s.MAX_ITER]
    return s.GAMMA ** sum(1 for x in steps if it >= x)


def lr_multiplier(cfg, it):
    """WarmupParamScheduler(MultiStepParamScheduler | CosineParamScheduler): the factor LRMultiplier puts on every group's
    initial lr (solver/build.py:220-262, lr_scheduler.py:37-49)"""
    s = cfg.SOLVER
    name = s.get("LR_SCHEDULER_NAME", "WarmupMultiStepLR")
    if name not in LR_SCHEDULERS:
        raise ValueError("Unknown LR scheduler: {}".format(name))
    if s.WARMUP_METHOD not in ("linear", "constant"):
        raise ValueError("Unknown warmup method: {}".format(s.WARMUP_METHOD))
    warm = min(s.WARMUP_ITERS, s.MAX_ITER)      # warm-up ends at min(WARMUP_ITERS / MAX_ITER, 1) of the run
    mult = _sched(s, name, it)
    if it < warm:
        start = s.WARMUP_FACTOR * _sched(s, name, 0)
        if s.WARMUP_METHOD == "constant":
            return start
        end = _sched(s, name, warm)
        a = it / warm
        mult = start * (1 - a) + end * a
    return mult


def lr_at(cfg, it):
    """base learning rate at iteration ``it``; KAT tests/test_scheduler.py:14-68."""
    return cfg.SOLVER.BASE_LR * lr_multiplier(cfg, it)


def get_default_optimizer_params(model, base_lr=None, weight_decay=None, weight_decay_norm=None, bias_lr_factor=1.0,
                                 weight_decay_bias=None, overrides=None):
    """One param group per trainable parameter, in ``model.parameters()`` order, with the reference's rules (solver/build.py:133-217):
    ``weight_decay_norm`` for the parameters of torch.nn normalisation layers, then ``overrides[name]`` for parameters called
    ``name`` inside their module; the "bias" override is made of ``bias_lr_factor`` (when not 1) and ``weight_decay_bias``.
    A parameter shared between modules appears once, a frozen one not at all."""
    overrides = dict(overrides or {})
    defaults = {}
    if base_lr is not None:
        defaults["lr"] = base_lr
    if weight_decay is not None:
        defaults["weight_decay"] = weight_decay
    bias = {}
    if bias_lr_factor is not None and bias_lr_factor != 1.0:
        if base_lr is None:
            raise ValueError("bias_lr_factor requires base_lr")
        bias["lr"] = base_lr * bias_lr_factor
    if weight_decay_bias is not None:
        bias["weight_decay"] = weight_decay_bias
    if bias:
        if "bias" in overrides:
            raise ValueError("Conflicting overrides for 'bias'")
        overrides["bias"] = bias
    groups, seen = [], set()
    for module in model.modules():
        for name, p in module.named_parameters(recurse=False):
            if not p.requires_grad or id(p) in seen:
                continue
            seen.add(id(p))
            hyper = dict(defaults)
            if weight_decay_norm is not None and isinstance(module, NORM_MODULE_TYPES):
                hyper["weight_decay"] = weight_decay_norm
            hyper.update(overrides.get(name, {}))
            groups.append({"params": [p], **hyper})
    return groups


def _clip_mode(cg):
    """SOLVER.CLIP_GRADIENTS -> (hip.SGD_CLIP_MODES value, clip value); solver/build.py:18-40"""
    if not cg.ENABLED:
        return hip.SGD_CLIP_MODES["none"], float("inf")
    if cg.CLIP_TYPE not in ("value", "norm"):
        raise ValueError("{!r} is not a valid GradientClipType".format(cg.CLIP_TYPE))
    if cg.CLIP_TYPE == "value":
        return hip.SGD_CLIP_MODES["value"], float(cg.CLIP_VALUE)
    nt = cg.NORM_TYPE
    if isinstance(nt, str) and nt.strip().lower() in ("inf", ".inf", "+inf", "+.inf", "infinity"):
        nt = float("inf")
    if isinstance(nt, bool) or not isinstance(nt, (int, float)) or nt not in (1.0, 2.0, float("inf")):
        raise ValueError("SOLVER.CLIP_GRADIENTS.NORM_TYPE {!r}: the supported norms are 1.0, 2.0 and inf".format(cg.NORM_TYPE))
    return hip.SGD_CLIP_MODES[{1.0: "l1", 2.0: "l2"}.get(float(nt), "inf")], float(cg.CLIP_VALUE)


class ClippedSGD:
    def __init__(self, params, cfg):
        """``params``: parameters (every one at BASE_LR / WEIGHT_DECAY) or param groups as get_default_optimizer_params makes them"""
        s = cfg.SOLVER
        self.cfg = cfg
        self.momentum, self.wd, self.nesterov = s.MOMENTUM, s.WEIGHT_DECAY, bool(s.NESTEROV)
        if self.nesterov and self.momentum <= 0:
            raise ValueError("Nesterov momentum requires a momentum and zero dampening")
        self.params, self.initial_lr, self.weight_decay = [], {}, {}
        for g in params:
            g = g if isinstance(g, dict) else {"params": [g]}
            for p in g["params"]:
                if p.requires_grad and id(p) not in self.initial_lr:
                    self.params.append(p)
                    self.initial_lr[id(p)] = g.get("lr", s.BASE_LR)
                    self.weight_decay[id(p)] = g.get("weight_decay", s.WEIGHT_DECAY)
        self.clip_mode, clip = _clip_mode(s.CLIP_GRADIENTS)
        modes = hip.SGD_CLIP_MODES
        # the configuration cddmsl_sgd_clip_step implements: plain SGD (solver/build.py:113-130; an infinite clip value = factor 1)
        # or per-parameter L2-norm clipping (:59-67), one lr and one weight decay for every parameter
        self.uniform = (not self.nesterov and self.clip_mode in (modes["none"], modes["l2"])
                        and all(self.initial_lr[id(p)] == s.BASE_LR and self.weight_decay[id(p)] == s.WEIGHT_DECAY for p in self.params))
        self.clip = clip
        self.moms = None
        self.norm_ws = None
        self.steps_done = 0
        self.iteration = 0

    @property
    def param_groups(self):
        """read-only view in torch.optim's layout, one group per parameter (``lr`` is the one the next step will use)"""
        mult = lr_multiplier(self.cfg, self.iteration)
        return tuple({"params": [p], "lr": self.initial_lr[id(p)] * mult, "initial_lr": self.initial_lr[id(p)],
                      "weight_decay": self.weight_decay[id(p)], "momentum": self.momentum, "nesterov": self.nesterov}
                     for p in self.params)

    def zero_grad(self):
        for p in self.params:
            if p.grad is not None:
                p.grad.zero_()

    def state_dict(self):
        """momentum buffers in parameter order (torch.optim.SGD's 'state' keyed by parameter index) + step counters"""
        moms = None if self.moms is None else [self.moms[id(p)].detach().cpu() for p in self.params]
        return {"momentum_buffers": moms, "steps_done": self.steps_done, "iteration": self.iteration}

    def load_state_dict(self, sd):
        self.steps_done, self.iteration = int(sd["steps_done"]), int(sd["iteration"])
        if sd["momentum_buffers"] is not None:
            assert len(sd["momentum_buffers"]) == len(self.params)
            self.moms = {id(p): m.to(p.device).clone(memory_format=torch.preserve_format) for p, m in zip(self.params, sd["momentum_buffers"])}
            self.norm_ws = torch.zeros(len(self.params), device=self.params[0].device, dtype=torch.float32)

    def step(self):
        touched = layers.take_touched()     # torch.optim.SGD skips parameters whose grad is None (e.g. the projector in stock configs)
        ps = [p for p in self.params if p.grad is not None and id(p) in touched]
        if self.moms is None:
            self.moms = {id(p): torch.zeros_like(p, memory_format=torch.preserve_format) for p in self.params}
            self.norm_ws = torch.zeros(len(self.params), device=self.params[0].device, dtype=torch.float32)
        lr = lr_at(self.cfg, self.iteration)
        with torch.no_grad():
            if self.uniform:
                hip.sgd_clip_step([p.data for p in ps], [p.grad for p in ps], [self.moms[id(p)] for p in ps], self.norm_ws,
                                  lr, self.momentum, self.wd, self.clip, self.steps_done == 0)
            else:
                mult = lr_multiplier(self.cfg, self.iteration)      # LRMultiplier: every group's initial lr times one multiplier
                hip.sgd_step_groups([p.data for p in ps], [p.grad for p in ps], [self.moms[id(p)] for p in ps], self.norm_ws,
                                    [self.initial_lr[id(p)] * mult for p in ps], [self.weight_decay[id(p)] for p in ps],
                                    self.momentum, self.nesterov, self.clip_mode, self.clip, self.steps_done == 0)
        self.steps_done += 1
        self.iteration += 1
        layers.bump_weight_version()   # prepared (cast / transposed) weights are stale now
        layers.FP8_SCALES.roll()       # fp8 configuration: this step's recorded activation maxima become the next step's scales
        return lr


def average_weight(mode, decay, n):
    """The weight ``w`` of update number ``n >= 1`` (``n`` updates done so far, the first of them the copy) in avg += w (param - avg):
    ``"ema"``: 1 - decay; ``"uniform"``: 1 / (n + 1), the running mean of n + 1 snapshots (torch.optim.swa_utils.AveragedModel)."""
    if n < 1:
        raise ValueError("average_weight: update 0 is the copy and has no weight")
    if mode == "ema":
        return 1.0 - float(decay)
    if mode == "uniform":
        return 1.0 / (n + 1.0)
    raise ValueError("MODEL_EMA.MODE {!r}: one of ('ema', 'uniform')".format(mode))


class WeightAverage:
    """An average of the trainable parameters, one f32 tensor per parameter, kept on the parameters' device by ONE multi-tensor HIP
    launch family per step (``hip.weight_average``): an exponential moving average (``mode`` "ema", D2Go's MODEL_EMA) or the uniform
    running mean of the snapshots taken since ``start_iter`` ("uniform", SWA / SWAD).  Every normalisation layer here is FrozenBN,
    so the averaged weights need no batch-norm re-estimation: ``applied(model)`` evaluates them as they are.
    Construction and the state handling work on CPU tensors; only ``update`` needs the device."""

    def __init__(self, named_params, mode="ema", decay=0.999, start_iter=0):
        average_weight(mode, decay, 1)                   # (refuses an unknown mode)
        self.mode, self.decay, self.start_iter = mode, float(decay), int(start_iter)
        self.names, self.params = [], []
        for name, p in named_params:
            self.names.append(name)
            self.params.append(p)
        if len(set(self.names)) != len(self.names):
            raise ValueError("WeightAverage: a parameter name appears twice")
        with torch.no_grad():
            self.tensors = [torch.zeros_like(p, memory_format=torch.preserve_format) for p in self.params]
        self.updates = 0

    def update(self, iteration):
        """after ``optimizer.step()`` of iteration ``iteration``: nothing before ``start_iter``, then a copy, then the average"""
        if iteration < self.start_iter:
            return
        with torch.no_grad():
            ps = [p.data for p in self.params]
            if self.updates == 0:
                hip.weight_average(self.tensors, ps, 0.0, True)
            else:
                hip.weight_average(self.tensors, ps, average_weight(self.mode, self.decay, self.updates), False)
        self.updates += 1

    def state_dict(self):
        return {"mode": self.mode, "decay": self.decay, "start_iter": self.start_iter, "updates": self.updates,
                "tensors": {k: t.detach().cpu().clone(memory_format=torch.contiguous_format) for k, t in zip(self.names, self.tensors)}}

    def load_state_dict(self, sd):
        if sd["mode"] != self.mode:
            raise ValueError(f"WeightAverage: the saved average is of mode {sd['mode']!r}, the configured one of {self.mode!r}")
        saved = sd["tensors"]
        if set(saved) != set(self.names):
            diff = sorted(set(saved) ^ set(self.names))
            raise ValueError(f"WeightAverage: the saved average covers other parameters ({len(diff)} names differ, e.g. {diff[:3]})")
        for k, t in zip(self.names, self.tensors):
            if tuple(saved[k].shape) != tuple(t.shape):
                raise ValueError(f"WeightAverage: {k} is {tuple(saved[k].shape)} in the saved average, {tuple(t.shape)} in the model")
        with torch.no_grad():
            for k, t in zip(self.names, self.tensors):
                t.copy_(saved[k])
        self.updates = int(sd["updates"])

    @contextlib.contextmanager
    def applied(self, model=None):
        """The averaged values in the parameters for the length of the block, the training values back on exit (also on an
        exception).  The contents are exchanged through the parameters' own storage, so every address the rest of the code holds
        (gradient views, momentum keys) stays valid; the weight version is bumped on entry and on exit, so no prepared (cast /
        transposed / FrozenBN-folded) weight of the other set survives.  Before the first update it does nothing."""
        if self.updates == 0:
            yield self
            return
        with torch.no_grad():
            kept = [p.detach().clone(memory_format=torch.preserve_format) for p in self.params]
            for p, t in zip(self.params, self.tensors):
                p.data.copy_(t)
        layers.bump_weight_version()
        try:
            yield self
        finally:
            with torch.no_grad():
                for p, k in zip(self.params, kept):
                    p.data.copy_(k)
            layers.bump_weight_version()


def build_weight_average(cfg, model, optimizer):
    """``cfg.MODEL_EMA`` -> a WeightAverage over the optimizer's parameters under their ``model.named_parameters()`` names, or None"""
    from .config import check_model_ema
    e = check_model_ema(cfg)
    if e is None:
        return None
    names = {id(p): k for k, p in model.named_parameters()}
    return WeightAverage([(names[id(p)], p) for p in optimizer.params], e.MODE, e.DECAY, e.START_ITER)


def linear_warmup_schedule(step, warmup, total):
    """transformers' ``get_linear_schedule_with_warmup`` (ClipCap's train.py): the factor on the base lr at scheduler step ``step``:
    a linear ramp 0 -> 1 over ``warmup`` steps, then linear 1 -> 0 at ``total``, never below 0."""
    if step < warmup:
        return float(step) / float(max(1, warmup))
    return max(0.0, float(total - step) / float(max(1, total - warmup)))


class AdamW:
    """torch.optim.AdamW (amsgrad off) over a list of f32 parameters as ONE multi-tensor HIP launch family (``hip.adamw_step``).
    The state carries torch's names: per parameter ``exp_avg``, ``exp_avg_sq`` and ``step``.  Parameters whose ``grad`` is None are
    skipped, as torch skips them.  ``lr`` is an attribute: the training loop sets it from its schedule before each step."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2):
        self.params = [p for p in params if p.requires_grad]
        self.lr, self.betas, self.eps, self.weight_decay = float(lr), (float(betas[0]), float(betas[1])), float(eps), float(weight_decay)
        self.state = {}

    def zero_grad(self):
        for p in self.params:
            if p.grad is not None:
                p.grad.zero_()

    def _state(self, p):
        s = self.state.get(id(p))
        if s is None:
            s = self.state[id(p)] = {"step": 0, "exp_avg": torch.zeros_like(p, memory_format=torch.preserve_format),
                                     "exp_avg_sq": torch.zeros_like(p, memory_format=torch.preserve_format)}
        return s

    def step(self):
        layers.take_touched()
        ps = [p for p in self.params if p.grad is not None]
        by_step = {}
        for p in ps:                                   # (one launch family per step count: they differ only after a late first gradient)
            s = self._state(p)
            s["step"] += 1
            by_step.setdefault(s["step"], []).append(p)
        with torch.no_grad():
            for k, group in by_step.items():
                hip.adamw_step([p.data for p in group], [p.grad for p in group], [self.state[id(p)]["exp_avg"] for p in group],
                               [self.state[id(p)]["exp_avg_sq"] for p in group], self.lr, self.betas[0], self.betas[1], self.eps,
                               self.weight_decay, k)
        layers.bump_weight_version()   # prepared (cast / transposed) weights are stale now
        return self.lr

    def state_dict(self):
        """torch.optim's layout: ``state`` keyed by the parameter's index, ``param_groups`` with the hyper-parameters"""
        state = {}
        for i, p in enumerate(self.params):
            s = self.state.get(id(p))
            if s is not None:
                state[i] = {"step": int(s["step"]), "exp_avg": s["exp_avg"].detach().cpu(), "exp_avg_sq": s["exp_avg_sq"].detach().cpu()}
        return {"state": state, "param_groups": [{"lr": self.lr, "betas": self.betas, "eps": self.eps, "weight_decay": self.weight_decay,
                                                  "params": list(range(len(self.params)))}]}

    def load_state_dict(self, sd):
        g = sd["param_groups"][0]
        assert len(g["params"]) == len(self.params), "optimizer state for another parameter list"
        self.lr, self.betas, self.eps, self.weight_decay = float(g["lr"]), tuple(float(b) for b in g["betas"]), float(g["eps"]), float(g["weight_decay"])
        self.state = {}
        for i, s in sd["state"].items():
            p = self.params[int(i)]
            self.state[id(p)] = {"step": int(s["step"]),
                                 "exp_avg": s["exp_avg"].to(p.device, torch.float32).clone(memory_format=torch.preserve_format),
                                 "exp_avg_sq": s["exp_avg_sq"].to(p.device, torch.float32).clone(memory_format=torch.preserve_format)}


def build_optimizer(cfg, model):
    s = cfg.SOLVER
    groups = get_default_optimizer_params(model, base_lr=s.BASE_LR, weight_decay=s.WEIGHT_DECAY, weight_decay_norm=s.WEIGHT_DECAY_NORM,
                                          bias_lr_factor=s.BIAS_LR_FACTOR, weight_decay_bias=s.WEIGHT_DECAY_BIAS)
    return ClippedSGD(groups, cfg)
