"""The e4m3 routes of the autograd nodes written plainly, for tests/test_graph_fp8_ref_host.py and tests/test_gpu_graph_fp8.py; not a
conftest, no tests.  Built on tests/graph_ref.py (the plain modules, bf16 rounding, the metric, the input builders) and on
tests/exact_fp8.py (round-to-nearest-even onto the e4m3 grid in plain arithmetic).

The element is ONE "e4m3 convolution with affine" (``_E4m3Conv``), a torch.autograd.Function whose three GEMMs are each torch's own
product on substituted operands -- nothing is derived by hand:

  forward          conv(Q(x; s_act), Q(w; 448 / max|w|)) * bn_scale                       (bias, residual, ReLU: plain autograd outside)
  input gradient   torch's vjp of F.conv2d wrt its input on Q(g; s_grad) and Q(bf16(w * bn_scale); 448 / max|.|)
  weight gradient  bn_scale * torch's vjp wrt the weight on the SAVED Q(x; s_act) and Q(g; s_grad)
  Q(t; s) = e4m3_rne(clamp(t * s, +-448)) / s

Which of the three is e4m3 and which plain is the case's ``plan`` (tests/graph_fp8_cases.py); which tensors share a slot is stated
by the slot NAMES below, following cddmsl_amd/layers.py:

  b<i>.c<j>.act   the input of conv j of block i (pw._fp8_slot): x, o1, p2 (= o2 in a stride-1 block), the downsample conv's px
  b<i>.gs         the block's masked output gradient (bp._fp8_gs): conv3's input gradient, the downsample conv's input gradient and
                  conv3's weight gradient read ONE copy
  b<i>.c2.g       dpre2 (pw[1]._fp8_g): conv2's two gradient GEMMs
  b<i>.c1.g       dpre1 (pw[0]._fp8_g): conv1's weight gradient only; conv1's input gradient is never e4m3
  act / g         the two slots of a ConvFn case

The scales are INPUTS of the model (``Scales``): the GPU test hands in what the product's slots hold; a name that is not given is
computed as 448 / max|tensor| from the model's own tensor and recorded, which is how the host test gets them.

``round_bf16`` as in graph_ref, and each tensor is rounded to bf16 before it is quantised where the product materialises it in bf16
first.  ``mut=<name>`` (MUTATIONS) makes exactly one routing mistake, in the style of graph_ref.DROPS."""
import torch
import torch.nn.functional as F

import exact_fp8 as X8
import graph_fp8_cases as GC8
import graph_ref as G
from graph_ref import BF, F64, _avg, _bf, _c, _grad_of, _r

E4M3_MAX = X8.E4M3_MAX
BF16_FACTOR, BF16_FLOOR, BF16_CAP = G.BF16_FACTOR, G.BF16_FLOOR, G.BF16_CAP

MUTATIONS = ("deq_neighbour_fwd", "deq_neighbour_dgrad", "deq_neighbour_wgrad", "stale_scale", "wgrad_unmasked", "dgrad_w_without_bn",
             "wgrad3_p2_under_o1", "cos_one_448", "stale_weights")


def f32(v):
    """a Python float rounded to f32, as a slot holds it"""
    return float(torch.tensor(float(v), dtype=torch.float32))


def scale_of(t):
    """448 / max|t| as Fp8Slot.calibrate and Fp8Scales.roll compute it (f32)"""
    return f32(E4M3_MAX / f32(t.detach().abs().max()))


def _scaled(t, s):
    """clamp(t * s, +-448), the product rounded to f32 as the quantising kernels form it: a bf16 value times 448 / (a bf16 maximum)
    lands EXACTLY on a tie of the e4m3 grid on some 0.4 % of the elements (3/16 of the maximum, say), and the f32 rounding of the
    scale decides on which side float64 would see it"""
    return (t.detach().to(F64) * s).to(torch.float32).to(F64).clamp(-E4M3_MAX, E4M3_MAX)


def Q(t, s, deq=None):
    """quantise under scale s, dequantise under 1 / s (or, for a mutation, under another slot's)"""
    return X8.e4m3_rne(_scaled(t, s)) / (s if deq is None else deq)


def codes(t, s):
    return X8.e4m3_encode(_scaled(t, s))


class Scales:
    """slot name -> scale.  ``given``: scales that are inputs; any other name is calibrated from the model's own tensor on first use.
    ``operands``: every (tensor, scale) that was quantised, for the byte check of the host test."""

    def __init__(self, given=None):
        self.given, self.used, self.own, self.operands = dict(given or {}), {}, {}, []

    def get(self, name, t):
        self.own.setdefault(name, scale_of(t))
        if name not in self.used:
            self.used[name] = self.given.get(name, self.own[name])
        return self.used[name]

    def peek(self, name):
        """another slot's scale, for a mutation (a mutated run is given every scale of the unmutated one)"""
        return self.used[name] if name in self.used else self.given[name]


class Opt:
    """what one evaluation of the model carries: the scales, the plan {conv name: (fwd, dgrad, wgrad) e4m3?}, round_bf16, the mutation
    (name, conv it applies to, slot whose factor it borrows), the previous weights {conv name: tensor} for "stale_weights"."""

    def __init__(self, plan, scales=None, round_bf16=False, mut=None, at=None, other=None, prev=None):
        self.plan, self.sc, self.rb, self.mut, self.at, self.other, self.prev = plan, scales or Scales(), round_bf16, mut, at, other, prev or {}

    def hit(self, mut, name):
        return self.mut == mut and self.at == name


def _rt(t, on):
    return t.to(BF).to(t.dtype) if on else t


def _wq(w, o):
    s = scale_of(w)
    o.sc.operands.append((w.detach(), s))
    return Q(w, s)


class _E4m3Conv(torch.autograd.Function):
    """z = conv(x, w) * bn with each GEMM on e4m3 or plain operands according to o.plan[name]; x NHWC, w [Cout, Cin, KH, KW]"""

    @staticmethod
    def forward(ctx, x, w, bn, o, name, act, grad, stride, pad):
        fwd8, _, _ = o.plan[name]
        xp, wp = _rt(x.detach(), o.rb), w.detach()
        x8 = None
        if fwd8:
            s = o.sc.get(act, xp)
            o.sc.operands.append((xp, s))
            deq = o.sc.peek(o.other) if o.hit("deq_neighbour_fwd", name) else None
            x8 = Q(xp, 1.0 if o.hit("stale_scale", name) else s, s if o.hit("stale_scale", name) else deq)
            xa, wa = x8, _wq(o.prev[name].to(w.dtype) if o.hit("stale_weights", name) else wp, o)
            if o.hit("deq_neighbour_fwd", name):
                x8 = Q(xp, s)                        # (the copy itself is right: the weight gradient reads it under its own factor)
        else:
            xa, wa = xp, _rt(wp, o.rb)
        z = _c(xa, wa, stride, pad)
        if bn is not None:
            z = z * bn
        ctx.o, ctx.name, ctx.grad, ctx.cfg, ctx.act = o, name, grad, (stride, pad), act
        ctx.save_for_backward(xp, wp, bn, x8)
        return _rt(z, o.rb)

    @staticmethod
    def backward(ctx, g):
        xp, wp, bn, x8 = ctx.saved_tensors
        o, name, (stride, pad) = ctx.o, ctx.name, ctx.cfg
        _, dgrad8, wgrad8 = o.plan[name]
        assert x8 is not None or not wgrad8, (name, "the e4m3 weight gradient reads the copy kept from an e4m3 forward")
        g = _rt(g.detach(), o.rb)
        g8 = None

        def gq(deq=None):
            s = o.sc.get(ctx.grad, g)
            o.sc.operands.append((g, s))
            return Q(g, s, deq)
        dx = dw = None
        if ctx.needs_input_grad[0]:
            wd = wp if bn is None or o.hit("dgrad_w_without_bn", name) else wp * bn.view(-1, 1, 1, 1)
            if dgrad8:
                ga = gq(o.sc.peek(o.other) if o.hit("deq_neighbour_dgrad", name) else None)
                wda = _wq(_rt(wd, True), o)           # (the prepared input-gradient weights are a bf16 tensor in the product)
            else:
                ga, wda = g, _rt(wd, o.rb)
            with torch.enable_grad():
                xx = torch.zeros_like(xp).requires_grad_(True)
                dx, = torch.autograd.grad(_c(xx, wda, stride, pad), xx, ga)
            dx = _rt(dx, o.rb)
        if ctx.needs_input_grad[1]:
            if wgrad8:
                xa = x8 * (o.sc.peek(ctx.act) / o.sc.peek(o.other)) if o.hit("wgrad3_p2_under_o1", name) else x8
                ga = gq(o.sc.peek(o.other) if o.hit("deq_neighbour_wgrad", name) else None)
            else:
                xa, ga = xp, g
            with torch.enable_grad():
                ww = torch.zeros_like(wp).requires_grad_(True)
                dw, = torch.autograd.grad(_c(xa, ww, stride, pad), ww, ga)
            if bn is not None:
                dw = dw * bn.view(-1, 1, 1, 1)
        return dx, dw, None, None, None, None, None, None, None


def conv8(x, w, o, name, act, grad, bn=None, b=None, relu=False, residual=None, stride=1, pad=0):
    """relu?(e4m3conv(x, w) * bn + b + residual)"""
    def pre(xx, ww):
        z = _E4m3Conv.apply(xx, ww, bn, o, name, act, grad, stride, pad)
        z = z if b is None else z + b
        return z if residual is None else z + _r(residual, o.rb)
    if relu and o.hit("wgrad_unmasked", name):
        zx, zw = pre(x, w.detach()), pre(x.detach(), w)
        # the value and the input's (and bias') gradient through the ReLU; the weight's from the gradient as it came
        y = torch.relu(zx) + (zw - zw.detach())
    else:
        z = pre(x, w)
        y = torch.relu(z) if relu else z
    return _r(y, o.rb)


def bottleneck8(x, w, bn, stride, o, bi, parts=None):
    """graph_ref.bottleneck with every convolution an ``_E4m3Conv``"""
    rb, k = o.rb, f"b{bi}."
    (s1, b1), (s2, b2), (s3, b3), bnd = bn
    w1, w2, w3, wd = w
    x = _r(x, rb)
    o1 = conv8(x, w1, o, k + "c1", k + "c1.act", k + "c1.g", s1, b1, relu=True)
    o2 = conv8(o1, w2, o, k + "c2", k + "c2.act", k + "c2.g", s2, b2, relu=True, pad=1)
    p2 = _r(_avg(o2, stride), rb)
    if wd is not None:
        px = _r(_avg(x, stride), rb)
        idn = conv8(px, wd, o, k + "cd", k + "cd.act", k + "gs", bnd[0], bnd[1])
    else:
        idn = x
    return conv8(p2, w3, o, k + "c3", k + "c3.act", k + "gs", s3, b3, relu=True, residual=idn)


def stage8(x, blocks, o):
    for i, b in enumerate(blocks):
        x = bottleneck8(x, b["w"], b["bn"], b["stride"], o, i)
    return x


def roi_stage8(feat, rois, blocks, o, extra=None, out_size=14, scale=1.0 / 16, sr=0):
    """stage8(cat([roi_crops(feat), extra])): the literal order; where the product runs conv1 (and the downsample conv) on the map
    in front of the pooling the plan has them plain, and a plain 1x1 convolution commutes with the pooling exactly"""
    feat, extra = _r(feat, o.rb), _r(extra, o.rb)
    crops = _r(G.roi_crops(feat, rois, out_size, scale, sr), o.rb)
    return stage8(crops if extra is None else torch.cat([crops, extra]), blocks, o)


def cosine8(x, wn, T, fp8, o, eps=1e-12):
    """[R, N + 1]: cosine logits / T with a zero last column; with ``fp8`` the value is the product of the two rows quantised at the
    fixed scale 448, the gradient the unquantised one's (straight-through, CosineLogitsFn)"""
    xn = x / x.norm(dim=1, keepdim=True).clamp_min(eps)
    plain = xn @ wn.t() / T
    if fp8:
        o.sc.operands += [(xn.detach(), E4M3_MAX), (wn.detach(), E4M3_MAX)]
        wq = Q(o.prev["wn"].to(F64), E4M3_MAX) if o.mut == "stale_weights" else Q(wn, E4M3_MAX)
        q = Q(xn, E4M3_MAX) @ wq.t() / T
        plain = _grad_of(q * (E4M3_MAX if o.mut == "cos_one_448" else 1.0), plain)
    return torch.cat([plain, torch.zeros(x.shape[0], 1, dtype=x.dtype)], dim=1)


# ---------------------------------------------------------------------------------------------------------------- inputs of a case
GRAD_SIZE = 2.0 ** -10       # upstream gradients of order 1e-3 against activations of order 1: no gradient slot near an activation's


def _make_blocks8(g, cin, planes, strides, x, gains):
    """graph_ref._make_blocks ("gated" ReLUs: see there) with a gain per layer on the N(0, 1 / fan-in) weights, so that the tensors
    one block quantises differ in magnitude: ``gains`` = per block (conv1, conv2, conv3, downsample)"""
    x = x.to(F64)
    rn = lambda *s: torch.randn(*s, generator=g)
    cw = lambda co, ci, k, gain: _bf(rn(co, ci, k, k) * (gain * (ci * k * k) ** -0.5))
    sc = lambda c: _bf(torch.rand(c, generator=g) + 0.5)
    blocks, margin = [], 1.0
    for bi, stride in enumerate(strides):
        g1, g2, g3, gd = gains[bi]
        w = [cw(planes, cin, 1, g1), cw(planes, planes, 3, g2), cw(4 * planes, planes, 1, g3), cw(4 * planes, cin, 1, gd) if bi == 0 else None]
        s = [sc(planes), sc(planes), sc(4 * planes), sc(4 * planes) if bi == 0 else None]
        d = [None if v is None else v.to(F64) for v in w]
        z1 = _c(x, d[0]) * s[0]
        b1, m1 = G._side_bias(z1, g, "gated")
        o1 = torch.relu(z1 + b1)
        z2 = _c(o1, d[1], pad=1) * s[1]
        b2, m2 = G._side_bias(z2, g, "gated", -1.0)
        p2 = _avg(torch.relu(z2 + b2), stride)
        z3 = _c(p2, d[2]) * s[2]
        idn = _c(_avg(x, stride), d[3]) * s[3] if bi == 0 else x
        bd = _bf(rn(4 * planes) * 2.0 * float((z3 + idn).std())) if bi == 0 else None
        idn = idn + bd if bi == 0 else idn
        b3, _ = G._side_bias(z3 + idn, g, "gated")
        m3 = float(((z3 + idn + b3).abs() / (z3.abs() + idn.abs() + b3.abs())).min())
        x = torch.relu(z3 + b3 + idn)
        margin = min(margin, m1, m2, m3)
        f = lambda v: v.to(torch.float32)
        blocks.append(dict(w=w, bn=[(s[0], f(b1)), (s[1], f(b2)), (s[2], f(b3)), (s[3], bd) if bi == 0 else None], stride=stride))
        cin = 4 * planes
    return blocks, x, margin


def _prev(w):
    """the "previous parameter values" of the stale-weights mutation: half of the neighbouring filter mixed in (the GPU test checks
    the weight copies' freshness through its audit, to the byte, not through a limit)"""
    return _bf(w + 0.5 * w.roll(1, 0))


def make_inputs(case, attempt=0):
    g = torch.Generator().manual_seed(case["seed"] + 1000 * attempt)
    rn = lambda *s: torch.randn(*s, generator=g)
    k, inp, margin = case["kind"], {}, 1.0
    if k == "conv":
        ws = tuple(case["w"])
        inp["x"] = _bf(rn(*case["x"]))
        inp["w"] = _bf(rn(*ws) * (case["gain"] * (ws[1] * ws[2] * ws[3]) ** -0.5))
        y = G.conv(inp["x"], inp["w"], stride=case["stride"], pad=case["pad"])
        if case["bias"]:
            inp["b"] = _bf(rn(ws[0]) * 0.3)
            if case["relu"]:
                b, margin = G._side_bias(y.to(F64), g, "gated")
                inp["b"] = b.to(torch.float32)
        inp["gy"] = _bf(rn(*y.shape) * GRAD_SIZE)
    elif k == "stage":
        inp["x"] = _bf(rn(*case["x"]).clamp_min(0))
        inp["blocks"], y, margin = _make_blocks8(g, case["x"][-1], case["planes"], case["strides"], inp["x"], case["gains"])
        inp["gy"] = _bf(rn(*y.shape) * GRAD_SIZE)
    elif k == "roi":
        inp["feat"] = _bf(rn(*case["feat"]).clamp_min(0))
        inp["rois"] = torch.tensor([G.ROIS[i] for i in case["rois"]], dtype=torch.float32)
        if case["extra"] != "none":
            inp["extra"] = _bf(rn(1, 14, 14, case["feat"][-1]).clamp_min(0) * 0.7)
        x0 = G.roi_crops(inp["feat"].to(F64), inp["rois"], 14, 1.0 / 16, 0)
        x0 = torch.cat([x0, inp["extra"].to(F64)]) if "extra" in inp else x0
        inp["blocks"], y, margin = _make_blocks8(g, case["feat"][-1], case["planes"], case["strides"], x0, case["gains"])
        inp["gy"] = _bf(rn(*y.shape) * GRAD_SIZE)
    elif k == "cosine":
        R, D = case["x"]
        inp["x"] = rn(R, D)
        inp["wn"] = F.normalize(rn(case["rows"], D), dim=1)
        inp["gy"] = rn(R, case["rows"] + 1)
    else:
        raise KeyError(k)
    inp["margin"], inp["attempt"] = margin, attempt
    return inp


def compared(case):
    return ["y", "dx"] if case["kind"] == "cosine" else G.compared(case)


def slot_pairs(case):
    """[(conv name, its activation slot, its gradient slot)] over the convolutions of a case with any e4m3 GEMM"""
    out = []
    for name, plan in case["plan"].items():
        if any(plan):
            if case["kind"] == "conv":
                out.append((name, "act", "g"))
            else:
                blk = name.split(".")[0]
                out.append((name, name + ".act", f"{blk}.gs" if name.endswith(("c3", "cd")) else name + ".g"))
    return out


def mutations_for(case):
    """[(mutation, conv it applies to, the slot whose factor it borrows)] this case can show"""
    k, plan = case["kind"], case.get("plan", {})
    if k == "cosine":
        return [("cos_one_448", None, None), ("stale_weights", None, None)] if case["fp8"] else []
    if k == "conv":
        if not any(plan["c"]):
            return []
        m = [("deq_neighbour_fwd", "c", "g"), ("stale_scale", "c", None), ("stale_weights", "c", None)]
        m += [("deq_neighbour_dgrad", "c", "act")] * (plan["c"][1] and case["x_grad"])
        m += [("deq_neighbour_wgrad", "c", "act"), ("wgrad_unmasked", "c", None)] * (plan["c"][2] and case["train_w"])
        return m
    m = []
    for bi in range(len(case["strides"])):
        b = f"b{bi}."
        if plan[b + "c2"] == (True, True, True):
            m += [("deq_neighbour_dgrad", b + "c2", b + "gs"), ("deq_neighbour_wgrad", b + "c2", b + "gs")]
        # (the mask at the e4m3 weight gradient whose tensor has the tighter limit: conv3's where it is e4m3, else conv2's)
        m += [("wgrad_unmasked", b + ("c3" if plan[b + "c3"][2] else "c2"), None)]
        if plan[b + "c3"][2]:
            m += [("wgrad3_p2_under_o1", b + "c3", b + "c2.act")]
        if plan.get(b + "cd", (False,))[0]:
            # (the downsample conv's input under conv3's factor: the slot next to its own in the table, in order of first use)
            m += [("stale_weights", b + "cd", None)]
            # (with appended maps a one-block RoI stage's output has a wider limit: these two move it by 9.4 and 10.1 times that)
            if k != "roi" or case["extra"] == "none" or case["deep"]:
                m += [("deq_neighbour_fwd", b + "cd", b + "c3.act"), ("stale_scale", b + "cd", None)]
            # (a FrozenBN scale lies in [0.5, 1.5): leaving it out moves a gradient by half of itself at the most, ten times the limit
            # only of dx, which the downsample path carries)
            m += [("dgrad_w_without_bn", b + "cd", None)] * bool(case.get("x_grad", True))
    return m


def reference(case, inp, given=None, round_bf16=False, mut=None, fp8=True, calibrating=False):
    """the quantised model on the case's inputs -> ({name: float64 tensor} over ``compared(case)``, the Scales it used).
    ``given``: {slot: scale}; ``mut``: one entry of ``mutations_for(case)``; ``fp8`` False: every GEMM plain (graph_ref's module);
    ``calibrating``: the plan of pass 1 (graph_fp8_cases.plan_for)."""
    k = case["kind"]
    plan = GC8.plan_for(case, calibrating) if fp8 else {n: (False, False, False) for n in case.get("plan", {})}
    m = mut or (None, None, None)
    o = Opt(plan, Scales(given), round_bf16, m[0], m[1], m[2])
    leaves = {}

    def leaf(name, t, grad=True):
        v = t.to(F64).clone().requires_grad_(bool(grad))
        if grad:
            leaves[name] = v
        return v

    def blocks_of(bl):
        out = []
        for bi, b in enumerate(bl):
            for wi, v in enumerate(b["w"]):
                if v is not None:
                    o.prev[f"b{bi}.c{'123d'[wi]}"] = _prev(v)
            w = [None if v is None else leaf(f"b{bi}.w{wi}", v) for wi, v in enumerate(b["w"])]
            out.append(dict(w=w, bn=[None if v is None else (v[0].to(F64), v[1].to(F64)) for v in b["bn"]], stride=b["stride"]))
        return out
    if k == "conv":
        x = leaf("dx", inp["x"], case["x_grad"])
        w = leaf("w", inp["w"], case["train_w"])
        b = leaf("b", inp["b"], case["train_w"]) if case["bias"] else None
        o.prev["c"] = _prev(inp["w"])
        y = conv8(x, w, o, "c", "act", "g", None, _r(b, o.rb), case["relu"], None, case["stride"], case["pad"])
    elif k == "stage":
        y = stage8(leaf("dx", inp["x"], case["x_grad"]), blocks_of(inp["blocks"]), o)
    elif k == "roi":
        extra = leaf("dextra", inp["extra"], case["extra"] == "grad") if "extra" in inp else None
        y = roi_stage8(leaf("dfeat", inp["feat"], case["feat_grad"]), inp["rois"], blocks_of(inp["blocks"]), o, extra)
    elif k == "cosine":
        o.prev["wn"] = F.normalize(inp["wn"] + 0.5 * inp["wn"].roll(1, 0), dim=1)
        y = cosine8(leaf("dx", inp["x"]), inp["wn"].to(F64), case["T"], case["fp8"] and fp8, o)
    else:
        raise KeyError(k)
    y.backward(inp["gy"].to(F64))
    out = {"y": y.detach()}
    for n in compared(case)[1:]:
        out[n] = leaves[n].grad if leaves[n].grad is not None else torch.zeros_like(leaves[n])
    return {n: v.to(F64) for n, v in out.items()}, o.sc


rel_err = G.rel_err
ATTEMPTS = G.ATTEMPTS
_cache = {}


def limits(case, inp, given=None, calibrating=False):
    """-> (exact quantised model, its Scales, {name: limit}) under ``given`` scales (None: the model's own): the limit of a tensor is
    max(BF16_FACTOR x error of the round_bf16 quantised model against the exact one, BF16_FLOOR), both under the SAME scales"""
    ref, sc = reference(case, inp, given, calibrating=calibrating)
    rbf, rsc = reference(case, inp, sc.used, round_bf16=True, calibrating=calibrating)
    sc.own_rounded = rsc.own                         # (448 / max|tensor| of the rounded run's tensors: how far a maximum moves)
    return ref, sc, {n: max(BF16_FACTOR * rel_err(rbf[n], v), BF16_FLOOR) for n, v in ref.items()}


def slots_apart(case, sc):
    """-> the smallest ratio between the scales of two slots of the case that quantise DIFFERENT tensors (conv1's and the downsample
    conv's slots of a stride-1 block both quantise x: the one pair that cannot differ)"""
    names, worst = sorted(sc.used), float("inf")
    for i, a in enumerate(names):
        for b in names[i + 1:]:
            same = case["kind"] == "stage" and a.split(".")[0] == b.split(".")[0] and case["strides"][int(a[1])] == 1 \
                and {a.split(".", 1)[1], b.split(".", 1)[1]} == {"c1.act", "cd.act"}
            if not same:
                worst = min(worst, max(sc.used[a] / sc.used[b], sc.used[b] / sc.used[a]))
    return worst


def own_cap(case, inp, ref=None):
    """the cap on the model's own error (round_bf16 against exact, same scales) under which a draw is taken.  The issue's 3e-2
    (BF16_CAP) -- except for the ``deep`` cases, chains of six and seven quantised convolutions, where no draw meets it
    (tests/test_graph_fp8_ref_host.py says why): there the cap is stated as the quantisation's own effect on the case, the largest
    error over the compared tensors of the exact quantised model against the plain float64 module on the same inputs.  bf16 rounding
    in front of a quantiser can move a value by one code at the most, as the quantiser itself does: where the rounded model differs
    from the exact one by more than quantisation differs from none, something other than rounding is at work."""
    if not case["deep"]:
        return BF16_CAP
    ref = ref if ref is not None else reference(case, inp)[0]
    plain, _ = reference(case, inp, fp8=False)
    return max(rel_err(ref[n], plain[n]) for n in ref)


def pass_inputs(inp, pass_no):
    """the inputs of pass 1 (as drawn) or of passes 2 and 3: activations and the incoming gradient halved (exact in bf16; nothing
    saturates under the scales of pass 1).  Scaling is delayed: pass 2 still runs under the scales of pass 1's maxima, pass 3 under
    those of pass 2's, which are about twice as large for the node's input and for every gradient -- a copy made under the scale of
    pass 2 and read under that of pass 3 is then wrong by that factor, in the numbers as well as in the audit's book-keeping.  The
    cosine head's rows are normalised and its scale is fixed: only its gradient is halved."""
    if pass_no == 1:
        return inp
    out = dict(inp, gy=inp["gy"] * 0.5)
    for n in ("x", "feat", "extra"):
        if n in inp and "wn" not in inp:
            out[n] = inp[n] * 0.5
    return out


def prepared(case):
    """-> (inputs, exact quantised model of pass 2 under its own scales, its Scales, limits), once per case: the first draw of seed,
    seed + 1000, ... whose ReLUs keep graph_ref's margin, whose slots' scales are a factor of 2 apart and on which the model's own
    error (round_bf16 against exact, same scales) stays under BF16_CAP on every compared tensor; if none does the last is returned and
    the host test fails on its conditions.  All three are properties of the model alone."""
    for attempt in range(ATTEMPTS if case["name"] not in _cache else 0):
        inp = make_inputs(case, attempt)
        if inp["margin"] < G.MARGIN["gated"]:
            continue
        ref, sc, lim = limits(case, inp)
        _cache[case["name"]] = (inp, ref, sc, lim)
        cap = own_cap(case, inp, ref)
        if all(v <= BF16_FACTOR * cap for v in lim.values()) and (case["deep"] or slots_apart(case, sc) >= 2.0):
            break
    assert case["name"] in _cache, f"{case['name']}: no draw with the ReLU margin"
    return _cache[case["name"]]
