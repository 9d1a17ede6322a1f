"""Exact reference, per-element error bounds and the shared case list of the grouped SGD step (cddmsl_sgd_step_groups: k_gnorm /
k_sgd_groups of elementwise.hip); imported by test_solver_host.py and test_gpu_solver.py, not a conftest.  The conventions are those
of exact_losses.py, whose helpers it uses: operands as stored (f32), the reference in float64, scalars rounded to f32 first (they
cross the C-ABI as float, the per-tensor lr / weight decay included), u = 2^-24, factor 1.01 for the second-order terms, TINY below
the normal range.  Ground truth is torch itself: test_solver_host.py checks groups_ref against torch.optim.SGD(per-parameter groups)
after clip_grad_value_ / clip_grad_norm_ per parameter, in float64.

Per tensor i and element, with c the clip value:
  mode 0  gc = g                                                   no rounding
  mode 1  gc = min(max(g, -c), c)                                  no rounding: checked through m on a first step with wd_i = 0, where
                                                                   buf = gc bit for bit (as a value: -0 + 0 = +0)
  mode 2  s = sum g^2, relative (depth + 1) u as k_sqnorm;  coef = min(c / (sqrt s + 1e-6), 1): r = r_s / 2 + (C_SQRT + 1 + C_DIV) u
  mode 3  s = sum |g|, relative depth u (bounded at mode 2's depth);  coef: r = r_s + (1 + C_DIV) u
  mode 4  s = max |g|: no rounding, norm_ws is checked BIT FOR BIT;  coef: r = (1 + C_DIV) u
  modes 2-4: gc = g coef: |g| e_coef + u |gc|
  d = gc + wd_i p:                     e_d = e_gc + u (|wd_i p| + |d|)
  buf = d  or  momentum buf + d:       e_m = e_d + u (|momentum buf| + |buf'|)
  step = buf'  or  d + momentum buf':  e_s = e_d + momentum e_m + u (|momentum buf'| + |step|)
  p' = p - lr_i step:                  e_p = lr_i e_s + u (|lr_i step| + |p'|)
each rounding counted once.  A NaN gradient element (modes 3 and 4) is not a bound but a convention: norm_ws[i] and every element of
p_i and buf_i are NaN, and the tensors around it pass their bounds."""
import torch

import exact_losses as E
from exact_losses import C_DIV, C_SQRT, S2, TINY, U, Report, _f64, _randn, bits_equal, f32, sgd_layout, sgd_views, tag  # noqa: F401

SGDG_MAX = 80                       # tensors per launch (SgdGBatch)
NONE, VALUE, L2, L1, INF = range(5)
CLIP = 1e-2
NAMES = ("none", "value", "l2", "l1", "inf")


def groups_grid(sizes):
    """grid.x of each tensor's launches: gsz(max size of its batch of SGDG_MAX, 2048 elements per block, cap 256)"""
    out = []
    for b0 in range(0, len(sizes), SGDG_MAX):
        mx = max(sizes[b0:b0 + SGDG_MAX])
        out += [min(256, max(1, (mx + 2047) // 2048))] * len(sizes[b0:b0 + SGDG_MAX])
    return out


def groups_ref(ps, gs, ms, lrs, wds, momentum, nesterov, mode, clip, first_step, exact_scalars=False):
    """lists of 1-D tensors (as stored before the step) -> list of dict(norm=(e, b) or None, p=(e, b), m=(e, b)).  exact_scalars: take
    the scalars and the 1e-6 as the doubles given (for the comparison with torch in float64), not rounded to f32"""
    r32 = (lambda v: v) if exact_scalars else f32
    mo, clip, eps = r32(momentum), r32(clip), r32(1e-6)
    out = []
    for p, g, m, lr, wd, gx in zip(ps, gs, ms, lrs, wds, groups_grid([p.numel() for p in ps])):
        p, g, lr, wd = _f64(p), _f64(g), r32(lr), r32(wd)
        n = p.numel()
        norm = None
        if mode == NONE:
            gc, e_gc = g, torch.zeros_like(g)
        elif mode == VALUE:
            gc, e_gc = g.clamp(-clip, clip), torch.zeros_like(g)
        else:
            depth = (n + gx * 256 - 1) // (gx * 256) + 3 + 6 + 3 + gx + 1
            if mode == L2:
                s = (g * g).sum()
                r_s = S2 * depth * U
                nrm, r_n = s.sqrt(), r_s / 2 + C_SQRT * U
            elif mode == L1:
                s = g.abs().sum()
                r_s = S2 * depth * U
                nrm, r_n = s, r_s
            else:
                s = g.abs().max()
                r_s = 0.0
                nrm, r_n = s, 0.0
            coef = (clip / (nrm + eps)).clamp(max=1.0)
            e_coef = S2 * (r_n + (1 + C_DIV) * U) * coef
            gc = g * coef
            e_gc = g.abs() * e_coef + U * gc.abs()
            norm = (s.reshape(1), (r_s * s + TINY).reshape(1))
        d = gc + wd * p
        e_d = e_gc + U * ((wd * p).abs() + d.abs())
        if first_step:
            m2, e_m = d, e_d
        else:
            mm = mo * _f64(m)
            m2 = mm + d
            e_m = e_d + U * (mm.abs() + m2.abs())
        if nesterov:
            la = mo * m2
            st = d + la
            e_s = e_d + mo * e_m + U * (la.abs() + st.abs())
        else:
            st, e_s = m2, e_m
        p2 = p - lr * st
        e_p = lr * e_s + U * ((lr * st).abs() + p2.abs())
        out.append(dict(norm=norm, m=(m2, S2 * e_m + TINY), p=(p2, S2 * e_p + TINY)))
    return out


# ================================================================================================== the shared case list
COUNTS = ((1, False), (4, True), (SGDG_MAX, False), (SGDG_MAX + 1, False), (2 * SGDG_MAX + 1, False))
COMBOS = ((0.9, 0), (0.9, 1), (0.0, 0))          # (momentum, nesterov); Nesterov needs a momentum
LRS = (0.02, 0.013, 0.002)                       # the base lr of the three steps
LR_FACTORS = (1.0, 2.0, 0.5)                     # tensor i: i % 3
WDS = (1e-4, 0.0, 5e-4, 0.0, 1e-3, 2e-4, 0.0)    # tensor i: i % 7
TARGETS = (300.0, 2.0, 0.3, 0.0, 7.0)            # tensor i: the gradient's norm (of the mode) over the clip, i % 5
NAN_TENSOR = 1


def groups_cases():
    """every mode at every count (1, 4 with four tensors of about 2^20 elements, B, B + 1, 2 B + 1), the (momentum, nesterov) pair
    rotating so that every mode meets each; a NaN gradient element under the inf norm and under the L1 norm"""
    out = [dict(mode=mode, count=count, big=big, mo=COMBOS[(mode + ci) % 3][0], nesterov=COMBOS[(mode + ci) % 3][1], nan=False)
           for mode in range(5) for ci, (count, big) in enumerate(COUNTS)]
    out += [dict(mode=mode, count=4, big=False, mo=0.9, nesterov=1, nan=True) for mode in (INF, L1)]
    return out


def groups_tag(c):
    return tag(dict(c, mode=NAMES[c["mode"]]))


def _mode_norm(g, mode):
    if mode in (NONE, L2):
        return g.norm()
    return g.abs().sum() if mode == L1 else g.abs().max()


def groups_buffers(c, lay, total):
    """p, g flat buffers with NaN between the tensors; per tensor the gradient's norm (the mode's own: the largest magnitude for the
    value clamp) far above the clip, around it (twice), below it, and zero"""
    p = torch.full((total,), float("nan"))
    g = torch.full((total,), float("nan"))
    for i, (n, op, og, om) in enumerate(lay):
        p[op:op + n] = _randn((n,), 182 + i)
        gi = _randn((n,), 183 + i)
        target = TARGETS[i % 5] * CLIP
        g[og:og + n] = gi / _mode_norm(gi, c["mode"]).clamp_min(1e-30) * target
        if c["nan"] and i == NAN_TENSOR:
            g[og + n // 2] = float("nan")
    return p, g


def groups_scalars(c, step):
    n = c["count"]
    return [LRS[step] * LR_FACTORS[i % 3] for i in range(n)], [WDS[i % 7] for i in range(n)]


def run_groups(c, impl, rep):
    """three steps (the first without a buffer: the momentum is NaN-filled) of ``impl.sgd_groups`` against groups_ref"""
    t, mode, count = groups_tag(c), c["mode"], c["count"]
    lay, total = sgd_layout(c)
    p, g = groups_buffers(c, lay, total)
    m = torch.full((total,), float("nan"))                       # first_step = 1 must not read the momentum
    ws = torch.full((count + 4,), 12345.0)                       # garbage: the norm modes zero what they use
    inside_p, inside_m = torch.zeros(total, dtype=torch.bool), torch.zeros(total, dtype=torch.bool)
    for n, op, og, om in lay:
        inside_p[op:op + n] = True
        inside_m[om:om + n] = True
    good = [i for i in range(count) if not (c["nan"] and i == NAN_TENSOR)]
    for step in range(3):
        first = int(step == 0)
        lrs, wds = groups_scalars(c, step)
        p2, m2, ws2 = impl.sgd_groups(lay, p, g, m, ws, lrs, wds, c["mo"], c["nesterov"], mode, CLIP, first)
        ref = groups_ref(sgd_views(p, lay, 1), sgd_views(g, lay, 2), sgd_views(m, lay, 3), lrs, wds, c["mo"], c["nesterov"], mode, CLIP, first)
        s = f"step {step + 1}"
        rep.exact("sgd_step_groups p", t, bits_equal(p2[~inside_p], p[~inside_p]), f"{s}: an element between the tensors was written")
        rep.exact("sgd_step_groups m", t, bits_equal(m2[~inside_m], m[~inside_m]), f"{s}: an element between the tensors was written")
        pv, mv, gv = sgd_views(p2, lay, 1), sgd_views(m2, lay, 3), sgd_views(g, lay, 2)
        if mode < L2:
            rep.exact("sgd_step_groups norm_ws", t, bits_equal(ws2, ws), f"{s}: norm_ws written without a norm mode")
        else:
            rep.exact("sgd_step_groups norm_ws", t, bits_equal(ws2[count:], ws[count:]), f"{s}: norm_ws written past count")
            if mode == INF:
                want = torch.stack([gv[i].abs().max() for i in good])
                rep.exact("sgd_step_groups norm_ws", t, bits_equal(ws2[good], want), f"{s}: the inf norm is not max |g| bit for bit")
            else:
                rep.bound(f"sgd_step_groups norm_ws {NAMES[mode]}", f"{t} {s}", ws2[good],
                          (torch.cat([ref[i]["norm"][0] for i in good]), torch.cat([ref[i]["norm"][1] for i in good])))
        if c["nan"]:
            i = NAN_TENSOR
            rep.exact("sgd_step_groups norm_ws", t, bool(torch.isnan(ws2[i])), f"{s}: a NaN gradient element is lost from norm_ws")
            rep.exact("sgd_step_groups p", t, bool(torch.isnan(pv[i]).all()), f"{s}: the tensor with a NaN gradient element is not all NaN")
            rep.exact("sgd_step_groups m", t, bool(torch.isnan(mv[i]).all()), f"{s}: the buffer of the tensor with a NaN gradient is not all NaN")
        if first and mode < L2:
            for i in good:
                if wds[i] == 0.0:
                    want = gv[i] if mode == NONE else gv[i].clamp(-f32(CLIP), f32(CLIP))
                    rep.exact("sgd_step_groups m", t, torch.equal(mv[i], want), f"{s}: tensor {i}: buf is not the (clamped) gradient exactly")
        cat = lambda k: (torch.cat([ref[i][k][0] for i in good]), torch.cat([ref[i][k][1] for i in good]))
        rep.bound("sgd_step_groups p", f"{t} {s}", torch.cat([pv[i] for i in good]), cat("p"))
        rep.bound("sgd_step_groups m", f"{t} {s}", torch.cat([mv[i] for i in good]), cat("m"))
        p, m, ws = p2, m2, ws2
