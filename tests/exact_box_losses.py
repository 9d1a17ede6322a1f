"""Exact references, per-element error bounds and the shared case list for the box-regression losses chosen by
MODEL.RPN / ROI_BOX_HEAD .BBOX_REG_LOSS_TYPE and .SMOOTH_L1_BETA: cddmsl_rpn_losses_reg / cddmsl_box_reg_loss of
cddmsl_amd/csrc/losses.hip (imported by test_box_losses_bound_host.py and test_gpu_box_losses.py; not a conftest).  Conventions,
constants and helpers are exact_losses.py's: operands as stored (f32), references in float64, scalars rounded to f32 first,
u = 2^-24, block_depth for the one-block sum, c_exp for expf, correctly rounded division, C_LOG for logf (inside get_deltas).

The bounds are DERIVED, not fitted: a first-order running bound.  ``V`` carries a float64 value v with a bound e of the error of its
f32 evaluation, and every f32 operation of the kernel is restated on it:
  a + b, a - b   e = e_a + e_b + u |v|                          (ABSOLUTE: what a cancellation leaves is the operands' errors --
                                                                 a1 + a2 - inter, ac - union, 1 - (...), 1 / ce against inter / ue^2)
  a * b          e = S2 (|a| e_b + |b| e_a) + u |v|             (S2 = 1.01 covers e_a e_b)
  a / b          e = S2 (e_a + |v| e_b) / |b| + C_DIV u |v|
  expf(a)        e = S2 |v| e_a + c_exp(a) |v|
  0.5 a, -a, a * share (0, 0.5, 1), a constant                  exact
  max, min, clamp, the intersection test                        the branch the float64 values take
Operands (boxes, deltas, f32 weights, eps = f32(1e-7), the clamp) are exact.  GIoU forward: Box2BoxTransform.apply_deltas
(box_regression.py:77-115) then fvcore's giou_loss; backward: the kernel's analytic gradient, restated operation by operation
(giou_ref).  The sum over the rows adds block_depth u sum|terms| and the final product u |loss|.

A GIoU row is DECIDED when each of its comparisons -- the four corner pairs (x1 : x1g, y1 : y1g, x2 : x2g, y2 : y2g), the two
intersection tests (xk2 > xk1, yk2 > yk1) and the two clamps (dw : scale_clamp, dh : scale_clamp) -- has a margin larger than the sum
of its operands' bounds: the f32 evaluation then takes the branch of the reference.  The gradient of a decided row is checked
against the bound.  The CONSTRUCTED rows meet some comparisons at exact equality on purpose, with operands that are exact in f32
and in float64 alike (small dyadic coordinates, zero deltas, expf(0) = 1, dw = d / w without a rounding); such a comparison counts
as decided, and the reference follows torch autograd's conventions there:
  max / min of two EQUAL operands hands HALF the gradient to the prediction,
  the clamp passes the gradient at dw == scale_clamp and blocks it above,
  a row whose intersection test fails (both comparisons strict) has no gradient through the intersection.
An undecided row outside the constructed ones must be finite and is otherwise skipped (its gradient is discontinuous there); at
most 1 % of a case's rows may be undecided, and the seeds are such that the reference alone leaves none.  The forward value is
continuous across every branch (taking the other branch moves it by less than the margin, which the bound already counts), so
the loss of every row is checked.

Smooth-L1 (fvcore): e = delta - get_deltas(src, tgt) with exact_losses.deltas_ref's bound e_b; n = |e|.  beta < 1e-5: exact_losses'
rpn_ref / box_ref apply unchanged (and the entry points return the bytes of cddmsl_rpn_losses / cddmsl_box_l1).  Otherwise
  term  n < beta ? 0.5 n n / beta : n - 0.5 beta    bound (n / beta) e_b + 3 u t   |   e_b + u t      (+ e_b^2 / 2 beta: the two
                                                    branches differ by (n - beta)^2 / 2 beta where e_b leaves the branch open)
  grad  n < beta ? e / beta : sgn(e), times gl      bound |gl| (e_b / beta + u |e / beta|) + u |g|; BIT FOR BIT sgn(e) gl where
                                                    n - beta > e_b decides the linear branch
The kernel-level cases use scale_clamp = 4.125 (log(1000 / 16) = 4.135..): 4.125 w is exact for the weights 0.5 and 5 of the case
lists, so ``dw == scale_clamp`` can be met exactly; the model-level tests and the reference fixture use Box2BoxTransform's value.
"""
import math

import torch

import exact_losses as E
from exact_losses import C_DIV, S2, TINY, U, block_depth, c_exp, f32  # noqa: F401

_f64 = E._f64
GIOU_EPS = f32(1e-7)
SCALE_CLAMP = math.log(1000.0 / 16)             # Box2BoxTransform's default
CLAMP_T = 4.125                                 # the kernel-level cases' clamp: see the docstring
MAX_UNDECIDED = 0.01


# ================================================================================================== running error arithmetic
class V:
    """a float64 value and a bound of the error of its f32 evaluation"""

    def __init__(self, v, e=None):
        self.v = v
        self.e = torch.zeros_like(v) if e is None else e

    def __add__(self, o):
        v = self.v + o.v
        return V(v, self.e + o.e + U * v.abs())

    def __sub__(self, o):
        v = self.v - o.v
        return V(v, self.e + o.e + U * v.abs())

    def __mul__(self, o):
        v = self.v * o.v
        return V(v, S2 * (self.v.abs() * o.e + o.v.abs() * self.e) + U * v.abs() + TINY)

    def __truediv__(self, o):
        v = self.v / o.v
        return V(v, S2 * (self.e + v.abs() * o.e) / o.v.abs() + C_DIV * U * v.abs() + TINY)

    def __neg__(self):
        return V(-self.v, self.e)

    def scale(self, k):
        """times an exact factor whose product needs no rounding: 0.5, or a share 0 / 0.5 / 1 (a tensor)"""
        return V(self.v * k, self.e * abs(k) if not torch.is_tensor(k) else self.e * k.abs())

    def exp(self):
        v = torch.exp(self.v)
        return V(v, S2 * v * self.e + c_exp(self.v) * v + TINY)

    def where(self, mask, o):
        return V(torch.where(mask, self.v, o.v), torch.where(mask, self.e, o.e))


def _const(like, c):
    return V(torch.full_like(like, float(c)))


def _gap(a, b, constructed):
    """is the comparison of a with b decided: a margin above the operands' bounds, or exact equality on a constructed row"""
    return ((a.v - b.v).abs() > a.e + b.e) | (constructed & (a.v == b.v))


def _share(p, g, hi):
    """share of the gradient max(p, g) (hi) / min(p, g) hands to p: 1, 0, or 0.5 at equality (torch.maximum / minimum backward)"""
    win = (p > g) if hi else (p < g)
    return torch.where(p == g, torch.full_like(p, 0.5), win.to(p.dtype))


def giou_ref(b, d, t, w, clamp, constructed=None, want_grad=True):
    """b (anchor / proposal), d (the row's four deltas), t (gt box): [n, 4] as stored -> dict(loss=(v, e) [n], grad=(v, e) [n, 4]
    = d loss / d delta before the gl factor, decided [n])"""
    b, d, t = _f64(b), _f64(d), _f64(t)
    n = b.shape[0]
    con = torch.zeros(n, dtype=torch.bool) if constructed is None else constructed
    wv = [_const(b[:, 0], f32(x)) for x in w]
    cl = _const(b[:, 0], f32(clamp))
    B, D, T = [V(b[:, i]) for i in range(4)], [V(d[:, i]) for i in range(4)], [V(t[:, i]) for i in range(4)]
    bw, bh = B[2] - B[0], B[3] - B[1]
    cx, cy = B[0] + bw.scale(0.5), B[1] + bh.scale(0.5)
    dx, dy, dw0, dh0 = D[0] / wv[0], D[1] / wv[1], D[2] / wv[2], D[3] / wv[3]
    over_w, over_h = dw0.v > cl.v, dh0.v > cl.v
    decided = _gap(dw0, cl, con) & _gap(dh0, cl, con)
    dw, dh = cl.where(over_w, dw0), cl.where(over_h, dh0)
    pcx, pcy = dx * bw + cx, dy * bh + cy
    pw, ph = dw.exp() * bw, dh.exp() * bh
    x1, y1, x2, y2 = pcx - pw.scale(0.5), pcy - ph.scale(0.5), pcx + pw.scale(0.5), pcy + ph.scale(0.5)
    P = (x1, y1, x2, y2)
    for p, g in zip(P, T):
        decided &= _gap(p, g, con)
    mx = lambda p, g: p.where(p.v > g.v, g)
    mn = lambda p, g: p.where(p.v < g.v, g)
    xk1, yk1, xk2, yk2 = mx(x1, T[0]), mx(y1, T[1]), mn(x2, T[2]), mn(y2, T[3])
    hit = (yk2.v > yk1.v) & (xk2.v > xk1.v)
    decided &= _gap(xk2, xk1, con) & _gap(yk2, yk1, con)
    iw, ih = xk2 - xk1, yk2 - yk1
    zero = _const(b[:, 0], 0.0)
    inter = (iw * ih).where(hit, zero)
    sw, sh = x2 - x1, y2 - y1
    uni = sw * sh + (T[2] - T[0]) * (T[3] - T[1]) - inter
    eps, one = _const(b[:, 0], GIOU_EPS), _const(b[:, 0], 1.0)
    ue = uni + eps
    iou = inter / ue
    xc1, yc1, xc2, yc2 = mn(x1, T[0]), mn(y1, T[1]), mx(x2, T[2]), mx(y2, T[3])
    cw, ch = xc2 - xc1, yc2 - yc1
    ac = cw * ch
    ce = ac + eps
    loss = one - (iou - (ac - uni) / ce)
    out = dict(loss=(loss.v, loss.e), decided=decided, hit=hit)
    if not want_grad:
        return out
    g_u = inter / (ue * ue) - one / ce
    g_i = (-(one / ue) - g_u).where(hit, zero)
    g_c = ue / (ce * ce)
    kx1, ky1, kx2, ky2 = _share(x1.v, T[0].v, True), _share(y1.v, T[1].v, True), _share(x2.v, T[2].v, False), _share(y2.v, T[3].v, False)
    ex1, ey1, ex2, ey2 = _share(x1.v, T[0].v, False), _share(y1.v, T[1].v, False), _share(x2.v, T[2].v, True), _share(y2.v, T[3].v, True)
    gx1 = -(g_u * sh) - (g_i * ih).scale(kx1) - (g_c * ch).scale(ex1)
    gx2 = (g_u * sh) + (g_i * ih).scale(kx2) + (g_c * ch).scale(ex2)
    gy1 = -(g_u * sw) - (g_i * iw).scale(ky1) - (g_c * cw).scale(ey1)
    gy2 = (g_u * sw) + (g_i * iw).scale(ky2) + (g_c * cw).scale(ey2)
    g0 = (gx1 + gx2) * bw / wv[0]
    g1 = (gy1 + gy2) * bh / wv[1]
    g2 = zero.where(over_w, (gx2 - gx1).scale(0.5) * pw / wv[2])
    g3 = zero.where(over_h, (gy2 - gy1).scale(0.5) * ph / wv[3])
    G = (g0, g1, g2, g3)
    out["grad"] = (torch.stack([g.v for g in G], 1), torch.stack([g.e for g in G], 1))
    return out


def sl1_ref(dsel, src, tgt, w, beta):
    """dsel [n, 4] the rows' deltas -> dict(term=(v, e), grad=(v, e) before the gl factor, linear [n, 4]: the linear branch decided)"""
    be = f32(beta)
    tg, e_tg = E.deltas_ref(src, tgt, w)
    e, eb = E._l1_parts(dsel, tg, e_tg)
    n = e.abs()
    quad = n < be
    t = torch.where(quad, 0.5 * n * n / be, n - 0.5 * be)
    tb = torch.where(quad, S2 * (n / be) * eb + 3 * U * t, eb + U * t) + eb * eb / (2 * be) + TINY
    g = torch.where(quad, e / be, torch.sign(e))
    gb = S2 * eb / be + U * g.abs() + TINY
    return dict(term=(t, tb), grad=(g, gb), linear=(n - be) > eb)


def _sum_bound(v, e, inn, depth):
    tot = v.sum() * inn
    return tot, S2 * inn * (e.sum() + depth * U * v.abs().sum()) + U * tot.abs() + TINY


def _rows_ref(dsel, src, tgt, w, inv_norm, loc, beta, clamp, gl, constructed, depth):
    """the regression half over the selected rows: forward (gl None) -> (loss, bound); backward -> dict(g, gb, exact, decided) [n, 4]"""
    inn = f32(inv_norm)
    n = dsel.shape[0]
    depth = block_depth(n) if depth is None else depth
    if loc == "giou":
        r = giou_ref(src, dsel, tgt, w, clamp, constructed, want_grad=gl is not None)
        if gl is None:
            return _sum_bound(r["loss"][0], r["loss"][1], inn, depth)
        g, gb = r["grad"]
        glv = _f64(gl)
        return dict(g=g * glv, gb=S2 * gb * glv.abs() + U * (g * glv).abs() + TINY, exact=torch.zeros(n, 4, dtype=torch.bool),
                    decided=r["decided"][:, None].expand(n, 4))
    r = sl1_ref(dsel, src, tgt, w, beta)
    if gl is None:
        return _sum_bound(r["term"][0], r["term"][1], inn, depth)
    g, gb = r["grad"]
    glv = _f64(gl)
    return dict(g=g * glv, gb=S2 * gb * glv.abs() + U * (g * glv).abs() + TINY, exact=r["linear"], decided=torch.ones(n, 4, dtype=torch.bool))


def _con_mask(n, ncon):
    m = torch.zeros(n, dtype=torch.bool)
    m[:ncon] = True
    return m


def rpn_reg_ref(a, loc, beta, clamp, gout=None, ncon=0, depth=None):
    """a: the operands of exact_losses.rpn_ref -> the loc half.  forward: (loss, bound); backward: dict(g, gb, exact, decided) over pos"""
    pos, A = a["pos"], a["A"]
    img = torch.div(pos, A, rounding_mode="floor")
    src, tgt = a["anchors"][pos - img * A], a["gt"][a["midx"][pos] + a["gt_off"][img]]
    gl = None if gout is None else gout.float()[1] * torch.tensor(f32(a["inv_norm"]), dtype=torch.float32)
    return _rows_ref(a["deltas"][pos], src, tgt, a["w"], a["inv_norm"], loc, beta, clamp, gl, _con_mask(pos.numel(), ncon), depth)


def box_cols(a):
    fg, cls = a["fg"], a["cls"]
    c0 = 4 * cls[fg] if cls is not None else torch.zeros_like(fg)
    return c0[:, None] + torch.arange(4)[None, :]


def box_reg_ref(a, loc, beta, clamp, gout=None, ncon=0, depth=None):
    fg = a["fg"]
    gl = None if gout is None else gout.float().reshape(()) * torch.tensor(f32(a["inv_norm"]), dtype=torch.float32)
    return _rows_ref(a["deltas"][fg[:, None], box_cols(a)], a["src"][fg], a["tgt"][fg], a["w"], a["inv_norm"], loc, beta, clamp, gl,
                     _con_mask(fg.numel(), ncon), depth)


# ================================================================================================== the shared case list
LOCS = (("giou", 0.0), ("smooth_l1", 1.0 / 9), ("smooth_l1", 1.0), ("smooth_l1", 0.0))
RPN_N, RPN_A = 3, 400
RPN_W = E.RPN_W                                                  # (2.0, 1.5, 0.5, 3.0)
BOX_KC, BOX_W = E.BOX_KC, E.BOX_W                                # 5, (10, 10, 5, 5)
ROW_MATCH, ROW_EDGE, ROW_TOUCH, ROW_CLAMP_EQ, ROW_CLAMP_OVER, ROW_TINY, ROW_INSIDE = range(7)
NCON = 7


def constructed_rows(w):
    """(box, gt, deltas) of the constructed rows: every operand of every comparison they make is exact in f32 and in float64.
    MATCH: box == gt, deltas 0 (all four corners tie).  EDGE: x1 == x1g only.  TOUCH: x2 == x1g, the boxes overlap in y (the strict
    intersection test fails).  CLAMP_EQ: dw == the clamp exactly.  CLAMP_OVER: dw, dh above it.  TINY: sides 1/16 next to the origin (eps = 1e-7
    is 2.6e-5 of the areas, 400 u).  INSIDE: the gt box inside the prediction"""
    box = torch.tensor([[16., 24, 48, 72], [16, 24, 48, 72], [16, 24, 48, 72], [16, 24, 18, 26], [16, 24, 18, 26],
                        [0.0625, 0.0625, 0.125, 0.125], [16, 24, 48, 72]])
    gt = torch.tensor([[16., 24, 48, 72], [16, 30, 60, 80], [48, 40, 90, 100], [0, 10, 100, 60], [0, 10, 100, 60],
                       [0.09375, 0.078125, 0.15625, 0.140625], [20, 30, 40, 60]])
    d = torch.zeros(NCON, 4)
    d[ROW_CLAMP_EQ, 2] = w[2] * CLAMP_T
    d[ROW_CLAMP_OVER, 2], d[ROW_CLAMP_OVER, 3] = w[2] * 6.0, w[3] * 5.0
    return box, gt, d


def _deltas(n, w, seed):
    """unit-normal deltas under the weights (10, 10, 5, 5), whatever the weights are: dx, dy of spread 0.1 and dw, dh of 0.2"""
    return E._randn((n, 4), seed) * torch.tensor([0.1 * w[0], 0.1 * w[1], 0.2 * w[2], 0.2 * w[3]])


def _f32_get_deltas(s, t, w):
    sw, sh = s[:, 2] - s[:, 0], s[:, 3] - s[:, 1]
    sx, sy = s[:, 0] + 0.5 * sw, s[:, 1] + 0.5 * sh
    tw, th = t[:, 2] - t[:, 0], t[:, 3] - t[:, 1]
    tx, ty = t[:, 0] + 0.5 * tw, t[:, 1] + 0.5 * th
    return torch.stack([w[0] * (tx - sx) / sw, w[1] * (ty - sy) / sh, w[2] * torch.log(tw / sw), w[3] * torch.log(th / sh)], 1)


def rpn_cases():
    return [dict(npos=a, nneg=b, loc=l, beta=be) for a, b in ((0, 0), (1, 0), (0, 7), (255, 0), (256, 0), (257, 0), (600, 400))
            for l, be in LOCS]


def box_cases():
    shapes = [(320, n, "specific") for n in (0, 1, 255, 256, 257, 300)] + [(320, 300, "specific_padded"), (320, 300, "agnostic"),
                                                                          (1200, 1000, "specific")]
    return [dict(R=R, nfg=n, form=f, loc=l, beta=be) for R, n, f in shapes for l, be in LOCS]


def rpn_inputs(c):
    """N = 3 images of A = 400 anchors; image 0 has 8 boxes (the first NCON are the constructed rows', matched by anchors 0..6, which
    are the first positives), image 1 none, image 2 four.  A third of the positives sit within beta of their target"""
    N, A, npos, nneg = RPN_N, RPN_A, c["npos"], c["nneg"]
    g = E._g(161 + npos + nneg)
    anchors, gt = E._boxes(A, 162), E._boxes(12, 163)
    gt_off = torch.tensor([0, 8, 8])
    midx = torch.zeros(N, A, dtype=torch.int64)
    midx[0] = torch.randint(0, 8, (A,), generator=g)
    midx[2] = torch.randint(0, 4, (A,), generator=g)
    forced = torch.arange(NCON)
    cand = torch.cat([torch.arange(NCON, A), 2 * A + torch.arange(A)])
    cand = cand[torch.randperm(cand.numel(), generator=g)]
    pos = torch.cat([forced, cand])[:npos]
    rest = torch.arange(N * A)
    rest = rest[~torch.isin(rest, pos)]
    neg = rest[torch.randperm(rest.numel(), generator=g)[:nneg]]
    logits = E._randn((N * A,), 164, 3.0)
    deltas = _deltas(N * A, RPN_W, 165)
    cb, cg, cd = constructed_rows(RPN_W)
    anchors[:NCON], gt[:NCON], deltas[:NCON] = cb, cg, cd
    midx[0, :NCON] = torch.arange(NCON)
    if c["loc"] == "smooth_l1" and npos > NCON:
        near = pos[NCON::3]
        img = torch.div(near, A, rounding_mode="floor")
        tg = _f32_get_deltas(anchors[near - img * A], gt[midx.view(-1)[near] + gt_off[img]], RPN_W)
        deltas[near] = tg + E._randn(tuple(tg.shape), 166, 0.05)
    return dict(logits=logits, deltas=deltas, pos=pos, neg=neg, midx=midx.view(-1), gt=gt, gt_off=gt_off, anchors=anchors, A=A, w=RPN_W,
                inv_norm=1.0 / (256.0 * N)), min(npos, NCON)


def box_inputs(c):
    R, Kc, nfg = c["R"], BOX_KC, c["nfg"]
    ld = {"specific": 4 * Kc, "specific_padded": 4 * Kc + 4, "agnostic": 4}[c["form"]]
    g = E._g(171 + nfg + R)
    cls = None if c["form"] == "agnostic" else torch.randint(0, Kc, (R,), generator=g)
    deltas = E._randn((R, ld), 172 + ld)
    fg = torch.cat([torch.arange(NCON), NCON + torch.randperm(R - NCON, generator=g)])[:nfg].sort().values
    src, tgt = E._boxes(R, 173), E._boxes(R, 174)
    cb, cg, cd = constructed_rows(BOX_W)
    ncon = min(nfg, NCON)
    src[:NCON], tgt[:NCON] = cb, cg
    a = dict(deltas=deltas, fg=fg, cls=cls, src=src, tgt=tgt, w=BOX_W, inv_norm=1.0 / R)
    cols = box_cols(a)
    own = _deltas(R, BOX_W, 175)[fg]
    if c["loc"] == "smooth_l1" and nfg > NCON:
        tg = _f32_get_deltas(src[fg], tgt[fg], BOX_W)
        own[NCON::3] = (tg + E._randn(tuple(tg.shape), 176, 0.05))[NCON::3]
    own[:ncon] = cd[:ncon]
    deltas[fg[:, None], cols] = own
    return a, ncon


def _loc_checks(rep, name, t, dd_rows, ref, c, ncon, own_zero=True):
    """dd_rows [n, 4]: the gradient at the rows' own four columns.  own_zero: the kernel's exact zero at the matching row (another
    evaluation order of the same gradient, such as autograd's, need not cancel to the last bit there)"""
    g32 = ref["g"].to(torch.float32)
    ex, dec = ref["exact"], ref["decided"]
    n = dd_rows.shape[0]
    rep.exact(name, t, bool(torch.isfinite(dd_rows).all()), "a gradient is not finite")
    rep.exact(name, t, bool((dd_rows[ex] == g32[ex]).all()), "the linear branch is not sgn(e) * f32(gout * inv_norm) bit for bit")
    m = dec & ~ex
    rep.bound(name, t, dd_rows[m], (ref["g"][m], ref["gb"][m]))
    und = int((~dec[:, 0]).sum()) if n else 0
    rep.exact(name, t, und <= MAX_UNDECIDED * n, f"{und} of {n} rows are undecided (more than 1 %)")
    if c["loc"] == "giou" and ncon > ROW_MATCH and own_zero:
        rep.exact(name, t, bool((dd_rows[ROW_MATCH, :2] == 0).all()), "the dx / dy gradient of the exactly matching row is not 0")
    if c["loc"] == "giou" and ncon > ROW_CLAMP_OVER:
        rep.exact(name, t, bool((dd_rows[ROW_CLAMP_OVER, 2:] == 0).all()), "a gradient passed a clamped dw / dh")
        rep.exact(name, t, bool(dd_rows[ROW_CLAMP_EQ, 2] != 0), "the clamp blocked the gradient at dw == scale_clamp")


# ================================================================================================== drivers
# ``impl``: rpn_reg(**operands, loc, beta, clamp, gout) / box_reg(...) next to exact_losses' rpn(...) / box(...) (the entry points of
# today), CPU tensors in and out -- the C-ABI on the GPU, the f32 emulation or one of its mutants on the CPU.
def run_rpn_reg(c, impl, rep):
    t = E.tag(c)
    a, ncon = rpn_inputs(c)
    loc, beta = c["loc"], c["beta"]
    gout = torch.tensor([1.5, 0.7])
    out2 = impl.rpn_reg(**a, loc=loc, beta=beta, clamp=CLAMP_T)
    again = impl.rpn_reg(**a, loc=loc, beta=beta, clamp=CLAMP_T)
    rep.exact("rpn_losses_reg out2", t, E.bits_equal(out2, again), "the forward is not bit-equal when repeated")
    dl, dd = impl.rpn_reg(**a, loc=loc, beta=beta, clamp=CLAMP_T, gout=gout)
    old_f, (old_dl, old_dd) = impl.rpn(**a), impl.rpn(**a, gout=gout)
    rep.exact("rpn_losses_reg out2", t, E.bits_equal(out2[:1], old_f[:1]), "loss_rpn_cls is not cddmsl_rpn_losses' bit for bit")
    rep.exact("rpn_losses_reg dlogits", t, E.bits_equal(dl, old_dl), "dlogits is not cddmsl_rpn_losses' bit for bit")
    isp = torch.zeros(a["logits"].numel(), dtype=torch.bool)
    isp[a["pos"]] = True
    rep.exact("rpn_losses_reg ddeltas", t, E.pos_zero(dd[~isp]), "an entry outside the positives is not exactly +0")
    if loc == "smooth_l1" and beta == 0.0:
        rep.exact("rpn_losses_reg beta 0", t, E.bits_equal(out2, old_f) and E.bits_equal(dd, old_dd), "not the bytes of cddmsl_rpn_losses")
        return
    name = f"rpn_losses_reg {loc}" + (f" beta {beta:.3g}" if loc == "smooth_l1" else "")
    rep.bound(name + " loss", t, out2[1:], tuple(x.reshape(1) for x in rpn_reg_ref(a, loc, beta, CLAMP_T)))
    _loc_checks(rep, name + " ddeltas", t, dd[a["pos"]], rpn_reg_ref(a, loc, beta, CLAMP_T, gout=gout, ncon=ncon), c, ncon)


def run_box_reg(c, impl, rep):
    t = E.tag(c)
    a, ncon = box_inputs(c)
    loc, beta = c["loc"], c["beta"]
    gout = torch.tensor([0.7])
    out1 = impl.box_reg(**a, loc=loc, beta=beta, clamp=CLAMP_T)
    again = impl.box_reg(**a, loc=loc, beta=beta, clamp=CLAMP_T)
    rep.exact("box_reg_loss out1", t, E.bits_equal(out1, again), "the forward is not bit-equal when repeated")
    dd = impl.box_reg(**a, loc=loc, beta=beta, clamp=CLAMP_T, gout=gout)
    cols = box_cols(a)
    touched = torch.zeros(a["deltas"].shape, dtype=torch.bool)
    touched[a["fg"][:, None], cols] = True
    rep.exact("box_reg_loss ddeltas", t, E.pos_zero(dd[~touched]), "an entry outside the foreground rows' class columns is not exactly +0")
    if loc == "smooth_l1" and beta == 0.0:
        same = E.bits_equal(out1, impl.box(**a)) and E.bits_equal(dd, impl.box(**a, gout=gout))
        rep.exact("box_reg_loss beta 0", t, same, "not the bytes of cddmsl_box_l1")
        return
    name = f"box_reg_loss {loc}" + (f" beta {beta:.3g}" if loc == "smooth_l1" else "")
    rep.bound(name + " loss", t, out1, tuple(x.reshape(1) for x in box_reg_ref(a, loc, beta, CLAMP_T)))
    _loc_checks(rep, name + " ddeltas", t, dd[a["fg"][:, None], cols], box_reg_ref(a, loc, beta, CLAMP_T, gout=gout, ncon=ncon), c, ncon)


FAMILIES = (("rpn_reg", rpn_cases, run_rpn_reg), ("box_reg", box_cases, run_box_reg))
