"""Exact references and per-element error bounds for RoIAlign (cddmsl_amd/csrc/roi_align.hip), imported by the RoI tests; not a
conftest.  Everything is torch float64 on the device of its inputs.  Units: u = 2^-24 (f32), u_b = 2^-8 (a round-to-nearest-even
bf16 store), TINY = 2^-126 (results below the normal range), as tests/exact_attn.py.

Geometry (roi_geom, axis_tap) starts from the f32 RoI fields and the f32 spatial_scale the kernel receives; a product of two f32
numbers is exact in float64, so sample coordinates, bin sizes and weights are exact here (to 2^-53):
  y0 = r2 * scale - off, y1 = r4 * scale - off, rh = y1 - y0 (floored at 1 when not aligned), bh = rh / ph,
  gh = sampling_ratio or ceil(rh / ph),  sample (i, iy) at  y = y0 + i bh + (iy + 0.5) bh / gh,
  valid for -1 <= y <= L; y <= 0 -> 0; lo = floor(y); lo >= L-1 -> lo = hi = L-1 (y = lo); wh = y - lo, wl = 1 - wh;
  count = max(gh gw, 1); a RoI whose batch index is outside [0, N) pools to zero (before the affine).

C_GEO.  The kernel evaluates the same expressions in f32; every rounding is at most u times the magnitude of its result, and every
magnitude is at most M = max(1, |y0| + |rh|).  In units of u M:
  y0, y1: a product and a subtraction, 2 each       rh = y1 - y0: 2 + 2 + 1 = 5        bh = rh / ph: (5 + 1) / ph
  i bh (i < ph): 6 + 1 = 7                           y0 + i bh: 2 + 7 + 1 = 10
  (iy + 0.5) bh / gh (iy + 0.5 <= gh): (6 / ph + 1 / ph) + 1 / ph <= 8          the last sum: 10 + 8 + 1 = 19
A fused multiply-add removes roundings and adds none.  C_GEO = 20 covers the 19 and their second-order products ((1 + u)^19).
A kernel coordinate is thus within  delta = C_GEO u max(1, |y0| + |rh|)  of the exact one (likewise along x).  delta is taken as 0 for
a RoI axis whose every f32 intermediate of the list above is exact (checked here by evaluating the chain in f32 next to float64): then
the kernel computes the exact coordinates whatever the contraction, and the window tests are decided exactly.  delta enters three ways:
  coordinate term   bilinear interpolation is continuous and piecewise linear in each coordinate (also across the clamp at 0 and the
                    snap at L-1: both are continuous), so a pooled value moves by at most  delta_y slope_y + delta_x slope_x,  the
                    slopes = the largest |difference| of vertically / horizontally adjacent pixels over the RoI's clamped
                    footprint dilated by one pixel, per channel
  ambiguous samples a sample within delta of -1 or of L may be counted or dropped: its whole absolute contribution
                    bilinear(|x|) / count goes into the bound of its bin
  ambiguous grid    a RoI whose exact rh / ph (rw / pw) is within C_GEO u max(1, q, M / ph) of an integer q could get either grid
                    size (rh carries 5 u M, the division one more rounding): geometry() flags it, and the case tables must hold none

Forward (k_roi_align_fwd tap by tap: acc += w1 v1 + w2 v2 + w3 v3 + w4 v4, w = wy wx; k_roi_align_fwd_rows: R = sum wy x over the
merged rows, acc = sum wx R; then one division or multiplication by the count).  Weights are nonnegative, so sum |w x| = pool(|x|).
Per term: wl = 1 - wh (1 rounding), wy wx (or the merged row weight) (1), the product with x (1), the division (1), and a sum of
n = 4 gh gw terms in any order (n - 1): (n + 3) u pool(|x|) <= the bound's  (4 gh gw + 8) u pool(|x|):
  pre_v = (4 gh gw + 8) u pool(|x|) + coordinate term + ambiguous term
  y = relu?(s v + b)  (one fma in the bf16 kernels; a multiply and an add in the f32 one, whose extra u |s v| is inside the 5 u
                       pool(|x|) >= 5 u |v| the line above leaves over):   pre = |s| pre_v + u (|s v| + |b|); relu is 1-Lipschitz
  store: exact_attn.store_bound: u_out |y| + (1 + u_out) pre + TINY
  pooled-only output (k_roi_align_fwd_rows<2>): the mean of four unrounded bins = one pooling with count 4 gh gw: the same form with
                       (16 gh gw + 8); coordinate and ambiguous terms are the means of the four bins'
  pooled by-product of the tap kernel (with_pooled): T(((a0 + a1) + (a2 + a3)) * 0.25f) of the four STORED crops: pooled_of_stored,
                       bit for bit in torch f32 arithmetic
  y8 = e4m3(clamp(y q8, +-448)) of the unrounded y (one more f32 rounding for the product): check_e4m3 accepts
                       |deq(y8) - clamp(exact q8)| <= half an e4m3 ulp (at |exact q8| + its error) + q8 pre + u |exact q8|: where the
                       error interval straddles a rounding boundary either neighbouring code passes
  amax8: max over the slots of the unrounded |y|: max(|y| - pre) <= amax8 <= max(|y| + pre)  (check_amax)

Backward (k_roi_tables, k_roi_align_bwd): exact tables  Ay[k][i][y] = (1 / gh) sum of wy over the samples of bin i  (Ax likewise);
dx[n, y, x, :] = sum over the RoIs of image n and bins (i, j) of Ay Ax dy.  fold = 2 (the gradient of the 2x2-average-pooled map):
table column i collects bins 2i, 2i + 1 of the 2 ph x 2 pw grid at half weight.
  pre = sum |dy| ((Ay + ey)(Ax + ex) - Ay Ax) + (n_terms + 2 (sh + sw) + 4) u sum Ay Ax |dy|
  ey / ex  2 delta on the rows / columns of the RoI's footprint dilated by one pixel (a sample moved by delta changes each of its two
           weights by delta; an entry is a mean over the samples), 0 elsewhere; plus the weight share of every ambiguous sample
  sh, sw   samples per table column, fold gh and fold gw: an entry is a sum of at most sh terms wl / gh, each with the rounding of wl
           and of the division (the factor 1 / fold is exact), doubled where the snap sends both taps to one row: (2 sh + 2) + (2 sw +
           2) + 1 for the product Ay Ax, and
  n_terms  the (RoI, bin) pairs with nonzero exact weight at the pixel, added one after another in f32 (n_terms - 1 roundings)
  then the store term, as above.
"""
import math

import torch

import exact_attn as A
import exact_gemm as X
from exact_attn import TINY, check, store_bound  # noqa: F401  (check: re-exported for the tests)
from exact_gemm import U_BF16, U_F32, round_bf16, rounding_bias  # noqa: F401

_f64 = X._f64

C_GEO = 20.0


def u_out(dtype):
    return U_BF16 if dtype == torch.bfloat16 else U_F32


# ---------------------------------------------------------------------------------------------------------------- geometry
def _taps(v, L):
    """one axis of the bilinear tap in float64 -> valid, lo, hi (int64), wl, wh"""
    valid = (v >= -1.0) & (v <= float(L))
    vc = v.clamp(0.0, float(L))
    fl = vc.floor()
    snap = fl >= L - 1
    lo = torch.where(snap, torch.full_like(fl, L - 1), fl)
    vc = torch.where(snap, lo, vc)
    hi = torch.where(snap, lo, lo + 1)
    wh = vc - lo
    return valid, lo.long(), hi.long(), 1.0 - wh, wh


def _table(lo, hi, wl, wh, keep, g, L):
    """[K, P, L] mean weight of pixel row l over the kept samples of bin p (divided by the grid size g [K])"""
    K, P, G = lo.shape
    w = keep.to(torch.float64) / g.clamp_min(1).to(torch.float64).view(K, 1, 1)
    t = torch.zeros(K, P, L, dtype=torch.float64, device=lo.device)
    t.scatter_add_(2, lo, wl * w)
    t.scatter_add_(2, hi, wh * w)
    return t


def _axis(r0, r1, scale, P, L, sr, aligned):
    """one axis of every RoI: r0, r1 f32 [K] (box corners in input pixels), P bins over L pixels.  -> dict: g [K] grid size, a0, ext,
    delta [K], amb_grid [K] bool, T / Tmin / Tmax [K, P, L] (exact table; without / with every ambiguous sample), namb [K, P]"""
    dev = r0.device
    K = r0.numel()
    s32 = torch.tensor(scale, dtype=torch.float32, device=dev)
    off = 0.5 if aligned else 0.0
    p0, p1 = _f64(r0) * _f64(s32), _f64(r1) * _f64(s32)
    a0, a1 = p0 - off, p1 - off
    ext = a1 - a0
    if not aligned:
        ext = ext.clamp_min(1.0)
    q = ext / P
    M = (a0.abs() + ext.abs()).clamp_min(1.0)
    if sr > 0:
        g = torch.full((K,), int(sr), dtype=torch.int64, device=dev)
        amb_grid = torch.zeros(K, dtype=torch.bool, device=dev)
    else:
        g = torch.ceil(q).long().clamp_min(0)
        qi = torch.round(q)
        amb_grid = (q - qi).abs() <= C_GEO * U_F32 * torch.maximum(torch.maximum(qi.abs(), M / P), torch.ones_like(q))
    G = max(int(g.max()) if K else 1, 1)
    i = torch.arange(P, dtype=torch.float64, device=dev).view(1, P, 1)
    s = torch.arange(G, dtype=torch.float64, device=dev).view(1, 1, G)
    gk = g.clamp_min(1).to(torch.float64).view(K, 1, 1)
    live = s < g.view(K, 1, 1).to(torch.float64)
    t1 = i * q.view(K, 1, 1)
    t2 = a0.view(K, 1, 1) + t1
    t3 = (s + 0.5) * q.view(K, 1, 1)
    t4 = t3 / gk
    v = t2 + t4
    # the same chain in f32, operation by operation: delta = 0 where every intermediate is exact
    f = torch.float32
    q0, q1 = r0 * s32, r1 * s32
    b0, b1 = q0 - off, q1 - off
    e32 = b1 - b0
    if not aligned:
        e32 = e32.clamp_min(1.0)
    bq = e32 / P
    head = (_f64(q0) == p0) & (_f64(q1) == p1) & (_f64(b0) == a0) & (_f64(b1) == a1) & (_f64(e32) == ext) & (_f64(bq) == q)
    amb_grid &= ~head                                              # a quotient the kernel computes exactly is decided exactly
    c1 = i.to(f) * bq.view(K, 1, 1)
    c2 = b0.view(K, 1, 1) + c1
    c3 = (s.to(f) + 0.5) * bq.view(K, 1, 1)
    c4 = c3 / gk.to(f)
    c5 = c2 + c4
    same = (_f64(c1) == t1) & (_f64(c2) == t2) & (_f64(c3) == t3) & (_f64(c4) == t4) & (_f64(c5) == v)
    exact = head & (same | ~live).reshape(K, -1).all(1)
    delta = torch.where(exact, torch.zeros_like(M), C_GEO * U_F32 * M)
    valid, lo, hi, wl, wh = _taps(v, L)
    d3 = delta.view(K, 1, 1)
    amb = live & (d3 > 0) & (((v + 1.0).abs() <= d3) | ((v - float(L)).abs() <= d3))
    T = _table(lo, hi, wl, wh, live & valid, g, L)
    Ta = _table(lo, hi, wl, wh, amb, g, L)                         # (clamped into the window by _taps: what counting it would add)
    Tv = _table(lo, hi, wl, wh, amb & valid, g, L)
    return dict(g=g, a0=a0, ext=ext, delta=delta, amb_grid=amb_grid, T=T, Tmin=T - Tv, Tmax=T - Tv + Ta, namb=amb.sum(2))


def _fold(t, fold):
    if fold == 1:
        return t
    K, P, L = t.shape
    return t.reshape(K, P // fold, fold, L).sum(2) / fold


def geometry(rois, H, W, ph, pw, scale, sr, aligned, fold=1):
    """rois [K, 5] f32 -> dict: b [K] batch index, y / x: the axis dicts of _axis (tables folded: [K, ph, H], [K, pw, W]),
    count [K] = max(gh gw, 1), amb_grid [K], amb_bins [K, ph, pw] bool (bins with an ambiguous-sample term)"""
    assert rois.dtype == torch.float32
    y = _axis(rois[:, 2], rois[:, 4], scale, ph * fold, H, sr, aligned)
    x = _axis(rois[:, 1], rois[:, 3], scale, pw * fold, W, sr, aligned)
    for a in (y, x):
        for k in ("T", "Tmin", "Tmax"):
            a[k] = _fold(a[k], fold)
        K, P = a["namb"].shape
        a["namb"] = a["namb"].reshape(K, P // fold, fold).sum(2)
    some = (y["g"] > 0) & (x["g"] > 0)
    amb_bins = ((y["namb"] > 0).unsqueeze(2) | (x["namb"] > 0).unsqueeze(1)) & some.view(-1, 1, 1)
    return dict(b=rois[:, 0].to(torch.int64), y=y, x=x, count=(y["g"] * x["g"]).clamp_min(1), amb_grid=(y["amb_grid"] | x["amb_grid"]) & some,
                amb_bins=amb_bins, fold=fold)


def table_conditions(geo):
    """-> (RoIs with an ambiguous grid size, share of bins carrying an ambiguous-sample term)"""
    return int(geo["amb_grid"].sum()), float(geo["amb_bins"].double().mean()) if geo["amb_bins"].numel() else 0.0


def _span(T, L):
    """footprint of every RoI on one axis, dilated by one pixel and clipped: lo [K], hi [K] inclusive (lo > hi: empty), mask [K, L]"""
    nz = (T > 0).any(1)
    idx = torch.arange(L, device=T.device).view(1, L)
    lo = torch.where(nz, idx, torch.full_like(idx, L)).amin(1)
    hi = torch.where(nz, idx, torch.full_like(idx, -1)).amax(1)
    has = hi >= lo
    lo = torch.where(has, (lo - 1).clamp_min(0), lo)
    hi = torch.where(has, (hi + 1).clamp_max(L - 1), hi)
    return lo, hi, (idx >= lo.view(-1, 1)) & (idx <= hi.view(-1, 1))


def _pool(Ty, Tx, xn):
    """[Kn, P, H], [Kn, Q, W], [H, W, C] -> [Kn, P, Q, C]"""
    Kn, P, H = Ty.shape
    Q, W = Tx.shape[1:]
    C = xn.shape[-1]
    r = (Ty.reshape(Kn * P, H) @ xn.reshape(H, W * C)).reshape(Kn, P, W, C)
    return torch.einsum("kqw,kpwc->kpqc", Tx, r)


# ---------------------------------------------------------------------------------------------------------------- forward
def roi_fwd(x, rois, ph, pw, scale, sr, aligned, esc=None, ebi=None, relu=False, pooled=False, out_dtype=None, geo=None):
    """x NHWC (any dtype, exact as float64), rois [K, 5] f32.  -> dict: v (the exact pooled value before the affine), pre_v, absw
    (pool(|x|)), exact = relu?(esc v + ebi), pre (its error bound before the store), bound; all [K, ph, pw, C] -- or, with ``pooled``,
    the 2x2-average-pooled map [K, ph/2, pw/2, C]; geo"""
    N, H, W, C = x.shape
    K = rois.shape[0]
    dev = x.device
    out_dtype = out_dtype or x.dtype
    geo = geo or geometry(rois, H, W, ph, pw, scale, sr, aligned)
    gy, gx = geo["y"], geo["x"]
    v = torch.zeros(K, ph, pw, C, dtype=torch.float64, device=dev)
    absw, coord, amb = torch.zeros_like(v), torch.zeros(K, 1, 1, C, dtype=torch.float64, device=dev), torch.zeros_like(v)
    ylo, yhi, _ = _span(gy["T"], H)
    xlo, xhi, _ = _span(gx["T"], W)
    has_amb = geo["amb_bins"].reshape(K, -1).any(1)
    for n in range(N):
        ks = torch.nonzero(geo["b"] == n).reshape(-1)
        if ks.numel() == 0:
            continue
        xn = _f64(x[n])
        xa = xn.abs()
        v[ks] = _pool(gy["T"][ks], gx["T"][ks], xn)
        absw[ks] = _pool(gy["T"][ks], gx["T"][ks], xa)
        ka = ks[has_amb[ks]]
        if ka.numel():
            amb[ka] = _pool(gy["Tmax"][ka], gx["Tmax"][ka], xa) - _pool(gy["Tmin"][ka], gx["Tmin"][ka], xa)
        dv = (xn[1:] - xn[:-1]).abs() if H > 1 else None
        dh = (xn[:, 1:] - xn[:, :-1]).abs() if W > 1 else None
        for k in ks.tolist():
            y0, y1, x0, x1 = int(ylo[k]), int(yhi[k]), int(xlo[k]), int(xhi[k])
            if y0 > y1 or x0 > x1:
                continue
            if dv is not None and y1 > y0 and float(gy["delta"][k]) > 0:
                coord[k, 0, 0] += gy["delta"][k] * dv[y0:y1, x0:x1 + 1].amax((0, 1))
            if dh is not None and x1 > x0 and float(gx["delta"][k]) > 0:
                coord[k, 0, 0] += gx["delta"][k] * dh[y0:y1 + 1, x0:x1].amax((0, 1))
    nterm = 4.0 * geo["count"].to(torch.float64).view(K, 1, 1, 1)
    if pooled:
        m4 = lambda t: t.reshape(K, ph // 2, 2, pw // 2, 2, C).mean((2, 4))
        v, absw, amb = m4(v), m4(absw), m4(amb)
        nterm = 4.0 * nterm
    pre_v = (nterm + 8.0) * U_F32 * absw + coord + amb
    return affine(dict(v=v, pre_v=pre_v, absw=absw, geo=geo), esc, ebi, relu, out_dtype)


def affine(f, esc=None, ebi=None, relu=False, out_dtype=torch.bfloat16, channels=None):
    """y = relu?(esc v + ebi) of a pooled value f["v"] with its bound f["pre_v"] (a roi_fwd result; ``channels``: only its first so
    many channels) -> a new dict with exact, pre and bound as well"""
    C = channels or f["v"].shape[-1]
    v, pre_v = f["v"][..., :C], f["pre_v"][..., :C]
    exact, pre = v, pre_v
    if esc is not None:
        s, b = _f64(esc).view(1, 1, 1, C), _f64(ebi).view(1, 1, 1, C)
        exact = s * v + b
        pre = s.abs() * pre_v + U_F32 * ((s * v).abs() + b.abs())
        if relu:
            exact = exact.clamp_min(0.0)
    return dict(v=v, pre_v=pre_v, absw=f["absw"][..., :C], exact=exact, pre=pre, bound=store_bound(exact, pre, u_out(out_dtype)), geo=f["geo"])


def pooled_of_stored(y):
    """the tap kernel's pooled by-product from the crops it stored, [K, ph, pw, C] -> [K, ph/2, pw/2, C] in y's dtype, bit for bit:
    T(((a0 + a1) + (a2 + a3)) * 0.25f) in f32 (also avgpool2_fwd's expression)"""
    f = y.float()
    a0, a1, a2, a3 = f[:, 0::2, 0::2], f[:, 0::2, 1::2], f[:, 1::2, 0::2], f[:, 1::2, 1::2]
    return (((a0 + a1) + (a2 + a3)) * 0.25).to(y.dtype)


# ---------------------------------------------------------------------------------------------------------------- e4m3
def e4m3_decode(codes):
    """uint8 OCP e4m3 (fn: no infinities, 0x7f / 0xff NaN) -> float64"""
    c = codes.to(torch.int64)
    sign = torch.where((c & 0x80) != 0, -1.0, 1.0).to(torch.float64)
    e, m = (c >> 3) & 0xF, (c & 7).to(torch.float64)
    val = torch.where(e == 0, m * 2.0 ** -9, (1.0 + m / 8.0) * torch.pow(2.0, (e - 7).to(torch.float64)))
    val = torch.where((c & 0x7F) == 0x7F, torch.full_like(val, math.nan), val)
    return sign * val


def check_e4m3(codes, exact, pre, q8):
    """codes: the kernel's e4m3 copy of the unrounded value ``exact`` (error bound ``pre``) times the f32 scale q8, saturated at
    +-448.  -> (ok, worst |err| / bound, flat index)"""
    q = float(torch.tensor(q8, dtype=torch.float32))
    t = _f64(exact) * q
    e = q * _f64(pre) + U_F32 * t.abs()
    top = (t.abs() + e).clamp(2.0 ** -6, 448.0)
    half = torch.pow(2.0, torch.floor(torch.log2(top)) - 4.0)     # half the spacing of e4m3 numbers there (2^-10 below 2^-6)
    return check(e4m3_decode(codes), t.clamp(-448.0, 448.0), half + e)


def check_amax(amax_slots, exact, pre):
    """amax_slots: the f32 slots the kernel max-ed |y| into (zero before the launch) -> (ok, got, lowest, highest allowed)"""
    got = float(amax_slots.max())
    a = _f64(exact).abs()
    lo, hi = float((a - _f64(pre)).max()), float((a + _f64(pre)).max())
    return lo <= got <= hi, got, lo, hi


# ---------------------------------------------------------------------------------------------------------------- backward
def roi_bwd(dy, rois, in_shape, scale, sr, aligned, fold=1, out_dtype=None, geo=None):
    """dy [K, ph, pw, C] (with fold = 2: the gradient of the 2x2-pooled map), rois [K, 5] f32 grouped or not (every RoI goes to the
    image it names; one outside [0, N) to none).  -> dict: exact [N, H, W, C], pre, bound, nterms [N, H, W], geo"""
    N, H, W, C = in_shape
    K, ph, pw, _ = dy.shape
    dev = dy.device
    out_dtype = out_dtype or dy.dtype
    geo = geo or geometry(rois, H, W, ph, pw, scale, sr, aligned, fold)
    gy, gx = geo["y"], geo["x"]
    _, _, my = _span(gy["T"], H)
    _, _, mx = _span(gx["T"], W)
    Ey = (2.0 * gy["delta"]).view(K, 1, 1) * my.view(K, 1, H).to(torch.float64) + (gy["Tmax"] - gy["Tmin"])
    Ex = (2.0 * gx["delta"]).view(K, 1, 1) * mx.view(K, 1, W).to(torch.float64) + (gx["Tmax"] - gx["Tmin"])
    ck = 2.0 * fold * (gy["g"] + gx["g"]).to(torch.float64) + 4.0
    exact = torch.zeros(N, H, W, C, dtype=torch.float64, device=dev)
    pre = torch.zeros_like(exact)
    nterms = torch.zeros(N, H, W, dtype=torch.float64, device=dev)

    def scatter(Ty, Tx, d):                                       # [Kn,P,H], [Kn,Q,W], [Kn,P,Q,C] -> [H,W,C]
        Kn = d.shape[0]
        t = torch.bmm(Ty.transpose(1, 2), d.reshape(Kn, ph, pw * C)).reshape(Kn, H, pw, C)
        return torch.einsum("kqw,khqc->hwc", Tx, t)

    for n in range(N):
        ks = torch.nonzero(geo["b"] == n).reshape(-1)
        if ks.numel() == 0:
            continue
        d = _f64(dy[ks])
        da = d.abs()
        Ty, Tx = gy["T"][ks], gx["T"][ks]
        exact[n] = scatter(Ty, Tx, d)
        s_abs = scatter(Ty, Tx, da)
        s_ck = scatter(Ty, Tx, da * ck[ks].view(-1, 1, 1, 1))
        s_geo = scatter(Ty + Ey[ks], Tx + Ex[ks], da) - s_abs
        nterms[n] = torch.einsum("kh,kw->hw", (Ty > 0).sum(1).double(), (Tx > 0).sum(1).double())
        pre[n] = s_geo.clamp_min(0.0) + (nterms[n].unsqueeze(-1) * s_abs + s_ck) * U_F32
    return dict(exact=exact, pre=pre, bound=store_bound(exact, pre, u_out(out_dtype)), nterms=nterms, geo=geo)


# ---------------------------------------------------------------------------------------------------------------- judging
def store_bias(got, exact, pre):
    """signed error of a bf16 store in ulps of the output, toward zero, over the elements whose pre-store bound is below 1/16 ulp
    (exact_gemm.rounding_bias): round-to-nearest-even ~0, truncation ~-0.5.  -> (bias, elements); judged from 20 000 elements on,
    |bias| <= 0.02, as in the attention tests"""
    return A.store_bias(got, exact, pre)


BIAS_MIN_ELEMENTS = 20000
BIAS_LIMIT = 0.02


def locate(flat, shape):
    """flat index -> tuple index of ``shape`` (for a failure message: RoI / image, bin or pixel, channel)"""
    out = []
    for s in reversed(shape):
        out.append(flat % s)
        flat //= s
    return tuple(reversed(out))


def old_criterion(got, ref, tol):
    """what tests/test_gpu_ops.py applied: max|got - ref| < tol * max(1, max|ref|); NaN fails"""
    d = float((_f64(got) - _f64(ref)).abs().max())
    return d < tol * max(1.0, float(_f64(ref).abs().max()))
