"""The RoI checker itself (tests/exact_roi.py), on the CPU: the float64 forward and backward against the oracle's f32 RoIAlign and its
autograd and the reference's 5x5 known-answer table; the dyadic edge cases against values worked out by hand; the bound against plain
f32 emulations that sum in other orders, on every case table of tests/test_gpu_roi_exact.py; mutants the bound must reject, with the
verdict of the old  max|got - ref| < tol * max(1, max|ref|)  criterion printed next to each; and the conditions on the case tables."""
import json
import os

import pytest
import torch

import exact_gemm as X
import exact_roi as R
import roi_exact_cases as T

S = T.SCALE
OLD_TOL = {torch.float32: 1e-5, torch.bfloat16: 1.5e-2}          # tests/test_gpu_ops.py, before it was re-pointed


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _map(N, H, W, C, seed, dtype=torch.bfloat16, spikes=True):
    """a feature map with a heavy tail: noise of 0.2 and two interior activations of ~60 in one row (what makes a global-max
    criterion blind to everything that happens at the borders or in the small-valued bins)"""
    x = torch.randn(N, H, W, C, generator=_g(seed)) * 0.2
    if spikes:
        for n in range(N):
            x[n, H // 3, W // 2, :] = 60.0
            x[n, H // 3, W // 3, ::2] = -45.0
    return x.to(dtype)


# the (table name, rows, N, H, W, ph, pw, sampling_ratio, aligned, fold) every GPU case runs on
def all_tables():
    out = []
    for (H, W) in T.MAPS:
        rows = T.table_F(H, W)
        out += [(f"F{H}x{W}", rows, 2, H, W, 14, 14, 0, True, 1), (f"F{H}x{W} sr2", rows, 2, H, W, 14, 14, 2, True, 1),
                (f"F{H}x{W} unaligned", rows, 2, H, W, 14, 14, 0, False, 1), (f"F{H}x{W} pooled bwd", rows, 2, H, W, 7, 7, 0, True, 2),
                (f"F{H}x{W} 6x14", rows, 2, H, W, 6, 14, 0, True, 1)]
    out.append(("bench", T.table_bench(), 2, 50, 84, 14, 14, 0, True, 1))
    out.append(("bench pooled bwd", T.table_bench(), 2, 50, 84, 7, 7, 0, True, 2))
    out.append(("counts", T.table_counts(13, 21, (64, 0, 130, 1, 65), 40), 5, 13, 21, 14, 14, 0, True, 1))
    out.append(("wide", T.table_counts(6, 7, (11, 9), 50), 2, 6, 7, 14, 14, 0, True, 1))
    out.append(("wide pooled bwd", T.table_counts(6, 7, (11, 9), 50), 2, 6, 7, 7, 7, 0, True, 2))
    return out


# ================================================================================================== f32 emulations (and mutants)
def _emu_axis(r0, r1, P, L, sr, aligned, mut, axis):
    """roi_geom + axis_tap in torch f32, one operation at a time.  -> lo, hi [K, P, G] int64 (indices into a map padded by 2 zero rows),
    wl, wh f32, keep bool, g int64 [K]"""
    f = torch.float32
    K = r0.numel()
    s32 = torch.tensor(S, dtype=f)
    off = 0.5 if (aligned and "no_aligned_offset" not in mut) else 0.0
    a0, a1 = r0 * s32 - off, r1 * s32 - off
    ext = a1 - a0
    if not aligned:
        ext = ext.clamp_min(1.0)
    bq = ext / P
    if sr > 0:
        g = torch.full((K,), sr, dtype=torch.int64)
    else:
        g = (torch.floor(bq) if "floor_grid" in mut else torch.ceil(bq)).long().clamp_min(0)
    G = max(int(g.max()), 1)
    i = torch.arange(P, dtype=f).view(1, P, 1)
    s = torch.arange(G, dtype=f).view(1, 1, G)
    gk = g.clamp_min(1).to(f).view(K, 1, 1)
    v = (a0.view(K, 1, 1) + i * bq.view(K, 1, 1)) + ((s + 0.5) * bq.view(K, 1, 1)) / gk
    keep = (s < g.view(K, 1, 1).to(f)).expand(K, P, G).clone()
    if "drop_last_y_sample" in mut and axis == "y":
        keep &= ~((s == (g.view(K, 1, 1) - 1).to(f)) & (g.view(K, 1, 1) > 4))
    if "window_0_L" in mut:
        keep &= (v >= 0.0) & (v < float(L))
    else:
        keep &= (v >= -1.0) & (v <= float(L))
    if "no_clamp0" not in mut:
        v = torch.where(v <= 0, torch.zeros_like(v), v)
    lo = v.to(torch.int64).clamp(0, L)                            # (int)v truncates toward zero
    if "no_snap" in mut:
        hi = lo + 1                                                # reads past the map: zeros here
    else:
        snap = lo >= L - 1
        lo = torch.where(snap, torch.full_like(lo, L - 1), lo)
        v = torch.where(snap, lo.to(f), v)
        hi = torch.where(snap, lo, lo + 1)
    wh = v - lo.to(f)
    wl = 1.0 - wh
    if "swap_wl_wh" in mut and axis == "x":
        wl, wh = wh, wl
    return lo, hi, wl, wh, keep, g


def _emu_tables(lo, hi, wl, wh, keep, L):
    K, P, G = lo.shape
    t = torch.zeros(K, P, L + 2, dtype=torch.float32)
    t.scatter_add_(2, lo, wl * keep)
    t.scatter_add_(2, hi, wh * keep)
    return t[:, :, :L]


def emu_fwd(x, rois, ph, pw, sr, aligned, order="tap", mut=(), pooled=False, out_dtype=None, truncate=False):
    """the forward in plain f32: ``tap``: sample by sample, w1 v1 + w2 v2 + w3 v3 + w4 v4 with w = wy wx; ``rows``: per-axis weight
    tables (duplicate rows merged), the map contracted with the row table first.  ``pooled``: the mean of 2x2 unrounded bins."""
    N, H, W, C = x.shape
    K = rois.shape[0]
    out_dtype = out_dtype or x.dtype
    ylo, yhi, ywl, ywh, ykeep, gh = _emu_axis(rois[:, 2], rois[:, 4], ph, H, sr, aligned, mut, "y")
    xlo, xhi, xwl, xwh, xkeep, gw = _emu_axis(rois[:, 1], rois[:, 3], pw, W, sr, aligned, mut, "x")
    b = rois[:, 0].long()
    inb = (b >= 0) & (b < N)
    xp = torch.zeros(N, H + 2, W + 2, C)
    xp[:, :H, :W] = x.float()
    xb = xp[b.clamp(0, N - 1)]
    count = ((gh * gh) if "count_ghgh" in mut else (gh * gw)).clamp_min(1).float().view(K, 1, 1, 1)
    kk = torch.arange(K).view(K, 1, 1)
    if order == "tap":
        acc = torch.zeros(K, ph, pw, C)
        for iy in range(ylo.shape[2]):
            for ix in range(xlo.shape[2]):
                m = (ykeep[:, :, iy].unsqueeze(2) & xkeep[:, :, ix].unsqueeze(1)).unsqueeze(-1)
                if not bool(m.any()):
                    continue
                yl, yh = ylo[:, :, iy].unsqueeze(2), yhi[:, :, iy].unsqueeze(2)
                xl, xh = xlo[:, :, ix].unsqueeze(1), xhi[:, :, ix].unsqueeze(1)
                wyl, wyh = ywl[:, :, iy].view(K, ph, 1, 1), ywh[:, :, iy].view(K, ph, 1, 1)
                wxl, wxh = xwl[:, :, ix].view(K, 1, pw, 1), xwh[:, :, ix].view(K, 1, pw, 1)
                t = (wyl * wxl) * xb[kk, yl, xl] + (wyl * wxh) * xb[kk, yl, xh] + (wyh * wxl) * xb[kk, yh, xl] + (wyh * wxh) * xb[kk, yh, xh]
                acc = acc + torch.where(m, t, torch.zeros_like(t))
    else:
        Ty = _emu_tables(ylo, yhi, ywl, ywh, ykeep, H)
        Tx = _emu_tables(xlo, xhi, xwl, xwh, xkeep, W)
        r = torch.einsum("kph,khwc->kpwc", Ty, xb[:, :H, :W])
        acc = torch.einsum("kqw,kpwc->kpqc", Tx, r)
    if pooled:
        acc = acc.reshape(K, ph // 2, 2, pw // 2, 2, C)
        acc = ((acc[:, :, 0, :, 0] + acc[:, :, 0, :, 1]) + (acc[:, :, 1, :, 0] + acc[:, :, 1, :, 1])) * (1.0 / (count * 4.0))
    else:
        acc = acc / count
    acc = acc * inb.view(K, 1, 1, 1)
    if truncate and out_dtype == torch.bfloat16:
        return X.truncate_bf16(acc).to(torch.bfloat16)
    return acc.to(out_dtype)


def emu_bwd(dy, rois, in_shape, sr, aligned, fold=1, mut=(), out_dtype=None):
    """the backward in plain f32 as a table product: f32 tables (fw * (w / g) added sample by sample), one f32 contraction per image"""
    N, H, W, C = in_shape
    K, ph, pw, _ = dy.shape
    out_dtype = out_dtype or dy.dtype
    fw = 1.0 if "fold_weight_1" in mut else 1.0 / fold
    tabs = []
    for (c0, c1, P, L, axis) in ((2, 4, ph, H, "y"), (1, 3, pw, W, "x")):
        lo, hi, wl, wh, keep, g = _emu_axis(rois[:, c0], rois[:, c1], P * fold, L, sr, aligned, (), axis)
        gk = g.clamp_min(1).float().view(K, 1, 1)
        t = _emu_tables(lo, hi, fw * (wl / gk), fw * (wh / gk), keep, L)
        tabs.append(t.reshape(K, P, fold, L).sum(2) if fold > 1 else t)
    Ty, Tx = tabs
    if "ax_stride_ph" in mut:                                      # Ax [k][x][j] read at x * ph + j
        flat = Tx.transpose(1, 2).reshape(K, W * pw)
        idx = (torch.arange(W).view(W, 1) * ph + torch.arange(pw).view(1, pw)).reshape(-1)
        Tx = flat[:, idx].reshape(K, W, pw).transpose(1, 2)
    b = rois[:, 0].long()
    dx = torch.zeros(N, H, W, C)
    for n in range(N):
        ks = torch.nonzero(b == n).reshape(-1)
        if "skip_rois_64_on" in mut:
            ks = ks[:64]
        if ks.numel() == 0:
            if "empty_image_unwritten" in mut:
                dx[n] = 7.0                                        # whatever the buffer held
            continue
        t = torch.einsum("kph,kpqc->khqc", Ty[ks], dy[ks].float())
        dx[n] = torch.einsum("kqw,khqc->hwc", Tx[ks], t)
    return dx.to(out_dtype)


# ================================================================================================== oracle agreement
@pytest.mark.parametrize("aligned", [False, True])
@pytest.mark.parametrize("sr", [0, 2])
def test_reference_equals_the_oracle_and_its_autograd(aligned, sr):
    """the float64 forward / backward against oracle.ops.roi_align (f32, native C) and its autograd, within the reference's own bound for
    an f32 computation"""
    from oracle import ops as oo
    H, W, C = 13, 21, 8
    rows = T.table_F(H, W)[:-1]                                    # (the oracle has no image N)
    rois = T.rois_tensor(rows)
    x = _map(2, H, W, C, 1, torch.float32)
    xr = x.permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    ref = oo.roi_align(xr, rois, 14, S, sr, aligned)
    f = R.roi_fwd(x, rois, 14, 14, S, sr, aligned)
    ok, r, w = R.check(ref.detach().permute(0, 2, 3, 1), f["exact"], f["bound"])
    print(f"forward: oracle within {r:.3g} of the bound")
    assert ok, (r, rows[R.locate(w, f["exact"].shape)[0]])
    dy = torch.randn(len(rows), 14, 14, C, generator=_g(2))
    ref.backward(dy.permute(0, 3, 1, 2).contiguous())
    bw = R.roi_bwd(dy, rois, (2, H, W, C), S, sr, aligned)
    ok, r, w = R.check(xr.grad.permute(0, 2, 3, 1), bw["exact"], bw["bound"])
    print(f"backward: oracle within {r:.3g} of the bound")
    assert ok, (r, R.locate(w, bw["exact"].shape))
    # and element by element close in the plain sense: no systematic difference hides in the bound
    assert float((xr.grad.permute(0, 2, 3, 1).double() - bw["exact"]).abs().max()) < 1e-4 * float(bw["exact"].abs().max())


@pytest.mark.parametrize("aligned", [False, True])
def test_reference_equals_the_known_answer_table(aligned):
    k = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "kat.json")))["roi_align_5x5"]
    x = torch.arange(25, dtype=torch.float32).reshape(1, 5, 5, 1)
    rois = torch.tensor([[0.0] + [float(v) for v in k["box"]]])
    f = R.roi_fwd(x, rois, 4, 4, 1.0, 0, aligned)
    exp = torch.tensor(k["aligned_true" if aligned else "aligned_false"], dtype=torch.float64)
    assert torch.equal(f["exact"][0, :, :, 0], exp)


# ================================================================================================== dyadic edge cases
def _ramp(H=13, W=21):
    """x[y][x] = 100 y + x: a bilinear sample at (y, x) inside the map is 100 y + x"""
    return (100.0 * torch.arange(H).view(H, 1) + torch.arange(W).view(1, W)).reshape(1, H, W, 1)


def _edge_expected(name):
    """[ph, pw] float64, by hand: bins of one pixel, one sample each, x samples at 2.5 + j"""
    i = torch.arange(14, dtype=torch.float64).view(14, 1)
    xs = 2.5 + torch.arange(14, dtype=torch.float64).view(1, 14)
    base = name[:-2] if name.endswith("_a") else name
    if base == "at_minus1":                                        # y = i - 1: -1 is counted and clamped to row 0; 12 = L - 1
        return 100.0 * (i - 1).clamp_min(0) + xs
    if base == "outside_minus1":                                   # y = i - 1 - 2^-10: dropped; clamped to 0; then between rows
        e = 100.0 * (i - 1) - 25.0 / 256 + xs
        e[0] = 0.0
        e[1] = xs[0]
        return e
    if base == "at_L":                                             # y = i + 1: 12 and 13 = L give row 12; 14 is dropped
        e = 100.0 * (i + 1).clamp_max(12) + xs
        e[13] = 0.0
        return e
    if base == "top_pixel":                                        # y = i + 0.5: 12.5 snaps to row 12; 13.5 is dropped
        e = 100.0 * (i + 0.5) + xs
        e[12] = 1200.0 + xs[0]
        e[13] = 0.0
        return e
    if base == "empty_sr2":                                        # every sample at (2.5, 2.5)
        return torch.full((14, 14), 252.5, dtype=torch.float64)
    if base == "subpixel_floored":                                 # 4 x 4 bins of 1/4 pixel from (2.5, 2.5), sampled at their centres
        j = torch.arange(4, dtype=torch.float64)
        return 100.0 * (2.625 + j.view(4, 1) / 4) + (2.625 + j.view(1, 4) / 4)
    assert base in ("empty_adaptive", "outside_image", "inverted")
    return torch.zeros(14, 14, dtype=torch.float64)


@pytest.mark.parametrize("case", T.EDGE, ids=[c[0] for c in T.EDGE])
def test_dyadic_edge_cases_have_the_values_worked_out_by_hand(case):
    name, box, aligned, sr, p = case
    rois = torch.tensor([[0.0, *box]])
    f = R.roi_fwd(_ramp(), rois, p, p, S, sr, aligned)
    geo = f["geo"]
    assert float(geo["y"]["delta"][0]) == 0.0 and float(geo["x"]["delta"][0]) == 0.0, "not exact in f32: the case decides nothing"
    assert torch.equal(f["exact"][0, :, :, 0], _edge_expected(name)), (f["exact"][0, :, :, 0], _edge_expected(name))
    # after the affine: relu(s * v + b); an empty box gives relu(b)
    esc, ebi = torch.tensor([-0.5]), torch.tensor([3.0])
    fa = R.roi_fwd(_ramp(), rois, p, p, S, sr, aligned, esc=esc, ebi=ebi, relu=True)
    assert torch.equal(fa["exact"][0, :, :, 0], (3.0 - 0.5 * _edge_expected(name)).clamp_min(0.0))
    # the f32 emulation agrees exactly (every operation is exact), and the bound leaves it no room beyond the sum's roundings
    e = emu_fwd(_ramp(), rois, p, p, sr, aligned)
    assert R.check(e, f["exact"], f["bound"])[0]


def test_a_roi_naming_an_image_outside_the_batch_pools_to_zero_before_the_affine():
    rois = torch.tensor([[1.0, 32.0, 32.0, 200.0, 200.0], [-1.0, 32.0, 32.0, 200.0, 200.0]])
    f = R.roi_fwd(_ramp(), rois, 14, 14, S, 0, True, esc=torch.tensor([2.0]), ebi=torch.tensor([0.75]), relu=True)
    assert bool((f["v"] == 0).all()) and bool((f["exact"] == 0.75).all())
    b = R.roi_bwd(torch.ones(2, 14, 14, 1), rois, (1, 13, 21, 1), S, 0, True)
    assert bool((b["exact"] == 0).all())


def test_ambiguous_samples_and_grid_sizes_are_flagged():
    """a sample 2 u from the window's edge, not exact in f32, is ambiguous and its bin's bound carries its whole contribution; a box
    whose height is within a rounding of 14 pixels has an ambiguous grid size"""
    y0 = -1.5 - 1.0 / 3 * 2.0 ** -20
    rois = torch.tensor([[0.0, 32.0, y0 * 16, 256.0, (y0 + 14.0) * 16]])
    x = _ramp() + 5.0
    f = R.roi_fwd(x, rois, 14, 14, S, 1, False)                   # (one sample per bin, at y0 + (i + 0.5) bh: the first ~ -1 - 3e-7)
    geo = f["geo"]
    assert float(geo["y"]["delta"][0]) > 0 and bool(geo["amb_bins"][0, 0].all()) and not bool(geo["amb_bins"][0, 1:].any())
    assert float(f["pre_v"][0, 0].min()) >= 5.0 and float(f["pre_v"][0, 1:].max()) < 1e-2
    r2 = torch.tensor([[0.0, 32.0, 8.0, 256.0, 8.0 + 16 * 14 * (1 + 2.0 ** -22)]])
    assert R.table_conditions(R.geometry(r2, 13, 21, 14, 14, S, 0, True))[0] == 1


# ================================================================================================== the bound accepts other f32 orders
@pytest.mark.parametrize("tab", all_tables(), ids=[t[0] for t in all_tables()])
def test_bound_accepts_plain_f32_in_other_orders(tab):
    name, rows, N, H, W, ph, pw, sr, aligned, fold = tab
    rois = T.rois_tensor(rows)
    K, C = len(rows), 8
    for dtype in (torch.bfloat16, torch.float32):
        if fold == 1:
            x = _map(N, H, W, C, 3, dtype)
            f = R.roi_fwd(x, rois, ph, pw, S, sr, aligned)
            for order in ("tap", "rows"):
                if order == "tap" and int(f["geo"]["count"].max()) > 40 and dtype == torch.float32:
                    continue                                       # (the tap loop over a 17 x 19 grid once per table is enough)
                ok, r, w = R.check(emu_fwd(x, rois, ph, pw, sr, aligned, order), f["exact"], f["bound"])
                print(f"{name} fwd {order} {dtype}: {r:.3g}")
                assert ok, (name, order, rows[R.locate(w, f["exact"].shape)[0]], r)
            if ph % 2 == 0 and pw % 2 == 0 and dtype == torch.bfloat16:
                fp = R.roi_fwd(x, rois, ph, pw, S, sr, aligned, pooled=True, geo=f["geo"])
                ok, r, w = R.check(emu_fwd(x, rois, ph, pw, sr, aligned, "rows", pooled=True), fp["exact"], fp["bound"])
                print(f"{name} fwd pooled-only: {r:.3g}")
                assert ok, (name, rows[R.locate(w, fp["exact"].shape)[0]], r)
        dy = (torch.randn(K, ph, pw, C, generator=_g(4)) * 0.5).to(dtype)
        dy[K // 2] = 0
        b = R.roi_bwd(dy, rois, (N, H, W, C), S, sr, aligned, fold)
        ok, r, w = R.check(emu_bwd(dy, rois, (N, H, W, C), sr, aligned, fold), b["exact"], b["bound"])
        print(f"{name} bwd {dtype}: {r:.3g}")
        assert ok, (name, R.locate(w, b["exact"].shape), r)


# ================================================================================================== mutants
FWD_MUTANTS = ["no_aligned_offset", "floor_grid", "window_0_L*", "no_clamp0", "no_snap*", "count_ghgh", "swap_wl_wh", "drop_last_y_sample*",
               "truncated_store*"]
BWD_MUTANTS = ["skip_rois_64_on", "fold_weight_1", "ax_stride_ph", "empty_image_unwritten"]


def _judge(got, exact, bound, pre):
    ok = R.check(got, exact, bound)[0]
    bias, n = R.store_bias(got, exact, pre)
    if n >= R.BIAS_MIN_ELEMENTS and abs(bias) > R.BIAS_LIMIT:
        ok = False
    return ok, bias, n


def test_mutants_are_rejected_and_the_old_criterion_misses_the_starred_ones():
    H, W, C = 13, 21, 8
    rows = T.table_F(H, W)
    rois = T.rois_tensor(rows)
    x = _map(2, H, W, C, 5)
    f = R.roi_fwd(x, rois, 14, 14, S, 0, True)
    good = emu_fwd(x, rois, 14, 14, 0, True)
    ok, bias, n = _judge(good, f["exact"], f["bound"], f["pre"])
    assert ok and n >= R.BIAS_MIN_ELEMENTS, (ok, bias, n)
    ref32 = emu_fwd(x.float(), rois, 14, 14, 0, True, out_dtype=torch.float32)   # what the old test compared with: an f32 RoIAlign
    lines, missed_by_old = [], []
    for m in FWD_MUTANTS:
        name = m.rstrip("*")
        got = emu_fwd(x, rois, 14, 14, 0, True, mut=(name,), truncate=name == "truncated_store")
        ok, bias, n = _judge(got, f["exact"], f["bound"], f["pre"])
        old = R.old_criterion(got, ref32, OLD_TOL[torch.bfloat16])
        lines.append(f"  {m:24s} new: {'accepted' if ok else 'rejected'} (store bias {bias:+.3f} over {n})   old: {'accepted' if old else 'rejected'}")
        assert not ok, f"mutant {name} passes the bound"
        if old:
            missed_by_old.append(m)
    # backward: 130 RoIs in one image and an image without any (table "counts"); the pooled fold; a 6 x 14 grid
    crow = T.table_counts(13, 21, (64, 0, 130, 1, 65), 40)
    crois = T.rois_tensor(crow)
    cases = {"skip_rois_64_on": (crow, crois, 5, 14, 14, 1), "empty_image_unwritten": (crow, crois, 5, 14, 14, 1),
             "fold_weight_1": (rows, rois, 2, 7, 7, 2), "ax_stride_ph": (rows, rois, 2, 6, 14, 1)}
    for m in BWD_MUTANTS:
        rw, rs, N, ph, pw, fold = cases[m]
        dy = (torch.randn(len(rw), ph, pw, C, generator=_g(6)) * 0.5).bfloat16()
        b = R.roi_bwd(dy, rs, (N, H, W, C), S, 0, True, fold)
        assert R.check(emu_bwd(dy, rs, (N, H, W, C), 0, True, fold), b["exact"], b["bound"])[0]
        got = emu_bwd(dy, rs, (N, H, W, C), 0, True, fold, mut=(m,))
        ok = R.check(got, b["exact"], b["bound"])[0]
        old = R.old_criterion(got, emu_bwd(dy.float(), rs, (N, H, W, C), 0, True, fold, out_dtype=torch.float32), OLD_TOL[torch.bfloat16])
        lines.append(f"  {m:24s} new: {'accepted' if ok else 'rejected'}   old: {'accepted' if old else 'rejected'}")
        assert not ok, f"mutant {m} passes the bound"
        if old:
            missed_by_old.append(m)
    print("\n".join(["mutants (* = the issue expects the old criterion to miss it):"] + lines))
    print("missed by the old criterion:", ", ".join(missed_by_old))
    for m in FWD_MUTANTS:
        if m.endswith("*"):
            assert m in missed_by_old, f"the old criterion catches {m} on this data: the starred list no longer demonstrates the gap"


# ================================================================================================== conditions on the tables
@pytest.mark.parametrize("tab", all_tables(), ids=[t[0] for t in all_tables()])
def test_table_conditions_hold(tab):
    name, rows, N, H, W, ph, pw, sr, aligned, fold = tab
    geo = R.geometry(T.rois_tensor(rows), H, W, ph, pw, S, sr, aligned, fold)
    n_amb, share = R.table_conditions(geo)
    print(f"{name}: {len(rows)} RoIs, ambiguous grid sizes {n_amb}, bins with an ambiguous-sample term {100 * share:.4f} %")
    assert n_amb == 0 and share <= 1e-3
    b = [r[1] for r in rows]
    assert b == sorted(b), "RoIs must be grouped by image"


def test_table_F_places_a_case_on_each_side_of_every_dispatch_threshold():
    """computed from the reference geometry, not from the names alone: grid sizes, merged feature rows per bin row, x slides"""
    for (H, W) in T.MAPS:
        rows = T.table_F(H, W)
        nm = T.names(rows)
        geo = R.geometry(T.rois_tensor(rows), H, W, 14, 14, S, 0, True)
        gh = {n: int(g) for n, g in zip(nm, geo["y"]["g"])}
        gw = {n: int(g) for n, g in zip(nm, geo["x"]["g"])}
        for g in (1, 2, 3, 4, 5, 8, 9, 16, 17):                    # ROW_MAXY: 2 ny > 32 <=> gh > 16 (crops), gh > 8 (pooled-only)
            assert gh[f"gh{g}"] == g and 14 * gw[f"gh{g}"] <= 256
        for g in (1, 2, 18, 19):                                   # ROI_MAXS: nx = 14 gw > 256 <=> gw >= 19
            assert gw[f"gw{g}"] == g and gh[f"gw{g}"] <= 8
        assert 14 * 18 <= 256 < 14 * 19
        tabled = (geo["y"]["g"] <= 16) & (geo["x"]["g"] <= 18) & (geo["b"] < 2)
        nrow = (geo["y"]["T"] > 0).sum(2)[tabled]                  # merged feature rows of every bin row (prefetch form: <= PF = 4)
        have = set(nrow.reshape(-1).tolist())
        assert {1, 2, 3, 4, 5, 6} <= have, have
        nrow2 = (geo["y"]["T"].reshape(len(rows), 7, 2, H).sum(2) > 0).sum(2)[(geo["y"]["g"] <= 8) & (geo["x"]["g"] <= 18)]
        assert {4, 5} <= set(nrow2.reshape(-1).tolist())           # the same for the pooled-only output's row pairs
        # under sampling_ratio = 2 a slide of more than one column between consecutive x samples
        g2 = R.geometry(T.rois_tensor(rows), H, W, 14, 14, S, 2, True)
        k = nm.index("wide_sr2")
        cols = (g2["x"]["T"][k] > 0).float()
        first = torch.where(cols.any(1), cols.argmax(1), torch.full((14,), -1))
        first = first[first >= 0]
        assert first.numel() >= 3 and int((first[1:] - first[:-1]).max()) >= 3
        # both images, an image index outside the batch, an empty box, an inverted one
        assert nm[-1] == "batch_index_N" and int(geo["b"][-1]) == 2 and gh["empty_adaptive"] == 0 and gw["inverted"] == 0
