"""CPU: the plain reference of tests/graph_ref.py is itself right, every case of tests/graph_exact_cases.py builds, the limits
derived from the plain module stay under their caps, and every ``drop`` (one backward term removed) moves a compared tensor by at
least ten times its limit in both dtypes -- so a node with that wiring error could not pass tests/test_gpu_graph_exact.py."""
import torch
import torch.nn.functional as F

import exact_roi as XR
import graph_exact_cases as GC
import graph_ref as G

F64 = torch.float64


def _rel(a, b):
    return float((a - b).abs().max()) / float(b.abs().max())


def test_roi_crops_agree_with_exact_roi():
    """the RoI set of the GPU cases: forward equal to exact_roi.roi_fwd's v, autograd gradient equal to exact_roi.roi_bwd's exact"""
    g = torch.Generator().manual_seed(3)
    feat = torch.randn(2, 10, 12, 32, generator=g, dtype=F64).requires_grad_(True)
    rois = torch.tensor(G.ROIS, dtype=torch.float32)
    dy = torch.randn(len(G.ROIS), 14, 14, 32, generator=g, dtype=F64)
    y = G.roi_crops(feat, rois, 14, 1.0 / 16, 0)
    v = XR.roi_fwd(feat.detach(), rois, 14, 14, 1.0 / 16, 0, True)["v"]
    assert y.shape == v.shape and _rel(y.detach(), v) <= 1e-12
    y.backward(dy)
    exact = XR.roi_bwd(dy, rois, tuple(feat.shape), 1.0 / 16, 0, True)["exact"]
    assert _rel(feat.grad, exact) <= 1e-12
    assert float(feat.grad[0].abs().max()) == 0.0 and list(G.ROI_START) == [0, 0, len(G.ROIS)]        # image 0 has no RoI
    # boxes over the border lose weight: rows of the separable tables that sum to less than one
    geo = XR.geometry(rois, 10, 12, 14, 14, 1.0 / 16, 0, True)
    lost = (geo["y"]["T"].sum(2) < 1 - 1e-9).any(1) | (geo["x"]["T"].sum(2) < 1 - 1e-9).any(1)
    assert lost.tolist() == [False, True, True, False, False, True], lost.tolist()


def test_attnpool_agrees_with_multi_head_attention():
    """graph_ref.attnpool against F.multi_head_attention_forward in float64 (query row 0, need_weights=False): output and all gradients"""
    g = torch.Generator().manual_seed(4)
    K, C, H, out = 3, 128, 2, 64
    mk = lambda *s: torch.randn(*s, generator=g, dtype=F64)
    x = mk(K, 7, 7, C)
    p = dict(pos=mk(50, C) * 0.5, q_w=mk(C, C) * C ** -0.5, q_b=mk(C) * 0.1, k_w=mk(C, C) * C ** -0.5, k_b=mk(C) * 0.1, v_w=mk(C, C) * C ** -0.5,
             v_b=mk(C) * 0.1, c_w=mk(out, C) * C ** -0.5, c_b=mk(out) * 0.1)
    gy = mk(K, out)
    res = []
    for which in (0, 1):
        xl = x.clone().requires_grad_(True)
        pl = {k: v.clone().requires_grad_(True) for k, v in p.items()}
        if which == 0:
            y = G.attnpool(xl, pl, H)
        else:
            t = xl.reshape(K, 49, C).permute(1, 0, 2)
            t = torch.cat([t.mean(0, keepdim=True), t], 0) + pl["pos"][:, None, :]
            y, _ = F.multi_head_attention_forward(
                query=t[:1], key=t, value=t, embed_dim_to_check=C, num_heads=H, q_proj_weight=pl["q_w"], k_proj_weight=pl["k_w"],
                v_proj_weight=pl["v_w"], in_proj_weight=None, in_proj_bias=torch.cat([pl["q_b"], pl["k_b"], pl["v_b"]]), bias_k=None, bias_v=None,
                add_zero_attn=False, dropout_p=0.0, out_proj_weight=pl["c_w"], out_proj_bias=pl["c_b"], use_separate_proj_weight=True,
                training=True, need_weights=False)
            y = y[0]
        y.backward(gy)
        res.append(dict(y=y.detach(), x=xl.grad, **{k: v.grad for k, v in pl.items()}))
    for k in res[0]:
        if k == "k_b":
            assert float(res[0][k].abs().max()) <= 1e-14 and float(res[1][k].abs().max()) <= 1e-14        # constant under the softmax
        else:
            assert _rel(res[0][k], res[1][k]) <= 1e-12, k


def test_required_branches_have_cases():
    names = [c["name"] for c in GC.CASES]
    assert len(set(names)) == len(names)
    for b in GC.REQUIRED_BRANCHES:
        cs = [c for c in GC.CASES if c["branch"] == b]
        assert any(set(c["dtypes"]) == {"f32", "bf16"} for c in cs), b
    assert {c["branch"] for c in GC.CASES} == set(GC.REQUIRED_BRANCHES)
    assert all(c["selects"] and c["why"] for c in GC.CASES) and set(GC.ACCUMULATE) <= set(names)
    # the RoI cross: every value of every switch meets extra present
    roi = [c for c in GC.CASES if c["kind"] == "roi" and c["extra"] != "none"]
    for key, values in (("CDDMSL_ROI_COMMUTE_DOWN", "01"), ("CDDMSL_POOL_MASK_BITS", "01")):
        assert {c["env"][key] for c in roi} == set(values)
    assert {c["feat_grad"] for c in roi} == {True, False} and {c["extra"] for c in roi} == {"grad", "nograd"}
    assert {c["extra"] for c in GC.CASES if c["kind"] == "roi"} == {"grad", "nograd", "none"}


def test_cases_build_and_limits_hold_their_caps():
    """every case builds on the CPU; every compared tensor has a non-zero maximum (k_proj.bias alone is exactly zero); no f32 limit
    above 1e-4, no bf16 limit above 3e-2.  Prints the limits table."""
    lines = []
    for c in GC.CASES:
        inp, ref, lim = G.prepared(c)
        assert list(ref) == G.compared(c)
        for n, v in ref.items():
            assert bool(torch.isfinite(v).all()), (c["name"], n)
            if lim[n] is None:
                assert n == "k_b", (c["name"], n)
                continue
            assert lim[n][0] <= G.F32_CAP, (c["name"], n, lim[n])
            assert "bf16" not in c["dtypes"] or lim[n][1] <= G.BF16_CAP, (c["name"], n, lim[n])
        w32 = max((v[0], n) for n, v in lim.items() if v)
        wbf = max((v[1], n) for n, v in lim.items() if v)
        bf = f"bf16 limit <= {wbf[0]:.2e} ({wbf[1]})" if "bf16" in c["dtypes"] else "f32 only"
        lines.append(f"{c['name']:44s} {len(ref):3d} tensors  margin {inp['margin']:.1e}  f32 limit <= {w32[0]:.2e} ({w32[1]})  {bf}")
    print("\nlimits per case (largest over its compared tensors)\n" + "\n".join(lines))


def test_every_drop_moves_a_compared_tensor():
    """for every ``drop`` name and every case it applies to: the float64 reference with that one term removed differs from the
    reference, on at least one compared tensor, by at least 10 times that tensor's limit in BOTH dtypes (graph_ref.drop_dtypes: the
    dtypes the case runs in, with one exception argued there)"""
    seen, lines = {}, []
    for c in GC.CASES:
        inp, ref, lim = G.prepared(c)
        for d in G.drops_for(c):
            mut = G.reference(c, inp, drop=d)
            worst_limit = lambda v: max(v[i] for i, t in enumerate(GC.DTYPES) if t in G.drop_dtypes(c, d))
            best = max((_rel(mut[n], ref[n]) / worst_limit(lim[n]), n) for n in ref if lim[n] is not None)
            seen.setdefault(d, []).append((best[0], c["name"], best[1]))
            assert best[0] >= 10.0, (d, c["name"], best)
    assert set(seen) == set(G.DROPS), set(G.DROPS) - set(seen)
    for d in G.DROPS:
        lo = min(seen[d])
        lines.append(f"{d:26s} {len(seen[d]):2d} cases   smallest move / limit {lo[0]:9.1f}   ({lo[1]}: {lo[2]})")
    print("\nsensitivity: one term removed from the reference\n" + "\n".join(lines))
