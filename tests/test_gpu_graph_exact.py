"""GPU: every hand-written autograd node of cddmsl_amd/layers.py and the stock ResNet's stage node (cddmsl_amd/modeling/resnet.py
StockStageFn), branch by branch (tests/graph_exact_cases.py), against float64 autograd of the plainly written module
(tests/graph_ref.py) on the same bf16-valued inputs, in f32 and in bf16.

Metric per tensor: max |got - ref| / max |ref|.  Limits come from the plain module alone (graph_ref.prepared): f32 -- 8 times the
error of the plain module run in float32 on the CPU, floor 1e-6; bf16 -- 4 times the error of the plain module with every
materialised tensor rounded to bf16, floor 2^-8; both recomputed here from the case's inputs.  tests/test_graph_ref_host.py shows that
each single dropped term of a backward pass moves some compared tensor by ten times its limit.

Routes are confirmed where a case names one: profiler rows (hip.PROFILE) for the sliced input gradient, the fused pooled residual
against its avgpool2_bwd fallback and the given pooled map; ``ctx`` fields for the attention pool's fused input gradient, the RoI
stage's ``on_map`` and the mask bits a pooled block keeps; the type and the saved tensors of the stock stage's node.

Measured on one MI355X, the ``stock_stage`` cases: worst error / limit over the compared tensors (the tensor), f32 then bf16.
  stock_s1_shortcut     0.179 (b0.w1)  0.366 (y)        stock_s1_two_blocks   0.302 (b0.w3)  0.265 (dx)
  stock_s2_odd          0.222 (b0.w1)  0.275 (y)        stock_s2_even         0.216 (b0.w2)  0.467 (dx)
  stock_no_dx           0.221 (b0.w0)  0.317 (y)        stock_res5_crops      0.308 (b0.w2)  0.321 (dx)
  stock_s1_two_blocks_natural 0.338 (b1.w2)             stock_s2_odd_natural  0.184 (b0.w2)
Below 0.05, the mark of a loose limit: the shortcut's weight gradient of a ONE-block case in bf16 (b0.w3: 1e-7 against a limit of
1e-2, as in f32).  Its operands are the stage's input and the incoming gradient masked by the output's sign -- bf16 values given, no
rounded intermediate, and the node hands the FrozenBN scale to the weight-gradient kernel, which applies it in f32 -- so the node's
result is as good as f32, while the rounded model rounds the scaled gradient to bf16 in front of the convolution's backward pass.
The same tensor is held at 0.15 to 0.23 where a second block follows (two_blocks, res5_crops).  stock_res5_crops y in bf16 sits
at 0.050: the mean over 49 pixels averages the roundings out, and the node rounds at fewer places than the model."""
import pytest
import torch

import graph_exact_cases as GC
import graph_ref as G

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF = torch.bfloat16
DT = {"f32": torch.float32, "bf16": BF}
PARAMS = [(c["name"], t) for c in GC.CASES for t in c["dtypes"]]


def _param(t, channels_last=False):
    p = t.to(DEV)
    if channels_last and p.dim() == 4:
        p = p.contiguous(memory_format=torch.channels_last)
    return torch.nn.Parameter(p, requires_grad=True)


def _blocks(spec, params, prefix=""):
    """graph_ref's block dicts -> layers.BlockParams (trainable, fp8 off), as tests/test_gpu_three_passes.py ``_blocks`` builds them"""
    from cddmsl_amd import layers
    out = []
    for bi, b in enumerate(spec):
        w = [None if v is None else _param(v, True) for v in b["w"]]
        bn = [None if v is None else (v[0].to(DEV).contiguous(), v[1].to(DEV).contiguous()) for v in b["bn"]]
        bp = layers.BlockParams(*w, *bn, b["stride"], False)
        bp.fp8 = False
        out.append(bp)
        for wi, v in enumerate(w):
            if v is not None:
                params[f"{prefix}b{bi}.w{wi}"] = v
    return out


def _stock_stage(spec, case, params):
    """graph_ref's block dicts -> resnet.Stage of BottleneckBlocks built directly.  The FrozenBN buffers are not the trivial ones: running
    statistics drawn from the case's seed, weight and bias chosen so that the fold gives the case's (scale, bias) -- exactly, since the
    reference keeps the case's own numbers: running_var + eps is 1/4, 1 or 4 in f32 (its rsqrt is exact), running_mean a multiple of 1/8,
    so every step of ``affine()`` is exact in f32.  Checked here, bit for bit."""
    from cddmsl_amd.modeling import resnet
    g = torch.Generator().manual_seed(case["seed"] + 7)
    cin, planes = case["x"][-1], case["planes"]
    blocks = []
    for bi, b in enumerate(spec):
        blk = resnet.BottleneckBlock(cin, 4 * planes, planes, b["stride"]).to(DEV)
        assert (blk.shortcut is not None) == (b["w"][3] is not None)
        for wi, m in enumerate((blk.conv1, blk.conv2, blk.conv3, blk.shortcut)):
            if m is None:
                continue
            m.weight.data.copy_(b["w"][wi].to(DEV))
            assert m.weight.requires_grad and m.weight.permute(0, 2, 3, 1).is_contiguous()
            params[f"b{bi}.w{wi}"] = m.weight
            sc, bias = (v.float() for v in b["bn"][wi])
            n, eps = sc.numel(), m.norm.eps
            p4 = torch.pow(4.0, torch.randint(-1, 2, (n,), generator=g).float())
            var = p4 - eps
            for _ in range(4):          # (the f32 number next to p4 - eps whose f32 sum with eps is p4 itself)
                d = (var + eps) - p4
                var = torch.where(d > 0, torch.nextafter(var, -p4), torch.where(d < 0, torch.nextafter(var, 2 * p4), var))
            assert torch.equal(var + eps, p4)
            mean = torch.randint(-8, 9, (n,), generator=g).float() / 8
            beta = bias + mean * sc
            assert torch.equal((beta.double() - mean.double() * sc.double()).float(), bias) and torch.equal(beta.double(), bias.double() + mean.double() * sc.double())
            for name, v in (("weight", sc * p4.sqrt()), ("bias", beta), ("running_mean", mean), ("running_var", var)):
                getattr(m.norm, name).copy_(v.to(DEV))
            fs, fb = (v.cpu() for v in m.norm.affine())
            assert torch.equal(fs, sc) and torch.equal(fb, bias), "the FrozenBN fold does not return the case's scale and bias"
        blocks.append(blk)
        cin = 4 * planes
    return resnet.Stage(*blocks).train()


def _attn_params(inp, case, params):
    from cddmsl_amd import layers
    p = {n: _param(v) for n, v in inp["p"].items()}
    if not case["frozen"]:
        params.update(p)
    return p, layers.AttnPoolParams(p["pos"], p["q_w"], p["q_b"], p["k_w"], p["k_b"], p["v_w"], p["v_b"], p["c_w"], p["c_b"], case["heads"], case["frozen"])


def run_node(case, inp, T, passes=1):
    """the node on the case's inputs -> (tensors by the names of graph_ref.compared, parameters that must have received a gradient,
    notes on the route taken).  ``passes``: forward + backward that many times into the same .grad buffers."""
    from cddmsl_amd import hip, layers
    k = case["kind"]
    data = lambda n, grad, dtype=T: inp[n].to(DEV, dtype).requires_grad_(bool(grad))
    params, leaves, notes = {}, {}, {}
    layers.take_touched()
    hip.PROFILE.enable()
    try:
        return _run_node(case, inp, T, passes, k, data, params, leaves, notes)
    finally:
        hip.PROFILE.on = False


def _run_node(case, inp, T, passes, k, data, params, leaves, notes):
    from cddmsl_amd import hip, layers
    for _ in range(passes):
        if k == "conv":
            if not leaves:
                leaves["dx"] = data("x", case["x_grad"])
                w = _param(inp["w"], True)
                b = _param(inp["b"]) if case["bias"] else None
                pw = layers.PreparedWeight(w, None, not case["train_w"])
                if case["residual"]:      # f32 with out_f32 on the bf16 path, else the compute dtype
                    leaves["dres"] = data("res", True, torch.float32 if case["out_f32"] else T)
                if case["train_w"]:
                    params.update({"w": w}, **({"b": b} if b is not None else {}))
            res = leaves.get("dres")
            if len(case["w"]) == 2:
                y = layers.linear(leaves["dx"], pw, b, case["relu"], case["out_f32"], case["train_w"], res)
            else:
                y = layers.conv(leaves["dx"], pw, b, case["stride"], case["pad"], case["relu"], case["out_f32"], case["train_w"], res)
            notes["unused"] = [] if case["train_w"] else [w] + ([b] if b is not None else [])
        elif k == "heads":
            if not leaves:
                leaves["dx"] = data("x", True)
                heads = [(_param(inp[f"w{i}"]), _param(inp[f"b{i}"])) for i in range(len(case["widths"]))]
                for i, (w, b) in enumerate(heads):
                    params[f"w{i}"], params[f"b{i}"] = w, b
            y = layers.fused_heads(leaves["dx"], heads, case["out_f32"])
            assert y.dtype == (torch.float32 if case["out_f32"] else T)
            assert float(y[..., sum(case["widths"]):].abs().max()) == 0.0, "the pad column of the fused heads' output is not zero"
        elif k == "mlp":
            if not leaves:
                leaves["dx"], leaves["dres"] = data("x", True), data("res", True, torch.float32)
                pw1, pw2 = (layers.PreparedWeight(_param(inp[n]), None, True) for n in ("w1", "w2"))
                b1, b2 = inp["b1"].to(DEV), inp["b2"].to(DEV)
            y = layers.frozen_mlp(leaves["dx"], pw1, b1, pw2, b2, leaves["dres"])
        elif k == "stage":
            if not leaves:
                leaves["dx"] = x = data("x", case["x_grad"])
                blocks = _blocks(inp["blocks"], params)
                N, H, W, C = x.shape
                if case["px"] == "match":
                    x._pooled2 = hip.avgpool2_fwd(x.detach())
                    notes["own_pool"] = 1                 # (this launch is in the profiler's rows as well)
                elif case["px"] == "mismatch":
                    x._pooled2 = torch.full((N, H // 2 + 1, W // 2, C), float("nan"), device=DEV, dtype=T)
            y = layers.res_stage(leaves["dx"], blocks, False, out_grad_premasked=case["premasked"])
            notes["saved_o2"] = y.grad_fn.saved_tensors[2].dtype
        elif k == "stock_stage":
            if not leaves:
                leaves["dx"] = data("x", case["x_grad"])
                stock = _stock_stage(inp["blocks"], case, params)
            y = stock.forward_nhwc(leaves["dx"])
            notes["stock_node"] = (type(y.grad_fn).__name__, len(y.grad_fn.saved_tensors))
            assert y.dtype == T
            if case["pool"]:
                y = layers.mean_pool(y)
        elif k == "halves":
            if not leaves:
                leaves["dx"], leaves["dxb"] = data("x", True), data("xb", True)
                blocks = _blocks(inp["blocks"], params)
            spec = hip.OutSpec()
            a = layers.res_stage(leaves["dx"], blocks, False, out_spec=spec)
            b = layers.res_stage(leaves["dxb"], blocks, False, out_spec=spec)
            assert spec.used == 2 and a.data_ptr() == spec.full.data_ptr(), "the two stages did not write the halves of one buffer"
            y = layers.stack_halves(a, b, spec.full)
        elif k == "roi":
            if not leaves:
                leaves["dfeat"] = data("feat", case["feat_grad"])
                if "extra" in inp:
                    leaves["dextra"] = data("extra", case["extra"] == "grad")
                blocks = _blocks(inp["blocks"], params)
                rois = inp["rois"].to(DEV)
                roi_start = torch.tensor(G.ROI_START, device=DEV, dtype=torch.int32)
            y = layers.roi_stage(leaves["dfeat"], rois, roi_start, blocks, False, 14, 1.0 / 16, 0, leaves.get("dextra"))
            notes["on_map"] = y.grad_fn.meta[4]
            notes["saved_o2"] = y.grad_fn.saved_tensors[5].dtype
        elif k == "attn":
            if not leaves:
                leaves["dx"] = data("x", case["x_grad"])
                p, ap = _attn_params(inp, case, params)
                blocks = _blocks(inp["blocks"], params) if case["stage"] else None
            if case["stage"]:
                y = layers.res_stage_attnpool(leaves["dx"], blocks, False, ap)
            else:
                y = layers.AttnPoolFn.apply(leaves["dx"], None if case["frozen"] else p["q_w"], ap, case["premask"])
            notes["fused_dx"] = y.grad_fn.fused_dx
            notes["unused"] = list(p.values()) if case["frozen"] else []
        elif k == "meanpool":
            if not leaves:
                leaves["dx"] = data("x", True)
            y = layers.mean_pool(leaves["dx"])
        else:
            raise KeyError(k)
        gy = inp["gy"].to(DEV, y.dtype)
        y.backward(gy)
    notes["rows"] = [e[0] for e in hip.PROFILE.events]
    hip.PROFILE.collect()
    torch.cuda.synchronize()
    if "dres" in leaves and k == "conv":
        assert leaves["dres"].grad.dtype == gy.dtype and torch.equal(leaves["dres"].grad, gy * passes), "the residual's gradient is not the incoming one"
    out = {"y": y.detach()}
    for n in G.compared(case)[1:]:
        t = leaves[n] if n in leaves else params[n]
        assert t.grad is not None, (case["name"], n, "received no gradient")
        out[n] = t.grad
    for t in notes.get("unused", []):
        assert t.grad is None, "a frozen parameter received a gradient"
    if k == "stock_stage" and case["x_grad"] and case["strides"][0] == 2:
        # a stride-2 1x1 reads the even pixels alone: every odd row and column of dx (on an even map the last ones) is exactly zero
        dx = out["dx"]
        assert float(dx[:, 1::2].abs().max()) == 0.0 and float(dx[:, :, 1::2].abs().max()) == 0.0, "dx of an unread pixel is not exactly zero"
        if case["x"][1] % 2 == 0:
            assert not bool(dx[:, -1].any()) and not bool(dx[:, :, -1].any()), "the last row / column of dx is not exactly zero"
    return out, params, notes


def _check_route(case, tname, notes):
    """the branch the case names was the one taken"""
    k, rows = case["kind"], notes["rows"]
    bf = tname == "bf16"
    if k == "conv" and case["route"]:
        assert ("gemm_nt_batched" in rows) == (case["route"] == "sliced"), rows
    if k == "stage":
        if case["pooled"] is not None and case["x_grad"]:
            # one avgpool2_bwd launch for dp2; the downsample path's only on the fallback route
            assert rows.count("avgpool2_bwd") == (1 if case["pooled"] else 2), rows
        if case["px"] != "none":
            assert rows.count("avgpool2_fwd") - notes.get("own_pool", 0) == (1 if case["px"] == "match" else 2), rows
        if case["strides"][0] > 1:
            bits = bf and case["env"]["CDDMSL_POOL_MASK_BITS"] == "1"
            assert notes["saved_o2"] == (torch.int32 if bits else DT[tname]), notes["saved_o2"]
    if k == "roi":
        assert notes["on_map"] == case["on_map"]
        bits = bf and case["env"]["CDDMSL_POOL_MASK_BITS"] == "1"
        assert notes["saved_o2"] == (torch.int32 if bits else DT[tname]), notes["saved_o2"]
    if k == "attn":
        assert notes["fused_dx"] == (case["fused"] and bf), notes["fused_dx"]
    if k == "stock_stage":      # the hand-written node (not a frozen stage's plain forward): it saved x and (o1, o2, out) of every block
        assert notes["stock_node"] == ("StockStageFnBackward", 1 + 3 * len(case["strides"])), notes["stock_node"]


_results = {}


def _evaluate(name, tname):
    """-> [(tensor, error, limit)] of one case in one dtype, run once; the per-call switches are set through MonkeyPatch"""
    if isinstance(_results.get((name, tname)), Exception):
        raise RuntimeError(f"{name} {tname} failed before: {_results[(name, tname)]!r}")        # (never run a failed case a second time)
    if (name, tname) not in _results:
        case = GC.BY_NAME[name]
        inp, ref, lim = G.prepared(case)
        try:
            with pytest.MonkeyPatch.context() as mp:
                for key, v in case["env"].items():
                    mp.setenv(key, v)
                got, _, notes = run_node(case, inp, DT[tname])
            _check_route(case, tname, notes)
        except Exception as e:
            _results[(name, tname)] = e
            raise
        rows = []
        for n, r in ref.items():
            assert bool(torch.isfinite(got[n].float()).all()), (name, tname, n)
            if lim[n] is None:
                assert float(got[n].abs().max()) == 0.0, (name, tname, n, "must be exactly zero")
            else:
                rows.append((n, G.rel_err(got[n], r), lim[n][GC.DTYPES.index(tname)]))
        _results[(name, tname)] = rows
    return _results[(name, tname)]


@pytest.mark.parametrize("name,tname", PARAMS, ids=[f"{n}-{t}" for n, t in PARAMS])
def test_node_against_float64_autograd(name, tname):
    rows = _evaluate(name, tname)
    for n, err, limit in rows:
        print(f"{name} {tname} {n}: error {err:.3e} limit {limit:.3e} ratio {err / limit:.3f}")
    bad = [(n, err, limit) for n, err, limit in rows if not err <= limit]
    assert not bad, bad


@pytest.mark.parametrize("name", GC.ACCUMULATE)
def test_gradients_accumulate(name):
    """two forward + backward passes into the same .grad, f32: every parameter gradient is twice the reference's within the limit, and
    layers.take_touched() names exactly the parameters that received one"""
    from cddmsl_amd import layers
    case = GC.BY_NAME[name]
    inp, ref, lim = G.prepared(case)
    with pytest.MonkeyPatch.context() as mp:
        for key, v in case["env"].items():
            mp.setenv(key, v)
        got, params, _ = run_node(case, inp, torch.float32, passes=2)
    assert params and layers.take_touched() == {id(p) for p in params.values()}
    assert layers.take_touched() == set()
    for n, p in params.items():
        if lim[n] is None:
            assert float(p.grad.abs().max()) == 0.0, n
        else:
            err = G.rel_err(got[n], 2.0 * ref[n])
            print(f"{name} accumulate {n}: error {err:.3e} limit {lim[n][0]:.3e}")
            assert err <= lim[n][0], (n, err, lim[n][0])


def test_worst_ratio_table(capsys):
    """one row per case and dtype: the worst error / limit and the tensor it occurred on; every REQUIRED_BRANCHES entry in both dtypes"""
    lines, seen = [], set()
    for name, tname in PARAMS:
        if isinstance(_results.get((name, tname)), Exception):
            lines.append(f"{name:44s} {tname:5s} not evaluated: {_results[(name, tname)]!r:.120}")
            continue
        rows = _evaluate(name, tname)
        n, err, limit = max(rows, key=lambda r: r[1] / r[2])
        seen.add((GC.BY_NAME[name]["branch"], tname))
        lines.append(f"{name:44s} {tname:5s} worst error / limit {err / limit:6.3f}  ({n}: {err:.2e} of {limit:.2e})")
    with capsys.disabled():
        print("\nnodes against float64 autograd: worst ratio per case and dtype\n" + "\n".join(lines))
    assert seen >= {(b, t) for b in GC.REQUIRED_BRANCHES for t in GC.DTYPES}
