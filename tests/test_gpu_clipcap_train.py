"""GPU: training the ClipCap mapper on the differentiable HIP GPT-2 (cddmsl_amd/csrc/gpt2_train.hip, GPT2Decoder.caption_loss,
TransformerMapper(trainable=True), solver.AdamW, clipcap_train.py).

Kernels: against float64 torch on the same bf16- or f32-valued inputs, within the elementwise bounds tests/clipcap_train_ref.py derives
from the number formats.  The step: against float64 autograd of the plainly written modules (clipcap_train_ref.plain_step) with
tests/test_gpu_graph_exact.py's limits (f32: 8 x the plain float32 CPU run's error, floor 1e-6; bf16: 4 x the error of the plain
module with every materialised tensor rounded to bf16, floor 2^-8; metric max |got - ref| / max |ref| per tensor), and in f32 against
the reference's own modules (tests/golden/ref_clipcap_train.npz) within 1e-3, the project's parity bound for losses.
tests/test_clipcap_train_host.py shows that each single dropped term moves some compared tensor past ten times its limit."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

import clipcap_train_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
DEV = "cuda"
BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
POISON = 777.0


def _rn(g, *s):
    return torch.randn(*s, generator=g)


def _within(got, ref, bound, what):
    err = (got.detach().to("cpu", F64).reshape(ref.shape) - ref).abs()
    worst = float((err / bound).max())
    print(f"{what}: worst error / bound = {worst:.3f}, max |err| = {float(err.max()):.3e}")
    assert worst <= 1.0, what


# ---------------------------------------------------------------------------------------------------------------- kernels
@pytest.mark.parametrize("t", [1, 2, 32, 33, 64, 65, 80, 96, 97, 128])
def test_attn_causal_bwd(t):
    """every tile count of the forward's templates, one and several heads / sequences, padded rows on either operand; the poison in
    the padding columns of dqkv must survive"""
    from cddmsl_amd import hip
    g = torch.Generator().manual_seed(100 + t)
    for heads, nseq, pq, po in [(1, 1, 0, 0), (2, 3, 8, 8), (2, 1, 8, 0), (1, 3, 0, 8)]:
        W, rows = 64 * heads, nseq * t
        qkv = R.bf(_rn(g, rows, 3 * W) * 1.5)
        do = R.bf(_rn(g, rows, W))
        ref, bound = R.attn_causal_bwd_ref(qkv, do, t, heads)
        qbuf = torch.full((rows, 3 * W + pq), POISON, dtype=BF, device=DEV)
        dbuf = torch.full((rows, W + po), POISON, dtype=BF, device=DEV)
        obuf = torch.full((rows, 3 * W + pq), POISON, dtype=BF, device=DEV)
        qbuf[:, :3 * W] = qkv.to(DEV, BF)
        dbuf[:, :W] = do.to(DEV, BF)
        out = hip.attn_causal_bwd(qbuf[:, :3 * W], dbuf[:, :W], t, heads, 64 ** -0.5, out=obuf[:, :3 * W])
        again = hip.attn_causal_bwd(qbuf[:, :3 * W], dbuf[:, :W], t, heads, 64 ** -0.5)
        _within(out, ref, bound, f"attn_causal_bwd t={t} heads={heads} nseq={nseq} ldqkv=3W+{pq} ldo=W+{po}")
        assert torch.equal(out, again[:, :3 * W]), "two calls differ"
        if pq:
            assert bool((obuf[:, 3 * W:] == POISON).all()), "padding columns of dqkv were written"
        # the node: forward on the fused kernel, backward on this one
        from cddmsl_amd import layers
        leaf = qkv.to(DEV, BF).requires_grad_(True)
        layers.causal_attention_grad(leaf, t, heads, 64 ** -0.5).backward(do.to(DEV, BF))
        assert torch.equal(leaf.grad, again)


@pytest.mark.parametrize("dtype", [BF, F32])
def test_gelu_new_bwd(dtype):
    from cddmsl_amd import hip, layers
    g = torch.Generator().manual_seed(7)
    n = 4096 * 3 + 5                                  # no multiple of the 8- / 4-element vectors: the scalar tail runs
    x = torch.cat([_rn(g, n - 64) * 3.0, torch.linspace(-12, 12, 64)])
    dy = _rn(g, n)
    if dtype == BF:
        x, dy = R.bf(x), R.bf(dy)
    ref, bound = R.gelu_new_bwd_ref(x, dy, dtype == BF)
    got = hip.gelu_new_bwd(x.to(DEV, dtype), dy.to(DEV, dtype))
    _within(got, ref, bound, f"gelu_new_bwd {dtype}")
    m = n - n % 8
    leaf = x[:m].to(DEV, dtype).requires_grad_(True)  # the node keeps the value from before the activation
    y = layers.gelu_new(leaf)
    y.backward(dy[:m].to(DEV, dtype))
    assert torch.equal(leaf.grad, got[:m]) and torch.equal(y.detach(), hip.gelu_new_(leaf.detach().clone()))


@pytest.mark.parametrize("shape", [(1, 7, 8), (5, 8, 8), (3, 50257, 50264)])
@pytest.mark.parametrize("shift", [0.0, -1e4])
@pytest.mark.parametrize("ign", [0, -1])
def test_token_ce(shape, shift, ign):
    """targets at column 0 (ignored with ignore_index 0, a class with -1) and V - 1; NaN in the padding columns; logits near -1e4;
    the gradient written in place"""
    from cddmsl_amd import hip
    Rr, V, ld = shape
    g = torch.Generator().manual_seed(Rr * 1000 + V)
    lg = torch.full((Rr, ld), float("nan"))
    lg[:, :V] = _rn(g, Rr, V) * 4.0 + shift
    target = torch.tensor([V - 1, 0, 1, V // 2, 0][:Rr])          # at least half of the rows count
    if ign == -1 and Rr >= 3:
        target[-1] = -1
    loss_ref, lse_ref, d_ref, count = R.token_ce_ref(lg, target, V, ign)
    dev = lg.to(DEV)
    loss, lse, n = hip.token_ce_fwd(dev[:, :V], target.to(DEV), V, ign)
    assert n == count
    keep = target != ign
    big = float(lg[:, :V].abs().max())
    # lse = max + log(sum): one rounding at its own size, the sum's (V + 8) f32 roundings of terms <= 1
    assert float((lse.cpu().to(F64) - lse_ref)[keep].abs().max()) <= R.ulp32(big) + (V + 8) * R.U_F32
    # the loss takes (max - target logit) first, exact to a rounding of that difference, then the log term
    assert abs(float(loss) - float(loss_ref)) <= 4 * R.U_F32 * float(loss_ref) + (V + 8) * R.U_F32 + 1e-6
    for out_dtype, inplace in ((BF, False), (F32, False), (F32, True)):
        src = dev.clone()
        d = hip.token_ce_bwd(src[:, :V], target.to(DEV), lse, 0.25, V, ign, out_dtype=out_dtype, inplace=inplace)
        if inplace:
            assert d.data_ptr() == src.data_ptr()
        full = torch.as_strided(d, (Rr, ld), (ld, 1))
        assert bool((full[:, V:] == 0).all()) and bool((full[~keep.to(DEV)] == 0).all()), "padding columns / ignored rows are not zero"
        p = torch.softmax(lg[:, :V].to(F64), dim=1)
        # exp(x - lse): x - lse carries lse's rounding (an ulp at the logits' size) and the exponential 2^-21 relative; then the
        # output's own rounding
        rel = 2 * R.ulp32(big) + 2.0 ** -20 + (R.U_BF if out_dtype == BF else R.U_F32)
        bound = (p * rel + (d_ref * count).abs() * (R.U_BF if out_dtype == BF else R.U_F32)) * 0.25 + 1e-12
        _within(full[:, :V], d_ref * count * 0.25, bound, f"token_ce_bwd {shape} {shift} {out_dtype} inplace={inplace}")


def test_token_ce_all_ignored():
    from cddmsl_amd import hip
    lg = torch.randn(4, 16, device=DEV)
    with pytest.raises(ValueError):
        hip.token_ce_fwd(lg, torch.zeros(4, dtype=torch.int64, device=DEV))
    sc = torch.full((2,), 5.0, device=DEV)
    lse, row = torch.empty(4, device=DEV), torch.empty(4, device=DEV)
    st = hip._L().cddmsl_token_ce_fwd(lg.data_ptr(), 16, torch.zeros(4, dtype=torch.int64, device=DEV).data_ptr(), 4, 16, 0, lse.data_ptr(),
                                      row.data_ptr(), sc.data_ptr(), None)
    torch.cuda.synchronize()
    assert st == 0 and sc.tolist() == [0.0, 0.0]


@pytest.mark.parametrize("D", [8, 768, 1024])
@pytest.mark.parametrize("dtype", [BF, F32])
def test_layernorm_bwd_params(D, dtype):
    from cddmsl_amd import hip
    g = torch.Generator().manual_seed(D)
    for Rr in (1, 63, 64, 65, 3200):
        x = _rn(g, Rr, D) * 2.0 + 0.5
        dy = _rn(g, Rr, D)
        dy = R.bf(dy) if dtype == BF else dy
        mean, rstd = x.mean(1), (x.var(1, unbiased=False) + 1e-5).rsqrt()
        dg_ref, db_ref, bg, bb = R.layernorm_params_ref(dy, x, mean, rstd)
        args = (dy.to(DEV, dtype), x.to(DEV), mean.to(DEV), rstd.to(DEV))
        dg, db = hip.layernorm_bwd_params(*args)
        _within(dg, dg_ref, bg, f"dgamma R={Rr} D={D} {dtype}")
        _within(db, db_ref, bb, f"dbeta R={Rr} D={D} {dtype}")
        dg2, db2 = hip.layernorm_bwd_params(*args)
        assert torch.equal(dg, dg2) and torch.equal(db, db2), "two calls differ"
        base_g, base_b = _rn(g, D), _rn(g, D)
        ag, ab = hip.layernorm_bwd_params(*args, dgamma=base_g.to(DEV), dbeta=base_b.to(DEV))       # accumulate = 1
        assert torch.equal(ag, base_g.to(DEV) + dg) and torch.equal(ab, base_b.to(DEV) + db)


@pytest.mark.parametrize("step", [1, 1000])
@pytest.mark.parametrize("wd", [0.0, 0.01])
def test_adamw_step(step, wd):
    """several sizes in one call (a single element, odd sizes, one past a block); tensor 2 carries a NaN gradient element: it turns
    that element NaN, as torch does, and leaves every other element and tensor alone"""
    from cddmsl_amd import hip
    g = torch.Generator().manual_seed(step)
    sizes = [1, 3, 4, 1023, 65537]
    P = [_rn(g, n) for n in sizes]
    G = [_rn(g, n) * 0.1 for n in sizes]
    M = [(_rn(g, n) * 0.05 if step > 1 else torch.zeros(n)) for n in sizes]
    V = [(_rn(g, n) * 0.05) ** 2 if step > 1 else torch.zeros(n) for n in sizes]
    G[2][1] = float("nan")
    lr, b1, b2, eps = 1e-3, 0.9, 0.999, 1e-6
    dev = [[t.to(DEV).clone() for t in L] for L in (P, G, M, V)]
    hip.adamw_step(dev[0], dev[1], dev[2], dev[3], lr, b1, b2, eps, wd, step)
    for i, n in enumerate(sizes):
        pr, mr, vr = R.adamw_ref(P[i], G[i], M[i], V[i], lr, b1, b2, eps, wd, step)
        for name, got, ref in (("p", dev[0][i], pr), ("exp_avg", dev[2][i], mr), ("exp_avg_sq", dev[3][i], vr)):
            got = got.cpu().to(F64)
            assert torch.equal(torch.isnan(got), torch.isnan(ref)), f"NaN pattern of {name}[{i}]"
            ok = ~torch.isnan(ref)
            # a handful of f32 operations per element (<= 8 roundings of 2^-24 relative to the largest operand): 4e-6 leaves 8 x
            assert float((got - ref)[ok].abs().max()) <= 4e-6 * max(float(ref[ok].abs().max()), lr), f"{name}[{i}] n={n}"
    assert int(torch.isnan(dev[0][2]).sum()) == 1 and not any(bool(torch.isnan(dev[0][i]).any()) for i in (0, 1, 3, 4))


def test_contract_refusals():
    """each entry returns non-zero on a call outside its contract, before any launch (the buffers hold what they held)"""
    from cddmsl_amd import hip
    L = hip._L()
    vp = lambda t: ctypes.c_void_p(t.data_ptr())      # noqa: E731
    a = torch.full((129 * 200,), 3.0, dtype=BF, device=DEV)
    b = torch.full((129 * 200,), 3.0, dtype=BF, device=DEV)
    c = torch.full((129 * 200,), 3.0, dtype=BF, device=DEV)
    bad = [dict(dh=96), dict(t=129), dict(ldqkv=196), dict(ldo=68), dict(dtype=1), dict(ldqkv=184)]
    for kw in bad:
        k = dict(nseq=1, t=8, heads=1, dh=64, ldqkv=192, ldo=64, dtype=0)
        k.update(kw)
        st = L.cddmsl_attn_causal_bwd(vp(a), vp(b), vp(c), k["nseq"], k["t"], k["heads"], k["dh"], k["ldqkv"], k["ldo"], 0.125, k["dtype"], None)
        assert st != 0, kw
    f = torch.full((4, 16), 2.0, device=DEV)
    tg = torch.ones(4, dtype=torch.int64, device=DEV)
    lse, row, sc = torch.full((4,), 9.0, device=DEV), torch.full((4,), 9.0, device=DEV), torch.full((2,), 9.0, device=DEV)
    for ld, V in ((16, 17), (12, 12), (16, 0)):       # V > ld; ld no multiple of 8; no classes
        assert L.cddmsl_token_ce_fwd(vp(f), ld, vp(tg), 4, V, 0, vp(lse), vp(row), vp(sc), None) != 0
        assert L.cddmsl_token_ce_bwd(vp(f), ld, vp(tg), vp(lse), 1.0, vp(f), 4, V, 0, 1, None) != 0
    assert L.cddmsl_token_ce_bwd(vp(f), 16, vp(tg), vp(lse), 1.0, vp(f), 4, 16, 0, 0, None) != 0        # bf16 result over the f32 logits
    assert L.cddmsl_gelu_new_bwd(vp(f), vp(f), vp(f), 8, 2, None) != 0 and L.cddmsl_gelu_new_bwd(vp(f), vp(f), vp(f), -1, 1, None) != 0
    ws = torch.zeros(1 << 16, device=DEV)
    assert L.cddmsl_layernorm_bwd_params(vp(f), vp(f), vp(lse), vp(lse), vp(f), vp(f), vp(ws), 8, 4, 16, 0, 1, None) != 0     # workspace too small
    assert L.cddmsl_layernorm_bwd_params(vp(f), vp(f), vp(lse), vp(lse), vp(f), vp(f), vp(ws), ws.numel() * 4, 4, 16, 2, 1, None) != 0
    assert L.cddmsl_layernorm_bwd_params_workspace(0, 16) == -1
    ptrs = (ctypes.c_void_p * 1)(f.data_ptr())
    n1 = (ctypes.c_long * 1)(64)
    assert L.cddmsl_adamw_step(ptrs, ptrs, ptrs, ptrs, n1, 1, 1e-3, 0.9, 0.999, 1e-6, 0.0, 0, None) != 0       # step 0
    assert L.cddmsl_adamw_step(ptrs, ptrs, ptrs, ptrs, n1, 1, 1e-3, 1.0, 0.999, 1e-6, 0.0, 1, None) != 0       # beta1 = 1
    torch.cuda.synchronize()
    assert bool((c == 3.0).all()) and bool((f == 2.0).all()) and sc.tolist() == [9.0, 9.0] and bool((lse == 9.0).all())


# ---------------------------------------------------------------------------------------------------------------- the step
sys.path.insert(0, GOLD)
_CACHE = {}


def _case(name):
    """inputs, the float64 plain step, its limits and the golden of a case: computed once, shared, left unchanged"""
    if name in _CACHE:
        return _CACHE[name]
    import make_golden_clipcap_train as MG
    from cddmsl_amd.synthetic import make_gpt2_state_dict, make_mapper_state_dict
    c = MG.CASES[name]
    P = c["P"]
    x, tok = MG.case_inputs(name)
    tokens = tok.clone()
    tokens[tokens < 0] = 0
    msd = make_mapper_state_dict(c["seed"], dim_clip=MG.DIM_CLIP, dim=MG.N_EMBD, length=P, layers=2)
    gsd = make_gpt2_state_dict(0, n_layer=2, n_embd=MG.N_EMBD, vocab=MG.VOCAB, n_positions=MG.N_POS)
    kw = dict(lr=MG.LR, wd=MG.WD, eps=MG.EPS)
    torch.set_num_threads(min(16, os.cpu_count() or 8))
    ref = R.plain_step(msd, gsd, x, tokens, P, 2, F64, **kw)
    e32 = R.plain_step(msd, gsd, x, tokens, P, 2, F32, **kw)
    ebf = R.plain_step(msd, gsd, x, tokens, P, 2, F64, rb=True, **kw)
    lim = {k: (max(8 * R.rel_err(e32[k], ref[k]), 1e-6), max(4 * R.rel_err(ebf[k], ref[k]), 2.0 ** -8))
           for k in ref if float(ref[k].abs().max()) > 0}
    gold = np.load(os.path.join(GOLD, "ref_clipcap_train.npz"))
    _CACHE[name] = dict(P=P, x=x, tokens=tokens, msd=msd, gsd=gsd, ref=ref, lim=lim, gold=gold, kw=kw)
    return _CACHE[name]


def _modules(C, T):
    from cddmsl_amd.modeling import TransformerMapper
    from cddmsl_amd.modeling.gpt2 import GPT2Decoder
    mapper = TransformerMapper(C["x"].shape[1], 768, C["P"], C["P"], 2, compute_dtype=T, trainable=True)
    mapper.load_state_dict(C["msd"])
    dec = GPT2Decoder.from_state_dict(C["gsd"], T)
    return mapper.to(DEV), dec.to(DEV)


def _run_steps(C, T, steps=2):
    """the product's training step on the case -> its tensors under plain_step's names (plus "g2.<name>", the second step's gradient,
    and "m<k>.<name>" / "v<k>.<name>", the moments after step k), and the profiler's rows of the first caption_loss"""
    from cddmsl_amd import hip
    from cddmsl_amd.solver import AdamW
    mapper, dec = _modules(C, T)
    opt = AdamW(list(mapper.parameters()), lr=C["kw"]["lr"], eps=C["kw"]["eps"], weight_decay=C["kw"]["wd"])
    out, rows = {"p0." + k: p.detach().clone() for k, p in mapper.named_parameters()}, None
    for s in range(1, steps + 1):
        opt.zero_grad()
        prefix = mapper(C["x"].to(DEV))
        prefix.retain_grad()
        if s == 1:
            hip.PROFILE.enable()
        loss = dec.caption_loss(prefix, C["tokens"].to(DEV))
        loss.backward()
        if s == 1:
            rows = hip.PROFILE.collect()
            out["loss"], out["dprefix"] = loss.detach(), prefix.grad.detach().clone()
        for k, p in mapper.named_parameters():
            assert p.grad is not None, f"{k} received no gradient"
            out[("g." if s == 1 else f"g{s}.") + k] = p.grad.detach().clone()
        opt.step()
        for k, p in mapper.named_parameters():
            out[f"p{s}." + k] = p.detach().clone()
            out[f"m{s}." + k], out[f"v{s}." + k] = opt.state[id(p)]["exp_avg"].clone(), opt.state[id(p)]["exp_avg_sq"].clone()
            assert opt.state[id(p)]["step"] == s
    return out, rows, mapper, dec


@pytest.mark.parametrize("name", ["A", "B"])
@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_step_against_float64(name, dt):
    """Two steps on one batch.  Compared with the limits: the loss, d loss / d prefix and every parameter gradient of the first step
    against plain_step's; every parameter gradient of the SECOND step against float64 autograd of the plain modules at the
    product's own parameters (the weights' compute-dtype copies were refreshed, the fused q | kv copy rebuilt, the gradient buffers
    cleared), with the rule's limits taken from the plain modules at those same parameters.  The parameters themselves are not compared along the trajectory:
    Adam's update lr m / (sqrt(v) + eps) has derivative lr eps / (|g| + eps)^2 in a gradient element, 1e3 at |g| <= eps, so two
    correct runs part by a whole lr where an element's gradient is near zero (measured: case B f32, second-step gradients within
    2.3e-6 of float64 at the product's parameters, while the parameters sit 7.7e-3 from the reference trajectory's).  Instead each
    step's update is replayed in float64 (torch.optim.AdamW's arithmetic) on the product's own gradient, parameters and moments:
    elementwise within 4e-6 of the largest operand, the bound of the kernel's own test."""
    C = _case(name)
    got, rows, _, _ = _run_steps(C, F32 if dt == "f32" else BF)
    col = 0 if dt == "f32" else 1
    names = list(C["msd"])

    def second(dtype, rb=False):          # the plain modules' gradient at the product's parameters after its first step
        ps = {k: got["p1." + k].detach().cpu().to(dtype).requires_grad_(True) for k in names}
        pre = R.plain_mapper(ps, C["x"].to(dtype), C["P"], C["P"], 2, rb)
        l2 = R.plain_caption_loss({k: v.to(dtype) for k, v in C["gsd"].items()}, pre, C["tokens"], rb)
        return dict(zip(names, torch.autograd.grad(l2, [ps[k] for k in names])))

    ref2 = second(F64)
    noisy = second(F32) if dt == "f32" else second(F64, rb=True)
    worst = []
    for k in ["loss", "dprefix"] + ["g." + n for n in names] + ["g2." + n for n in names]:
        if k.startswith("g2."):           # the rule's limit, from the plain module at the same parameters
            e0 = R.rel_err(noisy[k[3:]], ref2[k[3:]])
            ref, lim = ref2[k[3:]], (max(8 * e0, 1e-6) if dt == "f32" else max(4 * e0, 2.0 ** -8))
        else:
            ref, lim = C["ref"][k], C["lim"][k][col]
        e = R.rel_err(got[k], ref)
        print(f"{name} {dt} {k}: {e:.3e} (limit {lim:.3e})")
        if not e <= lim:
            worst.append((k, e, lim))
    lr, wd, eps = C["kw"]["lr"], C["kw"]["wd"], C["kw"]["eps"]
    for s in (1, 2):
        for k in names:
            g = got[("g." if s == 1 else "g2.") + k].cpu()
            m0 = got[f"m{s - 1}." + k].cpu() if s > 1 else torch.zeros_like(g)
            v0 = got[f"v{s - 1}." + k].cpu() if s > 1 else torch.zeros_like(g)
            pr, mr, vr = R.adamw_ref(got[f"p{s - 1}." + k].cpu(), g, m0, v0, lr, 0.9, 0.999, eps, wd, s)
            for what, a, b in ((f"p{s}", got[f"p{s}." + k], pr), (f"m{s}", got[f"m{s}." + k], mr), (f"v{s}", got[f"v{s}." + k], vr)):
                e = float((a.cpu().to(F64) - b).abs().max())
                if not e <= 4e-6 * max(float(b.abs().max()), lr):
                    worst.append((what + "." + k, e))
    assert not worst, worst
    if dt == "bf16":      # the route: the fused causal backward and the token cross-entropy kernels ran
        assert {"k_attn_causal_bwd", "k_token_ce_fwd", "k_token_ce_bwd", "attn_causal", "gelu_new_bwd"} <= set(rows), sorted(rows)
        assert rows["k_attn_causal_bwd"]["launches"] == 2 and rows["k_token_ce_fwd"]["launches"] == 1
    else:
        assert "k_attn_causal_bwd" not in rows and {"k_token_ce_fwd", "k_token_ce_bwd"} <= set(rows), sorted(rows)


@pytest.mark.parametrize("name", ["A", "B"])
def test_step_f32_against_reference_modules(name):
    """the reference's own TransformerMapper + transformers' GPT-2 + torch.optim.AdamW (the golden): 1e-3 relative"""
    C = _case(name)
    got, _, _, _ = _run_steps(C, F32)
    G = C["gold"]
    rel = lambda a, b: float(np.abs(a - b).max() / np.abs(b).max())       # noqa: E731
    assert abs(float(got["loss"]) - float(G[f"{name}.loss"])) <= 1e-3 * abs(float(G[f"{name}.loss"]))
    e = rel(got["dprefix"].cpu().numpy().astype(np.float64), G[f"{name}.dprefix"].astype(np.float64))
    print(f"{name} dprefix {e:.3e}")
    assert e <= 1e-3
    bad = []
    for i, k in enumerate(G[f"{name}.names"]):
        k = str(k)
        idx = torch.from_numpy(G[f"{name}.index"][i])
        take = lambda t: t.detach().cpu().reshape(-1)[idx].numpy().astype(np.float64)       # noqa: E731
        gn = float(got["g." + k].double().norm())
        checks = [("gnorm", abs(gn - G[f"{name}.gnorm"][i]) / G[f"{name}.gnorm"][i]), ("gsample", rel(take(got["g." + k]), G[f"{name}.gsample"][i])),
                  ("p2", rel(take(got["p2." + k]), G[f"{name}.p2"][i]))]
        for what, err in checks:
            print(f"{name} {k} {what}: {err:.3e}")
            if not err <= 1e-3:
                bad.append((k, what, err))
    assert not bad, bad


# the profiler's rows of one forward + backward of the FROZEN mapper (TransformerMapper(64, 768, 4, 4, 2), bf16, n = 3), recorded from
# the class as it stood before ``trainable=`` existed: name -> launches
FROZEN_ROWS = {"attn_small": 4, "k_conv_fwd": 18, "layernorm": 8, "weight_prep": 18}


def test_frozen_mapper_route_unchanged():
    from cddmsl_amd import hip
    from cddmsl_amd.modeling import TransformerMapper
    C = _case("A")
    mapper = TransformerMapper(64, 768, 4, 4, 2, compute_dtype=BF)
    mapper.load_state_dict(C["msd"])
    mapper.to(DEV)
    assert not any(p.requires_grad for p in mapper.parameters())
    x = C["x"].to(DEV).requires_grad_(True)
    hip.PROFILE.enable()
    mapper(x).sum().backward()
    rows = {k: v["launches"] for k, v in hip.PROFILE.collect().items()}
    print("frozen mapper rows:", rows)
    assert rows == FROZEN_ROWS
    assert all(p.grad is None for p in mapper.parameters()) and x.grad is not None


# ---------------------------------------------------------------------------------------------------------------- plumbing
def _tiny_training(tmp, resume_at=None, with_gpt=True, steps=4):
    """clipcap_train.train on 6 captions of 3 images, batches of 2, one epoch of 3 steps + 1 of a second; the full-size mapper geometry
    (1024 -> 40 x 768, 8 layers) on the 2-layer GPT-2, f32"""
    from cddmsl_amd import clipcap_train as ct
    from cddmsl_amd.modeling import TransformerMapper
    from cddmsl_amd.modeling.gpt2 import GPT2Decoder
    from cddmsl_amd.synthetic import make_gpt2_state_dict, make_mapper_state_dict
    g = torch.Generator().manual_seed(5)
    toks = [[int(v) for v in torch.randint(1, 4099, (n,), generator=g)] for n in (3, 9, 5, 7, 2, 6)]
    path = os.path.join(tmp, "data.pt")
    ct.save_dataset(path, torch.randn(3, 1024, generator=g), torch.tensor([0, 0, 1, 1, 2, 2]), toks, [f"caption {i}" for i in range(6)])
    data = ct.load_dataset(path)
    dec = GPT2Decoder.from_state_dict(make_gpt2_state_dict(0, n_layer=2, n_embd=768, vocab=4099, n_positions=1024), F32).to(DEV)
    mapper = TransformerMapper(1024, 768, 40, 40, 8, compute_dtype=F32, trainable=True)
    mapper.load_state_dict(make_mapper_state_dict(1))
    mapper.to(DEV)
    return ct, data, mapper, dec


def test_checkpoint_loads_where_it_is_read(tmp_path):
    """a checkpoint written after two steps: through SimpleTrainer's MODEL.VISION_TO_LANG_PATH code and gen_captions' loader"""
    ct, data, mapper, dec = _tiny_training(str(tmp_path))
    tr = ct.train(data, mapper, dec, str(tmp_path), "run", epochs=1, bs=3, lr=1e-3, warmup_steps=1, save_steps=2, with_gpt=True, log=lambda s: None)
    assert tr.global_step == 2
    path = os.path.join(str(tmp_path), "run_latest.pt")
    assert os.path.isfile(path) and os.path.isfile(os.path.join(str(tmp_path), "run-000.pt"))
    want = {k: v.detach().cpu() for k, v in mapper.state_dict().items()}
    # gen_captions.py's loader
    from cddmsl_amd.modeling import TransformerMapper, build_model
    from cddmsl_amd.modeling.gpt2 import GPT2Decoder
    cc = torch.load(path, map_location="cpu", weights_only=True)
    m2 = TransformerMapper(1024, 768, 40, 40, 8, compute_dtype=BF)
    m2.load_state_dict({k[len("clip_project."):]: v for k, v in cc.items() if k.startswith("clip_project.")})
    assert all(torch.equal(v, want[k]) for k, v in m2.state_dict().items())
    d2 = GPT2Decoder.from_state_dict(cc, BF)
    assert all(torch.equal(v.cpu(), d2.state_dict()[k]) for k, v in dec.state_dict().items())
    # SimpleTrainer's
    from cddmsl_amd.config import get_cfg
    from cddmsl_amd.engine import SimpleTrainer
    from cddmsl_amd.solver import build_optimizer
    cfg = get_cfg()
    cfg.merge_from_file(os.path.join(ROOT, "configs", "VOC-Experiments", "faster_rcnn_CLIP_R_50_C4.yaml"))
    cfg.merge_from_list(["MODEL.VISION_TO_LANG_PATH", path, "MODEL.DEVICE", "cuda:0"])
    model = build_model(cfg)
    st = SimpleTrainer(model, iter([]), build_optimizer(cfg, model), cfg, metrics_period=0)
    assert all(torch.equal(v.cpu(), want[k]) for k, v in st.clipcap_model.state_dict().items())
    assert not any(p.requires_grad for p in st.clipcap_model.parameters())


def test_resume_is_bit_exact(tmp_path):
    """two epochs in one go against one epoch + one step, then --resume: the same weights, moments, step counts, schedule position
    and generator state, bit for bit"""
    a, b = os.path.join(str(tmp_path), "a"), os.path.join(str(tmp_path), "b")
    os.makedirs(a), os.makedirs(b)
    kw = dict(bs=2, lr=1e-3, warmup_steps=2, log=lambda s: None)
    ct, data, mapper, dec = _tiny_training(a)
    full = ct.train(data, mapper, dec, a, "run", epochs=2, save_steps=100, **kw)
    ct, data, mapper2, dec2 = _tiny_training(b)

    class Stop(Exception):
        pass

    def stop_after(s):
        if " step 4 " in s:
            raise Stop

    try:    # killed right after the checkpoint of step 4 (the first step of the second epoch)
        ct.train(data, mapper2, dec2, b, "run", epochs=2, save_steps=4, bs=2, lr=1e-3, warmup_steps=2, log=stop_after, log_every=1)
    except Stop:
        pass
    ct, data, mapper3, dec3 = _tiny_training(b)
    part = ct.train(data, mapper3, dec3, b, "run", epochs=2, save_steps=100, resume=True, **kw)
    assert part.global_step == full.global_step == 6 and part.epoch == full.epoch and part.lr_now() == full.lr_now()
    assert torch.equal(part.generator.get_state(), full.generator.get_state())
    for (k, p), q in zip(mapper.named_parameters(), mapper3.parameters()):
        assert torch.equal(p, q), k
        sa, sb = full.optimizer.state[id(p)], part.optimizer.state[id(q)]
        assert sa["step"] == sb["step"] and torch.equal(sa["exp_avg"], sb["exp_avg"]) and torch.equal(sa["exp_avg_sq"], sb["exp_avg_sq"]), k
