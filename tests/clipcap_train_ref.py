"""References for mapper training (tests/test_gpu_clipcap_train.py, tests/test_clipcap_train_host.py), on the CPU, plainly written:

* float64 references of the new kernels with the error bound each comparison may use, derived from the number formats alone;
* ``plain_step``: the whole training step -- the mapper as clipcap.py writes it, GPT-2 as modeling_gpt2 writes it, the token
  cross-entropy, AdamW -- in a chosen dtype, optionally with every materialised tensor rounded to bf16 (the bf16 limit's yardstick,
  tests/test_gpu_graph_exact.py's rule) and optionally with ONE term dropped (the host test shows each drop is visible).
"""
import math

import torch
import torch.nn.functional as F

F64, BF = torch.float64, torch.bfloat16
U_BF, U_F32 = 2.0 ** -8, 2.0 ** -24          # unit roundoffs: 8 and 24 significand bits, round to nearest
GELU_K, GELU_A = 0.7978845608028654, 0.044715


def bf(t):
    """the values a bf16 tensor holds, as float32"""
    return t.to(BF).to(torch.float32)


def rel_err(got, ref):
    """max |got - ref| / max |ref| (the metric of tests/graph_ref.py)"""
    ref = ref.detach().to(F64)
    return float((got.detach().to("cpu", F64).reshape(ref.shape) - ref).abs().max()) / float(ref.abs().max())


# ---------------------------------------------------------------------------------------------------------------- kernels
def attn_causal_bwd_ref(qkv, dout, t, heads):
    """qkv [R, 3W], dout [R, W] (bf16 values, any float dtype) -> float64 (dqkv [R, 3W], bound [R, 3W]).

    bound: the kernel rounds P and dS to bf16 before the products that contract them (relative 2^-8 each: 8 significand bits) and
    its results to bf16 (2^-8): |error of sum_i a_i b_i| <= 2^-8 sum |a_i b_i| + 2^-8 |result| <= 2^-7 sum |a_i| |b_i|.  The f32 accumulation, the
    hardware exponential and the f32 softmax add relative 1e-5 of the same sums at most; a floor of 1e-6 of the largest reference
    entry covers entries whose sums cancel to nothing."""
    R, W = dout.shape
    n, dh = R // t, W // heads
    x = qkv.to(F64).view(n, t, 3, heads, dh).permute(2, 0, 3, 1, 4).detach().requires_grad_(True)       # [3, n, H, t, dh]
    q, k, v = x[0], x[1], x[2]
    mask = torch.full((t, t), float("-inf"), dtype=F64).triu_(1)
    P = torch.softmax((q @ k.transpose(-1, -2)) * dh ** -0.5 + mask, dim=-1)
    o = P @ v
    do = dout.to(F64).view(n, t, heads, dh).permute(0, 2, 1, 3)
    (o * do).sum().backward()
    back = lambda g: g.permute(1, 3, 0, 2, 4).reshape(R, 3 * W)                                         # noqa: E731
    with torch.no_grad():
        dP = do @ v.transpose(-1, -2)
        dS = P * (dP - (dP * P).sum(-1, keepdim=True)) * dh ** -0.5
        bq = dS.abs() @ k.abs()
        bk = dS.abs().transpose(-1, -2) @ q.abs()
        bv = P.transpose(-1, -2) @ do.abs()
        bound = back(torch.stack([bq, bk, bv])) * (2.0 ** -7 + 1e-5)
    ref = back(x.grad)
    return ref, bound + 1e-6 * float(ref.abs().max())


def gelu_new_grad_ref(x):
    x = x.to(F64)
    th = torch.tanh(GELU_K * (x + GELU_A * x ** 3))
    return 0.5 * (1 + th) + 0.5 * x * (1 - th * th) * GELU_K * (1 + 3 * GELU_A * x * x)


def gelu_new_bwd_ref(x, dy, out_bf16):
    """-> float64 (dx, bound).  The derivative is g(th) = 0.5 (1 + th) + 0.5 x (1 - th^2) c with c = k (1 + 3 a x^2): an error d in
    the f32 tanh (4 ulp at 1 = 2^-21 allowed) moves it by |0.5 - x th c| d <= (0.5 + |x| c) d; its own dozen f32 operations add
    12 * 2^-24 of the magnitudes they combine, 0.5 + |x| c at most.  The product with dy and, for bf16, the result's rounding (2^-8)
    are relative to the result."""
    x64, dy64 = x.to(F64), dy.to(F64)
    g = gelu_new_grad_ref(x64)
    amp = 0.5 + x64.abs() * GELU_K * (1 + 3 * GELU_A * x64 * x64)
    ref = dy64 * g
    bound = dy64.abs() * amp * (2.0 ** -21 + 12 * U_F32) + ref.abs() * (2 * U_F32 + (U_BF if out_bf16 else 0.0))
    return ref, bound + 1e-30


def token_ce_ref(logits, target, V, ignore_index=0):
    """logits [R, >= V] f32 -> float64 (mean loss, lse [R], d loss / d logits[:, :V] for gscale = 1 / count, count)"""
    lg = logits[:, :V].to(F64).detach().requires_grad_(True)
    keep = target != ignore_index
    count = int(keep.sum())
    loss = F.cross_entropy(lg, target, ignore_index=ignore_index, reduction="sum") / max(count, 1)
    loss.backward()
    return loss.detach(), torch.logsumexp(lg.detach(), dim=1), lg.grad, count


def ulp32(x):
    """the spacing of float32 at |x|"""
    return 2.0 ** (math.floor(math.log2(max(abs(float(x)), 2.0 ** -126))) - 23)


def layernorm_params_ref(dy, x, mean, rstd):
    """-> float64 (dgamma, dbeta, bound_gamma, bound_beta): sums of R terms in f32, each partial sum rounded once: (R + 8) 2^-24 of
    the sum of magnitudes (xhat itself costs three roundings of the 8)"""
    dy, x, mean, rstd = dy.to(F64), x.to(F64), mean.to(F64), rstd.to(F64)
    xh = (x - mean[:, None]) * rstd[:, None]
    R = x.shape[0]
    return ((dy * xh).sum(0), dy.sum(0), (dy * xh).abs().sum(0) * (R + 8) * U_F32 + 1e-30, dy.abs().sum(0) * (R + 8) * U_F32 + 1e-30)


def adamw_ref(p, g, m, v, lr, beta1, beta2, eps, wd, step):
    """torch.optim.AdamW (single-tensor path) in float64 on float32-valued inputs, ``step`` the step being taken -> (p, m, v)"""
    p, g, m, v = (t.to(F64).clone() for t in (p, g, m, v))
    q = torch.nn.Parameter(p)
    q.grad = g
    opt = torch.optim.AdamW([q], lr=lr, betas=(beta1, beta2), eps=eps, weight_decay=wd, foreach=False)
    opt.state[q] = {"step": torch.tensor(float(step - 1)), "exp_avg": m, "exp_avg_sq": v}
    opt.step()
    return q.detach(), m, v


# ---------------------------------------------------------------------------------------------------------------- the plain step
class _RoundBf16(torch.autograd.Function):
    @staticmethod
    def forward(ctx, t):
        return t.to(BF).to(t.dtype)

    @staticmethod
    def backward(ctx, g):
        return g.to(BF).to(g.dtype)


def _r(t, on):
    return _RoundBf16.apply(t) if on else t


def _ln(x, w, b, drop_w=False, drop_b=False):
    w = w.detach() if drop_w else w
    b = b.detach() if drop_b else b
    return F.layer_norm(x, (x.shape[-1],), w, b, 1e-5)


def plain_mapper(msd, x, P, clip_length, layers, rb=False, drop=None):
    """clipcap.py TransformerMapper.forward (8 heads, pre-norm, ReLU MLP of ratio 2, bias-free q / kv): msd = named parameters"""
    n, d, H = x.shape[0], msd["prefix_const"].shape[1], 8
    h = _r(F.linear(_r(x, rb), _r(msd["linear.weight"], rb), msd["linear.bias"]), False).view(n, clip_length, d)
    h = torch.cat((h, msd["prefix_const"].unsqueeze(0).expand(n, P, d)), dim=1)
    t = h.shape[1]
    for i in range(layers):
        q_ = f"transformer.layers.{i}."
        y = _r(_ln(h, msd[q_ + "norm1.weight"], msd[q_ + "norm1.bias"], drop == f"ln_gamma_{i}", drop == f"ln_beta_{i}"), rb)
        q = _r(F.linear(y, _r(msd[q_ + "attn.to_queries.weight"], rb)), rb).view(n, t, H, d // H)
        kv = _r(F.linear(y, _r(msd[q_ + "attn.to_keys_values.weight"], rb)), rb).view(n, t, 2, H, d // H)
        att = torch.einsum("bnhd,bmhd->bnmh", q, kv[:, :, 0]) * (d // H) ** -0.5
        att = _r(att.softmax(dim=2), rb)
        o = _r(torch.einsum("bnmh,bmhd->bnhd", att, kv[:, :, 1]).reshape(n, t, d), rb)
        h = h + F.linear(o, _r(msd[q_ + "attn.project.weight"], rb), msd[q_ + "attn.project.bias"])
        y = _r(_ln(h, msd[q_ + "norm2.weight"], msd[q_ + "norm2.bias"]), rb)
        f = _r(F.relu(F.linear(y, _r(msd[q_ + "mlp.fc1.weight"], rb), msd[q_ + "mlp.fc1.bias"])), rb)
        h = h + F.linear(f, _r(msd[q_ + "mlp.fc2.weight"], rb), msd[q_ + "mlp.fc2.bias"])
    return h[:, clip_length:]


def plain_caption_loss(gsd, prefix, tokens, rb=False, drop=None):
    """GPT-2 (bare names, Conv1D weights [in, out]) on cat(prefix, wte[tokens]) and ClipCap's loss; tokens carry 0 for the pads"""
    E = prefix.shape[2]
    n, P, L = prefix.shape[0], prefix.shape[1], tokens.shape[1]
    t, H = P + L, E // 64
    n_layer = len({k.split(".")[1] for k in gsd if k.startswith("h.")})
    x = torch.cat((prefix, gsd["wte.weight"][tokens]), dim=1) + gsd["wpe.weight"][:t]
    mask = torch.full((t, t), float("-inf"), dtype=x.dtype).triu_(1)
    for i in range(n_layer):
        q_ = f"h.{i}."
        y = _r(F.layer_norm(x, (E,), gsd[q_ + "ln_1.weight"], gsd[q_ + "ln_1.bias"], 1e-5), rb)
        qkv = _r(y @ _r(gsd[q_ + "attn.c_attn.weight"], rb) + gsd[q_ + "attn.c_attn.bias"], rb)
        q, k, v = qkv.view(n, t, 3, H, 64).permute(2, 0, 3, 1, 4)
        s = (q @ k.transpose(-1, -2)) * 64 ** -0.5
        att = torch.softmax(s + mask, dim=-1)
        if drop == "causal_mask_bwd":        # the forward's probabilities with the gradient of attention over ALL keys
            leak = torch.softmax(s, dim=-1)
            att = att.detach() + (leak - leak.detach())
        att = _r(att, rb)
        o = _r((att @ v).permute(0, 2, 1, 3).reshape(n, t, E), rb)
        x = x + (o @ _r(gsd[q_ + "attn.c_proj.weight"], rb) + gsd[q_ + "attn.c_proj.bias"])
        y = _r(F.layer_norm(x, (E,), gsd[q_ + "ln_2.weight"], gsd[q_ + "ln_2.bias"], 1e-5), rb)
        hpre = _r(y @ _r(gsd[q_ + "mlp.c_fc.weight"], rb) + gsd[q_ + "mlp.c_fc.bias"], rb)
        th = torch.tanh(GELU_K * (hpre + GELU_A * hpre ** 3))
        if drop == "tanh_derivative":
            th = th.detach()
        hact = _r(0.5 * hpre * (1.0 + th), rb)
        x = x + (hact @ _r(gsd[q_ + "mlp.c_proj.weight"], rb) + gsd[q_ + "mlp.c_proj.bias"])
    rows = x[:, P - 1:t - 1].reshape(n * L, E)
    y = _r(F.layer_norm(rows, (E,), gsd["ln_f.weight"], gsd["ln_f.bias"], 1e-5), rb)
    logits = y @ _r(gsd["wte.weight"], rb).t()
    tg = tokens.reshape(-1)
    if drop == "ignored_row":                # an ignored row counted after all: its target is class 0
        return F.cross_entropy(logits, tg)
    return F.cross_entropy(logits, tg, ignore_index=0)


def plain_adamw(p, g, m, v, lr, beta1, beta2, eps, wd, step, drop=None):
    """torch.optim.AdamW's arithmetic on tensors of one dtype, in place on m, v; returns the new p"""
    bc1 = 1.0 if drop == "bias_correction" else 1 - beta1 ** step
    bc2 = 1.0 if drop == "bias_correction" else 1 - beta2 ** step
    p = p * (1 - lr * wd)
    m.lerp_(g, 1 - beta1)
    v.mul_(beta2).addcmul_(g, g, value=1 - beta2)
    return p - (lr / bc1) * m / (v.sqrt() / math.sqrt(bc2) + eps)


def plain_step(msd, gsd, x, tokens, P, layers, dtype=F64, rb=False, drop=None, steps=2, lr=1e-3, wd=0.01, eps=1e-6):
    """``steps`` training steps on one batch -> dict: "loss", "dprefix", per parameter "g.<name>" (first step's gradient) and
    "p<k>.<name>" (the parameter after step k).  Everything in ``dtype`` on the CPU."""
    ps = {k: v.to(dtype).clone().requires_grad_(True) for k, v in msd.items()}
    gs = {k: v.to(dtype) for k, v in gsd.items()}
    ms = {k: torch.zeros_like(v) for k, v in ps.items()}
    vs = {k: torch.zeros_like(v) for k, v in ps.items()}
    out = {}
    for s in range(1, steps + 1):
        prefix = plain_mapper(ps, x.to(dtype), P, P, layers, rb, drop)
        prefix.retain_grad()
        loss = plain_caption_loss(gs, prefix, tokens, rb, drop)
        grads = torch.autograd.grad(loss, [prefix] + list(ps.values()), allow_unused=True)
        gp = {k: (torch.zeros_like(p) if g is None else g) for (k, p), g in zip(ps.items(), grads[1:])}
        if s == 1:
            out["loss"], out["dprefix"] = loss.detach(), grads[0].detach()
            out.update({"g." + k: g.detach() for k, g in gp.items()})
        with torch.no_grad():
            for k in ps:
                new = plain_adamw(ps[k].detach(), _r(gp[k], False), ms[k], vs[k], lr, 0.9, 0.999, eps, wd, s, drop)
                ps[k] = new.requires_grad_(True)
                out[f"p{s}." + k] = new.detach().clone()
    return out


DROPS = ("causal_mask_bwd", "tanh_derivative", "ignored_row", "ln_gamma_0", "bias_correction")
