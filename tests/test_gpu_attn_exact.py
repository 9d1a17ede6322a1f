"""Attention kernels against float64 references of the operands they were given (tests/exact_attn.py): cddmsl_attn_small_fwd/bwd,
cddmsl_attn_last_fwd/bwd, cddmsl_attn_tokens_fwd_mask, cddmsl_attnpool_softmax_fwd/bwd (both forms) and cddmsl_attnpool_dx, at the
bench's shapes and at the edges of each contract, called through the C-ABI with NaN-filled outputs and row strides wider than the
data; and the whole attention pool (layers.AttnPoolFn) at the bench's region counts, stage by stage.

The bench shapes, from one bf16 training step of bench.py's setup (800x1333, iteration past burn-in, shapes recorded at the hip
wrappers):
  mapper (ClipCap TransformerMapper via v2l, 2N + 2K rows: N images, K = 16 N regions):  n = 544 sequences at 16 images,
      1088 at 32; t = 80 tokens, 8 heads of 96, scale 96^-0.5; q / k / v standard deviation 0.56, |max| 2.8
  attention pool (2048 channels, 32 heads of 64, 7x7 map, scale 1/8):  K = 544 (the 2N image crops + 2K region crops) and
      8192 (the RoI head's 512 regions per image) at 16 images -- the batch counts of tests/golden/bench_gemm_launches.json;
      map standard deviation 0.86, positional embedding 0.022, scores 8.2 (scaled spread up to 6.7), U 0.19
cddmsl_attnpool_dx at K = 8192 runs 32 regions per block (bpb = ceil(C/128 * K / 4096)), 256 full runs."""
import ctypes

import pytest
import torch

import exact_attn as A
import exact_gemm as X

pytestmark = pytest.mark.gpu

DEV = "cuda"
MAPPER_N = {16: 544, 32: 1088}
POOL_K = {16: (544, 8192)}
MAPPER_SCALE = 96 ** -0.5
C_ACC_U = X.C_ACC * X.U_F32
WORST = {}                          # kernel output -> worst |err| / bound of this module's checks (printed at the module's end)


@pytest.fixture(scope="module", autouse=True)
def _worst_ratio_table(request):
    """after the last test of this module: the worst |err| / bound of every kernel output checked, one line each (shown without -s)"""
    WORST.clear()
    yield
    if not WORST:
        return
    lines = ["", "worst |err| / bound per kernel output:"] + [f"  {k:44s} {WORST[k]:.3f}" for k in sorted(WORST)]
    capman = request.config.pluginmanager.getplugin("capturemanager")
    with capman.global_and_fixture_disabled():
        print("\n".join(lines))


def _L():
    from cddmsl_amd import hip
    return hip._L()


def _stream():
    from cddmsl_amd import hip
    return hip.stream_ptr()


def _ptr(t, off=0):
    return ctypes.c_void_p(t.data_ptr() + off * t.element_size())


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def _randn(shape, seed, s=1.0, dtype=torch.bfloat16):
    return (torch.randn(shape, device=DEV, generator=_gen(seed)) * s).to(dtype)


def _nan(shape, dtype=torch.bfloat16):
    return torch.full(shape, float("nan"), device=DEV, dtype=dtype)


def _judge(kernel, case, got, exact, bound, bias=None):
    """``kernel``: the kernel output the check belongs to (the key of the worst-ratio table), ``case``: the shape / data"""
    ok, r, w = A.check(got, exact, bound)
    WORST[kernel] = max(WORST.get(kernel, 0.0), r)
    msg = f"{kernel} [{case}]: worst |err|/bound {r:.3g}"
    if bias is not None:
        rb, n = A.store_bias(got, *bias)
        msg += f", store bias {rb:+.4f} over {n}"
        if n >= 20000:
            assert abs(rb) <= 0.02, msg
    print(msg)
    g, e = A._f64(got).reshape(-1)[w], A._f64(exact).reshape(-1)[w]
    assert ok, f"{msg}; element {w}: got {float(g)!r}, exact {float(e)!r}"


def _untouched(buf, view_mask):
    """every element outside the view still holds the NaN it was filled with (bit pattern), every element inside is a number"""
    assert bool(torch.isfinite(buf[view_mask].float()).all()), "an element of the output view was not written"
    out = buf[~view_mask]
    assert bool(torch.isnan(out.float()).all()), "an element outside the output view was written"


# ================================================================================================== attn_small
def _small_launch(q, k, v, o, n, t, heads, scale, cols=(0, 0, 0, 0)):
    """the C-ABI with q / k / v / o as 2-D row buffers [>= n*t, ld] (heads at column cols[i] + h*96)"""
    e = _L().cddmsl_attn_small_fwd(_ptr(q, cols[0]), _ptr(k, cols[1]), _ptr(v, cols[2]), _ptr(o, cols[3]), n, t, heads, 96,
                                   q.shape[1], k.shape[1], v.shape[1], o.shape[1], ctypes.c_float(scale), 0, _stream())
    assert e == 0


def _small_bwd_launch(q, k, v, do, dq, dk, dv, n, t, heads, scale, cols=(0,) * 7):
    e = _L().cddmsl_attn_small_bwd(_ptr(q, cols[0]), _ptr(k, cols[1]), _ptr(v, cols[2]), _ptr(do, cols[3]), _ptr(dq, cols[4]),
                                   _ptr(dk, cols[5]), _ptr(dv, cols[6]), n, t, heads, 96, q.shape[1], k.shape[1], v.shape[1],
                                   do.shape[1], ctypes.c_float(scale), 0, _stream())
    assert e == 0


def _check_small(tag, q, k, v, do, o, dq, dk, dv, n, t, heads, scale, chunk=64, bias=True):
    """q..dv: [n*t, heads*96] views; references per chunk of sequences"""
    for s0 in range(0, n, chunk):
        s1 = min(n, s0 + chunk)
        rr = slice(s0 * t, s1 * t)
        hf = lambda x: A.heads_first(x[rr], s1 - s0, t, heads, 96)
        Q, K_, V = hf(q), hf(k), hf(v)
        f = A.attn_fwd(Q, K_, V, scale)
        _judge("attn_small_fwd o", tag, hf(o), f["o"], f["bound"], (f["o_rw"], f["pre_rw"]) if bias else None)
        if do is None:
            continue
        b = A.attn_small_bwd(Q, K_, V, hf(do), scale)
        _judge("attn_small_bwd dq", tag, hf(dq), *b["dq"], b["dq_rw"] if bias else None)
        _judge("attn_small_bwd dk", tag, hf(dk), *b["dk"], b["dk_rw"] if bias else None)
        _judge("attn_small_bwd dv", tag, hf(dv), *b["dv"], b["dv_rw"] if bias else None)


@pytest.mark.parametrize("images", [16, 32])
@pytest.mark.parametrize("form", ["separate", "fused_qkv"])
def test_attn_small_bench_shapes(images, form):
    """the mapper's launch: n sequences of 80 tokens, 8 heads of 96; q | kv as separate tensors, and the fused qkv (row stride 3d)"""
    from cddmsl_amd import hip
    n, t, heads, d = MAPPER_N[images], 80, 8, 768
    qkv = _randn((n * t, 3 * d), 1 + images, 0.56)
    do = _randn((n * t, d), 2 + images, 0.5)
    if form == "fused_qkv":
        o = hip.attn_small_fwd_qkv(qkv, t, heads, MAPPER_SCALE)
        dqkv = hip.attn_small_bwd_qkv(qkv, do, t, heads, MAPPER_SCALE)
    else:
        q, kv = qkv[:, :d].contiguous(), qkv[:, d:].contiguous()
        o = hip.attn_small_fwd(q, kv, t, heads, MAPPER_SCALE)
        dq, dkv = hip.attn_small_bwd(q, kv, do, t, heads, MAPPER_SCALE)
        dqkv = torch.cat([dq, dkv], 1)
    _check_small(f"n={n}", qkv[:, :d], qkv[:, d:2 * d], qkv[:, 2 * d:], do, o, dqkv[:, :d], dqkv[:, d:2 * d], dqkv[:, 2 * d:], n, t, heads,
                 MAPPER_SCALE, chunk=128)


@pytest.mark.parametrize("heads", [1, 3, 8])
@pytest.mark.parametrize("t", [1, 2, 31, 32, 33, 64, 65, 80, 95, 96])
def test_attn_small_edges_write_set_determinism(t, heads):
    """every t of the 96-row tile's boundaries; strides wider than the data, outputs NaN-filled with two rows past the last
    sequence: every element of the view written, nothing outside it (not the padded keys' dK / dV rows, not the columns past the
    heads); a second launch bit-identical"""
    n = 3
    W = heads * 96
    ld = W + 40                                   # (a multiple of 8: 16-byte rows)
    R = n * t
    ins = [_randn((R + 2, ld), 10 * t + heads + i, 0.56) for i in range(3)]
    do = _randn((R + 2, ld), 7 * t + heads, 0.5)
    mask = torch.zeros(R + 2, ld, dtype=torch.bool, device=DEV)
    mask[:R, 8:8 + W] = True                      # (the view starts 8 columns in)
    cols = (8,) * 7
    o = _nan((R + 2, ld))
    _small_launch(*ins, o, n, t, heads, MAPPER_SCALE, cols[:4])
    dq, dk, dv = _nan((R + 2, ld)), _nan((R + 2, ld)), _nan((R + 2, ld))
    _small_bwd_launch(*ins, do, dq, dk, dv, n, t, heads, MAPPER_SCALE, cols)
    torch.cuda.synchronize()
    for b in (o, dq, dk, dv):
        _untouched(b, mask)
    v_ = lambda x: x[:R, 8:8 + W]
    _check_small(f"t={t} heads={heads}", v_(ins[0]), v_(ins[1]), v_(ins[2]), v_(do), v_(o), v_(dq), v_(dk), v_(dv), n, t, heads,
                 MAPPER_SCALE, bias=False)
    o2, dq2, dk2, dv2 = _nan((R + 2, ld)), _nan((R + 2, ld)), _nan((R + 2, ld)), _nan((R + 2, ld))
    _small_launch(*ins, o2, n, t, heads, MAPPER_SCALE, cols[:4])
    _small_bwd_launch(*ins, do, dq2, dk2, dv2, n, t, heads, MAPPER_SCALE, cols)
    for a, b in ((o, o2), (dq, dq2), (dk, dk2), (dv, dv2)):
        assert torch.equal(a[mask], b[mask])


def test_attn_small_fused_backward_fills_dq_dk_dv():
    from cddmsl_amd import hip
    n, t, heads, d = 5, 80, 8, 768
    qkv = _randn((n * t, 3 * d), 31, 0.56)
    do = _randn((n * t, d), 32, 0.5)
    dqkv = _nan((n * t + 2, 3 * d))
    base, gbase = qkv.data_ptr(), dqkv.data_ptr()
    e = _L().cddmsl_attn_small_bwd(ctypes.c_void_p(base), ctypes.c_void_p(base + 2 * d), ctypes.c_void_p(base + 4 * d), _ptr(do),
                                   ctypes.c_void_p(gbase), ctypes.c_void_p(gbase + 2 * d), ctypes.c_void_p(gbase + 4 * d), n, t, heads, 96,
                                   3 * d, 3 * d, 3 * d, d, ctypes.c_float(MAPPER_SCALE), 0, _stream())
    assert e == 0
    torch.cuda.synchronize()
    mask = torch.zeros_like(dqkv, dtype=torch.bool)
    mask[:n * t] = True
    _untouched(dqkv, mask)
    assert torch.equal(dqkv[:n * t], hip.attn_small_bwd_qkv(qkv, do, t, heads, MAPPER_SCALE))


def _structured(n, t, heads, dh, sign=True):
    """q_i = e_0, k_j = j/4 e_0 (scores grow with j); v_j: key index + 1 in the first 32 channels, channel + head / 2 in the rest;
    the second sequence negated"""
    q = torch.zeros(n, t, heads, dh)
    k = torch.zeros(n, t, heads, dh)
    v = torch.zeros(n, t, heads, dh)
    j = torch.arange(t, dtype=torch.float32)
    q[..., 0] = 1.0
    k[..., 0] = (0.25 * j).view(1, t, 1)
    v[..., :32] = (j + 1).view(1, t, 1, 1)
    v[..., 32:] = torch.arange(dh - 32, dtype=torch.float32) + torch.arange(heads).view(heads, 1) * 0.5
    if sign and n > 1:
        v[1] *= -1
    f = lambda x: x.reshape(n * t, heads * dh).to(DEV).bfloat16()
    return f(q), f(k), f(v)


@pytest.mark.parametrize("regime", ["peaked", "equal", "structured"])
def test_attn_small_data_regimes(regime):
    """peaked: a score spread >= 40 (one key takes the weight, the rest underflow toward 0); equal scores (p = 1/t); structured
    operands where a transposed fragment, a shifted row or a wrong head offset moves the output by whole units"""
    n, t, heads = 4, 80, 8
    W = heads * 96
    if regime == "structured":
        q, k, v = _structured(n, t, heads, 96)
    else:
        q, k, v = (_randn((n * t, W), 40 + i, 4.0 if regime == "peaked" else 0.56) for i in range(3))
        if regime == "equal":
            k = k.view(n, t, W)[:, :1].expand(n, t, W).reshape(n * t, W).contiguous()
    do = _randn((n * t, W), 45, 0.5)
    o, dq, dk, dv = (_nan((n * t, W)) for _ in range(4))
    _small_launch(q, k, v, o, n, t, heads, MAPPER_SCALE)
    _small_bwd_launch(q, k, v, do, dq, dk, dv, n, t, heads, MAPPER_SCALE)
    if regime == "peaked":
        s = MAPPER_SCALE * (A.heads_first(q, n, t, heads, 96) @ A.heads_first(k, n, t, heads, 96).transpose(1, 2))
        assert float((s.amax(-1) - s.amin(-1)).min()) >= 40.0
    _check_small(regime, q, k, v, do, o, dq, dk, dv, n, t, heads, MAPPER_SCALE, bias=False)


def test_attn_small_sequences_are_independent():
    n, t, heads = 4, 80, 8
    W = heads * 96
    ins = [_randn((n * t, W), 50 + i, 0.56) for i in range(4)]
    outs = []
    for rep in range(2):
        if rep:
            for x in ins:
                x[t:2 * t] = _randn((t, W), 60, 2.0)          # sequence 1 only
        o, dq, dk, dv = (_nan((n * t, W)) for _ in range(4))
        _small_launch(*ins[:3], o, n, t, heads, MAPPER_SCALE)
        _small_bwd_launch(*ins, dq, dk, dv, n, t, heads, MAPPER_SCALE)
        outs.append(torch.cat([o, dq, dk, dv], 1))
    keep = torch.ones(n * t, dtype=torch.bool, device=DEV)
    keep[t:2 * t] = False
    assert torch.equal(outs[0][keep], outs[1][keep])
    assert not torch.equal(outs[0][~keep], outs[1][~keep])


# ================================================================================================== attn_last
def _last_inputs(n, t, heads, dh, seed, regime="gauss"):
    """q [n, ldq], kv [n*t + 1, ldkv] (K at column h*dh, V at voff + h*dh), do [n, ldo]: every stride wider than the data.
    regime: gauss (the mapper's magnitudes), peaked (score spread >= 40), equal (every key of a sequence the same: p = 1/t),
    structured (_structured's last query row)"""
    d = heads * dh
    ldq, ldkv, ldo = d + 8, 2 * d + 16, d + 24
    voff = d + 8
    s = 7.3 if regime == "peaked" else 1.0          # (peaked: q, k of standard deviation 4, as attn_small's peaked case)
    q = _randn((n, ldq), seed, 0.55 * s)
    kv = _randn((n * t + 1, ldkv), seed + 1, 0.56 * s)
    if regime == "equal":
        kv[:n * t, :d] = kv[:n * t, :d].reshape(n, t, d)[:, :1].expand(n, t, d).reshape(n * t, d)
    if regime == "structured":
        sq, sk, sv = _structured(n, t, heads, dh)
        q[:, :d] = sq.view(n, t, d)[:, -1]
        kv[:n * t, :d], kv[:n * t, voff:voff + d] = sk, sv
    do = _randn((n, ldo), seed + 2, 0.5)
    return dict(q=q, kv=kv, do=do, d=d, voff=voff)


def _last_case(n, t, heads, dh, seed, scale, regime="gauss"):
    return _last_run(_last_inputs(n, t, heads, dh, seed, regime), n, t, heads, dh, scale)


def _last_run(inp, n, t, heads, dh, scale):
    """both launches on NaN-filled outputs with a row (and for p a few elements) past the view"""
    q, kv, do, d, voff = inp["q"], inp["kv"], inp["do"], inp["d"], inp["voff"]
    ldq, ldkv, ldo = q.shape[1], kv.shape[1], do.shape[1]
    o, dq = _nan((n + 1, ldo)), _nan((n + 1, ldq))
    p = _nan((n * heads * t + 5,), torch.float32)
    dkv = _nan((n * t + 1, ldkv))
    e = _L().cddmsl_attn_last_fwd(_ptr(q), _ptr(kv), _ptr(o), _ptr(p), n, t, heads, dh, ldq, ldkv, voff, ldo, ctypes.c_float(scale), 0, _stream())
    assert e == 0
    e = _L().cddmsl_attn_last_bwd(_ptr(q), _ptr(kv), _ptr(do), _ptr(p), _ptr(dq), _ptr(dkv), n, t, heads, dh, ldq, ldkv, voff, ldo,
                                  ctypes.c_float(scale), 0, _stream())
    assert e == 0
    torch.cuda.synchronize()
    return dict(q=q, kv=kv, do=do, o=o, dq=dq, p=p, dkv=dkv, d=d, voff=voff)


def _check_last(tag, c, n, t, heads, dh, scale):
    d, voff = c["d"], c["voff"]
    mo = torch.zeros_like(c["o"], dtype=torch.bool)
    mo[:n, :d] = True
    _untouched(c["o"], mo)
    mq = torch.zeros_like(c["dq"], dtype=torch.bool)
    mq[:n, :d] = True
    _untouched(c["dq"], mq)
    mp = torch.zeros_like(c["p"], dtype=torch.bool)
    mp[:n * heads * t] = True
    _untouched(c["p"], mp)
    mk = torch.zeros_like(c["dkv"], dtype=torch.bool)
    mk[:n * t, :d] = True
    mk[:n * t, voff:voff + d] = True
    _untouched(c["dkv"], mk)
    Q = c["q"][:, :d].reshape(n * heads, 1, dh)
    K_ = A.heads_first(c["kv"][:n * t], n, t, heads, dh)
    V = A.heads_first(c["kv"][:n * t], n, t, heads, dh, col0=voff)
    f = A.attn_fwd(Q, K_, V, scale, depth=A.NORM_DEPTH_WAVE, p_bf16=False)
    p = c["p"][:n * heads * t].view(n * heads, t)
    _judge("attn_last_fwd p", tag, p, f["p"][:, 0], f["p_bound"][:, 0])
    _judge("attn_last_fwd o", tag, c["o"][:n, :d].reshape(n * heads, dh), f["o"][:, 0], f["bound"][:, 0], (f["o"][:, 0], f["pre"][:, 0]))
    b = A.attn_last_bwd(Q[:, 0], K_, V, c["do"][:, :d].reshape(n * heads, dh), p, scale)
    _judge("attn_last_bwd dq", tag, c["dq"][:n, :d].reshape(n * heads, dh), *b["dq"], (b["dq"][0], b["dq_pre"]))
    _judge("attn_last_bwd dk", tag, A.heads_first(c["dkv"][:n * t], n, t, heads, dh), *b["dk"], (b["dk"][0], b["dk_pre"]))
    dv = A.heads_first(c["dkv"][:n * t], n, t, heads, dh, col0=voff)
    assert torch.equal(dv, b["dv"]), "dV is not bf16(p * dO) of the kernel's own p"


@pytest.mark.parametrize("dh", [8, 64, 96, 128])
@pytest.mark.parametrize("t", [1, 63, 64, 65, 80, 127, 128])
def test_attn_last_edges_write_set_determinism(t, dh):
    n, heads = 5, 3
    scale = dh ** -0.5
    c = _last_case(n, t, heads, dh, 100 * t + dh, scale)
    _check_last(f"t={t} dh={dh}", c, n, t, heads, dh, scale)
    c2 = _last_case(n, t, heads, dh, 100 * t + dh, scale)
    for key in ("o", "dq", "p", "dkv"):
        assert torch.equal(c[key].nan_to_num(7.0), c2[key].nan_to_num(7.0)), key


@pytest.mark.parametrize("regime", ["bench16", "bench32", "structured", "peaked", "equal"])
def test_attn_last_bench_shapes_and_regimes(regime):
    """the mapper's last layer at both bench n; structured operands, a score spread >= 40, equal scores"""
    n = MAPPER_N[32] if regime == "bench32" else MAPPER_N[16] if regime == "bench16" else 4
    c = _last_case(n, 80, 8, 96, 7, MAPPER_SCALE, regime if regime in ("structured", "peaked", "equal") else "gauss")
    if regime == "peaked":
        Q = c["q"][:, :768].reshape(n * 8, 1, 96).double()
        s = MAPPER_SCALE * (Q @ A.heads_first(c["kv"][:n * 80], n, 80, 8, 96).transpose(1, 2))
        assert float((s.amax(-1) - s.amin(-1)).min()) >= 40.0
    _check_last(regime, c, n, 80, 8, 96, MAPPER_SCALE)


def test_attn_last_sequences_are_independent():
    """new q, K, V and dO for sequence 1 leave every output of the other sequences bit-identical"""
    n, t, heads, dh = 4, 80, 8, 96
    inp = _last_inputs(n, t, heads, dh, 90)
    a = _last_run(inp, n, t, heads, dh, MAPPER_SCALE)
    inp["q"][1] = _randn(inp["q"].shape[1:], 91, 2.0)
    inp["kv"][t:2 * t] = _randn((t, inp["kv"].shape[1]), 92, 2.0)
    inp["do"][1] = _randn(inp["do"].shape[1:], 93, 2.0)
    b = _last_run(inp, n, t, heads, dh, MAPPER_SCALE)
    seq = torch.ones(n, dtype=torch.bool, device=DEV)
    seq[1] = False
    rows = seq.repeat_interleave(t)
    for key, m in (("o", seq), ("dq", seq), ("p", seq.repeat_interleave(heads * t)), ("dkv", rows)):
        x, y = a[key][:m.numel()], b[key][:m.numel()]
        assert torch.equal(x[m].nan_to_num(7.0), y[m].nan_to_num(7.0)), key
        assert not torch.equal(x[~m].nan_to_num(7.0), y[~m].nan_to_num(7.0)), key


# ================================================================================================== attention-pool glue
def _tokens(x, pos, TP):
    K, P, C = x.shape
    tok = _nan((K + 1, TP, C))
    mbits = torch.full((K + 1, C), 0x5A5A, device=DEV, dtype=torch.int64)
    e = _L().cddmsl_attn_tokens_fwd_mask(_ptr(x), _ptr(pos), _ptr(tok), _ptr(mbits), K, P, TP, C, 0, _stream())
    assert e == 0
    torch.cuda.synchronize()
    return tok, mbits


@pytest.mark.parametrize("K", POOL_K[16])
def test_attn_tokens_fwd(K):
    """rows 1..P bit-exact, row 0 (the mean) within its bound, the pad rows written with zeros, mbits bit-exact, nothing past K"""
    P, TP, C = 49, 56, 2048
    x = _randn((K, P, C), K, 0.86)
    pos = _randn((P + 1, C), 3, 0.022, torch.float32)
    tok, mbits = _tokens(x, pos, TP)
    assert bool(torch.isnan(tok[K].float()).all()) and bool((mbits[K] == 0x5A5A).all())
    ref = A.tokens_fwd(x, pos, TP)
    assert torch.equal(tok[:K, 1:P + 1], ref["rows"])
    assert bool((tok[:K, P + 1:] == 0).all()) and not bool(torch.signbit(tok[:K, P + 1:].float()).any())
    assert torch.equal(mbits[:K], ref["mbits"])
    _judge("attn_tokens_fwd row 0", f"K={K}", tok[:K, 0], ref["row0"], ref["row0_bound"], (ref["row0"], ref["row0_pre"]))
    x2 = x.clone()
    x2[K // 2] = _randn((P, C), 9, 2.0)
    tok2, mbits2 = _tokens(x2, pos, TP)
    keep = torch.ones(K, dtype=torch.bool, device=DEV)
    keep[K // 2] = False
    assert torch.equal(tok[:K][keep], tok2[:K][keep]) and torch.equal(mbits[:K][keep], mbits2[:K][keep])
    tok3, _ = _tokens(x, pos, TP)
    assert torch.equal(tok[:K], tok3[:K])


def _softmax_launch(S, P1, scale):
    K, H, TP = S.shape
    p = _nan((K * H * P1 + 3,), torch.float32)
    pT = _nan((K * TP * H + 3,))
    assert _L().cddmsl_attnpool_softmax_fwd(_ptr(S), _ptr(p), _ptr(pT), K, H, P1, TP, ctypes.c_float(scale), 0, _stream()) == 0
    return p, pT


def _softmax_bwd_launch(p, dP, P1, scale):
    K, H, TP = dP.shape
    dsT = _nan((K * TP * H + 3,))
    pds = _nan((K * 2 * H * TP + 3,))
    assert _L().cddmsl_attnpool_softmax_bwd(_ptr(p), _ptr(dP), _ptr(dsT), _ptr(pds), K, H, P1, TP, ctypes.c_float(scale), 0, _stream()) == 0
    return dsT, pds


@pytest.mark.parametrize("regime", ["gauss", "peaked", "equal"])
@pytest.mark.parametrize("H", [8, 12, 20, 32, 40, 64])
def test_attnpool_softmax_fwd_bwd(H, regime):
    """both kernel forms (one wave per region for H <= 32 -- its 16-byte transposed stores for H % 8 == 0, one element at a time
    for H = 12, 20; one thread per row for H = 40, 64): p within its f32 bound, pT = bf16(p) bit for bit with zero rows past P1;
    ds within its bound (the cancellation term), pds = [bf16(p) ; ds], dsT = ds transposed, zero columns past P1; nothing
    written past the outputs; a second launch bit-identical; new scores and dP for one region leave every other region's
    outputs bit-identical"""
    K, P1, TP, scale = 544 if H == 32 else 300, 50, 56, 0.125
    form = "wave" if H <= 32 else "thread per row"
    S = _randn((K, H, TP), H, 8.2 * (40.0 if regime == "peaked" else 1.0), torch.float32)
    if regime == "equal":
        S[:] = 3.0
    p, pT = _softmax_launch(S, P1, scale)
    dP = _randn((K, H, TP), H + 1, 1e-3, torch.float32)
    pv = p[:K * H * P1].view(K, H, P1)
    dsT, pds = _softmax_bwd_launch(pv, dP, P1, scale)
    torch.cuda.synchronize()
    for b, nel in ((p, K * H * P1), (pT, K * TP * H), (dsT, K * TP * H), (pds, K * 2 * H * TP)):
        assert bool(torch.isfinite(b[:nel].float()).all()) and bool(torch.isnan(b[nel:].float()).all())
    depth = A.softmax_depth(H, TP, P1)
    pe, pb = A.softmax_fwd(S.view(K * H, TP), P1, scale, depth)
    _judge("attnpool_softmax_fwd p (" + form + ")", f"H={H} {regime}", pv.reshape(K * H, P1), pe, pb)
    if regime == "peaked":
        sc_ = S[..., :P1].double() * scale
        assert float((sc_.amax(-1) - sc_.amin(-1)).min()) >= 40.0
    pTv = pT[:K * TP * H].view(K, TP, H)
    assert torch.equal(pTv[:, :P1], pv.transpose(1, 2).bfloat16()) and bool((pTv[:, P1:] == 0).all())
    dse, dsb, dspre = A.softmax_bwd(pv.reshape(K * H, P1), dP.view(K * H, TP), scale, depth)
    pdsv = pds[:K * 2 * H * TP].view(K, 2 * H, TP)
    _judge("attnpool_softmax_bwd ds (" + form + ")", f"H={H} {regime}", pdsv[:, H:, :P1].reshape(K * H, P1), dse, dsb, (dse, dspre))
    assert torch.equal(pdsv[:, :H, :P1], pv.bfloat16()) and bool((pdsv[:, :, P1:] == 0).all())
    dsTv = dsT[:K * TP * H].view(K, TP, H)
    assert torch.equal(dsTv[:, :P1], pdsv[:, H:, :P1].transpose(1, 2)) and bool((dsTv[:, P1:] == 0).all())
    p2, pT2 = _softmax_launch(S, P1, scale)
    dsT2, pds2 = _softmax_bwd_launch(pv, dP, P1, scale)
    for a, b in ((p, p2), (pT, pT2), (dsT, dsT2), (pds, pds2)):
        assert torch.equal(a.nan_to_num(7.0), b.nan_to_num(7.0))
    k1 = K // 3
    S[k1] = _randn((H, TP), 99, 8.2, torch.float32)
    dP[k1] = _randn((H, TP), 98, 1e-3, torch.float32)
    p3, pT3 = _softmax_launch(S, P1, scale)
    dsT3, pds3 = _softmax_bwd_launch(p3[:K * H * P1].view(K, H, P1), dP, P1, scale)
    keep = torch.ones(K, dtype=torch.bool, device=DEV)
    keep[k1] = False
    for a, b, per in ((p, p3, H * P1), (pT, pT3, TP * H), (dsT, dsT3, TP * H), (pds, pds3, 2 * H * TP)):
        x, y = a[:K * per].view(K, per), b[:K * per].view(K, per)
        assert torch.equal(x[keep], y[keep]) and not torch.equal(x[k1], y[k1])


# ================================================================================================== attnpool_dx
def _bpb(K, C=2048):
    kt = C // 128
    return min(K, max(8, (kt * K + 4095) // 4096))


def _dx_inputs(K, seed, H=32, P=49, TP=56, C=2048):
    g = _gen(seed)
    S = torch.randn(K, H, P + 1, device=DEV, generator=g) * 8.2 * 0.125
    pds = torch.zeros(K, 2 * H, TP, device=DEV, dtype=torch.bfloat16)
    pds[:, :H, :P + 1] = torch.softmax(S, -1).bfloat16()
    pds[:, H:, :P + 1] = (torch.randn(K, H, P + 1, device=DEV, generator=g) * 1e-3).bfloat16()
    zu = torch.empty(K, 2 * H, C, device=DEV, dtype=torch.bfloat16)
    for c0 in range(0, K, 1024):
        c1 = min(K, c0 + 1024)
        zu[c0:c1, :H] = (torch.randn(c1 - c0, H, C, device=DEV, generator=g) * 0.05).bfloat16()
        zu[c0:c1, H:] = (torch.randn(c1 - c0, H, C, device=DEV, generator=g) * 0.19).bfloat16()
    g0 = torch.randn(K, C, device=DEV, generator=g) * 0.01
    mbits = torch.randint(-2 ** 62, 2 ** 62, (K, C), device=DEV, generator=g)
    return pds, zu, g0, mbits


def _dx_launch(pds, zu, g0, mbits, gpos, P=49):
    K, H2, TP = pds.shape
    C = zu.shape[2]
    dx = _nan((K + 1, P, C))
    assert _L().cddmsl_attnpool_dx(_ptr(pds), _ptr(zu), _ptr(g0), _ptr(mbits), _ptr(dx), _ptr(gpos), K, H2, P, TP, C, 0, _stream()) == 0
    torch.cuda.synchronize()
    return dx


@pytest.mark.parametrize("K", [300, 544, 8192, 8100, 8161])
def test_attnpool_dx(K):
    """K = 300 (8-region runs and a tail), the bench's 544 (8-region runs) and 8192 (32-region runs, no tail), 8100 (32-region runs
    and a 4-region tail), 8161 (a 1-region tail: the kernel's last-item path alone).  Sampled regions: two per run, the first
    and last region, every region of the last run.  dx within its bound, masked elements exactly 0, nothing past K; gpos over
    all regions within its bound; another region's inputs leave this one's dx bit-identical; two launches give the same dx"""
    P, C = 49, 2048
    pds, zu, g0, mbits = _dx_inputs(K, K)
    gpos = torch.full((P + 1, C), 0.25, device=DEV)
    dx = _dx_launch(pds, zu, g0, mbits, gpos)
    assert bool(torch.isnan(dx[K].float()).all()) and bool(torch.isfinite(dx[:K].float()).all())
    bpb = _bpb(K)
    blocks = (K + bpb - 1) // bpb
    rows = torch.unique(torch.cat([X.sample_rows(K, tile=bpb, per_tile=2), torch.arange((blocks - 1) * bpb, K)])).to(DEV)
    dxe, dxb, keep, pre = A.attnpool_dx(pds[rows], zu[rows], g0[rows], mbits[rows], P)
    got = dx[rows]
    assert bool((got[~keep] == 0).all()) and not bool(torch.signbit(got[~keep].float()).any())
    _judge("attnpool_dx dx", f"K={K}, runs of {bpb}, tail {K - (blocks - 1) * bpb}", got, dxe, dxb, (dxe, pre))
    ge, gb = A.attnpool_gpos(pds, zu, g0, torch.full((P + 1, C), 0.25, device=DEV), P, bpb, blocks)
    _judge("attnpool_dx gpos", f"K={K}", gpos, ge, gb)
    dx2 = _dx_launch(pds, zu, g0, mbits, torch.zeros(P + 1, C, device=DEV))
    assert torch.equal(dx[:K], dx2[:K])
    k1 = K - 1 if K % bpb == 1 else K // 2
    zu[k1] = (torch.randn(zu.shape[1:], device=DEV, generator=_gen(5)) * 3).bfloat16()
    g0[k1] += 1.0
    dx3 = _dx_launch(pds, zu, g0, mbits, torch.zeros(P + 1, C, device=DEV))
    keepk = torch.ones(K, dtype=torch.bool, device=DEV)
    keepk[k1] = False
    assert torch.equal(dx[:K][keepk], dx3[:K][keepk]) and not torch.equal(dx[k1], dx3[k1])


# ================================================================================================== the whole pool
@pytest.mark.parametrize("K", POOL_K[16])
def test_attention_pool_stages_at_bench_K(K):
    """layers.AttnPoolFn's forward at the bench's region count: every saved intermediate (tok, q0, U, p, z, o) and the output,
    each against float64 of the intermediates the pool itself computed before it -- the offsets and strides of the batched
    products at K regions, not only the kernels.  Sampled regions (first, last, one per 32)."""
    from cddmsl_amd import layers
    C, H, P, TP, D = 2048, 32, 49, 56, 64
    gw = lambda o, i, s, seed: (torch.randn(o, i, device=DEV, generator=_gen(seed)) * s).requires_grad_(True)
    pos = (torch.randn(P + 1, C, device=DEV, generator=_gen(70)) * 0.022).requires_grad_(True)
    ws = [gw(C, C, C ** -0.5, 71 + i) for i in range(3)] + [gw(1024, C, C ** -0.5, 74)]
    bs = [(torch.randn(m, device=DEV, generator=_gen(75 + i)) * 0.1).requires_grad_(True) for i, m in enumerate((C, C, C, 1024))]
    ap = layers.AttnPoolParams(pos, ws[0], bs[0], ws[1], bs[1], ws[2], bs[2], ws[3], bs[3], H)
    x = torch.relu(_randn((K, 7, 7, C), 80, 1.4, torch.float32)).bfloat16().requires_grad_(True)
    out = layers.AttnPoolFn.apply(x, ws[0], ap, True)
    tok, q0, zu, p, z, o = out.grad_fn.saved_tensors[:6]
    T = torch.bfloat16
    wq = ap.pq.get(T, False)[0].reshape(C, C)
    wkT = ap.pk.get(T, True)[1].reshape(C, C)
    wv = ap.pv.get(T, True)[0].reshape(C, C)
    wc = ap.pc.get(T, False)[0].reshape(1024, C)
    rows = X.sample_rows(K, tile=32, per_tile=1).to(DEV)
    f = A._f64
    # tok
    ref = A.tokens_fwd(x.detach().view(K, P, C)[rows], pos.detach(), TP)
    assert torch.equal(tok[rows, 1:P + 1], ref["rows"]) and bool((tok[rows, P + 1:] == 0).all())
    _judge("AttnPoolFn tok row 0", f"K={K}", tok[rows, 0], ref["row0"], ref["row0_bound"])
    # q0 = tok[:, 0] Wq^T + bq
    t0 = tok[rows, 0]
    e, ab = X.gemm_exact(t0.unsqueeze(0), wq.unsqueeze(0))
    e = e[0] + f(bs[0].detach())
    _judge("AttnPoolFn q0", f"K={K}", q0[rows], e, X.bound(e, ab[0], T, bias=bs[0].detach()))
    # U[k, h, :] = q0[k, hD:(h+1)D] Wk[hD:(h+1)D, :]
    q0h = f(q0[rows]).view(-1, H, D)
    wkh = f(wkT).view(C, H, D)
    Ue = torch.einsum("khd,nhd->khn", q0h, wkh)
    Ua = torch.einsum("khd,nhd->khn", q0h.abs(), wkh.abs())
    U = zu[rows, H:]
    _judge("AttnPoolFn U", f"K={K}", U, Ue, X.bound(Ue, Ua, T))
    # p = softmax(U tok^T * D^-0.5) over the P + 1 tokens (S in f32: its accumulation error enters as a score shift)
    tk = f(tok[rows, :P + 1])
    Se = f(U) @ tk.transpose(1, 2)
    eps = C_ACC_U * (f(U).abs() @ tk.abs().transpose(1, 2))
    pe, pb = A.softmax_fwd(Se.reshape(-1, P + 1), P + 1, D ** -0.5, A.NORM_DEPTH_WAVE)
    pb = pb + 2.02 * D ** -0.5 * eps.reshape(-1, P + 1).amax(-1, keepdim=True) * pe
    _judge("AttnPoolFn p", f"K={K}", p[rows].reshape(-1, P + 1), pe, pb)
    # z = bf16(p) tok
    ze, za = X.gemm_exact(p[rows].bfloat16().transpose(1, 2), tok[rows, :P + 1], transpose_a=True)
    _judge("AttnPoolFn z", f"K={K}", z[rows], ze, X.bound(ze, za, T))
    # o = bf16(bf16(z Wv^T per head) + bv)
    wvh = f(wv).view(H, D, C)
    oe = torch.einsum("khc,hnc->khn", f(z[rows]), wvh).reshape(-1, C)
    oa = torch.einsum("khc,hnc->khn", f(z[rows]).abs(), wvh.abs()).reshape(-1, C)
    vb = f(bs[2].detach().to(T))
    ob = X.U_BF16 * (oe + vb).abs() + (1 + X.U_BF16) * X.bound(oe, oa, T)
    _judge("AttnPoolFn o", f"K={K}", o[rows], oe + vb, ob)
    # out = o Wc^T + bc (f32)
    e, ab = X.gemm_exact(o[rows].unsqueeze(0), wc.unsqueeze(0))
    e = e[0] + f(bs[3].detach())
    _judge("AttnPoolFn out", f"K={K}", out.detach()[rows], e, X.bound(e, ab[0], torch.float32, bias=bs[3].detach()))

