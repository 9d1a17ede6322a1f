"""The CLIP text tower's kernels (cddmsl_amd/csrc/text_encoder.hip) and the GPT-2 decoder's (csrc/gpt2.hip) at their tile, tail and
dispatch edges, against the float64 references and bounds of tests/exact_text.py at the case tables of tests/text_exact_cases.py
(tests/test_text_bound_host.py runs f32 emulations and mutants against the same references, and proves the tables complete).

  attn_causal_fwd   through the C-ABI inside NaN-filled buffers: 128 NaN rows before and after qkv (rows >= t of the last sequence
                    belong to somebody else), NaN in the pitch gaps (ldqkv = 3 W + 8, ldo = W + 8), NaN rows around o that must come
                    back untouched (spare waves store nothing); every t class, nseq * heads mod 4 = 1, 2, 3, two scales, a dominant
                    key with logits up to 4096, row 0 of every sequence equal to v_0, the refusals
  text_pool         W / 64 = 1, 10, 16; one and two blocks; group 1, 3, 8; repeated and extreme indices; the constant row (exactly
                    beta), the row of mean 1e3; bf16 = the rounding of the f32 output; the refusals
  quick_gelu, gelu_new   one chunk and a partial second block, the table of special operands, the refusals
  text_embed, pos_embed  ids 0 and vocab - 1, t = the table's rows, pos0 + t = npos and npos + 1, ld_ids 1 and 9, both dtypes, W = 8
  skinny_gemm       tier A (integers: bit-exact) and tier B (Gaussian: the existing bound) at every chunks-per-split class, M = 1, 32,
                    33, 64, three epilogues, a partial last tile; rows independent of M bit for bit
  lm_head_argmax / lm_head_topk   V = 5, 32, 33: integer logits with planted ties, exact ids / indices, logZ under the bound
  decode_attn[_beam]    heads 1 and 3, the L edges of both Lmax, ldqkv = 3 W + 8, NaN in every cache row the step must not read,
                    a dominant key (output = that value row)
The module's last test prints the worst err / bound per kernel output.

Measured on one MI355X (114 tests in 4 s), worst |err| / bound over all cases:
  attn_causal random 0.629, spare waves 0.548, dominant key 0.000     decode_attn 0.801, decode_attn_beam 0.852
  text_pool f32 0.109, bf16 0.997                                     lm_head_topk logZ 0.007
  quick_gelu f32 0.245 (specials 0.154), gelu_new f32 0.184 (0.074)   both bf16 1.000
  skinny_gemm tier B epi 0 0.968, epi 1 0.010, epi 2 0.959            tier A epi 2 (gelu_new of the exact sum) 1.000
(0.96 .. 1.000 on a bf16 output is a correctly rounded store half an ulp off; tier B epi 1's bound is the (K + S + 4) u sum |x||w|
worst case of a sum whose errors mostly cancel.)  With tile_dot's leftover chunk dropped after a pass of the paired loop, the
skinny_gemm tests of tests/test_gpu_caption.py still pass (their shapes give at most one pass and no leftover after it) and the 9,
13 and 17 chunk classes here fail in both tiers."""
import ctypes
import functools

import pytest
import torch

import exact_text as E
import text_exact_cases as C

pytestmark = pytest.mark.gpu
DEV = "cuda"
ERR_ARG = 1
WORST = {}
CANARY = {torch.bfloat16: (torch.int16, 0x7FC1), torch.float32: (torch.int32, 0x7FC00001)}


def _hip():
    from cddmsl_amd import hip
    return hip


def _p(t, byte_offset=0):
    return ctypes.c_void_p((t.data_ptr() if t is not None else 0) + byte_offset)


def _rec(key, r):
    WORST[key] = max(WORST.get(key, 0.0), float(r))
    assert r <= 1.0, (key, r)


def _nan(shape, dtype):
    it, bits = CANARY[dtype]
    return torch.full(shape, bits, dtype=it, device=DEV).view(dtype)


def _bits(t):
    return t.contiguous().view(CANARY[t.dtype][0])


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


# ------------------------------------------------------------------------------------------------ causal attention
MARGIN_ROWS = 128


def _attn_call(qkv, n, t, heads, scale, pad, over=None, q_off=0, o_off=0):
    """run cddmsl_attn_causal_fwd on qkv [n*t, 3 W] (CPU bf16) placed in the middle of NaN; -> (rc, o [n*t, W] on the CPU, ok) where
    ok says that every element outside o's data is untouched"""
    hip = _hip()
    R, W = n * t, heads * 64
    ldq, ldo = 3 * W + pad, W + pad
    qb = _nan((MARGIN_ROWS + R + MARGIN_ROWS, ldq), torch.bfloat16)
    qb[MARGIN_ROWS:MARGIN_ROWS + R, :3 * W] = qkv.to(DEV)
    ob = _nan((4 + R + 4, ldo), torch.bfloat16)
    before = ob.clone()
    a = dict(t=t, dh=64, ldqkv=ldq, ldo=ldo)
    a.update(over or {})
    rc = hip._L().cddmsl_attn_causal_fwd(_p(qb[MARGIN_ROWS:], q_off), _p(ob[4:], o_off), n, a["t"], heads, a["dh"], a["ldqkv"], a["ldo"],
                                         float(scale), 0, hip.stream_ptr())
    torch.cuda.synchronize()
    after = ob.clone()
    after[4:4 + R, :W] = before[4:4 + R, :W]
    return rc, ob[4:4 + R, :W].contiguous().cpu(), _same_bits(after, before)


def _attn_check(key, qkv, n, t, heads, scale, pad):
    rc, got, clean = _attn_call(qkv, n, t, heads, scale, pad)
    assert rc == 0 and clean, (key, rc, "an element outside the output was written")
    assert bool(torch.isfinite(got.float()).all())
    ref, v = E.attn_ref(qkv, n, t, heads, scale)
    _rec(f"attn_causal {key}", E.ratio((got.double() - ref).abs(), E.attn_bound(ref, v, n, t, heads)))
    W = heads * 64
    v0 = qkv.view(n, t, 3 * W)[:, 0, 2 * W:]
    assert torch.equal(got.view(n, t, W)[:, 0], v0), "row 0 has p = 1 exactly: the output is v_0"
    return got, ref, v


@pytest.mark.parametrize("t", C.ATTN_T)
def test_attn_causal_pitches_and_scales(t):
    n, heads = 2, 3
    qkv = E.attn_case(n, t, heads)
    outs = {}
    for scale in C.ATTN_SCALES:
        for pad in (0, C.ATTN_PITCH_PAD):
            outs[(scale, pad)] = _attn_check("random", qkv, n, t, heads, scale, pad)[0]
        assert _same_bits(outs[(scale, 0)], outs[(scale, C.ATTN_PITCH_PAD)])          # the pitch changes addresses only
    if t > 1:
        assert not torch.equal(outs[(C.ATTN_SCALES[0], 0)], outs[(C.ATTN_SCALES[1], 0)])
    assert _same_bits(outs[(0.125, 0)], _hip().attn_causal_fwd(qkv.to(DEV), t, heads, 0.125).cpu())


@pytest.mark.parametrize("heads,n", C.ATTN_WAVES)
def test_attn_causal_spare_waves_store_nothing(heads, n):
    for t in (5, 33):
        _attn_check("spare waves", E.attn_case(n, t, heads, seed=1), n, t, heads, 0.125, C.ATTN_PITCH_PAD)


@pytest.mark.parametrize("t", [2, 33, 128])
def test_attn_causal_dominant_key(t):
    n, heads = 2, 3
    qkv = E.attn_dominant_case(n, t, heads)
    got, ref, v = _attn_check("dominant key", qkv, n, t, heads, 0.125, C.ATTN_PITCH_PAD)
    vrow = qkv[:, 2 * heads * 64:]
    assert bool(((got.double() - vrow.double()).abs() <= E.attn_bound(ref, v, n, t, heads)).all())


def test_attn_causal_refusals_write_nothing():
    n, t, heads = 2, 33, 3
    qkv = E.attn_case(n, t, heads)
    W = heads * 64
    for kw in (dict(over=dict(t=129)), dict(over=dict(dh=32)), dict(over=dict(ldo=W + 4)), dict(over=dict(ldqkv=3 * W - 8)), dict(q_off=8),
               dict(o_off=8)):
        rc, got, clean = _attn_call(qkv, n, t, heads, 0.125, 0, **kw)
        assert rc == ERR_ARG and clean and bool(torch.isnan(got.float()).all()), kw


# ------------------------------------------------------------------------------------------------ text_pool
def _pool_call(x, rows, gamma, beta, nout, group, W, dtype, R=None):
    hip = _hip()
    y = _nan((nout + 4, W), dtype)
    before = y.clone()
    rc = hip._L().cddmsl_text_pool(_p(x), _p(rows), _p(gamma), _p(beta), _p(y), x.shape[0] if R is None else R, nout, group, W, 1e-5,
                                   hip.DT[dtype], hip.stream_ptr())
    torch.cuda.synchronize()
    return rc, y[:nout].cpu(), _same_bits(y[nout:], before[nout:]), _same_bits(y, before)


@pytest.mark.parametrize("group", C.POOL_GROUP)
@pytest.mark.parametrize("nout", C.POOL_NOUT)
@pytest.mark.parametrize("W", C.POOL_W)
def test_text_pool(W, nout, group):
    x, rows, gamma, beta = E.pool_case(W, nout, group)
    d = [v.to(DEV) for v in (x, rows, gamma, beta)]
    ref, bound = E.pool_ref(x, rows, gamma, beta, group)
    rc, y32, guard, _ = _pool_call(*d, nout, group, W, torch.float32)
    assert rc == 0 and guard
    _rec("text_pool f32", E.ratio((y32.double() - ref).abs(), bound))
    rc, y16, guard, _ = _pool_call(*d, nout, group, W, torch.bfloat16)
    assert rc == 0 and guard and _same_bits(y16, y32.bfloat16())
    refb, boundb = E.pool_ref(x, rows, gamma, beta, group, out_dtype=torch.bfloat16)
    _rec("text_pool bf16", E.ratio((y16.double() - refb).abs(), boundb))
    if nout > 1 and group == 1:
        assert int(rows[-1]) == 0 and _same_bits(y32[-1], beta)                        # the constant row: variance 0, exactly beta
    assert _same_bits(y32, _hip().text_pool(*d, group).cpu())


def test_text_pool_refusals_write_nothing():
    x, rows, gamma, beta = [v.to(DEV) for v in E.pool_case(1024, 5, 1)]
    big = torch.zeros(E.POOL_R, 1088, device=DEV)
    vec = torch.ones(1088, device=DEV)
    for args in ((big, rows, vec, vec, 5, 1, 1088), (big, rows, vec, vec, 5, 1, 96), (x, rows, gamma, beta, 5, 0, 1024)):
        rc, _, _, untouched = _pool_call(*args, torch.float32)
        assert rc == ERR_ARG and untouched, args[4:]


# ------------------------------------------------------------------------------------------------ activations
ACTS = {"quick_gelu": "cddmsl_quick_gelu", "gelu_new": "cddmsl_gelu_new"}
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16}


def _act_call(name, x, numel=None, byte_offset=0):
    """in place on a copy of x with 16 guard elements behind it; -> (rc, result, guard untouched)"""
    hip = _hip()
    n = x.numel()
    buf = torch.cat([x, torch.full((16,), 123.0, dtype=x.dtype)]).to(DEV)
    rc = getattr(hip._L(), ACTS[name])(_p(buf, byte_offset), n if numel is None else numel, hip.DT[x.dtype], hip.stream_ptr())
    torch.cuda.synchronize()
    out = buf.cpu()
    return rc, out[:n], bool((out[n:].float() == 123.0).all())


@pytest.mark.parametrize("dname", list(DTYPES))
@pytest.mark.parametrize("name", list(ACTS))
def test_activation_sizes_and_specials(name, dname):
    dt = DTYPES[dname]
    g = torch.Generator().manual_seed(11)
    for numel in C.ACT_NUMEL[dname]:
        x = (torch.randn(numel, generator=g) * 4).to(dt)
        rc, got, guard = _act_call(name, x)
        assert rc == 0 and guard
        _rec(f"{name} {dname}", E.act_check(got, x, name))
    x = E.specials(dt)
    rc, got, guard = _act_call(name, x)
    assert rc == 0 and guard
    _rec(f"{name} {dname} specials", E.act_check(got, x, name))
    x = torch.linspace(-12, 12, 4096).to(dt)                          # the cancellation range of 1 + tanh and of the sigmoid's tail
    rc, got, guard = _act_call(name, x)
    assert rc == 0 and guard
    _rec(f"{name} {dname}", E.act_check(got, x, name))
    wrapped = getattr(_hip(), name + "_")(x.to(DEV).clone()).cpu()
    assert _same_bits(torch.nan_to_num(wrapped.float()), torch.nan_to_num(got.float()))


@pytest.mark.parametrize("name", list(ACTS))
def test_activation_refusals_write_nothing(name):
    xb = torch.ones(24, dtype=torch.bfloat16)
    for kw in (dict(numel=12), dict(numel=16, byte_offset=8)):
        rc, got, guard = _act_call(name, xb, **kw)
        assert rc == ERR_ARG and guard and bool((got.float() == 1.0).all()), kw
    xf = torch.ones(12, dtype=torch.float32)
    for kw in (dict(numel=6), dict(numel=8, byte_offset=8), dict(numel=-4)):
        rc, got, guard = _act_call(name, xf, **kw)
        assert rc == ERR_ARG and guard and bool((got == 1.0).all()), kw


# ------------------------------------------------------------------------------------------------ embeddings
@pytest.mark.parametrize("W", C.EMBED_W)
@pytest.mark.parametrize("dname", list(DTYPES))
def test_text_embed_edges(dname, W):
    hip = _hip()
    g = torch.Generator().manual_seed(W)
    V, n, t = 37, 3, 7
    tok = torch.randn(V, W, generator=g).to(DTYPES[dname]).to(DEV)
    pos = torch.randn(t, W, generator=g).to(DEV)                       # t = the position table's row count
    ids = torch.randint(0, V, (n, t), generator=g)
    ids[0, 0], ids[1, 3], ids[2, t - 1] = 0, V - 1, V - 1
    ids = ids.to(DEV)
    got = hip.text_embed(ids, tok, pos)
    assert _same_bits(got, (tok.float()[ids] + pos[None]).view(n * t, W))


@pytest.mark.parametrize("ld", C.EMBED_LD_IDS)
@pytest.mark.parametrize("W", C.EMBED_W)
@pytest.mark.parametrize("dname", list(DTYPES))
def test_pos_embed_edges(dname, W, ld):
    hip = _hip()
    g = torch.Generator().manual_seed(W + ld)
    V, n, t, npos = 37, 3, 5, 11
    tab = torch.randn(V, W, generator=g).to(DTYPES[dname]).to(DEV)
    wpe = torch.randn(npos, W, generator=g).to(DEV)
    idm = torch.randint(0, V, (n * t, ld), generator=g)                # column 0 is read; the others hold other valid ids
    idm[0, 0], idm[n * t - 1, 0] = V - 1, 0
    idm = idm.to(DEV)
    src = torch.randn(n * t, W, generator=g).to(DEV)

    def call(pos0, ids, src_):
        x = _nan((n * t + 2, W), torch.float32)
        rc = hip._L().cddmsl_pos_embed(_p(ids), ld, _p(tab if ids is not None else None), _p(src_), _p(wpe), _p(x), n * t, t, pos0, W,
                                       V if ids is not None else 0, npos, hip.DT[tab.dtype] if ids is not None else 1, hip.stream_ptr())
        torch.cuda.synchronize()
        return rc, x

    r = torch.arange(n * t, device=DEV)
    for pos0 in (0, npos - t):                                        # pos0 + t == npos is accepted
        rc, x = call(pos0, idm, None)
        assert rc == 0 and _same_bits(x[:n * t], tab.float()[idm[:, 0]] + wpe[pos0 + r % t]) and bool(torch.isnan(x[n * t:]).all())
        rc, x = call(pos0, None, src)
        assert rc == 0 and _same_bits(x[:n * t], src + wpe[pos0 + r % t]) and bool(torch.isnan(x[n * t:]).all())
    for ids, src_ in ((idm, None), (None, src)):                       # pos0 + t == npos + 1 is refused
        rc, x = call(npos - t + 1, ids, src_)
        assert rc == ERR_ARG and bool(torch.isnan(x).all())
    if ld > 1:
        assert _same_bits(hip.pos_embed(wpe, npos - t, t, ids=idm[:, 0], tab=tab), tab.float()[idm[:, 0]] + wpe[npos - t + r % t])


# ------------------------------------------------------------------------------------------------ skinny GEMM
@functools.lru_cache(maxsize=2)
def _skinny_ops(N, K, tier):
    """operands of one (N, K) shape for M = 64 (smaller M take the first rows) and the float64 products: computed once per shape"""
    if tier == "A":
        x, w = E.small_ints((64, K), 3 * K + 1), E.small_ints((N, K), N + K)
        bias, res = E.small_ints((N,), 5, lim=8, zero_frac=0.2), E.small_ints((64, N), 6, lim=64, zero_frac=0.2)
    else:
        g = torch.Generator().manual_seed(N + 7 * K)
        x, w = torch.randn(64, K, generator=g), torch.randn(N, K, generator=g) * 0.05
        bias, res = torch.randn(N, generator=g), torch.randn(64, N, generator=g)
    x, w, bias, res = x.to(DEV).bfloat16(), w.to(DEV).bfloat16(), bias.to(DEV), res.to(DEV)
    S = C.skinny_splits(N, K)
    return dict(x=x, w=w, bias=bias, res=res, S=S, exact=x.double() @ w.double().t(), acc=E.skinny_bound(x, w, bias, S))


def _skinny_call(o, M, epi, bias=True, res=False):
    hip = _hip()
    N = o["w"].shape[0]
    dt = torch.float32 if epi == 1 else torch.bfloat16
    buf = _nan((M + 2, N), dt)
    y = hip.skinny_gemm(o["x"][:M].contiguous(), o["w"], o["bias"] if bias else None, residual=o["res"][:M].contiguous() if res else None,
                        epi=epi, out=buf[:M])
    torch.cuda.synchronize()
    assert y.data_ptr() == buf.data_ptr() and bool(torch.isnan(buf[M:].float()).all()), "rows past M were written"
    return buf[:M]


SK_IDS = [f"N{N}_K{K}" for (N, K), _, _ in C.SKINNY_SHAPES]


@pytest.mark.parametrize("shape", [s for s, _, _ in C.SKINNY_SHAPES], ids=SK_IDS)
def test_skinny_gemm_tier_a_bit_exact(shape):
    N, K = shape
    o = _skinny_ops(N, K, "A")
    assert _hip().skinny_gemm_workspace(64, N, K) == o["S"] * 64 * N * 4              # the host table's split is the library's
    pre = o["exact"] + o["bias"].double()
    assert float(pre.abs().max()) < 2 ** 24 and bool((pre == pre.round()).all())
    for M in C.SKINNY_M:
        assert torch.equal(_skinny_call(o, M, 1, res=True), (pre + o["res"].double())[:M].float()), (M, "epi 1")
        assert torch.equal(_skinny_call(o, M, 1, bias=False), o["exact"][:M].float()), (M, "epi 1, no bias")
        assert torch.equal(_skinny_call(o, M, 0), pre[:M].float().bfloat16()), (M, "epi 0")
        y2 = _skinny_call(o, M, 2)
        g = E.gelu_new_ref(pre[:M])                                    # the pre-activation is exact: only gelu_new and the store remain
        _rec("skinny_gemm tier A epi 2 (gelu_new)", E.ratio((y2.double() - g).abs(), E.act_bound(pre[:M], g, torch.bfloat16)))


@pytest.mark.parametrize("shape", [s for s, _, _ in C.SKINNY_SHAPES], ids=SK_IDS)
def test_skinny_gemm_tier_b_bound_and_row_independence(shape):
    N, K = shape
    o = _skinny_ops(N, K, "B")
    ref = o["exact"] + o["bias"].double()
    ref1 = ref + o["res"].double()
    g = E.gelu_new_ref(ref)
    acc, S = o["acc"], o["S"]
    full = {}
    for M in sorted(C.SKINNY_M, reverse=True):
        y0, y1, y2 = _skinny_call(o, M, 0), _skinny_call(o, M, 1, res=True), _skinny_call(o, M, 2)
        _rec("skinny_gemm tier B epi 0", E.ratio((y0.double() - ref[:M]).abs(), acc[:M] + E.EPS_BF16 * ref[:M].abs()))
        _rec("skinny_gemm tier B epi 1", E.ratio((y1.double() - ref1[:M]).abs(),
                                                 acc[:M] + (K + S + 4) * E.U * o["res"][:M].double().abs() + E.U * ref1[:M].abs()))
        _rec("skinny_gemm tier B epi 2", E.ratio((y2.double() - g[:M]).abs(), 1.13 * acc[:M] + E.EPS_BF16 * g[:M].abs() + 1e-6))
        if M == C.SK_MAXM:
            full = {0: y0.clone(), 1: y1.clone(), 2: y2.clone()}
        else:                                                          # a row's result does not depend on M, bit for bit
            assert _same_bits(y0, full[0][:M]) and _same_bits(y1, full[1][:M]) and _same_bits(y2, full[2][:M]), M


# ------------------------------------------------------------------------------------------------ LM head
def _lm_case(V, M):
    """integer h, wte with planted ties: rows 1 and 3 of wte (and the last row: another tile at V = 33) are 4 sign(h[0]), row 0's
    largest possible logit; row 2 duplicates row 0 of wte, so every row of h has equal logits at columns 0 and 2"""
    h, wte = E.small_ints((M, C.LM_K), 100 + V + M), E.small_ints((V, C.LM_K), 200 + V)
    h[0, :8] = torch.tensor([1.0, -2, 3, -4, 1, 2, -3, 4])
    top = 4 * torch.sign(h[0])
    wte[1], wte[3], wte[V - 1], wte[2] = top, top, top, wte[0]
    return h.to(DEV).bfloat16(), wte.to(DEV).bfloat16()


@pytest.mark.parametrize("M", [1, 33])
@pytest.mark.parametrize("V", C.LM_V)
def test_lm_head_small_vocabulary(V, M):
    hip = _hip()
    h, wte = _lm_case(V, M)
    exact = h.double() @ wte.double().t()
    assert float(exact.abs().max()) < 2 ** 24
    ids, lg = hip.lm_head_argmax(h, wte, logits=True)
    assert torch.equal(lg, exact.float())
    assert torch.equal(ids, E.topk_order(exact, 1)[1][:, 0]) and int(ids[0]) == 1
    assert torch.equal(hip.lm_head_argmax(h, wte), ids)
    lse = torch.logsumexp(exact, dim=1)
    rb = ((C.LM_K + 4) * E.U * (h.double().abs() @ wte.double().abs().t())).max(dim=1).values
    for B in C.LM_B:
        vals, idx, logZ, lg2 = hip.lm_head_topk(h, wte, B, logits=True)
        ev, ei = E.topk_order(exact, B)
        assert torch.equal(lg2, exact.float()) and torch.equal(vals, ev.float()) and torch.equal(idx.long(), ei), (V, M, B)
        if B == 5:
            assert idx[0, :3].tolist() == [1, 3, V - 1]                 # the planted tie, lowest index first
        _rec("lm_head_topk logZ", E.ratio((logZ.double() - lse).abs(), rb + E.lse_chain(V) * E.U * (1 + logZ.double().abs())))
        v2, i2, z2 = hip.lm_head_topk(h, wte, B)
        assert torch.equal(v2, vals) and torch.equal(i2, idx) and _same_bits(z2, logZ)


# ------------------------------------------------------------------------------------------------ decode attention
def _decode_operands(n, heads, L, hist, dominant, seed):
    """qkv [n, 3 W] and the history keys / values [n, hist, W] (CPU bf16).  dominant = a key position: q = 64 e_0 per head, that key
    64 e_0 and every other key 0, so its logit is 512 above the others' and every other weight is exactly 0 in f32"""
    W = heads * 64
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(n, 3 * W, generator=g)
    hk, hv = torch.randn(n, hist, W, generator=g), torch.randn(n, hist, W, generator=g) * 2
    if dominant is not None:
        qkv[:, :2 * W] = 0
        hk[:] = 0
        qkv.view(n, 3, heads, 64)[:, 0, :, 0] = 64.0
        if dominant == L - 1:
            qkv.view(n, 3, heads, 64)[:, 1, :, 0] = 64.0
        else:
            hk.view(n, hist, heads, 64)[:, dominant, :, 0] = 64.0
    return qkv.bfloat16(), hk.bfloat16(), hv.bfloat16()


def _decode_check(key, o, qkv, k, v, heads, dominant):
    """o [n, W] against the float64 reference of q and the keys / values [n, L, W] the step is to see"""
    n, L, W = k.shape
    assert bool(torch.isfinite(o.float()).all()), key
    ref, vmax = E.decode_ref(qkv[:, :W].double().view(n, heads, 64), k.double().view(n, L, heads, 64), v.double().view(n, L, heads, 64), 0.125)
    _rec(key, E.ratio((o.double() - ref).abs(), E.decode_bound(ref, vmax)))
    if dominant is not None:
        assert torch.equal(o, v[:, dominant]), (key, "one key with weight 1: the output is its value row")


def _decode_run(heads, Lmax, L, pad, dominant=None):
    hip = _hip()
    n, W = 2, heads * 64
    qkv, hk, hv = _decode_operands(n, heads, L, L - 1, dominant, 31 * L + heads)
    qb = _nan((n, 3 * W + pad), torch.bfloat16)
    qb[:, :3 * W] = qkv.to(DEV)
    kc, vc = _nan((n, Lmax, W), torch.bfloat16), _nan((n, Lmax, W), torch.bfloat16)     # NaN in every row the step must not read
    kc[:, :L - 1], vc[:, :L - 1] = hk.to(DEV), hv.to(DEV)
    kc0, vc0 = kc.clone(), vc.clone()
    ob = _nan((n + 2, W), torch.bfloat16)
    rc = hip._L().cddmsl_decode_attn(_p(qb), _p(kc), _p(vc), _p(ob), n, heads, 64, L, Lmax, 3 * W + pad, 0.125, 0, hip.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0 and bool(torch.isnan(ob[n:].float()).all())
    k, v = torch.cat([hk, qkv[:, None, W:2 * W]], 1), torch.cat([hv, qkv[:, None, 2 * W:]], 1)
    _decode_check("decode_attn", ob[:n].cpu(), qkv, k, v, heads, dominant)
    kc0[:, L - 1], vc0[:, L - 1] = qkv[:, W:2 * W].to(DEV), qkv[:, 2 * W:].to(DEV)       # the step's own row, nothing else
    assert _same_bits(kc, kc0) and _same_bits(vc, vc0)
    return ob[:n].cpu()


DECODE_CASES = [(Lmax, L) for Lmax, Ls in C.DECODE_L.items() for L in Ls]


@pytest.mark.parametrize("Lmax,L", DECODE_CASES)
@pytest.mark.parametrize("heads", C.DECODE_HEADS)
def test_decode_attn_edges(heads, Lmax, L):
    a = _decode_run(heads, Lmax, L, 0)
    b = _decode_run(heads, Lmax, L, 8)                                 # ldqkv = 3 W + 8, NaN in the gap
    assert _same_bits(a, b)
    for dom in sorted({0, (L - 1) // 2, L - 1}):
        _decode_run(heads, Lmax, L, 8, dominant=dom)


BEAM_CASES = [(260, s) for s in (1, 31, 32, 33, 255, 256, 257)] + [(48, 47), (48, 48)]     # (Tg, L - P)


@pytest.mark.parametrize("Tg,s", BEAM_CASES)
@pytest.mark.parametrize("P", C.BEAM_P)
def test_decode_attn_beam_edges(P, Tg, s):
    hip = _hip()
    B, caps, heads = C.BEAM_B, 2, 3
    rows, W, L, t = caps * B, heads * 64, P + s, s - 1                 # t generated positions are read, position t is written
    for dominant in (None, L // 2):
        # ck / cv [rows, L - 1, W]: what each cache row holds (prefix positions, then generated positions 0..t-1)
        qkv, ck, cv = _decode_operands(rows, heads, L, L - 1, dominant, 17 * L + P)
        if P:                                                          # a caption's beams share its prefix
            ck[:, :P], cv[:, :P] = ck[::B, :P].repeat_interleave(B, 0), cv[::B, :P].repeat_interleave(B, 0)
        anc = torch.randint(0, B, (rows, Tg), generator=torch.Generator().manual_seed(s), dtype=torch.uint8)
        own = (torch.arange(rows) // B * B).unsqueeze(1) + anc[:, :t].long()        # the cache row that holds position j of row r
        st = torch.arange(t)
        hk, hv = ck.clone(), cv.clone()                                # the history row r sees: its ancestors' slots
        hk[:, P:], hv[:, P:] = ck[own, P + st], cv[own, P + st]
        named = torch.zeros(rows, t, dtype=torch.bool)
        named[own, st] = True
        gk, gv = _nan((rows, Tg, W), torch.bfloat16), _nan((rows, Tg, W), torch.bfloat16)     # NaN in every slot no beam names
        gk[:, :t][named.to(DEV)] = ck[:, P:][named].to(DEV)
        gv[:, :t][named.to(DEV)] = cv[:, P:][named].to(DEV)
        if P:
            pk, pv = ck[::B, :P].contiguous().to(DEV), cv[::B, :P].contiguous().to(DEV)
        else:
            pk, pv = (torch.empty((caps, 0, W), dtype=torch.bfloat16, device=DEV) for _ in range(2))   # never read
        gk0, gv0 = gk.clone(), gv.clone()
        o = hip.decode_attn_beam(qkv.to(DEV), pk, pv, gk, gv, anc.to(DEV), L, B, heads, 0.125)
        torch.cuda.synchronize()
        k, v = torch.cat([hk, qkv[:, None, W:2 * W]], 1), torch.cat([hv, qkv[:, None, 2 * W:]], 1)
        _decode_check("decode_attn_beam", o.cpu(), qkv, k, v, heads, dominant)
        gk0[:, t], gv0[:, t] = qkv[:, W:2 * W].to(DEV), qkv[:, 2 * W:].to(DEV)
        assert _same_bits(gk, gk0) and _same_bits(gv, gv0)


def test_decode_attn_refusals():
    hip = _hip()
    W = 192
    qb, kc, ob = _nan((2, 3 * W + 8), torch.bfloat16), _nan((2, 48, W), torch.bfloat16), _nan((2, W), torch.bfloat16)
    vc = kc.clone()
    for L, Lmax, ld, dh in ((49, 48, 3 * W, 64), (0, 48, 3 * W, 64), (4, 48, 3 * W + 4, 64), (4, 48, 3 * W - 8, 64), (4, 48, 3 * W, 32)):
        assert hip._L().cddmsl_decode_attn(_p(qb), _p(kc), _p(vc), _p(ob), 2, 3, dh, L, Lmax, ld, 0.125, 0, hip.stream_ptr()) == ERR_ARG
    torch.cuda.synchronize()
    assert bool(torch.isnan(ob.float()).all()) and bool(torch.isnan(kc.float()).all()) and bool(torch.isnan(vc.float()).all())


def test_worst_ratio_table(capsys):
    """the module's last test: the worst |err| / bound of every kernel output the tests before it checked, one line each (shown
    without -s); every ratio is at most 1"""
    lines = ["", "worst |err| / bound per kernel output:"] + [f"  {k:44s} {WORST[k]:.3f}" for k in sorted(WORST)]
    with capsys.disabled():
        print("\n".join(lines))
    assert all(v <= 1.0 for v in WORST.values()), WORST
