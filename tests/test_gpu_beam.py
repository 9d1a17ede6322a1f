"""GPU: beam-search captioning.  The three kernels it adds (csrc/gpt2.hip: LM-head top-B + log-sum-exp, beam selection, decode
attention through the ancestry table) against float64 references / the numpy restatement of the rule (tests/beam_ref.py), and
``GPT2Decoder.generate_beam`` against ``generate`` (one beam), ``torch_beam`` (f32 path), a teacher-forced rescoring (bf16 path),
itself on other batches, and through tools/gen_captions.py."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import beam_ref  # noqa: E402
from test_gpu_caption import BF, BF16_TOL, DEV, GOLD, KV_TOL, U, bf, decoders, prefixes, rnd  # noqa: E402,F401  (decoders: fixture)

pytestmark = pytest.mark.gpu
K = 768


# ------------------------------------------------------------------------------------------------ LM head top-B
@pytest.fixture(scope="module", params=[50257, 4099])
def head(request):
    """one 64-row problem per vocabulary size; the calls with fewer rows take its first rows, so one float64 product serves all"""
    V = request.param
    h, wte = bf(rnd(64, K, seed=V % 89 + 3)), bf(rnd(V, K, seed=21, scale=0.1))
    exact = h.double() @ wte.double().t()
    bound = (K + 4) * U * (h.double().abs() @ wte.double().abs().t())
    return V, h, wte, exact, bound, torch.logsumexp(exact, dim=1)


def lse_chain(V):
    """the longest chain of additions in k_lm_head_topk's sum of exponentials: a thread adds its ceil(V / 512) terms one after
    the other, the 64 lanes combine in 6 butterfly rounds, the 8 waves in 7 additions; plus 8 for expf, logf, the subtraction of the
    maximum inside the exponent and the final addition"""
    c = -(-V // 512) + 6 + 7 + 8
    assert c <= V
    return c


@pytest.mark.parametrize("B", [1, 5, 8])
@pytest.mark.parametrize("M", [1, 7, 64])
def test_lm_head_topk_exact(head, M, B):
    from cddmsl_amd import hip
    V, h, wte, exact, bound, lse = head
    hm, ex, bd = h[:M].contiguous(), exact[:M], bound[:M]
    vals, idx, logZ, lg = hip.lm_head_topk(hm, wte, B, logits=True)
    assert vals.shape == idx.shape == (M, B) and idx.dtype == torch.int32 and logZ.shape == (M,)
    assert ((lg.double() - ex).abs() <= bd).all()
    assert torch.equal(vals, lg.gather(1, idx.long()))
    if B > 1:                                                                   # strictly decreasing in the better() order
        a, b, ia, ib = vals[:, :-1], vals[:, 1:], idx[:, :-1], idx[:, 1:]
        assert ((a > b) | ((a == b) & (ia < ib))).all()
    rb = bd.max(dim=1).values
    top = ex.topk(B + 1, dim=1)
    got = ex.gather(1, idx.long())
    assert (got >= (top.values[:, B - 1] - 2 * rb).unsqueeze(1)).all()
    clear = top.values[:, B - 1] - top.values[:, B] > 2 * rb                    # rows whose top-B set no rounding can change
    assert clear.float().mean().item() >= 0.75, clear
    assert torch.equal(idx.long().sort(dim=1).values[clear], top.indices[:, :B].sort(dim=1).values[clear])
    err = (logZ.double() - lse[:M]).abs()
    tol = rb + lse_chain(V) * U * (1 + logZ.double().abs())
    print(f"V {V} M {M} B {B}: logZ error {err.max().item():.2e} (bound {tol.min().item():.2e}), {int(clear.sum())}/{M} rows clear")
    assert (err <= tol).all()
    v2, i2, z2 = hip.lm_head_topk(hm, wte, B)                                   # through the workspace instead of a logits output
    assert torch.equal(v2, vals) and torch.equal(i2, idx) and torch.equal(z2, logZ)


@pytest.mark.parametrize("B", [5, 8])
def test_lm_head_topk_row_independent_of_batch(head, B):
    from cddmsl_amd import hip
    V, h, wte = head[:3]
    vals, idx, logZ = hip.lm_head_topk(h, wte, B)
    for r in (0, 13, 31, 32, 63):
        v1, i1, z1 = hip.lm_head_topk(h[r:r + 1].contiguous(), wte, B)
        assert torch.equal(v1[0], vals[r]) and torch.equal(i1[0], idx[r]) and torch.equal(z1[0], logZ[r]), r


def test_lm_head_topk_duplicates_ascend():
    from cddmsl_amd import hip
    V = 50257
    h = bf(rnd(7, K, seed=30))
    wte = rnd(V, K, seed=31, scale=0.05)
    u = h[0].float().cpu().sign() * 0.25                       # row 0's largest possible logit, five times
    dup = [321, 333, 40000, 40031, 50256]                      # one tile (321, 333), across tiles, a tile's last column, the last row
    for j in dup:
        wte[j] = u
    wte = bf(wte)
    for B in (8, 5, 3, 1):
        vals, idx, _ = hip.lm_head_topk(h, wte, B)
        assert idx[0, :min(B, 5)].tolist() == dup[:B], B       # ascending; at the B boundary the lower indices stay
        assert (vals[0, :min(B, 5)] == vals[0, 0]).all()
        assert all(int(i) not in dup for i in idx[0, 5:])


def test_lm_head_topk_rejects_out_of_contract():
    from cddmsl_amd import hip
    from cddmsl_amd._lib import HipLibraryError
    wte = bf(torch.zeros(4099, K))
    for B in (0, 9):
        with pytest.raises(HipLibraryError):
            hip.lm_head_topk(bf(torch.zeros(4, K)), wte, B)
    with pytest.raises(HipLibraryError):
        hip.lm_head_topk(bf(torch.zeros(65, K)), wte, 5)
    with pytest.raises(HipLibraryError):
        hip.lm_head_topk(bf(torch.zeros(65, K)), wte, 5, logits=True)
    with pytest.raises(HipLibraryError):
        hip.lm_head_topk(bf(torch.zeros(4, 96)), bf(torch.zeros(4099, 96)), 5)         # K % 64 != 0


# ------------------------------------------------------------------------------------------------ beam selection
BV, BT, BSTEP, BSTOP = 4099, 9, 4, 7


def to_dev(st, n, B, T):
    from cddmsl_amd import hip
    bs = hip.BeamState(n, B, T, DEV)
    for k in ("sum", "len", "stop", "hist", "anc", "src", "next_tok"):
        getattr(bs, k).copy_(torch.from_numpy(st[k]))
    return bs


def from_dev(bs):
    return {k: getattr(bs, k).cpu().numpy() for k in ("sum", "len", "stop", "hist", "anc", "src", "next_tok")}


def garbage_state(rs, n, B, T):
    """what the output buffers held before: every entry the kernel does not write must come back unchanged"""
    st = beam_ref.empty_state(n, B, T)
    st["sum"][:] = rs.standard_normal((n, B))
    for k in ("len", "hist", "src", "next_tok"):
        st[k][:] = rs.randint(-5, 100, st[k].shape)
    st["stop"][:] = rs.randint(0, 2, (n, B))
    st["anc"][:] = rs.randint(0, 255, st["anc"].shape)
    return st


@pytest.mark.parametrize("mode", ["step0", "none", "some", "all", "ties"])
@pytest.mark.parametrize("B", [1, 2, 5, 8])
@pytest.mark.parametrize("n", [1, 12])
def test_beam_step_equals_reference(n, B, mode):
    from cddmsl_amd import hip
    rs = np.random.RandomState(1000 * n + 10 * B + len(mode))
    step = 0 if mode == "step0" else BSTEP
    rows = n if step == 0 else n * B
    stopped = {"some": rs.rand(n, B) < 0.4, "all": np.ones((n, B), bool)}.get(mode, np.zeros((n, B), bool))
    old = beam_ref.random_state(rs, n, B, BT, step, stopped, BV, BSTOP)
    logits = (rs.randint(-40, 8, (rows, BV)) * 0.25).astype(np.float32)          # coarse: equal values, equal keys
    if mode in ("none", "ties"):
        old["sum"][:, 0] = -0.01                                                  # beam 0 far ahead: several new beams share it
    if mode == "ties" and B > 1:
        old["sum"][:, 1], old["len"][:, 1] = old["sum"][:, 0], old["len"][:, 0]   # beams 0 and 1 tie in every key
        logits[1::B] = logits[0::B]
    vals, idx = beam_ref.top_b(logits, B)
    if mode == "ties" and BSTOP not in idx[0]:
        idx[0, 0] = BSTOP                                                         # the best candidate of caption 0 is the stop token
        if B > 1 and BSTOP not in idx[1]:
            idx[1, 0] = BSTOP
    logZ = np.log(np.exp(logits.astype(np.float64)).sum(1)).astype(np.float32)
    new = garbage_state(rs, n, B, BT)
    want = beam_ref.beam_step_ref(vals, idx, logZ, old, new, step, BSTOP)
    d_old, d_new = to_dev(old, n, B, BT), to_dev(new, n, B, BT)
    hip.beam_step(torch.from_numpy(vals).to(DEV), torch.from_numpy(idx).to(DEV), torch.from_numpy(logZ).to(DEV), d_old, d_new, step, BSTOP)
    got = from_dev(d_new)
    for k in want:
        assert np.array_equal(got[k], want[k]), (k, got[k], want[k])
    assert all(np.array_equal(v, old[k]) for k, v in from_dev(d_old).items())     # the old tables are only read
    if mode == "ties":
        assert want["stop"][0, 0] == 1 and want["next_tok"][0] == BSTOP
        if B > 2:
            assert max(np.bincount(want["src"][0], minlength=B)) >= 2               # shared source
    if mode == "all":
        assert np.array_equal(want["len"], np.take_along_axis(old["len"], want["src"], 1)) and (want["next_tok"] == BSTOP).all()


def test_beam_step_rejects_out_of_contract():
    from cddmsl_amd import hip
    from cddmsl_amd._lib import HipLibraryError
    z = torch.zeros((9, 9), device=DEV)
    a, b = hip.BeamState(1, 8, 4, DEV), hip.BeamState(1, 8, 4, DEV)
    a.B = b.B = 9                                                                 # (the tables are large enough for the call to be safe)
    with pytest.raises(HipLibraryError):
        hip.beam_step(z[:1], z[:1].int(), z[0, :1].contiguous(), a, b, 0)
    a.B = b.B = 8
    with pytest.raises(HipLibraryError):
        hip.beam_step(z[:8, :8].contiguous(), z[:8, :8].int().contiguous(), z[0, :8].contiguous(), a, b, 4)     # step == T


# ------------------------------------------------------------------------------------------------ decode attention through ancestry
@pytest.mark.parametrize("s", [1, 2, 27])
@pytest.mark.parametrize("P", [1, 40])
@pytest.mark.parametrize("caps,B", [(3, 5), (1, 8), (8, 8)])
def test_decode_attention_beam_exact(caps, B, P, s):
    from cddmsl_amd import hip
    H, W, Tg = 12, 768, 30
    rows, L, t = caps * B, P + s, s - 1                                           # t generated positions are read, position t is written
    qkv = bf(rnd(rows, 3 * W, seed=P + s + rows))
    pk, pv = bf(rnd(caps, P, W, seed=40)), bf(rnd(caps, P, W, seed=41))
    gk, gv = bf(rnd(rows, Tg, W, seed=42)), bf(rnd(rows, Tg, W, seed=43))
    anc = torch.randint(0, B, (rows, Tg), generator=torch.Generator().manual_seed(s), dtype=torch.uint8).to(DEV)
    pk0, pv0, gk0, gv0 = pk.clone(), pv.clone(), gk.clone(), gv.clone()
    o = hip.decode_attn_beam(qkv, pk, pv, gk, gv, anc, L, B, H, 0.125)
    cap = torch.arange(rows, device=DEV) // B
    own = (cap * B).unsqueeze(1) + anc[:, :t].long()
    st = torch.arange(t, device=DEV)
    k = torch.cat([pk0[cap], gk0[own, st], qkv[:, None, W:2 * W]], 1).double().view(rows, L, H, 64)
    v = torch.cat([pv0[cap], gv0[own, st], qkv[:, None, 2 * W:]], 1).double().view(rows, L, H, 64)
    q = qkv[:, :W].double().view(rows, H, 64)
    p = torch.softmax(torch.einsum("nhd,nlhd->nhl", q, k) * 0.125, dim=-1)
    ref = torch.einsum("nhl,nlhd->nhd", p, v).reshape(rows, W)
    vmax = v.abs().amax(dim=(1, 3)).repeat_interleave(64, dim=1)
    assert ((o.double() - ref).abs() <= BF * ref.abs() + 1e-4 * vmax).all()
    # one cache row written per row of the batch, every other byte of both caches unchanged
    assert torch.equal(gk[:, t], qkv[:, W:2 * W]) and torch.equal(gv[:, t], qkv[:, 2 * W:])
    gk0[:, t], gv0[:, t] = qkv[:, W:2 * W], qkv[:, 2 * W:]
    assert torch.equal(gk, gk0) and torch.equal(gv, gv0) and torch.equal(pk, pk0) and torch.equal(pv, pv0)
    # identity ancestry, the prefix replicated per row: bit-equal to decode_attn on the equivalent contiguous cache
    ident = (torch.arange(rows, device=DEV) % B).to(torch.uint8).unsqueeze(1).expand(rows, Tg).contiguous()
    gk1, gv1 = bf(rnd(rows, Tg, W, seed=42)), bf(rnd(rows, Tg, W, seed=43))
    kc = torch.cat([pk0[cap], gk1], 1).contiguous()
    vc = torch.cat([pv0[cap], gv1], 1).contiguous()
    o1 = hip.decode_attn_beam(qkv, pk, pv, gk1, gv1, ident, L, B, H, 0.125)
    o2 = hip.decode_attn(qkv, kc, vc, L, H, 0.125)
    assert torch.equal(o1, o2) and torch.equal(gk1, kc[:, P:]) and torch.equal(gv1, vc[:, P:])


def test_decode_attention_beam_rejects_out_of_contract():
    from cddmsl_amd import hip
    from cddmsl_amd._lib import HipLibraryError
    W = 768
    qkv, pk, gk = bf(torch.zeros(10, 3 * W)), bf(torch.zeros(2, 4, W)), bf(torch.zeros(10, 6, W))
    anc = torch.zeros((10, 6), dtype=torch.uint8, device=DEV)
    for L in (4, 11):                                                             # no generated position / past the generated cache
        with pytest.raises(HipLibraryError):
            hip.decode_attn_beam(qkv, pk, pk.clone(), gk, gk.clone(), anc, L, 5, 12, 0.125)
    with pytest.raises(HipLibraryError):
        hip.decode_attn_beam(qkv, pk, pk.clone(), gk, gk.clone(), anc, 9, 4, 12, 0.125)            # rows not a multiple of B


# ------------------------------------------------------------------------------------------------ the decoder
def early_stop(dec, p):
    """a token many sequences emit early, at different steps (as test_bf16_batch_invariance_with_stops picks it)"""
    t0, _ = dec.generate(p, max_tokens=16)
    vals, counts = torch.unique(t0[:, 1:6], return_counts=True)
    return int(vals[counts.argmax()])


def surviving_stop(dec, p, B, T):
    """(a stop token that leaves beams ended at different steps among the returned ones, the search with it).  A stopped beam keeps
    its score while the mean log-probability of the others goes on rising on this decoder (it repeats itself ever more surely), so
    after most tokens, early_stop's among them, every stopped beam is overtaken before the end.  The tokens of the search without a
    stop are tried, the most frequent first (the last step's are left out: a stop there ends nothing early), until one qualifies."""
    tokens = dec.generate_beam(p, beam_size=B, max_tokens=T)[0]
    vals, counts = torch.unique(tokens[:, :, :T - 1], return_counts=True)
    for stop in vals[counts.argsort(descending=True, stable=True)].tolist():
        out = dec.generate_beam(p, beam_size=B, max_tokens=T, stop_id=stop)
        if len(set(out[1][out[1] < T].tolist())) > 1:
            return stop, out
    raise AssertionError("no token of the search without a stop leaves stopped beams of different lengths")


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float32])
def test_one_beam_is_greedy(decoders, dt):
    dec = decoders[dt]
    p = prefixes(seed=11, n=70).to(DEV)
    stop = early_stop(dec, p)
    tg, lg = dec.generate(p, max_tokens=16, stop_id=stop)
    tb, lb, sc = dec.generate_beam(p, beam_size=1, max_tokens=16, stop_id=stop)
    assert len(set(lg.tolist())) > 1
    assert tb.shape == (70, 1, 16) and torch.equal(tb[:, 0], tg) and torch.equal(lb[:, 0], lg)
    assert sc.shape == (70, 1) and bool(torch.isfinite(sc).all()) and bool((sc <= 0).all())


def test_f32_path_matches_torch_beam(decoders):
    from cddmsl_amd.modeling.gpt2 import torch_beam, torch_greedy
    dec = decoders[torch.float32]
    n, B, T = 4, 5, 12
    p = prefixes(seed=6, n=n).to(DEV)          # (chosen on the reference alone: two captions compare in full, two up to steps 8 and 9)
    rt, rl, rs, gaps = torch_beam(dec, p, beam_size=B, max_tokens=T)
    # a key is a mean of logit - logZ terms; the KV-cache decode's logits (and so their log-sum-exp) are within KV_TOL * (1 + |logit|)
    # of the full recompute's (test_kv_cache_equals_full_recompute), so a key moves by at most tol and a gap by at most 2 tol
    lmax = torch_greedy(dec, p, max_tokens=T)[2].abs().max().item()
    tol = 2 * KV_TOL * (1 + lmax)
    margin = 2 * tol
    upto = [int(np.nonzero(g < margin)[0][0]) if (g < margin).any() else len(g) for g in gaps.cpu().numpy()]
    print(f"max |logit| {lmax:.2f}, margin {margin:.2e}, compared steps per caption {upto} of {gaps.shape[1]}, smallest gap {gaps.min().item():.2e}")
    assert sum(upto) >= n * T / 2                                                  # (a property of the reference alone)
    full = dec.generate_beam(p, beam_size=B, max_tokens=T)
    for c, u in enumerate(upto):
        if u == 0:
            continue
        # the beams after u tokens are what a run of u tokens returns: compare up to the first close call
        want = (rt[c], rl[c], rs[c]) if u == T else [v[0] for v in torch_beam(dec, p[c:c + 1], beam_size=B, max_tokens=u)[:3]]
        got = [v[c] for v in full] if u == T else [v[0] for v in dec.generate_beam(p[c:c + 1], beam_size=B, max_tokens=u)]
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), (c, u)
        err = (got[2] - want[2]).abs().max().item()
        print(f"caption {c}, {u} tokens: scores differ by {err:.2e} (tolerance {tol:.2e})")
        assert err <= tol, (c, u)


def rescore(dec, p, tokens, lengths):
    """mean log-softmax (f32, teacher-forced torch_gpt2_logits over prefix + tokens) at each returned beam's own tokens -> [N, B]"""
    from cddmsl_amd.modeling.gpt2 import torch_gpt2_logits
    N, B, T = tokens.shape
    P = p.shape[1]
    tk = tokens.clamp(min=0).view(N * B, T)
    emb = torch.cat([p.to(DEV).repeat_interleave(B, dim=0), dec.wte.weight[tk[:, :-1]]], dim=1)
    with torch.no_grad():
        lp = torch.log_softmax(torch_gpt2_logits(dec, emb)[:, P - 1:], dim=-1).gather(2, tk.unsqueeze(2)).squeeze(2)    # [N*B, T]
    keep = torch.arange(T, device=DEV).unsqueeze(0) < lengths.view(N * B, 1)
    return ((lp * keep).sum(1) / lengths.view(N * B)).view(N, B)


def test_bf16_beams_rescore(decoders):
    dec = decoders[torch.bfloat16]
    n, B, T = 6, 5, 16
    p = prefixes(seed=11, n=n).to(DEV)
    stop, (tokens, lengths, scores) = surviving_stop(dec, p, B, T)
    assert tokens.shape == (n, B, T) and tokens.dtype == lengths.dtype == torch.int64 and scores.dtype == torch.float32
    err = (rescore(dec, p, tokens, lengths) - scores).abs().max().item()
    print(f"bf16 beam scores vs f32 teacher-forced rescoring: {err:.4f} (tolerance {2 * BF16_TOL})")
    assert err <= 2 * BF16_TOL
    assert bool((scores[:, :-1] >= scores[:, 1:]).all())                           # best beam first
    pos = torch.arange(T, device=DEV).expand(n, B, T)
    hit = torch.where(tokens == stop, pos + 1, torch.full_like(pos, T)).min(dim=2).values
    assert torch.equal(lengths, hit) and torch.equal(tokens >= 0, pos < lengths.unsqueeze(2))
    assert len(set(lengths.view(-1).tolist())) > 1                                 # some beams stopped, at different steps


def test_bf16_beam_batch_invariance_with_stops(decoders):
    dec = decoders[torch.bfloat16]
    p = prefixes(seed=11, n=20).to(DEV)
    stop, (tb, lb, sb) = surviving_stop(dec, p, 5, 16)                             # two chunks: 12 + 8 captions
    assert len(set(lb.view(-1).tolist())) > 1                                      # beams ended at different steps
    for r in (0, 11, 12, 19):
        t1, l1, s1 = dec.generate_beam(p[r:r + 1], beam_size=5, max_tokens=16, stop_id=stop)
        assert torch.equal(t1[0], tb[r]) and torch.equal(l1[0], lb[r]) and torch.equal(s1[0], sb[r]), r


# ------------------------------------------------------------------------------------------------ tool end to end
def test_gen_captions_beam_end_to_end(tmp_path):
    from PIL import Image
    from cddmsl_amd import synthetic
    ck, cc, img = tmp_path / "det.pth", tmp_path / "clipcap.pt", tmp_path / "images"
    img.mkdir()
    torch.save({"model": synthetic.make_state_dict(0)}, ck)
    st = {"clip_project." + k: v for k, v in synthetic.make_mapper_state_dict(1).items()}
    g = synthetic.make_gpt2_state_dict(2, n_layer=2, n_embd=768, vocab=4099, n_positions=1024)
    st.update({"gpt.transformer." + k: v for k, v in g.items()})
    st["gpt.lm_head.weight"] = g["wte.weight"]
    torch.save(st, cc)
    rs = np.random.RandomState(0)
    for i, (h, w) in enumerate([(120, 160), (96, 96)]):
        Image.fromarray(rs.randint(0, 256, (h, w, 3), dtype=np.uint8)).save(img / f"im{i}.png")
    cfg = os.path.join(ROOT, "configs", "VOC-Experiments", "faster_rcnn_CLIP_R_50_C4.yaml")
    raw = {}
    for name, extra in (("greedy", []), ("one", ["--beam-size", "1"]), ("three", ["--beam-size", "3"])):
        out = tmp_path / name
        cmd = [sys.executable, os.path.join(ROOT, "tools", "gen_captions.py"), "--config-file", cfg, "--gpt2-vocab",
               os.path.join(GOLD, "gpt2_vocab.json"), "--regions", "--max-regions", "3", "--max-tokens", "8", *extra,
               "MODEL.WEIGHTS", str(ck), "MODEL.VISION_TO_LANG_PATH", str(cc), "INPUT_DIR", str(img), "OUTPUT_DIR", str(out),
               "MODEL.DEVICE", DEV, "INPUT.MIN_SIZE_TEST", "128", "INPUT.MAX_SIZE_TEST", "256", "MODEL.ROI_HEADS.SCORE_THRESH_TEST", "0.0"]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=dict(os.environ, PYTHONPATH=ROOT))
        assert r.returncode == 0, r.stderr[-3000:]
        raw[name] = open(out / "captions.json", "rb").read()
    assert raw["one"] == raw["greedy"]                                             # --beam-size 1 is the greedy path, byte for byte
    greedy, res = json.loads(raw["greedy"]), json.loads(raw["three"])
    assert sorted(res) == ["im0.png", "im1.png"] and sum(len(e["regions"]) for e in res.values()) >= 1
    for name, e in res.items():
        assert isinstance(e["caption"], str) and 1 <= len(e["tokens"]) <= 8 and np.isfinite(e["score"]) and e["score"] <= 0
        assert "score" not in greedy[name]
        for reg in e["regions"]:
            assert isinstance(reg["caption"], str) and np.isfinite(reg["score"]) and np.isfinite(reg["caption_score"]) and reg["caption_score"] <= 0
