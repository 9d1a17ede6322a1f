"""GPU: the CLIP text encoder's HIP kernels (csrc/text_encoder.hip) against float64 / torch f32, the encoder against the reference's
own ``encode_text`` (tests/golden/ref_text_encoder.npz), truncation, RN50x4 geometry, and tools/extract_concept_features.py end to
end into ``MODEL.CLIP.TEXT_EMB_PATH``."""
import gzip
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GOLD = os.path.join(ROOT, "tests", "golden", "ref_text_encoder.npz")
sys.path.insert(0, os.path.join(ROOT, "tests"))
DEV = "cuda:0"


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD, allow_pickle=False)


from exact_text import attn_ref, check_attn_bound  # noqa: E402  (the float64 reference and the bound, shared with test_gpu_text_exact.py)


@pytest.mark.parametrize("heads,n", [(8, 3), (10, 5)])
@pytest.mark.parametrize("t", [1, 2, 17, 31, 32, 33, 64, 77, 100, 128])
def test_attn_causal_random(t, heads, n):
    from cddmsl_amd import hip
    g = torch.Generator().manual_seed(1000 * t + heads)
    qkv = (torch.randn(n * t, 3 * heads * 64, generator=g) * 1.5).to(DEV).bfloat16()
    got = hip.attn_causal_fwd(qkv, t, heads, 0.125)
    ref, v = attn_ref(qkv, n, t, heads)
    check_attn_bound(got, ref, v, n, t, heads)


@pytest.mark.parametrize("t", [17, 33, 77])
def test_attn_causal_structured(t):
    """values encode their row (key) index in the first 32 channels and the channel in the others, and differ per head; the scores
    grow with the key index, so a transposed, shifted or wrongly masked tile moves the output by whole units"""
    from cddmsl_amd import hip
    n, heads = 3, 8
    qkv = torch.zeros(n, t, 3, heads, 64)
    j = torch.arange(t, dtype=torch.float32)
    qkv[:, :, 0, :, 0] = 1.0                                              # q_i = e_0
    qkv[:, :, 1, :, 0] = (0.25 * j).view(1, t, 1)                         # k_j = j/4 e_0: score(i, j) = j / 32
    qkv[:, :, 2, :, :32] = (j + 1).view(1, t, 1, 1)                       # v_j[c < 32] = j + 1
    qkv[:, :, 2, :, 32:] = torch.arange(32, dtype=torch.float32) + torch.arange(heads).view(heads, 1) * 0.5   # v_j[c >= 32]: channel, head
    qkv[1, :, 2] *= -1.0                                                  # another sequence, another sign
    qkv = qkv.view(n * t, 3 * heads * 64).to(DEV).bfloat16()
    got = hip.attn_causal_fwd(qkv, t, heads, 0.125)
    ref, v = attn_ref(qkv, n, t, heads)
    check_attn_bound(got, ref, v, n, t, heads)
    # row i of channel 0 is a weighted mean of 1 .. i+1: strictly inside (1, i + 1] and increasing in i
    o0 = got.float().view(n, t, heads, 64)[0, :, 0, 0].cpu()
    assert float(o0[0]) == 1.0 and bool((o0[1:] >= o0[:-1]).all()) and float(o0[-1]) > 0.5 * t


@pytest.mark.parametrize("t,i", [(33, 20), (77, 31), (77, 32), (64, 0)])
def test_attn_causal_rows_ignore_later_rows(t, i):
    """changing q, k, v of rows > i leaves rows <= i bit-identical"""
    from cddmsl_amd import hip
    n, heads = 3, 8
    g = torch.Generator().manual_seed(t * 100 + i)
    qkv = torch.randn(n, t, 3 * heads * 64, generator=g)
    a = hip.attn_causal_fwd(qkv.view(n * t, -1).to(DEV).bfloat16(), t, heads, 0.125).view(n, t, -1)
    qkv[:, i + 1:] = torch.randn(n, t - i - 1, 3 * heads * 64, generator=g) * 3.0
    b = hip.attn_causal_fwd(qkv.view(n * t, -1).to(DEV).bfloat16(), t, heads, 0.125).view(n, t, -1)
    assert torch.equal(a[:, :i + 1], b[:, :i + 1])
    assert not torch.equal(a[:, i + 1:], b[:, i + 1:])


def test_text_embed_quick_gelu_text_pool():
    from cddmsl_amd import hip
    g = torch.Generator().manual_seed(7)
    V, W, n, t = 1000, 640, 5, 23
    tok = torch.randn(V, W, generator=g).to(DEV)
    pos = torch.randn(77, W, generator=g).to(DEV)
    ids = torch.randint(0, V, (n, t), generator=g).to(DEV)
    for table in (tok, tok.bfloat16()):
        got = hip.text_embed(ids, table, pos)
        want = (table.float()[ids] + pos[:t]).view(n * t, W)
        assert torch.equal(got, want)
    x = (torch.randn(4096, 2048 + 8, generator=g) * 4).to(DEV)
    xb = x.bfloat16()
    got = hip.quick_gelu_(xb.clone()).float()
    want = (xb.float() * torch.sigmoid(1.702 * xb.float())).bfloat16().float()
    assert bool(((got - want).abs() <= 2.0 ** -7 * want.abs() + 1e-30).all())
    got32 = hip.quick_gelu_(x.clone())
    assert torch.allclose(got32, x * torch.sigmoid(1.702 * x), rtol=2e-6, atol=1e-7)
    R = n * t
    xs = torch.randn(R, W, generator=g).to(DEV) * 3 + 1
    gam, bet = (1 + 0.1 * torch.randn(W, generator=g)).to(DEV), (0.1 * torch.randn(W, generator=g)).to(DEV)
    rows = torch.randint(0, R, (12,), generator=g).to(DEV)
    for group in (1, 3, 4):
        want = F.layer_norm(xs[rows], (W,), gam, bet, 1e-5).view(12 // group, group, W).mean(1)
        got = hip.text_pool(xs, rows, gam, bet, group)
        assert torch.allclose(got, want, rtol=1e-5, atol=1e-5), (group, (got - want).abs().max())
        gb = hip.text_pool(xs, rows, gam, bet, group, out_dtype=torch.bfloat16)
        assert torch.equal(gb, got.bfloat16())


def rel(a, b):
    return float((a.float() - b.float()).abs().max() / b.float().abs().max())


def encoder(dtype, **geometry):
    from cddmsl_amd.modeling.text_encoder import load_text_encoder
    return load_text_encoder(synthetic_seed=geometry.pop("seed", 0), compute_dtype=dtype, **geometry).to(DEV)


def test_encoder_matches_reference(gold):
    ids = torch.from_numpy(gold["enc_ids"])
    want = torch.from_numpy(gold["enc_out"]).to(DEV)
    mids = torch.cat([torch.from_numpy(gold["ids"][c, :8].astype(np.int64)) for c in gold["mean_classes"]])
    mwant = torch.from_numpy(gold["mean_out"]).to(DEV)
    for dtype, tol in ((torch.float32, 1e-3), (torch.bfloat16, 3e-2)):
        enc = encoder(dtype)
        with torch.no_grad():
            got = enc.encode_text(ids)
            mgot = enc.encode_prompt_ids(mids, [8] * len(gold["mean_classes"]))
        cos = F.cosine_similarity(got, want, dim=1)
        mcos = F.cosine_similarity(mgot, mwant, dim=1)
        print(f"{dtype}: encode_text rel {rel(got, want):.2e} min cos {float(cos.min()):.6f}; class means rel {rel(mgot, mwant):.2e} "
              f"min cos {float(mcos.min()):.6f}")
        assert got.shape == (24, 1024) and got.dtype == torch.float32
        assert rel(got, want) <= tol and rel(mgot, mwant) <= tol
        if dtype == torch.bfloat16:
            assert float(cos.min()) >= 0.999 and float(mcos.min()) >= 0.999


def test_truncated_equals_full_width(gold):
    ids = torch.from_numpy(gold["enc_ids"][:20])            # longest prompt well short of 77
    assert int(ids.argmax(-1).max()) + 1 < 40
    for dtype in (torch.float32, torch.bfloat16):
        enc = encoder(dtype)
        with torch.no_grad():
            a, b = enc.encode_text(ids, truncate=True), enc.encode_text(ids, truncate=False)
        print(f"{dtype}: truncated vs 77 tokens: bit-equal {torch.equal(a, b)}, max |diff| {float((a - b).abs().max()):.3e}")
        if dtype == torch.float32:
            assert torch.allclose(a, b, rtol=1e-5, atol=1e-5)
        else:
            assert rel(a, b) <= 1e-2 and float(F.cosine_similarity(a, b, dim=1).min()) >= 0.9999


def test_rn50x4_geometry():
    from cddmsl_amd.modeling.text_encoder import torch_encode_text
    g = torch.Generator().manual_seed(11)
    ids = torch.randint(1, 900, (7, 77), generator=g)
    L = torch.randint(3, 40, (7,), generator=g)
    for r in range(7):
        ids[r, 0], ids[r, L[r]], ids[r, L[r] + 1:] = 998, 999, 0           # SOT, EOT (largest id), padding
    for dtype, tol in ((torch.float32, 1e-3), (torch.bfloat16, 3e-2)):
        enc = encoder(dtype, seed=5, width=640, layers=3, embed_dim=640, vocab_size=1000)
        assert enc.heads == 10
        with torch.no_grad():
            got = enc.encode_text(ids)
            want = torch_encode_text(enc, ids, torch.float64)
        assert got.shape == (7, 640) and rel(got, want) <= tol, (dtype, rel(got, want))


def test_extract_concept_features_tool(tmp_path, gold):
    from cddmsl_amd.config import get_cfg
    from cddmsl_amd.evaluation import VOC_CLASS_NAMES
    from cddmsl_amd.modeling import build_model
    (tmp_path / "in").mkdir()
    (tmp_path / "in" / "concepts.txt").write_text("\n".join(VOC_CLASS_NAMES) + "\n")
    (tmp_path / "templates.txt").write_text("\n".join(str(t) for t in gold["templates"][:8]) + "\n")
    with gzip.open(tmp_path / "vocab.txt.gz", "wt", encoding="utf-8") as f:       # the fixture's merges, as a toy vocab file
        f.write("#version: 0.2\n" + "\n".join(f"{a} {b}" for a, b in zip(gold["merge_a"], gold["merge_b"])) + "\n")
    cfgf = os.path.join(ROOT, "configs", "VOC-Experiments", "faster_rcnn_CLIP_R_50_C4.yaml")
    out = tmp_path / "out"
    cmd = [sys.executable, os.path.join(ROOT, "tools", "extract_concept_features.py"), "--config-file", cfgf,
           "--bpe-vocab", str(tmp_path / "vocab.txt.gz"), "--templates", str(tmp_path / "templates.txt"), "--synthetic-weights", "0",
           "MODEL.DEVICE", "cuda:0", "INPUT_DIR", str(tmp_path / "in"), "OUTPUT_DIR", str(out)]
    env = dict(os.environ, HIP_VISIBLE_DEVICES=os.environ.get("HIP_VISIBLE_DEVICES", "0"))
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    emb = torch.load(out / "concept_embeds.pth", map_location="cpu", weights_only=True)
    assert emb.shape == (20, 1024) and emb.dtype == torch.float32 and bool(torch.isfinite(emb).all())
    cfg = get_cfg()
    cfg.merge_from_file(cfgf)
    cfg.merge_from_list(["MODEL.DEVICE", "cpu", "MODEL.CLIP.TEXT_EMB_PATH", str(out / "concept_embeds.pth")])
    model = build_model(cfg)
    assert torch.equal(model.roi_heads.box_predictor.cls_score.weight.detach().cpu(), emb)
