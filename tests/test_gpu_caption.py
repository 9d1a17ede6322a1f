"""GPU: the GPT-2 decoder's HIP kernels (csrc/gpt2.hip) against float64 products of their bf16 operands and their formulas, the
decoder against the reference's GPT2LMHeadModel (tests/golden/ref_gpt2.npz), the KV-cache decode against the full recompute, batch
invariance of the bf16 path, and tools/gen_captions.py end to end."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GOLD = os.path.join(ROOT, "tests", "golden")
DEV = "cuda:0"
U = 2.0 ** -24                       # f32 unit roundoff
BF = 2.0 ** -8                       # twice bf16's unit roundoff
F32_TOL = 1e-4                       # f32 path vs the reference's logits, relative to 1 + |logit|
BF16_TOL = 0.25                      # bf16 path vs f32 path, logits (absolute; measured max is printed)
KV_TOL = 4e-5                        # f32 KV-cache decode vs f32 full recompute, relative to 1 + |logit|
MARGIN = 2 * BF16_TOL                # tokens must agree while the recorded top-2 margin is at least this


def prefixes(seed=1, n=3, p=40, e=768):
    return torch.from_numpy((np.random.RandomState(seed).standard_normal((n, p, e)) * 0.1).astype(np.float32))


def bf(t):
    return t.to(DEV, torch.bfloat16)


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLD, "ref_gpt2.npz"), allow_pickle=False)


@pytest.fixture(scope="module")
def decoders():
    from cddmsl_amd.modeling.gpt2 import GPT2Decoder
    from cddmsl_amd.synthetic import make_gpt2_state_dict
    sd = make_gpt2_state_dict(0, n_layer=2, n_embd=768, vocab=4099, n_positions=1024)
    return {dt: GPT2Decoder.from_state_dict(sd, dt).to(DEV) for dt in (torch.float32, torch.bfloat16)}


# ------------------------------------------------------------------------------------------------ skinny GEMM
SHAPES = [(768, 2304), (768, 768), (768, 3072), (3072, 768), (192, 200)]


@pytest.mark.parametrize("M", [1, 5, 16, 33, 64])
@pytest.mark.parametrize("K,N", SHAPES)
def test_skinny_gemm_exact(M, K, N):
    from cddmsl_amd import hip
    x, w = bf(rnd(M, K, seed=M)), bf(rnd(N, K, seed=N + K, scale=0.05))
    bias, res = rnd(N, seed=3).to(DEV), rnd(M, N, seed=4).to(DEV)
    exact = x.double() @ w.double().t()
    S = hip.skinny_gemm_workspace(M, N, K) // (M * N * 4)
    acc = (K + S + 4) * U * (x.double().abs() @ w.double().abs().t() + bias.double().abs())
    ref = exact + bias.double()
    y0 = hip.skinny_gemm(x, w, bias, epi=0)
    assert y0.dtype == torch.bfloat16 and ((y0.double() - ref).abs() <= acc + BF * ref.abs()).all()
    y1 = hip.skinny_gemm(x, w, bias, residual=res, epi=1)
    ref1 = ref + res.double()
    assert y1.dtype == torch.float32 and ((y1.double() - ref1).abs() <= acc + (K + S + 4) * U * res.double().abs() + U * ref1.abs()).all()
    y2 = hip.skinny_gemm(x, w, bias, epi=2)
    g = 0.5 * ref * (1 + torch.tanh(0.7978845608028654 * (ref + 0.044715 * ref ** 3)))
    assert ((y2.double() - g).abs() <= 1.13 * acc + BF * g.abs() + 1e-6).all()
    y3 = hip.skinny_gemm(x, w, None, epi=0)                                   # no bias
    assert ((y3.double() - exact).abs() <= acc + BF * exact.abs()).all()


@pytest.mark.parametrize("K,N", SHAPES)
def test_skinny_gemm_row_independent_of_batch(K, N):
    from cddmsl_amd import hip
    x, w = bf(rnd(64, K, seed=7)), bf(rnd(N, K, seed=8, scale=0.05))
    bias, res = rnd(N, seed=9).to(DEV), rnd(64, N, seed=10).to(DEV)
    full = hip.skinny_gemm(x, w, bias, residual=res, epi=1)
    for r in (0, 13, 31, 32, 63):
        one = hip.skinny_gemm(x[r:r + 1].contiguous(), w, bias, residual=res[r:r + 1].contiguous(), epi=1)
        assert torch.equal(one[0], full[r]), r
    assert torch.equal(hip.skinny_gemm(x[:5].contiguous(), w, bias, epi=2), hip.skinny_gemm(x, w, bias, epi=2)[:5])


def test_skinny_gemm_rejects_out_of_contract():
    from cddmsl_amd import hip
    from cddmsl_amd._lib import HipLibraryError
    with pytest.raises(HipLibraryError):
        hip.skinny_gemm(bf(torch.zeros(65, 768)), bf(torch.zeros(64, 768)))
    with pytest.raises(HipLibraryError):
        hip.skinny_gemm(bf(torch.zeros(4, 96)), bf(torch.zeros(64, 96)))                # K % 64 != 0


# ------------------------------------------------------------------------------------------------ LM head + argmax
@pytest.mark.parametrize("M", [1, 7, 64])
def test_lm_head_argmax_exact(M):
    from cddmsl_amd import hip
    V, K = 50257, 768
    h, wte = bf(rnd(M, K, seed=M + 20)), bf(rnd(V, K, seed=21, scale=0.1))
    ids, lg = hip.lm_head_argmax(h, wte, logits=True)
    exact = h.double() @ wte.double().t()
    bound = (K + 4) * U * (h.double().abs() @ wte.double().abs().t())
    assert ((lg.double() - exact).abs() <= bound).all()
    best = exact.max(dim=1).values
    got = exact.gather(1, ids.view(-1, 1)).view(-1)
    assert (got >= best - 2 * bound.max(dim=1).values).all()
    assert torch.equal(hip.lm_head_argmax(h, wte), ids)                       # without the logits output: the same ids


def test_lm_head_ties_go_to_lowest_index():
    from cddmsl_amd import hip
    V, K = 50257, 768
    h = bf(rnd(7, K, seed=30))
    wte = rnd(V, K, seed=31, scale=0.05)
    u = (h[0].float().cpu().sign() * 0.25)
    for j in (50256, 40000, 333, 321):                     # same tile (321, 333), other tiles, the vocabulary's last row
        wte[j] = u
    wte = bf(wte)
    ids = hip.lm_head_argmax(h, wte)
    assert int(ids[0]) == 321
    wte[321] = bf(rnd(K, seed=32, scale=0.05))
    wte[333] = bf(rnd(K, seed=33, scale=0.05))
    assert int(hip.lm_head_argmax(h, wte)[0]) == 40000
    ids7 = hip.lm_head_argmax(h, wte)
    assert torch.equal(ids7, hip.lm_head_argmax(h, wte))


# ------------------------------------------------------------------------------------------------ decode attention
@pytest.mark.parametrize("L", [1, 40, 41, 107, 1024])
@pytest.mark.parametrize("n", [1, 13])
def test_decode_attention_exact(L, n):
    from cddmsl_amd import hip
    H, W, Lmax = 12, 768, 1024
    qkv = bf(rnd(n, 3 * W, seed=L + n))
    kc, vc = bf(rnd(n, Lmax, W, seed=40)), bf(rnd(n, Lmax, W, seed=41))
    kc0, vc0 = kc.clone(), vc.clone()
    o = hip.decode_attn(qkv, kc, vc, L, H, 0.125)
    k = torch.cat([kc0[:, :L - 1], qkv[:, None, W:2 * W]], 1).double().view(n, L, H, 64)
    v = torch.cat([vc0[:, :L - 1], qkv[:, None, 2 * W:]], 1).double().view(n, L, H, 64)
    q = qkv[:, :W].double().view(n, H, 64)
    p = torch.softmax(torch.einsum("nhd,nlhd->nhl", q, k) * 0.125, dim=-1)
    ref = torch.einsum("nhl,nlhd->nhd", p, v).reshape(n, W)
    vmax = v.abs().amax(dim=(1, 3)).repeat_interleave(64, dim=1)
    assert ((o.double() - ref).abs() <= BF * ref.abs() + 1e-4 * vmax).all()
    assert torch.equal(kc[:, L - 1], qkv[:, W:2 * W]) and torch.equal(vc[:, L - 1], qkv[:, 2 * W:])
    assert torch.equal(kc[:, :L - 1], kc0[:, :L - 1]) and torch.equal(kc[:, L:], kc0[:, L:])


# ------------------------------------------------------------------------------------------------ gelu_new, embedding
def test_gelu_new_and_offset_embedding():
    from cddmsl_amd import hip, layers
    x = rnd(40 * 3, 3072, seed=50, scale=3).to(DEV)
    g = 0.5 * x.double() * (1 + torch.tanh(0.7978845608028654 * (x.double() + 0.044715 * x.double() ** 3)))
    assert ((hip.gelu_new_(x.clone()).double() - g).abs() <= 1e-6 * (1 + g.abs())).all()
    xb = bf(x)
    gb = 0.5 * xb.double() * (1 + torch.tanh(0.7978845608028654 * (xb.double() + 0.044715 * xb.double() ** 3)))
    assert ((hip.gelu_new_(xb.clone()).double() - gb).abs() <= BF * gb.abs() + 1e-6).all()
    wte, wpe = bf(rnd(4099, 768, seed=51)), rnd(1024, 768, seed=52).to(DEV)
    tokens = torch.randint(0, 4099, (13, 9), generator=torch.Generator().manual_seed(5)).to(DEV)
    got = layers.token_position_embed(tokens[:, 4], wte, wpe, 517)
    assert torch.equal(got, wte[tokens[:, 4]].float() + wpe[517])
    pre = rnd(5, 40, 768, seed=53).to(DEV)
    assert torch.equal(layers.prefix_position_embed(pre, wpe), (pre + wpe[:40]).view(200, 768))
    wte32 = rnd(4099, 768, seed=54).to(DEV)
    assert torch.equal(layers.token_position_embed(tokens[:, 0], wte32, wpe, 0), wte32[tokens[:, 0]] + wpe[0])


# ------------------------------------------------------------------------------------------------ model parity
def _first_small_margin(margins, bound):
    """per sequence: the first step whose recorded margin is below ``bound`` (len when none)"""
    out = []
    for m in margins:
        small = np.nonzero(m < bound)[0]
        out.append(int(small[0]) if len(small) else len(m))
    return out


def test_f32_path_matches_reference(gold, decoders):
    dec = decoders[torch.float32]
    steps = gold["tokens"].shape[1]
    tokens, lengths, logits = dec.generate(prefixes().to(DEV), max_tokens=steps, return_logits=True)
    ref_tok = torch.from_numpy(gold["tokens"])
    for i, s in enumerate(gold["logit_steps"].tolist()):
        ref = torch.from_numpy(gold["logits"][:, i]).to(DEV)
        err = ((logits[:, s] - ref).abs() / (1 + ref.abs())).max().item()
        print(f"f32 path vs reference, step {s}: {err:.2e}")
        assert err <= F32_TOL, s
    for r, upto in enumerate(_first_small_margin(gold["margins"], 1e-3)):
        assert torch.equal(tokens[r, :upto].cpu(), ref_tok[r, :upto]), r
    assert lengths.tolist() == [steps] * 3


def test_bf16_path_matches_f32_path(gold, decoders):
    steps = gold["tokens"].shape[1]
    p = prefixes().to(DEV)
    t32, _, l32 = decoders[torch.float32].generate(p, max_tokens=steps, return_logits=True)
    t16, _, l16 = decoders[torch.bfloat16].generate(p, max_tokens=steps, return_logits=True)
    worst = 0.0
    for r, upto in enumerate(_first_small_margin(gold["margins"], MARGIN)):
        assert torch.equal(t16[r, :upto], t32[r, :upto]), r
        same = int((t16[r] == t32[r]).long().cumprod(0).sum())          # logits comparable while the inputs agree
        d = (l16[r, :same + 1 if same < steps else steps] - l32[r, :same + 1 if same < steps else steps]).abs().max().item()
        worst = max(worst, d)
    print(f"bf16 vs f32 logits: max |diff| {worst:.4f}")
    assert worst <= BF16_TOL


def test_kv_cache_equals_full_recompute(decoders):
    from cddmsl_amd.modeling.gpt2 import torch_greedy
    dec = decoders[torch.float32]
    p = prefixes(seed=7, n=4).to(DEV)
    tokens, lengths, logits = dec.generate(p, max_tokens=12, return_logits=True)
    rt, rl, rlog = torch_greedy(dec, p, max_tokens=12)
    # both sides are f32 but sum in different orders (the HIP f32 GEMM vs torch's matmul, one row vs the whole sequence): measured
    # 1.8e-5 of 1 + |logit| on one MI355X, the same size as the f32 path's distance to the reference
    err = ((logits - rlog).abs() / (1 + rlog.abs())).max().item()
    print(f"KV cache vs full recompute: {err:.2e}")
    assert err <= KV_TOL
    assert torch.equal(tokens, rt) and torch.equal(lengths, rl)


def test_bf16_batch_invariance_with_stops(decoders):
    dec = decoders[torch.bfloat16]
    p = prefixes(seed=11, n=70).to(DEV)
    t0, _ = dec.generate(p, max_tokens=16)
    vals, counts = torch.unique(t0[:, 1:6], return_counts=True)
    stop = int(vals[counts.argmax()])                                  # a token many sequences emit early, at different steps
    tb, lb = dec.generate(p, max_tokens=16, stop_id=stop)
    assert len(set(lb.tolist())) > 1                                    # sequences end at different steps
    for r in (0, 3, 31, 63, 64, 69):
        t1, l1 = dec.generate(p[r:r + 1], max_tokens=16, stop_id=stop)
        assert torch.equal(t1[0], tb[r]) and int(l1[0]) == int(lb[r]), r
    tg, lg = dec.generate(p[60:70], max_tokens=16, stop_id=stop)
    assert torch.equal(tg, tb[60:70]) and torch.equal(lg, lb[60:70])


# ------------------------------------------------------------------------------------------------ tool end to end
def test_gen_captions_end_to_end(tmp_path):
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
    sizes = [(120, 160), (200, 150), (96, 96)]
    for i, (h, w) in enumerate(sizes):
        Image.fromarray(rs.randint(0, 256, (h, w, 3), dtype=np.uint8)).save(img / f"im{i}.png")
    cfg = os.path.join(ROOT, "configs", "VOC-Experiments", "faster_rcnn_CLIP_R_50_C4.yaml")
    for dt in ("bf16", "f32"):
        out = tmp_path / dt
        cmd = [sys.executable, os.path.join(ROOT, "tools", "gen_captions.py"), "--config-file", cfg, "--gpt2-vocab",
               os.path.join(GOLD, "gpt2_vocab.json"), "--regions", "--max-regions", "3", "--max-tokens", "8", "--dtype", dt,
               "MODEL.WEIGHTS", str(ck), "MODEL.VISION_TO_LANG_PATH", str(cc), "INPUT_DIR", str(img), "OUTPUT_DIR", str(out),
               "MODEL.DEVICE", DEV, "INPUT.MIN_SIZE_TEST", "128", "INPUT.MAX_SIZE_TEST", "256",
               "MODEL.ROI_HEADS.SCORE_THRESH_TEST", "0.0"]       # random weights score ~1/21 per class: keep detections
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=dict(os.environ, PYTHONPATH=ROOT))
        assert r.returncode == 0, r.stderr[-3000:]
        res = json.load(open(out / "captions.json", encoding="utf-8"))
        assert sorted(res) == [f"im{i}.png" for i in range(3)]
        assert sum(len(res[f"im{i}.png"]["regions"]) for i in range(3)) >= 1, res
        for i, (h, w) in enumerate(sizes):
            e = res[f"im{i}.png"]
            assert isinstance(e["caption"], str) and 1 <= len(e["tokens"]) <= 8
            assert len(e["regions"]) <= 3
            for reg in e["regions"]:
                x0, y0, x1, y1 = reg["box"]
                assert 0 <= x0 <= x1 <= w and 0 <= y0 <= y1 <= h and isinstance(reg["caption"], str)


# ------------------------------------------------------------------------------------------------ region embeddings
def test_kept_indices_map_back_to_proposals():
    """fast_rcnn_inference_single_image drops non-finite rows (ref_inference.npz has one); with proposal_indices the kept indices
    are rows of the input, so each detection's score is its own proposal's score for its class"""
    from cddmsl_amd.modeling.roi_heads import fast_rcnn_inference_single_image
    fx = np.load(os.path.join(GOLD, "ref_inference.npz"))
    boxes, scores = torch.from_numpy(fx["boxes"]).to(DEV), torch.from_numpy(fx["scores"]).to(DEV)
    valid = torch.isfinite(boxes).all(1) & torch.isfinite(scores).all(1)
    assert not bool(valid.all())
    inst, kept = fast_rcnn_inference_single_image(boxes, scores, (200, 300), 0.05, 0.5, 20)
    inst2, rows = fast_rcnn_inference_single_image(boxes, scores, (200, 300), 0.05, 0.5, 20, proposal_indices=True)
    assert torch.equal(rows, valid.nonzero()[:, 0][kept]) and torch.equal(inst2.pred_boxes.tensor, inst.pred_boxes.tensor)
    assert torch.equal(inst2.scores, scores[rows, inst2.pred_classes])


def test_inference_with_region_embeddings_matches_inference():
    """the new eval-only entry returns inference()'s detections, and each one's embedding is the attention-pool embedding of the
    proposal it came from"""
    from cddmsl_amd import synthetic
    from cddmsl_amd.config import get_cfg
    from cddmsl_amd.modeling import build_model
    from cddmsl_amd.modeling.postprocessing import detector_postprocess
    cfg = get_cfg()
    cfg.merge_from_file(os.path.join(ROOT, "configs", "VOC-Experiments", "faster_rcnn_CLIP_R_50_C4.yaml"))
    cfg.merge_from_list(["MODEL.DEVICE", DEV, "MODEL.ROI_HEADS.SCORE_THRESH_TEST", 0.0])
    model = build_model(cfg)
    model.load_state_dict(synthetic.make_state_dict(0), strict=False)
    model.eval()
    img = torch.from_numpy(np.random.RandomState(3).randint(0, 256, (3, 160, 224), dtype=np.uint8))
    inp = {"image": img, "height": 240, "width": 336}
    ref = model.inference([inp])[0]["instances"]
    got = model.inference_with_region_embeddings([inp])[0]["instances"]
    assert len(got) >= 1 and len(got) == len(ref)
    assert torch.equal(got.pred_classes, ref.pred_classes)
    assert torch.allclose(got.pred_boxes.tensor, ref.pred_boxes.tensor, rtol=1e-6, atol=1e-4)
    assert torch.allclose(got.scores, ref.scores, rtol=1e-6, atol=1e-7)
    # the same pipeline by hand: the kept proposals' rows of the pooled embeddings, through the same postprocess filter
    rh = model.roi_heads
    with torch.no_grad():
        images, sizes = model.preprocess_image([inp], "image")
        res4 = model.backbone.forward_nhwc(images, want_res5=False)["res4"]
        proposals, _ = model.proposal_generator.forward_nhwc(sizes, res4, None)
        att = rh._pooled_embeddings(res4, [p.proposal_boxes for p in proposals], model.backbone.layer4, model.backbone.attnpool)
        pred = rh.box_predictor(att)
        inst, kept = rh.box_predictor.inference(pred, proposals, proposal_indices=True)
        probs = rh.box_predictor.predict_probs(pred, proposals)[0]
        if rh.box_predictor.multiply_rpn_score:
            probs = (probs * proposals[0].objectness_logits[:, None]) ** 0.5
    assert torch.allclose(inst[0].scores, probs[kept[0], inst[0].pred_classes], rtol=1e-6, atol=1e-7)
    inst[0].region_embeds = att[kept[0]]
    want = detector_postprocess(inst[0], 240, 336)
    assert torch.allclose(got.region_embeds, want.region_embeds, rtol=1e-5, atol=1e-5)
