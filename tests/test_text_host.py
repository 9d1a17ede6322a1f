"""CPU: the CLIP tokenizer / prompt engineering (cddmsl_amd/clip_text.py) against the reference's own ids, the text encoder's
state-dict names and checkpoint layouts, the truncation argument in float64, and the concept tool's refusal to run off-GPU."""
import gzip
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GOLD = os.path.join(ROOT, "tests", "golden", "ref_text_encoder.npz")


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD, allow_pickle=False)


def pruned_tokenizer(z):
    from cddmsl_amd.clip_text import BPETokenizer
    ranks = {(a, b): int(r) for a, b, r in zip(z["merge_a"], z["merge_b"], z["merge_rank"])}
    vocab = {str(t): int(i) for t, i in zip(z["vocab_tok"], z["vocab_id"])}
    return BPETokenizer.from_tables(ranks, vocab)


def classes_of(z):
    return [n.split("|") if "|" in n else str(n) for n in z["names"]]


def test_tokenizer_reproduces_reference_ids(gold):
    from cddmsl_amd.clip_text import concept_prompts, tokenize_prompts
    bpe = pruned_tokenizer(gold)
    templates = [str(t) for t in gold["templates"]]
    assert bpe.sot == 49406 and bpe.eot == 49407
    for c, name in enumerate(classes_of(gold)):
        P = int(gold["nprompt"][c])
        got = tokenize_prompts(concept_prompts(name, templates), bpe)
        want = torch.from_numpy(gold["ids"][c, :P].astype(np.int64))
        assert torch.equal(got, want), (name, (got != want).nonzero()[:5])
    # the 77-token cut: the long name's prompts fill every position, most without their EOT
    last = gold["ids"][-1].astype(np.int64)
    assert (last[:, -1] != 0).sum() >= 40 and (last[:, -1] == 49407).sum() < (last[:, -1] != 0).sum()


def test_tokenize_concepts_shape_and_synonyms(gold):
    from cddmsl_amd.clip_text import tokenize_concepts
    bpe = pruned_tokenizer(gold)
    templates = [str(t) for t in gold["templates"]][:4]
    ids = tokenize_concepts(["person", "car"], templates, bpe)
    assert ids.shape == (2, 4, 77) and ids.dtype == torch.int64
    syn = tokenize_concepts([["sofa", "couch"]], templates, bpe)
    assert syn.shape == (1, 8, 77)
    assert torch.equal(syn[0, :4], tokenize_concepts(["sofa"], templates, bpe)[0])
    assert torch.equal(syn[0, 4:], tokenize_concepts(["couch"], templates, bpe)[0])
    with pytest.raises(ValueError):
        tokenize_concepts(["car", ["sofa", "couch"]], templates, bpe)


def test_prompt_engineering():
    from cddmsl_amd.clip_text import concept_prompts, prompt_engineering
    assert prompt_engineering("a+b,c", "a photo of a {}.") == "a photo of a a bc."
    assert prompt_engineering("traffic light", "{} in a video game.") == "traffic light in a video game."
    assert concept_prompts(["x", "y"], ["{}.", "a {}"]) == ["x.", "a x", "y.", "a y"]
    assert concept_prompts("x", ["{}!"]) == ["x!"]


def test_from_vocab_file_id_layout(tmp_path):
    from cddmsl_amd.clip_text import EOT, SOT, BPETokenizer, byte_symbols, token_order
    merges = ["h e", "l l", "he ll", "o</w>", "hell o</w>", "w o", "wo r", "l d</w>"]
    p = tmp_path / "toy.txt.gz"
    with gzip.open(p, "wt", encoding="utf-8") as f:
        f.write("#version: 0.2\n" + "\n".join(merges) + "\n")
    bpe = BPETokenizer.from_vocab_file(str(p))
    sym = byte_symbols()
    order = token_order()
    assert len(order) == 512 and len(set(order)) == 512 and len(set(sym)) == 256
    assert order[0] == "!" and order[93] == "~" and order[188] == sym[0] and order[256] == "!</w>"   # printable first, then the shifted bytes
    assert sym[ord(" ")] == "Ġ" and sym[ord("a")] == "a"
    for i, m in enumerate(merges):
        assert bpe.vocab[m.replace(" ", "")] == 512 + i and bpe.ranks[tuple(m.split())] == i
    assert bpe.vocab[SOT] == 512 + len(merges) and bpe.vocab[EOT] == 513 + len(merges)
    ids = bpe.encode("Hello  WORLD")
    assert ids == [bpe.vocab["hello</w>"], bpe.vocab["wor"], bpe.vocab["ld</w>"]]
    padded = bpe.encode_padded("hello", context_length=5)
    assert padded == [bpe.sot, bpe.vocab["hello</w>"], bpe.eot, 0, 0]
    assert bpe.encode_padded("hello world hello", context_length=3) == [bpe.sot, bpe.vocab["hello</w>"], bpe.vocab["wor"]]


def _small_state(seed=3, width=128, layers=2, embed_dim=96, vocab=600, ctx=77):
    from cddmsl_amd import synthetic
    return synthetic.make_text_state_dict(seed, width=width, layers=layers, embed_dim=embed_dim, vocab_size=vocab, context_length=ctx)


def test_state_dict_names_and_checkpoint_layouts():
    from cddmsl_amd import synthetic
    from cddmsl_amd.modeling.text_encoder import CLIPTextEncoder
    full = synthetic.make_text_state_dict(0)
    enc = CLIPTextEncoder.from_state_dict(full)
    assert set(enc.state_dict()) == set(full)
    assert "transformer.resblocks.11.attn.out_proj.weight" in full and "transformer.resblocks.0.mlp.c_fc.bias" in full
    assert (enc.width, enc.heads, len(enc.transformer.resblocks), enc.text_projection.shape[1]) == (512, 8, 12, 1024)
    sd = _small_state()
    # RegionCLIP layout: lang_encoder.* next to the detector's tensors
    rc = {"lang_encoder." + k: v for k, v in sd.items()}
    rc["backbone.attnpool.positional_embedding"] = torch.zeros(50, 256)
    rc["roi_heads.box_predictor.cls_score.weight"] = torch.zeros(20, 96)
    # OpenAI layout: top level, next to visual.*
    oai = dict(sd)
    oai["visual.attnpool.positional_embedding"] = torch.zeros(50, 256)
    oai["logit_scale"] = torch.zeros(())
    for ck in (rc, oai):
        e = CLIPTextEncoder.from_checkpoint(ck)
        assert (e.width, e.heads, len(e.transformer.resblocks)) == (128, 2, 2)
        for k, v in e.state_dict().items():
            assert torch.equal(v, sd[k]), k
    assert CLIPTextEncoder.from_checkpoint(rc).matched["lang_encoder.positional_embedding"] == "lang_encoder.positional_embedding"
    assert CLIPTextEncoder.from_checkpoint(oai).matched["lang_encoder.positional_embedding"] == "positional_embedding"
    broken = dict(oai)
    broken.pop("transformer.resblocks.1.mlp.c_proj.bias")
    with pytest.raises(KeyError):
        CLIPTextEncoder.from_checkpoint(broken)
    with pytest.raises(KeyError):
        CLIPTextEncoder.from_checkpoint({"backbone.conv1.weight": torch.zeros(1)})
    # RN50x4 geometry: 640 wide, 10 heads, 640 out
    g = CLIPTextEncoder.geometry(synthetic.make_text_state_dict(1, width=640, layers=1, embed_dim=640, vocab_size=50))
    assert g == dict(width=640, layers=1, embed_dim=640, vocab_size=50, context_length=77)


def test_truncation_is_exact_in_float64(gold):
    """encoding at T = 77 and at T = max(eot) + 1 gives the same EOT features (causal mask: no row <= EOT reads a later row)"""
    from cddmsl_amd.modeling.text_encoder import CLIPTextEncoder, torch_encode_text
    enc = CLIPTextEncoder.from_state_dict(_small_state(vocab=49408))
    ids = torch.from_numpy(gold["enc_ids"])
    short = torch_encode_text(enc, ids, torch.float64, truncate=True)
    full = torch_encode_text(enc, ids, torch.float64, truncate=False)
    assert torch.allclose(short, full, rtol=1e-12, atol=1e-12), (short - full).abs().max()
    sub = ids[:4]                               # a batch whose longest prompt is short: T << 77
    t = int(sub.argmax(-1).max()) + 1
    assert t < 30
    assert torch.allclose(torch_encode_text(enc, sub, torch.float64), full[:4], rtol=1e-12, atol=1e-12)


def test_encoder_refuses_cpu_tensors():
    from cddmsl_amd._lib import HipLibraryError
    from cddmsl_amd.modeling.text_encoder import CLIPTextEncoder
    enc = CLIPTextEncoder.from_state_dict(_small_state())
    with pytest.raises(HipLibraryError):
        enc.encode_text(torch.tensor([[49406 % 600, 5, 599, 0]]))


def test_tool_fails_loudly_without_gpu(tmp_path):
    (tmp_path / "in").mkdir()
    (tmp_path / "in" / "concepts.txt").write_text("car\nperson\n")
    (tmp_path / "t.txt").write_text("a photo of a {}.\n")
    with gzip.open(tmp_path / "v.gz", "wt") as f:
        f.write("#version\nc a\n")
    cmd = [sys.executable, os.path.join(ROOT, "tools", "extract_concept_features.py"), "--config-file",
           os.path.join(ROOT, "configs", "VOC-Experiments", "faster_rcnn_CLIP_R_50_C4.yaml"), "--bpe-vocab", str(tmp_path / "v.gz"),
           "--templates", str(tmp_path / "t.txt"), "--synthetic-weights", "0", "MODEL.DEVICE", "cpu",
           "INPUT_DIR", str(tmp_path / "in"), "OUTPUT_DIR", str(tmp_path / "out")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode != 0
    assert "MI355X" in r.stderr and "no CPU path" in r.stderr
    assert not (tmp_path / "out" / "concept_embeds.pth").exists()


def test_torch_restatement_matches_reference_fixture(gold):
    """the torch yardstick (used by the GPU tests' float64 checks and the bench tool) is the reference's encode_text"""
    from cddmsl_amd import synthetic
    from cddmsl_amd.modeling.text_encoder import CLIPTextEncoder, torch_encode_text
    enc = CLIPTextEncoder.from_state_dict(synthetic.make_text_state_dict(0))
    got = torch_encode_text(enc, torch.from_numpy(gold["enc_ids"]), torch.float64).float()
    want = torch.from_numpy(gold["enc_out"])
    assert float((got - want).abs().max() / want.abs().max()) < 1e-4
