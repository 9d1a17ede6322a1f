"""CPU: GPT-2 token decoding against GPT2Tokenizer (tests/golden/ref_gpt2.npz), GPT2Decoder state-dict loading (ClipCap /
transformers / bare layouts, Conv1D transpose, tied head, errors naming the bad keys), the f32 restatement against the reference's
GPT2LMHeadModel logits, the greedy control logic, and tools/gen_captions.py's argument errors."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GOLD = os.path.join(ROOT, "tests", "golden")

from cddmsl_amd.gpt2_text import GPT2Vocab  # noqa: E402
from cddmsl_amd.modeling.gpt2 import GPT2Decoder, finish_tokens, torch_gpt2_logits  # noqa: E402
from cddmsl_amd.synthetic import make_gpt2_state_dict  # noqa: E402

VOCAB = 4099


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLD, "ref_gpt2.npz"), allow_pickle=False)


@pytest.fixture(scope="module")
def small_sd():
    return make_gpt2_state_dict(0, n_layer=2, n_embd=128, vocab=203, n_positions=64)


def prefixes(seed=1, n=3, p=40, e=768):
    return torch.from_numpy((np.random.RandomState(seed).standard_normal((n, p, e)) * 0.1).astype(np.float32))


def test_tokenizer_decode_matches_gpt2tokenizer(gold):
    voc = GPT2Vocab(os.path.join(GOLD, "gpt2_vocab.json"))
    assert len(voc) == VOCAB and voc.token_id(".") == ord(".")      # the fixture lists the byte symbols by byte value
    ids, lens, texts = gold["dec_ids"], gold["dec_len"], gold["dec_text"]
    o = 0
    for n, want in zip(lens, texts):
        assert voc.decode(ids[o:o + n].tolist()) == str(want)
        o += n
    with pytest.raises(KeyError):
        voc.token_id("no such token")


@pytest.mark.parametrize("layout", ["clipcap", "transformers", "bare"])
def test_load_layouts_and_transpose(small_sd, layout):
    if layout == "clipcap":
        st = {"gpt.transformer." + k: v for k, v in small_sd.items()}
        st["gpt.lm_head.weight"] = small_sd["wte.weight"].clone()
        st["clip_project.linear.weight"] = torch.zeros(3, 3)                        # the mapper's entries are skipped
        st["gpt.transformer.h.0.attn.bias"] = torch.ones(1, 1, 64, 64)              # an old causal-mask buffer is tolerated
    elif layout == "transformers":
        st = {"transformer." + k: v for k, v in small_sd.items()}
        st["lm_head.weight"] = small_sd["wte.weight"]
    else:
        st = dict(small_sd)
    dec = GPT2Decoder.from_state_dict(st, torch.float32)
    assert (len(dec.h), dec.n_embd, dec.heads, dec.vocab_size, dec.n_positions) == (2, 128, 2, 203, 64)
    assert torch.equal(dec.h[1].attn.c_attn.weight, small_sd["h.1.attn.c_attn.weight"].t())
    assert torch.equal(dec.h[0].mlp.c_proj.weight, small_sd["h.0.mlp.c_proj.weight"].t())
    assert torch.equal(dec.wte.weight, small_sd["wte.weight"])


def test_load_errors_name_the_keys(small_sd):
    st = dict(small_sd)
    del st["h.1.mlp.c_fc.bias"]
    st["h.0.attn.extra"] = torch.zeros(1)
    with pytest.raises(KeyError, match=r"h\.1\.mlp\.c_fc\.bias.*h\.0\.attn\.extra"):
        GPT2Decoder.from_state_dict(st, torch.float32)
    st = {"gpt.transformer." + k: v for k, v in small_sd.items()}
    st["gpt.lm_head.weight"] = small_sd["wte.weight"] + 1
    with pytest.raises(ValueError, match="tied"):
        GPT2Decoder.from_state_dict(st, torch.float32)
    st = dict(small_sd)
    st["h.0.attn.c_proj.weight"] = torch.zeros(128, 64)
    with pytest.raises(ValueError, match=r"h\.0\.attn\.c_proj\.weight"):
        GPT2Decoder.from_state_dict(st, torch.float32)
    with pytest.raises(KeyError, match="no GPT-2 weights"):
        GPT2Decoder.from_state_dict({"clip_project.linear.weight": torch.zeros(1)}, torch.float32)


def test_torch_restatement_matches_reference_logits(gold):
    dec = GPT2Decoder.from_state_dict(make_gpt2_state_dict(0, n_layer=2, n_embd=768, vocab=VOCAB, n_positions=1024), torch.float32)
    toks = torch.from_numpy(gold["tokens"])
    emb = torch.cat([prefixes(), dec.wte.weight[toks[:, :-1]]], dim=1)
    with torch.no_grad():
        lg = torch_gpt2_logits(dec, emb)
    for i, s in enumerate(gold["logit_steps"].tolist()):
        got = lg[:, 40 - 1 + s]
        ref = torch.from_numpy(gold["logits"][:, i])
        assert ((got - ref).abs() / (1 + ref.abs())).max().item() <= 1e-5       # f32 rounding of logits up to ~10
    # and its greedy tokens are the recorded ones
    assert torch.equal(lg[:, 39:].argmax(-1), toks)


def test_finish_tokens_stop_and_max_tokens():
    t = torch.tensor([[5, 7, 1, 9, 1], [1, 4, 4, 4, 4], [3, 3, 3, 3, 3], [2, 8, -1, -1, -1]])
    out, lens = finish_tokens(t, stop_id=1)
    assert lens.tolist() == [3, 1, 5, 2]                       # the stop token is kept; no stop -> max_tokens; unrun steps
    assert out.tolist() == [[5, 7, 1, -1, -1], [1, -1, -1, -1, -1], [3, 3, 3, 3, 3], [2, 8, -1, -1, -1]]
    out, lens = finish_tokens(t, stop_id=None)
    assert lens.tolist() == [5, 5, 5, 2] and torch.equal(out[:3], t[:3])


def test_gen_captions_argument_errors(tmp_path):
    tool = os.path.join(ROOT, "tools", "gen_captions.py")
    cfg = os.path.join(ROOT, "configs", "VOC-Experiments", "faster_rcnn_CLIP_R_50_C4.yaml")
    env = dict(os.environ, PYTHONPATH=ROOT)

    def run(*a):
        return subprocess.run([sys.executable, tool, "--config-file", cfg, *a], capture_output=True, text=True, env=env, timeout=120)

    r = run("MODEL.WEIGHTS", "x", "INPUT_DIR", str(tmp_path), "OUTPUT_DIR", str(tmp_path))
    assert r.returncode != 0 and "--gpt2-vocab" in r.stderr
    r = run("--gpt2-vocab", str(tmp_path / "missing.json"), "MODEL.WEIGHTS", "x", "INPUT_DIR", str(tmp_path), "OUTPUT_DIR", str(tmp_path))
    assert r.returncode != 0 and "missing.json" in r.stderr
    voc = os.path.join(GOLD, "gpt2_vocab.json")
    r = run("--gpt2-vocab", voc, "MODEL.WEIGHTS", str(tmp_path / "nock.pth"), "MODEL.VISION_TO_LANG_PATH", str(tmp_path / "cc.pt"),
            "INPUT_DIR", str(tmp_path), "OUTPUT_DIR", str(tmp_path))
    assert r.returncode != 0 and "nock.pth" in r.stderr
    open(tmp_path / "w.pth", "wb").close()
    r = run("--gpt2-vocab", voc, "MODEL.WEIGHTS", str(tmp_path / "w.pth"), "MODEL.VISION_TO_LANG_PATH", str(tmp_path / "cc.pt"),
            "INPUT_DIR", str(tmp_path), "OUTPUT_DIR", str(tmp_path))
    assert r.returncode != 0 and "cc.pt" in r.stderr
    r = run("--gpt2-vocab", voc, "--gpt2-weights", str(tmp_path / "g.pt"), "MODEL.WEIGHTS", str(tmp_path / "w.pth"),
            "MODEL.VISION_TO_LANG_PATH", str(tmp_path / "w.pth"), "INPUT_DIR", str(tmp_path), "OUTPUT_DIR", str(tmp_path))
    assert r.returncode != 0 and "g.pt" in r.stderr


def test_c_abi_rejects_out_of_contract_arguments():
    """the new entries return CDDMSL_ERR_ARG (1) before launching anything: no GPU needed"""
    import ctypes
    import __graft_entry__ as g
    g.build()
    from cddmsl_amd import hip
    L = hip._L()
    p = ctypes.c_void_p(256)                 # aligned, never dereferenced: the checks return first
    # token rows without a table
    assert L.cddmsl_pos_embed(p, 1, None, None, p, p, 4, 1, 0, 8, 10, 4, 0, None) == 1
    # neither ids nor src / both / position past n_positions
    assert L.cddmsl_pos_embed(None, 1, None, None, p, p, 4, 1, 0, 8, 10, 4, 0, None) == 1
    assert L.cddmsl_pos_embed(p, 1, p, p, p, p, 4, 1, 0, 8, 10, 4, 0, None) == 1
    assert L.cddmsl_pos_embed(p, 1, p, None, p, p, 4, 1, 4, 8, 10, 4, 0, None) == 1
    # skinny GEMM: M above 64, N not a multiple of 8, K not a multiple of 64, too small a workspace
    ws = hip.skinny_gemm_workspace(4, 64, 128)
    assert ws > 0 and hip.skinny_gemm_workspace(65, 64, 128) == -1 and hip.skinny_gemm_workspace(4, 64, 96) == -1
    assert L.cddmsl_skinny_gemm(p, p, None, None, p, p, ws, 65, 64, 128, 0, None) == 1
    assert L.cddmsl_skinny_gemm(p, p, None, None, p, p, ws, 4, 60, 128, 0, None) == 1
    assert L.cddmsl_skinny_gemm(p, p, None, None, p, p, ws - 4, 4, 64, 128, 0, None) == 1
    assert L.cddmsl_skinny_gemm(p, p, None, p, p, p, ws, 4, 64, 128, 0, None) == 1          # residual needs the f32 epilogue
    # LM head: too small a workspace; decode attention: L beyond the cache
    assert L.cddmsl_lm_head_argmax(p, p, p, 1, None, p, 8, 4, 100, 64, None) == 1
    assert L.cddmsl_decode_attn(p, p, p, p, 2, 12, 64, 41, 40, 2304, ctypes.c_float(0.125), 0, None) == 1
