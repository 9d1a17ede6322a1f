"""Generates tests/golden/ref_clipcap_train.npz, tests/golden/gpt2_train_vocab.json and tests/golden/gpt2_train_merges.txt: ClipCap's
mapper-training step (clipcap.py ``ClipCaptionModel.forward`` + ``train``, ``--only_prefix``) on the build machine, offline.

The mapper is the reference's own ``TransformerMapper`` (its clipcap.py imported as make_golden.py imports it: ``clip`` stubbed, and
``transformers.AdamW``, which newer transformers no longer have, stubbed with torch's); GPT-2 is ``GPT2LMHeadModel(GPT2Config(...))``
with ``synthetic.make_gpt2_state_dict``.  ``ClipCaptionModel`` itself is never constructed (it calls ``from_pretrained``); the few
lines of ``step_loss`` below compose its forward and the loss of ``train``.  No weights are stored.  Per case (A: dim_clip 64,
P = clip_length = 4, 2 + 2 layers, n = 3, caption lengths 1 / 5 / 7 with a token 0 inside one; B: P = 40, L = 40, n = 2):

  <c>.loss, <c>.dprefix                      the loss and d loss / d prefix [n, P, 768]
  <c>.names                                  the mapper's parameter names
  <c>.gnorm [np], <c>.gsample [np, 64]       per parameter: the gradient's L2 norm and its entries at <c>.index [np, 64] (seeded)
  <c>.p0 / .p1 / .p2 [np, 64]                the same entries of the parameters before and after one / two torch.optim.AdamW steps
                                             (lr LR, eps 1e-6, weight decay WD; the second step on the same batch)
  sched_steps / sched (warm-up 10 of 100)    get_linear_schedule_with_warmup's factors
  enc_text / enc_ids / enc_len               strings and GPT2Tokenizer.encode of each, on the small vocabulary / merges written alongside

usage:  python tests/golden/make_golden_clipcap_train.py
"""
import importlib
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

N_EMBD, VOCAB, N_POS, DIM_CLIP = 768, 4099, 1024, 64
LR, WD, EPS = 1e-3, 0.01, 1e-6
SCHED_WARMUP, SCHED_TOTAL, SCHED_STEPS = 10, 100, [0, 1, 5, 9, 10, 11, 55, 99, 100, 130]
CASES = {"A": dict(P=4, lengths=(1, 5, 7), zero_at=(2, 3), seed=31), "B": dict(P=40, lengths=(40, 40), zero_at=(1, 17), seed=32)}

MERGES = [("t", "h"), ("th", "e"), ("Ġ", "the"), ("a", "t"), ("Ġ", "c"), ("Ġc", "at"), ("Ġ", "s"), ("Ġs", "at"), ("o", "n"), ("Ġ", "on"),
          ("Ġ", "m"), ("Ġm", "at"), ("'", "s"), ("1", "2"), ("12", "3"), ("Ġ", "Ġ"), ("!", "!"), ("Ã", "©"), ("c", "a"), ("ca", "f"),
          ("caf", "Ã©"), ("Ġ", "w"), ("Ġw", "e"), ("'", "re"), ("r", "e"), ("l", "l"), ("'", "ll"), ("i", "t")]
ENC_TEXTS = ["the cat sat on the mat", "The cat's 123 cats!!", " leading  double   spaces ", "café naïve 日本語", "it's we're they'll",
             "tab\tnew\nline  end", "", "!!!!! 123123 '", "On the the  the\n\nthe"]


def case_inputs(name):
    """(clip embedding [n, 64] f32, tokens [n, L] int64 padded with -1): seeded, one token 0 inside caption ``zero_at[0]``"""
    c = CASES[name]
    rs = np.random.RandomState(c["seed"])
    n, L = len(c["lengths"]), max(c["lengths"])
    x = torch.from_numpy(rs.standard_normal((n, DIM_CLIP)).astype(np.float32))
    tok = np.full((n, L), -1, np.int64)
    for i, ln in enumerate(c["lengths"]):
        tok[i, :ln] = rs.randint(1, VOCAB, ln)
    tok[c["zero_at"][0] % n, c["zero_at"][1]] = 0
    assert tok[c["zero_at"][0] % n, c["zero_at"][1] + 1] > 0, "the token 0 stands INSIDE a caption"
    return x, torch.from_numpy(tok)


def sample_index(numels, seed=7):
    rs = np.random.RandomState(seed)
    return np.stack([rs.randint(0, n, 64) for n in numels]).astype(np.int64)


def reference_mapper_class():
    """the reference's clipcap.py, package ``__init__``s bypassed, ``clip`` stubbed, ``transformers.AdamW`` stubbed (removed upstream)"""
    import make_golden as mg
    import transformers
    if not hasattr(transformers, "AdamW"):
        transformers.AdamW = torch.optim.AdamW
    mg._StubFinder.ROOTS = tuple(r for r in mg._StubFinder.ROOTS if r != "transformers")
    sys.meta_path.insert(0, mg._StubFinder())
    mg._pkg("detectron2", "detectron2")
    mg._pkg("detectron2.modeling", "detectron2/modeling")
    mg._pkg("detectron2.modeling.backbone", "detectron2/modeling/backbone")
    mg._pkg("detectron2.modeling.backbone.clipcap", "detectron2/modeling/backbone/clipcap")
    return importlib.import_module("detectron2.modeling.backbone.clipcap.clipcap").TransformerMapper


def step_loss(mapper, gpt, x, tokens_m1, P):
    """ClipCaptionModel.forward + the loss of train(): tokens padded with -1 -> (loss, prefix [n, P, E] with its grad retained)"""
    mask = tokens_m1.ge(0)                                      # pad_captions: zero where we are out of the sequence
    tokens = tokens_m1.clone()
    tokens[~mask] = 0
    mask = torch.cat((torch.ones(tokens.shape[0], P), mask.float()), dim=1)
    prefix = mapper(x).view(-1, P, N_EMBD)
    prefix.retain_grad()
    cat = torch.cat((prefix, gpt.transformer.wte(tokens)), dim=1)
    logits = gpt(inputs_embeds=cat, attention_mask=mask).logits[:, P - 1:-1]
    loss = torch.nn.functional.cross_entropy(logits.reshape(-1, logits.shape[-1]), tokens.flatten(), ignore_index=0)
    return loss, prefix


def main():
    from transformers import GPT2Config, GPT2LMHeadModel, GPT2Tokenizer, get_linear_schedule_with_warmup
    from cddmsl_amd.gpt2_text import byte_table
    from cddmsl_amd.synthetic import make_gpt2_state_dict, make_mapper_state_dict
    Mapper = reference_mapper_class()
    torch.manual_seed(0)
    sd = make_gpt2_state_dict(0, n_layer=2, n_embd=N_EMBD, vocab=VOCAB, n_positions=N_POS)
    cfg = GPT2Config(vocab_size=VOCAB, n_positions=N_POS, n_embd=N_EMBD, n_layer=2, n_head=N_EMBD // 64, activation_function="gelu_new",
                     resid_pdrop=0.0, embd_pdrop=0.0, attn_pdrop=0.0, layer_norm_epsilon=1e-5, bos_token_id=VOCAB - 1, eos_token_id=VOCAB - 1)
    gpt = GPT2LMHeadModel(cfg)
    gpt.config._attn_implementation = "eager"
    full = {"transformer." + k: v for k, v in sd.items()}
    full["lm_head.weight"] = sd["wte.weight"]
    missing, unexpected = gpt.load_state_dict(full, strict=False)
    assert not unexpected and all(k.endswith("attn.bias") or k.endswith("masked_bias") for k in missing), (missing, unexpected)
    gpt.eval()
    for p in gpt.parameters():
        p.requires_grad = False

    out = {}
    for name, c in CASES.items():
        P = c["P"]
        mapper = Mapper(DIM_CLIP, N_EMBD, P, P, 2)
        mapper.load_state_dict(make_mapper_state_dict(c["seed"], dim_clip=DIM_CLIP, dim=N_EMBD, length=P, layers=2), strict=True)
        mapper.train()
        x, tok = case_inputs(name)
        params = list(mapper.named_parameters())
        index = sample_index([p.numel() for _, p in params])
        take = lambda ts: np.stack([t.detach().reshape(-1)[torch.from_numpy(ix)].numpy() for t, ix in zip(ts, index)])   # noqa: E731
        opt = torch.optim.AdamW(mapper.parameters(), lr=LR, eps=EPS, weight_decay=WD)
        p0 = take([p for _, p in params])
        loss, prefix = step_loss(mapper, gpt, x, tok, P)
        loss.backward()
        out.update({f"{name}.loss": np.float64(loss.item()), f"{name}.dprefix": prefix.grad.numpy().copy(),
                    f"{name}.names": np.array([n for n, _ in params]), f"{name}.index": index,
                    f"{name}.gnorm": np.array([float(p.grad.double().norm()) for _, p in params]),
                    f"{name}.gsample": take([p.grad for _, p in params]), f"{name}.p0": p0})
        opt.step()
        out[f"{name}.p1"] = take([p for _, p in params])
        opt.zero_grad()
        loss2, _ = step_loss(mapper, gpt, x, tok, P)
        loss2.backward()
        opt.step()
        out[f"{name}.p2"] = take([p for _, p in params])
        out[f"{name}.loss2"] = np.float64(loss2.item())
        print(name, "loss", loss.item(), "->", loss2.item(), "|dprefix|", float(prefix.grad.norm()))

    dummy = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=1.0)
    sch = get_linear_schedule_with_warmup(dummy, num_warmup_steps=SCHED_WARMUP, num_training_steps=SCHED_TOTAL)
    out["sched_steps"] = np.array(SCHED_STEPS, np.int64)
    out["sched"] = np.array([sch.lr_lambdas[0](s) for s in SCHED_STEPS], np.float64)
    out["sched_warmup_total"] = np.array([SCHED_WARMUP, SCHED_TOTAL], np.int64)

    # a small vocabulary WITH merges for the encoder: the byte symbols, every merge's result, <|endoftext|>
    bu = byte_table()
    toks = [bu[b] for b in range(256)]
    for a, b in MERGES:
        if a + b not in toks:
            toks.append(a + b)
    toks.append("<|endoftext|>")
    vpath, mpath = os.path.join(HERE, "gpt2_train_vocab.json"), os.path.join(HERE, "gpt2_train_merges.txt")
    with open(vpath, "w", encoding="utf-8") as f:
        json.dump({t: i for i, t in enumerate(toks)}, f, ensure_ascii=False)
    with open(mpath, "w", encoding="utf-8") as f:
        f.write("#version: 0.2\n" + "".join(f"{a} {b}\n" for a, b in MERGES))
    tk = GPT2Tokenizer(vpath, mpath)
    ids = [tk.encode(s) for s in ENC_TEXTS]
    assert all(tk.decode(i) == s for i, s in zip(ids, ENC_TEXTS))
    out["enc_text"] = np.array(ENC_TEXTS)
    out["enc_ids"] = np.array([i for c in ids for i in c], np.int64)
    out["enc_len"] = np.array([len(c) for c in ids], np.int64)
    np.savez_compressed(os.path.join(HERE, "ref_clipcap_train.npz"), **out)
    print("encodings", ids)


if __name__ == "__main__":
    main()
