"""Generates tests/golden/ref_gpt2.npz, tests/golden/gpt2_vocab.json and tests/golden/gpt2_merges.txt with the ``transformers``
package of the build machine (the reference's own GPT-2 class, ``GPT2LMHeadModel``), built offline from a ``GPT2Config`` -- nothing
is fetched.  Weights: ``synthetic.make_gpt2_state_dict(0, n_layer=2, n_embd=768, vocab=4099, n_positions=1024)`` (12 heads), eager
attention, float32.  Prefixes: ``prefixes(seed)`` below, [3, 40, 768].  What travels:

  tokens / margins      the reference loop's greedy tokens (generate2 with its top-p filter, which never removes the arg-max: the full
                        sequence recomputed every step, STEPS steps, no stop token) [3, STEPS] and each step's top-2 logit margin
  logit_steps / logits  the last-row logits at a few steps [3, len(logit_steps), 4099] f32
  dec_ids / dec_len / dec_text   id lists (concatenated, with their lengths) and GPT2Tokenizer.decode of each: ASCII words, multi-byte
                        UTF-8 split across tokens, invalid byte runs
No weights are stored.  GPU tests never import transformers; they read these files.

usage:  python tests/golden/make_golden_gpt2.py
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

N_LAYER, N_EMBD, VOCAB, N_POS, STEPS = 2, 768, 4099, 1024, 24
LOGIT_STEPS = [0, 1, 7, STEPS - 1]


def prefixes(seed=1, n=3, p=40, e=N_EMBD):
    return torch.from_numpy((np.random.RandomState(seed).standard_normal((n, p, e)) * 0.1).astype(np.float32))


def vocab_tokens():
    """4099 entries: the 256 byte symbols, then deterministic multi-symbol tokens (words with and without the space marker 'Ġ', and
    a few UTF-8 pieces split across tokens)"""
    from cddmsl_amd.gpt2_text import byte_table
    bu = byte_table()
    toks = [bu[b] for b in range(256)]
    sym = lambda s: "".join(bu[b] for b in s.encode("utf-8"))                     # noqa: E731
    special = [sym(" café"), sym("é"), bu[0xe2] + bu[0x82], bu[0xac] + sym(" euro"), sym(" naïve"), sym(" 日本"), sym("語")]
    toks += special
    syll = ["ca", "ro", "tu", "mi", "ne", "sa", "lo", "be", "di", "ka", "po", "re", "ti", "va", "zu", "fe"]
    i = 0
    while len(toks) < VOCAB - 1:
        a, b, c = syll[i % 16], syll[(i // 16) % 16], syll[(i // 256) % 16]
        w = a + b + (c if i >= 256 else "")
        for t in (sym(" " + w), sym(w)):
            if t not in toks and len(toks) < VOCAB - 1:
                toks.append(t)
        i += 1
    toks.append("<|endoftext|>")
    assert len(toks) == len(set(toks)) == VOCAB
    return toks


def main():
    from transformers import GPT2Config, GPT2LMHeadModel, GPT2Tokenizer
    from cddmsl_amd.synthetic import make_gpt2_state_dict
    from cddmsl_amd.gpt2_text import byte_table
    torch.manual_seed(0)
    sd = make_gpt2_state_dict(0, n_layer=N_LAYER, n_embd=N_EMBD, vocab=VOCAB, n_positions=N_POS)
    cfg = GPT2Config(vocab_size=VOCAB, n_positions=N_POS, n_embd=N_EMBD, n_layer=N_LAYER, n_head=N_EMBD // 64,
                     activation_function="gelu_new", resid_pdrop=0.0, embd_pdrop=0.0, attn_pdrop=0.0, layer_norm_epsilon=1e-5,
                     bos_token_id=VOCAB - 1, eos_token_id=VOCAB - 1)
    model = GPT2LMHeadModel(cfg)
    model.config._attn_implementation = "eager"
    full = {"transformer." + k: v for k, v in sd.items()}
    full["lm_head.weight"] = sd["wte.weight"]
    missing, unexpected = model.load_state_dict(full, strict=False)
    assert not unexpected and all(k.endswith("attn.bias") or k.endswith("masked_bias") for k in missing), (missing, unexpected)
    model.eval()

    emb = prefixes().double().float()
    toks, margins, logits = [], [], []
    with torch.no_grad():
        for s in range(STEPS):
            lg = model(inputs_embeds=emb).logits[:, -1, :].float()
            top = lg.topk(2, dim=1).values
            t = lg.argmax(dim=1)
            toks.append(t)
            margins.append(top[:, 0] - top[:, 1])
            if s in LOGIT_STEPS:
                logits.append(lg)
            emb = torch.cat([emb, model.transformer.wte(t).unsqueeze(1)], dim=1)

    # vocabulary + tokenizer decode cases
    vt = vocab_tokens()
    vpath, mpath = os.path.join(HERE, "gpt2_vocab.json"), os.path.join(HERE, "gpt2_merges.txt")
    with open(vpath, "w", encoding="utf-8") as f:
        json.dump({t: i for i, t in enumerate(vt)}, f, ensure_ascii=False)
    with open(mpath, "w", encoding="utf-8") as f:
        f.write("#version: 0.2\n")                                     # decoding applies no merges
    tok = GPT2Tokenizer(vpath, mpath)
    bu = byte_table()
    idx = {t: i for i, t in enumerate(vt)}
    cases = [
        [idx["Ġcaro"], idx["Ġtumi"], ord(".")],                                   # words and the stop token
        [idx[bu[ord("A")]], 256, 257],                                            # " café", "é"
        [258, 259],                                                               # "€" split across two tokens, then " euro"
        [258, idx[bu[ord("x")]]],                                                 # a truncated 3-byte sequence, then ASCII
        [0xff, 0xfe, idx[bu[ord("a")]]],                                          # invalid bytes
        [260, 261, 262, VOCAB - 1],                                               # " naïve", " 日本", "語", <|endoftext|>
        [0xe6, 0x97, ord("!")],                                                   # an incomplete 3-byte sequence
        [idx[bu[ord("H")]], idx[bu[ord("i")]], idx[bu[ord(" ")]], idx["roca"], idx["Ġroca"]],
    ]
    texts = [tok.decode(c) for c in cases]
    np.savez_compressed(os.path.join(HERE, "ref_gpt2.npz"), tokens=torch.stack(toks, 1).numpy().astype(np.int64),
                        margins=torch.stack(margins, 1).numpy().astype(np.float32), logit_steps=np.array(LOGIT_STEPS, np.int64),
                        logits=torch.stack(logits, 1).numpy().astype(np.float32),
                        dec_ids=np.array([i for c in cases for i in c], np.int64), dec_len=np.array([len(c) for c in cases], np.int64),
                        dec_text=np.array(texts))
    print("tokens", torch.stack(toks, 1).tolist())
    print("min margin", float(torch.stack(margins).min()), "texts", texts)


if __name__ == "__main__":
    main()
