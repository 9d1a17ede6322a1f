"""CPU: the host side of mapper training -- GPT-2 encoding against ``GPT2Tokenizer`` strings of the golden, the padding and
``max_seq_len`` rules, the warm-up schedule against ``get_linear_schedule_with_warmup``'s stored factors, the dataset file, the
optimizer's state layout -- and the yardstick of tests/test_gpu_clipcap_train.py: in the plainly written training step
(tests/clipcap_train_ref.py) each single dropped term (the causal mask in the backward, the tanh derivative, an ignored row, one
LayerNorm parameter gradient, the bias correction) moves some compared tensor past ten times its limit."""
import os
import sys

import numpy as np
import pytest
import torch

import clipcap_train_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, GOLD)


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLD, "ref_clipcap_train.npz"))


@pytest.fixture(scope="module")
def vocab():
    from cddmsl_amd.gpt2_text import GPT2Vocab
    return GPT2Vocab(os.path.join(GOLD, "gpt2_train_vocab.json"), merges=os.path.join(GOLD, "gpt2_train_merges.txt"))


def test_encode_matches_gpt2_tokenizer(gold, vocab):
    ids, o = gold["enc_ids"].tolist(), 0
    assert len(vocab.ranks) > 20
    for text, n in zip(gold["enc_text"].tolist(), gold["enc_len"].tolist()):
        assert vocab.encode(text) == ids[o:o + n], text
        o += n
    assert o == len(ids)


def test_decode_inverts_encode(gold, vocab):
    for s in gold["enc_text"].tolist() + ["a  b\t\tc ", "ünïcödé ∑ 12 34's", "\n\n x"]:
        assert vocab.decode(vocab.encode(s)) == s


def test_encode_needs_merges():
    from cddmsl_amd.gpt2_text import GPT2Vocab
    v = GPT2Vocab(os.path.join(GOLD, "gpt2_train_vocab.json"))
    assert v.decode([257]) == "the"
    with pytest.raises(ValueError):
        v.encode("the")


def test_padding_and_max_seq_len_rules():
    from cddmsl_amd import clipcap_train as ct
    tok = torch.tensor([[5, 6, -1, -1, -1], [1, 2, 3, 4, 9], [7, 0, 8, -1, -1]])
    assert ct.token_lengths(tok).tolist() == [2, 5, 3]
    assert ct.pad_tokens(tok, 3).tolist() == [[5, 6, 0], [1, 2, 3], [7, 0, 8]]                     # cut; -1 becomes 0; a real 0 stays
    assert ct.pad_tokens(tok, 7).tolist() == [[5, 6, 0, 0, 0, 0, 0], [1, 2, 3, 4, 9, 0, 0], [7, 0, 8, 0, 0, 0, 0]]
    assert (tok < 0).any(), "pad_tokens works on a copy"
    ln = torch.tensor([10, 12, 11, 13, 60])
    want = min(int(ln.float().mean() + ln.float().std() * 10), int(ln.max()))                       # ClipCap's expression
    assert ct.choose_max_seq_len(ln, 40) == want == 60
    assert ct.choose_max_seq_len(torch.tensor([10, 10, 10, 10]), 40) == 10                          # std 0: the mean
    assert ct.choose_max_seq_len(torch.tensor([7]), 40) == 7                                        # one caption: no std
    assert ct.choose_max_seq_len(torch.tensor([100, 120, 140]), 40) == 88                           # prefix + tokens <= 128
    g = torch.Generator().manual_seed(3)
    b = ct.epoch_batches(11, 4, g)
    assert len(b) == 2 and sorted(torch.cat(b).tolist()) == sorted(set(torch.cat(b).tolist())) and all(len(x) == 4 for x in b)


def test_schedule_matches_stored_factors(gold):
    from cddmsl_amd.solver import linear_warmup_schedule
    w, t = gold["sched_warmup_total"].tolist()
    for s, f in zip(gold["sched_steps"].tolist(), gold["sched"].tolist()):
        assert linear_warmup_schedule(s, w, t) == f, s
    assert linear_warmup_schedule(0, 0, 10) == 1.0 and linear_warmup_schedule(3, 5000, 5000) == 3 / 5000


def test_dataset_file_loads_with_weights_only(tmp_path):
    from cddmsl_amd import clipcap_train as ct
    p = str(tmp_path / "d.pt")
    ct.save_dataset(p, torch.randn(2, 8), torch.tensor([0, 1, 1]), [[3, 4], [], [5]], ["a b", "", "c"])
    raw = torch.load(p, weights_only=True)
    assert set(raw) == set(ct.DATASET_KEYS) and raw["captions"] == ["a b", "", "c"]
    d = ct.load_dataset(p)
    assert d["tokens"].tolist() == [[3, 4], [-1, -1], [5, -1]] and d["clip_embedding"].dtype == torch.float32
    torch.save({"tokens": d["tokens"]}, p)
    with pytest.raises(KeyError):
        ct.load_dataset(p)


def test_adamw_state_layout():
    """torch's names, torch.optim's state_dict layout, and a round trip (host tensors: no step is taken)"""
    from cddmsl_amd.solver import AdamW
    ps = [torch.nn.Parameter(torch.randn(3)), torch.nn.Parameter(torch.randn(2, 2))]
    opt = AdamW(ps, lr=2e-5, eps=1e-6, weight_decay=0.0)
    s = opt._state(ps[1])
    assert set(s) == {"step", "exp_avg", "exp_avg_sq"} and s["exp_avg"].shape == (2, 2)
    s["step"], s["exp_avg"] = 4, torch.ones(2, 2)
    sd = opt.state_dict()
    assert list(sd["state"]) == [1] and sd["param_groups"][0]["params"] == [0, 1] and sd["param_groups"][0]["eps"] == 1e-6
    ref = torch.optim.AdamW(ps, lr=2e-5).state_dict()
    assert set(ref) == set(sd) and set(sd["param_groups"][0]) <= set(ref["param_groups"][0])
    opt2 = AdamW(ps)
    opt2.load_state_dict(sd)
    assert opt2.lr == 2e-5 and opt2.state[id(ps[1])]["step"] == 4 and torch.equal(opt2.state[id(ps[1])]["exp_avg"], torch.ones(2, 2))


def test_each_dropped_term_shows(gold):
    """case A in float64 with one term removed, against the limits the GPU test uses (computed the same way) on the tensors it
    compares with them: the loss, d loss / d prefix and the parameter gradients.  Every drop in the gradient chain moves one of them
    past ten times its f32 limit (by 2e4 times and more).  The bf16 limits are 4 x the rounded plain module's own error, 3 to 11 per
    cent on the gradients of this four-layer chain: the causal mask and the ignored row still show ten times over (56 % and 124 %
    against 4.1 % and 4.5 %); the tanh derivative moves 27 % against 4.5 % (6 x) and one LayerNorm gradient 100 % against 10.8 %
    (9 x): those two are held by the f32 run -- gelu_new_bwd and layernorm_bwd_params are the same kernels and nodes in both dtypes --
    and by the kernels' own tests.  The bias correction is held by the GPU test's float64 replay of each update (4e-6 of the largest
    operand): without it the first update is 3.2 times as long."""
    import make_golden_clipcap_train as MG
    from cddmsl_amd.synthetic import make_gpt2_state_dict, make_mapper_state_dict
    c = MG.CASES["A"]
    x, tok = MG.case_inputs("A")
    tokens = tok.clone()
    tokens[tokens < 0] = 0
    msd = make_mapper_state_dict(c["seed"], dim_clip=MG.DIM_CLIP, dim=MG.N_EMBD, length=c["P"], layers=2)
    gsd = make_gpt2_state_dict(0, n_layer=2, n_embd=MG.N_EMBD, vocab=MG.VOCAB, n_positions=MG.N_POS)
    kw = dict(lr=MG.LR, wd=MG.WD, eps=MG.EPS)
    run = lambda **k: R.plain_step(msd, gsd, x, tokens, c["P"], 2, **k, **kw)      # noqa: E731
    ref = run(dtype=R.F64)
    # the plain step IS the reference's: its loss and gradients equal the golden's (the reference's own modules, float32)
    assert abs(float(ref["loss"]) - float(gold["A.loss"])) <= 1e-5 * float(gold["A.loss"])
    assert R.rel_err(ref["dprefix"], torch.from_numpy(gold["A.dprefix"])) <= 1e-4
    e32, ebf = run(dtype=torch.float32), run(dtype=R.F64, rb=True)
    lim = {k: (max(8 * R.rel_err(e32[k], ref[k]), 1e-6), max(4 * R.rel_err(ebf[k], ref[k]), 2.0 ** -8))
           for k in ref if float(ref[k].abs().max()) > 0 and not k.startswith("p")}
    for drop in R.DROPS:
        if drop == "bias_correction":
            g, p = ref["g.linear.bias"], msd["linear.bias"].double()
            ok = R.plain_adamw(p, g, torch.zeros_like(g), torch.zeros_like(g), MG.LR, 0.9, 0.999, MG.EPS, MG.WD, 1)
            bad = R.plain_adamw(p, g, torch.zeros_like(g), torch.zeros_like(g), MG.LR, 0.9, 0.999, MG.EPS, MG.WD, 1, drop=drop)
            assert torch.equal(ok, ref["p1.linear.bias"])
            assert float((bad - ok).abs().max()) > 10 * 4e-6 * max(float(ok.abs().max()), MG.LR)
            continue
        got = run(dtype=R.F64, drop=drop)
        moved = {k: R.rel_err(got[k], ref[k]) for k in lim}
        k32 = max(lim, key=lambda k: moved[k] / lim[k][0])
        kbf = max(lim, key=lambda k: moved[k] / lim[k][1])
        print(f"{drop}: f32 {k32} {moved[k32]:.3e} / {lim[k32][0]:.3e}; bf16 {kbf} {moved[kbf]:.3e} / {lim[kbf][1]:.3e}")
        assert moved[k32] > 10 * lim[k32][0], drop
        assert drop not in ("causal_mask_bwd", "ignored_row") or moved[kbf] > 10 * lim[kbf][1], drop
