"""CPU: the beam-search selection rule.  tests/beam_ref.py's restatement on each beam's B best tokens equals a brute force over all
B x V candidates (so B tokens per beam suffice), and torch_beam with one beam is torch_greedy."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import beam_ref  # noqa: E402

V, T, STEP, STOP = 37, 7, 3, 5


@pytest.mark.parametrize("B", [1, 2, 5, 8])
@pytest.mark.parametrize("stops", ["none", "some", "all"])
def test_top_b_per_beam_equals_brute_force(B, stops):
    rs = np.random.RandomState(100 * B + len(stops))
    n = 6
    stopped = {"none": np.zeros((n, B), bool), "some": rs.rand(n, B) < 0.4, "all": np.ones((n, B), bool)}[stops]
    old = beam_ref.random_state(rs, n, B, T, STEP, stopped, V, STOP)
    # coarse logits: many equal values inside a row and equal keys across beams, so the tie rules are exercised
    logits = (rs.randint(-12, 4, (n * B, V)) * 0.25).astype(np.float32)
    if B > 1 and stops != "all":
        old["sum"][0, 1], old["len"][0, 1], old["stop"][0, :2] = old["sum"][0, 0], old["len"][0, 0], 0
        logits[1] = logits[0]                                            # caption 0: beams 0 and 1 tie in every key
    logZ = np.log(np.exp(logits.astype(np.float64)).sum(1)).astype(np.float32)
    new = beam_ref.empty_state(n, B, T)
    vals, idx = beam_ref.top_b(logits, B)
    got = beam_ref.beam_step_ref(vals, idx, logZ, old, new, STEP, STOP)
    every = np.tile(np.arange(V, dtype=np.int32), (n * B, 1))
    want = beam_ref.beam_step_ref(logits, every, logZ, old, new, STEP, STOP)
    for k in want:
        assert np.array_equal(got[k], want[k]), k
    if stops == "all":
        assert np.array_equal(np.sort(got["src"], 1), np.tile(np.arange(B), (n, 1)))      # every stopped beam survives once
    assert (got["len"] == old["len"][np.arange(n)[:, None], got["src"]] + (1 - old["stop"][np.arange(n)[:, None], got["src"]])).all()


def test_step0_takes_the_rows_pairs_in_order():
    rs = np.random.RandomState(3)
    n, B = 4, 5
    logits = rs.standard_normal((n, V)).astype(np.float32)
    vals, idx = beam_ref.top_b(logits, B)
    logZ = np.log(np.exp(logits.astype(np.float64)).sum(1)).astype(np.float32)
    idx[2, 3] = STOP
    st = beam_ref.beam_step_ref(vals, idx, logZ, beam_ref.empty_state(n, B, T), beam_ref.empty_state(n, B, T), 0, STOP)
    assert np.array_equal(st["hist"][:, :, 0], idx) and (st["hist"][:, :, 1:] == -1).all() and (st["len"] == 1).all()
    assert np.array_equal(st["sum"], vals - logZ[:, None]) and np.array_equal(st["stop"], idx == STOP)
    assert np.array_equal(st["next_tok"].reshape(n, B), idx)


def test_torch_beam_one_beam_is_greedy():
    from cddmsl_amd.modeling.gpt2 import GPT2Decoder, torch_beam, torch_greedy
    from cddmsl_amd.synthetic import make_gpt2_state_dict
    dec = GPT2Decoder.from_state_dict(make_gpt2_state_dict(0, n_layer=2, n_embd=128, vocab=211, n_positions=64), torch.float32)
    p = torch.from_numpy((np.random.RandomState(5).standard_normal((3, 4, 128)) * 0.1).astype(np.float32))
    with torch.no_grad():
        t0, _, _ = torch_greedy(dec, p, max_tokens=9)
        stop = int(t0[0, 2])                                              # sequence 0 stops early, the others may run on
        tg, lg, _ = torch_greedy(dec, p, max_tokens=9, stop_id=stop)
        tb, lb, sc, gaps = torch_beam(dec, p, beam_size=1, max_tokens=9, stop_id=stop)
        t5, l5, s5, _ = torch_beam(dec, p, beam_size=5, max_tokens=9, stop_id=stop)
    assert lg[0] <= 3 and torch.equal(tb[:, 0], tg) and torch.equal(lb[:, 0], lg)
    assert sc.shape == (3, 1) and gaps.shape[0] == 3 and bool((gaps >= 0).all())
    # five beams: sorted by score, -1 past each length
    assert bool((s5[:, :-1] >= s5[:, 1:]).all())
    pos = torch.arange(9).expand(3, 5, 9)
    assert torch.equal(t5 >= 0, pos < l5.unsqueeze(2))
