"""Host check of the text / caption checker (tests/exact_text.py, tests/text_exact_cases.py; no GPU): the case tables cover every
named class, the float32 emulations of attn_causal, text_pool and the activations stay under the derived bounds against the float64
references (worst err / bound printed), and the text_pool bound rejects its mutants.

Worst ratios of the unmutated emulations, as printed: attn_causal 0.63, text_pool f32 0.15 and bf16 1.00 (a correctly rounded store
half an ulp off), quick_gelu 0.23 / gelu_new 0.19 in f32 and 1.00 in bf16 (again the single rounding of the store)."""
import pytest
import torch

import exact_text as E
import text_exact_cases as C


def test_case_tables_cover_every_class():
    C.check_skinny_table()
    C.check_decode_table()
    C.check_attn_table()
    C.check_small_tables()


def test_skinny_wave_loops_as_listed():
    assert C.wave_loop(1) == [(0, 1), (0, 0), (0, 0), (0, 0)]
    assert C.wave_loop(5) == [(1, 0), (0, 1), (0, 1), (0, 1)]
    assert C.wave_loop(9) == [(1, 1), (1, 0), (1, 0), (1, 0)]
    assert C.wave_loop(13) == [(2, 0), (1, 1), (1, 1), (1, 1)]
    assert C.wave_loop(16) == [(2, 0)] * 4
    assert C.wave_loop(17) == [(2, 1), (2, 0), (2, 0), (2, 0)]
    for n in range(1, 40):                                              # every chunk is summed once
        assert sum(2 * p + t for p, t in C.wave_loop(n)) == n
    assert C.skinny_splits(768, 3072) == 11 and sorted(set(C.chunks_per_split(768, 3072))) == [4, 5]
    assert C.skinny_splits(8192, 1088) == 1 and C.skinny_splits(8, 64) == 1 and C.skinny_splits(40, 128) == 2


def test_tier_a_operands_are_exact():
    """|x|, |w| <= 4 and K <= 1088: every partial sum of products is an integer below 2^24"""
    K = max(k for (_, k), _, _ in C.SKINNY_SHAPES)
    assert 16 * K + 1024 < 2 ** 24
    x = E.small_ints((5, 128), 1)
    assert float(x.abs().max()) <= 4 and bool((x == x.round()).all()) and 0.3 < float((x == 0).float().mean()) < 0.8
    lg = torch.tensor([[1.0, 3.0, 3.0, 2.0, 3.0]])
    v, i = E.topk_order(lg, 4)
    assert i.tolist() == [[1, 2, 4, 3]] and v.tolist() == [[3.0, 3.0, 3.0, 2.0]]


def test_attn_emulation_under_bound(capsys):
    worst = {}
    for scale in C.ATTN_SCALES:
        for t in C.ATTN_T:
            qkv = E.attn_case(2, t, 3)
            ref, v = E.attn_ref(qkv, 2, t, 3, scale)
            r = E.check_attn_bound(E.attn_emulate(qkv, 2, t, 3, scale), ref, v, 2, t, 3)
            worst[f"scale {scale}"] = max(worst.get(f"scale {scale}", 0.0), r)
    for t in (33, 128):
        qkv = E.attn_dominant_case(2, t, 3)
        ref, v = E.attn_ref(qkv, 2, t, 3, 0.125)
        got = E.attn_emulate(qkv, 2, t, 3, 0.125)
        worst["dominant key"] = max(worst.get("dominant key", 0.0), E.check_attn_bound(got, ref, v, 2, t, 3))
        vrow = qkv.view(2 * t, 3, 192)[:, 2]
        assert bool(((got.double() - vrow.double()).abs() <= E.attn_bound(ref, v, 2, t, 3)).all())
        assert E.bits_equal(got.view(2, t, 192)[:, 0], vrow.view(2, t, 192)[:, 0])          # p = 1 exactly on row 0
    with capsys.disabled():
        print("\nattn_causal f32 emulation vs float64, worst err/bound: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert max(worst.values()) < 1.0


def _pool_cases():
    return [(W, nout, group) for W in C.POOL_W for nout in C.POOL_NOUT for group in C.POOL_GROUP]


def test_pool_emulation_under_bound(capsys):
    worst = {}
    for W, nout, group in _pool_cases():
        x, rows, gamma, beta = E.pool_case(W, nout, group)
        assert int(rows.min()) >= 0 and int(rows.max()) < E.POOL_R
        for dt in (torch.float32, torch.bfloat16):
            ref, bound = E.pool_ref(x, rows, gamma, beta, group, out_dtype=dt)
            got = E.pool_emulate(x, rows, gamma, beta, group, out_dtype=dt)
            k = f"W {W} {'f32' if dt == torch.float32 else 'bf16'}"
            worst[k] = max(worst.get(k, 0.0), E.ratio((got.double() - ref).abs(), bound))
        if nout == 5 and group == 1:
            assert E.bits_equal(E.pool_emulate(x, rows, gamma, beta, 1)[-1], beta)           # the constant row: exactly beta
    with capsys.disabled():
        print("\ntext_pool f32 emulation vs float64, worst err/bound: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert max(worst.values()) < 1.0


@pytest.mark.parametrize("mutant", E.POOL_MUTANTS)
def test_pool_bound_rejects_mutant(mutant, capsys):
    rs = {}
    for W, nout, group in _pool_cases():
        if nout != 5 or (mutant == "group mean before LN" and group == 1):
            continue
        x, rows, gamma, beta = E.pool_case(W, nout, group)
        ref, bound = E.pool_ref(x, rows, gamma, beta, group)
        err = (E.pool_emulate(x, rows, gamma, beta, group, mutant=mutant).double() - ref).abs()
        fin = torch.isfinite(err)            # (without eps the constant row is 0 * inf = NaN: judge the mutant on the finite outputs)
        assert bool(fin.any())
        rs[(W, group)] = E.ratio(err[fin], bound[fin])
    with capsys.disabled():
        print(f"\n  text_pool mutant {mutant:22s} err/bound min {min(rs.values()):.1f} max {max(rs.values()):.1f}")
    assert all(r > 1.0 for r in rs.values()), rs


def test_activation_emulation_under_bound(capsys):
    worst = {}
    for name in E.ACT_REF:
        for dt, key in ((torch.float32, "f32"), (torch.bfloat16, "bf16")):
            g = torch.Generator().manual_seed(3)
            x = torch.cat([(torch.randn(C.ACT_NUMEL[key][1], generator=g) * 4).to(dt), E.specials(dt),
                           torch.linspace(-12, 12, 4096).to(dt)])
            worst[f"{name} {key}"] = E.act_check(E.act_emulate(x, name), x, name)
    with capsys.disabled():
        print("\nactivation f32 emulation vs float64, worst err/bound: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert max(worst.values()) < 1.0


def test_activation_bound_cannot_be_relative():
    """where 1 + tanh cancels, the f32 result has no relative accuracy: an f32 evaluation is off by far more than a few u |g| at
    x ~ -5, while it stays within C_ACT u |x|"""
    x = torch.linspace(-6, -4, 257)
    g = E.gelu_new_ref(x)
    err = (E.act_emulate(x, "gelu_new").double() - g).abs()
    assert float((err / (E.U * g.abs())).max()) > 100 * E.C_ACT and bool((err <= E.act_bound(x, g, torch.float32)).all())


def test_specials_table():
    for dt, per in ((torch.float32, 4), (torch.bfloat16, 8)):
        s = E.specials(dt)
        assert s.numel() % per == 0 and bool(torch.isnan(s).any()) and int(torch.isinf(s).sum()) == 2
        assert float(s[torch.isfinite(s)].abs().max()) == E.BF16_MAX
        assert bool(((s != 0) & (s.float().abs() < 2.0 ** -126)).any())                   # subnormals survive the cast
    q, n = E.quick_gelu_ref(torch.tensor([float("-inf"), float("inf")])), E.gelu_new_ref(torch.tensor([float("-inf"), float("inf")]))
    assert bool(torch.isnan(q[0])) and bool(torch.isnan(n[0])) and float(q[1]) == float("inf") and float(n[1]) == float("inf")
