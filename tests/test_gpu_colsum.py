import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_colsum_periodic(dtype):
    from cddmsl_amd import hip
    g = torch.Generator().manual_seed(0)
    x = torch.randn(50 * 37 + 13, 96, generator=g).to(dtype)
    ref = x.float().sum(0)
    out = hip.colsum(x.cuda())
    assert (out.cpu() - ref).abs().max() < 1e-3 * max(1.0, float(ref.abs().max()))
    x2 = x[: 50 * 37]
    ref2 = x2.float().view(37, 50, 96).sum(0)
    out2 = hip.colsum(x2.cuda(), period=50)
    assert (out2.cpu() - ref2).abs().max() < 1e-3 * max(1.0, float(ref2.abs().max()))


# (name, rows, cols, period, dtypes, accumulate into a non-zero ``out``)
BOUND_CASES = [
    ("vec_96", 50 * 37 + 13, 96, 1, ("f32", "bf16"), False),            # cols a multiple of 8: k_colsum_vec in both dtypes
    ("scalar_15", 300, 15, 1, ("f32", "bf16"), False),                  # k_colsum
    ("vec_ragged_100", 300, 100, 1, ("f32",), False),                   # f32: 25 chunks of 4, the last 64-chunk column block ragged
    ("scalar_100_bf16", 300, 100, 1, ("bf16",), False),                 # 100 is no multiple of 8: the scalar kernel, two column blocks
    ("period_50_unequal", 50 * 37 + 13, 96, 50, ("f32", "bf16"), False),  # residues 0..12 hold 38 rows, the others 37
    ("two_slabs", 300 * 4 + 3, 96, 1, ("f32", "bf16"), False),          # 1203 rows: more than one 256-row slab per residue (5 slabs)
    ("period_1_two_slabs_scalar", 300 * 4 + 3, 15, 1, ("f32", "bf16"), False),
    ("one_row", 1, 96, 1, ("f32", "bf16"), False),
    ("one_row_period_50", 1, 96, 50, ("f32",), False),                  # 49 residue classes without a row: left as they were
    ("accumulate", 50 * 37 + 13, 96, 1, ("f32", "bf16"), True),
    ("accumulate_period_50", 50 * 37 + 13, 15, 50, ("f32", "bf16"), True),
]


@pytest.mark.parametrize("case", [(c, t) for c in BOUND_CASES for t in c[4]], ids=lambda ct: f"{ct[0][0]}-{ct[1]}")
def test_colsum_within_summation_bound(case):
    """per output: |got - exact| <= (n + 2) * 2^-24 * sum |x|, n = the rows of that output's residue class, exact = the float64 sum of
    the operands as given (with ``out=``: the buffer's previous value is one more operand).  A thread adds at most slab / 4 values one
    after another, four partial sums are added, and one f32 atomic adds the slab's sum to the output: fewer than n + 2 roundings, each
    at most 2^-24 of a partial sum that is at most sum |x|."""
    from cddmsl_amd import hip
    (name, rows, cols, period, _, accumulate), tname = case
    g = torch.Generator().manual_seed(rows * 131 + cols)
    x = torch.randn(rows, cols, generator=g).to(torch.float32 if tname == "f32" else torch.bfloat16)
    shape = (period, cols) if period > 1 else (cols,)
    out0 = torch.randn(shape, generator=g) * 3 if accumulate else torch.zeros(shape)
    x64 = x.double()
    pad = (-rows) % period
    folded = torch.cat([x64, torch.zeros(pad, cols, dtype=torch.float64)]).view(-1, period, cols)
    exact = folded.sum(0).view(shape) + out0.double()
    sumabs = folded.abs().sum(0).view(shape) + out0.double().abs()
    n = torch.tensor([(rows - r + period - 1) // period for r in range(period)], dtype=torch.float64).view(period, 1).expand(period, cols).reshape(shape)
    if accumulate or period > 1 and rows < period:
        buf = out0.cuda()
        got = hip.colsum(x.cuda(), period=period, out=buf)
        assert got.data_ptr() == buf.data_ptr()
    else:
        got = hip.colsum(x.cuda(), period=period)
    assert got.dtype == torch.float32 and tuple(got.shape) == shape
    err = (got.cpu().double() - exact).abs()
    bound = (n + 2) * 2.0 ** -24 * sumabs
    print(f"colsum {name} {tname}: worst error / bound {float((err / bound.clamp_min(1e-300)).max()):.3f}")
    assert bool((err <= bound).all()), (name, tname, float((err / bound.clamp_min(1e-300)).max()))
    if rows < period:
        assert bool((got[rows:] == 0).all())
