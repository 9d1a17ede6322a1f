"""Exact reference, per-element error bound and the shared case list of the weight averaging (cddmsl_weight_average:
k_weight_average of weight_average.hip); imported by test_weight_average_host.py and test_gpu_weight_average.py, not a conftest.  The
conventions are those of exact_solver.py / exact_losses.py: operands as stored (f32), the reference in float64, the scalar w rounded
to f32 first (it crosses the C-ABI as float), u = 2^-24, factor 1.01 for the second-order terms, TINY below the normal range.
Ground truth is torch itself: test_weight_average_host.py checks the reference and solver.average_weight against
torch.optim.swa_utils.AveragedModel in float64.

One update, per element:  r = e + w (p - e)
  d = p - e       one rounding: u |d|
  t = w d         one rounding: u |w d|, and w times d's error: together 2 u w |p - e|
  r = e + t       one rounding: u |r|
  bound = 1.01 u (2 w |p - e| + |r|) + TINY
each rounding counted once; a compiler that contracts the product and the sum into one fused multiply-add drops the second rounding
and stays inside.  Over a sequence of updates the error of the previous average is carried with the factor (1 - w_n) the exact
update puts on it:  b_n = (1 - w_n) b_{n-1} + step_n,  b_0 = 0 (the first update is a copy, bit for bit).
copy is compared bit for bit on int32 views; a NaN / Inf element of p is a convention, not a bound: that element of the average
is NaN / Inf and its neighbours pass their bounds."""
import torch

from exact_losses import S2, TINY, U, Report, _f64, _randn, bits_equal, f32, tag  # noqa: F401

AVG_MAX = 128                       # tensors per launch (AvgBatch)
AVG_CHUNK = 4096                    # elements per block: a tensor is cut into chunks of this many
SIZES = (0, 1, 3, 4, 5, 7, 8, 2047, 2048, 2049, AVG_CHUNK - 1, AVG_CHUNK, AVG_CHUNK + 1, 2 * AVG_CHUNK + 5)
BIG = 2 ** 20 + 3
WS = (0.0, 1.0 - 0.999, 1.0 / 3.0, 0.5, 1.0)
COUNTS = (1, 4, AVG_MAX, AVG_MAX + 1, 2 * AVG_MAX + 1)
# offsets (in floats) of the avg / params views from a 16-byte boundary, tensor i: i % 4 -- both aligned (the 16-byte path), avg off by
# one float, params off by one float, both off by two floats (the scalar path, three ways)
ALIGN = ((0, 0), (1, 0), (0, 1), (2, 2))
EQUAL_EVERY = 5                     # tensor i with i % 5 == 2 starts with avg == params


def average_ref(e, p, w, exact_scalar=False):
    """e, p as stored -> (r, bound) in float64 of one update; exact_scalar: w as the double given (for the comparison with torch
    in float64), not rounded to f32"""
    e, p = _f64(e), _f64(p)
    w = float(w) if exact_scalar else f32(w)
    d = p - e
    r = e + w * d
    return r, S2 * U * (2.0 * w * d.abs() + r.abs()) + TINY


def average_sequence(snapshots, weights):
    """snapshots [p_0, p_1, ...] as stored, weights [w_1, ...] (one per snapshot after the first) -> (average, bound) in float64 after
    the copy of p_0 and the updates with p_1 ...: b_n = (1 - w_n) b_{n-1} + step_n"""
    assert len(weights) == len(snapshots) - 1
    avg = _f64(snapshots[0]).clone()
    b = torch.zeros_like(avg)
    for p, w in zip(snapshots[1:], weights):
        avg, step = average_ref(avg, p, w)
        b = (1.0 - f32(w)) * b + step
    return avg, b


# ================================================================================================== the shared case list
def average_cases():
    """every w at every count (1, 4 with one tensor of 2^20 + 3 elements, B, B + 1, 2 B + 1), the size cycle starting one further for
    each w (so the single tensor is empty, 1, 3, 4 and 5 elements long, and the big tensor meets every alignment pattern); at B + 1:
    the copy with a NaN, an Inf and a -0.0 element, and an update with a NaN and an Inf element"""
    out = [dict(count=count, w=w, rot=wi, copy=0, special=False) for count in COUNTS for wi, w in enumerate(WS)]
    out.append(dict(count=AVG_MAX + 1, w=float("nan"), rot=0, copy=1, special=True))        # (copy ignores w: a NaN must not matter)
    out.append(dict(count=AVG_MAX + 1, w=1.0 / 3.0, rot=0, copy=0, special=True))
    return out


def average_tag(c):
    return tag({k: (f"{v:.4g}" if isinstance(v, float) else v) for k, v in c.items()})


def average_layout(c):
    """per tensor (size, start in the avg buffer, start in the params buffer), >= 4 guard elements between tensors; total length"""
    sizes = [SIZES[(i + c["rot"]) % len(SIZES)] for i in range(c["count"])]
    if c["count"] == 4:
        sizes[c["rot"] % 4] = BIG          # every alignment pattern once: 256 whole chunks and a last one that holds the tail of 3 alone
    lay, cur = [], 4
    for i, n in enumerate(sizes):
        oe, op = ALIGN[i % 4]
        lay.append((n, cur + oe, cur + op))
        cur = (cur + n + 3 + 4 + 3) // 4 * 4
    return lay, cur + 4


# the special elements of a ``special`` case: (tensor, element, value); tensors 7 / 8 / 9 are 2047 (scalar path), 2048 (16-byte path)
# and 2049 elements long with rot = 0, tensor 13 is 2 chunks + 5 elements long and its avg is off a 16-byte boundary
SPECIAL = ((8, 5, float("nan")), (7, 1023, float("inf")), (9, 2048, -0.0), (13, 2 * AVG_CHUNK + 4, float("-inf")))


def average_buffers(c, lay, total):
    """avg and params flat buffers, NaN between the tensors"""
    e = torch.full((total,), float("nan"))
    p = torch.full((total,), float("nan"))
    for i, (n, oe, op) in enumerate(lay):
        pi = _randn((n,), 412 + i)
        p[op:op + n] = pi
        e[oe:oe + n] = pi if i % EQUAL_EVERY == 2 else pi + 0.05 * _randn((n,), 977 + i)
    if c["special"]:
        for i, k, v in SPECIAL:
            assert lay[i][0] > k
            p[lay[i][2] + k] = v
    return e, p


def run_average(c, impl, rep):
    """one call of ``impl.average(lay, e, p, w, copy) -> e'`` (CPU tensors in and out; the implementation checks that p stayed as it
    was) against average_ref"""
    t = average_tag(c)
    lay, total = average_layout(c)
    e, p = average_buffers(c, lay, total)
    e2 = impl.average(lay, e, p, c["w"], c["copy"])
    inside = torch.zeros(total, dtype=torch.bool)
    for n, oe, op in lay:
        inside[oe:oe + n] = True
    rep.exact("weight_average avg", t, bits_equal(e2[~inside], e[~inside]), "an element between the tensors was written")
    special = {(i, k): v for i, k, v in SPECIAL} if c["special"] else {}
    got, want, bound = [], [], []
    for i, (n, oe, op) in enumerate(lay):
        ei, pi, gi = e[oe:oe + n], p[op:op + n], e2[oe:oe + n]
        if c["copy"]:
            rep.exact("weight_average copy", t, bits_equal(gi, pi), f"tensor {i}: the copy is not params bit for bit")
            continue
        r, b = average_ref(ei, pi, c["w"])
        keep = torch.ones(n, dtype=torch.bool)
        for (si, k), v in special.items():
            if si == i and v != v:
                rep.exact("weight_average avg", t, bool(torch.isnan(gi[k])), f"tensor {i}: a NaN element of params is lost")
                keep[k] = False
            elif si == i and abs(v) == float("inf"):
                rep.exact("weight_average avg", t, float(gi[k]) == v, f"tensor {i}: an Inf element of params did not reach the average")
                keep[k] = False
        if i % EQUAL_EVERY == 2 and not any(si == i for si, _ in special):
            rep.exact("weight_average avg", t, torch.equal(gi, pi), f"tensor {i}: avg == params before the update, not after it")
        if c["w"] == 0.0:
            rep.exact("weight_average avg", t, torch.equal(gi[keep], ei[keep]), f"tensor {i}: w == 0 changed a finite average")
        got.append(gi[keep]); want.append(r[keep]); bound.append(b[keep])
    if got:
        rep.bound("weight_average avg", t, torch.cat(got), (torch.cat(want), torch.cat(bound)))


class Emulation:
    """k_weight_average in f32 torch operations on the CPU; ``mut`` names one deliberate mistake"""

    def __init__(self, mut=None):
        self.mut = mut

    def average(self, lay, e, p, w, copy):
        out = e.clone()
        w32 = torch.tensor(w, dtype=torch.float32)
        for i, (n, oe, op) in enumerate(lay):
            if self.mut == "skip_after_batch" and i >= AVG_MAX:
                continue
            ei, pi = e[oe:oe + n], p[op:op + n]
            m = n - n % 4 if self.mut == "drop_tail" else n
            if copy:
                out[oe:oe + m] = pi[:m]
            elif self.mut == "swap":                             # the weight on the wrong operand
                out[oe:oe + m] = (pi + w32 * (ei - pi))[:m]
            elif self.mut == "w_off":                            # another weight: off by a thousandth
                out[oe:oe + m] = (ei + w32 * 1.001 * (pi - ei))[:m]
            else:
                out[oe:oe + m] = (ei + w32 * (pi - ei))[:m]
            if self.mut == "guard" and n:
                out[oe + n] = 0.0
        return out
