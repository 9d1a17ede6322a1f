"""The sparse backward pass of the RPN head (layers.RpnHeadFn, csrc/rpn_sparse.hip) against the dense one and against float64 autograd.

Shapes: 2 images of 3 x 3 and of 5 x 7 positions, 64 channels in and out, 3 anchors (heads of 3 + 12 = 15 -> 16 columns).

Two kinds of input.  "exact": every tensor holds small integers ({-2 .. 2}, bf16-exact) so that every partial sum of the backward
pass is exact in f32 (the largest, a heads' weight-gradient element, stays below 70 rows x 2304 x 2 < 2^24): the sparse and the
dense route then form the same numbers in any summation order and must agree BIT FOR BIT in all gradients -- this is what catches a
wrong tap, a flipped filter, a wrapped image border or a mis-ordered K.  "random": each route against float64 autograd of the plainly
written module (tests/graph_ref.py) on the same bf16-valued operands, under the limits tests/test_gpu_graph_exact.py applies to
ConvFn and FusedHeadsFn: f32 -- 8 times the error of the plain module in float32 on the CPU, floor 1e-6; bf16 -- 4 times the error
of the plain module with every materialised tensor rounded to bf16, floor 2^-8 (graph_ref's constants; nothing here looks at a
result of the node to set a limit).

Four tests without a GPU: the row-count rule that chooses the route, the trainer raising on the overflow flag, the sparse
kernels' entry points in the main library and its header, and the random cases' limits against graph_ref's caps."""
import pytest
import torch

import graph_ref as G

gpu = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
DT = {"f32": torch.float32, "bf16": BF}
C, A, NIMG = 64, 3, 2
NPAD = 16
SHAPES = [(3, 3), (5, 7)]
NAMES = ("dx", "w", "b", "w0", "b0", "w1", "b1")


def _positions(H, W):
    """named sets of active positions (image, row, column) on an H x W map"""
    h2, w2 = H // 2, W // 2
    single = {"corner_tl": (0, 0), "corner_tr": (0, W - 1), "corner_bl": (H - 1, 0), "corner_br": (H - 1, W - 1),
              "edge_t": (0, w2), "edge_l": (h2, 0), "edge_b": (H - 1, w2), "edge_r": (h2, W - 1), "centre": (h2, w2)}
    out = {k: [(0, h, w)] for k, (h, w) in single.items()}
    out["none"] = []
    out["last_of_image0"] = [(0, H - 1, W - 1)]
    out["first_of_image1"] = [(1, 0, 0)]
    out["mixed"] = [(0, 0, 0), (0, h2, w2), (0, H - 1, W - 1), (1, 0, 0), (1, 0, W - 1), (1, H - 1, w2)]
    out["all"] = [(n, h, w) for n in range(NIMG) for h in range(H) for w in range(W)]
    return out


def _ints(g, shape, lo=-2, hi=2):
    return torch.randint(lo, hi + 1, shape, generator=g).to(torch.float32)


def _bfv(t):
    return t.to(BF).to(torch.float32)


_inputs = {}


def make_inputs(H, W, kind):
    """CPU f32 tensors with bf16-exact values: x NHWC, the 3x3 filter [C, C, 3, 3] and bias, the two heads"""
    key = (H, W, kind)
    if key not in _inputs:
        g = torch.Generator().manual_seed(1000 * H + 10 * W + (kind == "exact"))
        if kind == "exact":
            d = {"x": _ints(g, (NIMG, H, W, C)), "w": _ints(g, (C, C, 3, 3)), "b": _ints(g, (C,)),
                 "w0": _ints(g, (A, C)), "b0": _ints(g, (A,)), "w1": _ints(g, (4 * A, C)), "b1": _ints(g, (4 * A,))}
        else:
            # the first of seed, seed + 1000, ... whose hidden ReLU has graph_ref's margin for biases drawn like these ("natural"): no
            # pre-activation so close to zero that f32 and float64 could put it on different sides
            for attempt in range(G.ATTEMPTS):
                g = torch.Generator().manual_seed(1000 * H + 10 * W + 100000 * attempt)
                r = lambda *s: torch.randn(*s, generator=g)
                d = {"x": _bfv(r(NIMG, H, W, C)), "w": _bfv(r(C, C, 3, 3) / 24.0), "b": _bfv(0.1 * r(C)),
                     "w0": _bfv(r(A, C) / 8.0), "b0": _bfv(0.1 * r(A)), "w1": _bfv(r(4 * A, C) / 8.0), "b1": _bfv(0.1 * r(4 * A))}
                z, b = G.conv(d["x"].to(G.F64), d["w"].to(G.F64), pad=1), d["b"].to(G.F64)
                d["margin"] = float(((z + b).abs() / (z.abs() + b.abs())).min())
                if d["margin"] >= G.MARGIN["natural"]:
                    break
        _inputs[key] = d
    return _inputs[key]


def make_dy(H, W, kind, pos, two_anchors=False):
    """the gradient of the heads' output: zero but on the rows ``pos``; never anything in the pad column.  ``two_anchors``: only two
    anchors' entries of a row (two sampled anchors on one position)"""
    g = torch.Generator().manual_seed(7 + 31 * len(pos) + H)
    dy = torch.zeros(NIMG, H, W, NPAD)
    for (n, h, w) in pos:
        if kind == "exact":
            row = _ints(g, (5 * A,))
            row[0] = 1.0                       # (never an all-zero row: the position is active)
        else:
            row = _bfv(torch.randn(5 * A, generator=g))
        if two_anchors:
            keep = torch.zeros(5 * A)
            keep[0], keep[2] = 1.0, 1.0
            row = row * keep + keep * (row == 0)
        dy[n, h, w, :5 * A] = row
    return dy


def run_head(inp, dy, T, sparse, cap):
    """forward + backward of layers.rpn_head on the GPU -> {name: gradient}, rows of the profiler"""
    from cddmsl_amd import hip, layers
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("CDDMSL_RPN_SPARSE_BWD", "1" if sparse else "0")
        x = inp["x"].to(DEV, T).requires_grad_(True)
        par = {n: torch.nn.Parameter(inp[n].to(DEV)) for n in ("b", "w0", "b0", "w1", "b1")}
        par["w"] = torch.nn.Parameter(inp["w"].to(DEV).contiguous(memory_format=torch.channels_last))
        active = layers.ActiveRows()
        y = layers.rpn_head(x, layers.PreparedWeight(par["w"], None, False), par["b"], [(par["w0"], par["b0"]), (par["w1"], par["b1"])], active)
        assert y.dtype == torch.float32 and tuple(y.shape) == tuple(dy.shape)
        active.cap = cap
        layers.take_touched()
        hip.PROFILE.enable()
        try:
            y.backward(dy.to(DEV))
            rows = [e[0] for e in hip.PROFILE.events]
            hip.PROFILE.collect()
        finally:
            hip.PROFILE.on = False
        torch.cuda.synchronize()
        assert layers.take_touched() == {id(p) for p in par.values()}
    out = {"dx": x.grad}
    out.update({n: p.grad for n, p in par.items()})
    assert ("rpn_dx_gather" in rows) == bool(sparse) and ("relu_bwd" in rows) == (not sparse), rows
    assert int(layers.RPN_SPARSE_OVERFLOW.flag(x.device).item()) == 0
    return out


def _plain(inp, dy, dtype, round_bf16):
    leaves = {n: inp[n].detach().clone().to(dtype).requires_grad_(True) for n in ("x", "w", "b", "w0", "b0", "w1", "b1")}
    t = G.conv(leaves["x"], leaves["w"], leaves["b"], pad=1, relu=True, round_bf16=round_bf16)
    y = G.fused_heads(t, [(leaves["w0"], leaves["b0"]), (leaves["w1"], leaves["b1"])], round_bf16=round_bf16)
    y.backward(dy.to(dtype))
    out = {("dx" if n == "x" else n): v.grad.to(G.F64) for n, v in leaves.items()}
    return out


_refs = {}


def reference(H, W, case, dy):
    """float64 reference and (f32, bf16) limits per gradient, once per case: graph_ref.prepared's recipe"""
    key = (H, W, case)
    if key not in _refs:
        inp = make_inputs(H, W, "random")
        ref = _plain(inp, dy, G.F64, False)
        threads = torch.get_num_threads()
        torch.set_num_threads(1)
        try:
            r32 = _plain(inp, dy, torch.float32, False)
        finally:
            torch.set_num_threads(threads)
        rbf = _plain(inp, dy, G.F64, True)
        # (a gradient whose reference is exactly zero -- a head none of whose columns got any -- has no limit: it must be exactly zero)
        lim = {n: None if float(v.abs().max()) == 0.0 else
               (max(G.F32_FACTOR * G.rel_err(r32[n], v), G.F32_FLOOR), max(G.BF16_FACTOR * G.rel_err(rbf[n], v), G.BF16_FLOOR))
               for n, v in ref.items()}
        _refs[key] = (ref, lim)
    return _refs[key]


def _over_limit(got, ref, lim, tname, label):
    """-> [(name, error, limit)] of the gradients beyond their limit; every figure is printed first"""
    bad = []
    for n in NAMES:
        assert bool(torch.isfinite(got[n].float()).all()), n
        if lim[n] is None:
            assert float(got[n].float().abs().max()) == 0.0, (label, n, "must be exactly zero")
            continue
        err, limit = G.rel_err(got[n], ref[n]), lim[n][0 if tname == "f32" else 1]
        print(f"{label} {n}: error {err:.3e} limit {limit:.3e} ratio {err / limit:.3f}")
        if not err <= limit:
            bad.append((n, err, limit))
    return bad


EXACT_CASES = [(s, c) for s in SHAPES for c in _positions(*s)]
RANDOM_CASES = [(s, c) for s, c in EXACT_CASES if c != "none"]          # (no active row: test_no_active_row_random_weights)


@gpu
@pytest.mark.parametrize("tname", ["bf16", "f32"])
@pytest.mark.parametrize("shape,case", EXACT_CASES, ids=[f"{h}x{w}-{c}" for (h, w), c in EXACT_CASES])
def test_exact_inputs_bit_equal_to_dense(shape, case, tname):
    """bf16 compute: dy arrives f32 and is cast on the way; f32 compute: dy arrives in the compute dtype.  cap = the active count
    (at least 1: exactly filled) -- the padded variant is test_padding_rows_contribute_nothing."""
    H, W = shape
    pos = _positions(H, W)[case]
    inp, dy = make_inputs(H, W, "exact"), make_dy(H, W, "exact", pos)
    dense = run_head(inp, dy, DT[tname], False, None)
    sparse = run_head(inp, dy, DT[tname], True, max(len(pos), 1))
    for n in NAMES:
        assert bool(torch.isfinite(sparse[n].float()).all()), n
        assert sparse[n].dtype == dense[n].dtype and torch.equal(sparse[n], dense[n]), (case, tname, n, float((sparse[n].float() - dense[n].float()).abs().max()))
    if case == "none":
        for n in NAMES:
            assert float(sparse[n].float().abs().max()) == 0.0, n
    if case == "last_of_image0":
        assert float(sparse["dx"][1].float().abs().max()) == 0.0 and float(sparse["dx"][0].float().abs().max()) > 0.0
    if case == "first_of_image1":
        assert float(sparse["dx"][0].float().abs().max()) == 0.0 and float(sparse["dx"][1].float().abs().max()) > 0.0


@gpu
@pytest.mark.parametrize("tname", ["bf16", "f32"])
@pytest.mark.parametrize("shape,case", RANDOM_CASES, ids=[f"{h}x{w}-{c}" for (h, w), c in RANDOM_CASES])
def test_random_inputs_against_float64_autograd(shape, case, tname):
    H, W = shape
    pos = _positions(H, W)[case]
    inp, dy = make_inputs(H, W, "random"), make_dy(H, W, "random", pos)
    ref, lim = reference(H, W, case, dy)
    for sparse in (True, False):
        got = run_head(inp, dy, DT[tname], sparse, len(pos) + (2 if sparse else 0))
        bad = _over_limit(got, ref, lim, tname, f"{H}x{W} {case} {tname} {'sparse' if sparse else 'dense'}")
        assert not bad, (sparse, bad)


@gpu
@pytest.mark.parametrize("tname", ["bf16", "f32"])
@pytest.mark.parametrize("kind", ["exact", "random"])
def test_no_active_row_random_weights(kind, tname):
    """no active row at all, cap > 0: every gradient exactly zero and finite"""
    H, W = 5, 7
    got = run_head(make_inputs(H, W, kind), torch.zeros(NIMG, H, W, NPAD), DT[tname], True, 4)
    for n in NAMES:
        assert bool(torch.isfinite(got[n].float()).all()) and float(got[n].float().abs().max()) == 0.0, n


@gpu
@pytest.mark.parametrize("tname", ["bf16", "f32"])
@pytest.mark.parametrize("kind", ["exact", "random"])
def test_padding_rows_contribute_nothing(kind, tname):
    """cap exactly filled against cap larger than the active count: the same bits (the padding rows are exact zeros)"""
    H, W = 5, 7
    pos = _positions(H, W)["mixed"]
    inp, dy = make_inputs(H, W, kind), make_dy(H, W, kind, pos)
    filled = run_head(inp, dy, DT[tname], True, len(pos))
    padded = run_head(inp, dy, DT[tname], True, len(pos) + 5)
    for n in NAMES:
        assert torch.equal(filled[n], padded[n]), n


@gpu
@pytest.mark.parametrize("tname", ["bf16", "f32"])
@pytest.mark.parametrize("kind", ["exact", "random"])
def test_sparse_route_twice_same_bits(kind, tname):
    H, W = 5, 7
    pos = _positions(H, W)["all"]
    inp, dy = make_inputs(H, W, kind), make_dy(H, W, kind, pos)
    a = run_head(inp, dy, DT[tname], True, len(pos))
    b = run_head(inp, dy, DT[tname], True, len(pos))
    for n in NAMES:
        assert torch.equal(a[n], b[n]), n


@gpu
@pytest.mark.parametrize("kind", ["exact", "random"])
def test_two_anchors_on_one_position_take_one_slot(kind):
    """two sampled anchors on one position: the bound counts two, the compaction finds one row; gradients as the dense route's"""
    from cddmsl_amd import hip
    H, W = 3, 3
    pos = [(1, 1, 2)]
    inp, dy = make_inputs(H, W, kind), make_dy(H, W, kind, pos, two_anchors=True)
    assert int((dy != 0).sum()) == 2
    flag = torch.zeros(1, device=DEV, dtype=torch.int32)
    rows, slot = hip.rpn_active_rows(dy.to(DEV).view(-1, NPAD), 2, flag)
    p = (1 * H + 1) * W + 2
    assert rows.tolist() == [p, -1] and int(flag.item()) == 0
    assert slot.tolist() == [0 if i == p else -1 for i in range(NIMG * H * W)]
    dense, sparse = run_head(inp, dy, BF, False, None), run_head(inp, dy, BF, True, 2)
    if kind == "exact":
        for n in NAMES:
            assert torch.equal(sparse[n], dense[n]), n
    else:
        ref, lim = reference(H, W, "two_anchors", dy)
        assert lim["w1"] is None and lim["w0"] is not None          # (objectness entries only: the delta head gets no gradient)
        bad = _over_limit(sparse, ref, lim, "bf16", "3x3 two_anchors bf16 sparse")
        assert not bad, bad


@gpu
@pytest.mark.parametrize("src", ["f32", "bf16"])
def test_active_rows_kernels(src):
    """mark + compact + gather on a dy that arrives f32 and on one that arrives in the compute dtype: ascending rows, the inverse map,
    -1 padding, -0.0 inactive, a NaN active; one row more than cap raises the flag and keeps the first cap rows"""
    from cddmsl_amd import hip
    M = 1000                                   # (several 256-row blocks of the mark kernel, a ragged last one, 16 ragged wave spans)
    g = torch.Generator().manual_seed(5)
    act = sorted(torch.randperm(M, generator=g)[:37].tolist() + [0, M - 1])
    act = sorted(set(act))
    dy = torch.zeros(M, NPAD)
    for i, r in enumerate(act):
        dy[r, i % NPAD] = float(i % 5 + 1)
    dy[next(i for i in range(M) if i not in act), 1] = -0.0
    dy[act[5], 2] = float("nan")
    d = dy.to(DEV, DT[src])
    flag = torch.zeros(1, device=DEV, dtype=torch.int32)
    rows, slot = hip.rpn_active_rows(d, len(act) + 3, flag)
    assert rows.tolist() == act + [-1] * 3 and int(flag.item()) == 0
    inv = [-1] * M
    for s, r in enumerate(act):
        inv[r] = s
    assert slot.tolist() == inv
    got = hip.rpn_gather_rows(d, rows, BF)
    want = torch.cat([dy[act], torch.zeros(3, NPAD)]).to(BF)
    assert bool(torch.isnan(got[5, 2])) and torch.equal(torch.nan_to_num(got.cpu().float(), nan=99.0), torch.nan_to_num(want.float(), nan=99.0))
    rows, slot = hip.rpn_active_rows(d, len(act) - 1, flag)
    assert int(flag.item()) == 1 and rows.tolist() == act[:-1] and slot[act[-1]].item() == -1


def test_rule_from_row_counts(monkeypatch):
    """the sparse route where it is cheaper by rows: the bench shape and the Cityscapes shape yes, a single small map no"""
    from cddmsl_amd import layers
    monkeypatch.delenv("CDDMSL_RPN_SPARSE_BWD", raising=False)
    bench = (16 * 256, 16 * 50 * 83)                     # 16 x 800 x 1333, stride 16
    city = (8 * 256, 8 * 64 * 128)                       # 8 x 1024 x 2048
    small = (256, 8 * 10)                                # one 128 x 160 image: more sampled anchors than positions
    for T in (2, 4):
        assert layers.rpn_sparse_bwd_wanted(*bench, 1024, T) and layers.rpn_sparse_bwd_wanted(*city, 1024, T)
        assert not layers.rpn_sparse_bwd_wanted(*small, 1024, T)
        s, d = layers.rpn_sparse_bwd_rows(*bench, 1024, T)
        assert d == 66400 and 4096 < s < 3 * 4096
    assert not layers.rpn_sparse_bwd_wanted(40000, 66400, 1024, 2)          # (most rows active: the gathers would cost more than they save)
    assert not layers.rpn_sparse_bwd_wanted(None, 66400, 1024, 2) and not layers.rpn_sparse_bwd_wanted(0, 66400, 1024, 2)
    monkeypatch.setenv("CDDMSL_RPN_SPARSE_BWD", "0")
    assert not layers.rpn_sparse_bwd_wanted(*bench, 1024, 2)
    monkeypatch.setenv("CDDMSL_RPN_SPARSE_BWD", "1")
    assert layers.rpn_sparse_bwd_wanted(*small, 1024, 2) and not layers.rpn_sparse_bwd_wanted(None, 80, 1024, 2)


def test_overflow_flag_makes_the_metrics_write_raise():
    """the trainer's read-back (engine._write_metrics) raises once a sparse backward pass has flagged dropped rows; host tensors suffice"""
    from types import SimpleNamespace
    from cddmsl_amd import engine, layers
    stub = SimpleNamespace(iter=7, storage={})
    flag = layers.RPN_SPARSE_OVERFLOW.flag(torch.device("cpu"))
    try:
        engine.SimpleTrainer._write_metrics(stub, {"loss": torch.tensor(1.0)}, 0.0)
        assert stub.storage["total_loss"] == 1.0
        flag.fill_(1)
        with pytest.raises(RuntimeError, match="sparse backward pass.*iteration=7"):
            engine.SimpleTrainer._write_metrics(stub, {"loss": torch.tensor(1.0)}, 0.0)
    finally:
        layers.RPN_SPARSE_OVERFLOW._flags.pop(torch.device("cpu"), None)


def test_sparse_kernels_live_in_the_main_library():
    """the five entry points are declared in include/cddmsl_hip.h, exported by libcddmsl_hip.so and typed by _lib.lib() (int return, one
    argtype per declared parameter), as tests/test_cabi_host.py holds every entry point; no library, loader or header beside them"""
    import ctypes
    import os
    import re
    import subprocess
    import __graft_entry__ as g
    g.build()
    from cddmsl_amd import _lib
    L = _lib.lib()
    hdr = re.sub(r"/\*.*?\*/", " ", open(_lib.HEADER_PATH).read(), flags=re.S)
    five = ["cddmsl_rpn_compact_rows", "cddmsl_rpn_dx_gather", "cddmsl_rpn_gather_rows", "cddmsl_rpn_im2col_rows", "cddmsl_rpn_mark_rows"]
    decls = {n: p.count(",") + 1 for n, p in re.findall(r"\bint\s+(cddmsl_\w+)\s*\(([^)]*)\)\s*;", hdr) if n in five}
    assert sorted(decls) == five
    exported = set(re.findall(r"\bT (cddmsl_\w+)", subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)))
    assert set(decls) <= exported
    for n, k in decls.items():
        fn = getattr(L, n)
        assert fn.restype is ctypes.c_int and len(fn.argtypes) == k, n
    stem = "rpn_sparse"                         # (the former side library's loader and header, named after the source file)
    assert not hasattr(_lib, "lib_" + stem)
    assert not [f for _, _, files in os.walk(os.path.dirname(_lib.HEADER_PATH)) for f in files if f == "cddmsl_" + stem + ".h"]


def _random_case_list():
    out = [((H, W), c, make_dy(H, W, "random", _positions(H, W)[c])) for (H, W), c in RANDOM_CASES]
    return out + [((3, 3), "two_anchors", make_dy(3, 3, "random", [(1, 1, 2)], two_anchors=True))]


def test_random_cases_hold_graph_ref_caps_and_margin():
    """what tests/test_graph_ref_host.py asserts of the existing cases, for the random cases here: no f32 limit above graph_ref.F32_CAP,
    no bf16 limit above graph_ref.BF16_CAP, and the hidden ReLU of each shape's inputs keeps graph_ref's margin.  Prints the table."""
    for H, W in SHAPES:
        assert make_inputs(H, W, "random")["margin"] >= G.MARGIN["natural"], (H, W, make_inputs(H, W, "random")["margin"])
    lines = []
    for (H, W), case, dy in _random_case_list():
        ref, lim = reference(H, W, case, dy)
        live = {n: v for n, v in lim.items() if v is not None}
        assert set(lim) - set(live) <= ({"w1", "b1"} if case == "two_anchors" else set()), (case, lim)
        for n, v in live.items():
            assert v[0] <= G.F32_CAP and v[1] <= G.BF16_CAP, (H, W, case, n, v)
        lines.append(f"{H}x{W} {case:16s} f32 limit <= {max(v[0] for v in live.values()):.2e}  bf16 limit <= {max(v[1] for v in live.values()):.2e}")
    print("\nlimits per random case (largest over its gradients)\n" + "\n".join(lines))


def _compaction_reference(dy):
    """(ascending active rows, inverse map) of dy [M, cols] by torch"""
    act = torch.nonzero((dy.float() != 0).any(1) | torch.isnan(dy.float()).any(1))[:, 0]
    inv = torch.full((dy.shape[0],), -1, dtype=torch.int32, device=dy.device)
    inv[act] = torch.arange(act.numel(), dtype=torch.int32, device=dy.device)
    return act.to(torch.int32), inv


@gpu
@pytest.mark.parametrize("src", ["f32", "bf16"])
def test_compaction_carries_its_base_over_many_steps(src):
    """5000 positions: each of the compaction's 16 waves owns 320 and walks them in five 64-wide steps, carrying its running base from
    step to step (at the bench's 66 400 positions it is 65 steps); about 300 active rows, some spans empty, against torch.nonzero.
    Then the same rows under a bound one short: the flag, the first cap rows kept, the last one without a slot."""
    from cddmsl_amd import hip
    M = 5000
    g = torch.Generator().manual_seed(11)
    act = torch.randperm(M, generator=g)[:300]
    act = act[(act < 640) | (act >= 1280)]                      # (waves 2 and 3 find nothing)
    dy = torch.zeros(M, NPAD)
    dy[act, torch.randint(0, NPAD, (act.numel(),), generator=g)] = 1.5
    d = dy.to(DEV, DT[src])
    want_rows, want_slot = _compaction_reference(d)
    n = want_rows.numel()
    assert 200 < n <= 300
    flag = torch.zeros(1, device=DEV, dtype=torch.int32)
    rows, slot = hip.rpn_active_rows(d, n + 7, flag)
    assert torch.equal(rows[:n], want_rows) and bool((rows[n:] == -1).all()) and torch.equal(slot, want_slot) and int(flag.item()) == 0
    rows, slot = hip.rpn_active_rows(d, n - 1, flag)
    want_slot[want_rows[-1].long()] = -1
    assert int(flag.item()) == 1 and torch.equal(rows, want_rows[:-1]) and torch.equal(slot, want_slot)


@gpu
def test_mark_rows_beyond_one_sweep_of_its_grid():
    """the mark kernel's grid stops at 65536 blocks of 256 rows: with more rows than that every block takes a second stride.  Rows of
    one 16-byte chunk (8 bf16), active rows in the first sweep, on the seam and in the ragged tail."""
    from cddmsl_amd import hip
    M = 65536 * 256 + 300
    d = torch.zeros(M, 8, device=DEV, dtype=BF)
    act = [0, 255, 256, 65536 * 256 - 1, 65536 * 256, 65536 * 256 + 255, 65536 * 256 + 256, M - 1]
    d[torch.tensor(act, device=DEV), 3] = 2.0
    flag = torch.zeros(1, device=DEV, dtype=torch.int32)
    rows, slot = hip.rpn_active_rows(d, len(act) + 1, flag)
    assert rows.tolist() == act + [-1] and int(flag.item()) == 0
    assert int((slot >= 0).sum()) == len(act) and slot[torch.tensor(act, device=DEV)].tolist() == list(range(len(act)))


@gpu
@pytest.mark.parametrize("tname", ["bf16", "f32"])
def test_dense_route_is_conv_then_fused_heads(tname):
    """CDDMSL_RPN_SPARSE_BWD=0: the node's dense branch runs the backward passes of FusedHeadsFn and ConvFn (layers._heads_backward,
    layers._conv_backward) -- the same launches, so the same bits as layers.conv followed by layers.fused_heads, in the output and in
    every gradient (shapes at which these kernels do not split their reductions: the sums have one order)"""
    from cddmsl_amd import layers
    H, W = 5, 7
    T = DT[tname]
    inp = make_inputs(H, W, "random")
    dy = make_dy(H, W, "random", _positions(H, W)["all"])
    one = run_head(inp, dy, T, False, NIMG * H * W)
    x = inp["x"].to(DEV, T).requires_grad_(True)
    par = {n: torch.nn.Parameter(inp[n].to(DEV)) for n in ("b", "w0", "b0", "w1", "b1")}
    par["w"] = torch.nn.Parameter(inp["w"].to(DEV).contiguous(memory_format=torch.channels_last))
    t = layers.conv(x, layers.PreparedWeight(par["w"], None, False), par["b"], 1, 1, relu=True)
    y = layers.fused_heads(t, [(par["w0"], par["b0"]), (par["w1"], par["b1"])])
    y.backward(dy.to(DEV))
    torch.cuda.synchronize()
    layers.take_touched()
    two = {"dx": x.grad, **{n: p.grad for n, p in par.items()}}
    for n in NAMES:
        assert torch.equal(one[n], two[n]), n
