"""Weight averaging (MODEL_EMA) without a GPU:
  a. the float64 reference of tests/exact_average.py and solver.average_weight, driven through solver.WeightAverage, reproduce
     torch.optim.swa_utils.AveragedModel to a few float64 roundings: EMA with decay 0.9 and 0.999, the default uniform mean over 5
     updates; the first update copies, the n of 1 / (n + 1), and start_iter delays the copy
  b. an f32 emulation of cddmsl_weight_average stays within the bound at the whole case list, and each mutant of it is rejected
  c. WeightAverage's state round trip and refusals, applied(), the config block and its ValueErrors, the _EMA key helper
  d. tools/average_checkpoints.py: its file logic on three tiny state dicts, its arithmetic against the float64 reference
  e. the argument errors of the raw C-ABI entry point, which return before any HIP call"""
import ctypes
import importlib.util
import math
import os

import pytest
import torch

import exact_average as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _f64_kernel(avgs, params, w, copy):
    """hip.weight_average's contract in float64 with the exact scalar: the reference itself"""
    for e, p in zip(avgs, params):
        e.copy_(p if copy else A.average_ref(e, p, w, exact_scalar=True)[0])


def _f32_kernel(avgs, params, w, copy):
    w32 = torch.tensor(w, dtype=torch.float32)
    for e, p in zip(avgs, params):
        e.copy_(p if copy else e + w32 * (p - e))


class _Small(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.a = torch.nn.Linear(5, 3).double()
        self.b = torch.nn.Parameter(torch.randn(7, dtype=torch.float64))


@pytest.mark.parametrize("mode,decay", [("ema", 0.9), ("ema", 0.999), ("uniform", 0.0)])
def test_schedule_matches_swa_utils(monkeypatch, mode, decay):
    from torch.optim import swa_utils
    from cddmsl_amd import hip
    from cddmsl_amd.solver import WeightAverage
    monkeypatch.setattr(hip, "weight_average", _f64_kernel)
    torch.manual_seed(3)
    model = _Small()
    kw = dict(multi_avg_fn=swa_utils.get_ema_multi_avg_fn(decay)) if mode == "ema" else {}
    ref = swa_utils.AveragedModel(model, **kw)
    start = 2
    wa = WeightAverage(list(model.named_parameters()), mode, decay, start_iter=start)
    for it in range(start + 6):                                    # the copy and 5 updates
        with torch.no_grad():
            for p in model.parameters():
                p.add_(torch.randn_like(p) * 0.1)
        wa.update(it)
        if it >= start:
            ref.update_parameters(model)
        assert wa.updates == max(0, it - start + 1)
        if it == start:                                            # the first update at start_iter is a copy
            assert all(torch.equal(t, p) for t, p in zip(wa.tensors, model.parameters()))
        if it < start:
            assert all(bool((t == 0).all()) for t in wa.tensors)
    assert int(ref.n_averaged) == wa.updates == 6
    want = dict(ref.module.named_parameters())
    for name, t in zip(wa.names, wa.tensors):
        assert not torch.equal(t, dict(model.named_parameters())[name])
        # 5 updates of 3 roundings each (4 for the uniform mean: torch divides by n + 1), relative to the largest operand, not to
        # the element: the subtraction cancels
        scale = float(max(t.abs().max(), dict(model.named_parameters())[name].detach().abs().max())) + 1.0
        assert float((t - want[name].detach()).abs().max()) <= 5 * 4 * 2.0 ** -53 * scale, name


def test_average_weight():
    from cddmsl_amd.solver import average_weight
    assert average_weight("ema", 0.999, 1) == 1.0 - 0.999 == average_weight("ema", 0.999, 1000)
    assert [average_weight("uniform", 0.999, n) for n in (1, 2, 4)] == [1.0 / 2.0, 1.0 / 3.0, 1.0 / 5.0]
    for bad in (lambda: average_weight("ema", 0.9, 0), lambda: average_weight("swa", 0.9, 1)):
        with pytest.raises(ValueError):
            bad()


class _Cpu:
    def __init__(self, mut=None):
        self.em = A.Emulation(mut)

    def average(self, lay, e, p, w, copy):
        before = p.clone()
        out = self.em.average(lay, e, p, w, copy)
        assert A.bits_equal(p, before)
        return out


def _run_all(impl):
    rep = A.Report()
    for c in A.average_cases():
        A.run_average(c, impl, rep)
    return rep


def test_emulation_within_bounds_and_mutants_rejected():
    cases = A.average_cases()
    assert len(cases) == len(A.COUNTS) * len(A.WS) + 2
    assert {c["count"] for c in cases} == {1, 4, A.AVG_MAX, A.AVG_MAX + 1, 2 * A.AVG_MAX + 1}
    lay, _ = A.average_layout(dict(count=4, rot=0))
    assert lay[0][0] == 2 ** 20 + 3 and [(oe % 4, op % 4) for _, oe, op in lay] == [(0, 0), (1, 0), (0, 1), (2, 2)]
    rep = _run_all(_Cpu())
    assert not rep.fail, "\n".join(rep.fail[:10])
    assert 0.0 < rep.worst["weight_average avg"] <= 1.0
    for mut in ("swap", "w_off", "drop_tail", "skip_after_batch", "guard"):
        assert _run_all(_Cpu(mut)).fail, f"the mutant {mut} passes every case"


def test_sequence_bound_recurrence():
    """b_n = (1 - w_n) b_{n-1} + step_n, against the f32 emulation over 6 snapshots"""
    snaps = [A._randn((4099,), 50 + k) for k in range(6)]
    for ws in ([0.5] * 5, [1.0 / (n + 1) for n in range(1, 6)], [1.0 - 0.999] * 5):
        e = snaps[0].clone()
        for p, w in zip(snaps[1:], ws):
            _f32_kernel([e], [p], w, False)
        want, bound = A.average_sequence(snaps, ws)
        assert bool(((e.double() - want).abs() <= bound).all())
        assert float(bound.max()) < 4 * 5 * A.U * 5.0                # a few roundings per update on values below 5
    want, _ = A.average_sequence(snaps, [1.0 / (n + 1) for n in range(1, 6)])
    assert torch.allclose(want, torch.stack(snaps).double().mean(0), rtol=0, atol=1e-7)


def _named(seed=0, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    conv = torch.randn(4, 3, 3, 3, generator=g, dtype=dtype).contiguous(memory_format=torch.channels_last)
    return [("conv.weight", torch.nn.Parameter(conv)), ("fc.weight", torch.nn.Parameter(torch.randn(6, 5, generator=g, dtype=dtype))),
            ("fc.bias", torch.nn.Parameter(torch.randn(6, generator=g, dtype=dtype)))]


def test_state_round_trip_and_refusals(monkeypatch):
    from cddmsl_amd import hip
    from cddmsl_amd.solver import WeightAverage
    monkeypatch.setattr(hip, "weight_average", _f32_kernel)
    named = _named()
    wa = WeightAverage(named, "ema", 0.5, start_iter=1)
    assert [t.stride() for t in wa.tensors] == [p.stride() for _, p in named] and all(t.dtype == torch.float32 for t in wa.tensors)
    assert wa.state_dict()["updates"] == 0
    for it in range(4):
        with torch.no_grad():
            for _, p in named:
                p.add_(1.0)
        wa.update(it)
    sd = wa.state_dict()
    assert sorted(sd) == ["decay", "mode", "start_iter", "tensors", "updates"]
    assert (sd["mode"], sd["decay"], sd["start_iter"], sd["updates"]) == ("ema", 0.5, 1, 3)
    assert list(sd["tensors"]) == ["conv.weight", "fc.weight", "fc.bias"] and all(t.device.type == "cpu" for t in sd["tensors"].values())
    sd["tensors"]["fc.bias"] += 0.0                                  # the saved tensors are copies, not views of the live ones
    assert sd["tensors"]["fc.bias"].data_ptr() != wa.tensors[2].data_ptr()
    other = WeightAverage(_named(5), "ema", 0.5, start_iter=1)
    other.load_state_dict(sd)
    assert other.updates == 3 and all(A.bits_equal(a, b) for a, b in zip(other.tensors, wa.tensors))
    assert [t.stride() for t in other.tensors] == [t.stride() for t in wa.tensors]
    # after 3 updates with decay 0.5 on p = p0 + 2, + 3, + 4: p0 + 3.25
    assert torch.allclose(wa.tensors[2], named[2][1].detach() - 4.0 + 3.25, atol=1e-6)
    with pytest.raises(ValueError, match="mode"):
        WeightAverage(_named(), "uniform", 0.5).load_state_dict(sd)
    with pytest.raises(ValueError, match="other parameters"):
        WeightAverage(_named()[:2], "ema", 0.5).load_state_dict(sd)
    with pytest.raises(ValueError, match="other parameters"):
        WeightAverage([("x." + k, p) for k, p in _named()], "ema", 0.5).load_state_dict(sd)
    bad = dict(sd, tensors=dict(sd["tensors"], **{"fc.bias": torch.zeros(7)}))
    with pytest.raises(ValueError, match="fc.bias"):
        WeightAverage(_named(), "ema", 0.5).load_state_dict(bad)
    with pytest.raises(ValueError, match="MODE"):
        WeightAverage(_named(), "swa", 0.5)


def test_applied_exchanges_contents_and_restores(monkeypatch):
    from cddmsl_amd import hip, layers
    from cddmsl_amd.solver import WeightAverage
    monkeypatch.setattr(hip, "weight_average", _f32_kernel)
    named = _named()
    params = [p for _, p in named]
    wa = WeightAverage(named, "uniform", 0.0)
    v0 = layers.weight_version()
    with wa.applied(None):                                           # before any update: nothing happens
        assert layers.weight_version() == v0
    for it in range(3):
        with torch.no_grad():
            for p in params:
                p.mul_(1.5)
        wa.update(it)
    before = [p.detach().clone() for p in params]
    ptrs = [p.data_ptr() for p in params]
    avg = [t.clone() for t in wa.tensors]
    with pytest.raises(RuntimeError, match="inside"):
        with wa.applied(None):
            assert layers.weight_version() == v0 + 1
            assert all(A.bits_equal(p.detach(), t) for p, t in zip(params, wa.tensors)) and [p.data_ptr() for p in params] == ptrs
            assert not any(torch.equal(p.detach(), b) for p, b in zip(params, before))
            raise RuntimeError("inside")
    assert layers.weight_version() == v0 + 2
    assert all(A.bits_equal(p.detach(), b) for p, b in zip(params, before)) and [p.data_ptr() for p in params] == ptrs
    assert all(A.bits_equal(t, a) for t, a in zip(wa.tensors, avg))


def test_config_block_and_errors():
    from cddmsl_amd import evaluation
    from cddmsl_amd.config import check_model_ema, get_cfg
    cfg = get_cfg()
    e = cfg.MODEL_EMA
    assert (e.ENABLED, e.MODE, e.DECAY, e.START_ITER, e.EVAL) == (False, "ema", 0.999, 0, "both")
    assert check_model_ema(cfg) is None
    cfg.merge_from_list(["MODEL_EMA.MODE", "bogus"])                 # a disabled block is not judged
    assert check_model_ema(cfg) is None
    for key, value in (("MODE", "swa"), ("EVAL", "ema"), ("DECAY", 1.0), ("DECAY", -0.1), ("DECAY", float("nan")), ("START_ITER", -1)):
        cfg = get_cfg()
        cfg.merge_from_list(["MODEL_EMA.ENABLED", True, "MODEL_EMA." + key, value])
        with pytest.raises(ValueError, match="MODEL_EMA." + key):
            check_model_ema(cfg)
        with pytest.raises(ValueError, match="MODEL_EMA." + key):    # the evaluation refuses it when it is built
            evaluation.averaged_passes(None, cfg, None)
    for mode in ("ema", "uniform"):
        for ev in ("plain", "averaged", "both"):
            cfg = get_cfg()
            cfg.merge_from_list(["MODEL_EMA.ENABLED", True, "MODEL_EMA.MODE", mode, "MODEL_EMA.EVAL", ev, "MODEL_EMA.DECAY", 0.0])
            assert check_model_ema(cfg) is cfg.MODEL_EMA


def test_ema_keys_and_passes(monkeypatch):
    from cddmsl_amd import evaluation, hip
    from cddmsl_amd.config import get_cfg
    from cddmsl_amd.solver import WeightAverage
    res = {"bbox": {"AP": 1.0}, "bbox_TTA": {"AP": 2.0}, "box_proposals": {"AR@100": 3.0}}
    out = evaluation.with_ema_suffix(res)
    assert list(out) == ["bbox_EMA", "bbox_TTA_EMA", "box_proposals_EMA"] and out["bbox_EMA"] is res["bbox"]
    assert evaluation.with_ema_suffix(None) == {}
    assert list(evaluation.flatten_results({"bdd_100k_val": out})) == ["bdd_100k_val/bbox_EMA/AP", "bdd_100k_val/bbox_TTA_EMA/AP",
                                                                       "bdd_100k_val/box_proposals_EMA/AR@100"]
    monkeypatch.setattr(hip, "weight_average", _f32_kernel)
    wa = WeightAverage(_named(), "ema", 0.5)
    passes = lambda ev, w, on=True: [a for a, _ in evaluation.averaged_passes(None, _cfg(on, ev), w)]

    def _cfg(on, ev):
        cfg = get_cfg()
        cfg.merge_from_list(["MODEL_EMA.ENABLED", on, "MODEL_EMA.EVAL", ev])
        return cfg
    assert passes("both", wa) == [False]                             # no update yet: the plain weights only
    wa.update(0)
    assert passes("both", wa) == [False, True] and passes("averaged", wa) == [True] and passes("plain", wa) == [False]
    assert passes("both", None) == [False] and passes("both", wa, on=False) == [False]


def _tool():
    spec = importlib.util.spec_from_file_location("average_checkpoints", os.path.join(ROOT, "tools", "average_checkpoints.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_average_checkpoints_file_logic():
    tool = _tool()
    g = torch.Generator().manual_seed(9)
    mk = lambda k: {"w": torch.randn(33, 5, generator=g), "b": torch.randn(5, generator=g).half(), "steps": torch.tensor([k]),
                    "pixel_mean": torch.randn(3, generator=g)}
    states = [mk(1), mk(2), mk(3)]
    del states[1]["pixel_mean"]                                      # absent from one file: taken from the last file, not averaged
    states[1]["extra"] = torch.ones(2)                               # held by one file only: kept as it is
    calls = []

    def accumulate(avgs, tensors, w, copy):
        assert all(t.dtype == torch.float32 and t.is_contiguous() for t in avgs + tensors)
        calls.append((w, copy))
        _f32_kernel(avgs, tensors, w, copy)
    out = tool.average_states(states, accumulate)
    assert calls == [(0.0, True), (1.0 / 2.0, False), (1.0 / 3.0, False)]
    assert list(out) == ["w", "b", "steps", "pixel_mean", "extra"]
    assert torch.equal(out["steps"], torch.tensor([3])) and A.bits_equal(out["pixel_mean"], states[2]["pixel_mean"])
    assert A.bits_equal(out["extra"], torch.ones(2))
    assert out["w"].dtype == torch.float32 and out["b"].dtype == torch.float16
    want, bound = A.average_sequence([s["w"] for s in states], [1.0 / 2.0, 1.0 / 3.0])
    assert bool(((out["w"].double() - want).abs() <= bound).all())
    mean = torch.stack([s["w"].double() for s in states]).mean(0)
    # the reference takes w as the f32 nearest to 1 / 3, the mean a third: |w - 1/3| <= u / 3 on |p_3 - e_2| <= |p_3| + (|p_1| + |p_2|) / 2
    assert bool(((want - mean).abs() <= A.U / 3 * torch.stack([s["w"].double().abs() for s in states]).sum(0) + A.TINY).all())
    assert torch.allclose(out["b"].double(), torch.stack([s["b"].double() for s in states]).mean(0), atol=2e-3)
    states[2]["w"] = torch.zeros(5, 33)
    with pytest.raises(ValueError, match=r"^w: shape"):
        tool.average_states(states, accumulate)


# ---------------------------------------------------------------------------------------------------- the raw C-ABI, no GPU needed
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from cddmsl_amd import _lib
    return _lib.lib_weight_average()


def test_side_library_exports_its_header(lib):
    """libcddmsl_weight_average.so exports what include/cddmsl_weight_average.h declares and nothing else; the header is C"""
    import re
    import subprocess
    from cddmsl_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", " ", open(_lib.WEIGHT_AVERAGE_HEADER_PATH).read(), flags=re.S)
    names = sorted(set(re.findall(r"\bint\s+(cddmsl_\w+)\s*\(", hdr)))
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.WEIGHT_AVERAGE_LIB_PATH], text=True)
    assert sorted(set(re.findall(r"\bT (cddmsl_\w+)", out))) == names == ["cddmsl_weight_average"]
    subprocess.check_call(["gcc", "-std=c99", "-fsyntax-only", "-x", "c", _lib.WEIGHT_AVERAGE_HEADER_PATH])
    main = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    assert "cddmsl_weight_average" not in main


def test_cabi_argument_errors_return_before_any_hip_call(lib):
    vp, ci, cf = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    assert lib.cddmsl_weight_average.restype is ctypes.c_int and lib.cddmsl_weight_average.argtypes == [vp, vp, vp, ci, cf, ci, vp]
    host = (ctypes.c_float * 16)()                                   # never dereferenced: every call below returns at the checks
    one = (ctypes.c_void_p * 2)(ctypes.addressof(host), ctypes.addressof(host))
    sizes = lambda *v: (ctypes.c_long * len(v))(*v)
    call = lambda s, count, w, copy: lib.cddmsl_weight_average(one, one, s, count, w, copy, None)
    assert call(sizes(8, 8), -1, 0.5, 0) == 1 and call(sizes(8, 8), -1, 0.5, 1) == 1
    assert call(sizes(8, -1), 2, 0.5, 0) == 1 and call(sizes(-8, 8), 2, 0.5, 1) == 1
    for w in (float("nan"), -0.1, 1.5, math.inf):
        assert call(sizes(8, 8), 2, w, 0) == 1
    assert call(sizes(8, 8), 0, 0.5, 0) == 0 and call(sizes(8, 8), 0, 0.5, 1) == 0
    assert lib.cddmsl_weight_average(None, None, None, 0, 0.5, 0, None) == 0
    assert call(sizes(0, 0), 2, 0.5, 0) == 0 and call(sizes(0, 0), 2, float("nan"), 1) == 0      # all sizes 0: nothing to launch
