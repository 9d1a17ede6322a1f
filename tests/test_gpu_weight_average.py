"""cddmsl_weight_average (k_weight_average of cddmsl_amd/csrc/weight_average.hip, in libcddmsl_weight_average.so) against the float64 reference of
tests/exact_average.py, called through the C-ABI at the case list the host test shares (tests/test_weight_average_host.py runs the
same driver on an f32 emulation and on its mutants); then MODEL_EMA end to end on the tiny trainer of test_gpu_eval_hook.py
(128x160, batch 2, synthetic weights, a learning rate above 0 so that the weights move): the averaged tensors against the float64
recurrence over the snapshots of the same run, the second evaluation pass under ``_EMA`` keys, and the checkpoint round trip with
``--eval-only`` from it.

The case that reaches each branch of the kernel:
  16-byte path / scalar path  avg and params both aligned; avg, params or both off a 16-byte boundary; the n % 4 tail
  batches                     count = 1, 4, B, B + 1, 2 B + 1 for B = 128 tensors per launch; sizes 0 (left out of the launch), 1, 3,
                              4, 5, 7, 8, 2047, 2048, 2049
  chunks                      a block takes 4096 elements of one tensor: sizes 4095, 4096, 4097, 2 x 4096 + 5, and one tensor of
                              2^20 + 3 elements per alignment pattern (256 whole chunks, then one that holds the tail of 3 alone)
  w                           0 (a finite average stays as it is), 1 - 0.999, 1 / 3, 1 / 2, 1; avg == params stays equal
  copy                        bit for bit with a NaN, an Inf and a -0.0 element, w = NaN ignored
  NaN / Inf                   one element of params each: exactly that element of the average
Every params buffer as a whole and every element between the avg tensors is compared bit for bit with what it was."""
import ctypes
import os

import pytest
import torch

import exact_average as A
from test_gpu_eval_hook import BDD_CLASSES, CITY_YAML, H, W, _tool, _write_bdd

pytestmark = pytest.mark.gpu

DEV = "cuda"
WORST = {}


def _L():
    from cddmsl_amd import _lib
    return _lib.lib_weight_average()


def _stream():
    from cddmsl_amd import hip
    return hip.stream_ptr()


class Gpu:
    """exact_average's implementation interface on the C-ABI: CPU tensors in, CPU tensors out"""

    def average(self, lay, e, p, w, copy):
        ed, pd = e.to(DEV), p.to(DEV)
        n = len(lay)
        at = lambda buf, k: (ctypes.c_void_p * n)(*[buf.data_ptr() + 4 * l[k] for l in lay])
        assert ed.data_ptr() % 16 == 0 and pd.data_ptr() % 16 == 0
        assert all(l[1] + l[0] <= e.numel() and l[2] + l[0] <= p.numel() for l in lay)
        sizes = (ctypes.c_long * n)(*[l[0] for l in lay])
        status = _L().cddmsl_weight_average(at(ed, 1), at(pd, 2), sizes, n, w, int(copy), _stream())
        assert status == 0, f"status {status}"
        torch.cuda.synchronize()
        assert A.bits_equal(pd.cpu(), p), "the params buffer was written"
        return ed.cpu()


_CASES = A.average_cases()


@pytest.mark.parametrize("case", _CASES, ids=[A.average_tag(c).replace(" ", ",") for c in _CASES])
def test_weight_average(case):
    rep = A.Report()
    A.run_average(case, Gpu(), rep)
    for k, v in rep.worst.items():
        WORST[k] = max(WORST.get(k, 0.0), v)
        print(f"{k} [{A.average_tag(case)}]: worst |err|/bound {v:.3g}")
    assert not rep.fail, "\n".join(rep.fail[:20])


def test_argument_errors_and_empty_launch_write_nothing():
    """CDDMSL_ERR_ARG (1) for count < 0, a negative size, w NaN or outside [0, 1] without copy; 0 for count == 0 and all sizes 0"""
    L, st = _L(), _stream()
    bufs = [torch.full((24,), float("nan"), device=DEV) for _ in range(2)]
    before = [b.clone() for b in bufs]
    two = lambda b: (ctypes.c_void_p * 2)(b.data_ptr() + 16, b.data_ptr() + 48)
    sizes = lambda *v: (ctypes.c_long * 2)(*v)
    call = lambda s, count, w, copy: L.cddmsl_weight_average(two(bufs[0]), two(bufs[1]), s, count, w, copy, st)
    assert call(sizes(4, 4), -1, 0.5, 0) == 1 and call(sizes(4, -4), 2, 0.5, 0) == 1 and call(sizes(-1, 4), 2, 0.5, 1) == 1
    assert [call(sizes(4, 4), 2, w, 0) for w in (float("nan"), -0.1, 1.5)] == [1, 1, 1]
    assert call(sizes(4, 4), 0, 0.5, 0) == 0 and call(sizes(0, 0), 2, 0.5, 0) == 0 and call(sizes(0, 0), 2, 0.5, 1) == 0
    assert L.cddmsl_weight_average(None, None, None, 0, 0.5, 0, st) == 0
    torch.cuda.synchronize()
    assert all(A.bits_equal(a.cpu(), b.cpu()) for a, b in zip(bufs, before))


def test_wrapper():
    """hip.weight_average passes raw pointers: it refuses other dtypes, layouts, lengths and devices; a channels-last pair works"""
    from cddmsl_amd import hip
    from cddmsl_amd._lib import HipLibraryError
    p = [torch.randn(4, 6, 3, 3, device=DEV).contiguous(memory_format=torch.channels_last), torch.randn(7, device=DEV)]
    e = [torch.zeros_like(x, memory_format=torch.preserve_format) for x in p]
    bad = [dict(avgs=e[:1]), dict(avgs=[e[0].contiguous(), e[1]]), dict(avgs=[e[0], e[1].double()]), dict(params=[p[0], p[1].bfloat16()]),
           dict(avgs=[e[0], torch.zeros(14, device=DEV)[::2]], params=[p[0], torch.zeros(14, device=DEV)[::2]])]
    for change in bad:
        with pytest.raises(AssertionError):
            hip.weight_average(**dict(dict(avgs=e, params=p, w=0.5, copy=False), **change))
    with pytest.raises(HipLibraryError):
        hip.weight_average(e, [p[0], p[1].cpu()], 0.5, False)
    with pytest.raises(HipLibraryError):                           # the library's own CDDMSL_ERR_ARG
        hip.weight_average(e, p, 1.5, False)
    hip.weight_average([], [], 0.5, False)
    before = [x.clone() for x in p]
    hip.weight_average(e, p, 0.0, True)
    torch.cuda.synchronize()
    assert all(A.bits_equal(a, b) for a, b in zip(e, p)) and e[0].stride() == p[0].stride()
    q = [x + 1.0 for x in p]
    hip.weight_average(e, q, 0.25, False)
    torch.cuda.synchronize()
    assert all(torch.allclose(a, b + 0.25, atol=1e-6) for a, b in zip(e, p)) and all(A.bits_equal(a, b) for a, b in zip(p, before))


# ==================================================================================================== the tiny trainer
def _cfg(*opts):
    from cddmsl_amd.config import get_cfg
    cfg = get_cfg()
    cfg.merge_from_file(CITY_YAML)
    cfg.merge_from_list(["MODEL.COMPUTE_DTYPE", "bf16", "SOLVER.IMS_PER_BATCH", 2, "DATALOADER.NUM_WORKERS", 0, "MODEL.DEVICE", "cuda:0",
                         "SOLVER.BASE_LR", 1e-3, "SOLVER.WARMUP_ITERS", 0, "TEST.EVAL_PERIOD", 2, "DATASETS.TEST", ("bdd_100k_val",),
                         "INPUT.MIN_SIZE_TRAIN", (H,), "INPUT.MAX_SIZE_TRAIN", W, "INPUT.MIN_SIZE_TEST", H, "INPUT.MAX_SIZE_TEST", W] + list(opts))
    return cfg


def _trainer(cfg):
    from cddmsl_amd import engine, synthetic
    tr = engine.build_trainer(cfg, 2, H, W, seed=cfg.SEED)
    tr.model.load_state_dict(synthetic.make_state_dict(0, num_classes=8), strict=False)
    tr.clipcap_model.load_state_dict(synthetic.make_mapper_state_dict(1))
    return tr


@pytest.fixture(scope="module")
def trainer():
    """one trainer for the module, built with the feature on; a test sets the MODEL_EMA keys it needs and starts a new average"""
    cfg = _cfg("MODEL_EMA.ENABLED", True, "MODEL_EMA.MODE", "ema", "MODEL_EMA.DECAY", 0.5, "MODEL_EMA.START_ITER", 1)
    tr = _trainer(cfg)
    wa = tr.weight_average
    assert wa is not None and (wa.mode, wa.decay, wa.start_iter, wa.updates) == ("ema", 0.5, 1, 0)
    names = {id(p): k for k, p in tr.model.named_parameters()}
    assert wa.names == [names[id(p)] for p in tr.optimizer.params] and all(a is b for a, b in zip(wa.params, tr.optimizer.params))
    assert all(t.dtype == torch.float32 and t.stride() == p.stride() and t.device == p.device for t, p in zip(wa.tensors, wa.params))
    return tr


def _restart(tr, *opts):
    from cddmsl_amd.solver import build_weight_average
    tr.cfg.merge_from_list(["MODEL_EMA.ENABLED", True] + list(opts))
    tr.weight_average = build_weight_average(tr.cfg, tr.model, tr.optimizer)
    tr.iter, tr.storage = 0, {}
    return tr.weight_average


@pytest.mark.parametrize("mode", ["ema", "uniform"])
def test_trainer_average_follows_the_recurrence(trainer, mode):
    """5 steps, START_ITER 1: nothing at iteration 0, a copy at 1, three updates; against the float64 recurrence over the snapshots
    of the same run, with the recurrence bound; update() leaves every parameter as it was"""
    from cddmsl_amd.solver import average_weight
    tr = trainer
    wa = _restart(tr, "MODEL_EMA.MODE", mode, "MODEL_EMA.DECAY", 0.5, "MODEL_EMA.START_ITER", 1, "MODEL_EMA.EVAL", "both")
    params = tr.optimizer.params
    inner, seen = wa.update, []

    def watched(iteration):
        before = [p.detach().clone() for p in params]
        inner(iteration)
        torch.cuda.synchronize()
        assert all(torch.equal(p.detach(), b) for p, b in zip(params, before)), "update() wrote a parameter"
        seen.append((iteration, wa.updates))
    wa.update = watched
    snaps = []
    for _ in range(5):
        tr.run_step()
        torch.cuda.synchronize()
        snaps.append([p.detach().cpu().clone() for p in params])
    assert seen == [(0, 0), (1, 1), (2, 2), (3, 3), (4, 4)]
    moved = [i for i in range(len(params)) if not torch.equal(snaps[1][i], snaps[4][i])]
    assert moved, "the weights did not move: the test would compare copies"
    ws = [average_weight(mode, 0.5, n) for n in (1, 2, 3)]
    assert ws == ([0.5, 0.5, 0.5] if mode == "ema" else [1 / 2, 1 / 3, 1 / 4])
    rep = A.Report()
    for i, t in enumerate(wa.tensors):
        want, bound = A.average_sequence([s[i] for s in snaps[1:]], ws)
        rep.bound(f"trainer average {mode}", wa.names[i], t.detach().cpu(), (want, bound))
    for k, v in rep.worst.items():
        WORST[k] = max(WORST.get(k, 0.0), v)
    assert not rep.fail, "\n".join(rep.fail[:20])
    assert any(not torch.equal(t.detach().cpu(), snaps[4][i]) for i, t in enumerate(wa.tensors))


def test_evaluation_runs_both_weight_sets(trainer, tmp_path, capsys, monkeypatch):
    from cddmsl_amd import evaluation, layers
    tr = trainer
    root = str(tmp_path)
    _write_bdd(root)
    args = type("Args", (), dict(datasets_root=root, voc_root="", dt_data="", voc_split="test", voc_year=2007))()
    wa = _restart(tr, "MODEL_EMA.MODE", "ema", "MODEL_EMA.DECAY", 0.5, "MODEL_EMA.START_ITER", 0, "MODEL_EMA.EVAL", "both")
    params = tr.optimizer.params
    holds_average = []
    inner_inference = evaluation.inference_on_dataset

    def inference(model, loader, evaluator):
        holds_average.append(all(torch.equal(p.detach(), t) for p, t in zip(params, wa.tensors)))
        return inner_inference(model, loader, evaluator)
    monkeypatch.setattr(evaluation, "inference_on_dataset", inference)
    hook = _tool().build_eval_hook(tr, tr.cfg, args, 0, 1, 4)
    inner, versions = hook.eval_fn, []

    def watched(prefix):
        before = [p.detach().clone() for p in params]
        avg = [t.clone() for t in wa.tensors]
        v0 = layers.weight_version()
        res = inner(prefix)
        torch.cuda.synchronize()
        assert all(torch.equal(p.detach(), b) for p, b in zip(params, before)), "an evaluation changed the training weights"
        assert all(torch.equal(t, a) for t, a in zip(wa.tensors, avg)), "an evaluation changed the averaged weights"
        versions.append(layers.weight_version() - v0)
        return res
    hook.eval_fn = watched
    capsys.readouterr()
    for it in range(4):
        tr.run_step()
        hook.after_step(it)
        assert tr.model.training
    hook.after_train()
    out = capsys.readouterr().out
    assert hook.evaluated_at == [1, 3] and holds_average == [False, True, False, True]
    assert all(v >= 2 for v in versions) and len(versions) == 2         # bumped on entry and on exit of applied()
    for task in ("bbox", "bbox_EMA"):
        assert isinstance(tr.storage[f"bdd_100k_val/{task}/AP"], float)
        assert [k for k in tr.storage if k.startswith(f"bdd_100k_val/{task}/")] == [f"bdd_100k_val/{task}/" + k for k in
                                                                                   ["AP", "AP50", "AP75", "APs", "APm", "APl"] + ["AP-" + c for c in BDD_CLASSES]]
    lines = [l for l in out.splitlines() if "bdd_100k_val: {" in l]
    assert ["bbox_EMA" in l for l in lines] == [False, True, False, True], out       # the averaged weights' line behind the plain one
    assert [l.split("bdd_100k_val")[0] for l in lines] == ["iter 1  "] * 2 + ["iter 3  "] * 2
    # EVAL averaged: that pass alone, its keys suffixed all the same; EVAL plain: no _EMA key, the average is still kept
    for ev, want in (("averaged", [True]), ("plain", [False])):
        tr.cfg.merge_from_list(["MODEL_EMA.EVAL", ev])
        tr.storage, updates = {}, wa.updates
        del holds_average[:]
        for it in range(tr.iter, tr.iter + 2):
            tr.run_step()
            hook.after_step(it)
        assert holds_average == want and wa.updates == updates + 2
        tasks = {k.split("/")[1] for k in tr.storage if k.startswith("bdd_100k_val/")}
        assert tasks == ({"bbox_EMA"} if ev == "averaged" else {"bbox"})


def test_checkpoint_round_trip_and_eval_only(trainer, tmp_path, capsys):
    from cddmsl_amd.checkpoint import DetectionCheckpointer
    from cddmsl_amd.solver import build_weight_average
    tr = trainer
    root = str(tmp_path / "data")
    os.makedirs(root)
    _write_bdd(root)
    wa = _restart(tr, "MODEL_EMA.MODE", "ema", "MODEL_EMA.DECAY", 0.5, "MODEL_EMA.START_ITER", 0, "MODEL_EMA.EVAL", "both")
    for _ in range(3):
        tr.run_step()
    out_dir = str(tmp_path / "out")
    with_entry = DetectionCheckpointer(tr.model, out_dir, optimizer=tr.optimizer, trainer=tr, weight_average=wa).save("with_average", iteration=2)
    without = DetectionCheckpointer(tr.model, out_dir, optimizer=tr.optimizer, trainer=tr).save("without_average", iteration=2)
    data = torch.load(with_entry, map_location="cpu", weights_only=True)
    assert sorted(data) == ["iteration", "model", "optimizer", "weight_average"] and data["weight_average"]["updates"] == 3
    assert "weight_average" not in torch.load(without, map_location="cpu", weights_only=True)
    # a fresh trainer: built with the feature off it has no average; given one, it resumes the saved one bit for bit
    tr2 = _trainer(_cfg())
    assert tr2.weight_average is None
    cfg2 = _cfg("MODEL_EMA.ENABLED", True, "MODEL_EMA.DECAY", 0.5)
    wa2 = tr2.weight_average = build_weight_average(cfg2, tr2.model, tr2.optimizer)
    capsys.readouterr()
    DetectionCheckpointer(tr2.model, out_dir, optimizer=tr2.optimizer, trainer=tr2, weight_average=wa2).load(without)
    assert wa2.updates == 0 and "without_average.pth holds no averaged weights" in capsys.readouterr().out
    DetectionCheckpointer(tr2.model, out_dir, optimizer=tr2.optimizer, trainer=tr2, weight_average=wa2).load(with_entry)
    assert "no averaged weights" not in capsys.readouterr().out
    assert tr2.iter == 3 and wa2.updates == wa.updates == 3 and wa2.names == wa.names
    assert all(A.bits_equal(a, b) for a, b in zip(wa2.tensors, wa.tensors))
    assert all(A.bits_equal(a.detach(), b.detach()) for a, b in zip(tr2.optimizer.params, tr.optimizer.params))
    wa.update(3)
    wa2.update(3)
    torch.cuda.synchronize()
    assert wa2.updates == 4 and all(A.bits_equal(a, b) for a, b in zip(wa2.tensors, wa.tensors))
    assert any(not torch.equal(t, p.detach()) for t, p in zip(wa.tensors, wa.params))
    del tr2, wa2
    # --eval-only through the command line's main(): the averaged weights' line from the file that holds them, a note from the other
    tool = _tool()
    common = ["--config-file", CITY_YAML, "--eval-only", "--datasets-root", root, "--height", str(H), "--width", str(W)]
    opts = ["MODEL.COMPUTE_DTYPE", "bf16", "DATALOADER.NUM_WORKERS", "0", "SOLVER.IMS_PER_BATCH", "2", "DATASETS.TEST", "('bdd_100k_val',)", "OUTPUT_DIR", out_dir,
            "INPUT.MIN_SIZE_TEST", str(H), "INPUT.MAX_SIZE_TEST", str(W), "MODEL_EMA.ENABLED", "True", "MODEL_EMA.DECAY", "0.5"]
    for path, averaged in ((with_entry, True), (without, False)):
        capsys.readouterr()
        with pytest.raises(SystemExit) as e:
            tool.main(tool.default_argument_parser().parse_args(common + opts + ["MODEL.WEIGHTS", path]))
        out = capsys.readouterr().out
        assert e.value.code == 0
        lines = [l for l in out.splitlines() if "bdd_100k_val: {" in l]
        assert ["bbox_EMA" in l for l in lines] == ([False, True] if averaged else [False]), out
        assert (f"{path} holds no averaged weights" in out) == (not averaged), out


def test_worst_ratio_table(capsys):
    """the module's last test: the worst |err| / bound of every output the tests before it checked (shown without -s)"""
    with capsys.disabled():
        print("\n".join(["", "worst |err| / bound per output:"] + [f"  {k:44s} {WORST[k]:.3f}" for k in sorted(WORST)]))
    assert all(v <= 1.0 for v in WORST.values())
