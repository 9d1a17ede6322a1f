"""cddmsl_voc_match (cddmsl_amd/csrc/voc_match.hip) against the host walk it restates, evaluation.class_ap, BIT FOR BIT: the tp and
fp masks of every detection, on the case sets of tests/voc_match_cases.py (which tests/test_voc_eval_host.py shows to hit every
rule of the walk) and on the shapes at which the kernel takes another path; then the evaluator with ``device`` against the
evaluator without, dictionary for dictionary, ``run_eval_only_catalog`` on the VOC config's names, and the training tool with
``--datasets-root`` on a tiny VOC-family tree."""
import os

import numpy as np
import pytest
import torch

import voc_match_cases as C

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VOC_YAML = os.path.join(ROOT, "configs", "VOC-Experiments", "faster_rcnn_CLIP_R_50_C4.yaml")
DEV = "cuda:0"


def _case(name):
    def build():
        if name == "big":
            return C.random_set(9, n_images=120)
        if name.startswith("seg"):
            g, d = name[3:].split("x")
            return C.segment_case(int(g), int(d))
        return C.random_set(int(name[4:]))
    return C.cached(("case", name), build)


def _host(name):
    """the yardstick, once per case: (tp bits, fp bits) per detection from the instrumented copy of class_ap's loop"""
    return C.cached(("host", name), lambda: C.instrumented_walk(_case(name)))


def _device(case, gt=None):
    """the product's own path from gathered arrays to masks: voc_segments on the host, one hip.voc_match launch"""
    from cddmsl_amd import evaluation as E
    from cddmsl_amd import hip
    b, s, cls, img = C.flat_dets(case)
    _, perm, seg_off, seg_gt = E.voc_segments(cls, img, E.voc_round_scores(s), range(C.NUM_CLASSES), len(case["names"]))
    gt = gt or hip.VocGroundTruth.from_host(C.gt_rows(case), [t / 100.0 for t in C.THRS], DEV)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    tp, fp, bad = hip.voc_match(up(b), up(perm), up(seg_off), up(seg_gt), gt)
    assert tp.dtype == fp.dtype == torch.int16 and bad.dtype == torch.int32 and not bad.any()
    return tp.cpu().numpy().view(np.uint16), fp.cpu().numpy().view(np.uint16), len(seg_gt)


@pytest.mark.parametrize("name", ["seed0", "seed1", "seed2", "big"])
def test_masks_equal_the_host_walk(name):
    tp, fp, nseg = _device(_case(name))
    want_tp, want_fp = _host(name)
    assert np.array_equal(tp, want_tp) and np.array_equal(fp, want_fp)
    assert want_tp.any() and want_fp.any() and not (want_tp & want_fp).any() and (want_tp | want_fp).max() < 1 << 10
    if name == "big":
        assert nseg >= 200                                   # a few hundred segments in one launch


@pytest.mark.parametrize("n_gt,n_det", [(0, 1), (0, 70), (1, 1), (1, 2), (2, 70), (63, 70), (64, 2), (64, 70), (65, 70), (130, 2), (130, 70)])
def test_edge_shapes_of_one_segment(n_gt, n_det):
    """one segment in the launch: no box, one, the 64 lanes one short / full / one over, three strides; one, two and 70 detections"""
    name = f"seg{n_gt}x{n_det}"
    tp, fp, nseg = _device(_case(name))
    want_tp, want_fp = _host(name)
    assert nseg == 1 and len(tp) == n_det
    assert np.array_equal(tp, want_tp) and np.array_equal(fp, want_fp)
    if n_gt == 0:
        assert not tp.any() and (fp == 0x3FF).all()          # no ground truth: best = -inf, a false positive at every threshold


def test_text_rounding_decides_the_mask():
    """The kernel's rounding where it shows: a 1000 x 1 box, so the overlap is the detection's rounded width / 1000, and a ladder of 16
    thresholds 0.0001 apart -- rounding a ``.x5`` tie the other way, or adding the + 1 in f64 instead of f32, moves the overlap across a
    step.  One detection per segment, each with its own copy of the box; expected from the f-string round trip and class_ap's expressions."""
    from cddmsl_amd import hip
    x1 = np.concatenate([np.arange(41, 47, 2) / 4.0, [10.35, 10.45, 11.0, 11.65]])               # 10.25, 10.75, 11.25: ties
    x0 = np.array([0.05, 0.15, 0.25, 0.35, 0.45, 0.0, 0.75])                                       # 0.05f + 1.0f = 1.04999995 -> "1.0"
    b = np.concatenate([np.stack([np.zeros_like(x1), np.zeros_like(x1), x1, np.ones_like(x1)], axis=1),
                        np.stack([x0, np.zeros_like(x0), np.full_like(x0, 11.5), np.ones_like(x0)], axis=1)]).astype(np.float32)
    n = len(b)
    thrs = np.array([(10.25 + 0.1 * k) / 1000.0 for k in range(16)])
    gtb = np.array([[1.0, 1.0, 1000.0, 1.0]])
    want = np.zeros(n, dtype=np.uint16)
    for i, (a0, a1, a2, a3) in enumerate(b):
        bb = np.array([float(f"{a0 + 1:.1f}"), float(f"{a1 + 1:.1f}"), float(f"{a2:.1f}"), float(f"{a3:.1f}")])
        iw = np.maximum(np.minimum(gtb[:, 2], bb[2]) - np.maximum(gtb[:, 0], bb[0]) + 1.0, 0.0)
        ih = np.maximum(np.minimum(gtb[:, 3], bb[3]) - np.maximum(gtb[:, 1], bb[1]) + 1.0, 0.0)
        inter = iw * ih
        union = (bb[2] - bb[0] + 1.0) * (bb[3] - bb[1] + 1.0) + (gtb[:, 2] - gtb[:, 0] + 1.0) * (gtb[:, 3] - gtb[:, 1] + 1.0) - inter
        ov = (inter / union)[0]
        want[i] = sum(1 << t for t in range(16) if ov > thrs[t])
    assert len(set(want.tolist())) >= 8 and want[0] == 0 and want[n - len(x0)] != want[n - len(x0) + 1]      # the ladder resolves them
    gt = hip.VocGroundTruth.from_host([(gtb, np.zeros(1, dtype=bool))] * n, thrs, DEV)
    ar = torch.arange(n + 1, dtype=torch.int64, device=DEV)
    tp, fp, bad = hip.voc_match(torch.from_numpy(b).to(DEV), ar[:n].clone(), ar, ar[:n].clone(), gt)
    tp, fp = tp.cpu().numpy().view(np.uint16), fp.cpu().numpy().view(np.uint16)
    assert not bad.any() and np.array_equal(tp, want) and np.array_equal(fp, ~want)


def test_no_detections_and_unlisted_detections():
    """zero detections (no segment: nothing is launched) and detections no segment lists (their masks stay 0)"""
    from cddmsl_amd import hip
    case = C.segment_case(5, 0)
    gt = hip.VocGroundTruth.from_host(C.gt_rows(case), [t / 100.0 for t in C.THRS], DEV)
    e = lambda n, dt: torch.zeros(n, dtype=dt, device=DEV)
    tp, fp, bad = hip.voc_match(torch.zeros((0, 4), device=DEV), e(0, torch.int64), e(1, torch.int64), e(0, torch.int64), gt)
    assert tp.numel() == fp.numel() == bad.numel() == 0
    case = _case("seed0")
    b, _, _, _ = C.flat_dets(case)
    tp, fp, bad = hip.voc_match(torch.from_numpy(b).to(DEV), e(0, torch.int64), e(1, torch.int64), e(0, torch.int64),
                                hip.VocGroundTruth.from_host(C.gt_rows(case), [t / 100.0 for t in C.THRS], DEV))
    assert len(tp) == len(b) and not tp.any() and not fp.any()
    with pytest.raises(TypeError, match="f32"):
        hip.voc_match(torch.from_numpy(b).double().to(DEV), e(0, torch.int64), e(1, torch.int64), e(0, torch.int64), gt)


def test_two_runs_byte_for_byte():
    from cddmsl_amd import hip
    case = _case("big")
    gt = hip.VocGroundTruth.from_host(C.gt_rows(case), [t / 100.0 for t in C.THRS], DEV)
    first = _device(case, gt)
    other = _device(_case("seed1"))                          # the workspace is used by another set in between
    second = _device(case, gt)
    assert first[0].tobytes() == second[0].tobytes() and first[1].tobytes() == second[1].tobytes()
    assert len(other[0]) != len(first[0])


# ------------------------------------------------------------------------------------------------ the evaluator
def _tree(tmp_path_factory, name):
    def build():
        from cddmsl_amd.evaluation import VOC_CLASS_NAMES
        d = str(tmp_path_factory.mktemp("voc_" + name))
        C.write_voc_tree(d, "test", _case(name), VOC_CLASS_NAMES)
        return d
    return C.cached(("tree", name), build)


def _evaluate(dirname, year, case, device, images=None):
    from cddmsl_amd import evaluation as E
    ev = E.PascalVOCDetectionEvaluator(dirname, "test", year, device=device)
    for i, (inputs, outputs) in enumerate(C.instances_of(case, DEV if device else "cpu")):
        if images is None or i in images:
            ev.process(inputs, outputs)
    return ev


@pytest.mark.parametrize("year", [2007, 2012])
def test_device_evaluator_equals_host_evaluator(tmp_path_factory, year):
    case, d = _case("seed0"), _tree(tmp_path_factory, "seed0")
    with np.errstate(invalid="ignore", divide="ignore"):
        host = C.cached(("host_eval", year), lambda: _evaluate(d, year, case, None).evaluate())
        ev = _evaluate(d, year, case, DEV)
        dev = ev.evaluate()
        assert C.same_results(dev, host), (dev, host)
        assert C.same_results(ev.evaluate(), host)           # evaluate() leaves the evaluator's state alone
        ev.reset()
        empty = ev.evaluate()                                # no detections at all: every class's AP is 0 on both paths
        assert C.same_results(empty, _evaluate(d, year, case, None, images=()).evaluate())
    assert 0 < host["bbox"]["AP50-present"] < 100 and np.isnan(host["bbox"]["AP"]) == (year == 2012)


def test_two_half_evaluators_merge_in_rank_order(tmp_path_factory):
    """what rank 0 does with two ranks' records: rank order, then processing order -- the order of the host path's merged lists"""
    from cddmsl_amd import evaluation as E
    case, d = _case("seed0"), _tree(tmp_path_factory, "seed0")
    n = len(case["names"])
    with np.errstate(invalid="ignore", divide="ignore"):
        host = C.cached(("host_eval", 2012), lambda: _evaluate(d, 2012, case, None).evaluate())
        a, b = _evaluate(d, 2012, case, DEV, images=range(0, n // 2)), _evaluate(d, 2012, case, DEV, images=range(n // 2, n))
        merged = E.merge_voc_records([a._device_records(), b._device_records()])
        assert len(merged[0]) == sum(len(x[1]) for x in case["dets"])
        assert C.same_results(a.evaluate_records(merged), host)


def test_process_checks_its_inputs(tmp_path_factory):
    case, d = _case("seed0"), _tree(tmp_path_factory, "seed0")
    from cddmsl_amd import evaluation as E
    ev = E.PascalVOCDetectionEvaluator(d, "test", 2007, device=DEV)
    inputs, outputs = C.instances_of(case, DEV)[1]
    with pytest.raises(KeyError):
        ev.process([{"image_id": "not_in_the_set"}], outputs)
    inst = outputs[0]["instances"]
    inst.pred_boxes.tensor = inst.pred_boxes.tensor.double()
    with pytest.raises(TypeError, match="f32"):
        ev.process(inputs, outputs)


# ------------------------------------------------------------------------------------------------ the catalog, with a model
def test_catalog_runs_the_voc_config_names(tmp_path, capsys):
    """DATASETS.TEST ("voc_2007_test", "Clipart1k_test") on a tiny tree with the synthetic model: both sets come back, and the values
    are those of a host evaluator fed with the very detections the model returned"""
    from cddmsl_amd import evaluation as E
    from cddmsl_amd import synthetic
    from cddmsl_amd.config import get_cfg
    from cddmsl_amd.modeling import build_model
    from cddmsl_amd.structures import Boxes, Instances
    root = str(tmp_path)
    cases = {"voc_2007_test": ("VOC2007", 2007, C.tiny_set(3, prefix="c")), "Clipart1k_test": ("clipart", 2012, C.tiny_set(4, prefix="d"))}
    for sub, _, case in cases.values():
        C.write_voc_tree(os.path.join(root, sub), "test", case, E.VOC_CLASS_NAMES, images=True)
    cfg = get_cfg()
    cfg.merge_from_file(VOC_YAML)
    cfg.merge_from_list(["MODEL.COMPUTE_DTYPE", "bf16", "MODEL.DEVICE", DEV, "DATASETS.TEST", ("voc_2007_test", "Clipart1k_test", "Comic_test"),
                         "INPUT.MIN_SIZE_TEST", 128, "INPUT.MAX_SIZE_TEST", 160, "MODEL.ROI_HEADS.SCORE_THRESH_TEST", 0.0])
    inner = build_model(cfg)
    inner.load_state_dict(synthetic.make_state_dict(0), strict=False)
    seen = {}

    class Recording(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.module = inner

        def forward(self, inputs):
            outputs = self.module(inputs)
            for inp, out in zip(inputs, outputs):
                i = out["instances"]
                seen[str(inp["image_id"])] = (i.image_size, i.pred_boxes.tensor.cpu().clone(), i.scores.cpu().clone(), i.pred_classes.cpu().clone())
            return outputs

    with np.errstate(invalid="ignore", divide="ignore"):
        res = E.run_eval_only_catalog(Recording(), cfg, root, return_results=True)
        out = capsys.readouterr().out
        assert list(res) == ["voc_2007_test", "Clipart1k_test"] and f"skipping Comic_test: {root}/comic/ImageSets/Main/test.txt not found" in out
        assert "voc_2007_test: {'AP': " in out and "Clipart1k_test: {'AP': " in out
        assert sum(len(v[2]) for v in seen.values()) > 10, "degenerate case: nothing detected"
        for name, (sub, year, case) in cases.items():
            host = E.PascalVOCDetectionEvaluator(os.path.join(root, sub), "test", year)
            for n in case["names"]:
                size, b, s, c = seen[n]
                host.process([{"image_id": n}], [{"instances": Instances(size, pred_boxes=Boxes(b), scores=s, pred_classes=c)}])
            assert C.same_results(res[name], host.evaluate()), name
            assert "AP50-present" in res[name]["bbox"] and "AP-present" in res[name]["bbox"]


def test_tool_trains_and_evaluates_the_voc_config_by_name(tmp_path, capsys, monkeypatch):
    """tools/train_caption_consistency.py --datasets-root on the tiny family tree: both DATASETS.TRAIN sets reach the paired loader in
    the order named, and TEST.EVAL_PERIOD evaluates the VOC-family DATASETS.TEST names that are on disk"""
    import importlib.util
    from cddmsl_amd import data
    spec = importlib.util.spec_from_file_location("train_caption_consistency", os.path.join(ROOT, "tools", "train_caption_consistency.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    root = str(tmp_path)
    cases = C.write_family(root)
    handed = []
    build = data.build_detection_train_loader
    monkeypatch.setattr(data, "build_detection_train_loader", lambda cfg, dicts, *a, **k: handed.append(dicts) or build(cfg, dicts, *a, **k))
    opts = ["SOLVER.IMS_PER_BATCH", "2", "INPUT.MIN_SIZE_TRAIN", "(128,)", "INPUT.MAX_SIZE_TRAIN", "160", "INPUT.MIN_SIZE_TEST", "128",
            "INPUT.MAX_SIZE_TEST", "160", "SOLVER.CHECKPOINT_PERIOD", "0", "OUTPUT_DIR", str(tmp_path / "out"), "DATALOADER.NUM_WORKERS", "0",
            "MODEL.RPN.PRE_NMS_TOPK_TRAIN", "300", "MODEL.RPN.POST_NMS_TOPK_TRAIN", "100", "MODEL.RPN.PRE_NMS_TOPK_TEST", "300",
            "MODEL.RPN.POST_NMS_TOPK_TEST", "50", "MODEL.ROI_HEADS.BATCH_SIZE_PER_IMAGE", "32", "TEST.DETECTIONS_PER_IMAGE", "20",
            "TEST.EVAL_PERIOD", "2"]
    with np.errstate(invalid="ignore", divide="ignore"):
        tool.main(tool.default_argument_parser().parse_args(["--config-file", VOC_YAML, "--datasets-root", root, "--max-iter", "2"] + opts))
    out = capsys.readouterr().out
    assert len(handed) == 1 and [d["image_id"] for d in handed[0]] == cases["VOC2007"]["names"] + cases["VOC2012"]["names"]
    assert all("dt_clipart" in d["data_dt_file_name"] for d in handed[0])
    assert "iter 1  voc_2007_test: {'AP': " in out and "iter 1  Clipart1k_test: {'AP': " in out and "'AP50-present': " in out
    assert f"iter 1  skipping Watercolor_test: {root}/watercolor/ImageSets/Main/test.txt not found" in out
    assert f"iter 1  skipping Comic_test: {root}/comic/ImageSets/Main/test.txt not found" in out
    assert out.count("voc_2007_test: {") == 1                      # period 2 over 2 iterations: once, not again after the last
