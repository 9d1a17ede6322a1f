"""tests/exact_soft_nms.py tied to the reference before it judges a kernel (CPU only).

tests/golden/ref_soft_nms.npz holds what the reference's own layers/soft_nms.py (batched_soft_nms) and its
fast_rcnn_inference_single_image with soft_nms_enabled=True returned on every case (tests/golden/make_golden_soft_nms.py): the numpy
references must reproduce it -- linear and hard bit for bit, gaussian with equal indices and scores within the derived bound.  The
negative controls show that the cases see the bugs they are there for, the margins that no gaussian decision hangs on expf's last
bit, and the last tests cover the config keys and the host wiring (they fail without the feature)."""
import os

import numpy as np
import pytest

import exact_soft_nms as X

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_soft_nms.npz"))
NAMES = [c["name"] for c in X.cases()]
GAUSS = [c["name"] for c in X.cases() if c["method"] == "gaussian"]


def _scores_ok(method, got, ref, bound):
    if method != "gaussian":
        return np.array_equal(got, ref)
    return bool((np.abs(got.astype(np.float64) - ref.astype(np.float64)) <= bound).all())


@pytest.mark.parametrize("name", NAMES)
def test_reference_reproduces_the_fixture(name):
    c, r = X.case(name), X.expected(name)
    chk = np.asarray([c["boxes"].astype(np.float64).sum(), c["scores"].astype(np.float64).sum(), float(c["idxs"].sum())])
    assert np.array_equal(chk, GOLD[f"sum/{name}"]), "the case builder no longer produces the inputs the fixture was made from"
    assert np.array_equal(r["keep"], GOLD[f"keep/{name}"]), (name, r["keep"][:12].tolist(), GOLD[f"keep/{name}"][:12].tolist())
    assert GOLD[f"scores/{name}"].dtype == np.float32
    assert _scores_ok(c["method"], GOLD[f"scores/{name}"], r["scores"], r["bound"]), name


@pytest.mark.parametrize("name", NAMES)
def test_per_category_walks_equal_the_single_walk(name):
    """the kernel's factorisation, capped per category, is the first max_keep entries of the reference's one walk -- bit for bit,
    gaussian included (both sides use the same exp here)"""
    c = X.case(name)
    p = X.per_category_ref(c["boxes"], c["scores"], c["idxs"], c["method"], c["sigma"], c["thr"], c["prune"], c["max_keep"])
    assert X.same(p, X.expected(name)), name


def test_max_keep_is_a_prefix_of_the_uncapped_result():
    full = X.expected("clustered300_s0_linear")
    for c in X.cases():
        if c["name"].startswith("max_keep_") and c["method"] == "linear":
            r = X.expected(c["name"])
            mk = c["max_keep"]
            assert np.array_equal(r["keep"], full["keep"][:mk]) and np.array_equal(r["scores"], full["scores"][:mk]), c["name"]
    assert {len(X.expected(f"max_keep_{mk}")["keep"]) for mk in (0, 1, 7)} == {0, 1, 7}


@pytest.mark.parametrize("name,variant", [(c["name"], v) for c in X.cases() for v in c["controls"]])
def test_negative_control_differs(name, variant):
    assert not X.same(X.control(name, variant), X.expected(name)), (name, variant)


def test_every_control_is_exercised():
    assert {v for c in X.cases() for v in c["controls"]} == {"sort_once", "no_shift", "tie_high", "prune_ge", "no_arrival_prune"}


def test_scores_that_start_below_prune():
    """the reference's first pick prunes every category: a category's own top is not kept when it starts at or below prune"""
    for m in X.METHODS:
        assert X.expected(f"category_top_below_prune_{m}")["keep"].tolist() == [0]
        assert X.control(f"category_top_below_prune_{m}", "no_arrival_prune")["keep"].tolist() == [0, 1]
    assert X.expected("all_below_prune")["keep"].tolist() == [1]
    assert X.expected("below_prune_is_global_top")["keep"].tolist() == [0]


def test_rerank_order():
    assert X.expected("rerank")["keep"].tolist() == [0, 2, 1]
    assert X.control("rerank", "sort_once")["keep"].tolist() == [0, 1, 2]


def test_strict_comparisons():
    """IoU == thr: linear leaves the score, hard suppresses (torchvision's NMS, iou > thr, would keep it); score == prune is dropped"""
    lin, hard = X.expected("iou_equals_thr_linear"), X.expected("iou_equals_thr_hard")
    assert lin["keep"].tolist() == [0, 1] and lin["scores"].tolist() == [np.float32(0.9), np.float32(0.8)]
    assert hard["keep"].tolist() == [0]
    assert X.expected("decayed_equals_prune")["keep"].tolist() == [0]
    assert X.expected("decayed_one_step_above_prune")["keep"].tolist() == [0, 1]
    assert X.expected("decayed_one_step_above_prune")["scores"][1] == np.float32(X.case("decayed_equals_prune")["prune"])


@pytest.mark.parametrize("name", GAUSS)
def test_gaussian_margins(name):
    """every arg-max decision and every prune decision of the reference lies >= MARGIN bounds from flipping; no case is excused"""
    m = X.expected(name)["margin"]
    print(f"{name}: smallest margin {m:.3g} bounds")
    assert m >= X.MARGIN, (name, m)


def test_structure_sizes_are_covered():
    ks = {len(c["scores"]) for c in X.cases() if len(np.unique(c["idxs"])) == 1}
    assert {1, X.WAVE - 1, X.WAVE, X.WAVE + 1, X.BLOCK, X.BLOCK + 1, X.LDS_CAP, X.LDS_CAP + 1} <= ks
    assert any(len(c["scores"]) == X.TOTAL_CAP for c in X.cases())
    assert any(len(np.unique(c["idxs"])) > X.GRID for c in X.cases())


# ------------------------------------------------------------------------------------------------------------ inference
@pytest.mark.parametrize("name", list(X.inference_configs()))
def test_inference_reference_reproduces_the_fixture(name):
    inp, cfg = X.inference_inputs(), X.inference_configs()[name]
    assert np.array_equal(inp["boxes"], GOLD["inf/boxes"], equal_nan=True) and np.array_equal(inp["scores"], GOLD["inf/scores"])
    r = X.inference_ref(inp, cfg)
    assert np.array_equal(r["pred_boxes"], GOLD[f"inf/{name}/pred_boxes"])
    assert np.array_equal(r["pred_classes"], GOLD[f"inf/{name}/pred_classes"])
    assert np.array_equal(r["kept"], GOLD[f"inf/{name}/kept"])
    assert _scores_ok(cfg["method"], GOLD[f"inf/{name}/scores"], r["scores"], r["bound"])
    assert r["margin"] >= X.MARGIN
    assert len(r["kept"]) > 0 and (r["kept_rows"] != r["kept"]).any(), "the dropped rows must shift the numbering"


# ------------------------------------------------------------------------------------------------------------ config, wiring
def test_config_carries_the_reference_defaults():
    from cddmsl_amd.config import get_cfg
    r = get_cfg().MODEL.ROI_HEADS
    assert (r.SOFT_NMS_ENABLED, r.SOFT_NMS_METHOD, r.SOFT_NMS_SIGMA, r.SOFT_NMS_PRUNE) == (False, "gaussian", 0.5, 0.001)


def _cfg(*opts):
    from cddmsl_amd.config import get_cfg
    cfg = get_cfg()
    cfg.merge_from_file(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "configs", "VOC-Experiments",
                                     "faster_rcnn_CLIP_R_50_C4.yaml"))
    cfg.merge_from_list(list(opts))
    return cfg


def test_merging_the_switch_builds_the_predictor():
    from cddmsl_amd.modeling.roi_heads import FastRCNNOutputLayers
    from cddmsl_amd.structures import ShapeSpec
    cfg = _cfg("MODEL.ROI_HEADS.SOFT_NMS_ENABLED", True, "MODEL.ROI_HEADS.SOFT_NMS_METHOD", "linear", "MODEL.ROI_HEADS.SOFT_NMS_PRUNE", 0.01,
               "MODEL.CLIP.TEXT_EMB_PATH", "")
    p = FastRCNNOutputLayers(cfg, ShapeSpec(channels=2048, height=1, width=1))
    assert (p.soft_nms_enabled, p.soft_nms_method, p.soft_nms_sigma, p.soft_nms_prune) == (True, "linear", 0.5, 0.01)
    off = FastRCNNOutputLayers(_cfg("MODEL.CLIP.TEXT_EMB_PATH", ""), ShapeSpec(channels=2048, height=1, width=1))
    assert off.soft_nms_enabled is False


def test_unknown_method_raises():
    from cddmsl_amd.modeling.roi_heads import FastRCNNOutputLayers, batched_soft_nms
    from cddmsl_amd.structures import ShapeSpec
    cfg = _cfg("MODEL.ROI_HEADS.SOFT_NMS_ENABLED", True, "MODEL.ROI_HEADS.SOFT_NMS_METHOD", "quadratic", "MODEL.CLIP.TEXT_EMB_PATH", "")
    with pytest.raises(NotImplementedError, match="quadratic soft nms method not implemented."):
        FastRCNNOutputLayers(cfg, ShapeSpec(channels=2048, height=1, width=1))
    import torch
    with pytest.raises(NotImplementedError, match="quadratic soft nms method not implemented."):
        batched_soft_nms(torch.zeros(2, 4), torch.zeros(2), torch.zeros(2, dtype=torch.int64), "quadratic", 0.5, 0.5, 0.001)


def test_empty_input_needs_no_gpu():
    import torch
    from cddmsl_amd.modeling.roi_heads import batched_soft_nms
    k, s = batched_soft_nms(torch.zeros(0, 4), torch.zeros(0), torch.zeros(0, dtype=torch.int64), "linear", 0.5, 0.5, 0.001)
    assert k.dtype == torch.int64 and s.dtype == torch.float32 and k.numel() == s.numel() == 0
