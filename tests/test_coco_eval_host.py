"""Host half of the COCO evaluation on records (CPU only): ``coco_accumulate`` fed with the host matcher's flags is EXACTLY
``coco_precision``; the case sets of tests/coco_match_cases.py hit every rule of the walk; the COCO-json reader
(cddmsl_amd/coco_json.py) and how ``run_eval_only_catalog`` treats ``bdd_100k_val``."""
import json
import os
import types

import numpy as np
import pytest

import coco_match_cases as C


def _host_records(dicts, dets):
    from cddmsl_amd import evaluation as E
    parts = []
    with np.errstate(invalid="ignore", divide="ignore"):
        for i, (gt, dt) in enumerate(zip(C.gt_tuples(dicts), C.dt_tuples(dets))):
            rank, matched, ignored = E.coco_match_host(gt, dt, C.NUM_CLASSES)
            keep = rank >= 0
            parts.append({"score": dt[1][keep], "cls": dt[2][keep], "img": np.full(int(keep.sum()), i, dtype=np.int64), "rank": rank[keep],
                          "matched": matched[keep], "ignored": ignored[keep]})
    return parts


def _coco_precision(dicts, dets):
    from cddmsl_amd import evaluation as E
    gt = {d["image_id"]: g for d, g in zip(dicts, C.gt_tuples(dicts))}
    dt = {d["image_id"]: t for d, t in zip(dicts, C.dt_tuples(dets))}
    with np.errstate(invalid="ignore", divide="ignore"):
        return E.coco_precision(gt, dt, C.NUM_CLASSES)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_case_sets_hit_every_rule(seed):
    count = C.cached(("rules", seed), lambda: C.rule_counters(*C.random_set(seed)))
    print(f"seed {seed}: {count}")
    assert all(count[k] > 0 for k in C.COUNTERS), count
    dicts, dets = C.random_set(seed)
    assert max(int((d[2] == 1).sum()) for d in dets) == 130           # more than COCO_MAX_DETS detections of one class in one image


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_accumulate_equals_coco_precision(seed):
    from cddmsl_amd import evaluation as E
    dicts, dets = C.random_set(seed)
    parts = _host_records(dicts, dets)
    ref = C.cached(("prec", seed), lambda: _coco_precision(dicts, dets))
    npig = E.coco_gt_counts(C.gt_tuples(dicts), C.NUM_CLASSES)
    got = E.coco_accumulate(E.merge_coco_records(parts), npig, C.NUM_CLASSES)
    assert got.shape == ref.shape == (10, 101, C.NUM_CLASSES, 4) and got.dtype == ref.dtype
    assert np.array_equal(got, ref)
    assert (ref > -1).any() and (ref[ref > -1] > 0).any() and (ref[ref > -1] < 1).any()
    # the records' order does not matter: shuffled, and merged from two halves as rank 0 merges its ranks' shards
    rec = E.merge_coco_records(parts)
    perm = np.random.RandomState(seed).permutation(len(rec["score"]))
    assert np.array_equal(E.coco_accumulate({k: v[perm] for k, v in rec.items()}, npig, C.NUM_CLASSES), ref)
    halves = [E.merge_coco_records(parts[1::2]), E.merge_coco_records(parts[0::2])]
    assert np.array_equal(E.coco_accumulate(E.merge_coco_records(halves), npig, C.NUM_CLASSES), ref)


def test_accumulate_without_detections_or_ground_truth():
    from cddmsl_amd import evaluation as E
    dicts, dets = C.random_set(0)
    npig = E.coco_gt_counts(C.gt_tuples(dicts), C.NUM_CLASSES)
    none = [C._empty_dets() for _ in dets]
    assert np.array_equal(E.coco_accumulate(E.empty_coco_records(), npig, C.NUM_CLASSES), _coco_precision(dicts, none))
    no_gt = [dict(d, annotations=[]) for d in dicts]
    parts = _host_records(no_gt, dets)
    got = E.coco_accumulate(E.merge_coco_records(parts), E.coco_gt_counts(C.gt_tuples(no_gt), C.NUM_CLASSES), C.NUM_CLASSES)
    assert np.array_equal(got, _coco_precision(no_gt, dets)) and (got == -1).all()


def test_host_evaluator_unchanged_without_device():
    """``device=None`` (and a CPU device) is the evaluator as it was: host copies, ``coco_precision``"""
    import torch
    from cddmsl_amd import evaluation as E
    from cddmsl_amd.structures import Boxes, Instances
    dicts, dets = C.random_set(1)
    names = ["a", "b", "c"]
    res = []
    for dev in (None, "cpu"):
        ev = E.COCODetectionEvaluator(dicts, names, device=dev)
        assert ev.device is None
        for d, (b, s, c) in zip(dicts, dets):
            inst = Instances((d["height"], d["width"]), pred_boxes=Boxes(torch.from_numpy(b)), scores=torch.from_numpy(s), pred_classes=torch.from_numpy(c))
            ev.process([{"image_id": d["image_id"]}], [{"instances": inst}])
        with np.errstate(invalid="ignore", divide="ignore"):
            res.append(ev.evaluate()["bbox"])
    prec = C.cached(("prec", 1), lambda: _coco_precision(dicts, dets))
    p = prec[:, :, :, 0]
    assert res[0]["AP"] == float(np.mean(p[p > -1])) * 100 and res[0] == res[1]
    assert list(res[0]) == ["AP", "AP50", "AP75", "APs", "APm", "APl", "AP-a", "AP-b", "AP-c"]


# ------------------------------------------------------------------------------------------------ the COCO-json reader
def _write_json(path, ignore=False):
    cats = [{"id": 7, "name": "car"}, {"id": 3, "name": "person"}, {"id": 5, "name": "rider"}]            # unsorted, not contiguous
    images = [{"id": 30, "file_name": "c.png", "height": 128, "width": 160}, {"id": 10, "file_name": "a.png", "height": 128, "width": 160},
              {"id": 20, "file_name": "b.png", "height": 128, "width": 160}]                            # unsorted; image 20 has no annotation
    anns = [{"id": 1, "image_id": 30, "category_id": 7, "bbox": [10.5, 20.25, 30.1, 40.7], "area": 900.0, "iscrowd": 0},
            {"id": 2, "image_id": 10, "category_id": 3, "bbox": [1, 2, 30, 40], "iscrowd": 0},                                 # no "area"
            {"id": 3, "image_id": 10, "category_id": 5, "bbox": [50, 60, 20, 10], "area": 150.0, "iscrowd": 1},                # a crowd region
            {"id": 4, "image_id": 30, "category_id": 3, "bbox": [0.1, 0.2, 0.3, 0.4], "area": 0.12},                           # no "iscrowd"
            {"id": 5, "image_id": 99, "category_id": 3, "bbox": [0, 0, 1, 1], "area": 1.0, "iscrowd": 0}]                      # no such image
    if ignore:
        anns[0]["ignore"] = 1
    with open(path, "w") as f:
        json.dump({"categories": cats, "images": images, "annotations": anns}, f)


def test_load_coco_json(tmp_path):
    from cddmsl_amd.coco_json import load_coco_json
    path = str(tmp_path / "val.json")
    _write_json(path)
    dicts, classes = load_coco_json(path, "/data/img")
    assert classes == ["person", "rider", "car"]
    assert [d["image_id"] for d in dicts] == [10, 20, 30] and [d["file_name"] for d in dicts] == ["/data/img/a.png", "/data/img/b.png", "/data/img/c.png"]
    assert all((d["height"], d["width"]) == (128, 160) for d in dicts)
    a, b, c = (d["annotations"] for d in dicts)
    assert b == []
    assert a == [{"bbox": [1.0, 2.0, 31.0, 42.0], "area": 1200.0, "iscrowd": False, "category_id": 0},
                 {"bbox": [50.0, 60.0, 70.0, 70.0], "area": 150.0, "iscrowd": True, "category_id": 1}]
    assert c == [{"bbox": [10.5, 20.25, 10.5 + 30.1, 20.25 + 40.7], "area": 900.0, "iscrowd": False, "category_id": 2},
                 {"bbox": [0.1, 0.2, 0.1 + 0.3, 0.2 + 0.4], "area": 0.12, "iscrowd": False, "category_id": 0}]
    assert all(type(x["iscrowd"]) is bool for d in dicts for x in d["annotations"])


def test_load_coco_json_refuses_ignore(tmp_path):
    from cddmsl_amd.coco_json import load_coco_json
    path = str(tmp_path / "val.json")
    _write_json(path, ignore=True)
    with pytest.raises(ValueError, match="ignore"):
        load_coco_json(path, "img")


def test_json_dicts_feed_the_evaluator(tmp_path):
    """ground truth from the reader scores 100 against itself; the image without annotations is kept and its detection counts"""
    import torch
    from cddmsl_amd import evaluation as E
    from cddmsl_amd.coco_json import load_coco_json
    from cddmsl_amd.structures import Boxes, Instances
    path = str(tmp_path / "val.json")
    _write_json(path)
    dicts, classes = load_coco_json(path, "img")

    def run(extra):
        ev = E.COCODetectionEvaluator(dicts, classes)
        for d in dicts:
            anns = [a for a in d["annotations"] if not a["iscrowd"]]
            b = [a["bbox"] for a in anns] + ([[5.0, 5.0, 50.0, 50.0]] if extra and not d["annotations"] else [])
            c = [a["category_id"] for a in anns] + ([0] if extra and not d["annotations"] else [])
            inst = Instances((128, 160), pred_boxes=Boxes(torch.tensor(b, dtype=torch.float64).reshape(-1, 4)),
                             scores=torch.linspace(0.9, 0.8, len(b)), pred_classes=torch.tensor(c, dtype=torch.int64))
            ev.process([{"image_id": d["image_id"]}], [{"instances": inst}])
        with np.errstate(invalid="ignore", divide="ignore"):
            return ev.evaluate()["bbox"]
    assert run(False)["AP50"] == pytest.approx(100.0)
    worse = run(True)                         # a 0.9-score false positive of class "person" on the empty image, ahead of one true one
    assert worse["AP-person"] < 100.0 and worse["AP-car"] == pytest.approx(run(False)["AP-car"])


# ------------------------------------------------------------------------------------------------ the catalog
def _cfg(tests):
    from cddmsl_amd.config import get_cfg
    cfg = get_cfg()
    cfg.merge_from_list(["DATASETS.TEST", tuple(tests), "MODEL.DEVICE", "cpu"])
    return cfg


def test_catalog_names():
    from cddmsl_amd import cityscapes, coco_json
    assert coco_json.is_coco_json("bdd_100k_val") and not coco_json.is_coco_json("cityscapes_val") and not cityscapes.is_cityscapes("bdd_100k_val")
    assert coco_json.coco_json_paths("bdd_100k_val", "/d") == ("/d/bdd100k/images/100k/val.json", "/d/bdd100k/images/100k/data")


def test_bdd_skipped_when_the_json_is_missing(tmp_path, capsys):
    from cddmsl_amd import evaluation as E
    res = E.run_eval_only_catalog(object(), _cfg(["bdd_100k_val", "no_such_set"]), str(tmp_path), return_results=True)
    out = capsys.readouterr().out
    assert res == {}
    assert f"skipping bdd_100k_val: {tmp_path}/bdd100k/images/100k/val.json not found" in out
    assert "skipping no_such_set: not in the dataset catalog" in out


def test_bdd_class_count_mismatch_raises(tmp_path, monkeypatch):
    from cddmsl_amd import evaluation as E
    os.makedirs(tmp_path / "bdd100k" / "images" / "100k")
    _write_json(str(tmp_path / "bdd100k" / "images" / "100k" / "val.json"))
    monkeypatch.setattr(E, "num_test_classes", lambda model, cfg: 8)
    with pytest.raises(ValueError, match=r"3 classes.*\b8\b"):
        E.run_eval_only_catalog(object(), _cfg(["bdd_100k_val"]), str(tmp_path))


def test_periodic_eval_schedule_and_storage():
    """EvalHook's schedule on a stub trainer: period 2 over 4 iterations -> after iterations 1 and 3, nothing more at the end; period 3
    over 4 -> after iteration 2 and once more after the last; the flattened values land in the storage; the model's mode, its
    generators, torch's generator and the shared-pass cache come back as they were"""
    import torch
    from cddmsl_amd import evaluation as E

    class Model(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.region_generator = torch.Generator().manual_seed(5)
            self.roi_heads = types.SimpleNamespace(sample_generator=torch.Generator().manual_seed(6))
            self.proposal_generator = types.SimpleNamespace(sample_generator=torch.Generator().manual_seed(7))
            self._shared = {"stale": 1}

    for period, n, expect in ((2, 4, [1, 3]), (3, 4, [2, 3]), (0, 4, [])):
        tr = types.SimpleNamespace(model=Model().train(), storage={})
        seen = []

        def fn(prefix, tr=tr, seen=seen):
            assert tr.model._shared is None
            seen.append(prefix)
            tr.model.eval()
            tr.model._shared = {"from": "eval"}
            torch.rand(3)
            torch.randperm(5, generator=tr.model.region_generator)
            torch.randperm(5, generator=tr.model.roi_heads.sample_generator)
            return {"bdd_100k_val": {"bbox": {"AP": 1.5, "AP50": float("nan")}}}
        hook = E.PeriodicEval(tr, period, fn, n)
        before = (torch.get_rng_state().clone(), tr.model.region_generator.get_state().clone(), tr.model.roi_heads.sample_generator.get_state().clone())
        for it in range(n):
            hook.after_step(it)
        hook.after_train()
        assert hook.evaluated_at == expect and seen == [f"iter {i}  " for i in expect]
        assert tr.model.training
        assert torch.equal(before[0], torch.get_rng_state()) and torch.equal(before[1], tr.model.region_generator.get_state())
        assert torch.equal(before[2], tr.model.roi_heads.sample_generator.get_state())
        if expect:
            assert tr.model._shared is None
            assert tr.storage["bdd_100k_val/bbox/AP"] == 1.5 and np.isnan(tr.storage["bdd_100k_val/bbox/AP50"])
        else:
            assert tr.storage == {}
