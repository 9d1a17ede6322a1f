"""CPU: Cityscapes / Foggy Cityscapes input side and the COCO-style box evaluator -- split listing and pairing on a tiny tree, the
annotation rules applied to kernel records, the crowd filters of the training input, and COCO AP cases worked out by hand."""
import os

import numpy as np
import pytest
import torch

BETAS = ("0.005", "0.01", "0.02")


def write_city_tree(root, frames, seed=0):
    """``frames``: {split: [(city, stem, instance-id map uint16 [H,W])]} -> ``root/cityscapes/{leftImg8bit, leftImg8bit_foggy,
    gtFine}`` as in the Cityscapes + Foggy Cityscapes downloads (clear frame, three foggy betas, 16-bit instanceIds png)."""
    from PIL import Image
    rng = np.random.RandomState(seed)
    for split, items in frames.items():
        for city, stem, inst in items:
            h, w = inst.shape
            dirs = {k: os.path.join(root, "cityscapes", k, split, city) for k in ("leftImg8bit", "leftImg8bit_foggy", "gtFine")}
            for d in dirs.values():
                os.makedirs(d, exist_ok=True)
            img = rng.randint(0, 256, (h, w, 3), dtype=np.uint8)
            Image.fromarray(img).save(os.path.join(dirs["leftImg8bit"], stem + "_leftImg8bit.png"))
            for beta in BETAS:
                fog = (img.astype(np.float32) * 0.6 + 100).astype(np.uint8)
                Image.fromarray(fog).save(os.path.join(dirs["leftImg8bit_foggy"], f"{stem}_leftImg8bit_foggy_beta_{beta}.png"))
            Image.fromarray(inst.astype(np.uint16)).save(os.path.join(dirs["gtFine"], stem + "_gtFine_instanceIds.png"))
    return root


def _tiny_tree(tmp_path):
    m = np.zeros((8, 16), dtype=np.uint16)
    frames = {"train": [(c, f"{c}_{i:06d}_000019", m) for c in ("zurich", "aachen") for i in (3, 1)],
              "val": [("frankfurt", "frankfurt_000000_000294", m), ("frankfurt", "frankfurt_000000_000001", m)]}
    return write_city_tree(str(tmp_path), frames)


def test_listing_sorted_and_paired(tmp_path):
    from cddmsl_amd import cityscapes as cs
    root = _tiny_tree(tmp_path)
    img, dt, gt = (os.path.join(root, d) for d in cs.SPLITS["cityscapes_DG_train"])
    files = cs.list_cityscapes_files(img, dt, gt)
    stems = [os.path.basename(f[0])[: -len("_leftImg8bit.png")] for f in files]
    assert stems == ["aachen_000001_000019", "aachen_000003_000019", "zurich_000001_000019", "zurich_000003_000019"]
    for image_file, twin, inst in files:
        city, stem = os.path.basename(os.path.dirname(image_file)), os.path.basename(image_file)[: -len("_leftImg8bit.png")]
        assert twin == os.path.join(dt, city, stem + "_leftImg8bit_foggy_beta_0.02.png") and os.path.exists(twin)
        assert inst == os.path.join(gt, city, stem + "_gtFine_instanceIds.png") and os.path.exists(inst)


def test_foggy_val_lists_every_beta_with_its_ground_truth(tmp_path):
    from cddmsl_amd import cityscapes as cs
    root = _tiny_tree(tmp_path)
    img, dt, gt = (None if d is None else os.path.join(root, d) for d in cs.SPLITS["cityscapes_foggy_val"])
    assert dt is None
    files = cs.list_cityscapes_files(img, dt, gt)
    assert len(files) == 2 * len(BETAS)
    names = [os.path.basename(f[0]) for f in files]
    assert names == sorted(names) and all(f[1] is None for f in files)
    for image_file, _, inst in files:
        stem = os.path.basename(image_file).split("leftImg8bit_foggy")[0]
        assert inst == os.path.join(gt, "frankfurt", stem + "gtFine_instanceIds.png") and os.path.exists(inst)
    clear = cs.list_cityscapes_files(*(None if d is None else os.path.join(root, d) for d in cs.SPLITS["cityscapes_val"]))
    assert [f[2] for f in clear] == [f[2] for f in files[:: len(BETAS)]]


def test_split_names():
    from cddmsl_amd import cityscapes as cs
    assert set(cs.SPLITS) == {"cityscapes_DG_train", "cityscapes_DG_val", "cityscapes_val", "cityscapes_foggy_val"}
    assert not cs.is_cityscapes("cityscapes_DG_test") and not cs.is_cityscapes("bdd_100k_val")
    with pytest.raises(KeyError):
        cs.load_cityscapes("cityscapes_DG_test", "/nonexistent")


def test_annotations_from_records():
    from cddmsl_amd import cityscapes as cs
    recs = np.array([[24, 1, 2, 5, 6, 10],            # person crowd region
                     [26, 0, 0, 0, 9, 10],            # car crowd, zero width -> skipped
                     [7005, 0, 0, 3, 3, 16],          # road (stuff) -> dropped
                     [26001, 3, 4, 9, 8, 30],         # car
                     [29000, 0, 0, 9, 9, 50],         # caravan: ignored in evaluation -> dropped
                     [30001, 0, 0, 9, 9, 50],         # trailer -> dropped
                     [31002, 2, 2, 3, 3, 4],          # train
                     [33000, 1, 1, 1, 4, 4]],         # bicycle, single column -> skipped
                    dtype=np.int32)
    a = cs.annotations_from_records(recs)
    assert [(x["category_id"], x["iscrowd"]) for x in a] == [(0, True), (2, False), (5, False)]
    assert a[1]["bbox"] == [3.0, 4.0, 9.0, 8.0] and a[1]["area"] == 30.0
    with pytest.raises(KeyError):
        cs.annotations_from_records(np.array([[500, 0, 0, 2, 2, 9]], dtype=np.int32))     # label 500: id2label raises


def test_crowd_only_images_are_filtered_and_crowd_boxes_dropped(tmp_path):
    from PIL import Image
    from cddmsl_amd import cityscapes as cs
    from cddmsl_amd.config import get_cfg
    from cddmsl_amd.data import DatasetMapper
    crowd = {"iscrowd": True, "category_id": 0, "bbox": [0.0, 0.0, 4.0, 4.0], "area": 16.0}
    real = {"iscrowd": False, "category_id": 2, "bbox": [2.0, 2.0, 10.0, 6.0], "area": 30.0}
    dicts = [{"image_id": "a", "annotations": [crowd]}, {"image_id": "b", "annotations": [crowd, real]}, {"image_id": "c", "annotations": []}]
    assert [d["image_id"] for d in cs.filter_images_with_only_crowd_annotations(dicts)] == ["b"]
    p = str(tmp_path / "x.png")
    Image.fromarray(np.zeros((8, 16, 3), dtype=np.uint8)).save(p)
    cfg = get_cfg()
    cfg.merge_from_list(["INPUT.MIN_SIZE_TRAIN", "(0,)", "INPUT.RANDOM_FLIP", "none"])
    out = DatasetMapper(cfg, True, np.random.RandomState(0))({"file_name": p, "height": 8, "width": 16, "annotations": [crowd, real]})
    assert out["instances"].gt_classes.tolist() == [2]
    assert out["instances"].gt_boxes.tensor.tolist() == [[2.0, 2.0, 10.0, 6.0]]


# ------------------------------------------------------------------------------------------------ COCO-style box AP by hand
CLASSES = ("person", "rider", "car")


def _gt(image_id, anns):
    return {"image_id": image_id, "annotations": [{"bbox": list(map(float, b)), "category_id": c, "iscrowd": cr,
                                                   "area": float(ar if ar is not None else (b[2] - b[0]) * (b[3] - b[1]))}
                                                  for b, c, cr, ar in anns]}


def _evaluate(dicts, dets):
    """dets: {image_id: [(xyxy, score, class)]}"""
    from cddmsl_amd.evaluation import COCODetectionEvaluator
    from cddmsl_amd.structures import Boxes, Instances
    ev = COCODetectionEvaluator(dicts, CLASSES)
    for d in dicts:
        ds = dets.get(d["image_id"], [])
        inst = Instances((1000, 1000), pred_boxes=Boxes(torch.tensor([x[0] for x in ds], dtype=torch.float32).reshape(-1, 4)),
                         scores=torch.tensor([x[1] for x in ds], dtype=torch.float32),
                         pred_classes=torch.tensor([x[2] for x in ds], dtype=torch.int64))
        ev.process([{"image_id": d["image_id"]}], [{"instances": inst}])
    return ev.evaluate()["bbox"]


def test_coco_perfect_detections():
    small, medium, large = (10, 10, 30, 30), (100, 100, 150, 150), (200, 200, 400, 300)
    dicts = [_gt("a", [(small, 0, False, None), (large, 2, False, None)]), _gt("b", [(medium, 0, False, None), (small, 2, False, None)])]
    dets = {"a": [(small, 0.9, 0), (large, 0.8, 2)], "b": [(medium, 0.7, 0), (small, 0.6, 2)]}
    r = _evaluate(dicts, dets)
    for k in ("AP", "AP50", "AP75", "APs", "APm", "APl", "AP-person", "AP-car"):
        assert r[k] == pytest.approx(100.0), (k, r[k])
    assert np.isnan(r["AP-rider"])
    assert list(r)[:6] == ["AP", "AP50", "AP75", "APs", "APm", "APl"] and len(r) == 6 + len(CLASSES)


def test_coco_false_positive_ranked_first_halves_ap():
    box = (100, 100, 200, 200)
    r = _evaluate([_gt("a", [(box, 1, False, None)])], {"a": [((500, 500, 600, 600), 0.9, 1), (box, 0.8, 1)]})
    assert r["AP"] == pytest.approx(50.0) and r["AP50"] == pytest.approx(50.0)


def test_coco_iou_062():
    r = _evaluate([_gt("a", [((0, 0, 100, 100), 0, False, None)])], {"a": [((0, 0, 100, 62), 0.9, 0)]})
    assert r["AP50"] == pytest.approx(100.0) and r["AP75"] == pytest.approx(0.0) and r["AP"] == pytest.approx(30.0)


def test_coco_detection_on_crowd_region_changes_nothing():
    box, crowd = (100, 100, 200, 200), (300, 300, 700, 700)
    dicts = [_gt("a", [(box, 0, False, None), (crowd, 0, True, None)])]
    base = _evaluate(dicts, {"a": [(box, 0.5, 0)]})
    with_hit = _evaluate(dicts, {"a": [(box, 0.5, 0), ((350, 350, 450, 450), 0.95, 0)]})
    assert repr(base) == repr(with_hit) and with_hit["AP"] == pytest.approx(100.0)
    # the same detection without the crowd region is a false positive ranked first
    assert _evaluate([_gt("a", [(box, 0, False, None)])], {"a": [(box, 0.5, 0), ((350, 350, 450, 450), 0.95, 0)]})["AP"] == pytest.approx(50.0)


def test_coco_only_top_100_detections_per_image_count():
    box = (0, 0, 50, 50)
    fps = [((100 + 5 * i, 100, 140 + 5 * i, 140), 0.9 - 0.001 * i, 0) for i in range(100)]
    dicts = [_gt("a", [(box, 0, False, None)])]
    assert _evaluate(dicts, {"a": fps + [(box, 0.1, 0)]})["AP"] == pytest.approx(0.0)           # true positive ranked 101st
    assert _evaluate(dicts, {"a": fps[:99] + [(box, 0.1, 0)]})["AP"] > 0.0                      # ranked 100th: it counts


def test_coco_area_is_the_stored_area():
    box = (0, 0, 40, 40)                       # 1600 px^2 box, but a 900-pixel mask: small
    r = _evaluate([_gt("a", [(box, 0, False, 900)])], {"a": [(box, 0.9, 0)]})
    assert r["APs"] == pytest.approx(100.0) and np.isnan(r["APm"]) and np.isnan(r["APl"]) and r["AP"] == pytest.approx(100.0)


def test_coco_no_detections_is_nan():
    r = _evaluate([_gt("a", [((0, 0, 50, 50), 0, False, None)])], {})
    assert set(r) >= {"AP", "AP50", "AP75", "APs", "APm", "APl"} and all(np.isnan(v) for v in r.values())
