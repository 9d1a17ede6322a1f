"""GPU: the instance-box kernel (cddmsl_instance_boxes) bit-exact against a numpy restatement of the reference's per-id scan, and
the Cityscapes -> Foggy Cityscapes benchmark end to end on a generated tree of 128x256 frames: dataset dicts, three training steps
of the AdverseWeather config on the real paired loader, ``--eval-only --datasets-root`` through the CLI, and ground truth fed back
as detections."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CITY_YAML = os.path.join(ROOT, "configs", "AdverseWeather-Experiments", "faster_rcnn_CLIP_R_50_C4.yaml")


def restated_records(inst_image):
    """data/datasets/cityscapes.py:501-540 restated: np.unique over ids >= 24, then per id a full-image compare + np.nonzero ->
    (id, xmin, ymin, xmax, ymax, npixels) for every id (the kernel reports them all; the annotation rules come after)."""
    out = []
    for iid in np.unique(inst_image[inst_image >= 24]):
        mask = np.asarray(inst_image == iid, dtype=np.uint8, order="F")
        ys, xs = np.nonzero(mask)
        out.append((int(iid), int(xs.min()), int(ys.min()), int(xs.max()), int(ys.max()), int(mask.sum())))
    return np.array(out, dtype=np.int32).reshape(-1, 6)


def blob_map(rng, h, w, n, ids=None):
    """stuff ids 0..23 in blocks, then ``n`` rectangles with ragged edges painted in order (later ones overwrite earlier ones)"""
    m = rng.randint(0, 24, (h // 8 + 1, w // 8 + 1)).repeat(8, 0).repeat(8, 1)[:h, :w].astype(np.int32)
    if ids is None:
        pool = list(range(24, 34)) + [k * 1000 + j for k in range(24, 34) for j in range(40)] + [7005, 11002, 23999]
        ids = rng.choice(pool, n)
    for iid in ids:
        y0, x0 = rng.randint(0, h), rng.randint(0, w)
        y1, x1 = min(h, y0 + rng.randint(1, max(2, h // 3))), min(w, x0 + rng.randint(1, max(2, w // 3)))
        region = rng.rand(y1 - y0, x1 - x0) < 0.85
        m[y0:y1, x0:x1][region] = iid
    return m


def _kernel(maps, dtype=torch.uint16):
    from cddmsl_amd import hip
    host = np.ascontiguousarray(maps, dtype=np.uint16 if dtype == torch.uint16 else np.int32)
    return hip.instance_boxes_host(torch.from_numpy(host).cuda())


def _check(maps, dtype=torch.uint16):
    got = _kernel(maps, dtype)
    assert len(got) == len(maps)
    for m, g in zip(maps, got):
        want = restated_records(m)
        assert g.dtype == np.int32 and g.shape == want.shape and np.array_equal(g, want), (g[:5], want[:5])
    return got


def test_kernel_random_blob_maps():
    rng = np.random.RandomState(0)
    for h, w, n in ((128, 256, 40), (53, 37, 12), (257, 129, 80)):      # 53 x 37: rows that do not align with a thread's 8 pixels
        m = blob_map(rng, h, w, n)
        _check(m[None], torch.uint16)
        _check(m[None], torch.int32)
    neg = blob_map(rng, 64, 96, 20)
    neg[::7, ::5] = -1                                                  # int32 maps: negative ids are below 24 and skipped
    _check(neg[None], torch.int32)


def test_kernel_single_pixel_and_single_row_instances():
    from cddmsl_amd import cityscapes as cs
    m = np.zeros((40, 70), dtype=np.int32)
    m[5, 9] = 26001                # single pixel
    m[12, 3:60] = 24002            # single row
    m[20:31, 44] = 33007           # single column
    m[0, 0] = 25                   # crowd single pixel in a corner
    m[30:35, 10:20] = 27003
    got = _check(m[None])[0]
    assert [r[0] for r in got] == [25, 24002, 26001, 27003, 33007]
    kept = cs.annotations_from_records(got)     # the reference's `xmax <= xmin or ymax <= ymin` drops all but the 5x10 truck
    assert [(a["category_id"], a["bbox"]) for a in kept] == [(3, [10.0, 30.0, 19.0, 34.0])]


def test_kernel_full_size_map_touching_borders():
    rng = np.random.RandomState(1)
    m = blob_map(rng, 1024, 2048, 60)
    m[0, 100:300] = 26010          # top row
    m[-1, 500:900] = 26011         # bottom row
    m[200:600, 0] = 24010          # left column
    m[300:1024, -1] = 24011        # right column
    m[-3:, -3:] = 33020            # bottom-right corner
    _check(m[None])


def test_kernel_many_instances_and_no_instances():
    rng = np.random.RandomState(2)
    ids = rng.permutation([k * 1000 + j for k in range(24, 34) for j in range(60)])[:512]
    m = blob_map(rng, 256, 512, 0)
    for n, iid in enumerate(ids):                     # a 16 x 32 grid of 16 x 16 cells, one ragged instance in each
        y, x = (n // 32) * 16, (n % 32) * 16
        m[y:y + 16, x:x + 16][rng.rand(16, 16) < 0.5] = iid
    got = _check(m[None])[0]
    assert len(got) == 512
    empty = rng.randint(0, 24, (96, 160))
    assert _check(empty[None])[0].shape == (0, 6)


def test_kernel_batch_and_repeatability():
    rng = np.random.RandomState(3)
    maps = np.stack([blob_map(rng, 160, 320, n) for n in (0, 5, 50, 200)])
    a = _check(maps)
    b = _kernel(maps)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    from cddmsl_amd import hip
    dev = torch.from_numpy(maps.astype(np.uint16)).cuda()
    r1, c1 = hip.instance_boxes(dev)
    r2, c2 = hip.instance_boxes(dev)
    assert torch.equal(c1, c2) and all(torch.equal(r1[i, :n], r2[i, :n]) for i, n in enumerate(c1.tolist()))


def test_kernel_rejects_ids_without_a_label():
    from cddmsl_amd._lib import HipLibraryError
    m = np.zeros((2, 32, 48), dtype=np.int32)
    m[0, 3:5, 3:5] = 26001
    m[1, 10, 10] = 40000
    with pytest.raises(HipLibraryError, match="status 1"):
        _kernel(m)


# ------------------------------------------------------------------------------------------------ end to end on a fixture tree
H, W = 128, 256


def _frame(rng, n, crowd_only=False):
    if crowd_only:
        m = rng.randint(0, 24, (H, W)).astype(np.int32)
        m[20:60, 30:90] = 26               # a car crowd region, nothing else
        m[70:100, 150:200] = 24
        return m
    ids = list(rng.choice([24, 26, 33], 1)) + [k * 1000 + j for k, j in zip(rng.choice([24, 25, 26, 27, 28, 29, 30, 31, 32, 33], n), range(n))]
    return blob_map(rng, H, W, len(ids), ids=ids)


@pytest.fixture(scope="module")
def city_root(tmp_path_factory):
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from test_cityscapes_host import write_city_tree
    rng = np.random.RandomState(7)
    frames = {"train": [("bochum", "bochum_000000_000313", _frame(rng, 6)), ("bochum", "bochum_000000_001097", _frame(rng, 0, True)),
                        ("aachen", "aachen_000000_000019", _frame(rng, 8)), ("aachen", "aachen_000001_000019", _frame(rng, 5)),
                        ("zurich", "zurich_000000_000019", _frame(rng, 7))],
              "val": [("frankfurt", "frankfurt_000000_000294", _frame(rng, 6)), ("lindau", "lindau_000000_000019", _frame(rng, 9))]}
    return write_city_tree(str(tmp_path_factory.mktemp("datasets")), frames), frames


def _restated_dicts(files):
    from cddmsl_amd import cityscapes as cs
    from cddmsl_amd.cityscapes import read_instance_map
    out = []
    for image_file, twin, inst in files:
        m = read_instance_map(inst)
        d = {"file_name": image_file, "image_id": os.path.basename(image_file), "height": m.shape[0], "width": m.shape[1]}
        if twin is not None:
            d["data_dt_file_name"] = twin
        d["annotations"] = cs.annotations_from_records(restated_records(m))
        out.append(d)
    return out


def test_dataset_dicts_match_restatement(city_root):
    from cddmsl_amd import cityscapes as cs
    root, _ = city_root
    for name in ("cityscapes_DG_train", "cityscapes_DG_val", "cityscapes_val", "cityscapes_foggy_val"):
        dicts = cs.load_cityscapes(name, root)
        files = cs.list_cityscapes_files(*(None if d is None else os.path.join(root, d) for d in cs.SPLITS[name]))
        assert dicts == _restated_dicts(files), name
        assert all((d["height"], d["width"]) == (H, W) for d in dicts)
    train = cs.load_cityscapes("cityscapes_DG_train", root)
    assert any(a["iscrowd"] for d in train for a in d["annotations"]) and any(not a["iscrowd"] for d in train for a in d["annotations"])
    assert {a["category_id"] for d in train for a in d["annotations"]} <= set(range(8))
    assert all(os.path.exists(d["data_dt_file_name"]) for d in train)


def test_three_training_steps_on_the_paired_loader(city_root):
    from cddmsl_amd import cityscapes as cs, data, engine, synthetic
    from cddmsl_amd.config import get_cfg
    root, _ = city_root
    cfg = get_cfg()
    cfg.merge_from_file(CITY_YAML)
    cfg.merge_from_list(["MODEL.COMPUTE_DTYPE", "bf16", "SOLVER.IMS_PER_BATCH", 2, "DATALOADER.NUM_WORKERS", 0, "MODEL.DEVICE", "cuda:0"])
    assert cfg.DATASETS.TRAIN[0] == "cityscapes_DG_train" and cfg.MODEL.KD_REGULRAZIATION
    tr = engine.build_trainer(cfg, 2, seed=cfg.SEED)
    tr.model.load_state_dict(synthetic.make_state_dict(0, num_classes=8), strict=False)
    tr.clipcap_model.load_state_dict(synthetic.make_mapper_state_dict(1))
    dicts = cs.filter_images_with_only_crowd_annotations(cs.load_cityscapes("cityscapes_DG_train", root))
    assert len(dicts) == 4 and not any("001097" in d["file_name"] for d in dicts)
    tr.data_loader = data.build_detection_train_loader(cfg, dicts, 2, 0, 1, cfg.MODEL.DEVICE)
    seen = []

    def recording(it):
        for batch in it:
            seen.extend(d["file_name"] for d in batch)
            yield batch
    tr._data_loader_iter = recording(iter(tr.data_loader))
    tr.iter = 20000                               # past burn-in: every branch and the KD loss are live
    for _ in range(3):
        losses = tr.run_step()
        tr.iter += 1
        assert {"kd_loss", "cont_loss", "cont_region_loss"} <= set(losses), sorted(losses)
        assert all(np.isfinite(float(v.detach())) for v in losses.values()), losses
    torch.cuda.synchronize()
    tr.data_loader.close()
    assert len(seen) == 6 and not any("001097" in f for f in seen)


def test_eval_only_cli_on_foggy_val(city_root, tmp_path):
    root, _ = city_root
    cmd = ["timeout", "-k", "10", "900", sys.executable, os.path.join(ROOT, "tools", "train_caption_consistency.py"), "--config-file",
           CITY_YAML, "--eval-only", "--datasets-root", root, "MODEL.COMPUTE_DTYPE", "bf16", "DATALOADER.NUM_WORKERS", "0",
           "OUTPUT_DIR", str(tmp_path / "out")]
    p = subprocess.run(cmd, cwd=str(tmp_path), capture_output=True, text=True)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    out = p.stdout
    assert "skipping bdd_100k_val" in out
    line = [l for l in out.splitlines() if l.startswith("cityscapes_foggy_val: {")]
    assert len(line) == 1 and re.search(r"cityscapes_foggy_val: 6 images", out), out
    keys = re.findall(r"'([A-Za-z0-9-]+)':", line[0])
    from cddmsl_amd.cityscapes import THING_CLASSES
    assert keys == ["AP", "AP50", "AP75", "APs", "APm", "APl"] + ["AP-" + c for c in THING_CLASSES], keys
    assert any(l.startswith("cityscapes_val: {") for l in out.splitlines())


def test_ground_truth_as_detections_scores_100(city_root):
    from cddmsl_amd import cityscapes as cs
    from cddmsl_amd.evaluation import COCODetectionEvaluator
    from cddmsl_amd.structures import Boxes, Instances
    root, _ = city_root
    dicts = cs.load_cityscapes("cityscapes_foggy_val", root)
    ev = COCODetectionEvaluator(dicts, cs.THING_CLASSES)
    ev.reset()
    for d in dicts:
        anns = [a for a in d["annotations"] if not a["iscrowd"]]
        inst = Instances((d["height"], d["width"]), pred_boxes=Boxes(torch.tensor([a["bbox"] for a in anns], dtype=torch.float32).reshape(-1, 4).cuda()),
                         scores=torch.linspace(1.0, 0.5, len(anns)).cuda(), pred_classes=torch.tensor([a["category_id"] for a in anns]).cuda())
        ev.process([{"image_id": d["image_id"]}], [{"instances": inst}])
    r = ev.evaluate()["bbox"]
    assert r["AP"] == pytest.approx(100.0) and r["AP50"] == pytest.approx(100.0) and r["AP75"] == pytest.approx(100.0)
    present = {cs.THING_CLASSES[a["category_id"]] for d in dicts for a in d["annotations"] if not a["iscrowd"]}
    assert all(r["AP-" + c] == pytest.approx(100.0) for c in present) and len(present) >= 3
