"""Periodic evaluation during training (TEST.EVAL_PERIOD, the reference's hooks.EvalHook) on a tiny trainer: synthetic weights, three
128x160 PNGs and a BDD-style COCO json in tmp_path.  Period 2 over 4 iterations evaluates after iterations 1 and 3 and not a third
time at the end, the AP values land in ``tr.storage``, and training goes on exactly as in a run without the hook.  The learning rate
is 0 so that both runs see the same weights whatever the order of a backward pass' additions: what differs can only come from
the evaluations."""
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CITY_YAML = os.path.join(ROOT, "configs", "AdverseWeather-Experiments", "faster_rcnn_CLIP_R_50_C4.yaml")
BDD_CLASSES = ["pedestrian", "rider", "car", "truck", "bus", "train", "motorcycle", "bicycle"]
H, W = 128, 160


def _write_bdd(root):
    from PIL import Image
    rng = np.random.RandomState(11)
    data = os.path.join(root, "bdd100k", "images", "100k", "data")
    os.makedirs(data)
    images, anns = [], []
    for i in range(3):
        name = f"frame{i}.png"
        Image.fromarray(rng.randint(0, 256, (H, W, 3)).astype(np.uint8)).save(os.path.join(data, name))
        images.append({"id": 100 - i, "file_name": name, "height": H, "width": W})
        for j in range(3):
            x, y, w, h = int(rng.randint(0, 80)), int(rng.randint(0, 60)), int(rng.randint(20, 70)), int(rng.randint(20, 60))
            anns.append({"id": len(anns) + 1, "image_id": 100 - i, "category_id": int(rng.randint(1, 9)), "bbox": [x, y, w, h], "area": w * h, "iscrowd": 0})
    with open(os.path.join(root, "bdd100k", "images", "100k", "val.json"), "w") as f:
        json.dump({"categories": [{"id": k + 1, "name": n} for k, n in enumerate(BDD_CLASSES)][::-1], "images": images, "annotations": anns}, f)


def _tool():
    spec = importlib.util.spec_from_file_location("train_caption_consistency", os.path.join(ROOT, "tools", "train_caption_consistency.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_eval_period_evaluates_and_leaves_training_alone(tmp_path, capsys):
    from cddmsl_amd import coco_json, data, engine, synthetic
    from cddmsl_amd.config import get_cfg
    root = str(tmp_path)
    _write_bdd(root)
    cfg = get_cfg()
    cfg.merge_from_file(CITY_YAML)
    cfg.merge_from_list(["MODEL.COMPUTE_DTYPE", "bf16", "SOLVER.IMS_PER_BATCH", 2, "DATALOADER.NUM_WORKERS", 0, "MODEL.DEVICE", "cuda:0",
                         "SOLVER.BASE_LR", 0.0, "TEST.EVAL_PERIOD", 2, "DATASETS.TEST", ("bdd_100k_val",),
                         "INPUT.MIN_SIZE_TRAIN", (H,), "INPUT.MAX_SIZE_TRAIN", W, "INPUT.MIN_SIZE_TEST", H, "INPUT.MAX_SIZE_TEST", W])
    tr = engine.build_trainer(cfg, 2, H, W, seed=cfg.SEED)
    tr.model.load_state_dict(synthetic.make_state_dict(0, num_classes=8), strict=False)
    tr.clipcap_model.load_state_dict(synthetic.make_mapper_state_dict(1))
    dicts, classes = coco_json.load_coco_json(*coco_json.coco_json_paths("bdd_100k_val", root))
    assert classes == BDD_CLASSES and [d["image_id"] for d in dicts] == [98, 99, 100]
    train_dicts = [dict(d, data_dt_file_name=d["file_name"]) for d in dicts]
    args = type("Args", (), dict(datasets_root=root, voc_root="", dt_data="", voc_split="test", voc_year=2007))()
    model = tr.model
    gens = (model.proposal_generator.sample_generator, model.roi_heads.sample_generator, model.region_generator)

    def run(with_hook):
        for k, g in enumerate(gens):
            g.manual_seed(100 + k)
        torch.manual_seed(5)
        tr.iter, tr.storage = 0, {}
        tr.data_loader = data.build_detection_train_loader(cfg, train_dicts, 2, 0, 1, cfg.MODEL.DEVICE)
        seen = []

        def recording(it):
            for batch in it:
                seen.append([os.path.basename(d["file_name"]) for d in batch])
                yield batch
        tr._data_loader_iter = recording(iter(tr.data_loader))
        hook = _tool().build_eval_hook(tr, cfg, args, 0, 1, 4) if with_hook else None
        around = []
        if hook is not None:
            inner = hook.eval_fn

            def watched(prefix):
                assert model._shared is None
                before = [g.get_state().clone() for g in gens]
                res = inner(prefix)
                around.append((before, [g.get_state().clone() for g in gens]))
                return res
            hook.eval_fn = watched
        for it in range(4):
            tr.run_step()
            if hook is not None:
                hook.after_step(it)
                assert model.training and model._shared is None
        if hook is not None:
            hook.after_train()
        nxt = next(tr._data_loader_iter)
        torch.cuda.synchronize()
        state = ([g.get_state().clone() for g in gens], torch.get_rng_state().clone(), torch.cuda.get_rng_state().clone(), model.training,
                 [os.path.basename(d["file_name"]) for d in nxt], seen, dict(tr.storage))
        tr.data_loader.close()
        return state, hook, around

    plain, _, _ = run(False)
    capsys.readouterr()
    hooked, hook, around = run(True)
    out = capsys.readouterr().out
    assert hook.evaluated_at == [1, 3]                             # after iterations 1 and 3; the last one is not evaluated twice
    lines = [l for l in out.splitlines() if "bdd_100k_val: {" in l]
    assert [l.split("bdd_100k_val")[0] for l in lines] == ["iter 1  ", "iter 3  "], out
    assert out.count("bdd_100k_val: 3 images") == 2
    keys = ["AP", "AP50", "AP75", "APs", "APm", "APl"] + ["AP-" + c for c in BDD_CLASSES]
    assert [k for k in hooked[6] if k.startswith("bdd_100k_val/")] == ["bdd_100k_val/bbox/" + k for k in keys]
    assert all(isinstance(hooked[6]["bdd_100k_val/bbox/" + k], float) for k in keys)
    assert not any(k.startswith("bdd_100k_val/") for k in plain[6])
    # the evaluations drew from the samplers' generators or they did not: either way the states are put back
    assert len(around) == 2
    for a, b in zip(plain[0], hooked[0]):
        assert torch.equal(a, b)
    assert torch.equal(plain[1], hooked[1]) and torch.equal(plain[2], hooked[2])
    assert plain[3] is True and hooked[3] is True
    assert plain[4] == hooked[4] and plain[5] == hooked[5] and len(plain[5]) == 5
