"""Generates tests/golden/ref_openset.npz by running the REFERENCE's own FastRCNNOutputLayers (modeling/roi_heads/fast_rcnn.py)
in eval mode with an open-set test vocabulary: ``openset_test=(None, <file>, 0.01, 0.5)``, ``cls_agnostic_bbox_reg=True``, K_train =
5, K_test = 37, D = 64, on R = 70 seeded region features (tests/openset_ref.py's ``fixture_inputs``: two-class mixtures whose scores
are spaced by more than any f32 implementation's error, so the ORDER of the detections is defined).  Reuses the make_golden.py
harness (reference leaf modules imported with their package __init__s bypassed, its stand-in for torchvision's batched_nms).
Recorded: the features, the test embeddings (un-normalised, as a checkpoint holds them), bbox_pred, the proposals, the scores and
deltas of ``forward``, the boxes of ``predict_boxes`` and what ``inference`` returns with ``multiply_rpn_score`` off and on
(soft-NMS off).  Only arrays are written.

usage:  python tests/golden/make_golden_openset.py
"""
import importlib
import os
import sys
import tempfile

import numpy as np
import torch

import make_golden as mg

sys.path.insert(0, os.path.join(mg.ROOT, "tests"))
import openset_ref as X  # noqa: E402

F = X.FIXTURE
K_TRAIN, K_TEST, D, R, SEED = 5, F["K"], F["D"], F["R"], F["seed"]
SCORE_THRESH, NMS_THRESH, TOPK = F["thresh"], F["nms"], F["topk"]


def main():
    mg.setup()
    fr = importlib.import_module("detectron2.modeling.roi_heads.fast_rcnn")
    br = importlib.import_module("detectron2.modeling.box_regression")
    L, S = sys.modules["detectron2.layers"], sys.modules["detectron2.structures"]
    inp = X.fixture_inputs()
    assert X.fixture_condition(inp) and X.fixture_first_seed() == SEED
    g = torch.Generator().manual_seed(SEED)
    emb = torch.from_numpy(inp["wn"]) * (0.5 + 2.0 * torch.rand(K_TEST, 1, generator=g))      # rows of any length: forward normalises
    out = {"feats": inp["x"], "test_emb": emb.numpy(), "image_size": np.asarray([X.IMG_H, X.IMG_W])}
    pboxes = torch.from_numpy(inp["boxes"]).clone()
    pboxes[7, 2] = float("inf")                                                               # a row the finite-row filter drops
    objectness = torch.from_numpy(inp["obj"])
    out["proposal_boxes"], out["objectness"] = pboxes.numpy(), objectness.numpy()
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "test_emb.pth")
        torch.save(emb, path)
        for name, mult in (("plain", False), ("rpn", True)):
            pred = fr.FastRCNNOutputLayers(
                L.ShapeSpec(channels=D, height=1, width=1), box2box_transform=br.Box2BoxTransform(weights=(10.0, 10.0, 5.0, 5.0)),
                num_classes=K_TRAIN, test_score_thresh=SCORE_THRESH, test_nms_thresh=NMS_THRESH, soft_nms_enabled=False,
                test_topk_per_image=TOPK, cls_agnostic_bbox_reg=True, clip_cls_emb=(True, None, "CLIPRes5ROIHeads", D),
                bg_cls_loss_weight=None, multiply_rpn_score=(mult, False), openset_test=(None, path, 0.01, 0.5))
            assert pred.test_cls_score.weight.shape == (K_TEST, D) and pred.bbox_pred.weight.shape == (4, D)
            with torch.no_grad():
                pred.cls_score.weight.copy_(mg.seeded((K_TRAIN, D), 51))
                pred.bbox_pred.weight.copy_(mg.seeded((4, D), 52, 0.05))
                pred.bbox_pred.bias.copy_(mg.seeded((4,), 53, 0.1))
            pred.eval()
            inst = S.Instances((X.IMG_H, X.IMG_W))
            inst.proposal_boxes, inst.objectness_logits = S.Boxes(pboxes), objectness
            with torch.no_grad():
                scores, deltas = pred(torch.from_numpy(inp["x"]))
                boxes = pred.predict_boxes((scores, deltas), [inst])[0]
                res, kept = pred.inference((scores, deltas), [inst])
            assert scores.shape == (R, K_TEST + 1) and deltas.shape == (R, 4) and float(scores[:, -1].abs().max()) == 0.0
            if name == "plain":
                out["cls_score"], out["bbox_w"], out["bbox_b"] = (pred.cls_score.weight.detach().numpy().copy(), pred.bbox_pred.weight.detach().numpy().copy(),
                                                                  pred.bbox_pred.bias.detach().numpy().copy())
                out["scores"], out["deltas"], out["pred_boxes_all"] = scores.numpy(), deltas.numpy(), boxes.numpy()
            out[f"{name}/pred_boxes"] = res[0].pred_boxes.tensor.numpy()
            out[f"{name}/scores"] = res[0].scores.numpy()
            out[f"{name}/pred_classes"] = res[0].pred_classes.numpy()
            out[f"{name}/kept"] = kept[0].numpy()
            print(name, len(kept[0]), "detections, classes up to", int(res[0].pred_classes.max()))
    path = os.path.join(mg.HERE, "ref_openset.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
