"""Generates tests/golden/ref_proposal_recall.npz by running the REFERENCE's own evaluation/coco_evaluation.py
``_evaluate_box_proposals`` in place on the images of tests/proposal_recall_cases.py, for all eight named area ranges and the limits
100, 1000 and None.  Reuses the make_golden.py harness (reference leaf modules imported with their package __init__s bypassed); the
COCO api is a stand-in object with ``getAnnIds`` / ``loadAnns`` over the cases' annotations (XYWH boxes, ``area``, ``iscrowd``).
Only data is written: the inputs and, per (range, limit), ``gt_overlaps``, ``num_pos``, ``recalls``, ``ar``.

usage:  python tests/golden/make_golden_proposal_recall.py
"""
import importlib
import os
import sys
import types

import numpy as np
import torch

import make_golden as mg

sys.path.insert(0, os.path.join(mg.ROOT, "tests"))
import proposal_recall_cases as C  # noqa: E402

AREAS = ("all", "small", "medium", "large", "96-128", "128-256", "256-512", "512-inf")


class CocoStandIn:
    def __init__(self, items):
        self.anns = {}
        for d, _, _ in items:
            out = []
            for a in d["annotations"]:
                x0, y0, x1, y1 = a["bbox"]
                out.append({"bbox": [x0, y0, x1 - x0, y1 - y0], "area": a.get("area", (x1 - x0) * (y1 - y0)), "iscrowd": a["iscrowd"]})
            self.anns[d["image_id"]] = out

    def getAnnIds(self, imgIds):
        return [(imgIds, k) for k in range(len(self.anns[imgIds]))]

    def loadAnns(self, ids):
        return [self.anns[i][k] for i, k in ids]


def main():
    mg.setup()
    evm = types.ModuleType("detectron2.evaluation.evaluator")
    evm.DatasetEvaluator = type("DatasetEvaluator", (), {})
    mg._pkg("detectron2.evaluation", "detectron2/evaluation")
    sys.modules["detectron2.evaluation.evaluator"] = evm
    sys.modules["detectron2.config"].CfgNode = mg._Anything
    sys.modules["detectron2.data"].MetadataCatalog = mg._Anything
    for n in ("detectron2.data.datasets", "detectron2.data.datasets.coco", "detectron2.data.datasets.coco_zeroshot_categories",
              "detectron2.evaluation.fast_eval_api", "tabulate"):
        sys.modules[n] = mg._StubModule(n)
    ce = importlib.import_module("detectron2.evaluation.coco_evaluation")
    S = sys.modules["detectron2.structures"]
    assert ce.pairwise_iou is S.pairwise_iou

    items = C.dataset()
    api = CocoStandIn(items)
    preds, out = [], {"n_images": np.asarray(len(items))}
    for k, (d, boxes, logits) in enumerate(items):
        inst = S.Instances((d["height"], d["width"]))
        inst.proposal_boxes = S.Boxes(torch.from_numpy(boxes.copy()))
        inst.objectness_logits = torch.from_numpy(logits.copy())
        preds.append({"image_id": d["image_id"], "proposals": inst})
        out[f"in/{k}/boxes"], out[f"in/{k}/logits"] = boxes, logits
        out[f"in/{k}/gt"] = np.asarray([a["bbox"] for a in d["annotations"]], dtype=np.float64).reshape(-1, 4)
        out[f"in/{k}/area"] = np.asarray([a["area"] for a in api.anns[d["image_id"]]], dtype=np.float64)
        out[f"in/{k}/crowd"] = np.asarray([a["iscrowd"] for a in d["annotations"]], dtype=np.int64)
    for area in AREAS:
        for limit in C.LIMITS:
            st = ce._evaluate_box_proposals(preds, api, area=area, limit=limit)
            key = f"{area}/{limit}"
            out[f"gt_overlaps/{key}"] = st["gt_overlaps"].numpy().astype(np.float32)
            out[f"num_pos/{key}"] = np.asarray(int(st["num_pos"]))
            out[f"recalls/{key}"] = st["recalls"].numpy().astype(np.float32)
            out[f"ar/{key}"] = np.asarray(st["ar"].item(), dtype=np.float32)
            print(key, int(st["num_pos"]), float(st["ar"]))
    path = os.path.join(mg.HERE, "ref_proposal_recall.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
