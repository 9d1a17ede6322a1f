"""Generates tests/golden/ref_soft_nms.npz by running the REFERENCE's own layers/soft_nms.py (batched_soft_nms) on every case of
tests/exact_soft_nms.py and its fast_rcnn_inference_single_image with soft_nms_enabled=True on a seeded head output.  Reuses the
make_golden.py harness (reference leaf modules imported with their package __init__s bypassed), loading the REAL
detectron2.layers.soft_nms in place of the harness' stub.  Only data is written: per case the keep list, the rescored scores and
a checksum of the inputs (the cases are rebuilt from their seeds by the tests), plus the inference inputs and outputs.

usage:  python tests/golden/make_golden_soft_nms.py
"""
import importlib
import os
import sys

import numpy as np
import torch

import make_golden as mg

sys.path.insert(0, os.path.join(mg.ROOT, "tests"))
import exact_soft_nms as X  # noqa: E402


def checksum(c):
    return np.asarray([c["boxes"].astype(np.float64).sum(), c["scores"].astype(np.float64).sum(), float(np.asarray(c["idxs"]).sum())])


def main():
    mg.setup()
    del sys.modules["detectron2.layers.soft_nms"]                      # the harness' stub
    sn = importlib.import_module("detectron2.layers.soft_nms")          # the reference's own file
    fr = importlib.import_module("detectron2.modeling.roi_heads.fast_rcnn")
    assert fr.batched_soft_nms is sn.batched_soft_nms
    out = {}
    for c in X.cases():
        keep, scores = sn.batched_soft_nms(torch.from_numpy(c["boxes"]), torch.from_numpy(c["scores"]), torch.from_numpy(c["idxs"]),
                                           c["method"], c["sigma"], c["thr"], c["prune"])
        if c["max_keep"] >= 0:                                          # fast_rcnn.py:198-199
            keep, scores = keep[:c["max_keep"]], scores[:c["max_keep"]]
        out[f"keep/{c['name']}"] = keep.numpy().astype(np.int64)
        out[f"scores/{c['name']}"] = scores.numpy().astype(np.float32)
        out[f"sum/{c['name']}"] = checksum(c)
        print(c["name"], len(keep))
    # the empty input (layers/soft_nms.py:118-122)
    k0, s0 = sn.batched_soft_nms(torch.zeros(0, 4), torch.zeros(0), torch.zeros(0, dtype=torch.int64), "linear", 0.5, 0.5, 0.001)
    assert k0.numel() == 0 and s0.numel() == 0 and k0.dtype == torch.int64
    # ---- fast_rcnn_inference_single_image, soft_nms_enabled=True
    inp = X.inference_inputs()
    out["inf/boxes"], out["inf/scores"] = inp["boxes"], inp["scores"]
    for name, cfg in X.inference_configs().items():
        res, kept = fr.fast_rcnn_inference_single_image(
            torch.from_numpy(inp["boxes"]), torch.from_numpy(inp["scores"]), inp["image_shape"], inp["score_thresh"], cfg["nms_thresh"],
            True, cfg["method"], cfg["sigma"], cfg["prune"], cfg["topk"], torch.from_numpy(inp["scores"]).clone())
        out[f"inf/{name}/pred_boxes"] = res.pred_boxes.tensor.numpy()
        out[f"inf/{name}/scores"] = res.scores.numpy()
        out[f"inf/{name}/pred_classes"] = res.pred_classes.numpy()
        out[f"inf/{name}/kept"] = kept.numpy()
        print("inference", name, len(kept))
    path = os.path.join(mg.HERE, "ref_soft_nms.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
