#!/usr/bin/env python
"""Times PascalVOCDetectionEvaluator with and without ``device`` on seeded synthetic sets of 20 classes.

  host    process() copies every image's detections to the host and formats them into the reference's result lines, evaluate()
          runs class_ap: the Python walk over (class, IoU threshold, detection) -- the evaluator as it was before hip.voc_match
  device  process() keeps the detections on the device, evaluate() reads them back once, sorts per class on the host, matches all
          (class, image) segments at all thresholds in one hip.voc_match launch and runs voc_accumulate

Both see the same detections (already on the GPU, as the model leaves them) and must return the same dictionary; the tool checks
that.  One JSON line per size: seconds of process() over all images and of evaluate(), per path.  The annotation files are written
to a temporary directory, outside the timed region.

    python tools/voc_eval_bench.py [--sizes 500x20,4952x100] [--gt 3] [--year 2007] [--skip-host]
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def make_set(dirname, n_images, n_dets, n_gt, class_names, seed=0):
    """500 x 375 frames; about ``n_gt`` boxes per image (10 % difficult), ``n_dets`` detections: jittered copies of the boxes with
    their class (80 %) or a random one, scores in (0.05, 1) -> (image ids, [(xyxy f32, score f32, class int64)])"""
    rng = np.random.RandomState(seed)
    os.makedirs(os.path.join(dirname, "Annotations"))
    os.makedirs(os.path.join(dirname, "ImageSets", "Main"))
    names, dets = [], []
    for i in range(n_images):
        g = max(1, rng.poisson(n_gt))
        wh = np.exp(rng.uniform(np.log(20), np.log(300), (g, 2)))
        xy = rng.uniform(0, 1, (g, 2)) * (np.array([500, 375]) - wh).clip(min=1)
        box = np.concatenate([np.floor(xy) + 1, np.floor(xy + wh) + 1], axis=1).astype(np.int64)
        cls = rng.randint(len(class_names), size=g)
        body = "".join(f"<object><name>{class_names[c]}</name><difficult>{int(rng.rand() < 0.1)}</difficult><bndbox><xmin>{b[0]}</xmin><ymin>{b[1]}</ymin>"
                       f"<xmax>{b[2]}</xmax><ymax>{b[3]}</ymax></bndbox></object>" for c, b in zip(cls, box))
        name = f"{i:06d}"
        with open(os.path.join(dirname, "Annotations", name + ".xml"), "w") as f:
            f.write(f"<annotation><size><width>500</width><height>375</height></size>{body}</annotation>")
        src = rng.randint(g, size=n_dets)
        b = box[src].astype(np.float64) - [1, 1, 0, 0] + rng.normal(0, 1, (n_dets, 4)) * np.tile(wh[src], 2) * 0.12
        b[:, 2:] = np.maximum(b[:, 2:], b[:, :2] + 1)
        c = np.where(rng.rand(n_dets) < 0.8, cls[src], rng.randint(len(class_names), size=n_dets))
        names.append(name)
        dets.append((b.astype(np.float32), rng.uniform(0.05, 1, n_dets).astype(np.float32), c.astype(np.int64)))
    with open(os.path.join(dirname, "ImageSets", "Main", "test.txt"), "w") as f:
        f.write("".join(n + "\n" for n in names))
    return names, dets


def run(dirname, names, dev_dets, year, device):
    from cddmsl_amd.evaluation import PascalVOCDetectionEvaluator
    from cddmsl_amd.structures import Boxes, Instances
    ev = PascalVOCDetectionEvaluator(dirname, "test", year, device=device)
    ev._ground_truth()                  # parsed once per evaluator on both paths: the XML files are not what is measured
    if device is not None:
        ev._device_ground_truth()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for n, (b, sc, c) in zip(names, dev_dets):
        ev.process([{"image_id": n}], [{"instances": Instances((375, 500), pred_boxes=Boxes(b), scores=sc, pred_classes=c)}])
    t1 = time.perf_counter()            # (device path: nothing has been waited for -- evaluate()'s readback does that)
    with np.errstate(invalid="ignore", divide="ignore"):
        res = ev.evaluate()
    t2 = time.perf_counter()
    return res, t1 - t0, t2 - t1


def same(a, b):
    return list(a["bbox"]) == list(b["bbox"]) and all(x == y or (x != x and y != y) for x, y in zip(a["bbox"].values(), b["bbox"].values()))


def main():
    from cddmsl_amd.evaluation import VOC_CLASS_NAMES
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="500x20,4952x100", help="comma-separated IMAGESxDETECTIONS-per-image")
    ap.add_argument("--gt", type=int, default=3)
    ap.add_argument("--year", type=int, default=2007)
    ap.add_argument("--skip-host", action="store_true")
    a = ap.parse_args()
    ok = True
    with tempfile.TemporaryDirectory() as tmp:
        warm = os.path.join(tmp, "warm")
        names, dets = make_set(warm, 8, 10, a.gt, VOC_CLASS_NAMES, seed=1)
        run(warm, names, [tuple(torch.from_numpy(x).cuda() for x in d) for d in dets], a.year, "cuda")      # library load, first launch
        for size in a.sizes.split(","):
            n_images, n_dets = (int(v) for v in size.split("x"))
            d = os.path.join(tmp, size)
            names, dets = make_set(d, n_images, n_dets, a.gt, VOC_CLASS_NAMES)
            dev_dets = [tuple(torch.from_numpy(x).cuda() for x in t) for t in dets]
            out = {"images": n_images, "dets_per_image": n_dets, "classes": len(VOC_CLASS_NAMES), "year": a.year}
            dev, out["device_process_s"], out["device_evaluate_s"] = run(d, names, dev_dets, a.year, "cuda")
            out["AP50"] = dev["bbox"]["AP50"]
            if not a.skip_host:
                host, out["host_process_s"], out["host_evaluate_s"] = run(d, names, dev_dets, a.year, None)
                out["results_equal"] = bool(same(host, dev))
                ok = ok and out["results_equal"]
            print(json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in out.items()}), flush=True)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
