#!/usr/bin/env python
"""Detections against a vocabulary the detector was not trained on -- the reference's MODEL.CLIP.OPENSET_TEST_TEXT_EMB_PATH switch on
this package's open-vocabulary HIP path (cddmsl_amd/csrc/openset.hip):

    python tools/detect_open_vocab.py --config-file configs/VOC-Experiments/faster_rcnn_CLIP_R_50_C4.yaml --concepts concepts.txt \\
        --embeddings concept_embeds.pth [--regions-per-image N] MODEL.WEIGHTS model_final.pth INPUT_DIR images OUTPUT_DIR out

``--concepts`` is one class name per line and ``--embeddings`` the [len(concepts), TEXT_EMB_DIM] tensor tools/extract_concept_features.py
writes for them.  A vocabulary of another size than the head's needs class-agnostic box regression (MODEL.ROI_BOX_HEAD.
CLS_AGNOSTIC_BBOX_REG True, what the reference's open-vocabulary configs set) or MODEL.CLIP.NO_BOX_DELTA True; the head refuses
anything else.  ``--regions-per-image N`` keeps the N best detections of an image (TEST.DETECTIONS_PER_IMAGE).  Every image of
INPUT_DIR (.jpg / .jpeg / .png) goes through the test loader's preprocessing; writes ``OUTPUT_DIR/detections.json``: per image file
name a list of {"box" [x0, y0, x1, y1] in original-image pixels, "class", "name", "score"}, highest score first.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

EXTS = (".jpg", ".jpeg", ".png")


def parse(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--config-file", required=True)
    ap.add_argument("--concepts", required=True, help="text file, one class name per line")
    ap.add_argument("--embeddings", required=True, help="[len(concepts), TEXT_EMB_DIM] tensor of their text embeddings")
    ap.add_argument("--regions-per-image", type=int, default=None, help="detections kept per image (default: TEST.DETECTIONS_PER_IMAGE)")
    ap.add_argument("opts", nargs=argparse.REMAINDER, help="KEY VALUE config overrides (MODEL.WEIGHTS, INPUT_DIR, OUTPUT_DIR, ...)")
    return ap.parse_args(argv)


def _need_file(path, what):
    if not path or not os.path.isfile(path):
        raise SystemExit(f"{what} not found: {path!r}")


def main(argv=None):
    args = parse(argv)
    from cddmsl_amd.config import get_cfg
    cfg = get_cfg()
    cfg.merge_from_file(args.config_file)
    cfg.merge_from_list(args.opts)
    _need_file(args.concepts, "--concepts")
    _need_file(args.embeddings, "--embeddings")
    _need_file(cfg.MODEL.WEIGHTS, "MODEL.WEIGHTS")
    if "INPUT_DIR" not in cfg or not os.path.isdir(cfg.INPUT_DIR):
        raise SystemExit(f"INPUT_DIR <dir of images> not found: {cfg.get('INPUT_DIR')!r}")
    device = torch.device(cfg.MODEL.DEVICE)
    if device.type != "cuda" or not torch.cuda.is_available():
        raise SystemExit(f"open-vocabulary detection runs on the MI355X only (HIP kernels, no CPU path); MODEL.DEVICE={cfg.MODEL.DEVICE}")
    with open(args.concepts, encoding="utf-8") as f:
        names = [ln.strip() for ln in f if ln.strip()]
    cfg.merge_from_list(["MODEL.CLIP.USE_TEXT_EMB_CLASSIFIER", True, "MODEL.CLIP.OPENSET_TEST_TEXT_EMB_PATH", args.embeddings,
                         "MODEL.CLIP.OPENSET_TEST_NUM_CLASSES", len(names)])        # (a file of another row count is refused by the head)
    if args.regions_per_image is not None:
        cfg.merge_from_list(["TEST.DETECTIONS_PER_IMAGE", args.regions_per_image])

    from cddmsl_amd.captioning import _resized
    from cddmsl_amd.checkpoint import DetectionCheckpointer
    from cddmsl_amd.data import read_image
    from cddmsl_amd.modeling import build_model

    try:
        model = build_model(cfg)
    except ValueError as e:
        raise SystemExit(str(e))
    DetectionCheckpointer(model).load(cfg.MODEL.WEIGHTS)
    model.eval()
    files = sorted(f for f in os.listdir(cfg.INPUT_DIR) if f.lower().endswith(EXTS))
    t0 = time.perf_counter()
    result = {}
    with torch.no_grad():
        for fn in files:
            img = read_image(os.path.join(cfg.INPUT_DIR, fn), cfg.INPUT.FORMAT)
            inst = model.inference([{"image": _resized(img, cfg), "height": img.shape[0], "width": img.shape[1]}])[0]["instances"]
            order = torch.argsort(inst.scores, descending=True, stable=True)
            boxes, cls, sc = inst.pred_boxes.tensor[order].cpu().tolist(), inst.pred_classes[order].cpu().tolist(), inst.scores[order].cpu().tolist()
            result[fn] = [{"box": b, "class": int(c), "name": names[int(c)], "score": float(s)} for b, c, s in zip(boxes, cls, sc)]
    os.makedirs(cfg.OUTPUT_DIR, exist_ok=True)
    path = os.path.join(cfg.OUTPUT_DIR, "detections.json")
    with open(path, "w", encoding="utf-8") as f:
        json.dump(result, f, indent=1, ensure_ascii=False)
    print(f"{len(files)} images, {sum(len(v) for v in result.values())} detections over {len(names)} concepts in "
          f"{time.perf_counter() - t0:.2f} s: {path}")
    return path


if __name__ == "__main__":
    main()
