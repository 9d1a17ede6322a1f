"""COCO-format json data sets -- detectron2/data/datasets/coco.py:73-216 (``load_coco_json``) with the ``json`` module (pycocotools
is not a dependency), and the one such set the reference registers for this project: ``bdd_100k_val``
(data/datasets/builtin.py:410-413), the second target domain of the adverse-weather experiment.

``load_coco_json(json_file, image_root) -> (dataset dicts, thing_classes)``:
* categories are sorted by id and mapped to contiguous ids 0..K-1; ``thing_classes`` are their names in that order;
* images are sorted by id; an image without annotations is kept (detections on it are false positives);
* per annotation (in the file's order inside its image; an annotation of an image the file does not list is dropped, as
  ``imgToAnns`` drops it): ``bbox`` XYWH -> this package's XYXY ``[x, y, x + w, y + h]``, ``area`` as stored (``w * h`` when the file
  has none), ``iscrowd`` as a bool, ``category_id`` contiguous; a non-zero ``"ignore"`` raises ``ValueError`` (the reference asserts).
The evaluator derives a box's width back as ``(x + w) - x``, which can differ from the file's ``w`` in the last bit.
"""
import json
import os

# name -> (json file, image root), relative to the datasets root (builtin.py:410-413)
COCO_JSON_SPLITS = {"bdd_100k_val": ("bdd100k/images/100k/val.json", "bdd100k/images/100k/data")}


def is_coco_json(name):
    return name in COCO_JSON_SPLITS


def coco_json_paths(name, datasets_root):
    json_rel, image_rel = COCO_JSON_SPLITS[name]
    return os.path.join(datasets_root, json_rel), os.path.join(datasets_root, image_rel)


def load_coco_json(json_file, image_root):
    with open(json_file) as f:
        data = json.load(f)
    cats = sorted(data.get("categories", []), key=lambda c: c["id"])
    thing_classes = [c["name"] for c in cats]
    id_map = {c["id"]: i for i, c in enumerate(cats)}
    images = sorted(data.get("images", []), key=lambda im: im["id"])
    by_image = {im["id"]: [] for im in images}
    ann_ids = set()
    for a in data.get("annotations", []):
        if a["image_id"] in by_image:
            by_image[a["image_id"]].append(a)
            if "id" in a:
                if a["id"] in ann_ids:
                    raise ValueError(f"Annotation ids in '{json_file}' are not unique!")
                ann_ids.add(a["id"])
    dicts = []
    for im in images:
        objs = []
        for a in by_image[im["id"]]:
            if a.get("ignore", 0) != 0:
                raise ValueError(f'{json_file}: "ignore" in COCO json file is not supported (annotation {a.get("id")} of image {im["id"]})')
            if len(a["bbox"]) != 4:
                raise ValueError(f"One annotation of image {im['id']} contains empty 'bbox' value! This json does not have valid COCO format.")
            if a["category_id"] not in id_map:
                raise KeyError(f"Encountered category_id={a['category_id']} but this id does not exist in 'categories' of the json file.")
            x, y, w, h = (float(v) for v in a["bbox"])
            objs.append({"bbox": [x, y, x + w, y + h], "area": float(a["area"]) if "area" in a else w * h, "iscrowd": bool(a.get("iscrowd", 0)),
                         "category_id": id_map[a["category_id"]]})
        dicts.append({"file_name": os.path.join(image_root, im["file_name"]), "height": im["height"], "width": im["width"], "image_id": im["id"],
                      "annotations": objs})
    return dicts, thing_classes


def load_coco_json_split(name, datasets_root):
    """a registered name under ``datasets_root`` -> (dicts, thing_classes); prints the image count the way the Cityscapes loader does"""
    json_file, image_root = coco_json_paths(name, datasets_root)
    dicts, thing_classes = load_coco_json(json_file, image_root)
    print(f"{name}: {len(dicts)} images in {image_root}")
    return dicts, thing_classes
