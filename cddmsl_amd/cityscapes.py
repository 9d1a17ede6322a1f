"""Cityscapes / Foggy Cityscapes dataset dicts (the adverse-weather benchmark, BASELINE.json configs[3]).

Follows ``_get_cityscapes_DG_files`` / ``_cityscapes_DG_files_to_dict`` with ``from_json=False`` (data/datasets/cityscapes.py:94-127,
384-540) and the split table of data/datasets/builtin.py:228-234.  Boxes come from the ``*_gtFine_instanceIds.png`` maps; the
per-id scan the reference runs on the host is the HIP kernel ``cddmsl_instance_boxes`` (one pass per map, maps of one size sent in
batches).  The 16-bit PNGs are decoded by a small thread pool.

Label facts used here (Cityscapes label definition; ``cityscapesscripts`` is not a dependency):
  * an instance id >= 1000 is ``label_id * 1000 + k``; an id < 1000 is a crowd region whose id is the label id itself;
  * label ids run 0..33; the classes that have instances and are evaluated are person 24, rider 25, car 26, truck 27, bus 28,
    train 31, motorcycle 32, bicycle 33 -> contiguous ids 0..7 in that order (caravan 29 and trailer 30 have instances but are
    ignored in evaluation, so they are dropped like every stuff class).
"""
import os
from concurrent.futures import ThreadPoolExecutor
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

THING_CLASSES = ("person", "rider", "car", "truck", "bus", "train", "motorcycle", "bicycle")
THING_LABEL_IDS = (24, 25, 26, 27, 28, 31, 32, 33)
LABEL_TO_CONTIGUOUS = {l: i for i, l in enumerate(THING_LABEL_IDS)}
NUM_LABEL_IDS = 34                      # label ids 0..33
FOGGY_SUFFIX = "_foggy_beta_0.02.png"   # the twin the DG splits pair with a clear frame (cityscapes.py:107)

# name -> (image dir, foggy twin dir or None, gt dir), relative to the datasets root (builtin.py:228-234; the test split has no
# public ground truth and is not offered)
SPLITS = {
    "cityscapes_DG_train": ("cityscapes/leftImg8bit/train/", "cityscapes/leftImg8bit_foggy/train/", "cityscapes/gtFine/train/"),
    "cityscapes_DG_val": ("cityscapes/leftImg8bit/val/", "cityscapes/leftImg8bit_foggy/val/", "cityscapes/gtFine/val/"),
    "cityscapes_val": ("cityscapes/leftImg8bit/val/", None, "cityscapes/gtFine/val/"),
    "cityscapes_foggy_val": ("cityscapes/leftImg8bit_foggy/val/", None, "cityscapes/gtFine/val/"),
}


def is_cityscapes(name: str) -> bool:
    return name in SPLITS


def list_cityscapes_files(image_dir: str, image_dt_dir: Optional[str], gt_dir: str) -> List[Tuple[str, Optional[str], str]]:
    """``_get_cityscapes_DG_files``: (image, foggy twin or None, instanceIds png) for every file of every city directory.

    Cities and file names are SORTED; the reference lists them in ``PathManager.ls`` order, which is whatever order the filesystem
    returns, so its dataset order (and with it the sampler's permutation -> image mapping) is not reproducible across machines.
    A clear frame ``<stem>_leftImg8bit.png`` gets the twin ``<twin dir>/<city>/<stem>_leftImg8bit_foggy_beta_0.02.png``; any
    other file (a foggy frame) finds its ground truth by splitting its name at ``leftImg8bit_foggy``, exactly as the reference
    does, so every beta of a Foggy download is its own entry."""
    files = []
    for city in sorted(os.listdir(image_dir)):
        city_img_dir, city_gt_dir = os.path.join(image_dir, city), os.path.join(gt_dir, city)
        for basename in sorted(os.listdir(city_img_dir)):
            image_file = os.path.join(city_img_dir, basename)
            twin = None
            if basename.endswith("leftImg8bit.png"):
                if image_dt_dir is not None:
                    twin = os.path.join(image_dt_dir, city, basename[: -len(".png")] + FOGGY_SUFFIX)
                stem = basename[: -len("leftImg8bit.png")]
            else:
                stem = basename.split("leftImg8bit_foggy")[0]
            files.append((image_file, twin, os.path.join(city_gt_dir, stem + "gtFine_instanceIds.png")))
    assert files, f"No images found in {image_dir}"
    return files


def read_instance_map(path: str) -> np.ndarray:
    """16-bit instanceIds png -> uint16 [H,W] (int32 if the decoder hands back 32-bit pixels)"""
    from PIL import Image
    with open(path, "rb") as f:
        a = np.asarray(Image.open(f))
    if a.dtype != np.uint16:
        a = a.astype(np.int32)
    return np.ascontiguousarray(a)


def annotations_from_records(records: np.ndarray) -> List[Dict]:
    """kernel records (id, xmin, ymin, xmax, ymax, npixels), ascending id -> annotation dicts (cityscapes.py:522-540)"""
    annos = []
    for iid, x0, y0, x1, y1, npix in records.tolist():
        label = iid // 1000 if iid >= 1000 else iid
        if label >= NUM_LABEL_IDS:
            raise KeyError(f"instance id {iid}: label id {label} is not a Cityscapes label")      # id2label[label_id]
        if label not in LABEL_TO_CONTIGUOUS:
            continue
        if x1 <= x0 or y1 <= y0:
            continue
        annos.append({"iscrowd": iid < 1000, "category_id": LABEL_TO_CONTIGUOUS[label], "bbox": [float(x0), float(y0), float(x1), float(y1)],
                      "area": float(npix)})
    return annos


def files_to_dicts(files: Sequence[Tuple[str, Optional[str], str]], device="cuda", batch: int = 8, threads: int = 8) -> List[Dict]:
    """``_cityscapes_DG_files_to_dict`` (from_json=False) for every file: decode the maps (thread pool, <= 8 threads), send maps
    of one size and dtype to the kernel ``batch`` at a time, build the dicts in file order."""
    from . import hip
    gt_paths = [f[2] for f in files]
    out: List[Optional[Dict]] = [None] * len(files)
    with ThreadPoolExecutor(max_workers=max(1, min(8, threads))) as pool:
        maps = list(pool.map(read_instance_map, gt_paths))
    groups: Dict[Tuple, List[int]] = {}
    for i, m in enumerate(maps):
        groups.setdefault((m.shape, m.dtype.str), []).append(i)
    for idx in groups.values():
        for s in range(0, len(idx), batch):
            part = idx[s:s + batch]
            t = torch.from_numpy(np.stack([maps[i] for i in part])).to(device)
            recs = hip.instance_boxes_host(t)
            for i, r in zip(part, recs):
                image_file, twin, _ = files[i]
                d = {"file_name": image_file, "image_id": os.path.basename(image_file), "height": int(maps[i].shape[0]),
                     "width": int(maps[i].shape[1])}
                if twin is not None:
                    d["data_dt_file_name"] = twin
                d["annotations"] = annotations_from_records(r)
                out[i] = d
    return out


def load_cityscapes(name: str, datasets_root: str, device="cuda") -> List[Dict]:
    """dataset dicts of a split of ``SPLITS`` under ``datasets_root`` (the directory holding ``cityscapes/``)"""
    if name not in SPLITS:
        raise KeyError(f"{name} is not a Cityscapes split here (known: {sorted(SPLITS)})")
    image_dir, dt_dir, gt_dir = (None if d is None else os.path.join(datasets_root, d) for d in SPLITS[name])
    files = list_cityscapes_files(image_dir, dt_dir, gt_dir)
    if name == "cityscapes_foggy_val":     # a full Foggy download holds three betas per frame: each is its own image
        print(f"{name}: {len(files)} images in {image_dir}")
    return files_to_dicts(files, device)


def filter_images_with_only_crowd_annotations(dicts: List[Dict]) -> List[Dict]:
    """data/build.py:41-60 (DATALOADER.FILTER_EMPTY_ANNOTATIONS): keep images with at least one non-crowd annotation"""
    return [d for d in dicts if any(not a.get("iscrowd", 0) for a in d["annotations"])]
