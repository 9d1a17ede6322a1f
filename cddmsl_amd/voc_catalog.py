"""The Pascal VOC family of the dataset catalog: VOC proper, its domain-generalisation twins and the art test sets
(configs/VOC-Experiments; BASELINE.json configs[0]).

The reference registers these names in data/datasets/builtin.py:306-407 (``register_all_pascal_voc``, ``register_all_pascal_DG``,
``register_all_water`` / ``_clipart`` / ``_comic``); the tables below hold the same facts as data.  Directories are relative to the
datasets root (Detectron2's DETECTRON2_DATASETS):

    VOC2007/ VOC2012/                      Annotations/ ImageSets/Main/ JPEGImages/   (the devkit's year directories)
    dt_clipart/ dt_watercolor/ dt_comic/   VOC2007/JPEGImages/ VOC2012/JPEGImages/   (the translated twins; dt_clipart also has
                                           Annotations/ and ImageSets/ and is a data set of its own, ``dt_Clipart_*_trainval``)
    clipart/ watercolor/ comic/            Annotations/ ImageSets/Main/ JPEGImages/

The year decides the AP metric (11-point for 2007, area under the envelope otherwise).  The art sets are registered with year 2012
in the reference, and so they are here.  A ``voc_<style>_<year>_<split>`` name pairs every image with its twin
``<dirname>/../<dt_data>/<VOC2007|VOC2012>/JPEGImages/<id>.jpg`` (``data.load_voc_instances`` builds that path).
"""
import os
from typing import Dict, List, Optional, Sequence, Tuple

from .evaluation import VOC_CLASS_NAMES


def _table():
    t = {}
    for year, splits in ((2007, ("trainval", "train", "val", "test")), (2012, ("trainval", "train", "val"))):
        for split in splits:
            t[f"voc_{year}_{split}"] = (f"VOC{year}", split, year, None)
    for style in ("clipart", "watercolor", "comic"):
        for year in (2007, 2012):
            for split in ("trainval", "train"):
                t[f"voc_{style}_{year}_{split}"] = (f"VOC{year}", split, year, "dt_" + style)
    for name, dirname in (("Clipart1k", "clipart"), ("Watercolor", "watercolor"), ("Comic", "comic")):
        for split in ("train", "test"):
            t[f"{name}_{split}"] = (dirname, split, 2012, None)
    for year in (2007, 2012):
        t[f"dt_Clipart_{year}_trainval"] = (f"dt_clipart/VOC{year}", "trainval", 2012, None)
    return t


# name -> (directory under the datasets root, split, year, directory name of the translated twins or None)
ENTRIES: Dict[str, Tuple[str, str, int, Optional[str]]] = _table()

_CACHE: Dict[Tuple[str, str], List[Dict]] = {}


def is_voc_family(name: str) -> bool:
    return name in ENTRIES


def voc_entry(name: str, root: str) -> Tuple[str, str, int, Optional[str]]:
    """-> (dirname under ``root``, split, year, dt_data)"""
    if name not in ENTRIES:
        raise KeyError(f"{name} is not a VOC-family data set here (known: {sorted(ENTRIES)})")
    rel, split, year, dt_data = ENTRIES[name]
    return os.path.join(root, *rel.split("/")), split, year, dt_data


def image_set_file(name: str, root: str) -> str:
    dirname, split, _, _ = voc_entry(name, root)
    return os.path.join(dirname, "ImageSets", "Main", split + ".txt")


def twin_dir(name: str, root: str) -> Optional[str]:
    """the JPEGImages directory of a DG name's translated twins (None for a name without twins)"""
    dirname, _, year, dt_data = voc_entry(name, root)
    if dt_data is None:
        return None
    return os.path.join(dirname, "..", dt_data, f"VOC{year}", "JPEGImages")


def load_voc_family(name: str, root: str) -> List[Dict]:
    """dataset dicts of one name (``data.load_voc_instances``), parsed once per (name, root) for the life of the process: a
    periodic evaluation does not read thousands of XML files again every period.  A DG name whose twin directory is missing raises
    a FileNotFoundError naming it -- here, not in a loader worker."""
    key = (name, os.path.abspath(root))
    if key not in _CACHE:
        from .data import load_voc_instances
        dirname, split, _, dt_data = voc_entry(name, root)
        twins = twin_dir(name, root)
        if twins is not None and not os.path.isdir(twins):
            raise FileNotFoundError(f"{name}: the translated twins' directory {os.path.normpath(twins)} is missing")
        _CACHE[key] = load_voc_instances(dirname, split, VOC_CLASS_NAMES, dt_data=dt_data)
    return _CACHE[key]


def load_train_sets(names: Sequence[str], root: str, filter_empty: bool = True) -> List[Dict]:
    """``get_detection_dataset_dicts`` (data/build.py) for VOC-family names: the sets' dicts chained in the order named; with
    ``filter_empty`` (DATALOADER.FILTER_EMPTY_ANNOTATIONS) images without annotations are dropped.  Names of another family raise a
    ValueError naming them."""
    others = [n for n in names if not is_voc_family(n)]
    if others:
        raise ValueError(f"DATASETS.TRAIN mixes families: {others} are not VOC-family names (all names: {list(names)})")
    dicts = [d for n in names for d in load_voc_family(n, root)]
    if filter_empty:
        dicts = [d for d in dicts if d["annotations"]]
    return dicts
