"""Dependency-free config with the reference's key names (yacs/fvcore are not installed here).

``get_cfg()`` returns the defaults of the hot-path keys (detectron2/config/defaults.py values, file:line in
SURVEY.md Appendix A); ``merge_from_file`` reads the reference's YAMLs incl. ``_BASE_`` inheritance
(configs/Base-RCNN-C4.yaml, configs/VOC-Experiments/faster_rcnn_CLIP_R_50_C4.yaml, ...); ``merge_from_list``
takes the CLI ``KEY VALUE`` pairs (engine/defaults.py:133-140).
"""
import ast
import copy
import math
import os

import yaml


class CfgNode(dict):
    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError:
            raise AttributeError(k)

    def __setattr__(self, k, v):
        self[k] = v

    def clone(self):
        return copy.deepcopy(self)

    def freeze(self):
        return self

    def merge_from_other(self, other, allow_new=True):
        for k, v in other.items():
            if isinstance(v, dict) and isinstance(self.get(k), dict):
                self[k].merge_from_other(v, allow_new)
            else:
                self[k] = _to_node(v)

    def merge_from_file(self, path):
        with open(path) as f:
            d = yaml.safe_load(f) or {}
        base = d.pop("_BASE_", None)
        d.pop("BASE_", None)  # typo'd key in configs/AdverseWeather-Experiments/faster_rcnn_CLIP_R_50_C4.yaml:1
        if base:
            self.merge_from_file(os.path.join(os.path.dirname(path), base))
        self.merge_from_other(_to_node(_eval_strings(d)))

    def merge_from_list(self, lst):
        assert len(lst) % 2 == 0, "Override list has odd length"
        for k, v in zip(lst[0::2], lst[1::2]):
            node = self
            parts = k.split(".")
            for p in parts[:-1]:
                node = node.setdefault(p, CfgNode())
            if isinstance(v, str):
                try:
                    v = ast.literal_eval(v)
                except (ValueError, SyntaxError):
                    pass
            node[parts[-1]] = _to_node(v)


def auto_scale_workers(cfg, num_workers):
    """``DefaultTrainer.auto_scale_workers`` (engine/defaults.py:633-701; called from ``DefaultTrainer.__init__`` :374): a config
    written for ``SOLVER.REFERENCE_WORLD_SIZE`` workers, run on ``num_workers``, keeps its PER-GPU batch: total batch and base LR
    scale with the worker count, iteration counts (MAX_ITER, WARMUP_ITERS, STEPS, TEST.EVAL_PERIOD, CHECKPOINT_PERIOD) inversely.
    Returns the config itself when ``REFERENCE_WORLD_SIZE`` is 0 or already equals ``num_workers``, a scaled clone otherwise."""
    old = cfg.SOLVER.get("REFERENCE_WORLD_SIZE", 0)
    if old == 0 or old == num_workers:
        return cfg
    cfg = cfg.clone()
    assert cfg.SOLVER.IMS_PER_BATCH % old == 0, "Invalid REFERENCE_WORLD_SIZE in config!"
    scale = num_workers / old
    cfg.SOLVER.IMS_PER_BATCH = int(round(cfg.SOLVER.IMS_PER_BATCH * scale))
    cfg.SOLVER.BASE_LR = cfg.SOLVER.BASE_LR * scale
    cfg.SOLVER.MAX_ITER = int(round(cfg.SOLVER.MAX_ITER / scale))
    cfg.SOLVER.WARMUP_ITERS = int(round(cfg.SOLVER.WARMUP_ITERS / scale))
    cfg.SOLVER.STEPS = tuple(int(round(s / scale)) for s in cfg.SOLVER.STEPS)
    cfg.TEST.EVAL_PERIOD = int(round(cfg.TEST.EVAL_PERIOD / scale))
    cfg.SOLVER.CHECKPOINT_PERIOD = int(round(cfg.SOLVER.CHECKPOINT_PERIOD / scale))
    cfg.SOLVER.REFERENCE_WORLD_SIZE = num_workers      # maintain the invariant
    return cfg


def _eval_strings(d):
    """YAML leaves like "(480, 512)" are python tuples in the reference's configs."""
    if isinstance(d, dict):
        return {k: _eval_strings(v) for k, v in d.items()}
    if isinstance(d, str) and d[:1] in "([":
        try:
            return ast.literal_eval(d)
        except (ValueError, SyntaxError):
            return d
    return d


def _to_node(v):
    if isinstance(v, dict) and not isinstance(v, CfgNode):
        n = CfgNode()
        for k, x in v.items():
            n[k] = _to_node(x)
        return n
    return v


def get_cfg():
    C = _to_node({
        "VERSION": 2,
        "SEED": 1,
        "VIS_PERIOD": 0,
        "MODEL": {
            "DEVICE": "cuda", "META_ARCHITECTURE": "GeneralizedRCNN", "WEIGHTS": "", "MASK_ON": False, "KEYPOINT_ON": False,
            "KD_REGULRAZIATION": True, "PRE_TRAINED_RCLIP_PATH": "", "VISION_TO_LANG_PATH": "",
            "PIXEL_MEAN": [103.530, 116.280, 123.675], "PIXEL_STD": [1.0, 1.0, 1.0],
            "COMPUTE_DTYPE": "bf16",  # build-specific: "bf16" throughput path / "f32" parity path
            "BACKBONE": {"NAME": "build_resnet_backbone", "FREEZE_AT": 2},
            "RESNETS": {"DEPTH": 50, "OUT_FEATURES": ["res4"], "NORM": "FrozenBN", "RES2_OUT_CHANNELS": 256,
                        "STEM_OUT_CHANNELS": 64},
            "ANCHOR_GENERATOR": {"NAME": "DefaultAnchorGenerator", "SIZES": [[32, 64, 128, 256, 512]],
                                 "ASPECT_RATIOS": [[0.5, 1.0, 2.0]], "OFFSET": 0.0},
            "PROPOSAL_GENERATOR": {"NAME": "RPN", "MIN_SIZE": 0},
            "RPN": {"HEAD_NAME": "StandardRPNHead", "IN_FEATURES": ["res4"], "BOUNDARY_THRESH": -1,
                    "IOU_THRESHOLDS": [0.3, 0.7], "IOU_LABELS": [0, -1, 1], "BATCH_SIZE_PER_IMAGE": 256,
                    "POSITIVE_FRACTION": 0.5, "BBOX_REG_LOSS_TYPE": "smooth_l1", "BBOX_REG_LOSS_WEIGHT": 1.0,
                    "BBOX_REG_WEIGHTS": (1.0, 1.0, 1.0, 1.0), "SMOOTH_L1_BETA": 0.0, "LOSS_WEIGHT": 1.0,
                    "PRE_NMS_TOPK_TRAIN": 12000, "PRE_NMS_TOPK_TEST": 6000, "POST_NMS_TOPK_TRAIN": 2000,
                    "POST_NMS_TOPK_TEST": 1000, "NMS_THRESH": 0.7, "CONV_DIMS": [-1]},
            "ROI_HEADS": {"NAME": "Res5ROIHeads", "NUM_CLASSES": 80, "IN_FEATURES": ["res4"], "IOU_THRESHOLDS": [0.5],
                          "IOU_LABELS": [0, 1], "BATCH_SIZE_PER_IMAGE": 512, "POSITIVE_FRACTION": 0.25,
                          "SCORE_THRESH_TEST": 0.05, "NMS_THRESH_TEST": 0.5, "PROPOSAL_APPEND_GT": True,
                          # soft-NMS at inference (defaults.py:399-404); NMS_THRESH_TEST doubles as the linear / hard threshold
                          "SOFT_NMS_ENABLED": False, "SOFT_NMS_METHOD": "gaussian", "SOFT_NMS_SIGMA": 0.5, "SOFT_NMS_PRUNE": 0.001},
            "ROI_BOX_HEAD": {"BBOX_REG_LOSS_TYPE": "smooth_l1", "BBOX_REG_LOSS_WEIGHT": 1.0,
                             "BBOX_REG_WEIGHTS": (10.0, 10.0, 5.0, 5.0), "SMOOTH_L1_BETA": 0.0, "POOLER_RESOLUTION": 14,
                             "POOLER_SAMPLING_RATIO": 0, "POOLER_TYPE": "ROIAlignV2", "CLS_AGNOSTIC_BBOX_REG": False},
            "CLIP": {"CROP_REGION_TYPE": "", "USE_TEXT_EMB_CLASSIFIER": False, "TEXT_EMB_PATH": None, "TEXT_EMB_DIM": 1024,
                     "NO_BOX_DELTA": False, "BG_CLS_LOSS_WEIGHT": None, "ONLY_SAMPLE_FG_PROPOSALS": False,
                     "CLSS_TEMP": 0.01, "FOCAL_SCALED_LOSS": None, "MULTIPLY_RPN_SCORE": False,
                     # open-vocabulary inference (defaults.py: MODEL.CLIP.OPENSET_TEST_*): embeddings of the vocabulary to evaluate on
                     "OPENSET_TEST_NUM_CLASSES": None, "OPENSET_TEST_TEXT_EMB_PATH": None},
        },
        "INPUT": {"MIN_SIZE_TRAIN": (800,), "MAX_SIZE_TRAIN": 1333, "MIN_SIZE_TEST": 800, "MAX_SIZE_TEST": 1333, "FORMAT": "BGR",
                  "MIN_SIZE_TRAIN_SAMPLING": "choice", "RANDOM_FLIP": "horizontal",
                  # defaults.py:68-73: T.RandomCrop in front of the resize (training mapper only)
                  "CROP": {"ENABLED": False, "TYPE": "relative_range", "SIZE": [0.9, 0.9]},
                  # project-specific: RandomBrightness / RandomContrast / RandomSaturation (intensity_min, intensity_max) and RandomLighting
                  # (scale) of the reference, in that order, on the final uint8 image of the training mapper; a range of exactly (1.0, 1.0)
                  # and a scale of 0.0 switch an operation off.  PROB: RandomApply's.  TWIN: the domain twin gets the "same" draws, draws of
                  # its own ("independent") or is left alone ("none").  With DATALOADER.DEVICE_RESIZE one HIP launch per batch, same bytes
                  "COLOR_JITTER": {"ENABLED": False, "PROB": 1.0, "BRIGHTNESS": (1.0, 1.0), "CONTRAST": (1.0, 1.0), "SATURATION": (1.0, 1.0),
                                   "LIGHTING": 0.0, "TWIN": "same"}},
        "DATASETS": {"TRAIN": (), "TEST": ()},
        "DATALOADER": {"NUM_WORKERS": 4, "ASPECT_RATIO_GROUPING": True, "FILTER_EMPTY_ANNOTATIONS": True,
                       # build-specific: ResizeShortestEdge / RandomFlip / HWC -> CHW / RGB -> BGR of the loader's images in one HIP launch per
                       # batch (bit-equal to the PIL path) instead of in the mapper; the loader's device must be a GPU
                       "DEVICE_RESIZE": False},
        "SOLVER": {"IMS_PER_BATCH": 16, "BASE_LR": 0.001, "MOMENTUM": 0.9, "NESTEROV": False, "WEIGHT_DECAY": 0.0001,
                   "WEIGHT_DECAY_NORM": 0.0, "GAMMA": 0.1, "STEPS": (30000,), "MAX_ITER": 40000, "WARMUP_FACTOR": 1.0 / 1000,
                   "WARMUP_ITERS": 1000, "WARMUP_METHOD": "linear", "LR_SCHEDULER_NAME": "WarmupMultiStepLR", "CHECKPOINT_PERIOD": 5000, "BIAS_LR_FACTOR": 1.0,
                   "WEIGHT_DECAY_BIAS": 0.0001, "REFERENCE_WORLD_SIZE": 0,
                   "CLIP_GRADIENTS": {"ENABLED": False, "CLIP_TYPE": "value", "CLIP_VALUE": 1.0, "NORM_TYPE": 2.0},
                   "AMP": {"ENABLED": False}},
        "TEST": {"EVAL_PERIOD": 0, "DETECTIONS_PER_IMAGE": 100,
                 # project-specific: GeneralizedRCNN.inference also returns its RPN proposals ("proposals") and the evaluation entry
                 # points report their recall (box_proposals: AR@100 ... ARl@1000) next to the box AP of every test set
                 "PROPOSAL_RECALL": False,
                 # test-time augmentation (defaults.py:718-721): multi-scale + flip views, merged by per-class NMS; results under *_TTA
                 "AUG": {"ENABLED": False, "MIN_SIZES": (400, 500, 600, 700, 800, 900, 1000, 1100, 1200), "MAX_SIZE": 4000, "FLIP": True}},
        # project-specific (block name and DECAY as D2Go's MODEL_EMA): an average of the trainable weights kept after every step on the
        # GPU, MODE "ema" (avg += (1 - DECAY)(w - avg)) or "uniform" (running mean of the snapshots since START_ITER, SWA); saved with
        # every checkpoint and evaluated next to the training weights under *_EMA keys: EVAL "plain" / "averaged" / "both"
        "MODEL_EMA": {"ENABLED": False, "MODE": "ema", "DECAY": 0.999, "START_ITER": 0, "EVAL": "both"},
        "OUTPUT_DIR": "./output",
    })
    return C


MODEL_EMA_MODES = ("ema", "uniform")
MODEL_EMA_EVALS = ("plain", "averaged", "both")


def check_model_ema(cfg):
    """-> cfg.MODEL_EMA if it is enabled and valid, None if absent or disabled; ValueError naming the key otherwise"""
    e = cfg.get("MODEL_EMA", None)
    if e is None or not e.ENABLED:
        return None
    if e.MODE not in MODEL_EMA_MODES:
        raise ValueError("MODEL_EMA.MODE {!r}: one of {}".format(e.MODE, MODEL_EMA_MODES))
    if e.EVAL not in MODEL_EMA_EVALS:
        raise ValueError("MODEL_EMA.EVAL {!r}: one of {}".format(e.EVAL, MODEL_EMA_EVALS))
    if isinstance(e.DECAY, bool) or not isinstance(e.DECAY, (int, float)) or not 0.0 <= e.DECAY < 1.0:
        raise ValueError("MODEL_EMA.DECAY {!r}: a number in [0, 1)".format(e.DECAY))
    if isinstance(e.START_ITER, bool) or not isinstance(e.START_ITER, int) or e.START_ITER < 0:
        raise ValueError("MODEL_EMA.START_ITER {!r}: an integer >= 0".format(e.START_ITER))
    return e


COLOR_JITTER_TWINS = ("same", "independent", "none")


def _number(v):
    return isinstance(v, (int, float)) and not isinstance(v, bool) and math.isfinite(v)


def check_color_jitter(cfg):
    """-> cfg.INPUT.COLOR_JITTER if it is enabled and valid, None if absent or disabled; ValueError naming the key otherwise.  The
    values are judged whether the block is enabled or not; the channel order only when it is."""
    j = cfg.INPUT.get("COLOR_JITTER", None)
    if j is None:
        return None
    for name in ("BRIGHTNESS", "CONTRAST", "SATURATION"):
        v = j[name]
        if not (isinstance(v, (tuple, list)) and len(v) == 2 and all(_number(a) for a in v) and 0 <= v[0] <= v[1]):
            raise ValueError("INPUT.COLOR_JITTER.{} {!r}: two finite numbers (intensity_min, intensity_max) with 0 <= min <= max".format(name, v))
    if not _number(j.LIGHTING) or j.LIGHTING < 0:
        raise ValueError("INPUT.COLOR_JITTER.LIGHTING {!r}: a finite number >= 0".format(j.LIGHTING))
    if not _number(j.PROB) or not 0.0 <= j.PROB <= 1.0:
        raise ValueError("INPUT.COLOR_JITTER.PROB {!r}: a number in [0, 1]".format(j.PROB))
    if j.TWIN not in COLOR_JITTER_TWINS:
        raise ValueError("INPUT.COLOR_JITTER.TWIN {!r}: one of {}".format(j.TWIN, COLOR_JITTER_TWINS))
    if not j.ENABLED:
        return None
    channels = tuple(float(a) for a in j.SATURATION) != (1.0, 1.0) or j.LIGHTING != 0
    if channels and cfg.INPUT.FORMAT not in ("RGB", "BGR"):
        raise ValueError("INPUT.FORMAT {!r}: INPUT.COLOR_JITTER.SATURATION and .LIGHTING need RGB or BGR channels".format(cfg.INPUT.FORMAT))
    return j
