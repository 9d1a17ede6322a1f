"""Pascal VOC detection evaluation (CPU / numpy) -- detectron2/evaluation/pascal_voc_evaluation.py:20-313.

``PascalVOCDetectionEvaluator`` keeps the reference's protocol: ``reset()``, ``process(inputs, outputs)`` per batch,
``evaluate()`` on every rank (predictions are gathered to rank 0) returning
``{"bbox": {"AP", "AP50", "AP75", "AP50-<class>"..., "AP50-present", "AP-present"}}`` with AP in percent: VOC07 11-point AP for
year 2007, area under the monotone precision envelope otherwise, averaged over IoU thresholds 0.50:0.05:0.95 for "AP"; the two
"-present" keys are the AP50 / AP means over the classes that have a non-difficult ground-truth box in the set.  With ``device``
the matching runs on the GPU (cddmsl_voc_match) and the dictionary is the same, value for value.

Details that decide the numbers and are therefore kept exactly:
* a detection is serialised the way the reference writes its result files -- score to 3 decimals, box to 1 decimal, with
  +1 on xmin/ymin (the inverse of the loader's -1, datasets/pascal_voc.py) -- and evaluated from those rounded values;
* detections are ranked with ``np.argsort(-confidence)`` on the per-class list in processing order (ties between equal
  rounded scores fall where that call puts them);
* overlaps use the devkit's inclusive pixel convention (+1 on widths/heights), a match needs IoU strictly above the threshold,
  "difficult" ground truth neither counts as positive nor as false positive, a second match of one box is a false positive.
"""
import os
import xml.etree.ElementTree as ET
from collections import OrderedDict, defaultdict

import numpy as np
import torch

def gather_to_rank0(part):
    """The evaluators' one gather: without a process group (or with one rank) ``[part]``; else rank 0 gets every rank's part in rank
    order and the other ranks None.  Each caller merges the list in its own way."""
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1):
        return [part]
    parts = [None] * dist.get_world_size() if dist.get_rank() == 0 else None
    dist.gather_object(part, parts, dst=0)
    return parts


def merge_by_key(parts):
    """the ranks' dictionaries (keyed by image) -> one, a later rank's entry replacing an earlier rank's; None stays None"""
    if parts is None:
        return None
    merged = {}
    for part in parts:
        merged.update(part)
    return merged


def matching_device(device):
    """the evaluators' ``device`` argument -> a non-CPU ``torch.device`` (the matching runs there), or None (it runs on the host)"""
    return torch.device(device) if device is not None and torch.device(device).type != "cpu" else None


VOC_CLASS_NAMES = ("aeroplane", "bicycle", "bird", "boat", "bottle", "bus", "car", "cat", "chair", "cow", "diningtable", "dog",
                   "horse", "motorbike", "person", "pottedplant", "sheep", "sofa", "train", "tvmonitor")   # datasets/pascal_voc.py:19-24


def read_voc_objects(xml_path):
    """One annotation file -> list of {name, difficult, bbox [xmin, ymin, xmax, ymax] (1-based ints as stored)}"""
    out = []
    for obj in ET.parse(xml_path).getroot().findall("object"):
        bb = obj.find("bndbox")
        out.append({"name": obj.find("name").text, "difficult": int(obj.find("difficult").text),
                    "bbox": [int(bb.find(k).text) for k in ("xmin", "ymin", "xmax", "ymax")]})
    return out


def average_precision(rec, prec, use_07_metric):
    """VOC AP from a recall / precision curve (pascal_voc_evaluation.py:166-196)"""
    if use_07_metric:
        ap = 0.0
        for t in np.arange(0.0, 1.1, 0.1):
            sel = rec >= t
            ap += (np.max(prec[sel]) if sel.any() else 0.0) / 11.0
        return ap
    mrec = np.concatenate(([0.0], rec, [1.0]))
    mpre = np.concatenate(([0.0], prec, [0.0]))
    mpre = np.maximum.accumulate(mpre[::-1])[::-1]            # precision envelope
    step = np.where(mrec[1:] != mrec[:-1])[0]
    return float(np.sum((mrec[step + 1] - mrec[step]) * mpre[step + 1]))


def class_ap(image_ids, confidence, boxes, gt_by_image, ovthresh, use_07_metric):
    """AP of one class at one IoU threshold.  ``gt_by_image[id] = (bbox [G,4] float, difficult [G] bool)`` for that class."""
    npos = sum(int((~d).sum()) for _, d in gt_by_image.values())
    claimed = {k: np.zeros(len(d), dtype=bool) for k, (_, d) in gt_by_image.items()}
    order = np.argsort(-confidence)
    tp, fp = np.zeros(len(order)), np.zeros(len(order))
    for rank, d in enumerate(order):
        gtb, diff = gt_by_image[image_ids[d]]
        best, arg = -np.inf, -1
        if gtb.size:
            bb = boxes[d]
            iw = np.maximum(np.minimum(gtb[:, 2], bb[2]) - np.maximum(gtb[:, 0], bb[0]) + 1.0, 0.0)
            ih = np.maximum(np.minimum(gtb[:, 3], bb[3]) - np.maximum(gtb[:, 1], bb[1]) + 1.0, 0.0)
            inter = iw * ih
            union = (bb[2] - bb[0] + 1.0) * (bb[3] - bb[1] + 1.0) + (gtb[:, 2] - gtb[:, 0] + 1.0) * (gtb[:, 3] - gtb[:, 1] + 1.0) - inter
            ov = inter / union
            arg = int(np.argmax(ov))
            best = ov[arg]
        if best > ovthresh:
            if not diff[arg]:
                if not claimed[image_ids[d]][arg]:
                    tp[rank] = 1.0
                    claimed[image_ids[d]][arg] = True
                else:
                    fp[rank] = 1.0
        else:
            fp[rank] = 1.0
    fp, tp = np.cumsum(fp), np.cumsum(tp)
    rec = tp / float(npos) if npos else tp * np.nan          # no positives: the reference divides by zero as well
    prec = tp / np.maximum(tp + fp, np.finfo(np.float64).eps)
    return average_precision(rec, prec, use_07_metric)


VOC_IOU_THRS = tuple(range(50, 100, 5))              # percent; the walk compares with t / 100.0


def voc_round_boxes(boxes):
    """f32 XYXY [D, 4] -> f64 [D, 4]: what the reference's result line ``{xmin:.1f} {ymin:.1f} {xmax:.1f} {ymax:.1f}`` (with + 1 on
    xmin / ymin, an f32 addition) reads back as -- ``float(f"{x0 + 1:.1f}")`` without the text.  An f32 times 10 is exact in f64,
    Python's formatting rounds the exact value half-even like ``rint``, and the division is the nearest double, which is what
    ``float("...")`` returns.  cddmsl_voc_match does the same per detection."""
    b = np.asarray(boxes, dtype=np.float32).reshape(-1, 4)
    out = np.empty(b.shape, dtype=np.float64)
    out[:, :2] = np.rint((b[:, :2] + np.float32(1.0)).astype(np.float64) * 10.0) / 10.0
    out[:, 2:] = np.rint(b[:, 2:].astype(np.float64) * 10.0) / 10.0
    return out


def voc_round_scores(scores):
    """f32 [D] -> f64 [D]: ``float(f"{s:.3f}")`` without the text (see ``voc_round_boxes``)"""
    return np.rint(np.asarray(scores, dtype=np.float32).astype(np.float64) * 1000.0) / 1000.0


def voc_accumulate(tp_bits, fp_bits, npos, use_07_metric, num_thrs=len(VOC_IOU_THRS)):
    """The second half of ``class_ap`` for all thresholds of one class: ``tp_bits`` / ``fp_bits`` [n] hold the walk's flags of the
    class's detections IN RANK ORDER (bit t = threshold t) -> [AP at threshold t].  Cumulative sums of 0 / 1 flags are exact and
    ``rec`` / ``prec`` / ``average_precision`` are ``class_ap``'s expressions, so the values are equal to its, not close."""
    sh = np.arange(num_thrs, dtype=np.int64)[:, None]
    tp = np.cumsum(((np.asarray(tp_bits).astype(np.int64)[None, :] >> sh) & 1).astype(np.float64), axis=1)
    fp = np.cumsum(((np.asarray(fp_bits).astype(np.int64)[None, :] >> sh) & 1).astype(np.float64), axis=1)
    rec = tp / float(npos) if npos else tp * np.nan
    prec = tp / np.maximum(tp + fp, np.finfo(np.float64).eps)
    return [average_precision(rec[t], prec[t], use_07_metric) for t in range(num_thrs)]


def voc_segments(cls, img, conf, class_ids, n_images):
    """How ``class_ap`` visits the gathered detections, as cddmsl_voc_match wants it: per class of ``class_ids`` the rank order
    ``np.argsort(-conf)`` over the class's detections in processing order (the same call on the same values as ``class_ap``'s, so
    equal rounded scores fall the same way), then a stable partition of that order by image.
    -> (ranked {class: detection indices in rank order}, perm int64 [P], seg_off int64 [S + 1], seg_gt int64 [S] = class * n_images +
    image index)."""
    ranked, perm, seg_len, seg_gt = {}, [], [], []
    for cid in class_ids:
        sel = np.flatnonzero(cls == cid)
        r = sel[np.argsort(-np.ascontiguousarray(conf[sel], dtype=np.float64))]
        ranked[cid] = r
        if not r.size:
            continue
        seg = r[np.argsort(img[r], kind="stable")]
        im = img[seg]
        starts = np.flatnonzero(np.concatenate([[True], im[1:] != im[:-1]]))
        perm.append(seg)
        seg_len.append(np.diff(np.concatenate([starts, [len(seg)]])))
        seg_gt.append(cid * n_images + im[starts])
    cat = lambda parts: np.concatenate(parts).astype(np.int64) if parts else np.zeros(0, dtype=np.int64)
    seg_off = np.concatenate([[0], np.cumsum(cat(seg_len))]).astype(np.int64)
    return ranked, cat(perm), seg_off, cat(seg_gt)


def merge_voc_records(parts):
    """the ranks' (boxes, scores, classes, image indices) -> one set, in rank order and inside a rank in processing order: the order
    ``merged[c].extend(lines)`` gives the host path's per-class lists"""
    parts = [p for p in parts if p is not None]
    return tuple(np.concatenate([np.asarray(p[k]) for p in parts]) for k in range(4))


class PascalVOCDetectionEvaluator:
    """``device``: a GPU device moves the matching there (cddmsl_voc_match).  ``process`` keeps each call's detections on the
    device -- no copy to the host, no synchronisation; ``evaluate`` reads them back in ONE copy per rank, gathers the arrays to
    rank 0 in rank order and processing order (the order the host path's per-class lists have), sorts per class on the host with
    ``class_ap``'s own call, matches every (class, image) at all ten thresholds in ONE launch and accumulates with
    ``voc_accumulate``.  Same dictionary as without ``device``, value for value.  The ground truth is parsed once per evaluator."""

    def __init__(self, dirname, split, year, class_names=VOC_CLASS_NAMES, target_classnames=None, device=None):
        assert year in (2007, 2012), year
        self.anno = os.path.join(dirname, "Annotations", "{}.xml")
        self.image_set = os.path.join(dirname, "ImageSets", "Main", split + ".txt")
        self.class_names = list(class_names)
        self.target_classnames = list(target_classnames) if target_classnames is not None else list(class_names)
        self.is_2007 = year == 2007
        self.device = matching_device(device)
        self._gt, self._gt_dev = None, None
        self.reset()

    def reset(self):
        self._predictions = defaultdict(list)        # class id -> [(image_id, score, xmin, ymin, xmax, ymax)] as written
        self._batches = []                           # device path: (image index, [n, 6] int32 rows still on the device) per image

    def _ground_truth(self):
        """-> (image names, per class {image name: (bbox [G,4] float, difficult [G] bool)}), parsed once"""
        if self._gt is None:
            with open(self.image_set) as f:
                image_names = [l.strip() for l in f.readlines()]
            recs = {n: read_voc_objects(self.anno.format(n)) for n in image_names}
            per_class = []
            for cname in self.class_names:
                gt = {}
                for n in image_names:
                    objs = [o for o in recs[n] if o["name"] == cname]
                    gt[n] = (np.array([o["bbox"] for o in objs], dtype=float).reshape(-1, 4), np.array([o["difficult"] for o in objs], dtype=bool))
                per_class.append(gt)
            self._gt = (image_names, per_class)
        return self._gt

    def _device_ground_truth(self):
        """-> (image id -> index in the image-set file's order, hip.VocGroundTruth), uploaded once"""
        if self._gt_dev is None:
            from . import hip
            image_names, per_class = self._ground_truth()
            rows = [gt[n] for gt in per_class for n in image_names]             # row = class * n_images + image index
            self._gt_dev = ({n: i for i, n in enumerate(image_names)},
                            hip.VocGroundTruth.from_host(rows, [t / 100.0 for t in VOC_IOU_THRS], self.device))
        return self._gt_dev

    def _process_device(self, inputs, outputs):
        index = self._device_ground_truth()[0]
        for inp, out in zip(inputs, outputs):
            i = index[str(inp["image_id"])]          # an image outside the set: KeyError (the host path raises it in evaluate)
            inst = out["instances"]
            b, s, c = inst.pred_boxes.tensor.detach(), inst.scores.detach(), inst.pred_classes.detach()
            if b.dtype != torch.float32 or s.dtype != torch.float32:
                raise TypeError(f"PascalVOCDetectionEvaluator(device=...): detections must be f32, got boxes {b.dtype}, scores {s.dtype}")
            b, s, c = (t.to(self.device, non_blocking=True) for t in (b, s, c))
            rows = torch.cat([b.reshape(-1, 4).view(torch.int32), s.reshape(-1, 1).view(torch.int32), c.reshape(-1, 1).to(torch.int32)], dim=1)
            self._batches.append((i, rows))

    def _device_records(self):
        """the ONE readback -> (boxes f32 [n,4], scores f32 [n], classes int64 [n], image indices int64 [n]) in processing order"""
        if not self._batches:
            return np.zeros((0, 4), dtype=np.float32), np.zeros(0, dtype=np.float32), np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)
        tab = torch.cat([r for _, r in self._batches]).cpu().numpy()
        img = np.repeat(np.array([i for i, _ in self._batches], dtype=np.int64), [len(r) for _, r in self._batches])
        return (np.ascontiguousarray(tab[:, :4]).view(np.float32), np.ascontiguousarray(tab[:, 4]).view(np.float32),
                tab[:, 5].astype(np.int64), img)

    def _gathered_records(self):
        parts = gather_to_rank0(self._device_records())
        return None if parts is None else merge_voc_records(parts)

    def _match_device(self, rec, class_ids):
        """rank 0: one upload, ONE launch for all classes and thresholds, one readback -> {class: (tp bits, fp bits) in rank order}"""
        from . import hip
        from ._lib import to_device_async
        boxes, scores, cls, img = rec
        n_images = len(self._ground_truth()[0])
        ranked, perm, seg_off, seg_gt = voc_segments(cls, img, voc_round_scores(scores), class_ids, n_images)
        D, P, S = len(boxes), len(perm), len(seg_gt)
        if P == 0:
            return {c: (np.zeros(0, dtype=np.uint16), np.zeros(0, dtype=np.uint16)) for c in class_ids}
        boxes = np.ascontiguousarray(boxes, dtype=np.float32)
        buf = to_device_async(torch.from_numpy(np.concatenate([boxes.reshape(-1).view(np.int64), perm, seg_off, seg_gt])), self.device)
        tp, fp, bad = hip.voc_match(buf[: 2 * D].view(torch.float32).view(D, 4), buf[2 * D: 2 * D + P], buf[2 * D + P: 2 * D + P + S + 1],
                                    buf[2 * D + P + S + 1:], self._device_ground_truth()[1])
        host = torch.cat([tp.to(torch.int32), fp.to(torch.int32), bad]).cpu().numpy()
        if host[2 * D:].any():
            raise RuntimeError("cddmsl_voc_match refused a segment the evaluator built: inconsistent offsets")
        tp, fp = (host[:D] & 0xFFFF).astype(np.uint16), (host[D: 2 * D] & 0xFFFF).astype(np.uint16)
        return {c: (tp[r], fp[r]) for c, r in ranked.items()}

    def process(self, inputs, outputs):
        if self.device is not None:
            return self._process_device(inputs, outputs)
        for inp, out in zip(inputs, outputs):
            inst = out["instances"]
            boxes = inst.pred_boxes.tensor.detach().cpu().numpy()
            scores = inst.scores.detach().cpu().tolist()
            classes = inst.pred_classes.detach().cpu().tolist()
            for (x0, y0, x1, y1), s, c in zip(boxes, scores, classes):
                # what the reference's result line "{id} {score:.3f} {xmin:.1f} {ymin:.1f} {xmax:.1f} {ymax:.1f}" reads back as
                self._predictions[c].append((str(inp["image_id"]), float(f"{s:.3f}"), float(f"{x0 + 1:.1f}"), float(f"{y0 + 1:.1f}"),
                                             float(f"{x1:.1f}"), float(f"{y1:.1f}")))

    def _gathered(self):
        parts = gather_to_rank0(dict(self._predictions))
        if parts is None:
            return None
        merged = defaultdict(list)
        for part in parts:
            for c, lines in part.items():
                merged[c].extend(lines)
        return merged

    def evaluate(self):
        if self.device is not None:
            rec = self._gathered_records()
            return None if rec is None else self.evaluate_records(rec)
        preds = self._gathered()
        return None if preds is None else self._evaluate(preds, None)

    def evaluate_records(self, rec):
        """the device path's rank-0 half on gathered records (``_device_records`` of one rank, or ``merge_voc_records`` of several)"""
        return self._evaluate(None, rec)

    def _evaluate(self, preds, rec):
        _, per_class = self._ground_truth()
        class_ids = [cid for cid, cname in enumerate(self.class_names) if cname in self.target_classnames]
        if rec is not None:
            flags = self._match_device(rec, class_ids)
        aps, npos = defaultdict(list), []
        for cid in class_ids:
            gt = per_class[cid]
            npos.append(sum(int((~d).sum()) for _, d in gt.values()))
            if rec is not None:
                for thresh, ap in zip(VOC_IOU_THRS, voc_accumulate(*flags[cid], npos[-1], self.is_2007)):
                    aps[thresh].append(ap * 100)
                continue
            lines = preds.get(cid, [])
            ids = [l[0] for l in lines]
            conf = np.array([l[1] for l in lines], dtype=float)
            bbs = np.array([l[2:] for l in lines], dtype=float).reshape(-1, 4)
            for thresh in VOC_IOU_THRS:
                aps[thresh].append(class_ap(ids, conf, bbs, gt, thresh / 100.0, self.is_2007) * 100)
        mean = {t: float(np.mean(v)) for t, v in aps.items()}
        ret = OrderedDict()
        ret["bbox"] = {"AP": float(np.mean(list(mean.values()))), "AP50": mean[50], "AP75": mean[75]}
        for i, name in enumerate(self.target_classnames):
            ret["bbox"]["AP50-" + name] = aps[50][i]
        # the same means over the classes the set annotates (at least one non-difficult box): Watercolor and Comic annotate 6 of the
        # 20 classes, and with the 2012 metric a class without positives is a NaN that the means above keep, as the reference does
        present = [i for i, n in enumerate(npos) if n > 0]
        over = {t: float(np.mean([v[i] for i in present])) if present else float("nan") for t, v in aps.items()}
        ret["bbox"]["AP50-present"] = over[50]
        ret["bbox"]["AP-present"] = float(np.mean(list(over.values())))
        return ret


@torch.no_grad()
def inference_on_dataset(model, data_loader, evaluator):
    """evaluation/evaluator.py:85-181 without the timing log: eval mode, one ``process`` per batch, then ``evaluate``."""
    was_training = model.training
    model.eval()
    evaluator.reset()
    for inputs in data_loader:
        evaluator.process(inputs, model(inputs))
    model.train(was_training)
    return evaluator.evaluate()


def run_eval_only(model, cfg, args, rank=0, world=1, return_results=False, prefix="", weight_average=None):
    """tools/train_caption_consistency.py:143-152 (``--eval-only``): VOC-style test set under ``args.voc_root`` -> AP dict
    printed by rank 0.  Every rank evaluates its shard of the test set (``world`` has to be the process group's size: the
    evaluator merges all ranks' detections, so unsharded ranks would count every detection ``world`` times).  Returns the
    process exit code (or the result dict: rank 0, ``return_results``).  ``weight_average`` (MODEL_EMA): see ``averaged_passes``."""
    res = None
    for averaged, weights in averaged_passes(model, cfg, weight_average):
        with weights:
            part = _eval_only_pass(model, cfg, args, rank, world, prefix, averaged)
        if part is not None:
            res = part if res is None else res
            res.update(part)
    return res if return_results else 0


def _eval_only_pass(model, cfg, args, rank, world, prefix, averaged):
    """one pass of ``run_eval_only`` over the weights the model holds now; ``averaged``: its task keys carry ``_EMA``"""
    mark = with_ema_suffix if averaged else (lambda r: r)
    import torch.distributed as dist
    ws = dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1
    assert world == ws, f"run_eval_only: world={world} but the process group has {ws} ranks"
    from .data import build_detection_test_loader, load_voc_instances
    names = VOC_CLASS_NAMES[: num_test_classes(model, cfg)]
    dicts = load_voc_instances(args.voc_root, args.voc_split, names)
    loader = build_detection_test_loader(cfg, dicts, batch_size=1, rank=rank, world=world, device=cfg.MODEL.DEVICE)
    ev = PascalVOCDetectionEvaluator(args.voc_root, args.voc_split, args.voc_year, names)
    res = mark(inference_on_dataset(model, loader, with_proposal_recall(ev, model, cfg, dicts)))
    if rank == 0:
        _print_results(prefix, res)
    if tta_enabled(cfg) and not is_proposal_network(model):            # train_caption_consistency.py:105-118,149-150: the same set again through the TTA model
        loader = build_detection_test_loader(cfg, dicts, batch_size=1, rank=rank, world=world, device=cfg.MODEL.DEVICE)
        tta = mark(with_tta_suffix(inference_on_dataset(tta_model(cfg, model), loader, ev)))
        if rank == 0:
            print(prefix + str({k: {m: round(v, 4) for m, v in r.items()} for k, r in tta.items()}))
            res.update(tta)
    return res


def num_test_classes(model, cfg):
    """classes of the detections the model returns: the box head's test vocabulary (open-set inference evaluates on another
    vocabulary than the head was trained on), NUM_CLASSES for a model without such a head"""
    from .modeling.tta_vocabulary import merge_num_classes
    return merge_num_classes(model, cfg)


def tta_enabled(cfg):
    return bool(cfg.TEST.get("AUG", {}).get("ENABLED", False))


def tta_model(cfg, model):
    """``GeneralizedRCNNWithTTA(cfg, model)`` (looked up at call time: with ``TEST.AUG.ENABLED`` off it is never constructed)"""
    from .modeling import test_time_augmentation
    return test_time_augmentation.GeneralizedRCNNWithTTA(cfg, model)


def with_tta_suffix(res):
    """train_caption_consistency.py:117: ``{k + "_TTA": v}`` over the top-level keys (``bbox_TTA``); None (not rank 0) stays empty"""
    return OrderedDict((k + "_TTA", v) for k, v in (res or {}).items())


def with_ema_suffix(res):
    """``{k + "_EMA": v}`` over the top-level keys, for the results of the averaged weights (``bbox_EMA``, ``bbox_TTA_EMA``,
    ``box_proposals_EMA``; in the storage ``<dataset>/bbox_EMA/AP``); None (not rank 0) stays empty"""
    return OrderedDict((k + "_EMA", v) for k, v in (res or {}).items())


def averaged_passes(model, cfg, weight_average):
    """The passes of one evaluation under ``MODEL_EMA``: [(averaged, context manager)].  The plain pass runs the weights the model
    holds; the averaged one runs inside ``weight_average.applied(model)`` and reports under ``_EMA`` keys -- also when it is the only
    pass (``EVAL "averaged"``), so that a key never means two things.  Without a WeightAverage that has been updated at least once
    (feature off, ``EVAL "plain"``, a checkpoint without the entry) there is the plain pass alone."""
    import contextlib
    from .config import check_model_ema
    e = check_model_ema(cfg)
    if e is None or weight_average is None or weight_average.updates == 0 or e.EVAL == "plain":
        return [(False, contextlib.nullcontext())]
    averaged = (True, weight_average.applied(model))
    return [averaged] if e.EVAL == "averaged" else [(False, contextlib.nullcontext()), averaged]


# ------------------------------------------------------------------------------------------------ COCO-style box AP
COCO_IOU_THRS = np.linspace(0.5, 0.95, 10)
COCO_REC_THRS = np.linspace(0.0, 1.0, 101)
COCO_AREA_RNGS = ((0.0, 1e5 ** 2), (0.0, 32.0 ** 2), (32.0 ** 2, 96.0 ** 2), (96.0 ** 2, 1e5 ** 2))    # all, small, medium, large
COCO_MAX_DETS = 100


def coco_box_iou(dt, gt, iscrowd):
    """pycocotools ``maskUtils.iou`` on XYWH boxes: [D,G] IoU; against a crowd GT the union is the detection's own area"""
    if len(dt) == 0 or len(gt) == 0:
        return np.zeros((len(dt), len(gt)))
    iw = np.minimum(dt[:, None, 0] + dt[:, None, 2], gt[None, :, 0] + gt[None, :, 2]) - np.maximum(dt[:, None, 0], gt[None, :, 0])
    ih = np.minimum(dt[:, None, 1] + dt[:, None, 3], gt[None, :, 1] + gt[None, :, 3]) - np.maximum(dt[:, None, 1], gt[None, :, 1])
    inter = np.maximum(iw, 0.0) * np.maximum(ih, 0.0)
    da, ga = dt[:, 2] * dt[:, 3], gt[:, 2] * gt[:, 3]
    union = np.where(np.asarray(iscrowd, dtype=bool)[None, :], da[:, None], da[:, None] + ga[None, :] - inter)
    return inter / union


def _coco_match(dt_boxes, dt_scores, gt_boxes, gt_area, gt_crowd, area_rng):
    """``COCOeval.evaluateImg`` for one (image, class, area range): -> (scores, matched [T,D] bool, ignored [T,D] bool, n non-ignored gt)"""
    gt_ig = gt_crowd | (gt_area < area_rng[0]) | (gt_area > area_rng[1])
    gorder = np.argsort(gt_ig, kind="mergesort")                # non-ignored GT first
    gb, gig, gcrowd = gt_boxes[gorder], gt_ig[gorder], gt_crowd[gorder]
    dorder = np.argsort(-dt_scores, kind="mergesort")[:COCO_MAX_DETS]
    db, ds = dt_boxes[dorder], dt_scores[dorder]
    ious = coco_box_iou(db, gb, gcrowd)
    T, D, G = len(COCO_IOU_THRS), len(db), len(gb)
    gtm = np.zeros((T, G), dtype=bool)
    dtm = np.zeros((T, D), dtype=bool)
    dtig = np.zeros((T, D), dtype=bool)
    for ti, t in enumerate(COCO_IOU_THRS):
        for d in range(D):
            iou, m = min(t, 1 - 1e-10), -1
            for g in range(G):
                if gtm[ti, g] and not gcrowd[g]:
                    continue
                if m > -1 and not gig[m] and gig[g]:         # already matched a real GT: stop at the ignored ones
                    break
                if ious[d, g] < iou:
                    continue
                iou, m = ious[d, g], g
            if m == -1:
                continue
            dtig[ti, d], dtm[ti, d], gtm[ti, m] = gig[m], True, True
    darea = db[:, 2] * db[:, 3]
    out_rng = (darea < area_rng[0]) | (darea > area_rng[1])
    dtig |= ~dtm & out_rng[None, :]
    return ds, dtm, dtig, int((~gig).sum())


def coco_precision(gt_by_image, dt_by_image, num_classes):
    """``COCOeval.evaluate`` + ``accumulate`` (bbox, maxDets 100): precision [T, R=101, K, A=4], -1 where a class has no non-ignored GT.
    ``gt_by_image[img] = (xywh [G,4], area [G], crowd [G] bool, class [G])``, ``dt_by_image[img] = (xywh [D,4], score [D], class [D])``."""
    T, R, A = len(COCO_IOU_THRS), len(COCO_REC_THRS), len(COCO_AREA_RNGS)
    prec = -np.ones((T, R, num_classes, A))
    imgs = list(gt_by_image)
    for k in range(num_classes):
        for a, rng in enumerate(COCO_AREA_RNGS):
            scores, dtm, dtig, npig = [], [], [], 0
            for img in imgs:
                gb, garea, gcrowd, gcls = gt_by_image[img]
                g = gcls == k
                db, dsc, dcls = dt_by_image.get(img, (np.zeros((0, 4)), np.zeros(0), np.zeros(0, dtype=np.int64)))
                d = dcls == k
                if not g.any() and not d.any():
                    continue
                s, m, ig, n = _coco_match(db[d], dsc[d], gb[g], garea[g], gcrowd[g], rng)
                scores.append(s); dtm.append(m); dtig.append(ig); npig += n
            if npig == 0:
                continue
            s = np.concatenate(scores) if scores else np.zeros(0)
            order = np.argsort(-s, kind="mergesort")
            m = np.concatenate(dtm, axis=1)[:, order] if dtm else np.zeros((T, 0), dtype=bool)
            ig = np.concatenate(dtig, axis=1)[:, order] if dtig else np.zeros((T, 0), dtype=bool)
            tps = np.cumsum(m & ~ig, axis=1, dtype=np.float64)
            fps = np.cumsum(~m & ~ig, axis=1, dtype=np.float64)
            for t in range(T):
                tp, fp = tps[t], fps[t]
                rc = tp / npig
                pr = (tp / (fp + tp + np.spacing(1))).tolist()
                for i in range(len(pr) - 1, 0, -1):           # precision envelope, from the right
                    if pr[i] > pr[i - 1]:
                        pr[i - 1] = pr[i]
                q = np.zeros(R)
                inds = np.searchsorted(rc, COCO_REC_THRS, side="left")
                for ri, pi in enumerate(inds):
                    if pi < len(pr):
                        q[ri] = pr[pi]
                prec[t, :, k, a] = q
    return prec


# ---- the same in two halves: per-detection records (from hip.coco_match, or from coco_match_host below) -> coco_accumulate
COCO_RECORD_FIELDS = (("score", np.float64), ("cls", np.int64), ("img", np.int64), ("rank", np.int32), ("matched", np.int64), ("ignored", np.int64))


def empty_coco_records():
    return {k: np.zeros(0, dtype=dt) for k, dt in COCO_RECORD_FIELDS}


def coco_match_host(gt, dt, num_classes):
    """``hip.coco_match``'s outputs for ONE image from the host matcher: ``gt = (xywh, area, crowd, class)``, ``dt = (xywh, score,
    class)`` -> (rank int32 [D], matched int64 [D], ignored int64 [D]) in the detections' input order; bit ``a * T + t`` of a mask is
    ``_coco_match``'s flag at threshold t in area range a, rank is the position in ``argsort(-score, mergesort)`` of the detection's
    class, -1 beyond COCO_MAX_DETS (masks 0).  The no-device path, and what an image beyond the kernel's caps goes through."""
    gb, garea, gcrowd, gcls = gt
    db, ds, dc = dt
    T = len(COCO_IOU_THRS)
    rank = -np.ones(len(ds), dtype=np.int32)
    matched, ignored = np.zeros(len(ds), dtype=np.int64), np.zeros(len(ds), dtype=np.int64)
    for k in range(num_classes):
        d = np.flatnonzero(dc == k)
        if not d.size:
            continue
        g = gcls == k
        kept = d[np.argsort(-ds[d], kind="mergesort")[:COCO_MAX_DETS]]
        rank[kept] = np.arange(len(kept), dtype=np.int32)
        for a, rng in enumerate(COCO_AREA_RNGS):
            _, m, ig, _ = _coco_match(db[d], ds[d], gb[g], garea[g], gcrowd[g], rng)
            bits = (np.int64(1) << (a * T + np.arange(T, dtype=np.int64)))[:, None]
            matched[kept] |= (m * bits).sum(axis=0)
            ignored[kept] |= (ig * bits).sum(axis=0)
    return rank, matched, ignored


def coco_gt_counts(gt_per_image, num_classes):
    """non-ignored ground truth per (class, area range) -> int64 [K, A]: what ``coco_precision`` sums up as ``npig``"""
    n = np.zeros((num_classes, len(COCO_AREA_RNGS)), dtype=np.int64)
    for _, garea, gcrowd, gcls in gt_per_image:
        for a, rng in enumerate(COCO_AREA_RNGS):
            ok = ~(gcrowd | (garea < rng[0]) | (garea > rng[1])) & (gcls >= 0) & (gcls < num_classes)
            np.add.at(n[:, a], gcls[ok], 1)
    return n


def merge_coco_records(parts):
    """records of several evaluators (ranks) -> one set ordered by data-set image index, then by rank inside the image: the order in
    which ``coco_precision`` concatenates its per-image results, so equal scores of different images fall the same way"""
    parts = [p for p in parts if p is not None]
    rec = {k: np.concatenate([np.asarray(p[k], dtype=dt) for p in parts] or [np.zeros(0, dtype=dt)]) for k, dt in COCO_RECORD_FIELDS}
    order = np.lexsort((rec["rank"], rec["img"]))
    return {k: v[order] for k, v in rec.items()}


def coco_accumulate(rec, npig, num_classes):
    """``COCOeval.accumulate`` on per-detection records (the second half of ``coco_precision``, vectorised; exactly equal to it):
    ``rec`` = arrays score / cls / img / rank / matched / ignored over the KEPT detections (rank >= 0) of all images, any order;
    ``npig`` int [K, A] from ``coco_gt_counts``.  -> precision [T, 101, K, A], -1 where a class has no non-ignored ground truth."""
    T, R, A = len(COCO_IOU_THRS), len(COCO_REC_THRS), len(COCO_AREA_RNGS)
    prec = -np.ones((T, R, num_classes, A))
    base = np.lexsort((rec["rank"], rec["img"]))
    cls = rec["cls"][base]
    for k in range(num_classes):
        if not npig[k].any():
            continue
        sel = base[cls == k]
        sel = sel[np.argsort(-rec["score"][sel], kind="mergesort")]
        N = len(sel)
        mbits, ibits = rec["matched"][sel], rec["ignored"][sel]
        for a in range(A):
            if npig[k, a] == 0:
                continue
            sh = (a * T + np.arange(T, dtype=np.int64))[:, None]
            m, ig = ((mbits[None, :] >> sh) & 1).astype(bool), ((ibits[None, :] >> sh) & 1).astype(bool)
            tps = np.cumsum(m & ~ig, axis=1, dtype=np.float64)
            fps = np.cumsum(~m & ~ig, axis=1, dtype=np.float64)
            rc = tps / int(npig[k, a])
            pr = tps / (fps + tps + np.spacing(1))
            pr = np.maximum.accumulate(pr[:, ::-1], axis=1)[:, ::-1]      # precision envelope, from the right
            for t in range(T):
                inds = np.searchsorted(rc[t], COCO_REC_THRS, side="left")
                q = np.zeros(R)
                ok = inds < N
                q[ok] = pr[t, inds[ok]]
                prec[t, :, k, a] = q
    return prec


class COCODetectionEvaluator:
    """COCO-style box AP (evaluation/coco_evaluation.py:292-360 over pycocotools ``COCOeval``, iouType "bbox") in numpy, with the
    same ``reset / process / evaluate`` protocol and rank-0 gather as ``PascalVOCDetectionEvaluator``.  pycocotools is not a
    dependency: parity unpinned against pycocotools -- the semantics below restate its published behaviour.

    Ground truth comes from the dataset dicts: XYWH = (xmin, ymin, xmax - xmin, ymax - ymin), ``area`` as stored (the Cityscapes
    loader stores the mask's pixel count, what D2's ``mask_util.area`` gives its RLE annotations), ``iscrowd`` regions are ignored
    GT whose IoU with a detection is intersection over the detection's area.  Detections: XYXY -> XYWH, unrounded
    (``instances_to_coco_json``).  Per (image, class) the top 100 by score (stable order) are matched at IoU .50:.05:.95 to the best
    still-unmatched GT (non-ignored GT preferred; a detection matched to an ignored GT is ignored); area ranges all / small (<= 32^2)
    / medium / large (> 96^2) judge the GT by ``area`` and unmatched detections by their box area; precision is made monotone from
    the right and sampled at 101 recall points; classes without non-ignored GT are left out of the means.  Returns
    ``{"bbox": {AP, AP50, AP75, APs, APm, APl, "AP-<class>"...}}`` in percent; NaN where nothing is defined (every key when there
    are no detections at all).

    ``device``: a GPU device moves the matching there.  The ground truth is uploaded once; ``process`` copies nothing to the host and
    does not synchronise -- one ``hip.coco_match`` launch per call matches the batch's detections where the model left them;
    ``evaluate`` reads the per-detection records (score, class, rank, two 40-bit masks) back in ONE copy, gathers only those to
    rank 0 and runs ``coco_accumulate``.  Same dictionary as without ``device``, value for value.  An image beyond the kernel's caps
    (hip.COCO_MATCH_MAX_DETS / COCO_MATCH_MAX_GT of one class) is matched by ``coco_match_host``, never truncated."""

    def __init__(self, dataset_dicts, class_names, device=None):
        self.class_names = list(class_names)
        self.device = matching_device(device)
        self._gt = {}
        for d in dataset_dicts:
            anns = d.get("annotations", [])
            xyxy = np.array([a["bbox"] for a in anns], dtype=np.float64).reshape(-1, 4)
            xywh = np.concatenate([xyxy[:, :2], xyxy[:, 2:] - xyxy[:, :2]], axis=1)
            area = np.array([a.get("area", (a["bbox"][2] - a["bbox"][0]) * (a["bbox"][3] - a["bbox"][1])) for a in anns], dtype=np.float64)
            crowd = np.array([bool(a.get("iscrowd", 0)) for a in anns], dtype=bool)
            cls = np.array([a["category_id"] for a in anns], dtype=np.int64)
            self._gt[str(d["image_id"])] = (xywh, area, crowd, cls)
        if self.device is not None:
            from . import hip
            self._index = {k: i for i, k in enumerate(self._gt)}      # image id -> data-set index (coco_precision's image order)
            self._gt_list = list(self._gt.values())
            self._gt_dev = hip.CocoGroundTruth.from_host(self._gt_list, np.minimum(COCO_IOU_THRS, 1 - 1e-10), COCO_AREA_RNGS, self.device)
        self.reset()

    def reset(self):
        self._predictions = {}           # image id -> (xywh [D,4], scores [D], classes [D])
        self._batches = []               # device path: one entry per process() call, everything still on the device

    def _process_device(self, inputs, outputs):
        from . import hip
        from ._lib import to_device_async
        idx, boxes, scores, classes = [], [], [], []
        for inp, out in zip(inputs, outputs):
            i = self._index.get(str(inp["image_id"]))
            if i is None:                # not an image of this data set: the host path never looks at it either
                continue
            inst = out["instances"]
            idx.append(i)
            boxes.append(inst.pred_boxes.tensor.detach().float().reshape(-1, 4))
            scores.append(inst.scores.detach().float().reshape(-1))
            classes.append(inst.pred_classes.detach().long().reshape(-1))
        if not idx:
            return
        lens = [len(s) for s in scores]
        meta = to_device_async(torch.tensor(np.concatenate([[0], np.cumsum(lens), idx]).astype(np.int64)), self.device)
        b, s, c = torch.cat(boxes).contiguous(), torch.cat(scores).contiguous(), torch.cat(classes).contiguous()
        rank, matched, ignored, over = hip.coco_match(b, s, c, meta[: len(idx) + 1], meta[len(idx) + 1:], self._gt_dev, len(self.class_names),
                                                      COCO_MAX_DETS)
        self._batches.append({"idx": idx, "lens": lens, "boxes": b, "scores": s, "cls": c, "rank": rank, "matched": matched,
                              "ignored": ignored, "over": over})

    def _device_records(self):
        """the ONE readback -> (records of the kept detections, number of detections seen)"""
        if not self._batches:
            return empty_coco_records(), 0
        rows = [torch.stack([e["scores"].view(torch.int32).long(), e["cls"], e["rank"].long(), e["matched"], e["ignored"]], dim=1).reshape(-1)
                for e in self._batches]
        host = torch.cat(rows + [e["over"].long() for e in self._batches]).cpu().numpy()
        n = sum(sum(e["lens"]) for e in self._batches)
        tab, over = host[: 5 * n].reshape(n, 5), host[5 * n:]
        score = tab[:, 0].astype(np.int32).view(np.float32).astype(np.float64)
        cls, rank, matched, ignored = tab[:, 1].copy(), tab[:, 2].astype(np.int32), tab[:, 3].copy(), tab[:, 4].copy()
        idx = np.array([i for e in self._batches for i in e["idx"]], dtype=np.int64)
        lens = np.array([l for e in self._batches for l in e["lens"]], dtype=np.int64)
        start = np.concatenate([[0], np.cumsum(lens)])
        img = np.repeat(idx, lens)
        live = np.ones(n, dtype=bool)
        last = {int(i): j for j, i in enumerate(idx)}                # an image processed twice: the later call replaces the earlier
        for j, i in enumerate(idx):
            if last[int(i)] != j:
                live[start[j]: start[j + 1]] = False
        if over.any():                                               # beyond a cap of the kernel: the host matcher, on the same values
            j0 = 0
            for e in self._batches:
                nb = len(e["idx"])
                if over[j0: j0 + nb].any():
                    bx = e["boxes"].cpu().numpy().astype(np.float64)
                    for j in range(j0, j0 + nb):
                        if over[j] and last[int(idx[j])] == j:
                            lo, hi = start[j], start[j + 1]
                            b = bx[lo - start[j0]: hi - start[j0]]
                            xywh = np.concatenate([b[:, :2], b[:, 2:] - b[:, :2]], axis=1)
                            with np.errstate(invalid="ignore", divide="ignore"):        # (a 0 / 0 IoU is a NaN on purpose)
                                rank[lo:hi], matched[lo:hi], ignored[lo:hi] = coco_match_host(self._gt_list[int(idx[j])],
                                                                                              (xywh, score[lo:hi], cls[lo:hi]), len(self.class_names))
                j0 += nb
        keep = live & (rank >= 0)
        rec = {"score": score[keep], "cls": cls[keep], "img": img[keep], "rank": rank[keep], "matched": matched[keep], "ignored": ignored[keep]}
        return rec, int(live.sum())

    def _gathered_records(self):
        parts = gather_to_rank0(self._device_records())
        if parts is None:
            return None, 0
        return merge_coco_records([p[0] for p in parts]), sum(p[1] for p in parts)

    def process(self, inputs, outputs):
        if self.device is not None:
            return self._process_device(inputs, outputs)
        for inp, out in zip(inputs, outputs):
            inst = out["instances"]
            b = inst.pred_boxes.tensor.detach().float().cpu().numpy().astype(np.float64).reshape(-1, 4)
            xywh = np.concatenate([b[:, :2], b[:, 2:] - b[:, :2]], axis=1)
            self._predictions[str(inp["image_id"])] = (xywh, inst.scores.detach().float().cpu().numpy().astype(np.float64),
                                                       inst.pred_classes.detach().cpu().numpy().astype(np.int64))

    def _gathered(self):
        return merge_by_key(gather_to_rank0(self._predictions))

    def evaluate(self):
        if self.device is not None:
            rec, ndet = self._gathered_records()
            if rec is None:
                return None
        else:
            preds = self._gathered()
            if preds is None:
                return None
            ndet = sum(len(p[1]) for p in preds.values())
        metrics = ("AP", "AP50", "AP75", "APs", "APm", "APl")
        res = OrderedDict()
        if ndet == 0:
            res.update({m: float("nan") for m in metrics})
            res.update({"AP-" + n: float("nan") for n in self.class_names})
            return {"bbox": res}
        if self.device is not None:
            prec = coco_accumulate(rec, coco_gt_counts(self._gt_list, len(self.class_names)), len(self.class_names))
        else:
            prec = coco_precision(self._gt, preds, len(self.class_names))

        def mean(p):
            p = p[p > -1]
            return float(np.mean(p)) * 100 if p.size else float("nan")
        res["AP"], res["AP50"], res["AP75"] = mean(prec[:, :, :, 0]), mean(prec[0, :, :, 0]), mean(prec[5, :, :, 0])
        res["APs"], res["APm"], res["APl"] = mean(prec[:, :, :, 1]), mean(prec[:, :, :, 2]), mean(prec[:, :, :, 3])
        for k, n in enumerate(self.class_names):
            res["AP-" + n] = mean(prec[:, :, k, 0])
        return {"bbox": res}


# ------------------------------------------------------------------------------------------------ proposal recall (AR)
# evaluation/coco_evaluation.py:492-511: the named area ranges of _evaluate_box_proposals, in its order
PROPOSAL_AREA_NAMES = ("all", "small", "medium", "large", "96-128", "128-256", "256-512", "512-inf")
PROPOSAL_AREA_RNGS = ((0 ** 2, 1e5 ** 2), (0 ** 2, 32 ** 2), (32 ** 2, 96 ** 2), (96 ** 2, 1e5 ** 2), (96 ** 2, 128 ** 2),
                      (128 ** 2, 256 ** 2), (256 ** 2, 512 ** 2), (512 ** 2, 1e5 ** 2))
PROPOSAL_LIMITS = (100, 1000)                            # coco_evaluation.py:284
PROPOSAL_REPORTED = (("all", ""), ("small", "s"), ("medium", "m"), ("large", "l"))     # coco_evaluation.py:283: range, key suffix


def proposal_area_bits(areas):
    """stored areas -> u8 [G], bit a = the box counts in PROPOSAL_AREA_RNGS[a].  The reference compares
    ``torch.as_tensor([area, ...])`` -- Python floats become float32 -- with ``lo <= area <= hi``, inclusive at both ends, the bounds
    taking the tensor's type: so the areas pass through float32 first (1024.00001 is 1024 and counts as small AND as medium; an
    integer below 2^24 is itself)."""
    a = np.asarray(areas, dtype=np.float64).reshape(-1).astype(np.float32)
    bits = np.zeros(len(a), dtype=np.uint8)
    for i, (lo, hi) in enumerate(PROPOSAL_AREA_RNGS):
        bits |= (((a >= np.float32(lo)) & (a <= np.float32(hi))).astype(np.uint8) << np.uint8(i))
    return bits


def proposal_ground_truth(dataset_dicts):
    """{image id: (boxes f32 [g, 4] XYXY, range bits u8 [g])} in data-set order, as the recall walk reads the dicts: ``iscrowd``
    boxes are left out (coco_evaluation.py:527-534), the area is the stored ``area``, else the box area"""
    gt = OrderedDict()
    for d in dataset_dicts:
        anns = [a for a in d.get("annotations", []) if not a.get("iscrowd", 0)]
        boxes = np.array([a["bbox"] for a in anns], dtype=np.float64).reshape(-1, 4).astype(np.float32)
        areas = [a.get("area", (a["bbox"][2] - a["bbox"][0]) * (a["bbox"][3] - a["bbox"][1])) for a in anns]
        gt[str(d["image_id"])] = (boxes, proposal_area_bits(areas))
    return gt


def pairwise_iou_f32(boxes1, boxes2):
    """structures/boxes.py:322-367 ``pairwise_iou`` in numpy f32, operation for operation: [N, M]"""
    b1, b2 = np.asarray(boxes1, dtype=np.float32).reshape(-1, 4), np.asarray(boxes2, dtype=np.float32).reshape(-1, 4)
    area1 = (b1[:, 2] - b1[:, 0]) * (b1[:, 3] - b1[:, 1])
    area2 = (b2[:, 2] - b2[:, 0]) * (b2[:, 3] - b2[:, 1])
    wh = np.minimum(b1[:, None, 2:], b2[None, :, 2:]) - np.maximum(b1[:, None, :2], b2[None, :, :2])
    wh = np.maximum(wh, np.float32(0))
    inter = wh[:, :, 0] * wh[:, :, 1]
    with np.errstate(invalid="ignore", divide="ignore"):
        iou = inter / (area1[:, None] + area2[None, :] - inter)
    return np.where(inter > 0, iou, np.float32(0)).astype(np.float32)


def proposal_cover_host(boxes, logits, gt_boxes, gt_rng, limits=PROPOSAL_LIMITS, num_ranges=len(PROPOSAL_AREA_RNGS)):
    """``hip.proposal_cover``'s output for ONE image from the host walk -- the per-image body of ``_evaluate_box_proposals``
    (coco_evaluation.py:517-571) for every (limit, area range): ``boxes`` f32 [P, 4] XYXY, ``logits`` f32 [P], ``gt_boxes`` f32
    [G, 4], ``gt_rng`` u8 [G] (``proposal_area_bits``; crowd boxes left out or without a bit), ``limits``: ints, None = no limit
    -> cover f32 [L, A, G]: -1 = the box is not counted (bit clear, or P == 0: the reference skips an image without proposals
    before it adds to num_pos), else the IoU recorded on the box, 0.0 when the walk ended before it.
    The proposals are ranked by logit descending, stably (equal logits by input index, NaN last; the reference's ``Tensor.sort`` is
    not stable, so with equal logits this is one of its possible orders); a pick is ``overlaps.max(dim=0)`` then ``.max(dim=0)`` with
    the first maximal index each time.  The no-device path, and what an image beyond the kernel's caps goes through."""
    boxes = np.asarray(boxes, dtype=np.float32).reshape(-1, 4)
    logits = np.asarray(logits, dtype=np.float32).reshape(-1)
    gt_boxes = np.asarray(gt_boxes, dtype=np.float32).reshape(-1, 4)
    gt_rng = np.asarray(gt_rng, dtype=np.uint8).reshape(-1)
    P, G = len(logits), len(gt_rng)
    cover = -np.ones((len(limits), num_ranges, G), dtype=np.float32)
    if P == 0 or G == 0:
        return cover
    order = np.argsort(-logits, kind="stable")              # NaN last, equal logits by input index
    iou = pairwise_iou_f32(boxes[order], gt_boxes)          # independent of limit and range: rows by rank
    for li, limit in enumerate(limits):
        pk = P if limit is None else min(P, max(int(limit), 0))
        for a in range(num_ranges):
            cols = np.flatnonzero((gt_rng >> a) & 1)
            if not cols.size:
                continue
            overlaps = iou[:pk][:, cols].copy()
            rec = np.zeros(len(cols), dtype=np.float32)
            for _ in range(min(pk, len(cols))):
                argmax_overlaps = overlaps.argmax(axis=0)   # (numpy, like torch on the host, returns the first maximal index)
                max_overlaps = overlaps[argmax_overlaps, np.arange(len(cols))]
                gt_ind = int(max_overlaps.argmax())
                box_ind = int(argmax_overlaps[gt_ind])
                rec[gt_ind] = overlaps[box_ind, gt_ind]
                overlaps[box_ind, :] = -1
                overlaps[:, gt_ind] = -1
            cover[li, a, cols] = rec
    return cover


def proposal_recall_stats(values):
    """The tail of ``_evaluate_box_proposals`` (coco_evaluation.py:572-592), its own expressions, on one (limit, range)'s cover
    values of all images (-1 = not counted) -> {"ar", "recalls", "thresholds", "gt_overlaps", "num_pos"}"""
    values = np.asarray(values, dtype=np.float32).reshape(-1)
    counted = values >= 0
    num_pos = int(counted.sum())
    gt_overlaps, _ = torch.sort(torch.from_numpy(np.ascontiguousarray(values[counted])))
    thresholds = torch.arange(0.5, 0.95 + 1e-5, 0.05, dtype=torch.float32)
    recalls = torch.zeros_like(thresholds)
    for i, t in enumerate(thresholds):
        recalls[i] = (gt_overlaps >= t).float().sum() / float(num_pos)      # (num_pos == 0: 0 / 0, a NaN, as in the reference)
    return {"ar": recalls.mean(), "recalls": recalls, "thresholds": thresholds, "gt_overlaps": gt_overlaps, "num_pos": num_pos}


class ProposalRecallEvaluator:
    """Proposal recall, the ``box_proposals`` task of the reference's COCO evaluator (``COCOEvaluator._eval_box_proposals`` over
    ``_evaluate_box_proposals``, coco_evaluation.py:253-290,484-592), with the ``reset / process / evaluate`` protocol and rank-0
    gather of the other evaluators.  ``process`` reads ``output["proposals"]`` (``proposal_boxes``, ``objectness_logits``) -- what
    ``ProposalNetwork`` returns, and ``GeneralizedRCNN`` with ``TEST.PROPOSAL_RECALL`` -- and ``evaluate`` returns
    ``{"box_proposals": {"AR@100", "ARs@100", "ARm@100", "ARl@100", "AR@1000", ...}}`` in percent: per image the proposals are ranked
    by objectness and cut at the limit, then the best-covered unused ground-truth box is retired with its proposal until either runs
    out; recall = the share of counted boxes covered at IoU >= t, averaged over t = .50:.05:.95.  NaN where no box is counted.
    An image without any proposal does not count its boxes (the reference skips it before ``num_pos``), ``iscrowd`` boxes are left
    out, the area ranges judge the stored ``area`` (else the box area) after a pass through float32, inclusive at both ends.

    ``device``: a GPU device moves the walk there.  The ground truth is uploaded once; ``process`` copies nothing to the host and
    does not synchronise -- one ``hip.proposal_cover`` launch per call; ``evaluate`` reads the cover records back in ONE copy and
    gathers only those to rank 0.  Same dictionary as without ``device``, value for value.  An image beyond the kernel's caps
    (hip.PROPOSAL_COVER_MAX_PROPOSALS / PROPOSAL_COVER_MAX_GT) is walked by ``proposal_cover_host``, never truncated."""

    def __init__(self, dataset_dicts, device=None, limits=PROPOSAL_LIMITS):
        self.limits = tuple(limits)
        self.num_ranges = len(PROPOSAL_REPORTED)
        assert [n for n, _ in PROPOSAL_REPORTED] == list(PROPOSAL_AREA_NAMES[: self.num_ranges])
        self.device = matching_device(device)
        self._gt = proposal_ground_truth(dataset_dicts)
        self._index = {k: i for i, k in enumerate(self._gt)}          # image id -> data-set index
        self._gt_list = list(self._gt.values())
        if self.device is not None:
            from . import hip
            self._gt_dev = hip.ProposalGroundTruth.from_host(self._gt_list, self.limits, self.num_ranges, self.device)
        self.reset()

    def reset(self):
        self._cover = {}                 # data-set index -> cover [L, A, g] of the image
        self._batches = []               # device path: one entry per process() call, everything still on the device

    def _process_device(self, inputs, outputs):
        from . import hip
        from ._lib import to_device_async
        idx, boxes, logits = [], [], []
        for inp, out in zip(inputs, outputs):
            i = self._index.get(str(inp["image_id"]))
            if i is None:                # not an image of this data set
                continue
            prop = out["proposals"]
            idx.append(i)
            boxes.append(prop.proposal_boxes.tensor.detach().float().reshape(-1, 4).to(self.device, non_blocking=True))
            logits.append(prop.objectness_logits.detach().float().reshape(-1).to(self.device, non_blocking=True))
        if not idx:
            return
        lens = [len(s) for s in logits]
        gcounts = [len(self._gt_list[i][1]) for i in idx]
        n = len(idx)
        meta = to_device_async(torch.tensor(np.concatenate([[0], np.cumsum(lens), idx, [0], np.cumsum(gcounts)]).astype(np.int64)), self.device)
        b, s = torch.cat(boxes).contiguous(), torch.cat(logits).contiguous()
        cover, over = hip.proposal_cover(b, s, meta[: n + 1], meta[n + 1: 2 * n + 1], meta[2 * n + 1:], sum(gcounts), self._gt_dev)
        self._batches.append({"idx": idx, "lens": lens, "gcounts": gcounts, "boxes": b, "logits": s, "cover": cover, "over": over})

    def _device_records(self):
        """the ONE readback -> {data-set index: cover [L, A, g]}; an image processed twice: the later call replaces the earlier"""
        rec = {}
        if not self._batches:
            return rec
        host = torch.cat([e["cover"].reshape(-1) for e in self._batches] + [e["over"].view(torch.float32) for e in self._batches]).cpu().numpy()
        L, A = len(self.limits), self.num_ranges
        sizes = [L * A * sum(e["gcounts"]) for e in self._batches]
        over = np.ascontiguousarray(host[sum(sizes):]).view(np.int32)
        pos, j0 = 0, 0
        for e, size in zip(self._batches, sizes):
            cover = host[pos: pos + size].reshape(L, A, -1)
            pos += size
            nb = len(e["idx"])
            starts = np.concatenate([[0], np.cumsum(e["gcounts"])])
            pstarts = np.concatenate([[0], np.cumsum(e["lens"])])
            bx = lg = None
            for j, i in enumerate(e["idx"]):
                if over[j0 + j]:                                     # beyond a cap of the kernel: the host walk, on the same values
                    if bx is None:
                        bx, lg = e["boxes"].cpu().numpy(), e["logits"].cpu().numpy()
                    gb, gr = self._gt_list[i]
                    rec[i] = proposal_cover_host(bx[pstarts[j]: pstarts[j + 1]], lg[pstarts[j]: pstarts[j + 1]], gb, gr, self.limits, A)
                else:
                    rec[i] = cover[:, :, starts[j]: starts[j + 1]].copy()
            j0 += nb
        return rec

    def process(self, inputs, outputs):
        if self.device is not None:
            return self._process_device(inputs, outputs)
        for inp, out in zip(inputs, outputs):
            i = self._index.get(str(inp["image_id"]))
            if i is None:
                continue
            prop = out["proposals"]
            gb, gr = self._gt_list[i]
            self._cover[i] = proposal_cover_host(prop.proposal_boxes.tensor.detach().float().cpu().numpy(),
                                                 prop.objectness_logits.detach().float().cpu().numpy(), gb, gr, self.limits, self.num_ranges)

    def _gathered(self):
        return merge_by_key(gather_to_rank0(self._device_records() if self.device is not None else self._cover))

    def stats(self, rec):
        """{(limit index, range index): ``proposal_recall_stats``} over the images of ``rec`` in data-set order"""
        out = {}
        for li in range(len(self.limits)):
            for a in range(self.num_ranges):
                vals = [rec[i][li, a] for i in sorted(rec)]
                out[li, a] = proposal_recall_stats(np.concatenate(vals) if vals else np.zeros(0, dtype=np.float32))
        return out

    def evaluate(self):
        rec = self._gathered()
        if rec is None:
            return None
        st = self.stats(rec)
        res = OrderedDict()
        for li, limit in enumerate(self.limits):
            for a, (_, suffix) in enumerate(PROPOSAL_REPORTED):
                key = "AR{}@{}".format(suffix, "all" if limit is None else "{:d}".format(limit))
                res[key] = float(st[li, a]["ar"].item() * 100)          # coco_evaluation.py:287-288
        return {"box_proposals": res}


class DatasetEvaluators:
    """evaluation/evaluator.py:67-100: several evaluators behind one ``reset / process / evaluate``; ``evaluate`` merges their
    dictionaries (on the rank that has them) and refuses a task two of them report"""

    def __init__(self, evaluators):
        self._evaluators = list(evaluators)

    def reset(self):
        for e in self._evaluators:
            e.reset()

    def process(self, inputs, outputs):
        for e in self._evaluators:
            e.process(inputs, outputs)

    def evaluate(self):
        results, any_result = OrderedDict(), False
        for e in self._evaluators:
            res = e.evaluate()               # (every evaluator gathers, so every rank calls every one)
            if res is None:
                continue
            any_result = True
            for k, v in res.items():
                if k in results:
                    raise ValueError(f"Different evaluators produce results with the same key {k}")
                results[k] = v
        return results if any_result else None


def proposal_recall_enabled(cfg):
    return bool(cfg.TEST.get("PROPOSAL_RECALL", False))


def is_proposal_network(model):
    """a model whose outputs hold ``"proposals"`` only (``ProposalNetwork.proposals_only``)"""
    return bool(getattr(getattr(model, "module", model), "proposals_only", False))


def with_proposal_recall(evaluator, model, cfg, dicts):
    """the evaluator of one test set's plain pass: ``evaluator`` itself, paired with a ``ProposalRecallEvaluator`` under
    ``TEST.PROPOSAL_RECALL``, replaced by one for a ``ProposalNetwork`` (its outputs hold proposals only)"""
    if is_proposal_network(model):
        return ProposalRecallEvaluator(dicts, device=cfg.MODEL.DEVICE)
    if proposal_recall_enabled(cfg):
        return DatasetEvaluators([evaluator, ProposalRecallEvaluator(dicts, device=cfg.MODEL.DEVICE)])
    return evaluator


def _print_results(prefix, res):
    """one line per task of a result dict: the box AP line as it always was, then the others"""
    for task, metrics in res.items():
        print(prefix + str({k: round(v, 4) for k, v in metrics.items()} if task == "bbox" else {task: {k: round(v, 4) for k, v in metrics.items()}}),
              flush=True)


_VOC_EVALUATORS = {}            # (name, datasets root, device) -> PascalVOCDetectionEvaluator of run_eval_only_catalog


def run_eval_only_catalog(model, cfg, datasets_root, rank=0, world=1, return_results=False, prefix="", weight_average=None):
    """``--eval-only --datasets-root DIR``: every ``cfg.DATASETS.TEST`` name the catalog knows -- the Cityscapes splits of
    cddmsl_amd/cityscapes.py and the COCO-json sets of cddmsl_amd/coco_json.py (``bdd_100k_val``) -> COCO-style box AP; the VOC
    family of cddmsl_amd/voc_catalog.py (``voc_2007_test``, ``Clipart1k_test`` ...) -> Pascal VOC AP with the set's year's metric.
    One printed line per set from rank 0 (each starting with ``prefix``); a name the catalog does not know, or a set whose json /
    image-set file is not there, is skipped with one printed line.  The matching runs on ``cfg.MODEL.DEVICE`` (the evaluators' ``device``).
    Returns the exit code (or {name: result dict} on rank 0 with ``return_results``).  ``weight_average`` (MODEL_EMA): see
    ``averaged_passes``; the averaged weights' lines follow the plain ones."""
    results = OrderedDict()
    for averaged, weights in averaged_passes(model, cfg, weight_average):
        with weights:
            part = _eval_only_catalog_pass(model, cfg, datasets_root, rank, world, prefix, averaged)
        for name, res in part.items():
            results.setdefault(name, res).update(res)
    return results if return_results else 0


def _eval_only_catalog_pass(model, cfg, datasets_root, rank, world, prefix, averaged):
    """one pass of ``run_eval_only_catalog`` over the weights the model holds now -> {name: result dict} (rank 0; else empty);
    ``averaged``: the task keys carry ``_EMA``"""
    mark = with_ema_suffix if averaged else (lambda r: r)
    import torch.distributed as dist
    from . import cityscapes, coco_json, voc_catalog
    from .data import build_detection_test_loader
    ws = dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1
    assert world == ws, f"run_eval_only_catalog: world={world} but the process group has {ws} ranks"
    results = OrderedDict()
    for name in cfg.DATASETS.TEST:
        voc = None
        if cityscapes.is_cityscapes(name):
            dicts, classes = cityscapes.load_cityscapes(name, datasets_root, device=cfg.MODEL.DEVICE), cityscapes.THING_CLASSES
        elif voc_catalog.is_voc_family(name):
            set_file = voc_catalog.image_set_file(name, datasets_root)
            if not os.path.exists(set_file):
                if rank == 0:
                    print(f"{prefix}skipping {name}: {set_file} not found")
                continue
            if num_test_classes(model, cfg) != len(VOC_CLASS_NAMES):
                raise ValueError(f"{name}: a VOC-family set has {len(VOC_CLASS_NAMES)} classes but the model's detections have {num_test_classes(model, cfg)}")
            dicts, classes = voc_catalog.load_voc_family(name, datasets_root), VOC_CLASS_NAMES
            key = (name, os.path.abspath(datasets_root), str(cfg.MODEL.DEVICE))
            if key not in _VOC_EVALUATORS:          # kept like the catalog's dicts: a periodic evaluation parses and uploads the ground truth once
                dirname, split, year, _ = voc_catalog.voc_entry(name, datasets_root)
                _VOC_EVALUATORS[key] = PascalVOCDetectionEvaluator(dirname, split, year, VOC_CLASS_NAMES, device=cfg.MODEL.DEVICE)
            voc = _VOC_EVALUATORS[key]
        elif coco_json.is_coco_json(name):
            json_file = coco_json.coco_json_paths(name, datasets_root)[0]
            if not os.path.exists(json_file):
                if rank == 0:
                    print(f"{prefix}skipping {name}: {json_file} not found")
                continue
            dicts, classes = coco_json.load_coco_json_split(name, datasets_root)
            if len(classes) != num_test_classes(model, cfg):
                raise ValueError(f"{name}: {json_file} has {len(classes)} classes but the model's detections have {num_test_classes(model, cfg)}")
        else:
            if rank == 0:
                print(f"{prefix}skipping {name}: not in the dataset catalog")
            continue
        loader = build_detection_test_loader(cfg, dicts, batch_size=1, rank=rank, world=world, device=cfg.MODEL.DEVICE)
        new_evaluator = (lambda: voc) if voc is not None else (lambda: COCODetectionEvaluator(dicts, classes, device=cfg.MODEL.DEVICE))
        res = mark(inference_on_dataset(model, loader, with_proposal_recall(new_evaluator(), model, cfg, dicts)))
        if rank == 0:
            _print_results(f"{prefix}{name}: ", res)
            results[name] = res
        if tta_enabled(cfg) and not is_proposal_network(model):
            loader = build_detection_test_loader(cfg, dicts, batch_size=1, rank=rank, world=world, device=cfg.MODEL.DEVICE)
            tta = mark(with_tta_suffix(inference_on_dataset(tta_model(cfg, model), loader, new_evaluator())))
            if rank == 0:
                print(f"{prefix}{name}: " + str({k: {m: round(v, 4) for m, v in r.items()} for k, r in tta.items()}), flush=True)
                results[name].update(tta)
    return results


def flatten_results(results):
    """{dataset: {"bbox": {"AP": v}}} -> {"dataset/bbox/AP": v}: the keys the reference's EvalHook puts into the storage"""
    flat = OrderedDict()
    for name, res in (results or {}).items():
        for task, metrics in res.items():
            for m, v in metrics.items():
                flat[f"{name}/{task}/{m}"] = float(v)
    return flat


class PeriodicEval:
    """engine/hooks.py ``EvalHook``: ``after_step(it)`` evaluates on every rank when ``(it + 1) % period == 0`` and ``after_train()``
    once after the last iteration unless that iteration was just evaluated.  ``eval_fn(prefix)`` runs the sharded evaluation and
    returns {dataset: results} on rank 0 (``run_eval_only_catalog`` / ``run_eval_only`` with ``return_results``); the flattened
    values go to ``trainer.storage``.  An evaluation leaves training as it found it: ``model.training``, the model's three sampler
    generators and torch's CPU / GPU generators are restored, the training loader is not touched, and the model's cache of the
    shared source pass is dropped instead of being carried across."""

    def __init__(self, trainer, period, eval_fn, max_iter, rank=0):
        self.trainer, self.period, self.eval_fn, self.max_iter, self.rank = trainer, int(period), eval_fn, int(max_iter), rank
        self.evaluated_at = []

    def _generators(self):
        m = self.trainer.model
        gens = [g for g in (getattr(getattr(m, "proposal_generator", None), "sample_generator", None),
                            getattr(getattr(m, "roi_heads", None), "sample_generator", None), getattr(m, "region_generator", None)) if g is not None]
        return list({id(g): g for g in gens}.values())

    def _do_eval(self, it):
        m = self.trainer.model
        was_training = m.training
        gens = self._generators()
        states = [g.get_state() for g in gens]
        cpu_state = torch.get_rng_state()
        cuda_state = torch.cuda.get_rng_state() if torch.cuda.is_available() else None
        if hasattr(m, "_shared"):
            m._shared = None
        try:
            results = self.eval_fn(f"iter {it}  ")
        finally:
            m.train(was_training)
            if hasattr(m, "_shared"):
                m._shared = None
            for g, s in zip(gens, states):
                g.set_state(s)
            torch.set_rng_state(cpu_state)
            if cuda_state is not None:
                torch.cuda.set_rng_state(cuda_state)
        self.evaluated_at.append(it)
        if self.rank == 0 and isinstance(results, dict):
            for k, v in flatten_results(results).items():
                self.trainer.storage[k] = v
        return results

    def after_step(self, it):
        if self.period > 0 and (it + 1) % self.period == 0:
            return self._do_eval(it)

    def after_train(self):
        last = self.max_iter - 1
        if self.period > 0 and last >= 0 and (not self.evaluated_at or self.evaluated_at[-1] != last):
            return self._do_eval(last)
