"""Test-time augmentation for GeneralizedRCNN (detectron2/modeling/test_time_augmentation.py): multi-scale + flip views of one
image, one forward pass per batch of views, the detections mapped back to the original image and merged by per-class NMS.

Two ways to the views:
  * default (``tta_mapper=None``): ``hip.tta_views`` makes them on the device from the uint8 image the model is handed -- the PIL
    bilinear resize bit for bit, mirror, normalise, pad, straight into the NHWC batches ``GeneralizedRCNN._inference_preprocessed``
    takes.  The host never sees a view;
  * ``tta_mapper=DatasetMapperTTA(cfg)`` (or any callable with its contract): the reference's host path -- PIL on the host, then
    ``model.inference(group, do_postprocess=False)``.
Both produce the same pixels (tests/test_gpu_tta.py), so the same detections.

A view's ``transforms`` record is the tuple ``(orig_h, orig_w, in_h, in_w, newh, neww, flipped)``: the dataset image's size, the size
of the image the model was handed (the test loader's resize: the reference's ``pre_tfm``), the view's size, mirrored or not.

The merge is upstream Detectron2's: ``fast_rcnn_inference_single_image(all_boxes, one-hot scores, orig shape, 1e-8, NMS_THRESH_TEST,
DETECTIONS_PER_IMAGE)``, per-class HARD NMS, also when the model's own passes use soft-NMS.  (The reference's call at :271-278 passes
these six arguments to its eleven-parameter soft-NMS variant of that function and cannot run as shipped.)"""
import copy
from typing import Dict, List

import numpy as np
import torch
from torch import nn
from torch.nn.parallel import DistributedDataParallel

from .. import hip
from . import roi_heads as _roi_heads
from .rcnn import GeneralizedRCNN

__all__ = ["DatasetMapperTTA", "GeneralizedRCNNWithTTA"]


def view_sizes(in_h, in_w, min_sizes, max_size):
    """ResizeShortestEdge(min_size, max_size) of every TTA scale -> [(newh, neww)]"""
    from ..data import shortest_edge_size
    return [shortest_edge_size(in_h, in_w, int(s), int(max_size)) for s in min_sizes]


class DatasetMapperTTA:
    """test_time_augmentation.py:29-98 on the host: a dataset dict with ``image`` (u8 CHW), ``height``, ``width`` -> the list of
    ``len(MIN_SIZES) * (2 if FLIP else 1)`` dicts in the order [s0, s0 mirrored, s1, ...], each with its ``image`` (PIL bilinear resize
    of the handed image) and its ``transforms`` record."""

    def __init__(self, cfg):
        a = cfg.TEST.AUG
        self.min_sizes, self.max_size, self.flip = list(a.MIN_SIZES), a.MAX_SIZE, bool(a.FLIP)

    def __call__(self, dataset_dict: Dict) -> List[Dict]:
        from ..data import resize_image
        image = dataset_dict["image"]
        numpy_image = np.ascontiguousarray(image.cpu().permute(1, 2, 0).numpy())
        in_h, in_w = numpy_image.shape[:2]
        orig_h, orig_w = dataset_dict["height"], dataset_dict["width"]
        rest = {k: v for k, v in dataset_dict.items() if k != "image"}
        ret = []
        for newh, neww in view_sizes(in_h, in_w, self.min_sizes, self.max_size):
            resized = resize_image(numpy_image, newh, neww)
            for flipped in ((False, True) if self.flip else (False,)):
                view = resized[:, ::-1] if flipped else resized
                dic = copy.deepcopy(rest)
                dic["transforms"] = (orig_h, orig_w, in_h, in_w, newh, neww, flipped)
                dic["image"] = torch.from_numpy(np.ascontiguousarray(view.transpose(2, 0, 1)))
                ret.append(dic)
        return ret


def _f32(x):
    return float(np.float32(x))


def unmap_boxes(boxes, record):
    """The inverse of a view's transforms on XYXY f32 boxes [R, 4] (TransformList.inverse().apply_box on float32 arrays): mirror
    (``x0' = neww - x1, x1' = neww - x0``), then x * f32(in_w / neww), y * f32(in_h / newh), then -- when the handed image is not the
    dataset image's size -- x * f32(orig_w / in_w), y * f32(orig_h / in_h).  The two ratios are applied one after the other, each
    rounded to f32 first, which is what numpy does with the reference's in-place float32 coordinate arrays."""
    orig_h, orig_w, in_h, in_w, newh, neww, flipped = record
    b = boxes.float()
    x0, y0, x1, y1 = b[:, 0], b[:, 1], b[:, 2], b[:, 3]
    if flipped:
        x0, x1 = _f32(neww) - x1, _f32(neww) - x0
    sx, sy = _f32(in_w * 1.0 / neww), _f32(in_h * 1.0 / newh)
    x0, x1, y0, y1 = x0 * sx, x1 * sx, y0 * sy, y1 * sy
    if (in_h, in_w) != (orig_h, orig_w):
        px, py = _f32(orig_w * 1.0 / in_w), _f32(orig_h * 1.0 / in_h)
        x0, x1, y0, y1 = x0 * px, x1 * px, y0 * py, y1 * py
    return torch.stack([x0, y0, x1, y1], dim=1)


def merge_detections(all_boxes, all_scores, all_classes, shape_hw, num_classes, nms_thresh, topk):
    """:262-280, with upstream's call: one-hot [R, K+1] scores (one indexed assignment), then score threshold 1e-8, per-class hard NMS
    at ``nms_thresh``, the best ``topk`` -> Instances(shape_hw) with pred_boxes, scores, pred_classes"""
    num_boxes = all_boxes.shape[0]
    scores_2d = torch.zeros(num_boxes, num_classes + 1, device=all_boxes.device)
    scores_2d[torch.arange(num_boxes, device=all_boxes.device), all_classes.long()] = all_scores.float()
    merged, _ = _roi_heads.fast_rcnn_inference_single_image(all_boxes, scores_2d, shape_hw, 1e-8, nms_thresh, topk)
    return merged


class GeneralizedRCNNWithTTA(nn.Module):
    """test_time_augmentation.py:101-280.  ``__call__`` has the contract of the model in eval mode: a list of dataset dicts -> a list
    of ``{"instances": Instances}`` in the dataset image's coordinates."""

    def __init__(self, cfg, model, tta_mapper=None, batch_size=3):
        super().__init__()
        if isinstance(model, DistributedDataParallel):
            model = model.module
        assert isinstance(model, GeneralizedRCNN), "TTA is only supported on GeneralizedRCNN. Got a model of type {}".format(type(model))
        self.cfg = cfg.clone()
        assert not self.cfg.MODEL.KEYPOINT_ON, "TTA for keypoint is not supported yet"
        assert not self.cfg.MODEL.MASK_ON, "the mask branch of TTA is not built (MASK_ON is false in every config here)"
        self.model = model
        self.tta_mapper = tta_mapper            # None: the views are made on the device
        self.batch_size = batch_size
        a = self.cfg.TEST.AUG
        self.min_sizes, self.max_size, self.flip = list(a.MIN_SIZES), a.MAX_SIZE, bool(a.FLIP)
        self.training = model.training          # (a wrapper left in nn.Module's default train mode would flip the model on .train(was))

    def _batch_inference(self, batched_inputs):
        """:162-186: ``model.inference`` on groups of ``batch_size`` inputs"""
        outputs = []
        for i in range(0, len(batched_inputs), self.batch_size):
            outputs.extend(self.model.inference(batched_inputs[i:i + self.batch_size], None, do_postprocess=False))
        return outputs

    def forward(self, batched_inputs):
        return [self._inference_one_image(self._maybe_read_image(x)) for x in batched_inputs]

    def _maybe_read_image(self, dataset_dict):
        ret = copy.copy(dataset_dict)
        if "image" not in ret:
            from ..data import read_image
            image = read_image(ret.pop("file_name"), self.model.input_format)
            ret["image"] = torch.from_numpy(np.ascontiguousarray(image.transpose(2, 0, 1)))
        if "height" not in ret and "width" not in ret:
            ret["height"], ret["width"] = int(ret["image"].shape[1]), int(ret["image"].shape[2])
        return ret

    @torch.no_grad()
    def _inference_one_image(self, input):
        orig_shape = (input["height"], input["width"])
        if self.tta_mapper is None:
            outputs, records = self._device_views_inference(input)
        else:
            views = self.tta_mapper(input)
            records = [v.pop("transforms") for v in views]
            outputs = self._batch_inference(views)
        all_boxes, all_scores, all_classes = self._get_augmented_boxes(outputs, records)
        return {"instances": self._merge_detections(all_boxes, all_scores, all_classes, orig_shape)}

    def _device_views_inference(self, input):
        m = self.model
        image = input["image"].to(m.device).contiguous()
        in_h, in_w = int(image.shape[-2]), int(image.shape[-1])
        sizes = view_sizes(in_h, in_w, self.min_sizes, self.max_size)
        groups = hip.tta_views(image, sizes, self.flip, m.pixel_mean_list, m.pixel_std_list, m.compute_dtype, self.batch_size,
                               div255=m.div_pixel)
        outputs = []
        for images, group_sizes in groups:
            outputs.extend(m._inference_preprocessed(images, group_sizes))
        records = [(input["height"], input["width"], in_h, in_w, nh, nw, f) for nh, nw, f in hip.tta_view_list(sizes, self.flip)]
        return outputs, records

    @staticmethod
    def _get_augmented_boxes(outputs, records):
        """:244-260: every view's boxes in the dataset image's coordinates, and the union's scores and classes"""
        boxes = torch.cat([unmap_boxes(o.pred_boxes.tensor, r) for o, r in zip(outputs, records)], dim=0)
        scores = torch.cat([o.scores for o in outputs], dim=0)
        classes = torch.cat([o.pred_classes for o in outputs], dim=0)
        return boxes, scores, classes

    def _merge_detections(self, all_boxes, all_scores, all_classes, shape_hw):
        return merge_detections(all_boxes, all_scores, all_classes, shape_hw, self.cfg.MODEL.ROI_HEADS.NUM_CLASSES,
                                self.cfg.MODEL.ROI_HEADS.NMS_THRESH_TEST, self.cfg.TEST.DETECTIONS_PER_IMAGE)
