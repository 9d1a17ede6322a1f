"""The class count ``GeneralizedRCNNWithTTA`` merges its views' detections over.

The wrapper (test_time_augmentation.py:171-173) sizes the one-hot score matrix of ``merge_detections`` with
``cfg.MODEL.ROI_HEADS.NUM_CLASSES``.  With open-vocabulary inference (roi_heads.FastRCNNOutputLayers.test_cls_score) the detections
carry classes of the TEST vocabulary, which may be larger: indexed into a matrix of NUM_CLASSES + 1 columns they would land on wrong
cells and past the end of the tensor.  This module gives the wrapper class the method it needs -- the count comes from the wrapped
model's ``roi_heads.box_predictor.num_test_classes`` and falls back to the config value for a model without such a head -- so every
way of constructing the wrapper, not only ``evaluation.tta_model``, merges over the right vocabulary.  It is installed when the
``modeling`` package is imported, which any import of the wrapper goes through."""
from . import test_time_augmentation as _tta


def merge_num_classes(model, cfg):
    """classes of the detections ``model`` returns: the box head's test vocabulary, else ``MODEL.ROI_HEADS.NUM_CLASSES``"""
    head = getattr(getattr(getattr(model, "module", model), "roi_heads", None), "box_predictor", None)
    return getattr(head, "num_test_classes", cfg.MODEL.ROI_HEADS.NUM_CLASSES)


def _merge_detections(self, all_boxes, all_scores, all_classes, shape_hw):
    return _tta.merge_detections(all_boxes, all_scores, all_classes, shape_hw, merge_num_classes(self.model, self.cfg),
                                 self.cfg.MODEL.ROI_HEADS.NMS_THRESH_TEST, self.cfg.TEST.DETECTIONS_PER_IMAGE)


_tta.GeneralizedRCNNWithTTA._merge_detections = _merge_detections
