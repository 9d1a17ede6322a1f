"""Generates tests/golden/ref_augment.npz by running the REFERENCE's own training augmentations (read from where the reference lies,
never copied; runs only in the build container) -- the INPUT.CROP / MIN_SIZE_TRAIN_SAMPLING "range" / RANDOM_FLIP "vertical" options
of ``DatasetMapper.from_config`` (data/dataset_mapper.py:94-97) and ``build_augmentation`` (data/detection_utils.py:590-614):

  * ``RandomCrop.get_crop_size / get_transform`` (data/transforms/augmentation_impl.py:367-399), all four crop types,
  * ``ResizeShortestEdge.get_transform`` (:179-199) with sample_style "choice" and "range",
  * ``RandomFlip.get_transform`` (:117-126) horizontal and vertical,
  * ``transform_instance_annotations`` / ``annotations_to_instances`` / ``filter_empty_instances`` (data/detection_utils.py),
  applied the way ``DatasetMapper.__call__`` applies them (dataset_mapper.py:154-216): the augmentations draw one after the other from
  ``np.random``, each on the image the one before it made, and ONE transform list goes over the image, its twin and the boxes.

Stand-ins with the published behaviour for two more fvcore classes, next to the ones of make_golden_data.py (parity unpinned for THOSE
lines only): ``CropTransform`` (image[y0:y0 + h, x0:x0 + w]; coords - (x0, y0)) and ``VFlipTransform`` (image[::-1]; y -> height - y).

usage:  python tests/golden/make_golden_augment.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_data as mgd  # noqa: E402


# ---------------------------------------------------------------- fvcore.transforms.transform stand-ins (published behaviour; parity unpinned)
class CropTransform(mgd.Transform):
    def __init__(self, x0, y0, w, h, orig_w=None, orig_h=None):
        super().__init__()
        self._set_attributes(locals())

    def apply_image(self, img):                                                   # parity unpinned
        return img[self.y0:self.y0 + self.h, self.x0:self.x0 + self.w]

    def apply_coords(self, coords):                                               # parity unpinned
        coords[:, 0] -= self.x0
        coords[:, 1] -= self.y0
        return coords


class VFlipTransform(mgd.Transform):
    def __init__(self, height):
        super().__init__()
        self._set_attributes(locals())

    def apply_image(self, img):                                                   # parity unpinned
        return np.flip(img, axis=0)

    def apply_coords(self, coords):                                               # parity unpinned
        coords[:, 1] = self.height - coords[:, 1]
        return coords


# (a): (image h, w), crop type, crop size, short edges, sampling, max size, flip, the flip decision the chosen seed must give
SAMPLES = [((72, 96), "relative", (0.6, 0.7), (48, 64, 80), "choice", 100, "horizontal", True),
           ((96, 70), "relative_range", (0.5, 0.5), (56, 88), "range", 120, "vertical", True),
           ((80, 100), "absolute", (50, 64), (64, 72), "choice", 90, "vertical", True),
           ((90, 84), "absolute_range", (40, 70), (40, 72), "range", 1000, "horizontal", False)]

# (b): crop (type, size) or None, short edges, sampling, flip
SEQUENCES = [(("relative_range", (0.9, 0.9)), tuple(range(480, 801, 32)), "choice", "horizontal"),
             (("absolute_range", (200, 300)), (480, 800), "range", "vertical"),
             (None, (480, 800), "range", "none")]


def augmentations(ai, crop, sizes, style, max_size, flip):
    """the list ``DatasetMapper.from_config`` builds"""
    augs = [ai.ResizeShortestEdge(sizes, max_size, style)]
    if flip != "none":
        augs.append(ai.RandomFlip(horizontal=flip == "horizontal", vertical=flip == "vertical"))
    if crop is not None:
        augs.insert(0, ai.RandomCrop(*crop))
    return augs


def sample_transforms(augs, img):
    """``AugmentationList.__call__``: every augmentation draws on the image the ones before it made"""
    tfms = []
    for a in augs:
        t = a.get_transform(img)
        img = t.apply_image(img)
        tfms.append(t)
    return tfms, img


def one_sample(ai, du, S, n, seed):
    (h, w), ctype, csize, sizes, style, max_size, flip, want_flip = SAMPLES[n]
    g = np.random.RandomState(40 + n)
    img = g.randint(0, 256, (h, w, 3), dtype=np.uint8)
    twin = (255 - img).astype(np.uint8)
    boxes = np.stack([g.uniform(-3, w * 0.7, 6), g.uniform(-3, h * 0.7, 6), np.zeros(6), np.zeros(6)], axis=1)
    boxes[:, 2] = boxes[:, 0] + g.uniform(4, w * 0.5, 6)
    boxes[:, 3] = boxes[:, 1] + g.uniform(4, h * 0.5, 6)
    boxes[4] = [1.0, 1.0, 7.0, 6.0]                                # small ones in two opposite corners: a window smaller than the
    boxes[5] = [w - 8.0, h - 7.0, w - 1.0, h - 1.0]                # image misses at least one of them
    classes = g.randint(0, 20, 6)
    np.random.seed(seed)
    tfms, final = sample_transforms(augmentations(ai, (ctype, csize), sizes, style, max_size, flip), img)
    crop_t, resize_t = tfms[0], tfms[1]
    flipped = isinstance(tfms[2], (mgd.HFlipTransform, VFlipTransform))
    y0, x0, ch, cw = crop_t.y0, crop_t.x0, crop_t.h, crop_t.w
    inside = (boxes[:, 0] >= x0) & (boxes[:, 1] >= y0) & (boxes[:, 2] <= x0 + cw) & (boxes[:, 3] <= y0 + ch)
    outside = (boxes[:, 2] <= x0) | (boxes[:, 3] <= y0) | (boxes[:, 0] >= x0 + cw) | (boxes[:, 1] >= y0 + ch)
    ok = inside.any() and outside.any() and (~inside & ~outside).any() and flipped == want_flip and ch < h and cw < w
    if not ok:
        return None
    tl = mgd.TransformList(tfms)
    image_size = final.shape[:2]
    annos = [{"bbox": b.tolist(), "bbox_mode": S.BoxMode.XYXY_ABS, "category_id": int(c)} for b, c in zip(boxes, classes)]
    annos_t = [du.transform_instance_annotations(dict(a), tl, image_size) for a in annos]
    inst = du.filter_empty_instances(du.annotations_to_instances(annos_t, image_size))
    # the three conditions of the fixture (conditions, not measurements): a box survives whole, a box is cut, a box is outside and filtered
    assert inside.any() and (~inside & ~outside).any() and outside.any() and len(inst) == int((~outside).sum()), (n, seed)
    assert np.array_equal(inst.gt_classes.numpy(), classes[~outside])
    assert image_size == (resize_t.new_h, resize_t.new_w) and flipped == want_flip
    return {"seed": np.array(seed), "img": img, "boxes_in": boxes, "classes_in": classes, "window": np.array([y0, x0, ch, cw]),
            "outside": outside, "final": np.ascontiguousarray(final), "twin_final": np.ascontiguousarray(tl.apply_image(twin)),
            "boxes_out": inst.gt_boxes.tensor.numpy(), "classes_out": inst.gt_classes.numpy(), "flipped": np.array(int(flipped)),
            "crop_type": np.array(ctype), "crop_size": np.array(csize, dtype=np.float64), "min_sizes": np.array(sizes), "sampling": np.array(style),
            "max_size": np.array(max_size), "flip": np.array(flip)}


def main():
    tr, ai, du, S = mgd.setup_data()
    ai.CropTransform, ai.VFlipTransform = CropTransform, VFlipTransform        # (augmentation_impl imported the stub module's names)
    out = {}
    for n in range(len(SAMPLES)):
        for seed in range(1000):                                               # the first seed under which the conditions hold
            r = one_sample(ai, du, S, n, seed)
            if r is not None:
                break
        assert r is not None, n
        out.update({f"{k}{n}": v for k, v in r.items()})
    assert sum(str(out[f"flip{n}"]) == "vertical" and int(out[f"flipped{n}"]) for n in range(len(SAMPLES))) >= 2
    # (b) the draw ORDER: crop (rand(2) or two randint, then the two offsets), the short edge, the flip -- 16 consecutive samples per setting
    im = np.zeros((375, 500, 3), np.uint8)
    for n, (crop, sizes, style, flip) in enumerate(SEQUENCES):
        np.random.seed(700 + n)
        augs = augmentations(ai, crop, sizes, style, 1333, flip)
        seq = []
        for _ in range(16):
            tfms, final = sample_transforms(augs, im)
            y0, x0, ch, cw = (tfms[0].y0, tfms[0].x0, tfms[0].h, tfms[0].w) if crop is not None else (0, 0, 375, 500)
            seq.append((y0, x0, ch, cw, final.shape[0], final.shape[1], int(isinstance(tfms[-1], (mgd.HFlipTransform, VFlipTransform)))))
        out[f"sequence{n}"], out[f"sequence_seed{n}"] = np.array(seq), np.array(700 + n)
    # (c) RandomFlip's draw with vertical=True
    np.random.seed(123)
    rf = ai.RandomFlip(prob=0.5, horizontal=False, vertical=True)
    dummy = np.zeros((4, 6, 3), np.uint8)
    out["vflip_draws"] = np.array([isinstance(rf.get_transform(dummy), VFlipTransform) for _ in range(32)])
    np.savez_compressed(os.path.join(HERE, "ref_augment.npz"), **out)
    print("augment ok", [(int(out[f"seed{n}"]), out[f"window{n}"].tolist(), out[f"final{n}"].shape, int(out[f"flipped{n}"])) for n in range(len(SAMPLES))],
          [out[f"sequence{n}"][:2].tolist() for n in range(len(SEQUENCES))], out["vflip_draws"].astype(int).tolist())


if __name__ == "__main__":
    main()
