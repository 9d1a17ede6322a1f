"""Generates tests/golden/ref_color_jitter.npz by running the REFERENCE's own photometric augmentations (read from where the reference
lies, never copied; runs only in the build container): ``RandomBrightness``, ``RandomContrast``, ``RandomSaturation``, ``RandomLighting``
(data/transforms/augmentation_impl.py:493-600) in an ``AugmentationList`` (augmentation.py:241-272: each draws on the image the ones
before it made), behind ``RandomApply`` (:63-94) where PROB < 1, under ``np.random.seed(s)`` on a few small seeded RGB images.

What is recorded is what the reference hands to fvcore's ``BlendTransform``: ``src_weight``, ``dst_weight`` and ``src_image`` of every
transform, in order.  ``BlendTransform`` itself is a recording stand-in with the published behaviour (``src_weight * src_image +
dst_weight * img`` on the float32 image, clipped to [0, 255], back to uint8), next to the ones of make_golden_data.py: fvcore is not
vendored, so parity of the PIXELS is unpinned; the draws and the blend parameters are the reference's.

usage:  python tests/golden/make_golden_color_jitter.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_data as mgd  # noqa: E402


class BlendTransform(mgd.Transform):
    log = []

    def __init__(self, src_image, src_weight, dst_weight):
        super().__init__()
        self._set_attributes(locals())
        BlendTransform.log.append(self)

    def apply_image(self, img, interp=None):                                      # parity unpinned
        if img.dtype == np.uint8:
            img = img.astype(np.float32)
            img = self.src_weight * self.src_image + self.dst_weight * img
            return np.clip(img, 0, 255).astype(np.uint8)
        return self.src_weight * self.src_image + self.dst_weight * img

    def apply_coords(self, coords):
        return coords


# name -> (PROB, BRIGHTNESS, CONTRAST, SATURATION, LIGHTING); a range of (1, 1) / a scale of 0 leaves the class out, as the mapper does
CASES = {"all": (1.0, (0.6, 1.4), (0.5, 1.5), (0.4, 1.6), 40.0),
         "contrast": (1.0, (1.0, 1.0), (0.5, 1.5), (1.0, 1.0), 0.0),
         "prob": (0.5, (0.6, 1.4), (0.5, 1.5), (0.4, 1.6), 40.0)}
SHAPES = [(5, 7), (12, 9), (16, 16)]
NAMES = {"RandomBrightness": 0, "RandomContrast": 1, "RandomSaturation": 2, "RandomLighting": 3}


def augmentation(ai, aug_mod, prob, brightness, contrast, saturation, lighting):
    augs = []
    for cls, r in ((ai.RandomBrightness, brightness), (ai.RandomContrast, contrast), (ai.RandomSaturation, saturation)):
        if tuple(r) != (1.0, 1.0):
            augs.append(cls(*r))
    if lighting != 0.0:
        augs.append(ai.RandomLighting(lighting))
    aug = aug_mod.AugmentationList(augs)
    return ai.RandomApply(aug, prob) if prob < 1.0 else aug, [NAMES[type(a).__name__] for a in augs]


def main():
    import importlib
    tr, ai, du, S = mgd.setup_data()
    ai.BlendTransform = BlendTransform                     # (augmentation_impl imported the stub module's name)
    aug_mod = importlib.import_module("detectron2.data.transforms.augmentation")
    out = {"case_names": np.array(list(CASES))}
    for n, (h, w) in enumerate(SHAPES):
        out[f"img{n}"] = np.random.RandomState(90 + n).randint(0, 256, (h, w, 3), dtype=np.uint8)
    for name, spec in CASES.items():
        out[f"{name}/spec"] = np.array([spec[0], *spec[1], *spec[2], *spec[3], spec[4]], dtype=np.float64)
        seeds, outcomes = [], set()
        for seed in range(100):
            runs = []
            for n in range(len(SHAPES)):
                aug, ops = augmentation(ai, aug_mod, *spec)
                np.random.seed(seed)
                BlendTransform.log = []
                aug(aug_mod.AugInput(out[f"img{n}"].copy()))
                runs.append((ops if BlendTransform.log else [], list(BlendTransform.log)))
            applied = bool(runs[0][1])
            assert all(bool(r[1]) == applied for r in runs)            # (the first draw does not depend on the image)
            if spec[0] < 1.0 and applied in outcomes and len(outcomes) < 2:
                continue                                               # PROB 0.5: keep looking for the other outcome
            outcomes.add(applied)
            seeds.append(seed)
            for n, (ops, log) in enumerate(runs):
                key = f"{name}/{seed}/{n}"
                out[key + "/ops"] = np.array(ops, dtype=np.int64)
                for i, t in enumerate(log):
                    out[f"{key}/{i}/src_weight"] = np.float64(t.src_weight)
                    out[f"{key}/{i}/dst_weight"] = np.float64(t.dst_weight)
                    out[f"{key}/{i}/src_image"] = np.asarray(t.src_image, dtype=np.float64)
            if len(seeds) >= 4 and (spec[0] >= 1.0 or len(outcomes) == 2):
                break
        assert spec[0] >= 1.0 or outcomes == {True, False}, name
        out[f"{name}/seeds"] = np.array(seeds)
    np.savez_compressed(os.path.join(HERE, "ref_color_jitter.npz"), **out)
    print("color jitter ok", {name: out[f"{name}/seeds"].tolist() for name in CASES}, os.path.getsize(os.path.join(HERE, "ref_color_jitter.npz")), "bytes")


if __name__ == "__main__":
    main()
