"""Photometric augmentation of the training pairs (``INPUT.COLOR_JITTER``): the reference's ``RandomBrightness``, ``RandomContrast``,
``RandomSaturation`` and ``RandomLighting`` (data/transforms/augmentation_impl.py:493-600), in that fixed order, each a
``BlendTransform`` on the final uint8 image the model receives (after crop, resize and flip, in the model's channel order).  They leave
the geometry alone, so an image and its domain twin keep sharing one set of boxes.

  * ``ColorJitter.draw(rng)``: the random draws, in the reference classes' own calls and order;
  * ``color_jitter_u8``: the canonical arithmetic in numpy -- the host path of the mapper and the exact reference of the HIP kernel
    (``cddmsl_color_jitter_batch_u8``, csrc/color_jitter.hip), which follows it bit for bit;
  * ``descriptor``: the kernel's per-image record.

Arithmetic: fvcore's ``BlendTransform`` formula with ALL-float32 operands, every product and sum rounded on its own:
``out = trunc(min(max(fl32(fl32(sw * src) + fl32(dw * fl32(x))), 0), 255))`` with ``dw = fl32(w)``, ``sw = fl32(1 - w)`` (``1 - w`` in
double).  Where fvcore itself evaluates depends on the NumPy version's promotion rules (float64 for the contrast mean and the grey
array under NumPy 2), and fvcore is not installed here: bit parity with fvcore's pixels is not claimed; the draws and the blend
parameters are pinned to the reference (tests/golden/make_golden_color_jitter.py).
"""
import numpy as np

BRIGHTNESS, CONTRAST, SATURATION, LIGHTING = 1, 2, 4, 8            # the kernel's operation bits, in application order
BLENDS = (("brightness", BRIGHTNESS), ("contrast", CONTRAST), ("saturation", SATURATION))
# RandomLighting's fixed PCA over ImageNet (augmentation_impl.py:590-593), RGB
EIGEN_VECS = np.array([[-0.5675, 0.7192, 0.4009], [-0.5808, -0.0045, -0.8140], [-0.5836, -0.6948, 0.4203]])
EIGEN_VALS = np.array([0.2175, 0.0188, 0.0045])

_F = np.float32
_GREY = (_F(0.299), _F(0.587), _F(0.114))


class ColorJitter:
    """The draws of one enabled ``INPUT.COLOR_JITTER`` block (``config.check_color_jitter`` has judged it)."""

    def __init__(self, block):
        self.prob, self.twin, self.lighting = float(block.PROB), block.TWIN, float(block.LIGHTING)
        self.ranges = {name: tuple(float(v) for v in block[name.upper()]) for name, _ in BLENDS}
        self.blends = [name for name, _ in BLENDS if self.ranges[name] != (1.0, 1.0)]

    @property
    def active(self):
        return bool(self.blends) or self.lighting != 0.0

    def draw(self, rng):
        """One image's parameters: ``{"brightness": w, "contrast": w, "saturation": w, "lighting": [r, g, b]}`` with the active
        operations only, or None when PROB's draw (``RandomApply``) says not to apply.  ``w`` is a Python float as the reference's
        ``np.random.uniform`` gives it; the lighting vector is ``eigen_vecs @ (weights * eigen_vals)`` in double, RGB."""
        if self.prob < 1.0 and not rng.uniform() < self.prob:
            return None
        p = {}
        for name in self.blends:
            p[name] = float(rng.uniform(*self.ranges[name]))
        if self.lighting != 0.0:
            weights = rng.normal(scale=self.lighting, size=3)
            p["lighting"] = [float(v) for v in EIGEN_VECS.dot(weights * EIGEN_VALS)]
        return p

    def draw_pair(self, rng, has_twin):
        """(image's parameters, twin's parameters) under ``TWIN``; a parameter set is None where nothing is to be applied"""
        p = self.draw(rng)
        if not has_twin or self.twin == "none":
            return p, None
        return p, (p if self.twin == "same" else self.draw(rng))


def weights_f32(w):
    """(dw, sw) = (fl32(w), fl32(1 - w)), the subtraction in double"""
    return _F(w), _F(1.0 - float(w))


def _blend(x, sw, src, dw):
    """x: float32 array of byte values; src: float32 scalar or array.  -> float32 array of byte values"""
    v = sw * src + dw * x                                   # float32 throughout: np.float32 scalars and float32 arrays
    assert v.dtype == np.float32
    return np.trunc(np.minimum(np.maximum(v, _F(0)), _F(255)))


def color_jitter_u8(img_hwc, params, bgr, record=None):
    """uint8 [h, w, 3] -> a new uint8 [h, w, 3]: the active operations of ``params`` (``ColorJitter.draw``) chained, each on the uint8
    result of the one before.  ``bgr``: channel 0 is blue.  ``record``: a list that receives each blend's ``(name, src_weight,
    dst_weight, src_image)`` as this function used them (float32)."""
    img = np.asarray(img_hwc)
    assert img.dtype == np.uint8 and img.ndim == 3 and img.shape[2] == 3, "color_jitter_u8 takes a uint8 [h, w, 3] image"
    x = img.astype(np.float32)
    rec = record.append if record is not None else (lambda t: None)
    params = params or {}
    if "brightness" in params:
        dw, sw = weights_f32(params["brightness"])
        rec(("brightness", sw, dw, _F(0)))
        x = _blend(x, sw, _F(0), dw)
    if "contrast" in params:
        dw, sw = weights_f32(params["contrast"])
        total = int(x.astype(np.uint8).sum(dtype=np.int64))         # exact; x holds byte values
        mean = _F(total / x.size)                                    # the division in double: image.mean() of a uint8 array
        rec(("contrast", sw, dw, mean))
        x = _blend(x, sw, mean, dw)
    if "saturation" in params:
        dw, sw = weights_f32(params["saturation"])
        r, g, b = (x[..., 2], x[..., 1], x[..., 0]) if bgr else (x[..., 0], x[..., 1], x[..., 2])
        grey = ((_GREY[0] * r + _GREY[1] * g) + _GREY[2] * b)[..., None]
        assert grey.dtype == np.float32
        rec(("saturation", sw, dw, grey))
        x = _blend(x, sw, grey, dw)
    if "lighting" in params:
        vec = np.asarray(params["lighting"], dtype=np.float64).astype(np.float32)      # RGB
        rec(("lighting", _F(1), _F(1), vec))
        x = _blend(x, _F(1), vec[::-1] if bgr else vec, _F(1))
    return x.astype(np.uint8)


def _bits(v):
    return int(np.asarray(v, dtype=np.float32).view(np.int32))


def descriptor(off, h, w, params, bgr):
    """``cddmsl_jitter_item`` (include/cddmsl_color_jitter.h) as a tuple in member order: byte offset of the CHW image, h, w, the bit
    set of active operations, the channel-order flag, (dw, sw) of the three blends and the lighting offsets as float32 bits, 0."""
    params = params or {}
    ops, wbits = 0, []
    for name, bit in BLENDS:
        if name in params:
            ops |= bit
            dw, sw = weights_f32(params[name])
            wbits += [_bits(dw), _bits(sw)]
        else:
            wbits += [0, 0]
    light = [0, 0, 0]
    if "lighting" in params:
        ops |= LIGHTING
        light = [_bits(v) for v in params["lighting"]]
    return (int(off), int(h), int(w), ops, int(bool(bgr)), *wbits, *light, 0)

