"""Reference arithmetic of test-time augmentation (imported by tests/test_tta_host.py and tests/test_gpu_tta.py; not a conftest;
numpy only -- no PIL, no torch and no GPU needed to import).

  * ``resize``: Pillow's ``Image.resize((neww, newh), BILINEAR)`` on uint8 [h, w, 3] as plain integer arithmetic: per axis the windows
    and double-precision triangle weights of ``precompute_coeffs`` (scalar loops, Pillow's order of operations), 22-bit fixed-point
    coefficients, ``clip8((2^21 + sum k * pixel) >> 22)`` per pass, horizontal pass first with a uint8 intermediate, a pass whose
    size does not change skipped.  tests/test_tta_host.py ties it to the installed Pillow bit for bit; the GPU tests depend on this
    restatement, not on the Pillow of the GPU box.
  * ``view_list`` / ``views``: the reference's views and their order (test_time_augmentation.py:79-98).
  * ``unmap`` / ``merge``: the inverse transforms on float32 boxes and the merge (one-hot scores, threshold 1e-8, clip, per-class hard
    NMS through the coordinate offset, top-k) in numpy float32, one IEEE operation at a time; the NMS walk is tests/exact_boxes.py's.
"""
import math

import numpy as np

import exact_boxes as XB

F32 = np.float32
PRECISION_BITS = 22

# (h, w) -> (newh, neww): upscale, downscale by 1.5 to 2.7, one axis unchanged, identity, and a factor 4 (ksize 9)
PAIRS = [((37, 53), (24, 34)), ((37, 53), (60, 86)), ((48, 64), (48, 64)), ((50, 31), (25, 16)), ((33, 80), (20, 48)),
         ((64, 48), (96, 72)), ((19, 23), (7, 9)), ((120, 90), (45, 34)), ((30, 30), (30, 61)), ((120, 90), (30, 23))]


def shortest_edge_size(h, w, size, max_size):
    """ResizeShortestEdge.get_output_shape (augmentation_impl.py:188-198)"""
    scale = size * 1.0 / min(h, w)
    newh, neww = (size, scale * w) if h < w else (scale * h, size)
    if max(newh, neww) > max_size:
        scale = max_size * 1.0 / max(newh, neww)
        newh, neww = newh * scale, neww * scale
    return int(newh + 0.5), int(neww + 0.5)


def coeffs(insize, outsize):
    """-> (xmin [out], n [out], k [out][ksize] int, ksize) of the bilinear filter along one axis"""
    scale = insize / outsize
    fs = max(scale, 1.0)
    support = 1.0 * fs
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / fs
    xmins, ns, ks = [], [], []
    for i in range(outsize):
        center = (i + 0.5) * scale
        xmin = max(0, int(center - support + 0.5))
        xmax = min(insize, int(center + support + 0.5))
        n = xmax - xmin
        w, ww = [], 0.0
        for x in range(n):
            a = abs((x + xmin - center + 0.5) * ss)
            v = 1.0 - a if a < 1.0 else 0.0
            w.append(v)
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        k = [int(0.5 + v * (1 << PRECISION_BITS)) for v in w]           # bilinear weights are never negative
        xmins.append(xmin), ns.append(n), ks.append(k + [0] * (ksize - n))
    return xmins, ns, ks, ksize


def _pass(img, axis, outsize):
    """one pass along ``axis`` (0 vertical, 1 horizontal) of uint8 [h, w, c] -> uint8"""
    xmins, ns, ks, _ = coeffs(img.shape[axis], outsize)
    src = np.moveaxis(img, axis, 0).astype(np.int32)                      # int32 is exact: the sum stays below 255 * 2^22 + 2^21 < 2^31
    out = np.empty((outsize,) + src.shape[1:], dtype=np.uint8)
    for i in range(outsize):
        acc = np.full(src.shape[1:], 1 << (PRECISION_BITS - 1), dtype=np.int32)
        for t in range(ns[i]):
            acc = acc + src[xmins[i] + t] * np.int32(ks[i][t])
        out[i] = np.clip(acc >> PRECISION_BITS, 0, 255).astype(np.uint8)
    return np.moveaxis(out, 0, axis)


def resize(img, newh, neww):
    """uint8 [h, w, 3] -> uint8 [newh, neww, 3], Pillow bilinear"""
    assert img.dtype == np.uint8 and img.ndim == 3
    out = img
    if neww != img.shape[1]:
        out = _pass(out, 1, neww)
    if newh != img.shape[0]:
        out = _pass(out, 0, newh)
    return np.ascontiguousarray(out)


def view_list(in_h, in_w, min_sizes, max_size, flip):
    """[(newh, neww, flipped)] in the reference's order [s0, s0 mirrored, s1, ...]"""
    out = []
    for s in min_sizes:
        nh, nw = shortest_edge_size(in_h, in_w, s, max_size)
        out.append((nh, nw, False))
        if flip:
            out.append((nh, nw, True))
    return out


def views(img, min_sizes, max_size, flip):
    """uint8 [h, w, 3] -> [(uint8 view [newh, neww, 3], (newh, neww, flipped))]"""
    out = []
    for nh, nw, f in view_list(img.shape[0], img.shape[1], min_sizes, max_size, flip):
        v = resize(img, nh, nw)
        out.append((np.ascontiguousarray(v[:, ::-1]) if f else v, (nh, nw, f)))
    return out


def seeded_image(h, w, seed):
    return np.random.RandomState(seed).randint(0, 256, (h, w, 3), dtype=np.uint8)


# ================================================================================================================ boxes
def unmap(boxes, record):
    """float32 XYXY boxes of one view -> the dataset image's coordinates; record = (orig_h, orig_w, in_h, in_w, newh, neww, flipped)"""
    orig_h, orig_w, in_h, in_w, newh, neww, flipped = record
    b = np.array(boxes, dtype=np.float32).reshape(-1, 4)
    if flipped:
        x0, x1 = F32(neww) - b[:, 2], F32(neww) - b[:, 0]
        b[:, 0], b[:, 2] = x0, x1
    b[:, 0::2] = b[:, 0::2] * F32(in_w / neww)
    b[:, 1::2] = b[:, 1::2] * F32(in_h / newh)
    if (in_h, in_w) != (orig_h, orig_w):
        b[:, 0::2] = b[:, 0::2] * F32(orig_w / in_w)
        b[:, 1::2] = b[:, 1::2] * F32(orig_h / in_h)
    assert b.dtype == np.float32
    return b


def merge(per_view, records, shape_hw, nms_thresh, topk, score_thresh=1e-8):
    """per_view = [(boxes f32 [r, 4], scores f32 [r], classes [r])] -> (boxes, scores, classes) of the merged detections, in order"""
    boxes = np.concatenate([unmap(b, r) for (b, _, _), r in zip(per_view, records)]).astype(np.float32)
    scores = np.concatenate([np.asarray(s, np.float32) for _, s, _ in per_view])
    classes = np.concatenate([np.asarray(c, np.int64) for _, _, c in per_view])
    ok = np.isfinite(boxes).all(axis=1) & np.isfinite(scores)
    boxes, scores, classes = boxes[ok], scores[ok], classes[ok]
    h, w = shape_hw
    boxes[:, 0::2] = np.clip(boxes[:, 0::2], F32(0), F32(w))
    boxes[:, 1::2] = np.clip(boxes[:, 1::2], F32(0), F32(h))
    cand = scores > F32(score_thresh)
    boxes, scores, classes = boxes[cand], scores[cand], classes[cand]
    if len(scores) == 0:
        return boxes, scores, classes
    off = classes.astype(np.float32) * (boxes.max() + F32(1.0))          # torchvision's coordinate trick, in f32
    shifted = boxes + off[:, None]
    order = np.argsort(-scores, kind="stable")                            # descending, ties to the first index
    kept = XB.nms_ref(shifted[order], np.ones(len(order), np.int32), nms_thresh, len(order))
    keep = order[kept][:topk] if topk >= 0 else order[kept]
    return boxes[keep], scores[keep], classes[keep]
