"""Case builders for cddmsl_voc_match (cddmsl_amd/csrc/voc_match.hip), the VOC evaluator and the VOC-family catalog, imported by
tests/test_voc_eval_host.py and tests/test_gpu_voc_match.py; not a conftest; numpy only.

A case is ``{"names": image ids, "gt": per image [(class, difficult, [xmin, ymin, xmax, ymax] 1-based ints)], "dets": per image
(xyxy f32 [n,4], score f32 [n], class int64 [n])}`` over the 20 VOC classes.

``random_set(seed)``: ground-truth boxes are 20 x 20 pixels (inclusive) with corners on a grid of 10, a quarter of them copies of an
earlier box of the image (equal overlaps; second claims), a quarter difficult.  Detections are copies of a box, copies cut to a
height of 10..19 rows -- the overlap is then h / 20 EXACTLY, i.e. it lands on every threshold .50:.05:.95 --, copies shifted by 10,
and copies with a quarter-pixel offset (x.25 / x.75 times 10 is a ``.x5`` tie of the text rounding).  Scores are odd and even
sixteenths (an odd sixteenth times 1000 ends in .5: a ``.xxx5`` tie; few values, so rounded scores tie inside an image).  Class 3
has ground truth and no detections, class 5 detections and no ground truth, and one degenerate box (xmax = xmin - 1) with
detections of the same shape gives 0 / 0 overlaps.

``instrumented_walk`` is a copy of evaluation.class_ap's loop that counts which of its rules fired; the tests assert every counter
reaches 5 over the random sets: a condition on these INPUTS, not on the code under test."""
import os

import numpy as np

NUM_CLASSES = 20
USED = (0, 7, 14)                    # classes with ground truth and detections
GT_ONLY, DT_ONLY, DEGENERATE = 3, 5, 14
COUNTERS = ("on_threshold", "first_of_equal", "difficult_matched", "second_claim", "no_ground_truth", "equal_scores_in_image",
            "box_tie", "score_tie", "nan_overlap")
THRS = tuple(range(50, 100, 5))


def _name(i):
    return f"{i:06d}"


def _dets_for(rng, boxes_cls, n):
    """n detections derived from the image's boxes [(class, box)] (or free ones when there are none)"""
    b, s, c = [], [], []
    for _ in range(n):
        if boxes_cls:
            cls, (x0, y0, x1, y1) = boxes_cls[rng.randint(len(boxes_cls))]
            raw = [x0 - 1.0, y0 - 1.0, float(x1), float(y1)]            # reads back as the box itself
            kind = rng.randint(5)
            if kind == 1:
                raw[3] = y0 - 1.0 + rng.randint(10, 20)                 # h of 20 rows: overlap h / 20
            elif kind == 2:
                raw[0] += 10.0; raw[2] += 10.0
            elif kind == 3:
                raw[rng.randint(4)] += (0.25, 0.75)[rng.randint(2)]
            elif kind == 4:
                raw[1] += 10.0; raw[3] += 10.0; raw[2] -= rng.randint(0, 10)
            if rng.rand() < 0.2:
                cls = (USED + (DT_ONLY,))[rng.randint(4)]
        else:
            x, y = 10.0 * rng.randint(0, 12), 10.0 * rng.randint(0, 10)
            raw, cls = [x, y, x + 20.0, y + 20.0], (USED[0], DT_ONLY)[rng.randint(2)]
        b.append(raw); c.append(cls); s.append(rng.randint(1, 16) / 16.0)
    return np.array(b, dtype=np.float32).reshape(-1, 4), np.array(s, dtype=np.float32), np.array(c, dtype=np.int64)


def _grid_box(rng):
    x, y = 1 + 10 * rng.randint(0, 13), 1 + 10 * rng.randint(0, 10)
    return [x, y, x + 19, y + 19]


def random_set(seed, n_images=10):
    rng = np.random.RandomState(seed)
    gt, dets = [], []
    for i in range(n_images):
        objs = []
        for _ in range(rng.randint(0, 7)):
            if objs and rng.rand() < 0.25:
                cls, _, box = objs[rng.randint(len(objs))]
                box = list(box)
            else:
                cls, box = (USED + (GT_ONLY,))[rng.randint(4)], _grid_box(rng)
            objs.append((cls, int(rng.rand() < 0.25), box))
        if i == 0:                                                       # 0 / 0 overlaps: zero-width box, zero-width detections
            objs.append((DEGENERATE, 0, [50, 50, 49, 60]))
        b, s, c = _dets_for(rng, [(o[0], o[2]) for o in objs if o[0] != GT_ONLY], rng.randint(0, 3 * len(objs) + 3))
        if i == 0:
            b = np.concatenate([b, np.array([[49, 49, 49, 60]] * 3, dtype=np.float32)])
            s = np.concatenate([s, np.array([0.9375, 0.5, 0.5], dtype=np.float32)])
            c = np.concatenate([c, np.full(3, DEGENERATE, dtype=np.int64)])
        gt.append(objs); dets.append((b, s, c))
    return {"names": [_name(i) for i in range(n_images)], "gt": gt, "dets": dets}


def segment_case(n_gt, n_det, seed=0):
    """one image, one class (0): ``n_gt`` boxes (copies and difficult ones among them) and ``n_det`` detections"""
    rng = np.random.RandomState(1000 * n_gt + n_det + seed)
    objs = []
    for _ in range(n_gt):
        box = list(objs[rng.randint(len(objs))][2]) if objs and rng.rand() < 0.2 else _grid_box(rng)
        objs.append((0, int(rng.rand() < 0.2), box))
    b, s, _ = _dets_for(rng, [(0, o[2]) for o in objs], n_det)
    return {"names": [_name(0)], "gt": [objs], "dets": [(b, s, np.zeros(n_det, dtype=np.int64))]}


def tiny_set(seed, n_images=3, prefix="t"):
    """three images of 128 x 160 for the catalog tests: boxes inside the frame, detections near them"""
    rng = np.random.RandomState(seed)
    gt, dets = [], []
    for _ in range(n_images):
        objs = []
        for _ in range(rng.randint(1, 4)):
            x, y = 1 + 10 * rng.randint(0, 10), 1 + 10 * rng.randint(0, 7)
            objs.append((USED[rng.randint(3)], 0, [x, y, x + 39, y + 39]))
        b, s, c = _dets_for(rng, [(o[0], o[2]) for o in objs], 4)
        gt.append(objs); dets.append((b, s, c))
    return {"names": [f"{prefix}{seed}_{i}" for i in range(n_images)], "gt": gt, "dets": dets}


# ------------------------------------------------------------------------------------------------ views of a case
def flat_dets(case):
    """the gathered detections in processing order: (boxes f32 [D,4], scores f32 [D], classes int64 [D], image indices int64 [D])"""
    b = np.concatenate([d[0].reshape(-1, 4) for d in case["dets"]]).astype(np.float32)
    s = np.concatenate([d[1] for d in case["dets"]]).astype(np.float32)
    c = np.concatenate([d[2] for d in case["dets"]]).astype(np.int64)
    img = np.repeat(np.arange(len(case["dets"]), dtype=np.int64), [len(d[1]) for d in case["dets"]])
    return b, s, c, img


def gt_by_class(case):
    """what the evaluator builds from the XML: per class {image id: (bbox [G,4] float, difficult [G] bool)}"""
    out = []
    for k in range(NUM_CLASSES):
        gt = {}
        for n, objs in zip(case["names"], case["gt"]):
            mine = [o for o in objs if o[0] == k]
            gt[n] = (np.array([o[2] for o in mine], dtype=float).reshape(-1, 4), np.array([o[1] for o in mine], dtype=bool))
        out.append(gt)
    return out


def gt_rows(case):
    """the kernel's CSR rows: row = class * n_images + image index"""
    return [gt[n] for gt in gt_by_class(case) for n in case["names"]]


def text_round_trip(case):
    """the host evaluator's ``process``, verbatim: per class [(image id, score, xmin, ymin, xmax, ymax)] read back from the reference's
    result line, plus each line's index into ``flat_dets``"""
    lines, flat = {k: [] for k in range(NUM_CLASSES)}, {k: [] for k in range(NUM_CLASSES)}
    i = 0
    for n, (boxes, scores, classes) in zip(case["names"], case["dets"]):
        for (x0, y0, x1, y1), s, c in zip(boxes, scores.tolist(), classes.tolist()):
            lines[c].append((n, float(f"{s:.3f}"), float(f"{x0 + 1:.1f}"), float(f"{y0 + 1:.1f}"), float(f"{x1:.1f}"), float(f"{y1:.1f}")))
            flat[c].append(i)
            i += 1
    return lines, flat


def _ties(values, scale):
    v = np.asarray(values, dtype=np.float32).astype(np.float64) * scale
    return int((v - np.floor(v) == 0.5).sum())


def instrumented_walk(case, count=None):
    """evaluation.class_ap's loop, line for line, for every class and threshold on the text-round-tripped detections, with counters
    on the rules -> (tp bits uint16 [D], fp bits uint16 [D]) indexed like ``flat_dets`` (bit t = threshold THRS[t])"""
    count = count if count is not None else {k: 0 for k in COUNTERS}
    lines, flat = text_round_trip(case)
    gts = gt_by_class(case)
    D = sum(len(d[1]) for d in case["dets"])
    tpb, fpb = np.zeros(D, dtype=np.uint16), np.zeros(D, dtype=np.uint16)
    b, s, _, _ = flat_dets(case)
    count["box_tie"] += _ties(b[:, 2:], 10.0) + _ties(b[:, :2] + np.float32(1.0), 10.0)
    count["score_tie"] += _ties(s, 1000.0)
    for k in range(NUM_CLASSES):
        gt_by_image = gts[k]
        image_ids = [l[0] for l in lines[k]]
        confidence = np.array([l[1] for l in lines[k]], dtype=float)
        boxes = np.array([l[2:] for l in lines[k]], dtype=float).reshape(-1, 4)
        for n in set(image_ids):
            sc = confidence[[i for i, m in enumerate(image_ids) if m == n]]
            count["equal_scores_in_image"] += len(sc) - len(np.unique(sc))
        for t, thresh in enumerate(THRS):
            ovthresh = thresh / 100.0
            claimed = {key: np.zeros(len(d), dtype=bool) for key, (_, d) in gt_by_image.items()}
            order = np.argsort(-confidence)
            for d in order:
                gtb, diff = gt_by_image[image_ids[d]]
                best, arg = -np.inf, -1
                if gtb.size:
                    bb = boxes[d]
                    with np.errstate(invalid="ignore", divide="ignore"):
                        iw = np.maximum(np.minimum(gtb[:, 2], bb[2]) - np.maximum(gtb[:, 0], bb[0]) + 1.0, 0.0)
                        ih = np.maximum(np.minimum(gtb[:, 3], bb[3]) - np.maximum(gtb[:, 1], bb[1]) + 1.0, 0.0)
                        inter = iw * ih
                        union = (bb[2] - bb[0] + 1.0) * (bb[3] - bb[1] + 1.0) + (gtb[:, 2] - gtb[:, 0] + 1.0) * (gtb[:, 3] - gtb[:, 1] + 1.0) - inter
                        ov = inter / union
                    arg = int(np.argmax(ov))
                    best = ov[arg]
                    count["nan_overlap"] += int(np.isnan(best))
                    count["first_of_equal"] += int(best > 0 and (ov == best).sum() > 1)
                else:
                    count["no_ground_truth"] += 1
                count["on_threshold"] += int(best == ovthresh)
                if best > ovthresh:
                    if not diff[arg]:
                        if not claimed[image_ids[d]][arg]:
                            tpb[flat[k][d]] |= np.uint16(1 << t)
                            claimed[image_ids[d]][arg] = True
                        else:
                            count["second_claim"] += 1
                            fpb[flat[k][d]] |= np.uint16(1 << t)
                    else:
                        count["difficult_matched"] += 1
                else:
                    fpb[flat[k][d]] |= np.uint16(1 << t)
    return tpb, fpb


def class_aps(case, use_07_metric):
    """the yardstick's values: evaluation.class_ap per class and threshold on the text-round-tripped detections -> [K][T]"""
    from cddmsl_amd.evaluation import class_ap
    lines, _ = text_round_trip(case)
    gts = gt_by_class(case)
    out = []
    with np.errstate(invalid="ignore", divide="ignore"):
        for k in range(NUM_CLASSES):
            ids = [l[0] for l in lines[k]]
            conf = np.array([l[1] for l in lines[k]], dtype=float)
            bbs = np.array([l[2:] for l in lines[k]], dtype=float).reshape(-1, 4)
            out.append([class_ap(ids, conf, bbs, gts[k], t / 100.0, use_07_metric) for t in THRS])
    return out


# ------------------------------------------------------------------------------------------------ a devkit tree on disk
def write_voc_tree(dirname, split, case, class_names, images=False, hw=(128, 160)):
    """Annotations/<id>.xml + ImageSets/Main/<split>.txt (+ JPEGImages/<id>.jpg holding a PNG) of a case"""
    for sub in ("Annotations", os.path.join("ImageSets", "Main"), "JPEGImages"):
        os.makedirs(os.path.join(dirname, sub), exist_ok=True)
    rng = np.random.RandomState(len(case["names"]))
    for n, objs in zip(case["names"], case["gt"]):
        body = "".join(f"<object><name>{class_names[c]}</name><difficult>{d}</difficult><bndbox><xmin>{b[0]}</xmin><ymin>{b[1]}</ymin>"
                       f"<xmax>{b[2]}</xmax><ymax>{b[3]}</ymax></bndbox></object>" for c, d, b in objs)
        with open(os.path.join(dirname, "Annotations", n + ".xml"), "w") as f:
            f.write(f"<annotation><filename>{n}.jpg</filename><size><width>{hw[1]}</width><height>{hw[0]}</height><depth>3</depth></size>{body}</annotation>")
        if images:
            from PIL import Image
            Image.fromarray(rng.randint(0, 256, (hw[0], hw[1], 3)).astype(np.uint8)).save(os.path.join(dirname, "JPEGImages", n + ".jpg"), format="PNG")
    with open(os.path.join(dirname, "ImageSets", "Main", split + ".txt"), "w") as f:
        f.write("".join(n + "\n" for n in case["names"]))


def write_family(root):
    """VOC2007 + VOC2012 trainval (three images each) with dt_clipart twins, VOC2007 test, clipart test"""
    from cddmsl_amd.evaluation import VOC_CLASS_NAMES
    cases = {"VOC2007": tiny_set(1, prefix="a"), "VOC2012": tiny_set(2, prefix="b")}
    for d, case in cases.items():
        write_voc_tree(os.path.join(root, d), "trainval", case, VOC_CLASS_NAMES, images=True)
        write_voc_tree(os.path.join(root, "dt_clipart", d), "trainval", case, VOC_CLASS_NAMES, images=True)
    cases["test"] = tiny_set(3, prefix="c")
    write_voc_tree(os.path.join(root, "VOC2007"), "test", cases["test"], VOC_CLASS_NAMES, images=True)
    cases["clipart"] = tiny_set(4, prefix="d")
    write_voc_tree(os.path.join(root, "clipart"), "test", cases["clipart"], VOC_CLASS_NAMES, images=True)
    return cases


def instances_of(case, device="cpu"):
    """[(inputs, outputs)] per image, as ``evaluator.process`` takes them"""
    import torch
    from cddmsl_amd.structures import Boxes, Instances
    out = []
    for n, (b, s, c) in zip(case["names"], case["dets"]):
        inst = Instances((128, 160), pred_boxes=Boxes(torch.from_numpy(b).to(device)), scores=torch.from_numpy(s).to(device),
                         pred_classes=torch.from_numpy(c).to(device))
        out.append(([{"image_id": n}], [{"instances": inst}]))
    return out


def same_results(a, b):
    """two result dictionaries equal value for value (a NaN equals a NaN), keys in the same order"""
    return list(a) == list(b) and all(list(a[k]) == list(b[k]) and all(x == y or (x != x and y != y) for x, y in zip(a[k].values(), b[k].values()))
                                      for k in a)


_CACHE = {}


def cached(key, fn):
    """one computation per test process (the host walk is a Python loop: references are computed once and shared)"""
    if key not in _CACHE:
        _CACHE[key] = fn()
    return _CACHE[key]
