"""Case builders for cddmsl_coco_match (cddmsl_amd/csrc/coco_match.hip) and the COCO evaluator, imported by
tests/test_coco_eval_host.py and tests/test_gpu_coco_match.py; not a conftest; numpy only.

``random_set(seed)``: 12 images, 3 classes, boxes on an integer grid so that exact IoU ties and threshold hits occur -- corners are
multiples of 16, sides come from {16, 32, 48, 96, 192} (areas land exactly on 32^2 and 96^2), 0-13 ground-truth boxes per image (20 %
crowd, some of them copies of an earlier box of the image), detections are ground-truth boxes with every coordinate shifted by -16,
0 or +16 (sides clamped at 0: some are zero-area), 20 % of them with a random class, scores on a grid of eighths (many equal,
within and across images); plus one image with 130 detections of one class.  ``edge_set()``: the shapes at which the kernel takes
another path (empty sides, D = G = 1, 100 / 101 detections of one class, 33 / 65 / cap / cap + 1 boxes of one class).

``instrumented_match`` is a copy of evaluation._coco_match's loop that counts which of its rules fired; ``rule_counters`` sums
them over a set.  The tests assert every counter is non-zero: a condition on these INPUTS, not on the code under test."""
import numpy as np

SIDES = (16, 32, 48, 96, 192)
NUM_CLASSES = 3
COUNTERS = ("later_wins_tie", "break_at_ignored", "crowd_rematch", "match_to_ignored", "nan_iou", "iou_on_threshold", "gt_area_on_edge",
            "dt_area_on_edge", "unmatched_out_of_range", "skip_matched")


def _ann(x0, y0, w, h, cls, crowd):
    return {"bbox": [float(x0), float(y0), float(x0 + w), float(y0 + h)], "area": float(w * h), "iscrowd": int(crowd), "category_id": int(cls)}


def _dets_from(rng, anns, n, p_random_cls=0.2):
    boxes, scores, classes = [], [], []
    for _ in range(n):
        a = anns[rng.randint(len(anns))]
        b = np.array(a["bbox"]) + 16.0 * rng.randint(-1, 2, size=4)
        b[2], b[3] = max(b[2], b[0]), max(b[3], b[1])              # sides clamped at 0
        boxes.append(b)
        scores.append(rng.randint(1, 9) / 8.0)
        classes.append(rng.randint(NUM_CLASSES) if rng.rand() < p_random_cls else a["category_id"])
    return (np.array(boxes, dtype=np.float32).reshape(-1, 4), np.array(scores, dtype=np.float32), np.array(classes, dtype=np.int64))


def _image(image_id, anns, dets):
    return {"image_id": image_id, "height": 1024, "width": 1024, "annotations": anns}, dets


def _empty_dets():
    return np.zeros((0, 4), dtype=np.float32), np.zeros(0, dtype=np.float32), np.zeros(0, dtype=np.int64)


def random_set(seed):
    """-> (dataset dicts, [(xyxy f32 [D,4], score f32 [D], class int64 [D])] per image)"""
    rng = np.random.RandomState(seed)
    dicts, dets = [], []
    for i in range(12):
        anns = []
        for _ in range(rng.randint(0, 14)):
            if anns and rng.rand() < 0.25:                           # the same box again (another flag, maybe another class)
                x0, y0, x1, y1 = anns[rng.randint(len(anns))]["bbox"]
                w, h = x1 - x0, y1 - y0
            else:
                x0, y0 = 16 * rng.randint(2, 14), 16 * rng.randint(2, 14)
                w, h = SIDES[rng.randint(len(SIDES))], SIDES[rng.randint(len(SIDES))]
            anns.append(_ann(x0, y0, w, h, rng.randint(NUM_CLASSES), rng.rand() < 0.2))
        d = _dets_from(rng, anns, rng.randint(0, 3 * len(anns) + 1)) if anns else _empty_dets()
        im, d = _image(f"s{seed}_{i:02d}", anns, d)
        dicts.append(im); dets.append(d)
    anns = [_ann(16 * rng.randint(2, 8), 16 * rng.randint(2, 8), SIDES[rng.randint(5)], SIDES[rng.randint(5)], 1, rng.rand() < 0.2) for _ in range(9)]
    im, d = _image(f"s{seed}_130", anns, _dets_from(rng, anns, 130, p_random_cls=0.0))
    dicts.append(im); dets.append(d)
    return dicts, dets


def edge_set(gt_cap):
    """the edge shapes, one image each; ``gt_cap`` = ground-truth boxes of one class the kernel holds (cap and cap + 1 are both built)"""
    rng = np.random.RandomState(1234)
    dicts, dets = [], []

    def add(name, anns, d):
        im, d = _image("edge_" + name, anns, d)
        dicts.append(im); dets.append(d)

    some = [_ann(32, 32, 96, 48, 0, False), _ann(64, 32, 96, 96, 1, False), _ann(32, 64, 32, 32, 0, True)]
    add("no_gt", [], _dets_from(rng, some, 7))
    add("no_dets", some, _empty_dets())
    add("neither", [], _empty_dets())
    add("one_one", some[:1], _dets_from(rng, some[:1], 1, 0.0))
    for n in (100, 101):
        add(f"d{n}", some, _dets_from(rng, [some[0], some[2]], n, 0.0))
    for g in (33, 65, gt_cap, gt_cap + 1):
        anns = [_ann(16 * rng.randint(2, 10), 16 * rng.randint(2, 10), SIDES[rng.randint(5)], SIDES[rng.randint(5)], 2, rng.rand() < 0.2) for _ in range(g)]
        anns.append(_ann(48, 48, 96, 96, 0, False))
        add(f"g{g}", anns, _dets_from(rng, anns, 12 if g >= gt_cap else 40, 0.1))
    return dicts, dets


def gt_tuples(dicts):
    """the evaluator's view of the ground truth: per image (xywh f64 [G,4], area f64 [G], crowd bool [G], class int64 [G])"""
    out = []
    for d in dicts:
        anns = d["annotations"]
        xyxy = np.array([a["bbox"] for a in anns], dtype=np.float64).reshape(-1, 4)
        out.append((np.concatenate([xyxy[:, :2], xyxy[:, 2:] - xyxy[:, :2]], axis=1), np.array([a["area"] for a in anns], dtype=np.float64),
                    np.array([bool(a["iscrowd"]) for a in anns], dtype=bool), np.array([a["category_id"] for a in anns], dtype=np.int64)))
    return out


def dt_tuples(dets):
    """the host evaluator's view of the detections: per image (xywh f64, score f64, class)"""
    out = []
    for b, s, c in dets:
        b = b.astype(np.float64)
        out.append((np.concatenate([b[:, :2], b[:, 2:] - b[:, :2]], axis=1), s.astype(np.float64), c))
    return out


def instrumented_match(dt_boxes, dt_scores, gt_boxes, gt_area, gt_crowd, area_rng, count):
    """evaluation._coco_match, line for line, with counters on the rules -> (matched [T,D], ignored [T,D])"""
    from cddmsl_amd.evaluation import COCO_IOU_THRS, COCO_MAX_DETS, coco_box_iou
    gt_ig = gt_crowd | (gt_area < area_rng[0]) | (gt_area > area_rng[1])
    count["gt_area_on_edge"] += int(np.isin(gt_area, area_rng).sum())
    gorder = np.argsort(gt_ig, kind="mergesort")
    gb, gig, gcrowd = gt_boxes[gorder], gt_ig[gorder], gt_crowd[gorder]
    dorder = np.argsort(-dt_scores, kind="mergesort")[:COCO_MAX_DETS]
    db = dt_boxes[dorder]
    with np.errstate(invalid="ignore", divide="ignore"):
        ious = coco_box_iou(db, gb, gcrowd)
    T, D, G = len(COCO_IOU_THRS), len(db), len(gb)
    gtm, dtm, dtig = np.zeros((T, G), dtype=bool), np.zeros((T, D), dtype=bool), np.zeros((T, D), dtype=bool)
    for ti, t in enumerate(COCO_IOU_THRS):
        for d in range(D):
            iou, m = min(t, 1 - 1e-10), -1
            for g in range(G):
                if gtm[ti, g] and not gcrowd[g]:
                    count["skip_matched"] += 1
                    continue
                if m > -1 and not gig[m] and gig[g]:
                    count["break_at_ignored"] += 1
                    break
                v = ious[d, g]
                count["nan_iou"] += int(np.isnan(v))
                if v < iou:
                    continue
                if m > -1 and v == iou:
                    count["later_wins_tie"] += 1
                if m == -1 and v == iou:
                    count["iou_on_threshold"] += 1
                iou, m = v, g
            if m == -1:
                continue
            count["crowd_rematch"] += int(gtm[ti, m])
            count["match_to_ignored"] += int(gig[m])
            dtig[ti, d], dtm[ti, d], gtm[ti, m] = gig[m], True, True
    darea = db[:, 2] * db[:, 3]
    count["dt_area_on_edge"] += int(np.isin(darea, area_rng).sum())
    out_rng = (darea < area_rng[0]) | (darea > area_rng[1])
    count["unmatched_out_of_range"] += int((~dtm & out_rng[None, :]).sum())
    dtig |= ~dtm & out_rng[None, :]
    return dtm, dtig


def rule_counters(dicts, dets):
    """which rules of the walk the set exercises -> {counter: times}; also checks the instrumented copy against the real matcher"""
    from cddmsl_amd.evaluation import COCO_AREA_RNGS, _coco_match
    count = {k: 0 for k in COUNTERS}
    for (gb, garea, gcrowd, gcls), (db, ds, dc) in zip(gt_tuples(dicts), dt_tuples(dets)):
        for k in range(NUM_CLASSES):
            g, d = gcls == k, dc == k
            for rng in COCO_AREA_RNGS:
                m, ig = instrumented_match(db[d], ds[d], gb[g], garea[g], gcrowd[g], rng, count)
                with np.errstate(invalid="ignore", divide="ignore"):
                    _, m0, ig0, _ = _coco_match(db[d], ds[d], gb[g], garea[g], gcrowd[g], rng)
                assert np.array_equal(m, m0) and np.array_equal(ig, ig0)
    return count


_CACHE = {}


def cached(key, fn):
    """one computation per test process (the host matcher is a Python loop: references are computed once and shared)"""
    if key not in _CACHE:
        _CACHE[key] = fn()
    return _CACHE[key]
