"""Case builders for proposal recall (cddmsl_amd/csrc/proposal_recall.hip, evaluation.ProposalRecallEvaluator), imported by
tests/test_proposal_recall_host.py, tests/test_gpu_proposal_recall.py and tests/golden/make_golden_proposal_recall.py.

Rules: ground-truth coordinates are multiples of 0.25 below 2048, so XYWH <-> XYXY is exact in double and in f32; proposal
coordinates are arbitrary f32; all logits of an image are distinct (the reference's ``Tensor.sort`` is not stable, so tie order is
pinned only against the package's host walk, in ``tie_case``)."""
import numpy as np

LIMITS = (100, 1000, None)


def _quarter(r, n, lo, hi):
    return np.round(r.uniform(lo, hi, size=n) * 4.0) / 4.0


def _gt_boxes(r, n, min_side=8.0, max_side=400.0):
    x0, y0 = _quarter(r, n, 0, 1500), _quarter(r, n, 0, 1500)
    w, h = _quarter(r, n, min_side, max_side), _quarter(r, n, min_side, max_side)
    return np.stack([x0, y0, x0 + w, y0 + h], axis=1)


def _logits(r, n):
    """n distinct f32 values in a shuffled order"""
    return (r.permutation(n).astype(np.float64) * 0.01 - 4.0).astype(np.float32)


def _proposals(r, gt, n):
    """jittered ground truth (arbitrary f32 coordinates) + random boxes, n in all"""
    out = []
    for k in range(n):
        if len(gt) and k % 3 != 2:
            b = gt[r.randint(len(gt))] + r.randn(4) * r.choice([0.5, 4.0, 25.0])
        else:
            x0, y0 = r.uniform(0, 1700, size=2)
            b = np.array([x0, y0, x0 + r.uniform(1, 300), y0 + r.uniform(1, 300)])
        out.append([min(b[0], b[2]), min(b[1], b[3]), max(b[0], b[2]), max(b[1], b[3])])
    return np.asarray(out, dtype=np.float64).reshape(-1, 4).astype(np.float32)


def _ann(box, area=None, crowd=0):
    a = {"bbox": [float(v) for v in box], "category_id": 0, "iscrowd": int(crowd)}
    if area is not None:
        a["area"] = area
    return a


def dataset():
    """-> [(dataset dict, proposal boxes f32 [P, 4], logits f32 [P])]: a dozen images covering P in {0, 1, 99, 100, 101, 1200},
    G in {0, 1, many}, P < G, duplicate proposals and boxes, a proposal equal to a box, zero-area proposals, non-overlapping pairs,
    a crowd box, stored areas exactly on and just off the range edges, and an image whose boxes all miss a range"""
    r = np.random.RandomState(20240607)
    items = []

    def add(anns, boxes, logits=None):
        boxes = np.ascontiguousarray(boxes, dtype=np.float32).reshape(-1, 4)
        logits = _logits(r, len(boxes)) if logits is None else np.asarray(logits, dtype=np.float32)
        assert len(np.unique(logits)) == len(logits)
        items.append(({"image_id": f"img{len(items):02d}", "height": 2048, "width": 2048, "annotations": anns}, boxes, logits))

    # 0: P = 1200, many boxes of all sizes; duplicates of proposals and of boxes, a proposal equal to a box, zero-area proposals
    gt = np.concatenate([_gt_boxes(r, 14, 6.0, 60.0), _gt_boxes(r, 16, 40.0, 700.0)])
    gt[7] = gt[3]                                  # duplicate boxes: exact IoU ties between columns
    p = _proposals(r, gt, 1200)
    p[10] = p[500] = gt[3].astype(np.float32)        # two proposals equal to a (duplicated) box: IoU 1, ties between rows
    p[20] = p[21]
    p[30, 2] = p[30, 0]                              # zero width
    p[31] = [100.5, 200.25, 100.5, 200.25]           # a point
    add([_ann(b) for b in gt], p)
    # 1: boxes and no proposals (the reference does not count these boxes)
    add([_ann(b) for b in _gt_boxes(r, 3)], np.zeros((0, 4)))
    # 2: P = 1, G = 1
    gt = _gt_boxes(r, 1)
    add([_ann(gt[0])], _proposals(r, gt, 1))
    # 3-5: P at the limit of 100 and one either side; the lowest-ranked proposal is the only good one for box 0
    for n in (99, 100, 101):
        gt = _gt_boxes(r, 5)
        p = _proposals(r, gt[1:], n)
        lg = _logits(r, n)
        last = int(np.argmin(lg))
        p[last] = (gt[0] + np.array([0.5, 0.25, -0.5, 0.0])).astype(np.float32)
        add([_ann(b) for b in gt], p, lg)
    # 6: P < G
    gt = _gt_boxes(r, 8)
    add([_ann(b) for b in gt], _proposals(r, gt, 3))
    # 7: proposals and no boxes
    add([], _proposals(r, np.zeros((0, 4)), 50))
    # 8: a crowd box; stored areas exactly 1024 (small and medium), 9216 (medium and large), 1024.00001 (1024 after float32)
    gt = _gt_boxes(r, 5, 20.0, 120.0)
    add([_ann(gt[0], area=1024), _ann(gt[1], area=9216), _ann(gt[2], area=1024.00001), _ann(gt[3], area=500.5, crowd=1),
         _ann(gt[4], area=9216.001)], _proposals(r, gt, 40))
    # 9: every box large (nothing in "small" ... "256-512" below its size); the proposals overlap none of them
    gt = np.array([[0, 0, 600, 600], [700, 0, 1300, 620.5], [0, 700, 640.25, 1400]], dtype=np.float64)
    far = np.array([[1500 + 10 * k, 1500 + 7 * k, 1540 + 10 * k, 1560 + 7 * k] for k in range(20)], dtype=np.float64)
    add([_ann(b) for b in gt], far)
    # 10: two boxes that are the same box and two proposals equal to it, plus a near miss
    box = np.array([64.0, 32.0, 192.0, 160.0])
    add([_ann(box), _ann(box)], np.array([box, box, box + [1.5, 0, 1.5, 0]] + [[300 + k, 300, 340 + k, 350] for k in range(7)]))
    # 11: P = 1200 where the limit of 1000 matters: the good proposals of the first three boxes rank below 1000
    gt = _gt_boxes(r, 12)
    p = _proposals(r, gt[3:], 1200)
    lg = _logits(r, 1200)
    low = np.argsort(lg)[:3]
    for k, i in enumerate(low):
        p[i] = (gt[k] + np.array([1.0, 0.5, -0.25, 0.0])).astype(np.float32)
    add([_ann(b) for b in gt], p, lg)
    return items


def tie_case():
    """equal logits (the stable order decides which of two different proposals survives the limit) and a NaN logit, which ranks
    last; pinned against the package's host walk only -> (gt boxes f32 [G, 4], range bits u8 [G], boxes f32 [P, 4], logits f32 [P])"""
    r = np.random.RandomState(7)
    gt = _gt_boxes(r, 6).astype(np.float32)
    p = _proposals(r, gt, 130)
    lg = np.round(r.uniform(-2, 2, size=130) * 4.0).astype(np.float32) / np.float32(4.0)       # 17 distinct values: many ties
    lg[5] = np.nan
    p[5] = gt[0]                                     # the perfect proposal carries the NaN: it only survives "no limit"
    rng = np.full(6, 0xFF, dtype=np.uint8)
    return gt, rng, p, lg


def seeded_image(seed, P, G, num_bits=8):
    """one image of P proposals and G boxes with random range bits -> (gt f32, bits u8, boxes f32, logits f32)"""
    r = np.random.RandomState(seed)
    gt = _gt_boxes(r, G).astype(np.float32)
    bits = r.randint(0, 1 << num_bits, size=G).astype(np.uint8)
    return gt, bits, _proposals(r, gt, P), _logits(r, P)
