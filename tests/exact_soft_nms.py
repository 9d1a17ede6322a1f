"""References and case builders for cddmsl_soft_nms (cddmsl_amd/csrc/soft_nms.hip), imported by tests/test_soft_nms_ref_host.py and
tests/test_gpu_soft_nms.py; not a conftest; numpy only.

``soft_nms_ref`` restates the reference's walk (layers/soft_nms.py:186-261) as a plain loop over picks, every f32 operation on
``np.float32`` values in the reference's order (the IoU is exact_boxes.iou_match32, pairwise_iou's form), ``batched_soft_nms_ref``
adds the coordinate shift of layers/soft_nms.py:127-129 on top -- ONE walk over all categories, as the reference does it.
``per_category_ref`` is the kernel's factorisation (a capped walk per category, then one stable descending merge); the host tests
show that it equals the first ``max_keep`` entries of the single walk on every case.

Linear and hard decays contain no transcendental: keep lists and scores are defined bit for bit.  The gaussian decay is
exp(-(iou*iou)/sigma): its ARGUMENT is f32 arithmetic (bit for bit), exp is evaluated here in float64 on that f32 argument and
rounded once to f32.  A kernel's expf may differ from it by EXPF_ULP ulps (exact_boxes.EXPF_ULP), so a gaussian score carries a
running first-order bound, built like the one exact_boxes.decode_ref derives: per non-trivial decay (argument != 0) the relative
difference between the kernel's score and this one grows by
    EXPF_ULP * 2U   the kernel's expf against the real exponential (an ulp of y is at most 2U |y|)
  + U               this reference's single rounding of the float64 exponential
  + 2U              the rounding of the product score * decay, once on either side
and ``bound = 2 * (number of non-trivial decays) * DECAY_CHARGE * U * |score|`` (the factor 2 covers the dropped second-order terms).
A decay with a zero argument is exactly 1 on both sides (expf(-0) == 1) and charges nothing.  Every decision of a gaussian case --
the arg-max winner against every other live score, every decayed score against ``prune`` -- must lie at least MARGIN bounds away
from flipping (``margin`` in the result; the host tests assert it for every gaussian case), so the keep list is the same for any
expf within its documented error."""
import functools

import numpy as np

import exact_boxes as E

F32 = np.float32
U = E.U
DECAY_CHARGE = 2.0 * E.EXPF_ULP + 3.0
MARGIN = 4.0
METHODS = {"gaussian": 0, "linear": 1, "hard": 2}

# structure constants of the kernel the size cases are built around (cddmsl_amd/csrc/soft_nms.hip)
WAVE = 64            # lanes of a wave: 63 / 64 / 65 candidates straddle the first wave's edge
BLOCK = 256          # threads of a walk workgroup: from 257 candidates on a thread holds a second candidate
LDS_CAP = 2048       # candidates of one category held in LDS; 2049 takes the scratch-buffer walk
GRID = 1024          # walk workgroups launched at most: more categories than that and a workgroup walks a second segment
TOTAL_CAP = 32768    # candidates per call; one more is refused


def _decay(iou, method, sigma, thr):
    if method == "linear":
        return np.where(iou > F32(thr), F32(1) - iou, F32(1)).astype(F32)
    if method == "hard":
        return (iou < F32(thr)).astype(F32)
    if method == "gaussian":
        arg = -(iou * iou) / F32(sigma)
        assert arg.dtype == np.float32
        return np.exp(arg.astype(np.float64)).astype(F32)
    raise NotImplementedError("{} soft nms method not implemented.".format(method))


def soft_nms_ref(boxes, scores, method, sigma, thr, prune, max_keep=-1, variant=None, dead=None):
    """-> dict(keep int64 [n], scores f32 [n], bound f64 [n], margin float).  ``variant`` selects a NEGATIVE CONTROL (never a
    reference): "sort_once" walks in the initial score order, "tie_high" breaks ties by the highest index, "prune_ge" lets a score
    equal to ``prune`` survive.  ``dead``: candidates that are gone before the first pick (per_category_ref)."""
    b, s = E.f32a(boxes).reshape(-1, 4), E.f32a(scores).copy()
    n = len(s)
    alive = np.ones(n, bool) if dead is None else ~np.asarray(dead, bool)
    ndec = np.zeros(n, np.int64)
    keep, out, bnd = [], [], []
    margin = np.inf
    once = np.argsort(-s.astype(np.float64), kind="stable") if variant == "sort_once" else None
    bound = lambda i: 2.0 * ndec[i] * DECAY_CHARGE * U * np.abs(s[i].astype(np.float64))
    while alive.any() and (max_keep < 0 or len(keep) < max_keep):
        live = np.nonzero(alive)[0]
        if variant == "sort_once":
            top = int(next(i for i in once if alive[i]))
        elif variant == "tie_high":
            top = int(live[len(live) - 1 - np.argmax(s[live][::-1])])
        else:
            top = int(live[np.argmax(s[live])])                      # the first of equal maxima: the lowest index
        alive[top] = False
        rest = np.nonzero(alive)[0]
        if variant is None and len(rest):
            gap = s[top].astype(np.float64) - s[rest].astype(np.float64)
            den = bound(top) + bound(rest)
            assert (gap >= 0).all()
            if (den > 0).any():
                margin = min(margin, float((gap[den > 0] / den[den > 0]).min()))
        keep.append(top); out.append(s[top]); bnd.append(float(bound(top)))
        if not len(rest):
            break
        iou = E.iou_match32(b[top], b[rest])
        d = _decay(iou, method, sigma, thr)
        s[rest] = s[rest] * d
        if method == "gaussian":
            ndec[rest] += iou != 0
        surv = (s[rest] >= F32(prune)) if variant == "prune_ge" else (s[rest] > F32(prune))
        if variant is None:
            bb = bound(rest)
            if (bb > 0).any():
                margin = min(margin, float((np.abs(s[rest].astype(np.float64) - float(F32(prune)))[bb > 0] / bb[bb > 0]).min()))
        alive[rest[~surv]] = False
    return dict(keep=np.asarray(keep, np.int64), scores=np.asarray(out, F32), bound=np.asarray(bnd, np.float64), margin=margin)


def shifted(boxes, idxs):
    """layers/soft_nms.py:127-129 in f32: offsets = idxs.to(f32) * (boxes.max() + 1), one rounded addition per coordinate"""
    b = E.f32a(boxes).reshape(-1, 4)
    off = np.asarray(idxs).astype(F32) * (b.max() + F32(1))
    out = b + off[:, None]
    assert out.dtype == np.float32
    return out


def batched_soft_nms_ref(boxes, scores, idxs, method, sigma, thr, prune, max_keep=-1, variant=None):
    """the reference's batched_soft_nms followed by fast_rcnn.py:198-199's cut ``keep[:max_keep]``; variant "no_shift" is the
    negative control that walks each category on the raw coordinates"""
    if len(scores) == 0:
        return dict(keep=np.zeros(0, np.int64), scores=np.zeros(0, F32), bound=np.zeros(0), margin=np.inf)
    if variant == "no_shift":
        r = per_category_ref(boxes, scores, idxs, method, sigma, thr, prune, -1, shift=False)
    elif variant == "no_arrival_prune":
        r = per_category_ref(boxes, scores, idxs, method, sigma, thr, prune, -1, arrival_prune=False)
    else:
        r = soft_nms_ref(shifted(boxes, idxs), scores, method, sigma, thr, prune, -1, variant)
    if max_keep >= 0:
        r = dict(r, keep=r["keep"][:max_keep], scores=r["scores"][:max_keep], bound=r["bound"][:max_keep])
    return r


def per_category_ref(boxes, scores, idxs, method, sigma, thr, prune, max_keep=-1, shift=True, arrival_prune=True):
    """the kernel's factorisation: a walk per category stopped after max_keep picks, the union ordered by (rescored score
    descending, input index ascending), cut at max_keep.  The single walk tests every remaining score against prune after every
    pick, its first included: outside the category of that first pick (the global arg-max, lowest index) the decay is exactly 1,
    so a candidate that starts at or below prune is gone before its own category picks (``arrival_prune``; without it: the
    negative control "no_arrival_prune")."""
    idxs = np.asarray(idxs, np.int64)
    b = shifted(boxes, idxs) if shift else E.f32a(boxes).reshape(-1, 4)
    s = E.f32a(scores)
    dense = np.full(len(s), -np.inf, np.float64)
    first_cat = idxs[int(np.argmax(s))]
    for c in np.unique(idxs):
        sel = np.nonzero(idxs == c)[0]
        dead = ~(s[sel] > F32(prune)) if (arrival_prune and c != first_cat) else None
        r = soft_nms_ref(b[sel], s[sel], method, sigma, thr, prune, max_keep, dead=dead)
        dense[sel[r["keep"]]] = r["scores"]
    order = np.argsort(-dense, kind="stable")
    order = order[dense[order] > -np.inf]
    if max_keep >= 0:
        order = order[:max_keep]
    return dict(keep=order.astype(np.int64), scores=dense[order].astype(F32), bound=np.zeros(len(order)), margin=np.inf)


# =============================================================================================================== cases
def clustered(n, cats, seed, ngt=6, jitter=8.0, origin=(0.0, 0.0)):
    """n jittered copies of ngt ground-truth boxes in a 640 x 480 image, scores in (0.05, 1), categories drawn from ``cats``"""
    r = np.random.RandomState(seed)
    x0, y0 = r.uniform(0, 440, ngt), r.uniform(0, 280, ngt)
    gt = np.stack([x0, y0, x0 + r.uniform(40, 200, ngt), y0 + r.uniform(40, 200, ngt)], 1)
    b = gt[r.randint(ngt, size=n)] + r.normal(0, jitter, (n, 4)) + np.asarray(origin * 2)[None]
    b = np.maximum(b, 0.0)
    scores = r.uniform(0.05, 1.0, n)
    idxs = np.asarray(cats, np.int64)[r.randint(len(cats), size=n)]
    return E.f32a(b), E.f32a(scores), idxs


def _c(name, data, method, max_keep=-1, sigma=0.5, thr=0.5, prune=0.001, controls=()):
    b, s, i = data
    return dict(name=name, boxes=E.f32a(b).reshape(-1, 4), scores=E.f32a(s), idxs=np.asarray(i, np.int64), method=method, sigma=sigma,
                thr=thr, prune=prune, max_keep=max_keep, controls=tuple(controls))


SHIFT_SEED = 0          # a seed of the far-corner case on which the unshifted walk differs (asserted by the host tests)
GAUSS_SEEDS = (0, 1)    # seeds of the clustered gaussian cases: every decision >= MARGIN bounds from flipping (asserted likewise)


def _grid_boxes(n, side=10.0, pitch=12.0, per_row=16):
    i = np.arange(n)
    x, y = (i % per_row) * pitch, (i // per_row) * pitch
    return np.stack([x, y, x + side, y + side], 1)


@functools.lru_cache(maxsize=None)
def cases():
    out = []
    one = lambda n, seed, c=4: clustered(n, [c], seed)
    # ---- sizes: one category at the wave edge, the thread edge and the LDS edge; K = 1
    out.append(_c("k1", ([[1.0, 2.0, 30.0, 40.0]], [0.3], [7]), "linear"))
    for n in (WAVE - 1, WAVE, WAVE + 1, BLOCK - 1, BLOCK, BLOCK + 1):
        out.append(_c(f"one_cat_{n}_linear", one(n, 100 + n), "linear", thr=0.3))
    out.append(_c(f"one_cat_{WAVE + 1}_gaussian", one(WAVE + 1, 201), "gaussian"))
    out.append(_c(f"one_cat_{BLOCK + 1}_gaussian", one(BLOCK + 1, 202), "gaussian"))
    out.append(_c(f"one_cat_{LDS_CAP}_linear", one(LDS_CAP, 203), "linear", thr=0.3, prune=0.02))
    out.append(_c(f"one_cat_{LDS_CAP + 1}_linear", one(LDS_CAP + 1, 204), "linear", thr=0.3, prune=0.02))
    out.append(_c(f"one_cat_{LDS_CAP + 1}_hard", one(LDS_CAP + 1, 205), "hard"))
    out.append(_c(f"lds_and_scratch_segments", clustered(LDS_CAP + 700, [2, 11], 206, ngt=3) , "hard", thr=0.4))
    out.append(_c(f"total_cap_{TOTAL_CAP}_hard", clustered(TOTAL_CAP, [1, 5, 6], 207, ngt=4), "hard", thr=0.3))
    # ---- categories
    r = np.random.RandomState(208)
    b, s, _ = clustered(GRID + 6, [0], 208)
    out.append(_c(f"singleton_categories_{GRID + 6}", (b, s, r.permutation(GRID + 6) * 3 - 40), "linear", thr=0.3))
    for m in METHODS:
        out.append(_c(f"unsorted_ids_{m}", clustered(300, [3, 79, 7], 210), m))
    b, s, _ = clustered(201, [0], 211)
    out.append(_c("single_between_two_large", (b, s, [5] * 100 + [9] * 50 + [6] + [9] * 50), "linear", thr=0.3))
    # ---- ties
    b, s, i = clustered(120, [2, 3, 4], 212)
    s = np.random.RandomState(213).choice(np.asarray([0.9, 0.5, 0.25], np.float32), 120)
    out.append(_c("tied_scores_linear", (b, s, i), "linear", thr=0.3, controls=("tie_high",)))      # decays of exactly 1 keep the ties
    out.append(_c("tied_scores_hard", (b, s, i), "hard", controls=("tie_high",)))
    out.append(_c("tied_nonoverlapping_gaussian", (_grid_boxes(70), s[:70], i[:70]), "gaussian", controls=("tie_high",)))
    # ---- strict comparisons.  IoU([0,0,2,1], [0,0,1,1]) == 0.5 exactly: linear leaves the score (iou > thr is false), hard
    # suppresses it (iou < thr is false).  torchvision's hard NMS (iou > thr suppresses) would KEEP it: the two forms differ here.
    pair = ([[0, 0, 2, 1], [0, 0, 1, 1]], [0.9, 0.8], [0, 0])
    out.append(_c("iou_equals_thr_linear", pair, "linear", thr=0.5))
    out.append(_c("iou_equals_thr_hard", pair, "hard", thr=0.5))
    pb = E.f32a([[0, 0, 10, 10], [0, 0, 10, 7]])                                      # IoU 0.7 (rounded), decay 1 - iou
    prod = F32(0.8) * (F32(1) - E.iou_match32(pb[0], pb[1:])[0])
    out.append(_c("decayed_equals_prune", (pb, [0.9, 0.8], [1, 1]), "linear", thr=0.3, prune=float(prod), controls=("prune_ge",)))
    out.append(_c("decayed_one_step_above_prune", (pb, [0.9, 0.8], [1, 1]), "linear", thr=0.3, prune=float(np.nextafter(prod, F32(0)))))
    # ---- scores that START at or below prune: the single walk drops them after its first pick whatever their category, unless
    # they are that pick (or share its category, where the decay decides).  (a) a category whose top score is <= prune, (b) every
    # score <= prune in several categories: only the global top is kept, (c) prune above every score: the global top is picked
    # before any comparison with prune and is the only pick, plus a clustered case with a fifth of the scores below prune
    low = ([[0, 0, 10, 10], [0, 0, 10, 10], [20, 20, 30, 30]], [0.9, 0.0005, 0.0004], [0, 1, 1])
    for m in METHODS:
        out.append(_c(f"category_top_below_prune_{m}", low, m, controls=("no_arrival_prune",)))
    out.append(_c("all_below_prune", (_grid_boxes(9), [0.0003, 0.0009, 0.0009, 0.0002, 0.0009, 0.0001, 0.0005, 0.0009, 0.0004],
                                      [4, 2, 7, 4, 2, 7, 9, 7, 2]), "linear", controls=("no_arrival_prune",)))
    out.append(_c("below_prune_is_global_top", ([[0, 0, 10, 10], [0, 0, 10, 9], [40, 40, 50, 50], [40, 40, 50, 49]], [0.4, 0.3, 0.35, 0.2],
                                                [0, 0, 1, 1]), "linear", prune=0.45, controls=("no_arrival_prune",)))
    b, s, i = clustered(300, [0, 1, 2, 3, 4], 214)
    s = np.where(np.random.RandomState(215).rand(300) < 0.2, s * F32(0.02), s)          # a fifth of the scores in (0.001, 0.02)
    for m in METHODS:
        out.append(_c(f"clustered300_low_scores_{m}", (b, s, i), m, prune=0.01))
    # ---- re-ranking: B (0.8) overlaps A (0.9) and falls below C (0.5): picks A, C, B -- a walk that sorts once says A, B, C
    out.append(_c("rerank", ([[0, 0, 10, 10], [0, 1, 10, 10], [50, 50, 60, 60]], [0.9, 0.8, 0.5], [2, 2, 2]), "linear", thr=0.3,
                  controls=("sort_once",)))
    out.append(_c("rerank_gaussian", ([[0, 0, 10, 10], [0, 1, 10, 10], [50, 50, 60, 60]], [0.9, 0.8, 0.5], [2, 2, 2]), "gaussian",
                  controls=("sort_once",)))
    # ---- shift: fractional coordinates near the far corner in a high category -- the IoU on shifted coordinates is another number
    out.append(_c("shift_far_corner", clustered(80, [19], SHIFT_SEED, ngt=3, origin=(500.0, 480.0)), "linear", thr=0.3, controls=("no_shift",)))
    # ---- seeded clustered cases, all methods
    for seed in GAUSS_SEEDS:
        for m in METHODS:
            out.append(_c(f"clustered300_s{seed}_{m}", clustered(300, [0, 1, 2, 3, 4], 300 + seed), m))
    # ---- max_keep: -1 (above), 1, exactly the pick count, one below it
    base = clustered(300, [0, 1, 2, 3, 4], 300)
    npick = len(batched_soft_nms_ref(*base, "linear", 0.5, 0.5, 0.001)["keep"])
    for mk in (0, 1, 7, npick - 1, npick, npick + 5):
        out.append(_c(f"max_keep_{mk}", base, "linear", max_keep=mk))
    out.append(_c("max_keep_7_gaussian", base, "gaussian", max_keep=7))
    names = [c["name"] for c in out]
    assert len(set(names)) == len(names)
    return tuple(out)


def case(name):
    return next(c for c in cases() if c["name"] == name)


@functools.lru_cache(maxsize=None)
def expected(name):
    """the reference result of a case, computed once and shared (do not modify)"""
    c = case(name)
    return batched_soft_nms_ref(c["boxes"], c["scores"], c["idxs"], c["method"], c["sigma"], c["thr"], c["prune"], c["max_keep"])


def control(name, variant):
    c = case(name)
    return batched_soft_nms_ref(c["boxes"], c["scores"], c["idxs"], c["method"], c["sigma"], c["thr"], c["prune"], c["max_keep"], variant)


def same(a, b):
    return np.array_equal(a["keep"], b["keep"]) and np.array_equal(a["scores"], b["scores"])


# =============================================================================================================== inference
INFER_SEED = 410       # chosen like GAUSS_SEEDS: both gaussian configurations keep every decision >= MARGIN bounds from flipping


@functools.lru_cache(maxsize=None)
def inference_inputs(seed=None):
    """a seeded head output for fast_rcnn_inference_single_image: class-specific boxes [R, 4C] (some outside the image, so the clip
    acts), probabilities [R, C + 1], one row with a NaN box and one with an infinite score"""
    R, C = 60, 5
    seed = INFER_SEED if seed is None else seed
    r = np.random.RandomState(seed)
    b = np.concatenate([clustered(R, [0], seed + 1 + k, ngt=4, jitter=10.0, origin=(-20.0, -15.0))[0] for k in range(C)], 1)
    b = b + np.tile(np.asarray([0.0, 0.0, 60.0, 40.0], np.float32), C)[None]
    logits = r.normal(0, 1.5, (R, C + 1))
    p = np.exp(logits) / np.exp(logits).sum(1, keepdims=True)
    b[7, 5], p[20, 2] = np.nan, np.inf
    return dict(boxes=E.f32a(b), scores=E.f32a(p), image_shape=(480, 640), score_thresh=0.05)


def inference_configs():
    return {"linear_top100": dict(method="linear", sigma=0.5, prune=0.001, nms_thresh=0.5, topk=100),
            "linear_top10": dict(method="linear", sigma=0.5, prune=0.001, nms_thresh=0.5, topk=10),
            "hard_all": dict(method="hard", sigma=0.5, prune=0.001, nms_thresh=0.5, topk=-1),
            "gaussian_top100": dict(method="gaussian", sigma=0.5, prune=0.001, nms_thresh=0.5, topk=100),
            "gaussian_top10": dict(method="gaussian", sigma=0.5, prune=0.01, nms_thresh=0.5, topk=10)}


def inference_candidates(boxes, scores, image_shape, score_thresh):
    """fast_rcnn.py:155-180: drop non-finite rows, clip, threshold per (proposal, class) in row-major order
    -> (boxes [n, 4], scores [n], proposal index among the finite rows [n], class [n], finite rows)"""
    valid = np.isfinite(boxes).all(1) & np.isfinite(scores).all(1)
    rows = np.nonzero(valid)[0]
    b, s = boxes[valid], scores[valid][:, :-1]
    C = b.shape[1] // 4
    h, w = image_shape
    b = b.reshape(-1, C, 4).copy()
    b[..., 0::2] = np.minimum(np.maximum(b[..., 0::2], F32(0)), F32(w))
    b[..., 1::2] = np.minimum(np.maximum(b[..., 1::2], F32(0)), F32(h))
    pi, ci = np.nonzero(s > F32(score_thresh))
    return b[pi, ci if C > 1 else 0], s[pi, ci], pi, ci, rows


def inference_ref(inp, cfg):
    """fast_rcnn.py:182-209 with soft_nms_enabled: the kept detections carry the rescored scores, the cut follows the pick order
    -> dict(pred_boxes, scores, bound, pred_classes, kept (finite-row numbering), kept_rows (input rows), margin)"""
    b, s, pi, ci, rows = inference_candidates(inp["boxes"], inp["scores"], inp["image_shape"], inp["score_thresh"])
    r = batched_soft_nms_ref(b, s, ci, cfg["method"], cfg["sigma"], cfg["nms_thresh"], cfg["prune"], cfg["topk"])
    k = r["keep"]
    return dict(pred_boxes=b[k], scores=r["scores"], bound=r["bound"], pred_classes=ci[k], kept=pi[k], kept_rows=rows[pi[k]], margin=r["margin"],
                candidates=(b, s, ci))
