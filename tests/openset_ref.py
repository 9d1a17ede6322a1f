"""Float64 references, seeded cases and the error model of the open-vocabulary pair (cddmsl_amd/csrc/openset.hip):
``cddmsl_openset_logits`` and ``cddmsl_openset_select``.  tests/test_openset_host.py ties the references to the fixture recorded
from the reference's own FastRCNNOutputLayers (tests/golden/ref_openset.npz) and asserts the condition on the inputs below;
tests/test_gpu_openset.py compares the kernels against them.

Error model (u = 2^-24, first order; every constant is a count of roundings in the kernel's documented arithmetic order)

  logit.  The kernel forms iv = 1 / max(sqrt(ss), eps) with ss the f32 sum of the D squares in lane-strided order (ceil(D / 64)
  additions per lane, 6 reduction steps, one rounded product per term: every term passes through at most ceil(D/64) + 7 roundings,
  all terms are positive, so ss is relatively exact to (ceil(D/64) + 7) u); the square root halves that and adds 1 ulp = 2 u, the
  division adds u.  iv is a common factor of the row, so its error scales the dot product: c2 u |dot| with
  c2 = (ceil(D/64) + 7) / 2 + 3, plus one rounding of 1/T and one of the final multiply: C2(D) = (ceil(D/64) + 7) / 2 + 5.
  Each x_hat element is one rounded multiply (1 rounding), each product enters the MFMA accumulator (at most 1 rounding if the
  product is rounded at all) and then passes through at most D accumulator additions: (D + 2) u per unit of |x_hat_d wn_d|; C1 = 3
  leaves one u for the second-order terms (D u << 1).  So
      |logit - ref| <= ((D + C1) u * sum_d |x_hat_d wn_d| + C2(D) u |dot|) / T
  with the per-entry sum of absolute products evaluated in float64.  The reference takes wn as given (f32 values) and T, eps as
  the f32 numbers the C ABI receives.  The background logit is exactly 0.

  statistics.  m = max of the K+1 logits: |m - ref| <= E = the row's largest logit bound (max is 1-Lipschitz).  Each term of l is
  expf(fl(z_c - m)): its argument is off by e_c + E + u |z_c - m|, expf adds 1 ulp = 2 u, so the term is relatively off by
  t_c = expm1(e_c + E + u |a_c|) + 2 u; l is their f32 sum in lane-strided order (ceil((K+1)/64) + 6 roundings per term, all
  positive): rel(l) <= sum_c p_c t_c + (ceil((K+1)/64) + 6) u -- the probability-weighted mean of the terms' errors.

  score.  p_c = fl(expf(fl(z_c - m)) / l).  The device's m is one number in numerator and denominator, so its error E cancels in the
  quotient: with t'_c = expm1(e_c + u |a_c|) + 2 u, rel(p_c) <= t'_c + sum_j p_j t'_j + (ceil((K+1)/64) + 6) u + 2 u (the division is
  allowed 1 ulp).  With the objectness,
  q = fl(p o) adds u and s = sqrtf(q) halves the total and adds 1 ulp.  Below the normal range the f32 result is either flushed or a
  denormal: a value whose upper bound lies below 2^-125 is given the interval [0, upper + 2^-149], and one below 2^-150 is exactly
  0 either way.  ``score_interval`` returns [lo, hi] for every entry; an entry is AMBIGUOUS for a threshold when lo <= thresh < hi,
  certainly selected when lo > thresh and certainly not when hi <= thresh.

Condition on the inputs: every case of ``SHAPES`` has an empty ambiguous set for every configuration it is used in (asserted on the
CPU by the host test), so the GPU tests demand the exact candidate list.  The seeds below are the first of ``range(SEED_SEARCH)``
with that property (``first_seed``; the host test re-derives them).  The large case is the one exception.
"""
import math

import numpy as np

U = 2.0 ** -24
C1 = 3
T_DEFAULT = 0.01
EPS = 1e-12
SEED_SEARCH = 64
# (threshold, temperature): at T = 0.01 the logits span 200 and the smallest probabilities lie in or below the f32 denormal range,
# where "p > 0" depends on how the device rounds there; the threshold-0 configuration therefore runs at T = 0.05 (every probability
# is a normal number, every class of a valid row is selected) and ``underflow_case`` covers the exactly-zero probability
THRESHOLDS = ((0.05, 0.01), (0.001, 0.01), (0.0, 0.05))
IMG_H, IMG_W = 120, 160


def c2(D):
    return (math.ceil(D / 64) + 7) / 2 + 5


# ------------------------------------------------------------------------------------------------------------- references
def ref_logits(x, wn, T=T_DEFAULT, eps=EPS):
    """x [R, D] f32, wn [K, D] f32 -> (z [R, K+1] f64 with z[:, K] = 0, bound [R, K+1] f64)"""
    x64, w64 = x.astype(np.float64), wn.astype(np.float64)
    T32, eps32 = float(np.float32(T)), float(np.float32(eps))
    D = x.shape[1]
    nrm = np.sqrt((x64 * x64).sum(axis=1, keepdims=True))
    xh = x64 / np.maximum(nrm, eps32)
    dot = xh @ w64.T
    sabs = np.abs(xh) @ np.abs(w64).T
    z = np.concatenate([dot / T32, np.zeros((x.shape[0], 1))], axis=1)
    bound = np.concatenate([((D + C1) * U * sabs + c2(D) * U * np.abs(dot)) / T32, np.zeros((x.shape[0], 1))], axis=1)
    return z, bound


def ref_stats(z):
    m = z.max(axis=1)
    return m, np.exp(z - m[:, None]).sum(axis=1)


def stats_bounds(z, bound):
    """-> (|m - ref| bound [R], relative bound of l [R], relative bound of every p [R, K+1])"""
    m, l = ref_stats(z)
    E = bound.max(axis=1)
    a = z - m[:, None]
    t = np.expm1(bound + E[:, None] + U * np.abs(a)) + 2 * U
    p = np.exp(a) / l[:, None]
    depth = (math.ceil(z.shape[1] / 64) + 6) * U
    rel_l = (p * t).sum(axis=1) + depth
    tp = np.expm1(bound + U * np.abs(a)) + 2 * U          # m is the same number in p's numerator and denominator: E cancels
    return E, rel_l, tp + (p * tp).sum(axis=1, keepdims=True) + depth + 2 * U


def score_interval(z, bound, obj=None):
    """-> (s [R, K+1] f64 reference scores, lo, hi); rows whose reference score is not finite keep NaN"""
    m, l = ref_stats(z)
    _, _, rel_p = stats_bounds(z, bound)
    p = np.exp(z - m[:, None]) / l[:, None]

    def sub(lo, hi):       # below the normal range: flushed or denormal
        small, zero = hi < 2.0 ** -125, hi < 2.0 ** -150
        lo = np.where(small, 0.0, lo)
        return lo, np.where(zero, 0.0, np.where(small, hi + 2.0 ** -149, hi))

    lo, hi = sub(p * (1 - rel_p), p * (1 + rel_p))
    if obj is None:
        return p, lo, hi
    o = obj.astype(np.float64)[:, None]
    with np.errstate(invalid="ignore"):
        s = np.sqrt(p * o)
        qlo, qhi = sub(lo * o * (1 - U), hi * o * (1 + U))
        return s, np.sqrt(qlo) * (1 - 2 * U), np.sqrt(qhi) * (1 + 2 * U)


def ref_select(z, bound, boxes, obj, thresh, img_h=IMG_H, img_w=IMG_W):
    """fast_rcnn_inference_single_image:155-180 in float64 on the reference logits -> dict(valid [R] bool, rows, cls (row-major
    order), scores f64, lo, hi (the f32 result's interval), boxes f32 [n, 4] clipped, ambiguous [m, 2] (row, class) entries that may
    or may not be selected)"""
    R, K = z.shape[0], z.shape[1] - 1
    th = float(np.float32(thresh))
    s, lo, hi = score_interval(z, bound, obj)
    valid = np.isfinite(boxes).all(axis=1) & np.isfinite(s).all(axis=1)
    sel = (lo[:, :K] > th) & valid[:, None]          # certainly selected: with an empty ambiguous set, exactly the f32 selection
    amb = (lo[:, :K] <= th) & (th < hi[:, :K]) & valid[:, None]
    rows, cls = np.nonzero(sel)
    ldb = boxes.shape[1]
    b = boxes[rows] if ldb == 4 else boxes.reshape(R, K, 4)[rows, cls]
    b = b.astype(np.float32).copy()
    b[:, 0::2] = np.clip(b[:, 0::2], np.float32(0), np.float32(img_w))
    b[:, 1::2] = np.clip(b[:, 1::2], np.float32(0), np.float32(img_h))
    return dict(valid=valid, rows=rows.astype(np.int64), cls=cls.astype(np.int64), scores=s[rows, cls], lo=lo[rows, cls], hi=hi[rows, cls],
                boxes=b.reshape(-1, 4), ambiguous=np.argwhere(amb))


# ------------------------------------------------------------------------------------------------------------------ cases
def make_inputs(seed, R, K, D, ldb4k=False, spread=0.15, orthonormal=False):
    """clustered region features: every row is a mixture of three unit class embeddings with nearly equal weights plus a little
    noise, so that at T = 0.01 several classes of a row hold comparable probabilities and the thresholds cut through them; boxes that
    stick out of the image on every side; objectness in [0.05, 1].  ``orthonormal`` (K <= D): class embeddings without
    cross-correlation, so no row is dominated by one class and the scores do not crowd at 1"""
    g = np.random.default_rng(seed)
    wn = g.standard_normal((K, D))
    if orthonormal:
        wn = np.linalg.qr(wn.T)[0].T
    wn = (wn / np.linalg.norm(wn, axis=1, keepdims=True)).astype(np.float32)
    own = np.argsort(g.random((R, K)), axis=1)[:, np.arange(3) % K]        # three different classes per row (K >= 3)
    mix = np.concatenate([np.ones((R, 1)), 1.0 - g.uniform(0, 0.08, size=(R, 2))], axis=1)
    x = ((mix[:, :, None] * wn[own]).sum(axis=1) + spread * g.standard_normal((R, D)) / math.sqrt(D)).astype(np.float32) * np.float32(3.0)
    nb = K if ldb4k else 1
    x0 = g.uniform(-20, IMG_W - 10, size=(R, nb))
    y0 = g.uniform(-20, IMG_H - 10, size=(R, nb))
    bw, bh = g.uniform(4, 90, size=(R, nb)), g.uniform(4, 90, size=(R, nb))
    boxes = np.stack([x0, y0, x0 + bw, y0 + bh], axis=2).reshape(R, 4 * nb).astype(np.float32)
    obj = g.uniform(0.05, 1.0, size=R).astype(np.float32)
    return dict(x=x, wn=wn, boxes=boxes, obj=obj)


# name -> (R, K, D, class-specific boxes); the shapes sit below, at and above the kernels' tile extents: 32 rows per panel, 32 classes
# per wave, 128 per workgroup, 64 logits (K+1!) per pass of the statistics / selection waves, 8 elements of D per MFMA step
SHAPES = {
    "r1_k1_d4": (1, 1, 4, False), "r31_k31_d8": (31, 31, 8, True), "r32_k32_d64": (32, 32, 64, False), "r33_k33_d12": (33, 33, 12, True),
    "r70_k37_d64": (70, 37, 64, False), "r70_k63_d8": (70, 63, 8, False), "r70_k64_d64": (70, 64, 64, True),
    "r32_k127_d64": (32, 127, 64, False), "r33_k128_d64": (33, 128, 64, True), "r31_k129_d64": (31, 129, 64, False),
    "r70_k130_d64": (70, 130, 64, True), "r33_k257_d64": (33, 257, 64, False),
}
# the first seed of range(SEED_SEARCH) whose ambiguous set is empty for every threshold, with and without objectness (first_seed)
SEEDS = {n: 0 for n in SHAPES}
LARGE = dict(R=300, K=1203, D=1024, seed=0, thresh=0.05)


# the case behind tests/golden/ref_openset.npz and the open-set / closed-set comparison: the detections are ORDERED by score, so on
# top of an empty ambiguous set no two candidates' score intervals may overlap (``order_overlaps``) -- with and without objectness
FIXTURE = dict(R=70, K=37, D=64, seed=0, thresh=0.05, nms=0.5, topk=100)


def fixture_inputs(seed=None):
    """Designed, not drawn: orthonormal class embeddings and every row a unit mixture of two of them whose logit gap puts the larger
    probability on a jittered grid over (0.5, 0.95) -- the smaller one on its mirror image over (0.05, 0.5) -- with the objectness
    rising along the same grid (slowly enough that the smaller class's product still falls), rows shuffled.  All ~140 scores above the threshold are then spaced by more than their error
    intervals, which random draws of that many scores in (0.05, 1) cannot be."""
    f = FIXTURE
    R, K, D = f["R"], f["K"], f["D"]
    g = np.random.default_rng(f["seed"] if seed is None else seed)
    inp = make_inputs(int(g.integers(1 << 30)), R, K, D, False, orthonormal=True)
    t = (g.permutation(R) + 0.5 + g.uniform(-0.2, 0.2, size=R)) / R
    ptop = 0.5 + 0.45 * t
    gap = np.log(ptop / (1 - ptop)) * float(np.float32(T_DEFAULT))           # cos_1 - cos_2
    theta = np.arccos(gap / math.sqrt(2.0)) - math.pi / 4
    own = np.argsort(g.random((R, K)), axis=1)[:, :2]
    w = inp["wn"].astype(np.float64)
    inp["x"] = (3.0 * (np.cos(theta)[:, None] * w[own[:, 0]] + np.sin(theta)[:, None] * w[own[:, 1]])).astype(np.float32)
    # o(t) = 0.5 e^(0.6 t): p_top o rises and (1 - p_top) o falls along the grid, both fast enough to keep sqrt(p o) spaced
    inp["obj"] = (0.5 * np.exp(0.6 * t)).astype(np.float32)
    return inp


def order_overlaps(sel, head=None):
    """pairs of candidates, neighbours in descending-score order, whose f32 scores could sort either way; ``head``: among the
    highest ``head`` candidates and the one behind them only"""
    o = np.argsort(-sel["scores"], kind="stable")[:None if head is None else head + 1]
    return int((sel["hi"][o][1:] >= sel["lo"][o][:-1]).sum())


def fixture_condition(inp):
    """the fixture's inputs are unambiguous: no score at the threshold and a strict f32 order among ALL candidates (so the kept
    list, its order and the top-k cut are the same for every implementation inside the error model) -- with and without the
    objectness product; more candidates than the top-k keeps, two per row"""
    f = FIXTURE
    z, bound = ref_logits(inp["x"], inp["wn"])
    for ob in (None, inp["obj"]):
        sel = ref_select(z, bound, inp["boxes"], ob, f["thresh"])
        if len(sel["ambiguous"]) or order_overlaps(sel) or len(sel["rows"]) <= f["topk"]:
            return False
    return True


def fixture_first_seed():
    for seed in range(SEED_SEARCH):
        if fixture_condition(fixture_inputs(seed)):
            return seed
    raise AssertionError("no fixture seed")


def configs():
    return [(th, T, ob) for th, T in THRESHOLDS for ob in (False, True)]


def ambiguous_count(inp):
    n = 0
    for th, T, ob in configs():
        z, bound = ref_logits(inp["x"], inp["wn"], T)
        n += len(ref_select(z, bound, inp["boxes"], inp["obj"] if ob else None, th)["ambiguous"])
    return n


def underflow_case():
    """T = 0.01, two opposite classes: z = (100, -100, 0), so p_1 = e^-200 / l is 0 in f32 however the device treats denormals --
    not selected at threshold 0 -- while p_0 is"""
    wn = np.asarray([[1, 0, 0, 0], [-1, 0, 0, 0]], np.float32)
    x = np.asarray([[2, 0, 0, 0], [0, 0, 0, -3]], np.float32)
    boxes = np.asarray([[1, 2, 30, 40], [5, 6, 70, 80]], np.float32)
    return dict(x=x, wn=wn, boxes=boxes, obj=np.asarray([0.5, 0.25], np.float32))


def first_seed(name):
    R, K, D, spec = SHAPES[name]
    for seed in range(SEED_SEARCH):
        if ambiguous_count(make_inputs(seed, R, K, D, spec)) == 0:
            return seed
    raise AssertionError(f"{name}: no seed below {SEED_SEARCH} has an empty ambiguous set")


_CACHE = {}


def case(name):
    """inputs, float64 logits and bounds of a named case (computed once, shared and never modified)"""
    if name not in _CACHE:
        if name == "large":
            inp = make_inputs(LARGE["seed"], LARGE["R"], LARGE["K"], LARGE["D"], False)
        elif name == "fixture":
            inp = fixture_inputs()
        else:
            R, K, D, spec = SHAPES[name]
            inp = make_inputs(SEEDS[name], R, K, D, spec)
        inp["z"], inp["zbound"] = {}, {}
        for T in sorted({T for _, T in THRESHOLDS}):
            inp["z"][T], inp["zbound"][T] = ref_logits(inp["x"], inp["wn"], T)
            inp["z"][T].setflags(write=False)
            inp["zbound"][T].setflags(write=False)
        inp["name"] = name
        for v in inp.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _CACHE[name] = inp
    return _CACHE[name]


# -------------------------------------------------------------------------------------------------- the rest of inference
def py_nms(boxes, scores, thr):
    """torchvision.ops.nms' published algorithm in f32 (make_golden.py's stand-in): kept indices in descending-score order"""
    order = sorted(range(len(scores)), key=lambda i: (-float(scores[i]), i))
    b = np.asarray(boxes, np.float32)
    area = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    keep, dead = [], np.zeros(len(scores), bool)
    for ai, i in enumerate(order):
        if dead[i]:
            continue
        keep.append(i)
        for j in order[ai + 1:]:
            if dead[j]:
                continue
            w = max(np.float32(0), min(b[i, 2], b[j, 2]) - max(b[i, 0], b[j, 0]))
            h = max(np.float32(0), min(b[i, 3], b[j, 3]) - max(b[i, 1], b[j, 1]))
            inter = np.float32(w * h)
            union = area[i] + area[j] - inter
            if union > 0 and inter / union > np.float32(thr):          # (two boxes clipped to nothing: 0 / 0, never suppressed)
                dead[j] = True
    return np.asarray(keep, np.int64)


def ref_inference(z, bound, boxes, obj, thresh, nms_thresh, topk, img_h, img_w):
    """the whole fast_rcnn_inference_single_image with hard NMS on the float64 scores -> (boxes f32, scores f64, classes, kept row
    indices counting finite rows only)"""
    sel = ref_select(z, bound, boxes, obj, thresh, img_h, img_w)
    if len(sel["rows"]) == 0:
        e = np.zeros(0, np.int64)
        return np.zeros((0, 4), np.float32), np.zeros(0), e, e
    b = sel["boxes"]
    off = sel["cls"].astype(np.float32) * (b.max() + np.float32(1))
    keep = py_nms(b + off[:, None], sel["scores"].astype(np.float32), nms_thresh)
    if topk >= 0:
        keep = keep[:topk]
    rank = np.cumsum(sel["valid"]) - 1
    return b[keep], sel["scores"][keep], sel["cls"][keep], rank[sel["rows"][keep]]
