"""References and case builders for the index stages of cddmsl_amd/csrc/boxes.hip (imported by tests/test_boxes_ref_host.py and
tests/test_gpu_boxes_exact.py; not a conftest; numpy only, no GPU and no torch needed to import).

What "bit-exact" means here.  The contract at the top of boxes.hip is the reference's f32 expression, one IEEE operation at a time in
the reference's association order: every operation below is evaluated on ``np.float32`` values (numpy's elementwise f32 operations are
single correctly rounded IEEE operations, never contracted), so each expression has exactly one answer, and comparisons are strict,
ties go to the first index and signed zeros are equal scores.  The float64 / ``fractions.Fraction`` evaluations are witnesses: they
describe a case (clear or near-threshold, exact or not), they never replace the expected value and never loosen a comparison.

The references are plain loops (a scalar loop over candidates / boxes, f32 array operations across the other axis), independent of
oracle/ops.py and of torch; tests/test_boxes_ref_host.py ties them to the oracle on every case before they judge a kernel."""
import functools
import math
from fractions import Fraction

import numpy as np

F32 = np.float32
U = 2.0 ** -24                     # unit roundoff of f32: |fl(x) - x| <= U |x|
NEAR = Fraction(1, 2 ** 22)        # a pair is "near-threshold" when its exact IoU lies within 2^-22 of thr
# Maximum error of expf in the HIP math API reference ("Single precision mathematical functions", table of supported device functions
# with their maximum ULP error, ROCm documentation): expf -- 1 ULP.  An ulp of y is at most 2 U |y|.
EXPF_ULP = 1.0
BAND = 2.5e-7                      # k_nms_mask takes the division when 0 < inter - thr * u < BAND * u


def f32a(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float32))


# =============================================================================================================== IoU, NMS form
def areas32(b):
    return (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])


def nms_row32(b, i, area):
    """inter and union of box i with every box, each f32 operation in torchvision's order -> (inter, u, the raw intermediates)"""
    xx1, yy1 = np.maximum(b[i, 0], b[:, 0]), np.maximum(b[i, 1], b[:, 1])
    xx2, yy2 = np.minimum(b[i, 2], b[:, 2]), np.minimum(b[i, 3], b[:, 3])
    dw, dh = xx2 - xx1, yy2 - yy1
    w, h = np.maximum(F32(0), dw), np.maximum(F32(0), dh)
    inter = w * h
    s = area[i] + area
    u = s - inter
    assert inter.dtype == u.dtype == np.float32
    return inter, u, (dw, dh, s)


def over32(inter, u, thr):
    """the contract: inter / u > thr, one IEEE f32 division (0 / 0 is NaN, which is not greater)"""
    with np.errstate(divide="ignore", invalid="ignore"):
        return inter / u > F32(thr)


def over_without_division(inter, u, thr):
    """NEGATIVE CONTROL, not a reference: the sign of inter - thr * u (exact in float64: 24 x 24 bit product, correctly rounded
    difference keeps its sign), which is what a kernel without the division fallback decides"""
    u64 = u.astype(np.float64)
    return (inter.astype(np.float64) - float(F32(thr)) * u64 > 0) & (u64 > 0)


def nms_ref(boxes, valid, thr, max_keep, over=over32):
    """greedy NMS over score-descending boxes [n, 4] f32; only valid == 1 are candidates -> kept positions (int32), at most max_keep"""
    boxes = f32a(boxes).reshape(-1, 4)
    n = boxes.shape[0]
    area = areas32(boxes)
    dead = np.asarray(valid).reshape(-1) != 1
    keep = []
    for i in range(n):
        if dead[i]:
            continue
        if len(keep) >= max_keep:
            break
        keep.append(i)
        inter, u, _ = nms_row32(boxes, i, area)
        ov = over(inter, u, thr)
        ov[:i + 1] = False
        dead = dead | ov
    return np.asarray(keep, dtype=np.int32)


def classify_pairs(boxes, thr):
    """float64 witness over all pairs i < j with a positive intersection -> (clear, near): near = |IoU - thr| <= 2^-22"""
    b = f32a(boxes).reshape(-1, 4).astype(np.float64)
    t = float(F32(thr))
    clear = near = 0
    a = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    for i in range(b.shape[0] - 1):
        c = b[i + 1:]
        w = np.maximum(0.0, np.minimum(b[i, 2], c[:, 2]) - np.maximum(b[i, 0], c[:, 0]))
        h = np.maximum(0.0, np.minimum(b[i, 3], c[:, 3]) - np.maximum(b[i, 1], c[:, 1]))
        inter = w * h
        u = a[i] + a[i + 1:] - inter
        m = (inter > 0) & (u > 0)
        d = np.abs(inter[m] / u[m] - t)
        near += int((d <= float(NEAR)).sum())
        clear += int((d > float(NEAR)).sum())
    return clear, near


def grid_exact(boxes):
    """True when every f32 operation of the NMS IoU except the division is exact for every pair of ``boxes``: each f32 intermediate
    equals the same operation in float64 (which is exact for these magnitudes: 24-bit operands, 53-bit results)"""
    b = f32a(boxes).reshape(-1, 4)
    d = b.astype(np.float64)
    area = areas32(b)
    a64 = (d[:, 2] - d[:, 0]) * (d[:, 3] - d[:, 1])
    if not np.array_equal(area.astype(np.float64), a64):
        return False
    for i in range(b.shape[0]):
        inter, u, (dw, dh, s) = nms_row32(b, i, area)
        dw64 = np.minimum(d[i, 2], d[:, 2]) - np.maximum(d[i, 0], d[:, 0])
        dh64 = np.minimum(d[i, 3], d[:, 3]) - np.maximum(d[i, 1], d[:, 1])
        in64 = np.maximum(0.0, dw64) * np.maximum(0.0, dh64)
        s64 = a64[i] + a64
        for got, exp in ((dw, dw64), (dh, dh64), (inter, in64), (s, s64), (u, s64 - in64)):
            if not np.array_equal(got.astype(np.float64), exp):
                return False
    return True


def pair_exact(bi, bj):
    """(inter, u) of two boxes as Fractions of their f32 coordinates (the high-precision witness)"""
    bi, bj = [Fraction(float(v)) for v in bi], [Fraction(float(v)) for v in bj]
    w = max(Fraction(0), min(bi[2], bj[2]) - max(bi[0], bj[0]))
    h = max(Fraction(0), min(bi[3], bj[3]) - max(bi[1], bj[1]))
    inter = w * h
    return inter, (bi[2] - bi[0]) * (bi[3] - bi[1]) + (bj[2] - bj[0]) * (bj[3] - bj[1]) - inter


# =============================================================================================================== matcher
def iou_match32(g, p):
    """pairwise_iou of one box g [4] with predictions p [P, 4], f32 operation by operation (structures/boxes.py order)"""
    w = np.minimum(g[2], p[:, 2]) - np.maximum(g[0], p[:, 0])
    h = np.minimum(g[3], p[:, 3]) - np.maximum(g[1], p[:, 1])
    w, h = np.maximum(w, F32(0)), np.maximum(h, F32(0))
    inter = w * h
    ag = (g[2] - g[0]) * (g[3] - g[1])
    ap = (p[:, 2] - p[:, 0]) * (p[:, 3] - p[:, 1])
    u = (ag + ap) - inter
    with np.errstate(divide="ignore", invalid="ignore"):
        q = inter / u
    v = np.where(inter > 0, q, F32(0))
    assert v.dtype == np.float32
    return v


def matcher_ref(gt, preds, thresholds, labels, allow_low_quality):
    """-> (matches int64 [P], labels int8 [P]): argmax over boxes with the FIRST maximum, strict < against the f32 cut points, and
    label 1 for every prediction that attains some box's row maximum (ties included; a row maximum of 0 marks every prediction)"""
    gt, preds = f32a(gt).reshape(-1, 4), f32a(preds).reshape(-1, 4)
    G, P = gt.shape[0], preds.shape[0]
    if G == 0 or P == 0:
        return np.zeros(P, np.int64), np.full(P, labels[0], np.int8)
    best, arg = np.full(P, -1, np.float32), np.zeros(P, np.int64)
    hit = np.zeros(P, bool)
    for g in range(G):
        v = iou_match32(gt[g], preds)
        m = v > best
        best[m], arg[m] = v[m], g
        if allow_low_quality:
            hit |= v == v.max()
    t = [F32(x) for x in thresholds]
    if len(t) == 1:
        lab = np.where(best < t[0], labels[0], labels[1])
    else:
        lab = np.where(best < t[0], labels[0], np.where(best < t[1], labels[1], labels[2]))
    lab = lab.astype(np.int8)
    lab[hit] = 1
    return arg, lab


def matcher_ref_batched(gts, preds, counts, thresholds, labels, allow_low_quality):
    """per image, then laid out as cddmsl_iou_match_batched documents: [N][P] for shared predictions (counts None), [sum P] else"""
    ms, ls = [], []
    off = 0
    for n, g in enumerate(gts):
        p = preds if counts is None else preds[off:off + counts[n]]
        off += 0 if counts is None else counts[n]
        m, l = matcher_ref(g, p, thresholds, labels, allow_low_quality)
        ms.append(m)
        ls.append(l)
    return (np.stack(ms), np.stack(ls)) if counts is None else (np.concatenate(ms), np.concatenate(ls))


# =============================================================================================================== sort
def sort_ref(keys):
    """stable descending sort of every row of keys [N, total] f32 -> order int32 [N, total]: Python's sorted with key
    (-value, index) on the f32 values, so -0.0 == 0.0 and equal scores keep the lower index first.  NaN keys are out of scope (no
    order is defined for them; the RPN raises on non-finite logits before sorting)."""
    keys = f32a(keys)
    assert not np.isnan(keys).any()
    out = np.empty(keys.shape, np.int32)
    for n in range(keys.shape[0]):
        row = [float(v) for v in keys[n]]
        out[n] = sorted(range(len(row)), key=lambda i: (-row[i], i))
    return out


# =============================================================================================================== anchors, decode
def cell_anchors(sizes=(32, 64, 128, 256, 512), ratios=(0.5, 1.0, 2.0)):
    """anchor_generator.py:39-51 in float64, stored as f32 (what the kernels are given)"""
    out = []
    for s in sizes:
        for r in ratios:
            w = math.sqrt(s * s / r)
            h = r * w
            out.append([-w / 2, -h / 2, w / 2, h / 2])
    return f32a(out)


def anchors_ref(cell, Hf, Wf, stride, offset):
    """[Hf * Wf * A, 4] float64 (hw-major, a-minor).  For the strides and offsets of the cases the shift is an exact f32 value, so the
    kernel's anchor is ONE rounded addition of exact operands: np.float32 of this result, bit for bit."""
    loc = np.arange(Hf * Wf)
    sx = float(F32(offset)) * float(F32(stride)) + (loc % Wf) * float(F32(stride))
    sy = float(F32(offset)) * float(F32(stride)) + (loc // Wf) * float(F32(stride))
    assert np.array_equal(sx, sx.astype(np.float32)) and np.array_equal(sy, sy.astype(np.float32))
    sh = np.stack([sx, sy, sx, sy], 1)
    return (sh[:, None, :] + cell.astype(np.float64)[None]).reshape(-1, 4)


def decode_ref(case):
    """k_rpn_decode's expression (apply_deltas + clip + nonempty) in float64 from the f32 inputs, with a first-order running error
    bound for the f32 kernel: every f32 operation contributes U |result| (an exactly representable result, such as 0.5 * x, nothing),
    expf contributes EXPF_ULP ulps = EXPF_ULP * 2 U |result|, and the errors of the operands propagate through the derivative of the
    operation.  Counted per x coordinate (y alike): shift 3 roundings, anchor corner 1, w 1, cx 1, dx 1, dx * w 1, pcx 1, dw 1,
    expf (1 ulp), pw 1, x 1 -- scaled by the magnitudes of the terms as they occur, not by one worst case.  ``bound`` is that
    first-order sum times 2 (the margin covers the dropped second-order terms).  A clipped coordinate whose unclipped value lies more
    than the bound outside the image is exact (bound 0).

    -> dict: boxes [N, topk, 4] f64, bound [N, topk, 4], finite [N, topk], valid [N, topk] uint8 (0 / 1 / 2 as the kernel documents),
    ambiguous [N, topk]: finite entries whose width or height lies within the bound of min_size (either verdict is accepted there)."""
    c = case
    N, total = c["order"].shape
    A, Wf, topk = c["A"], c["Wf"], c["topk"]
    a = c["order"][:, :topk].astype(np.int64)
    ca, loc = a % A, a // A
    st, off = float(F32(c["stride"])), float(F32(c["offset"]))
    cell = c["cell"].astype(np.float64)[ca]                                   # [N, topk, 4]
    d = np.take_along_axis(c["deltas"].astype(np.float64), a[:, :, None], 1)  # [N, topk, 4]
    wts = [float(F32(x)) for x in c["weights"]]
    clamp = float(F32(c["scale_clamp"]))
    ab = np.abs
    out, err = [None] * 4, [None] * 4
    with np.errstate(invalid="ignore", over="ignore"):
        for ax, pos in ((0, loc % Wf), (1, loc // Wf)):
            s = off * st + pos * st
            e_s = U * (ab(off * st) + ab(pos * st) + ab(s))
            a0, a1 = s + cell[..., ax], s + cell[..., ax + 2]
            e_a0, e_a1 = e_s + U * ab(a0), e_s + U * ab(a1)
            w = a1 - a0
            e_w = e_a0 + e_a1 + U * ab(w)
            cx = a0 + 0.5 * w
            e_cx = e_a0 + 0.5 * e_w + U * ab(cx)
            dx = d[..., ax] / wts[ax]
            e_dx = U * ab(dx)
            dwq = d[..., ax + 2] / wts[ax + 2]
            e_dw = U * ab(dwq)
            dw = np.minimum(dwq, clamp)                                       # (NaN propagates, as torch.clamp(max=) does)
            prod = dx * w
            e_prod = ab(dx) * e_w + ab(w) * e_dx + U * ab(prod)
            pcx = prod + cx
            e_pcx = e_prod + e_cx + U * ab(pcx)
            ex = np.exp(dw)
            e_ex = ex * e_dw + EXPF_ULP * 2 * U * ex
            pw = ex * w
            e_pw = ex * e_w + ab(w) * e_ex + U * ab(pw)
            out[ax], out[ax + 2] = pcx - 0.5 * pw, pcx + 0.5 * pw
            err[ax] = e_pcx + 0.5 * e_pw + U * ab(out[ax])
            err[ax + 2] = e_pcx + 0.5 * e_pw + U * ab(out[ax + 2])
        raw = np.stack(out, -1)
        e = np.stack(err, -1)
        finite = np.isfinite(raw).all(-1)
        hw = np.asarray(c["img_hw"], np.float64)
        lim = np.stack([hw[:, 1], hw[:, 0], hw[:, 1], hw[:, 0]], -1)[:, None, :]
        boxes = np.minimum(np.maximum(raw, 0.0), lim)
        saturated = (raw < -2 * e) | (raw > lim + 2 * e)
        e = np.where(saturated, 0.0, e)
        ms = float(F32(c["min_size"]))
        amb = np.zeros(finite.shape, bool)
        fail = np.zeros(finite.shape, bool)
        ok = np.ones(finite.shape, bool)
        for lo, hi in ((0, 2), (1, 3)):
            ext = boxes[..., hi] - boxes[..., lo]
            be = e[..., hi] + e[..., lo] + U * ab(ext)
            close = (ab(ext - ms) <= 2 * be) & (be > 0)
            fail |= (ext <= ms) & ~close
            amb |= close
            ok &= ext > ms
    valid = np.where(finite, ok.astype(np.uint8), np.uint8(2)).astype(np.uint8)
    return dict(boxes=boxes, bound=2 * e, finite=finite, valid=valid, ambiguous=finite & amb & ~fail)


# =============================================================================================================== NMS cases
Q = 0.25     # the grid of every case that claims exactness: quarter pixels


def _case(name, boxes, valid, thr, max_keep):
    boxes = f32a(boxes)
    if boxes.ndim == 2:
        boxes = boxes[None]
    N, n = boxes.shape[:2]
    valid = np.ones((N, n), np.uint8) if valid is None else np.ascontiguousarray(np.asarray(valid, np.uint8).reshape(N, n))
    return dict(name=name, boxes=boxes, valid=valid, thr=thr, max_keep=int(max_keep))


def _clustered(n, seed):
    """n boxes around a few centres on the quarter-pixel grid: widths 20 - 60 px, coordinates below 400 px (areas and unions far
    below 2^24 grid units), heavy overlap inside a cluster"""
    r = np.random.RandomState(seed)
    k = max(1, n // 24)
    cen = r.randint(40, 300, size=(k, 2)) * 4
    which = r.randint(0, k, size=n)
    x0 = cen[which, 0] + r.randint(-40, 41, size=n)
    y0 = cen[which, 1] + r.randint(-40, 41, size=n)
    w, h = r.randint(80, 241, size=n), r.randint(80, 241, size=n)
    return f32a(np.stack([x0, y0, x0 + w, y0 + h], 1) * Q)


def _locations():
    """64 disjoint 40 x 40 px boxes, 100 px apart"""
    i = np.arange(64)
    x, y = (i % 8) * 100.0, (i // 8) * 100.0
    return np.stack([x, y, x + 40, y + 40], 1)


DENSE_KEPT = (1, 15, 16, 17, 32, 64)


def dense_slots(k):
    """the k slots of chunk 0 that survive: slot 0 always, slot 63 when k >= 2 (the walk's b == 63 branch), the rest spread evenly"""
    if k == 1:
        return [0]
    if k == 64:
        return list(range(64))
    mid = sorted({1 + (j * 61) // (k - 2) for j in range(k - 2)}) if k > 2 else []
    assert len(mid) == k - 2 and all(0 < m < 63 for m in mid)
    return [0] + mid + [63]


def _dense(k):
    """192 candidates.  Chunk 0: slot m holds location m when m is one of the k surviving slots, else a copy of slot 0's box (removed
    by slot 0).  Chunk 1: location m shifted by 2 px in x -- removed by chunk 0's slot m only, so by exactly one kept row each: a kept
    row missing from the OR of the rows (or a wrong padding row) changes the result.  Chunk 2: location m shifted by 4 px in y --
    removed by chunk 0's slot m when that survives, else by chunk 1's slot m (IoU 0.82 and 0.75 at threshold 0.7)."""
    loc = _locations()
    slots = set(dense_slots(k))
    c0 = np.stack([loc[m] if m in slots else loc[0] for m in range(64)])
    c1 = loc + np.array([2.0, 0, 2.0, 0])
    c2 = loc + np.array([0, 4.0, 0, 4.0])
    return np.concatenate([c0, c1, c2])


def _ladder(n, lead):
    """boxes 10 x 10 px, 3 px apart along x: IoU with the successor 7/13 > 0.5, with the one after 4/16 -- each removes only its
    successor.  ``lead`` isolated boxes in front shift the parity of the survivors."""
    x = np.arange(n - lead) * 3.0
    lad = np.stack([x, np.zeros_like(x), x + 10, np.full_like(x, 10.0)], 1)
    iso = np.stack([np.array([0.0, 100.0 + 50 * i, 10.0, 110.0 + 50 * i]) for i in range(lead)]) if lead else np.zeros((0, 4))
    return np.concatenate([iso, lad])


def kept_in_chunk0(case, img=0):
    k = nms_ref(case["boxes"][img], case["valid"][img], case["thr"], case["boxes"].shape[1])
    return int((k < 64).sum())


@functools.lru_cache(None)
def nms_cases():
    cs = []
    thrs = (0.3, 0.5, 0.7)
    for t, n in enumerate((1, 63, 64, 65, 127, 128, 129)):
        cs.append(_case(f"clustered_n{n}", _clustered(n, 100 + n), None, thrs[t % 3], n))
    big = np.stack([_clustered(327, 7 + s) for s in range(3)])
    for thr in thrs:
        cs.append(_case(f"clustered_3x327_thr{thr}", big, None, thr, 327))
    v = (np.arange(3 * 327).reshape(3, 327) + np.arange(3)[:, None]) % 3              # 0 / 1 / 2, a different phase per image
    cs.append(_case("valid_0_1_2_3x327", big, v, 0.5, 327))
    cs.append(_case("valid_0_1_2_n129", big[0, :129], np.arange(129) % 3, 0.7, 129))
    cs.append(_case("valid_all_0_n129", big[1, :129], np.zeros(129), 0.7, 129))
    v = np.ones((3, 327), np.uint8)
    v[1] = 0                                                                          # an image without candidates between two with
    cs.append(_case("valid_middle_image_0", big, v, 0.7, 100))
    for k in DENSE_KEPT:
        cs.append(_case(f"dense_keep{k}", _dense(k), None, 0.7, 192))
    for mk in (63, 64, 65):                                                           # max_keep at / around a chunk's last bit
        cs.append(_case(f"dense_keep64_max{mk}", _dense(64), None, 0.7, mk))
    cs.append(_case("dense_keep17_max17", _dense(17), None, 0.7, 17))
    cs.append(_case("ladder_odd", _ladder(200, 1), None, 0.5, 200))                   # survivors 0, 1, 3, .. 63, 65, .. 127, 129
    cs.append(_case("ladder_even", _ladder(200, 0), None, 0.5, 200))                  # survivors 0, 2, .. 62, 64, .. 126, 128
    cs.append(_case("identical_n70", np.tile(np.array([[8.0, 8.0, 40.25, 30.5]]), (70, 1)), None, 0.5, 70))
    deg = _clustered(100, 55)
    deg[3::7, 2] = deg[3::7, 0]                                                       # zero width
    deg[5::11, 3] = deg[5::11, 1]                                                     # zero height
    deg[2::13, [0, 2]] = deg[2::13, [2, 0]]                                           # x1 < x0
    deg[6::17] = deg[6]                                                               # identical, one of them degenerate or not
    deg[[20, 21, 22]] = np.array([50.0, 50.0, 50.0, 50.0])                            # identical zero-area points: 0 / 0
    cs.append(_case("degenerate_n100", deg, None, 0.3, 100))
    for n, seed in ((129, 0), (327, 1)):
        base = _case("", big[seed, :n], None, 0.5, n)
        c0 = kept_in_chunk0(base)
        for mk in sorted({1, c0, c0 + 1, n}):
            cs.append(_case(f"max_keep{mk}_n{n}", big[seed, :n], None, 0.5, mk))
    for thr in thrs:
        t = threshold_cases(thr)
        for cls in "abc":
            if len(t[cls]):
                cs.append(_case(f"threshold_{cls}_thr{thr}", spread(t[cls]).reshape(-1, 4), None, thr, 2 * len(t[cls])))
        allp = spread(np.concatenate([t[cls] for cls in "abc" if len(t[cls])]))
        cs.append(_case(f"threshold_all_thr{thr}", allp.reshape(-1, 4), None, thr, 2 * len(allp)))
    names = [c["name"] for c in cs]
    assert len(set(names)) == len(names)
    return tuple(cs)


def anyorder_inputs(case):
    """image 0 of an NMS case as cddmsl_nms_anyorder / torchvision.ops.nms take it: a seeded permutation of the boxes, scores tied in
    groups (about three candidates per score)"""
    b = case["boxes"][0]
    n = b.shape[0]
    r = np.random.RandomState(n + 1)
    return np.ascontiguousarray(b[r.permutation(n)]), f32a(r.randint(0, n // 3 + 1, size=n))


def anyorder_ref(boxes, scores, thr):
    """kept input indices (int64) in descending score order, equal scores by index: sort_ref, then nms_ref on the sorted boxes"""
    if len(scores) == 0:
        return np.zeros(0, np.int64)
    order = sort_ref(scores[None])[0]
    return order[nms_ref(boxes[order], np.ones(len(order), np.uint8), thr, len(order))].astype(np.int64)


# =============================================================================================================== threshold pairs
def spread(pairs):
    """pairs [k, 2, 4] moved 1024 px apart along x (whole pixels: every coordinate stays on the grid), so that only the two boxes of
    a pair meet"""
    return f32a(pairs + (np.arange(len(pairs)) * 1024.0)[:, None, None] * np.array([1.0, 0, 1.0, 0]))


def _quotient_over(inter, u, thr):
    return bool(F32(inter) / F32(u) > F32(thr))


def pair_class(inter, u, thr):
    """class of a pair with integer inter, u (grid units^2, both exact in f32): 'a' exact IoU above thr but the f32 quotient not
    greater (the 700 / 1000 family); 'b' inside the kernel's fallback band with the quotient greater; None otherwise"""
    T = Fraction(float(F32(thr)))
    r = Fraction(inter) - T * u
    if r <= 0:
        return None
    q = _quotient_over(inter, u, thr)
    if not q:
        return "a"
    if r < Fraction(2.0e-7) * u:          # (well inside BAND = 2.5e-7, so that the kernel's own rounded test agrees)
        return "b"
    return None


def _factor(a2, w1, h1):
    """w2 <= w1, h2 <= h1 with w2 * h2 == a2, or None"""
    lo = max(1, -(-a2 // h1))
    ws = np.arange(lo, w1 + 1, dtype=np.int64)
    ws = ws[a2 % ws == 0]
    return (int(ws[0]), int(a2 // ws[0])) if len(ws) else None


CLASS_A_IMPOSSIBLE = (0.5,)


@functools.lru_cache(None)
def threshold_cases(thr, count=8):
    """Pairs (A, B) with B inside A on the quarter-pixel grid, found by a seeded search; A is the higher-scoring box.  With B inside A
    inter = area(B) and u = area(A), with area(A) < 2^23 grid units^2, so that the sum of any two areas is below 2^24: every operation
    but the division is exact, for the two boxes of a pair and across pairs.  -> dict of [count, 2, 4] f32 arrays:
      a: exact IoU > thr, f32 quotient not > thr -- both boxes are KEPT; a kernel deciding by the sign of inter - thr * u removes B
      b: 0 < inter - thr * u < 2e-7 u (the kernel's fallback band) and the f32 quotient > thr -- B is removed
      c: exact IoU at or just below thr: area(B) = floor(thr * area(A)) (the next unit of area is above thr), and the class a / b pairs
         with B one grid step narrower -- B is kept
    Class a is EMPTY for thr = 0.5, provably: inter and u are f32 values, and inter > u / 2 with u / 2 an f32 value means
    inter >= u / 2 (1 + 2^-23), whose quotient rounds to at least 0.5 (1 + 2^-23) > 0.5.  No f32 inputs exist for that class."""
    T = Fraction(float(F32(thr)))
    rng = np.random.RandomState(int(round(thr * 1000)))
    out = {"a": [], "b": [], "c": []}
    want = {"a": 0 if thr in CLASS_A_IMPOSSIBLE else count, "b": count, "c": count}
    step = []

    def place(w1, h1, w2, h2):
        ox, oy = int(rng.randint(0, w1 - w2 + 1)), int(rng.randint(0, h1 - h2 + 1))
        return np.array([[0, 0, w1, h1], [ox, oy, ox + w2, oy + h2]], np.float64) * Q

    for _ in range(200000):
        if all(len(out[k]) >= want[k] for k in out):
            break
        w1, h1 = int(rng.randint(1800, 3600)), int(rng.randint(1800, 3600))
        a1 = w1 * h1
        base = int(T * a1)                                   # floor
        if a1 >= 2 ** 23:                                    # area(A) + area(A') of two different pairs stays exact as well
            continue
        for a2 in (base, base + 1, base + 2, base + 3):
            cls = "c" if a2 == base else pair_class(a2, a1, thr)
            if cls is None or len(out[cls]) >= want[cls]:
                continue
            f = _factor(a2, w1, h1)
            if f is None:
                continue
            out[cls].append(place(w1, h1, *f))
            if cls in "ab" and len(step) < count and f[0] > 1:
                step.append(place(w1, h1, f[0] - 1, f[1]))
    if thr == 0.7:                                           # the smallest members of the family: 700 / 1000
        out["a"][0] = np.array([[0, 0, 40, 25], [2, 0, 30, 25]], np.float64)   # inter 28 x 25 = 700, u 1000
    if thr == 0.5:                                           # IoU exactly on the threshold: 1/2 is not > 0.5
        out["c"][0] = np.array([[0, 0, 40, 25], [7, 0, 27, 25]], np.float64)
    out["c"] = out["c"] + step
    return {k: f32a(np.stack(v)) if v else np.zeros((0, 2, 4), np.float32) for k, v in out.items()}


# =============================================================================================================== sort cases
@functools.lru_cache(None)
def sort_cases():
    r = np.random.RandomState(11)
    sub = np.array([1e-45, -1e-45, 5e-39, -5e-39], np.float64).astype(np.float32)
    special = np.concatenate([f32a([0.0, -0.0, np.inf, -np.inf, 1.0, -1.0, 3.4e38, -3.4e38, 1.1754944e-38]), sub])

    def mixed(N, total):
        k = f32a(r.randn(N, total))
        m = r.rand(N, total) < 0.5
        k[m] = special[r.randint(0, len(special), size=int(m.sum()))]
        return k

    cs = [("signed_zero_row", f32a([[0.0, -0.0, 1.0, -0.0, 0.0, -1.0]])),
          ("n1_total1", f32a([[-0.0]])),
          ("n17_total1", f32a(r.randn(17, 1))),
          ("n1_total1000_random", f32a(r.randn(1, 1000))),
          ("n2_total255_mixed", mixed(2, 255)),
          ("n3_total256_mixed", mixed(3, 256)),
          ("n5_total257_few_values", f32a(r.randint(-2, 3, size=(5, 257)) * 0.5)),
          ("n16_total1000_mixed", mixed(16, 1000)),
          ("n17_total255_rows_equal", np.repeat(f32a(r.randn(17, 1)), 255, 1)),
          ("n3_total257_all_equal_zero_signs", np.where(r.rand(3, 257) < 0.5, F32(0.0), F32(-0.0)).astype(np.float32)),
          ("n5_total1000_signed_zeros_and_inf", f32a(r.choice(f32a([0.0, -0.0, np.inf, -np.inf, 1e-45, -1e-45]), size=(5, 1000)))),
          ("n2_total256_random", f32a(r.randn(2, 256)))]
    return tuple(dict(name=n, keys=np.ascontiguousarray(k)) for n, k in cs)


# =============================================================================================================== matcher cases
def _grid_boxes(n, seed, span=200, wmax=60):
    r = np.random.RandomState(seed)
    x0, y0 = r.randint(0, span, size=n), r.randint(0, span, size=n)
    return f32a(np.stack([x0, y0, x0 + r.randint(1, wmax, size=n), y0 + r.randint(1, wmax, size=n)], 1))


RPN_T, RPN_L = (0.3, 0.7), (0, -1, 1)
ROI_T, ROI_L = (0.5,), (0, 1)
BATCH_PRED_COUNTS = (0, 1, 255, 1025, 3000)
BATCH_BOX_COUNTS = (2, 0, 1, 0, 300)


def _m(name, gt, preds, thr, lab, lq):
    return dict(name=name, gt=f32a(gt).reshape(-1, 4), preds=f32a(preds).reshape(-1, 4), thresholds=thr, labels=lab, allow_low_quality=lq)


@functools.lru_cache(None)
def match_cases():
    cs = []
    g = [[0, 0, 10, 10]]
    # IoU 3/10, 1/2, 7/10 (= RN(7/10) = 0.7f), one unit either side of each, no overlap, identical
    cut = [[0, 0, 3, 10], [0, 0, 5, 10], [0, 0, 7, 10], [0, 0, 10, 10], [20, 20, 30, 30], [0, 0, 2, 10], [0, 0, 4, 10], [0, 0, 6, 10],
           [0, 0, 8, 10], [0, 0, 10, 5], [0, 0, 10, 7], [0, 0, 10, 3]]
    for lq in (False, True):
        cs.append(_m(f"cut_points_rpn_lq{int(lq)}", g, cut, RPN_T, RPN_L, lq))
        cs.append(_m(f"cut_points_roi_lq{int(lq)}", g, cut, ROI_T, ROI_L, lq))
    # two boxes with the same IoU for one prediction (and two identical boxes): the first wins
    cs.append(_m("equal_iou_two_boxes", [[0, 0, 10, 10], [10, 0, 20, 10], [10, 0, 20, 10]], [[5, 0, 15, 10], [10, 0, 20, 10], [12, 0, 22, 10]],
                 ROI_T, ROI_L, True))
    # several predictions tied for a box's row maximum: all of them get label 1
    cs.append(_m("tied_row_maximum", [[0, 0, 100, 100]], [[0, 0, 20, 20], [80, 80, 100, 100], [0, 80, 20, 100], [40, 40, 50, 50], [0, 0, 20, 20]],
                 RPN_T, RPN_L, True))
    # a box that no prediction overlaps: row maximum 0, every prediction is labelled 1
    far = _grid_boxes(300, 3)
    cs.append(_m("box_without_overlap_lq1", [[10, 10, 60, 60], [5000, 5000, 5010, 5010]], far, RPN_T, RPN_L, True))
    cs.append(_m("box_without_overlap_lq0", [[10, 10, 60, 60], [5000, 5000, 5010, 5010]], far, RPN_T, RPN_L, False))
    cs.append(_m("no_boxes", np.zeros((0, 4)), far, RPN_T, RPN_L, True))
    cs.append(_m("g1", _grid_boxes(1, 4, wmax=150), _grid_boxes(700, 5), RPN_T, RPN_L, True))
    cs.append(_m("g300_more_than_a_block", _grid_boxes(300, 6), _grid_boxes(517, 7), ROI_T, ROI_L, True))
    for P in (255, 256, 257, 1023, 1024, 1025):
        cs.append(_m(f"p{P}", _grid_boxes(3, 8, wmax=120), _grid_boxes(P, 9 + P), RPN_T, RPN_L, True))
    return tuple(cs)


@functools.lru_cache(None)
def match_batched_cases():
    gts = [_grid_boxes(g, 20 + i, wmax=120) for i, g in enumerate(BATCH_BOX_COUNTS)]
    shared = _grid_boxes(1025, 30)
    cat = _grid_boxes(sum(BATCH_PRED_COUNTS), 31)
    cs = []
    for lq in (True, False):
        cs.append(dict(name=f"shared_p1025_lq{int(lq)}", gts=gts, preds=shared, counts=None, thresholds=RPN_T, labels=RPN_L, allow_low_quality=lq))
        cs.append(dict(name=f"concatenated_lq{int(lq)}", gts=gts, preds=cat, counts=BATCH_PRED_COUNTS, thresholds=ROI_T, labels=ROI_L,
                       allow_low_quality=lq))
    cs.append(dict(name="shared_p257_middle_image_without_boxes", gts=[gts[0], gts[1], gts[2]], preds=shared[:257], counts=None,
                   thresholds=ROI_T, labels=ROI_L, allow_low_quality=True))
    cs.append(dict(name="no_image_has_boxes", gts=[gts[1], gts[3]], preds=shared[:300], counts=None, thresholds=RPN_T, labels=RPN_L,
                   allow_low_quality=True))
    return tuple(cs)


# =============================================================================================================== decode cases
SCALE_CLAMP = math.log(1000.0 / 16)
DECODE_SKIP_CAP = 0.01          # at most 1 % of the valid entries may lie within the bound of min_size (0 % of the coordinates)


@functools.lru_cache(None)
def decode_cases():
    cs = []
    cell = cell_anchors()
    A = cell.shape[0]
    k = 0
    for (Hf, Wf), sizes in (((5, 7), ((70, 100), (80, 112))), ((12, 17), ((180, 260), (192, 272)))):
        total = Hf * Wf * A
        for topk in (total, total - 1):
            for offset, min_size, weights in ((0.0, 0.0, (1.0, 1.0, 1.0, 1.0)), (0.5, 4.0, (1.0, 1.0, 1.0, 1.0)), (0.5, 0.0, (10.0, 10.0, 5.0, 5.0)),
                                              (0.0, 4.0, (10.0, 10.0, 5.0, 5.0))):
                r = np.random.RandomState(1000 + k)
                k += 1
                deltas = f32a(r.randn(2, total, 4) * 0.4 * np.array(weights))
                order = np.stack([r.permutation(total) for _ in range(2)]).astype(np.int32)
                deltas[1, order[1, 3], 2] = 50.0 * weights[2]         # the scale clamp
                deltas[0, order[0, 5], 3] = 50.0 * weights[3]
                deltas[0, order[0, 7], 0] = np.inf                    # non-finite: valid == 2
                deltas[1, order[1, 11], 2] = np.nan                   # (torch.clamp(max=) keeps a NaN: the box is not finite)
                deltas[1, order[1, 13], 1] = np.nan
                cs.append(dict(name=f"{Hf}x{Wf}_topk{topk}_off{offset}_min{min_size}_w{weights[0]}", Hf=Hf, Wf=Wf, A=A, topk=topk, stride=16.0,
                               offset=offset, min_size=min_size, weights=weights, scale_clamp=SCALE_CLAMP, cell=cell, deltas=deltas,
                               order=np.ascontiguousarray(order), img_hw=np.asarray(sizes, np.int32)))
    return tuple(cs)
