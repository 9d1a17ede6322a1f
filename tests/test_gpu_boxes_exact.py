"""The index stages of cddmsl_amd/csrc/boxes.hip (sort, anchors, decode, bitmask NMS, fused IoU + matcher), each called directly through
the C-ABI and compared with the numpy references of tests/exact_boxes.py on every case of its builders: indices, labels, keep lists
and sorted keys ``array_equal`` (no pair is excused), the decoded boxes within the bound derived there.  Every output buffer is
longer than documented and pre-filled with a sentinel (keep -7, labels 0x55, floats NaN): the documented part must be written
completely, everything behind it not at all.  tests/test_boxes_ref_host.py ties the references to the CPU oracle first.

Not run, and unexamined: the workload's 12000-candidate NMS shape (covered at bench shapes by the end-to-end suites), and the
matcher's G = 4096 cap -- 64 KiB of dynamic LDS on top of the batched kernel's static ``wmax`` may simply be refused at launch; that
is noted here rather than probed."""
import ctypes

import numpy as np
import pytest
import torch

import exact_boxes as E

pytestmark = pytest.mark.gpu
DEV = "cuda"
TAIL = 64
KEEP_S, LAB_S, WS_S = -7, 0x55, 0x5A
NMS = {c["name"]: c for c in E.nms_cases()}


def _L():
    from cddmsl_amd import hip
    return hip._L()


def _st():
    from cddmsl_amd import hip
    return hip.stream_ptr()


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def _dev(a, dtype=None):
    """a host array on the device (never an empty allocation: a dummy element stands in)"""
    a = np.ascontiguousarray(a if dtype is None else np.asarray(a, dtype))
    if a.size == 0:
        a = np.zeros(4, a.dtype)
    return torch.from_numpy(a).to(DEV)


def _buf(n, dtype, fill):
    return torch.full((n + TAIL,), fill, device=DEV, dtype=dtype)


def _host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def _untouched(t, start, fill, what):
    h = _host(t)[start:]
    assert (np.isnan(h).all() if isinstance(fill, float) else (h == fill).all()), f"{what}: an element past the documented output was written"


# ================================================================================================================= NMS
def _run_nms(c):
    N, n = c["boxes"].shape[:2]
    mk, nw = c["max_keep"], (n + 63) // 64
    boxes, valid = _dev(c["boxes"]), _dev(c["valid"])
    mask = _buf(N * n * nw, torch.int64, -1)                     # stale all-ones words: nothing may depend on what was there
    keep, nkeep = _buf(N * mk, torch.int32, KEEP_S), _buf(N, torch.int32, KEEP_S)
    assert _L().cddmsl_nms(_p(boxes), _p(valid), _p(mask), _p(keep), _p(nkeep), N, n, c["thr"], mk, _st()) == 0
    k, nk = _host(keep), _host(nkeep)
    assert (nk[N:] == KEEP_S).all() and (k[N * mk:] == KEEP_S).all() and (_host(mask)[N * n * nw:] == -1).all(), c["name"]
    for img in range(N):
        ref = E.nms_ref(c["boxes"][img], c["valid"][img], c["thr"], mk)
        row = k[img * mk:(img + 1) * mk]
        assert nk[img] == len(ref), (c["name"], img, int(nk[img]), len(ref))
        assert np.array_equal(row[:len(ref)], ref), (c["name"], img, row[:len(ref)].tolist(), ref.tolist())
        assert (row[len(ref):] == KEEP_S).all(), (c["name"], img, "keep[nkeep:] was written")


@pytest.mark.parametrize("name", list(NMS))
def test_nms(name):
    _run_nms(NMS[name])


def test_nms_without_candidates():
    """n == 0: nkeep is zeroed, keep is not touched"""
    keep, nkeep = _buf(3 * 5, torch.int32, KEEP_S), _buf(3, torch.int32, KEEP_S)
    d = _dev(np.zeros(4, np.float32))
    assert _L().cddmsl_nms(_p(d), _p(d), None, _p(keep), _p(nkeep), 3, 0, 0.7, 5, _st()) == 0
    assert _host(nkeep)[:3].tolist() == [0, 0, 0]
    _untouched(nkeep, 3, KEEP_S, "nkeep")
    _untouched(keep, 0, KEEP_S, "keep")


def _run_anyorder(boxes_h, scores_h, thr):
    K = len(scores_h)
    boxes, scores = _dev(boxes_h), _dev(scores_h)
    keep, nkeep = _buf(K, torch.int64, KEEP_S), _buf(1, torch.int32, KEEP_S)
    nbytes = ctypes.c_size_t(12345)
    assert _L().cddmsl_nms_anyorder(_p(boxes), _p(scores), _p(keep), _p(nkeep), K, thr, None, ctypes.byref(nbytes), _st()) == 0
    _untouched(keep, 0, KEEP_S, "keep (size query)")
    ws = _buf(nbytes.value, torch.uint8, WS_S)
    assert _L().cddmsl_nms_anyorder(_p(boxes), _p(scores), _p(keep), _p(nkeep), K, thr, _p(ws), ctypes.byref(nbytes), _st()) == 0
    ref = E.anyorder_ref(boxes_h, scores_h, thr)
    k, nk = _host(keep), _host(nkeep)
    assert nk[0] == len(ref) and (nk[1:] == KEEP_S).all()
    assert np.array_equal(k[:len(ref)], ref), (k[:len(ref)].tolist(), ref.tolist())
    assert (k[len(ref):K] == -1).all(), "keep[nkeep:K] must be -1"
    assert (k[K:] == KEEP_S).all()
    _untouched(ws, nbytes.value, WS_S, "workspace")


@pytest.mark.parametrize("name", list(NMS))
def test_nms_anyorder(name):
    """image 0 of every NMS case under a seeded permutation with tied scores (K = 1: clustered_n1)"""
    _run_anyorder(*E.anyorder_inputs(NMS[name]), NMS[name]["thr"])


def test_nms_anyorder_k0():
    _run_anyorder(np.zeros((0, 4), np.float32), np.zeros(0, np.float32), 0.5)


# ================================================================================================================= sort
@pytest.mark.parametrize("c", E.sort_cases(), ids=lambda c: c["name"])
def test_sort_desc(c):
    """order and keys bit for bit, except that a -0.0 key may come back as +0.0 (it is documented to)"""
    N, total = c["keys"].shape
    n = N * total
    keys = _dev(c["keys"])
    keys_out, idx, order = _buf(n, torch.float32, float("nan")), _buf(n, torch.int32, KEEP_S), _buf(n, torch.int32, KEEP_S)
    nbytes = ctypes.c_size_t(0)
    assert _L().cddmsl_sort_desc(_p(keys), _p(keys_out), _p(idx), _p(order), None, N, total, None, ctypes.byref(nbytes), _st()) == 0
    ws = _buf(nbytes.value, torch.uint8, WS_S)
    assert _L().cddmsl_sort_desc(_p(keys), _p(keys_out), _p(idx), _p(order), None, N, total, _p(ws), ctypes.byref(nbytes), _st()) == 0
    ref = E.sort_ref(c["keys"])
    got = _host(order)
    assert np.array_equal(got[:n].reshape(N, total), ref), (c["name"], got[:n].reshape(N, total)[0, :12].tolist(), ref[0, :12].tolist())
    assert (got[n:] == KEEP_S).all() and (_host(idx)[n:] == KEEP_S).all()
    g = _host(keys_out).view(np.uint32)
    e = np.take_along_axis(c["keys"], ref.astype(np.int64), 1).reshape(-1).view(np.uint32)
    assert (np.isnan(_host(keys_out)[n:])).all()
    assert ((g[:n] == e) | ((e == 0x80000000) & (g[:n] == 0))).all(), c["name"]
    _untouched(ws, nbytes.value, WS_S, "workspace")


# ================================================================================================================= matcher
def _thr(c):
    t = [float(x) for x in c["thresholds"]] + [0.0]
    l = [int(x) for x in c["labels"]] + [0]
    return len(c["thresholds"]), t[0], t[1], l[0], l[1], l[2]


@pytest.mark.parametrize("c", E.match_cases(), ids=lambda c: c["name"])
def test_iou_match(c):
    G, P = c["gt"].shape[0], c["preds"].shape[0]
    gt, preds = _dev(c["gt"]), _dev(c["preds"])
    matches, labels, best = _buf(P, torch.int64, KEEP_S), _buf(P, torch.int8, LAB_S), _buf(max(G, 1), torch.int32, KEEP_S)
    assert _L().cddmsl_iou_match(_p(gt), G, _p(preds), P, _p(matches), _p(labels), _p(best), *_thr(c), int(c["allow_low_quality"]), _st()) == 0
    m, l = E.matcher_ref(c["gt"], c["preds"], c["thresholds"], c["labels"], c["allow_low_quality"])
    gm, gl = _host(matches), _host(labels)
    assert np.array_equal(gm[:P], m), (c["name"], np.nonzero(gm[:P] != m)[0][:8].tolist())
    assert np.array_equal(gl[:P], l), (c["name"], np.nonzero(gl[:P] != l)[0][:8].tolist())
    assert (gm[P:] == KEEP_S).all() and (gl[P:] == LAB_S).all() and (_host(best)[max(G, 1):] == KEEP_S).all()


@pytest.mark.parametrize("c", E.match_batched_cases(), ids=lambda c: c["name"])
def test_iou_match_batched(c):
    """against the reference image by image, not against the per-image entry point"""
    ng = [len(g) for g in c["gts"]]
    N, totalG = len(ng), sum(ng)
    gt = _dev(np.concatenate(c["gts"]))
    gt_off = _dev(np.cumsum([0] + ng), np.int32)
    preds = _dev(c["preds"])
    if c["counts"] is None:
        P, pred_off, nout = len(c["preds"]), None, N * len(c["preds"])
    else:
        P, pred_off, nout = max(c["counts"]), _dev(np.cumsum([0] + list(c["counts"])), np.int32), sum(c["counts"])
    matches, labels, best = _buf(nout, torch.int64, KEEP_S), _buf(nout, torch.int8, LAB_S), _buf(max(totalG, 1), torch.int32, KEEP_S)
    assert _L().cddmsl_iou_match_batched(_p(gt), _p(gt_off), _p(preds), _p(pred_off), _p(matches), _p(labels), _p(best), N, P, max(ng), totalG,
                                         *_thr(c), int(c["allow_low_quality"]), _st()) == 0
    m, l = E.matcher_ref_batched(c["gts"], c["preds"], c["counts"], c["thresholds"], c["labels"], c["allow_low_quality"])
    gm, gl = _host(matches), _host(labels)
    assert np.array_equal(gm[:nout], m.reshape(-1)), (c["name"], np.nonzero(gm[:nout] != m.reshape(-1))[0][:8].tolist())
    assert np.array_equal(gl[:nout], l.reshape(-1)), (c["name"], np.nonzero(gl[:nout] != l.reshape(-1))[0][:8].tolist())
    assert (gm[nout:] == KEEP_S).all() and (gl[nout:] == LAB_S).all() and (_host(best)[max(totalG, 1):] == KEEP_S).all()


# ================================================================================================================= anchors, decode
@pytest.mark.parametrize("Hf,Wf,offset", [(5, 7, 0.0), (5, 7, 0.5), (12, 17, 0.5), (1, 1, 0.0)])
def test_anchors(Hf, Wf, offset):
    """one rounded addition of exact operands: the float64 sum rounded to f32, bit for bit"""
    cell = E.cell_anchors()
    total = Hf * Wf * cell.shape[0]
    out = _buf(total * 4, torch.float32, float("nan"))
    assert _L().cddmsl_anchors(_p(_dev(cell)), _p(out), Hf, Wf, cell.shape[0], 16.0, offset, _st()) == 0
    got = _host(out)
    assert np.array_equal(got[:total * 4].reshape(-1, 4), E.anchors_ref(cell, Hf, Wf, 16.0, offset).astype(np.float32))
    assert np.isnan(got[total * 4:]).all()


@pytest.mark.parametrize("c", E.decode_cases(), ids=lambda c: c["name"])
def test_rpn_decode(c):
    """every coordinate of a finite box within the derived bound of the float64 value (the largest error and its bound are printed);
    valid == 2 exactly on the non-finite rows, and the float64 verdict wherever width and height are further than the bound from
    min_size"""
    N, total = c["order"].shape
    topk, n = c["topk"], N * c["topk"]
    boxes, valid = _buf(n * 4, torch.float32, float("nan")), _buf(n, torch.uint8, LAB_S)
    assert _L().cddmsl_rpn_decode(_p(_dev(c["order"])), _p(_dev(c["deltas"])), _p(_dev(c["cell"])), _p(_dev(c["img_hw"])), _p(boxes), _p(valid),
                                  N, c["Hf"], c["Wf"], c["A"], topk, c["stride"], c["offset"], *[float(w) for w in c["weights"]],
                                  c["scale_clamp"], c["min_size"], _st()) == 0
    d = E.decode_ref(c)
    gb, gv = _host(boxes), _host(valid)
    assert np.isnan(gb[n * 4:]).all() and (gv[n:] == LAB_S).all()
    gb, gv = gb[:n * 4].reshape(N, topk, 4).astype(np.float64), gv[:n].reshape(N, topk)
    assert not np.isnan(gb).any(), "a coordinate was not written"
    assert set(np.unique(gv)) <= {0, 1, 2}
    f = d["finite"]
    err = np.abs(gb - d["boxes"])[f]
    w = int(np.argmax(err - d["bound"][f]))
    print(f"rpn_decode {c['name']}: largest |error| {err.max():.3e} px (largest bound {d['bound'][f].max():.3e}); "
          f"worst error / bound {np.max(err[d['bound'][f] > 0] / d['bound'][f][d['bound'][f] > 0]):.3f}; "
          f"entries excused from the valid check {int(d['ambiguous'].sum())} of {f.size}")
    assert (err <= d["bound"][f]).all(), (c["name"], float(err.reshape(-1)[w]), float(d["bound"][f].reshape(-1)[w]))
    assert np.array_equal(gv == 2, ~f), (c["name"], "valid == 2 must mark exactly the non-finite rows", np.argwhere((gv == 2) != ~f)[:4].tolist())
    chk = f & ~d["ambiguous"]
    assert np.array_equal(gv[chk], d["valid"][chk]), c["name"]
    assert d["ambiguous"].mean() <= E.DECODE_SKIP_CAP


# ================================================================================================================= refusals
def test_documented_refusals_leave_the_outputs_alone():
    """each returns an error code before any launch: the sentinel-filled outputs stay as they were"""
    L, st = _L(), _st()
    d = _dev(np.zeros(64, np.float32))
    keep, nkeep = _buf(8, torch.int32, KEEP_S), _buf(2, torch.int32, KEEP_S)
    assert L.cddmsl_nms(_p(d), _p(d), _p(d), _p(keep), _p(nkeep), 1, 64 * 192 + 1, 0.5, 4, st) != 0          # n > 64 * 192
    assert L.cddmsl_nms(_p(d), _p(d), _p(d), _p(keep), _p(nkeep), 1, 4, 0.5, 0, st) != 0                     # max_keep = 0
    keep64 = _buf(8, torch.int64, KEEP_S)
    nb = ctypes.c_size_t(0)
    assert L.cddmsl_nms_anyorder(_p(d), _p(d), _p(keep64), _p(nkeep), 64 * 192 + 1, 0.5, None, ctypes.byref(nb), st) != 0
    assert L.cddmsl_nms_anyorder(_p(d), _p(d), _p(keep64), _p(nkeep), 8, 0.5, None, ctypes.byref(nb), st) == 0 and nb.value > 0
    ws = _buf(nb.value, torch.uint8, WS_S)
    small = ctypes.c_size_t(nb.value - 1)
    assert L.cddmsl_nms_anyorder(_p(d), _p(d), _p(keep64), _p(nkeep), 8, 0.5, _p(ws), ctypes.byref(small), st) != 0   # temp_bytes too small
    boxes, valid = _buf(16, torch.float32, float("nan")), _buf(4, torch.uint8, LAB_S)
    assert L.cddmsl_rpn_decode(_p(d), _p(d), _p(d), _p(d), _p(boxes), _p(valid), 1, 1, 1, 3, 4, 16.0, 0.0, 1.0, 1.0, 1.0, 1.0, 4.0, 0.0, st) != 0  # topk > total
    matches, labels, best = _buf(4, torch.int64, KEEP_S), _buf(4, torch.int8, LAB_S), _buf(4, torch.int32, KEEP_S)
    assert L.cddmsl_iou_match(_p(d), 1, _p(d), 4, _p(matches), _p(labels), _p(best), 3, 0.3, 0.7, 0, -1, 1, 1, st) != 0            # nthr = 3
    off = _dev(np.array([0, 1], np.int32))
    assert L.cddmsl_iou_match_batched(_p(d), _p(off), _p(d), None, _p(matches), _p(labels), _p(best), 1, 4, 1, 1, 3, 0.3, 0.7, 0, -1, 1, 1, st) != 0
    keys_out, idx, order = _buf(8, torch.float32, float("nan")), _buf(8, torch.int32, KEEP_S), _buf(8, torch.int32, KEEP_S)
    sb = ctypes.c_size_t(0)
    assert L.cddmsl_sort_desc(_p(d), _p(keys_out), _p(idx), _p(order), None, 1, 8, None, ctypes.byref(sb), st) == 0 and sb.value > 0
    ws2 = _buf(sb.value, torch.uint8, WS_S)
    small = ctypes.c_size_t(sb.value - 1)
    assert L.cddmsl_sort_desc(_p(d), _p(keys_out), _p(idx), _p(order), None, 1, 8, _p(ws2), ctypes.byref(small), st) != 0          # temp_bytes too small
    for t, fill in ((keep, KEEP_S), (nkeep, KEEP_S), (keep64, KEEP_S), (matches, KEEP_S), (best, KEEP_S), (idx, KEEP_S), (order, KEEP_S),
                    (labels, LAB_S), (valid, LAB_S), (ws, WS_S), (ws2, WS_S), (boxes, float("nan")), (keys_out, float("nan"))):
        _untouched(t, 0, fill, "a refused call")
