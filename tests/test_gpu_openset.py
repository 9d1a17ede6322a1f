"""cddmsl_openset_logits / cddmsl_openset_select (cddmsl_amd/csrc/openset.hip) against the float64 references and the derived
error model of tests/openset_ref.py, which tests/test_openset_host.py ties to the reference's own FastRCNNOutputLayers first.  The
kernels are called through the raw C-ABI with outputs longer than documented and pre-filled with sentinels; then the Python layers:
FastRCNNOutputLayers.inference on the reference fixture, open-set pointed at the training vocabulary against the closed-set path,
batched_nms_grouped, class-agnostic box-regression losses, and tools/detect_open_vocab.py end to end.

  test_logits_grid      R in {1, 31, 32, 33, 70} x K in {1, 31, 32, 33, 37, 63, 64, 127, 128, 129, 130, 257} x D in {4, 8, 12, 64}: one
                        below, at and above the row panel (32), the wave's and the workgroup's class tile (32, 128), the statistics
                        wave's 64 logits (K + 1 = 64 at K = 63) and the MFMA step (8; D = 4 and 12 end on a half step).  A row of
                        zeros (the eps branch) wherever R > 1; ld = K + 1 and ld = K + 6; logits[:, K] == 0 exactly; padding columns
                        untouched; the statistics within their bounds; a second call bit-equal.
  test_select           the named shapes of openset_ref.SHAPES x thresholds (0.05, 0.001 at T = 0.01; 0.0 at T = 0.05) x objectness
                        off / on, class-agnostic and class-specific boxes, a negative objectness and an infinite box coordinate
                        wherever R >= 31: the candidate list equal in content and order, scores inside their intervals, boxes bit-equal.
  test_large            R = 300, K = 1203, D = 1024, threshold 0.05: entries of the ambiguous set may be present or absent.

Measured on one MI355X (34 tests in 8 s), worst observed error as a fraction of its bound over all shapes: logits 0.273, row maximum
0.244, sum of exponentials 0.042, scores 0.135; the large case: 584 candidates, none ambiguous, all matched, scores at 0.011 of their
bound; the fixture end to end: boxes within 7.6e-6 and scores within 3.8e-6 (2.3e-6 with objectness) of the reference's, against the
1e-4 allowed; class-agnostic losses: L1 0 (bit-equal), GIoU loss 0.024 and gradient 0.078 of exact_box_losses' bounds.
"""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import openset_ref as X

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "ref_openset.npz"))
TAIL = 64
NANF = float("nan")
WORST = {}


def _hip():
    from cddmsl_amd import hip
    return hip


def _L():
    return _hip()._L()


def _st():
    return _hip().stream_ptr()


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def _dev(a, dtype=None):
    a = np.array(a if dtype is None else np.asarray(a, dtype), order="C")      # a copy: the shared cases are read-only arrays
    if a.size == 0:
        a = np.zeros(4, a.dtype)
    return torch.from_numpy(a).to(DEV)


def _buf(n, dtype, fill):
    return torch.full((n + TAIL,), fill, device=DEV, dtype=dtype)


def _host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def _note(key, ratio):
    WORST[key] = max(WORST.get(key, 0.0), float(ratio))


def _ratio(err, bound):
    """worst err / bound; an error where the bound is 0 must be 0"""
    assert (err[bound == 0] == 0).all()
    pos = bound > 0
    return float((err[pos] / bound[pos]).max()) if pos.any() else 0.0


# ------------------------------------------------------------------------------------------------------------ raw calls
def call_logits(x, wn, K=None, D=None, ld=None, T=X.T_DEFAULT, R=None):
    R = x.shape[0] if R is None else R
    D = x.shape[1] if D is None else D
    K = wn.shape[0] if K is None else K
    ld = K + 1 if ld is None else ld
    logits = _buf(max(R * max(ld, 1), 0), torch.float32, NANF)
    stats = _buf(2 * R, torch.float32, NANF)
    dx, dw = _dev(x), _dev(wn)                     # (held until the call is enqueued and the outputs are read back)
    rc = _L().cddmsl_openset_logits(_p(dx), _p(dw), _p(logits), _p(stats), R, D, K, ld, T, X.EPS, _st())
    torch.cuda.synchronize()
    return rc, logits, stats


def call_select(logits, stats, ld, boxes, obj, R, K, thresh, cap, ldb=None, img=(X.IMG_H, X.IMG_W)):
    """size query + run -> (rc, dict of the sentinel-filled outputs)"""
    ldb = boxes.shape[1] if ldb is None else ldb
    o = dict(row=_buf(cap, torch.int32, -7), cls=_buf(cap, torch.int32, -7), score=_buf(cap, torch.float32, NANF),
             box=_buf(4 * cap, torch.float32, NANF), valid=_buf(R, torch.uint8, 9), count=_buf(1, torch.int32, -7))
    db, do = _dev(boxes), (None if obj is None else _dev(obj))
    head = (_p(logits), _p(stats), ld, _p(db), ldb, _p(do), R, K, float(img[0]), float(img[1]), float(thresh), _p(o["row"]), _p(o["cls"]),
            _p(o["score"]), _p(o["box"]), _p(o["valid"]), _p(o["count"]), cap)
    nbytes = ctypes.c_size_t(12345)
    rc = _L().cddmsl_openset_select(*head, None, ctypes.byref(nbytes), _st())
    if rc != 0:
        return rc, o
    assert (_host(o["count"]) == -7).all() and (_host(o["valid"]) == 9).all(), "the size query wrote an output"
    ws = _buf(nbytes.value, torch.uint8, 0x5A)
    rc = _L().cddmsl_openset_select(*head, _p(ws), ctypes.byref(nbytes), _st())
    assert (_host(ws)[nbytes.value:] == 0x5A).all(), "the scratch buffer was written past the size the query returned"
    return rc, o


def _untouched(o, R, n, cap):
    w = min(n, cap)
    assert (_host(o["row"])[w:] == -7).all() and (_host(o["cls"])[w:] == -7).all()
    assert np.isnan(_host(o["score"])[w:]).all() and np.isnan(_host(o["box"])[4 * w:]).all()
    assert (_host(o["valid"])[R:] == 9).all() and (_host(o["count"])[1:] == -7).all()


# ----------------------------------------------------------------------------------------------------------- the logits
def _check_logits(x, wn, ld, T=X.T_DEFAULT, tag=""):
    R, K = x.shape[0], wn.shape[0]
    z, bound = X.ref_logits(x, wn, T)
    rc, logits, stats = call_logits(x, wn, ld=ld, T=T)
    assert rc == 0
    lg, st = _host(logits), _host(stats)
    got = lg[:R * ld].reshape(R, ld)
    assert np.isnan(got[:, K + 1:]).all() and np.isnan(lg[R * ld:]).all(), (tag, "a padding column or the tail was written")
    assert np.isnan(st[2 * R:]).all()
    assert (got[:, K] == 0).all() and not np.signbit(got[:, K]).any(), (tag, "the background logit must be exactly +0")
    err = np.abs(got[:, :K + 1].astype(np.float64) - z)
    assert (err <= bound).all(), (tag, float((err - bound).max()))
    _note("logit", _ratio(err, bound))
    m, l = X.ref_stats(z)
    E, rel_l, _ = X.stats_bounds(z, bound)
    s = st[:2 * R].reshape(R, 2).astype(np.float64)
    assert (np.abs(s[:, 0] - m) <= E).all(), (tag, "row maximum")
    assert (np.abs(s[:, 1] - l) <= rel_l * l).all(), (tag, "sum of exponentials", float((np.abs(s[:, 1] - l) / (rel_l * l)).max()))
    _note("stat m", _ratio(np.abs(s[:, 0] - m), E))
    _note("stat l", _ratio(np.abs(s[:, 1] - l), rel_l * l))
    rc2, logits2, stats2 = call_logits(x, wn, ld=ld, T=T)
    assert rc2 == 0 and np.array_equal(_host(logits2), lg, equal_nan=True) and np.array_equal(_host(stats2), st, equal_nan=True)
    return logits, stats, z, bound


@pytest.mark.parametrize("D", [4, 8, 12, 64])
def test_logits_grid(D):
    for R in (1, 31, 32, 33, 70):
        for K in (1, 31, 32, 33, 37, 63, 64, 127, 128, 129, 130, 257):
            inp = X.make_inputs(1000 + R + K, R, K, D)
            x = inp["x"].copy()
            if R > 1:
                x[R // 2] = 0                      # 1 / max(0, eps): the eps branch, every logit of the row 0
            ld = K + 1 if (R + K) % 2 else K + 6
            _check_logits(x, inp["wn"], ld, tag=f"R{R} K{K} D{D} ld{ld}")
    print(f"logits D={D}: worst |err| / bound so far " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(WORST.items())))


def test_zero_row_gives_zero_logits_and_uniform_stats():
    inp = X.make_inputs(5, 3, 37, 64)
    x = inp["x"].copy()
    x[1] = 0
    rc, logits, stats = call_logits(x, inp["wn"])
    assert rc == 0
    assert (_host(logits)[38:76] == 0).all()
    assert np.array_equal(_host(stats)[2:4], np.asarray([0.0, 38.0], np.float32))


# -------------------------------------------------------------------------------------------------------- the selection
def _modified(c):
    """the case's boxes and objectness with, where it has the rows, a negative objectness and an infinite box coordinate"""
    boxes, obj = c["boxes"].copy(), c["obj"].copy()
    if boxes.shape[0] >= 31:
        obj[2] = -0.5
        boxes[5, boxes.shape[1] - 3] = np.inf
    return boxes, obj


def _check_select(o, ref, R, cap, tag):
    n = len(ref["rows"])
    assert int(_host(o["count"])[0]) == n, (tag, int(_host(o["count"])[0]), n)
    assert np.array_equal(_host(o["valid"])[:R], ref["valid"].astype(np.uint8)), (tag, "valid")
    w = min(n, cap)
    assert np.array_equal(_host(o["row"])[:w], ref["rows"][:w]) and np.array_equal(_host(o["cls"])[:w], ref["cls"][:w]), (tag, "candidate list")
    sc = _host(o["score"])[:w].astype(np.float64)
    assert ((ref["lo"][:w] <= sc) & (sc <= ref["hi"][:w])).all(), (tag, "a score outside its interval")
    half = np.maximum(ref["hi"][:w] - ref["scores"][:w], ref["scores"][:w] - ref["lo"][:w])
    _note("score", _ratio(np.abs(sc - ref["scores"][:w]), half))
    assert np.array_equal(_host(o["box"])[:4 * w].reshape(-1, 4), ref["boxes"][:w]), (tag, "boxes")
    _untouched(o, R, n, cap)


@pytest.mark.parametrize("name", list(X.SHAPES))
def test_select(name):
    c = X.case(name)
    R, K, D, spec = X.SHAPES[name]
    boxes, obj = _modified(c)
    total = 0
    for th, T, use_obj in X.configs():
        rc, logits, stats = call_logits(c["x"], c["wn"], T=T)
        assert rc == 0
        ref = X.ref_select(c["z"][T], c["zbound"][T], boxes, obj if use_obj else None, th)
        assert len(ref["ambiguous"]) == 0
        rc, o = call_select(logits, stats, K + 1, boxes, obj if use_obj else None, R, K, th, R * K)
        assert rc == 0
        _check_select(o, ref, R, R * K, f"{name} thresh {th} objectness {use_obj}")
        if th == 0.0:
            assert len(ref["rows"]) == int(ref["valid"].sum()) * K      # every class of every valid row
        if R >= 31:
            assert not ref["valid"][5] and ref["valid"][2] == (not use_obj)
        total += len(ref["rows"])
    assert total > 0
    print(f"select {name}: worst |score err| / bound so far {WORST.get('score', 0.0):.3f}")


def test_select_with_row_pitch():
    """logits with ld > K + 1 feed the selection through the same pitch"""
    c = X.case("r70_k37_d64")
    rc, logits, stats = call_logits(c["x"], c["wn"], ld=44)
    assert rc == 0
    ref = X.ref_select(c["z"][0.01], c["zbound"][0.01], c["boxes"], None, 0.05)
    rc, o = call_select(logits, stats, 44, c["boxes"], None, 70, 37, 0.05, 70 * 37)
    assert rc == 0
    _check_select(o, ref, 70, 70 * 37, "ld 44")


def test_underflowed_probability_is_not_selected():
    u = X.underflow_case()
    z, bound = X.ref_logits(u["x"], u["wn"])
    rc, logits, stats = call_logits(u["x"], u["wn"])
    assert rc == 0
    for obj in (None, u["obj"]):
        ref = X.ref_select(z, bound, u["boxes"], obj, 0.0)
        assert len(ref["ambiguous"]) == 0 and len(ref["rows"]) == 3
        rc, o = call_select(logits, stats, 3, u["boxes"], obj, 2, 2, 0.0, 4)
        assert rc == 0
        _check_select(o, ref, 2, 4, "underflow")


def test_no_candidate_and_r0():
    c = X.case("r33_k33_d12")
    rc, logits, stats = call_logits(c["x"], c["wn"])
    rc, o = call_select(logits, stats, 34, c["boxes"], None, 33, 33, 2.0, 16)
    assert rc == 0 and int(_host(o["count"])[0]) == 0 and (_host(o["valid"])[:33] == 1).all()
    _untouched(o, 33, 0, 16)
    # R = 0: success, nothing launched by the logits call; the selection writes count = 0 only
    rc, lg, st = call_logits(c["x"], c["wn"], R=0)
    assert rc == 0 and np.isnan(_host(lg)).all() and np.isnan(_host(st)).all()
    rc, o = call_select(logits, stats, 34, c["boxes"], None, 0, 33, 0.05, 16)
    assert rc == 0 and int(_host(o["count"])[0]) == 0
    _untouched(o, 0, 0, 16)
    hip = _hip()
    e = torch.empty((0, 12), device=DEV)
    lg0, st0 = hip.openset_logits(e, _dev(c["wn"]), 0.01)
    assert tuple(lg0.shape) == (0, 34) and tuple(st0.shape) == (0, 2)
    rows, cls, sc, bx, valid = hip.openset_select(lg0, st0, 33, torch.empty((0, 4), device=DEV), None, 100, 100, 0.05)
    assert rows.numel() == cls.numel() == sc.numel() == bx.numel() == valid.numel() == 0


def test_cap_one_below_the_count():
    c = X.case("r70_k37_d64")
    ref = X.ref_select(c["z"][0.01], c["zbound"][0.01], c["boxes"], None, 0.001)
    n = len(ref["rows"])
    assert n > 70
    rc, logits, stats = call_logits(c["x"], c["wn"])
    rc, o = call_select(logits, stats, 38, c["boxes"], None, 70, 37, 0.001, n - 1)
    assert rc == 0
    _check_select(o, ref, 70, n - 1, "cap n - 1")             # the full count, the first n - 1 entries, nothing behind them
    hip = _hip()
    lg, st = hip.openset_logits(_dev(c["x"]), _dev(c["wn"]), 0.01)
    with pytest.raises(ValueError):
        hip.openset_select(lg, st, 37, _dev(c["boxes"]), None, X.IMG_H, X.IMG_W, 0.001, cap=n - 1)
    rows, cls, sc, bx, valid = hip.openset_select(lg, st, 37, _dev(c["boxes"]), None, X.IMG_H, X.IMG_W, 0.001, cap=n)
    assert np.array_equal(_host(rows), ref["rows"]) and np.array_equal(_host(cls), ref["cls"])
    # the default cap holds every list a softmax row can produce
    assert hip.openset_cap(70, 37, 0.05, False) == 70 * 20 and hip.openset_cap(70, 37, 0.001, False) == 70 * 37
    assert hip.openset_cap(70, 37, 0.0, False) == 70 * 37 and hip.openset_cap(70, 37, 0.05, True) == 70 * 37


def test_large():
    """R = 300, K = 1203, D = 1024, threshold 0.05, no objectness: every certainly-selected entry present and in order, nothing
    outside the certain and the ambiguous entries, the ambiguous set at most 5 % of the reference's candidates"""
    c = X.case("large")
    R, K = X.LARGE["R"], X.LARGE["K"]
    z, bound = c["z"][0.01], c["zbound"][0.01]
    logits, stats, _, _ = _check_logits(c["x"], c["wn"], K + 1, tag="large")
    ref = X.ref_select(z, bound, c["boxes"], None, X.LARGE["thresh"])
    n, amb = len(ref["rows"]), {(int(r), int(k)) for r, k in ref["ambiguous"]}
    assert n > 0 and len(amb) <= 0.05 * n, (len(amb), n)
    cap = _hip().openset_cap(R, K, X.LARGE["thresh"], False)
    rc, o = call_select(logits, stats, K + 1, c["boxes"], None, R, K, X.LARGE["thresh"], cap)
    assert rc == 0
    cnt = int(_host(o["count"])[0])
    got = list(zip(_host(o["row"])[:cnt].tolist(), _host(o["cls"])[:cnt].tolist()))
    assert got == sorted(got) and len(set(got)) == cnt, "row-major order"
    certain = list(zip(ref["rows"].tolist(), ref["cls"].tolist()))
    assert [g for g in got if g not in amb] == certain
    pos = {g: i for i, g in enumerate(got)}
    idx = np.asarray([pos[g] for g in certain])
    sc = _host(o["score"])[idx].astype(np.float64)
    assert ((ref["lo"] <= sc) & (sc <= ref["hi"])).all()
    assert np.array_equal(_host(o["box"])[:4 * cnt].reshape(-1, 4)[idx], ref["boxes"])
    half = np.maximum(ref["hi"] - ref["scores"], ref["scores"] - ref["lo"])
    print(f"large: {n} certain candidates, {len(amb)} ambiguous, {cnt} selected; worst |score err| / bound "
          f"{_ratio(np.abs(sc - ref['scores']), half):.3f}; logits {WORST['logit']:.3f}")


# ------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_write_nothing():
    c = X.case("r33_k33_d12")
    x, wn = c["x"], c["wn"]
    for kw in (dict(D=6), dict(D=0), dict(K=0), dict(K=16385, ld=16400), dict(ld=33), dict(R=-1), dict(T=0.0)):
        rc, lg, st = call_logits(x, wn, **kw)
        assert rc == 1, kw
        assert np.isnan(_host(lg)).all() and np.isnan(_host(st)).all(), kw
    rc, logits, stats = call_logits(x, wn)
    assert rc == 0
    good = dict(ld=34, R=33, K=33, ldb=4)
    for kw in (dict(K=0), dict(K=16385), dict(ld=33), dict(ldb=8), dict(ldb=0), dict(ldb=4 * 33 + 4), dict(R=-1)):
        a = dict(good, **kw)
        rc, o = call_select(logits, stats, a["ld"], c["boxes"], None, a["R"], a["K"], 0.05, 16, ldb=a["ldb"])
        assert rc == 1, kw
        assert (_host(o["count"]) == -7).all() and (_host(o["valid"]) == 9).all() and (_host(o["row"]) == -7).all(), kw
    # misaligned vector operands: x / wn of the logits call, boxes / cand_box of the selection, 4 bytes off a 16-byte boundary
    dx, dw = torch.zeros(33 * 12 + 8, device=DEV), torch.zeros(33 * 12 + 8, device=DEV)
    for ox, ow in ((4, 0), (0, 4)):
        lg, st = _buf(33 * 34, torch.float32, NANF), _buf(66, torch.float32, NANF)
        rc = _L().cddmsl_openset_logits(ctypes.c_void_p(dx.data_ptr() + ox), ctypes.c_void_p(dw.data_ptr() + ow), _p(lg), _p(st), 33, 12, 33, 34,
                                        0.01, X.EPS, _st())
        assert rc == 1 and np.isnan(_host(lg)).all() and np.isnan(_host(st)).all()
    bx = torch.zeros(33 * 4 + 8, device=DEV)
    for ob, oc in ((4, 0), (0, 4)):
        o = dict(row=_buf(16, torch.int32, -7), cls=_buf(16, torch.int32, -7), score=_buf(16, torch.float32, NANF),
                 box=_buf(64, torch.float32, NANF), valid=_buf(33, torch.uint8, 9), count=_buf(1, torch.int32, -7))
        ws, nb = _buf(4096, torch.uint8, 0x5A), ctypes.c_size_t(4096)
        rc = _L().cddmsl_openset_select(_p(logits), _p(stats), 34, ctypes.c_void_p(bx.data_ptr() + ob), 4, None, 33, 33, 120.0, 160.0, 0.05,
                                        _p(o["row"]), _p(o["cls"]), _p(o["score"]), ctypes.c_void_p(o["box"].data_ptr() + oc), _p(o["valid"]),
                                        _p(o["count"]), 16, _p(ws), ctypes.byref(nb), _st())
        assert rc == 1 and (_host(o["count"]) == -7).all() and (_host(o["valid"]) == 9).all() and np.isnan(_host(o["box"])).all()
    # a scratch buffer one byte short
    o = dict(row=_buf(16, torch.int32, -7), cls=_buf(16, torch.int32, -7), score=_buf(16, torch.float32, NANF), box=_buf(64, torch.float32, NANF),
             valid=_buf(33, torch.uint8, 9), count=_buf(1, torch.int32, -7))
    db = _dev(c["boxes"])
    head = (_p(logits), _p(stats), 34, _p(db), 132, None, 33, 33, 120.0, 160.0, 0.05, _p(o["row"]), _p(o["cls"]), _p(o["score"]),
            _p(o["box"]), _p(o["valid"]), _p(o["count"]), 16)
    nbytes = ctypes.c_size_t(0)
    assert _L().cddmsl_openset_select(*head, None, ctypes.byref(nbytes), _st()) == 0 and nbytes.value > 0
    ws = _buf(nbytes.value, torch.uint8, 0x5A)
    short = ctypes.c_size_t(nbytes.value - 1)
    assert _L().cddmsl_openset_select(*head, _p(ws), ctypes.byref(short), _st()) == 1
    assert (_host(o["count"]) == -7).all() and (_host(ws) == 0x5A).all()


# ------------------------------------------------------------------------------------------------------- the head, end to end
def _cfg(tmp_path, emb, k_train, dim, over=()):
    from cddmsl_amd.config import get_cfg
    path = os.path.join(str(tmp_path), f"emb{len(os.listdir(str(tmp_path)))}.pth")
    torch.save(torch.from_numpy(np.array(emb, order="C")), path)
    cfg = get_cfg()
    cfg.merge_from_list(["MODEL.CLIP.USE_TEXT_EMB_CLASSIFIER", True, "MODEL.CLIP.TEXT_EMB_DIM", dim, "MODEL.ROI_HEADS.NUM_CLASSES", k_train,
                         "MODEL.COMPUTE_DTYPE", "f32", "MODEL.CLIP.OPENSET_TEST_TEXT_EMB_PATH", path, *over])
    return cfg


def _head(cfg, dim):
    from cddmsl_amd.modeling.roi_heads import FastRCNNOutputLayers
    from cddmsl_amd.structures import ShapeSpec
    return FastRCNNOutputLayers(cfg, ShapeSpec(channels=dim, height=1, width=1))


def _proposals(boxes, obj, size):
    from cddmsl_amd.structures import Boxes, Instances
    p = Instances(tuple(size))
    p.proposal_boxes, p.objectness_logits = Boxes(_dev(boxes)), _dev(obj)
    return p


@pytest.mark.parametrize("name", ["plain", "rpn"])
def test_inference_reproduces_the_reference_fixture(name, tmp_path):
    """FastRCNNOutputLayers (eval, open-set file of 37 classes on a head trained for 5, class-agnostic deltas) on the fixture's
    features and proposals: the reference's classes and kept indices; boxes and scores within atol 1e-4, rtol 0 -- the tolerance
    tests/test_gpu_ops.py applies to the computed quantities of ref_inference.npz (its torch.equal checks are on values that
    inference only gathers; here both are computed, the boxes by the head's GEMM and the decoder, the scores by the softmax)"""
    cfg = _cfg(tmp_path, GOLD["test_emb"], 5, 64, ["MODEL.ROI_BOX_HEAD.CLS_AGNOSTIC_BBOX_REG", True, "MODEL.CLIP.MULTIPLY_RPN_SCORE", name == "rpn"])
    head = _head(cfg, 64)
    with torch.no_grad():
        head.cls_score.weight.copy_(torch.from_numpy(GOLD["cls_score"]))
        head.bbox_pred.weight.copy_(torch.from_numpy(GOLD["bbox_w"]))
        head.bbox_pred.bias.copy_(torch.from_numpy(GOLD["bbox_b"]))
    head.to(DEV).eval()
    props = [_proposals(GOLD["proposal_boxes"], GOLD["objectness"], GOLD["image_size"].tolist())]
    with torch.no_grad():
        pred = head(torch.from_numpy(GOLD["feats"]).to(DEV))
        assert len(pred) == 3 and tuple(pred[0].shape) == (70, 38) and tuple(pred[1].shape) == (70, 4)
        z, bound = X.ref_logits(GOLD["feats"], _host(head._test_text_emb()))               # the unit rows the kernel was given
        assert (np.abs(_host(pred[0]).astype(np.float64) - z) <= bound).all()
        assert np.allclose(_host(pred[1]), GOLD["deltas"], rtol=0, atol=1e-5)
        inst, kept = head.inference(pred, props)
        inst2, kept2 = head.inference(pred, props, proposal_indices=True)
    assert np.array_equal(_host(inst[0].pred_classes), GOLD[f"{name}/pred_classes"])
    assert np.array_equal(_host(kept[0]), GOLD[f"{name}/kept"])
    db = np.abs(_host(inst[0].pred_boxes.tensor) - GOLD[f"{name}/pred_boxes"]).max()
    ds = np.abs(_host(inst[0].scores) - GOLD[f"{name}/scores"]).max()
    print(f"fixture {name}: max |box diff| {db:.3e}, max |score diff| {ds:.3e}")
    assert db <= 1e-4 and ds <= 1e-4
    # and every score inside the error model's interval around the float64 score of its (row, class) entry
    _, lo, hi = X.score_interval(z, bound, GOLD["objectness"] if name == "rpn" else None)
    rows, got = _host(kept2[0]), _host(inst[0].scores).astype(np.float64)
    assert ((lo[rows, _host(inst[0].pred_classes)] <= got) & (got <= hi[rows, _host(inst[0].pred_classes)])).all()
    # proposal_indices: rows of the input -- one more than the finite-row count from the dropped proposal (row 7) on
    k1, k2 = _host(kept[0]), _host(kept2[0])
    assert np.array_equal(k2, k1 + (k1 >= 7)) and torch.equal(inst2[0].pred_classes, inst[0].pred_classes)
    assert head.training is False
    head.train()
    assert len(head(torch.from_numpy(GOLD["feats"]).to(DEV))) == 2          # training: the closed-set pair on cls_score, as before


@pytest.mark.parametrize("mult", [False, True])
def test_openset_on_the_training_vocabulary_equals_closed_set(mult, tmp_path):
    """the test embeddings are the training vocabulary's own file: same classes and kept indices as the closed-set path, scores
    inside the bound (class-specific deltas: the sizes agree); the case (the fixture's inputs) has an empty ambiguous set at the
    threshold and disjoint score intervals, so the order of the detections is defined"""
    c = X.case("fixture")
    over = ["MODEL.CLIP.MULTIPLY_RPN_SCORE", mult, "MODEL.CLIP.TEXT_EMB_PATH", None]
    cfg = _cfg(tmp_path, c["wn"], 37, 64, over)
    cfg.MODEL.CLIP.TEXT_EMB_PATH = cfg.MODEL.CLIP.OPENSET_TEST_TEXT_EMB_PATH
    open_head = _head(cfg, 64)
    cfg2 = cfg.clone()
    cfg2.MODEL.CLIP.OPENSET_TEST_TEXT_EMB_PATH = None
    closed_head = _head(cfg2, 64)
    assert open_head.openset and not closed_head.openset
    with torch.no_grad():
        open_head.bbox_pred.weight.copy_(torch.randn(148, 64, generator=torch.Generator().manual_seed(9)) * 0.05)
        closed_head.bbox_pred.weight.copy_(open_head.bbox_pred.weight)
    open_head.to(DEV).eval()
    closed_head.to(DEV).eval()
    ref = X.ref_select(c["z"][0.01], c["zbound"][0.01], c["boxes"], c["obj"] if mult else None, 0.05)
    assert len(ref["ambiguous"]) == 0 and X.order_overlaps(ref) == 0
    props = [_proposals(c["boxes"], c["obj"], (X.IMG_H, X.IMG_W))]
    x = _dev(c["x"])
    with torch.no_grad():
        a, ka = open_head.inference(open_head(x), props)
        b, kb = closed_head.inference(closed_head(x), props)
    assert len(ka[0]) > 10
    assert torch.equal(a[0].pred_classes, b[0].pred_classes) and torch.equal(ka[0], kb[0])
    assert torch.equal(a[0].pred_boxes.tensor, b[0].pred_boxes.tensor)
    # both scores lie in the interval around the float64 score of their (row, class) entry
    s, lo, hi = X.score_interval(c["z"][0.01], c["zbound"][0.01], c["obj"] if mult else None)
    r, k = _host(ka[0]), _host(a[0].pred_classes)
    for got in (_host(a[0].scores), _host(b[0].scores)):
        assert ((lo[r, k] <= got) & (got <= hi[r, k])).all()


def test_openset_inference_with_soft_nms(tmp_path):
    """MODEL.ROI_HEADS.SOFT_NMS_ENABLED on the open-set path: ``batched_soft_nms`` unchanged on the selected candidates -- the
    detections carry the rescored scores in pick order, cut at the top-k"""
    from cddmsl_amd.modeling import roi_heads as rh
    c = X.case("fixture")
    cfg = _cfg(tmp_path, c["wn"], 5, 64, ["MODEL.ROI_BOX_HEAD.CLS_AGNOSTIC_BBOX_REG", True, "MODEL.ROI_HEADS.SOFT_NMS_ENABLED", True,
                                          "MODEL.ROI_HEADS.SOFT_NMS_METHOD", "linear", "TEST.DETECTIONS_PER_IMAGE", 60])
    head = _head(cfg, 64).to(DEV).eval()
    props = [_proposals(c["boxes"], c["obj"], (X.IMG_H, X.IMG_W))]
    with torch.no_grad():
        pred = head(_dev(c["x"]))
        inst, kept = head.inference(pred, props)
        boxes = head.predict_boxes(pred, props)[0].contiguous()
        rows, cls, sc, bx, valid = _hip().openset_select(pred[0], pred[2], 37, boxes, None, X.IMG_H, X.IMG_W, 0.05)
        keep, soft = rh.batched_soft_nms(bx, sc.clone(), cls.long(), "linear", 0.5, 0.5, 0.001, max_keep=60)
    assert len(keep) == 60 and bool(valid.all())
    assert torch.equal(inst[0].pred_classes, cls.long()[keep]) and torch.equal(inst[0].scores, soft)
    assert torch.equal(inst[0].pred_boxes.tensor, bx[keep]) and torch.equal(kept[0], rows.long()[keep])


# ------------------------------------------------------------------------------------------------------- batched_nms_grouped
def test_batched_nms_grouped_equals_batched_nms():
    from cddmsl_amd.modeling import roi_heads as rh
    g = np.random.default_rng(3)
    n = 300
    ctr = g.uniform(20, 200, size=(12, 2))
    p = ctr[g.integers(0, 12, size=n)] + g.normal(0, 6, size=(n, 2))
    wh = g.uniform(20, 60, size=(n, 2))
    boxes = torch.from_numpy(np.concatenate([p - wh / 2, p + wh / 2], axis=1).astype(np.float32)).to(DEV)
    scores = torch.from_numpy(np.round(g.uniform(0.05, 1, size=n), 2).astype(np.float32)).to(DEV)      # rounded: equal scores occur
    idxs = torch.from_numpy(g.integers(0, 9, size=n)).to(DEV)
    want = rh.batched_nms(boxes, scores, idxs, 0.5)
    assert 0 < want.numel() < n
    calls = []
    orig = rh._nms_sorted
    rh._nms_sorted = lambda b, s, t: (calls.append(b.shape[0]), orig(b, s, t))[1]
    try:
        got = rh.batched_nms_grouped(boxes, scores, idxs, 0.5, cap=64)
        assert len(calls) > 1 and max(calls) <= 64 and sum(calls) == n      # several runs, each within the cap
        assert torch.equal(got, want)
        calls.clear()
        assert torch.equal(rh.batched_nms_grouped(boxes, scores, idxs, 0.5), want) and calls == [n]       # default cap: the same single pass
        with pytest.raises(ValueError):
            rh.batched_nms_grouped(boxes, scores, idxs, 0.5, cap=int(torch.bincount(idxs).max()) - 1)
    finally:
        rh._nms_sorted = orig
    e = rh.batched_nms_grouped(boxes[:0], scores[:0], idxs[:0], 0.5, cap=64)
    assert e.numel() == 0 and e.dtype == torch.int64


# ------------------------------------------------------------------------------------------------------ class-agnostic training
@pytest.mark.parametrize("loc,beta", [("smooth_l1", 0.0), ("giou", 0.0)], ids=["l1", "giou"])
def test_cls_agnostic_losses(loc, beta, tmp_path):
    """FastRCNNOutputLayers.losses with [R, 4] deltas (CLS_AGNOSTIC_BBOX_REG: the kernels take cls = NULL, ld = 4) against
    exact_box_losses' float64 reference, forward and the gradient of the deltas, within the bounds it derives for these kernels"""
    import exact_box_losses as B
    import exact_losses as E
    from cddmsl_amd.structures import Boxes, Instances
    cfg = _cfg(tmp_path, X.case("fixture")["wn"], 5, 64, ["MODEL.ROI_BOX_HEAD.CLS_AGNOSTIC_BBOX_REG", True,
                                                          "MODEL.ROI_BOX_HEAD.BBOX_REG_LOSS_TYPE", loc, "MODEL.ROI_BOX_HEAD.SMOOTH_L1_BETA", beta])
    head = _head(cfg, 64)
    head.train()
    K, R = 5, 128
    w = head.box_weights
    g = E._g(611)
    cls = torch.randint(0, K, (R,), generator=g)
    cls[torch.rand(R, generator=g) < 0.4] = K
    fg = torch.nonzero(cls < K)[:, 0]
    src, tgt = E._boxes(R, 612), E._boxes(R, 613)
    deltas = B._deltas(R, w, 615)
    a = dict(deltas=deltas, fg=fg, cls=None, src=src, tgt=tgt, w=w, inv_norm=1.0 / R)
    gout = torch.tensor([0.7])
    props = []
    for h in (slice(0, R // 2), slice(R // 2, R)):
        p = Instances((480, 640))
        p.proposal_boxes, p.gt_boxes, p.gt_classes = Boxes(src[h].to(DEV)), Boxes(tgt[h].to(DEV)), cls[h].to(DEV)
        props.append(p)
    d1 = deltas.to(DEV).requires_grad_(True)
    out = head.losses((E._randn((R, K + 1), 617).to(DEV), d1), props)
    (gout[0] * out["loss_box_reg"]).backward()
    rep = E.Report()
    name = f"cls-agnostic losses {loc}"
    rep.bound(name + " loss", "kernel", out["loss_box_reg"].detach().cpu().reshape(1),
              tuple(x.reshape(1) for x in B.box_reg_ref(a, loc, beta, B.SCALE_CLAMP)))
    dd = d1.grad.cpu()
    touched = torch.zeros(R, dtype=torch.bool)
    touched[fg] = True
    rep.exact(name + " ddeltas", "kernel", bool((dd[~touched] == 0).all()), "a gradient outside the foreground rows")
    B._loc_checks(rep, name + " ddeltas", "kernel", dd[fg], B.box_reg_ref(a, loc, beta, B.SCALE_CLAMP, gout=gout), dict(loc=loc, beta=beta), 0)
    for k, v in rep.worst.items():
        print(f"{k}: worst |err|/bound {v:.3g}")
    assert not rep.fail, "\n".join(rep.fail)


# ------------------------------------------------------------------------------------------------------------------ TTA
@pytest.mark.parametrize("direct", [True, False], ids=["direct", "tta_model"])
def test_tta_with_an_open_set_vocabulary(direct, tmp_path):
    """GeneralizedRCNNWithTTA, constructed directly with the model's own config (NUM_CLASSES 20) or by evaluation.tta_model, on a
    model with a 37-class test vocabulary: the views' detections (classes up to 36) merge over 37 classes; equal to the merge
    function called on the same per-view outputs"""
    from cddmsl_amd import evaluation, synthetic
    from cddmsl_amd.modeling import GeneralizedRCNNWithTTA
    from cddmsl_amd.config import get_cfg
    from cddmsl_amd.modeling import build_model
    from cddmsl_amd.modeling import test_time_augmentation as tt
    path = os.path.join(str(tmp_path), "emb.pth")
    g = torch.Generator().manual_seed(4)
    torch.save(torch.randn(37, 1024, generator=g), path)
    cfg = get_cfg()
    cfg.merge_from_file(os.path.join(ROOT, "configs", "VOC-Experiments", "faster_rcnn_CLIP_R_50_C4.yaml"))
    cfg.merge_from_list(["MODEL.DEVICE", DEV, "INPUT.MIN_SIZE_TEST", 128, "INPUT.MAX_SIZE_TEST", 256, "MODEL.RPN.PRE_NMS_TOPK_TEST", 300,
                         "MODEL.RPN.POST_NMS_TOPK_TEST", 50, "MODEL.ROI_HEADS.SCORE_THRESH_TEST", 0.0, "TEST.DETECTIONS_PER_IMAGE", 20,
                         "TEST.AUG.MIN_SIZES", (96, 128), "TEST.AUG.MAX_SIZE", 256, "TEST.AUG.FLIP", True,
                         "MODEL.CLIP.OPENSET_TEST_TEXT_EMB_PATH", path, "MODEL.ROI_BOX_HEAD.CLS_AGNOSTIC_BBOX_REG", True])
    model = build_model(cfg)
    model.load_state_dict({k: v for k, v in synthetic.make_state_dict(0).items() if "bbox_pred" not in k}, strict=False)
    model.eval()
    tta = GeneralizedRCNNWithTTA(cfg, model) if direct else evaluation.tta_model(cfg, model)
    assert tta.cfg.MODEL.ROI_HEADS.NUM_CLASSES == 20
    img = torch.from_numpy(np.random.RandomState(0).randint(0, 256, (3, 120, 160), dtype=np.uint8))
    captured = []
    orig = tta._merge_detections
    tta._merge_detections = lambda b, s, c, hw: (captured.append((b, s, c, hw)), orig(b, s, c, hw))[1]
    inst = tta([{"image": img, "height": 120, "width": 160}])[0]["instances"]
    b, s, c, hw = captured[0]
    assert 0 < len(inst) <= 20 and int(c.max()) >= 20 and int(c.max()) < 37          # classes beyond the training vocabulary reach the merge
    want = tt.merge_detections(b, s, c, hw, 37, cfg.MODEL.ROI_HEADS.NMS_THRESH_TEST, 20)
    assert torch.equal(inst.pred_classes, want.pred_classes) and torch.equal(inst.scores, want.scores)
    assert torch.equal(inst.pred_boxes.tensor, want.pred_boxes.tensor) and int(inst.pred_classes.max()) < 37


# ------------------------------------------------------------------------------------------------------------- the tool
def test_detect_open_vocab_end_to_end(tmp_path):
    from PIL import Image
    from cddmsl_amd import synthetic
    ck, img, emb, con = tmp_path / "det.pth", tmp_path / "images", tmp_path / "concepts.pth", tmp_path / "concepts.txt"
    img.mkdir()
    sd = synthetic.make_state_dict(0)
    g = torch.Generator().manual_seed(4)
    sd["roi_heads.box_predictor.bbox_pred.weight"] = torch.randn(4, 1024, generator=g) * 0.5 * 1024 ** -0.5      # class-agnostic
    sd["roi_heads.box_predictor.bbox_pred.bias"] = torch.zeros(4)
    torch.save({"model": sd}, ck)
    torch.save(torch.randn(37, 1024, generator=g), emb)
    names = [f"concept {i}" for i in range(37)]
    con.write_text("\n".join(names) + "\n", encoding="utf-8")
    rs = np.random.RandomState(0)
    sizes = {"a.png": (120, 160), "b.png": (150, 110)}
    for fn, (h, w) in sizes.items():
        Image.fromarray(rs.randint(0, 256, (h, w, 3), dtype=np.uint8)).save(img / fn)
    out = tmp_path / "out"
    cmd = [sys.executable, os.path.join(ROOT, "tools", "detect_open_vocab.py"), "--config-file",
           os.path.join(ROOT, "configs", "VOC-Experiments", "faster_rcnn_CLIP_R_50_C4.yaml"), "--concepts", str(con), "--embeddings", str(emb),
           "--regions-per-image", "12", "MODEL.WEIGHTS", str(ck), "INPUT_DIR", str(img), "OUTPUT_DIR", str(out), "MODEL.DEVICE", DEV,
           "INPUT.MIN_SIZE_TEST", "128", "INPUT.MAX_SIZE_TEST", "256", "MODEL.ROI_BOX_HEAD.CLS_AGNOSTIC_BBOX_REG", "True",
           "MODEL.ROI_HEADS.SCORE_THRESH_TEST", "0.0"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=dict(os.environ, PYTHONPATH=ROOT))
    assert r.returncode == 0, r.stderr[-3000:]
    res = json.load(open(out / "detections.json", encoding="utf-8"))
    assert sorted(res) == sorted(sizes)
    assert sum(len(v) for v in res.values()) >= 1
    for fn, (h, w) in sizes.items():
        assert len(res[fn]) <= 12
        sc = [d["score"] for d in res[fn]]
        assert sc == sorted(sc, reverse=True)
        for d in res[fn]:
            assert sorted(d) == ["box", "class", "name", "score"]
            assert isinstance(d["class"], int) and 0 <= d["class"] < 37 and d["name"] == names[d["class"]]
            x0, y0, x1, y1 = d["box"]
            assert 0 <= x0 <= x1 <= w and 0 <= y0 <= y1 <= h and 0 <= d["score"] <= 1
