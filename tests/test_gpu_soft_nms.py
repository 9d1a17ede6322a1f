"""cddmsl_soft_nms (cddmsl_amd/csrc/soft_nms.hip) against the numpy references of tests/exact_soft_nms.py, which
tests/test_soft_nms_ref_host.py ties to the reference first.  Every case goes through the raw C-ABI with outputs that are longer than
documented and pre-filled with sentinels (keep -7, scores NaN, scratch 0x5A): ``nkeep`` and ``keep[:nkeep]`` array_equal,
``keep[nkeep:K] == -1``, scores past ``nkeep`` and everything past ``K`` untouched; linear and hard scores bit-equal, gaussian scores
within the derived bound (the worst ratio to the bound is printed).  Then the Python layers on the same cases, inference against
the reference fixture, and a small model end to end."""
import ctypes
import os

import numpy as np
import pytest
import torch

import exact_soft_nms as X

pytestmark = pytest.mark.gpu
DEV = "cuda"
TAIL = 64
KEEP_S, WS_S = -7, 0x5A
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "ref_soft_nms.npz"))
NAMES = [c["name"] for c in X.cases()]


def _L():
    from cddmsl_amd import hip
    return hip._L()


def _st():
    from cddmsl_amd import hip
    return hip.stream_ptr()


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def _dev(a, dtype=None):
    a = np.ascontiguousarray(a if dtype is None else np.asarray(a, dtype))
    if a.size == 0:
        a = np.zeros(4, a.dtype)
    return torch.from_numpy(a).to(DEV)


def _buf(n, dtype, fill):
    return torch.full((n + TAIL,), fill, device=DEV, dtype=dtype)


def _host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def _call(c, K=None, method=None, ws_fill=WS_S, max_keep=None, sigma=None):
    """one size query + one run through the C-ABI -> (status of the run, keep, keep_scores, nkeep, scratch, scratch bytes)"""
    K = len(c["scores"]) if K is None else K
    boxes, scores, idxs = _dev(c["boxes"]), _dev(c["scores"]), _dev(c["idxs"], np.int64)
    keep, ks, nkeep = _buf(K, torch.int64, KEEP_S), _buf(K, torch.float32, float("nan")), _buf(1, torch.int32, KEEP_S)
    args = (K, X.METHODS[c["method"]] if method is None else method, c["sigma"] if sigma is None else sigma, c["thr"], c["prune"],
            c["max_keep"] if max_keep is None else max_keep)
    nbytes = ctypes.c_size_t(12345)
    rc = _L().cddmsl_soft_nms(_p(boxes), _p(scores), _p(idxs), _p(keep), _p(ks), _p(nkeep), *args, None, ctypes.byref(nbytes), _st())
    if rc != 0:
        return rc, keep, ks, nkeep, None, nbytes.value
    assert (_host(keep) == KEEP_S).all() and (_host(nkeep) == KEEP_S).all(), "the size query wrote an output"
    ws = _buf(nbytes.value, torch.uint8, ws_fill)
    rc = _L().cddmsl_soft_nms(_p(boxes), _p(scores), _p(idxs), _p(keep), _p(ks), _p(nkeep), *args, _p(ws), ctypes.byref(nbytes), _st())
    return rc, keep, ks, nkeep, ws, nbytes.value


def _check(c, ref, keep, ks, nkeep):
    K, n = len(c["scores"]), len(ref["keep"])
    k, s, nk = _host(keep), _host(ks), _host(nkeep)
    assert nk[0] == n and (nk[1:] == KEEP_S).all(), (c["name"], int(nk[0]), n)
    assert np.array_equal(k[:n], ref["keep"]), (c["name"], k[:12].tolist(), ref["keep"][:12].tolist())
    assert (k[n:K] == -1).all(), (c["name"], "keep[nkeep:K] must be -1")
    assert (k[K:] == KEEP_S).all() and np.isnan(s[n:]).all(), (c["name"], "an element past the documented output was written")
    if c["method"] != "gaussian":
        assert np.array_equal(s[:n], ref["scores"]), (c["name"], np.nonzero(s[:n] != ref["scores"])[0][:8].tolist())
        return 0.0
    err = np.abs(s[:n].astype(np.float64) - ref["scores"].astype(np.float64))
    assert (err <= ref["bound"]).all(), (c["name"], float(err.max()), float(ref["bound"][np.argmax(err - ref["bound"])]))
    pos = ref["bound"] > 0
    ratio = float((err[pos] / ref["bound"][pos]).max()) if pos.any() else 0.0
    print(f"soft_nms {c['name']}: worst |error| / bound {ratio:.4f} over {int(pos.sum())} decayed scores (largest bound {ref['bound'].max():.3e})")
    return ratio


# ================================================================================================================= C-ABI
@pytest.mark.parametrize("name", NAMES)
def test_soft_nms_cabi(name):
    c = X.case(name)
    rc, keep, ks, nkeep, ws, nb = _call(c)
    assert rc == 0
    _check(c, X.expected(name), keep, ks, nkeep)
    assert (_host(ws)[nb:] == WS_S).all(), "the scratch buffer was written past the size the query returned"


def test_k0_writes_nkeep_only():
    c = dict(X.case("k1"), boxes=np.zeros((0, 4), np.float32), scores=np.zeros(0, np.float32), idxs=np.zeros(0, np.int64))
    rc, keep, ks, nkeep, ws, nb = _call(c)
    assert rc == 0 and nb == 0
    assert _host(nkeep)[0] == 0 and (_host(nkeep)[1:] == KEEP_S).all()
    assert (_host(keep) == KEEP_S).all() and np.isnan(_host(ks)).all()


def test_refusals_write_nothing():
    """one candidate more than the cap, an unknown method, sigma <= 0 for the gaussian method, max_keep < -1, a scratch buffer one
    byte short: CDDMSL_ERR_ARG (1) before any launch"""
    c = X.case("clustered300_s0_linear")
    big = dict(c, boxes=np.zeros((X.TOTAL_CAP + 1, 4), np.float32), scores=np.zeros(X.TOTAL_CAP + 1, np.float32),
               idxs=np.zeros(X.TOTAL_CAP + 1, np.int64))
    for kw, case in ((dict(), big), (dict(method=3), c), (dict(method=-1), c), (dict(method=0, sigma=0.0), c), (dict(method=0, sigma=-1.0), c),
                     (dict(max_keep=-2), c)):
        rc, keep, ks, nkeep, _, _ = _call(case, **kw)
        assert rc == 1, kw
        assert (_host(keep) == KEEP_S).all() and np.isnan(_host(ks)).all() and (_host(nkeep) == KEEP_S).all(), kw
    K = len(c["scores"])
    boxes, scores, idxs = _dev(c["boxes"]), _dev(c["scores"]), _dev(c["idxs"])
    keep, ks, nkeep = _buf(K, torch.int64, KEEP_S), _buf(K, torch.float32, float("nan")), _buf(1, torch.int32, KEEP_S)
    nb = ctypes.c_size_t(0)
    args = (K, 1, 0.5, 0.5, 0.001, -1)
    assert _L().cddmsl_soft_nms(_p(boxes), _p(scores), _p(idxs), _p(keep), _p(ks), _p(nkeep), *args, None, ctypes.byref(nb), _st()) == 0
    ws = _buf(nb.value, torch.uint8, WS_S)
    small = ctypes.c_size_t(nb.value - 1)
    assert _L().cddmsl_soft_nms(_p(boxes), _p(scores), _p(idxs), _p(keep), _p(ks), _p(nkeep), *args, _p(ws), ctypes.byref(small), _st()) == 1
    assert (_host(keep) == KEEP_S).all() and (_host(nkeep) == KEEP_S).all() and (_host(ws) == WS_S).all()
    exact = ctypes.c_size_t(nb.value)                                     # the size the query returned is the size the run accepts
    assert _L().cddmsl_soft_nms(_p(boxes), _p(scores), _p(idxs), _p(keep), _p(ks), _p(nkeep), *args, _p(ws), ctypes.byref(exact), _st()) == 0
    _check(c, X.expected(c["name"]), keep, ks, nkeep)


@pytest.mark.parametrize("name", ["unsorted_ids_gaussian", f"one_cat_{X.LDS_CAP + 1}_hard", "max_keep_7"])
def test_stale_scratch_changes_nothing(name):
    c = X.case(name)
    outs = []
    for fill in (WS_S, 0xFF, 0x00):
        rc, keep, ks, nkeep, _, _ = _call(c, ws_fill=fill)
        assert rc == 0
        n = int(_host(nkeep)[0])
        outs.append((n, _host(keep)[:n].copy(), _host(ks)[:n].copy()))
    for o in outs[1:]:
        assert o[0] == outs[0][0] and np.array_equal(o[1], outs[0][1]) and np.array_equal(o[2], outs[0][2])


def test_capped_equals_prefix_of_uncapped():
    c = X.case("clustered300_s0_linear")
    rc, keep, ks, nkeep, _, _ = _call(c)
    n = int(_host(nkeep)[0])
    full_k, full_s = _host(keep)[:n].copy(), _host(ks)[:n].copy()
    for mk in (0, 1, 7, n - 1, n, n + 5):
        rc, keep, ks, nkeep, _, _ = _call(c, max_keep=mk)
        m = int(_host(nkeep)[0])
        assert rc == 0 and m == min(mk, n)
        assert np.array_equal(_host(keep)[:m], full_k[:m]) and np.array_equal(_host(ks)[:m], full_s[:m]), mk


# ================================================================================================================= Python layers
PY_CASES = ["k1", "unsorted_ids_linear", "unsorted_ids_hard", "unsorted_ids_gaussian", "tied_scores_linear", "rerank", "shift_far_corner",
            "max_keep_7", "max_keep_7_gaussian", "category_top_below_prune_linear", "all_below_prune", "clustered300_low_scores_gaussian"]


@pytest.mark.parametrize("name", PY_CASES)
def test_python_wrappers(name):
    from cddmsl_amd import hip
    from cddmsl_amd.modeling.roi_heads import batched_soft_nms
    c, ref = X.case(name), X.expected(name)
    b, s, i = _dev(c["boxes"]), _dev(c["scores"]), _dev(c["idxs"])
    keep, ks, nkeep = hip.soft_nms(b, s, i, c["method"], c["sigma"], c["thr"], c["prune"], c["max_keep"])
    n = int(nkeep[0])
    assert keep.dtype == torch.int64 and ks.dtype == torch.float32 and n == len(ref["keep"])
    assert np.array_equal(_host(keep)[:n], ref["keep"]) and (_host(keep)[n:] == -1).all()
    k2, s2 = batched_soft_nms(b, s, i, c["method"], c["sigma"], c["thr"], c["prune"], max_keep=c["max_keep"])
    assert np.array_equal(_host(k2), ref["keep"]) and np.array_equal(_host(s2), _host(ks)[:n])
    err = np.abs(_host(s2).astype(np.float64) - ref["scores"].astype(np.float64))
    assert (err <= ref["bound"]).all() if c["method"] == "gaussian" else np.array_equal(_host(s2), ref["scores"])
    assert np.array_equal(ref["keep"], GOLD[f"keep/{name}"])


def test_python_wrapper_refuses_too_many_candidates():
    from cddmsl_amd.modeling.roi_heads import batched_soft_nms
    n = X.TOTAL_CAP + 1
    with pytest.raises(ValueError, match="exceed"):
        batched_soft_nms(torch.zeros(n, 4, device=DEV), torch.zeros(n, device=DEV), torch.zeros(n, dtype=torch.int64, device=DEV), "linear", 0.5, 0.5, 0.001)


@pytest.mark.parametrize("name", list(X.inference_configs()))
def test_inference_single_image_against_the_reference_fixture(name):
    """boxes, classes and kept-proposal indices equal the reference's; the scores are the rescored ones (bit-equal for linear and
    hard, within the bound for gaussian); non-finite rows are dropped first; proposal_indices=True maps back to input rows"""
    from cddmsl_amd.modeling.roi_heads import fast_rcnn_inference_single_image
    inp, cfg = X.inference_inputs(), X.inference_configs()[name]
    ref = X.inference_ref(inp, cfg)
    kw = dict(soft_nms_enabled=True, soft_nms_method=cfg["method"], soft_nms_sigma=cfg["sigma"], soft_nms_prune=cfg["prune"])
    b, s = _dev(inp["boxes"]), _dev(inp["scores"])
    inst, kept = fast_rcnn_inference_single_image(b, s, inp["image_shape"], inp["score_thresh"], cfg["nms_thresh"], cfg["topk"], **kw)
    assert np.array_equal(_host(inst.pred_boxes.tensor), GOLD[f"inf/{name}/pred_boxes"])
    assert np.array_equal(_host(inst.pred_classes), GOLD[f"inf/{name}/pred_classes"])
    assert np.array_equal(_host(kept), GOLD[f"inf/{name}/kept"])
    got = _host(inst.scores)
    if cfg["method"] == "gaussian":
        assert (np.abs(got.astype(np.float64) - GOLD[f"inf/{name}/scores"].astype(np.float64)) <= ref["bound"]).all()
    else:
        assert np.array_equal(got, GOLD[f"inf/{name}/scores"])
    inst2, rows = fast_rcnn_inference_single_image(b, s, inp["image_shape"], inp["score_thresh"], cfg["nms_thresh"], cfg["topk"], True, **kw)
    assert np.array_equal(_host(rows), ref["kept_rows"]) and np.array_equal(_host(inst2.scores), got)
    assert not np.isin(_host(rows), [7, 20]).any()


def test_inference_single_image_switch_off_is_todays_path():
    from cddmsl_amd.modeling import roi_heads as R
    inp = X.inference_inputs()
    b, s = _dev(inp["boxes"]), _dev(inp["scores"])
    a, ka = R.fast_rcnn_inference_single_image(b, s, inp["image_shape"], 0.05, 0.5, 20, soft_nms_enabled=False, soft_nms_method="linear")
    bb, sc, pi, ci, rows = X.inference_candidates(inp["boxes"], inp["scores"], inp["image_shape"], 0.05)
    keep = R.batched_nms(_dev(bb), _dev(sc), _dev(ci), 0.5)[:20]             # the hard path, by hand
    assert np.array_equal(_host(a.pred_boxes.tensor), bb[_host(keep)]) and np.array_equal(_host(a.scores), sc[_host(keep)])
    assert np.array_equal(_host(a.pred_classes), ci[_host(keep)]) and np.array_equal(_host(ka), pi[_host(keep)])


# ================================================================================================================= model
def _model(*opts):
    from cddmsl_amd import synthetic
    from cddmsl_amd.config import get_cfg
    from cddmsl_amd.modeling import build_model
    cfg = get_cfg()
    cfg.merge_from_file(os.path.join(ROOT, "configs", "VOC-Experiments", "faster_rcnn_CLIP_R_50_C4.yaml"))
    cfg.merge_from_list(["MODEL.DEVICE", DEV, "INPUT.MIN_SIZE_TEST", 128, "INPUT.MAX_SIZE_TEST", 256, "MODEL.RPN.PRE_NMS_TOPK_TEST", 300,
                         "MODEL.RPN.POST_NMS_TOPK_TEST", 50, "MODEL.ROI_HEADS.SCORE_THRESH_TEST", 0.0, "TEST.DETECTIONS_PER_IMAGE", 20, *opts])
    model = build_model(cfg)
    model.load_state_dict(synthetic.make_state_dict(0), strict=False)
    return model.eval()


def test_model_detections_equal_the_reference_on_the_captured_candidates(monkeypatch):
    """a small model with SOFT_NMS_ENABLED (linear): its detections are batched_soft_nms_ref of the candidates in front of the NMS;
    with the switch off the same model takes the hard path and the soft entry is never reached"""
    from cddmsl_amd.modeling import roi_heads as R
    model = _model("MODEL.ROI_HEADS.SOFT_NMS_ENABLED", True, "MODEL.ROI_HEADS.SOFT_NMS_METHOD", "linear")
    seen = []
    orig = R.batched_soft_nms

    def spy(boxes, scores, idxs, *a, **k):
        seen.append((boxes.clone(), scores.clone(), idxs.clone(), a, k))
        return orig(boxes, scores, idxs, *a, **k)

    monkeypatch.setattr(R, "batched_soft_nms", spy)
    img = torch.from_numpy(np.random.RandomState(3).randint(0, 256, (3, 128, 256), dtype=np.uint8))
    inp = {"image": img, "height": 128, "width": 256}
    rh = model.roi_heads
    with torch.no_grad():
        images, sizes = model.preprocess_image([inp], "image")
        res4 = model.backbone.forward_nhwc(images, want_res5=False)["res4"]
        proposals, _ = model.proposal_generator.forward_nhwc(sizes, res4, None)
        att = rh._pooled_embeddings(res4, [p.proposal_boxes for p in proposals], model.backbone.layer4, model.backbone.attnpool)
        pred = rh.box_predictor(att)
        inst, kept = rh.box_predictor.inference(pred, proposals)
    assert len(seen) == 1
    b, s, i, a, k = seen[0]
    assert a == ("linear", 0.5, 0.5, 0.001) and k == {"max_keep": 20} and len(s) >= 100
    ref = X.batched_soft_nms_ref(_host(b), _host(s), _host(i), "linear", 0.5, 0.5, 0.001, 20)
    assert len(ref["keep"]) == 20 == len(inst[0])
    assert np.array_equal(_host(inst[0].scores), ref["scores"])
    assert np.array_equal(_host(inst[0].pred_boxes.tensor), _host(b)[ref["keep"]])
    assert np.array_equal(_host(inst[0].pred_classes), _host(i)[ref["keep"]])
    out = model.inference([inp])[0]["instances"]                          # and the public entry point runs end to end
    assert len(seen) == 2 and len(out) <= 20
    # uncapped (TEST.DETECTIONS_PER_IMAGE -1): the whole walk, its tail included -- at SCORE_THRESH_TEST 0.0 many candidates start
    # below SOFT_NMS_PRUNE, which the reference's first pick removes in every category
    rh.box_predictor.test_topk_per_image = -1
    with torch.no_grad():
        inst_all, _ = rh.box_predictor.inference(pred, proposals)
    assert len(seen) == 3 and seen[2][4] == {"max_keep": -1} and torch.equal(seen[2][1], s)
    assert int((s <= 0.001).sum()) > 0, "the case must hold scores that start at or below prune"
    full = X.batched_soft_nms_ref(_host(b), _host(s), _host(i), "linear", 0.5, 0.5, 0.001, -1)
    assert len(inst_all[0]) == len(full["keep"]) > 20
    assert np.array_equal(_host(inst_all[0].scores), full["scores"])
    assert np.array_equal(_host(inst_all[0].pred_boxes.tensor), _host(b)[full["keep"]])
    assert np.array_equal(_host(inst_all[0].pred_classes), _host(i)[full["keep"]])
    rh.box_predictor.test_topk_per_image = 20
    # switch off: the predictor of the same model falls back to hard NMS, output == the function with today's positional signature
    rh.box_predictor.soft_nms_enabled = False
    with torch.no_grad():
        inst_off, kept_off = rh.box_predictor.inference(pred, proposals)
        boxes = rh.box_predictor.predict_boxes(pred, proposals)[0]
        probs = rh.box_predictor.predict_probs(pred, proposals)[0]
        if rh.box_predictor.multiply_rpn_score:
            probs = (probs * proposals[0].objectness_logits[:, None]) ** 0.5
        want, want_kept = R.fast_rcnn_inference_single_image(boxes, probs, proposals[0].image_size, 0.0, 0.5, 20)
    assert len(seen) == 3
    assert torch.equal(inst_off[0].pred_boxes.tensor, want.pred_boxes.tensor) and torch.equal(inst_off[0].scores, want.scores)
    assert torch.equal(inst_off[0].pred_classes, want.pred_classes) and torch.equal(kept_off[0], want_kept)
