"""cddmsl_coco_match (cddmsl_amd/csrc/coco_match.hip) against the host matcher it restates, evaluation._coco_match, BIT FOR BIT:
ranks and both 40-bit masks of every detection, on the case sets of tests/coco_match_cases.py (which tests/test_coco_eval_host.py
shows to hit every rule of the walk: later-wins ties, the break, crowd re-matches, matches to ignored boxes, NaN IoUs, IoUs on a
threshold, areas on a range edge) and on the edge shapes; then the evaluator with ``device`` against the evaluator without."""
import ctypes

import numpy as np
import pytest
import torch

import coco_match_cases as C

pytestmark = pytest.mark.gpu
DEV = "cuda"
SETS = ["seed0", "seed1", "seed2", "edge"]


def _set(name):
    from cddmsl_amd import hip
    return C.cached(("set", name), lambda: C.edge_set(hip.COCO_MATCH_MAX_GT) if name == "edge" else C.random_set(int(name[4:])))


def _host(name):
    """the yardstick, once per set: per image (rank, matched, ignored) from evaluation._coco_match"""
    from cddmsl_amd import evaluation as E

    def run():
        dicts, dets = _set(name)
        with np.errstate(invalid="ignore", divide="ignore"):
            return [E.coco_match_host(g, d, C.NUM_CLASSES) for g, d in zip(C.gt_tuples(dicts), C.dt_tuples(dets))]
    return C.cached(("host", name), run)


def _gt_dev(dicts):
    from cddmsl_amd import evaluation as E, hip
    return hip.CocoGroundTruth.from_host(C.gt_tuples(dicts), np.minimum(E.COCO_IOU_THRS, 1 - 1e-10), E.COCO_AREA_RNGS, DEV)


def _inputs(dets, images):
    lens = [len(dets[i][1]) for i in images]
    cat = lambda j, dt, shape: torch.from_numpy(np.concatenate([np.asarray(dets[i][j], dtype=dt).reshape(shape) for i in images])).to(DEV)
    off = torch.tensor(np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)).to(DEV)
    return cat(0, np.float32, (-1, 4)), cat(1, np.float32, (-1,)), cat(2, np.int64, (-1,)), off, torch.tensor(list(images), dtype=torch.int64).to(DEV), lens


def _launch(name, images=None, gt=None):
    """one launch over ``images`` (default: all, in order) -> per image (rank, matched, ignored), over [B]"""
    from cddmsl_amd import hip
    dicts, dets = _set(name)
    images = list(range(len(dicts))) if images is None else images
    b, s, c, off, idx, lens = _inputs(dets, images)
    rank, matched, ignored, over = hip.coco_match(b, s, c, off, idx, gt if gt is not None else _gt_dev(dicts), C.NUM_CLASSES)
    torch.cuda.synchronize()
    rank, matched, ignored = rank.cpu().numpy(), matched.cpu().numpy(), ignored.cpu().numpy()
    st = np.concatenate([[0], np.cumsum(lens)])
    return [(rank[st[j]: st[j + 1]], matched[st[j]: st[j + 1]], ignored[st[j]: st[j + 1]]) for j in range(len(images))], over.cpu().numpy()


def _same(got, ref, what):
    for k, n in enumerate(("rank", "matched", "ignored")):
        assert got[k].dtype == ref[k].dtype and np.array_equal(got[k], ref[k]), f"{what}: {n} differs at {np.flatnonzero(got[k] != ref[k])[:8]}"


@pytest.mark.parametrize("name", SETS)
def test_matches_the_host_matcher_bit_for_bit(name):
    from cddmsl_amd import hip
    dicts, dets = _set(name)
    got, over = _launch(name)
    ref = _host(name)
    expect_over = [int(d["image_id"] == f"edge_g{hip.COCO_MATCH_MAX_GT + 1}") for d in dicts]
    assert over.tolist() == expect_over                       # only the image beyond the cap is handed back, and it IS handed back
    assert sum(expect_over) == (1 if name == "edge" else 0)
    kept = dropped = 0
    for i, d in enumerate(dicts):
        if not expect_over[i]:
            _same(got[i], ref[i], d["image_id"])
            kept += int((ref[i][0] >= 0).sum()); dropped += int((ref[i][0] < 0).sum())
    assert kept > 100 and dropped > 0                          # every set holds an image with more than COCO_MAX_DETS of one class
    assert any(r[1].any() for r in ref) and any(r[2].any() for r in ref)


def test_edge_set_holds_the_edge_shapes():
    """what the edge set is there for (a condition on the inputs)"""
    from cddmsl_amd import hip
    dicts, dets = _set("edge")
    by = {d["image_id"][5:]: (d["annotations"], t) for d, t in zip(dicts, dets)}
    assert not by["no_gt"][0] and len(by["no_gt"][1][1]) > 0 and by["no_dets"][0] and len(by["no_dets"][1][1]) == 0
    assert not by["neither"][0] and len(by["neither"][1][1]) == 0 and len(by["one_one"][0]) == len(by["one_one"][1][1]) == 1
    assert np.bincount(by["d100"][1][2]).max() == 100 and np.bincount(by["d101"][1][2]).max() == 101
    for g in (33, 65, hip.COCO_MATCH_MAX_GT, hip.COCO_MATCH_MAX_GT + 1):
        assert sum(a["category_id"] == 2 for a in by[f"g{g}"][0]) == g and (by[f"g{g}"][1][2] == 2).sum() > 0
    assert hip.COCO_MATCH_MAX_GT >= 256 and hip.COCO_MATCH_MAX_DETS >= 1024 and hip.COCO_MATCH_MAX_KEPT >= 100


@pytest.mark.parametrize("name", ["seed0", "edge"])
def test_one_call_per_image_equals_the_batch(name):
    dicts, _ = _set(name)
    gt = _gt_dev(dicts)
    batch, over = _launch(name, gt=gt)
    order = list(range(len(dicts)))[::-1]                      # and the batch order is free
    rev, over_r = _launch(name, order, gt=gt)
    for j, i in enumerate(order):
        one, over_1 = _launch(name, [i], gt=gt)
        assert over_1.tolist() == [over[i]] == [over_r[j]]
        if not over[i]:
            _same(one[0], batch[i], dicts[i]["image_id"])
            _same(rev[j], batch[i], dicts[i]["image_id"])


def test_two_runs_give_identical_bytes():
    from cddmsl_amd import hip
    dicts, dets = _set("seed1")
    gt = _gt_dev(dicts)
    b, s, c, off, idx, _ = _inputs(dets, list(range(len(dicts))))
    first = hip.coco_match(b, s, c, off, idx, gt, C.NUM_CLASSES)
    junk = [torch.full((1 << 18,), v, device=DEV, dtype=torch.int64) for v in (-1, 0x5A5A5A5A5A5A5A5A)]   # dirty the allocator's blocks
    del junk
    second = hip.coco_match(b, s, c, off, idx, gt, C.NUM_CLASSES)
    torch.cuda.synchronize()
    for x, y in zip(first, second):
        assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes()


def test_cabi_writes_inside_its_outputs_and_checks_arguments():
    from cddmsl_amd import hip
    from cddmsl_amd._lib import HipLibraryError
    dicts, dets = _set("seed0")
    gt = _gt_dev(dicts)
    images = list(range(len(dicts)))
    b, s, c, off, idx, lens = _inputs(dets, images)
    D, B, TAIL = int(sum(lens)), len(images), 64
    rank = torch.full((D + TAIL,), -77, device=DEV, dtype=torch.int32)
    matched, ignored = torch.full((D + TAIL,), -77, device=DEV, dtype=torch.int64), torch.full((D + TAIL,), -77, device=DEV, dtype=torch.int64)
    over = torch.full((B + TAIL,), -77, device=DEV, dtype=torch.int32)
    p = lambda t: ctypes.c_void_p(t.data_ptr())

    def call(T=10, A=4, K=C.NUM_CLASSES, max_dets=100):
        return hip._L().cddmsl_coco_match(p(b), p(s), p(c), p(off), p(idx), B, D, p(gt.xywh), p(gt.area), p(gt.crowd), p(gt.cls), p(gt.off), gt.n_images,
                                          p(gt.thrs), T, p(gt.rngs), A, K, max_dets, p(rank), p(matched), p(ignored), p(over), hip.stream_ptr())
    for bad in (dict(T=0), dict(A=5), dict(T=17), dict(K=0), dict(max_dets=0), dict(max_dets=hip.COCO_MATCH_MAX_KEPT + 1)):
        assert call(**bad) == 1, bad
    torch.cuda.synchronize()
    assert (rank == -77).all() and (matched == -77).all() and (over == -77).all()          # a refused call writes nothing
    assert call() == 0
    torch.cuda.synchronize()
    for t in (rank, matched, ignored, over):
        assert (t[-TAIL:] == -77).all()
    ref = _host("seed0")
    assert np.array_equal(rank[:D].cpu().numpy(), np.concatenate([r[0] for r in ref]))
    assert np.array_equal(matched[:D].cpu().numpy(), np.concatenate([r[1] for r in ref]))
    assert np.array_equal(ignored[:D].cpu().numpy(), np.concatenate([r[2] for r in ref])) and not over[:B].any()
    with pytest.raises(ValueError, match="max_dets"):
        hip.coco_match(b, s, c, off, idx, gt, C.NUM_CLASSES, max_dets=hip.COCO_MATCH_MAX_KEPT + 1)
    with pytest.raises(HipLibraryError):
        hip.coco_match(b.cpu(), s.cpu(), c.cpu(), off.cpu(), idx.cpu(), gt, C.NUM_CLASSES)


# ------------------------------------------------------------------------------------------------ the evaluator
NAMES = ["alpha", "beta", "gamma"]


def _feed(ev, dicts, dets, images, per_call=1):
    from cddmsl_amd.structures import Boxes, Instances
    for s in range(0, len(images), per_call):
        inputs, outputs = [], []
        for i in images[s: s + per_call]:
            b, sc, c = dets[i]
            inst = Instances((dicts[i]["height"], dicts[i]["width"]), pred_boxes=Boxes(torch.from_numpy(b).to(DEV)), scores=torch.from_numpy(sc).to(DEV),
                             pred_classes=torch.from_numpy(c).to(DEV))
            inputs.append({"image_id": dicts[i]["image_id"]}); outputs.append({"instances": inst})
        ev.process(inputs, outputs)


def _host_result(name):
    from cddmsl_amd import evaluation as E

    def run():
        dicts, dets = _set(name)
        ev = E.COCODetectionEvaluator(dicts, NAMES)
        _feed(ev, dicts, dets, list(range(len(dicts))))
        with np.errstate(invalid="ignore", divide="ignore"):
            return ev.evaluate()
    return C.cached(("host_result", name), run)


def _equal_results(a, b):
    assert list(a) == list(b) == ["bbox"] and list(a["bbox"]) == list(b["bbox"])
    for k in a["bbox"]:
        x, y = a["bbox"][k], b["bbox"][k]
        assert type(x) is type(y) is float and (x == y or (x != x and y != y)), (k, x, y)


@pytest.mark.parametrize("name", SETS)
def test_device_evaluator_equals_the_host_evaluator(name):
    from cddmsl_amd import evaluation as E
    dicts, dets = _set(name)
    ref = _host_result(name)
    assert any(v == v and 0 < v < 100 for v in ref["bbox"].values())
    for per_call in (1, 5):
        ev = E.COCODetectionEvaluator(dicts, NAMES, device=DEV)
        _feed(ev, dicts, dets, list(range(len(dicts))), per_call)
        assert ev._predictions == {} and all(e["rank"].is_cuda and e["boxes"].is_cuda for e in ev._batches)      # nothing came to the host
        _equal_results(ev.evaluate(), ref)
    ev.reset()
    empty = ev.evaluate()["bbox"]
    assert list(empty) == list(ref["bbox"]) and all(v != v for v in empty.values())


def test_an_image_processed_twice_counts_once_like_on_the_host():
    from cddmsl_amd import evaluation as E
    dicts, dets = _set("seed2")
    swapped = list(dets)
    swapped[3] = dets[5]
    res = []
    for dev in (None, DEV):
        ev = E.COCODetectionEvaluator(dicts, NAMES, device=dev)
        _feed(ev, dicts, swapped, [3])                           # first with other detections ...
        _feed(ev, dicts, dets, list(range(len(dicts))))          # ... then the whole set: the later call replaces the earlier
        with np.errstate(invalid="ignore", divide="ignore"):
            res.append(ev.evaluate())
    _equal_results(res[1], res[0])
    _equal_results(res[1], _host_result("seed2"))


@pytest.mark.parametrize("name", ["seed0", "edge"])
def test_records_of_two_evaluators_merge_to_the_one_evaluator_result(name):
    """what rank 0 does with its ranks' shards: each evaluator matched half of the images"""
    from cddmsl_amd import evaluation as E
    dicts, dets = _set(name)
    images = list(range(len(dicts)))
    parts, n = [], 0
    for shard in (images[1::2], images[0::2]):                   # (rank order and image order differ)
        ev = E.COCODetectionEvaluator(dicts, NAMES, device=DEV)
        _feed(ev, dicts, dets, shard, per_call=2)
        rec, seen = ev._device_records()
        parts.append(rec); n += seen
    assert n == sum(len(d[1]) for d in dets)
    whole = E.COCODetectionEvaluator(dicts, NAMES, device=DEV)
    _feed(whole, dicts, dets, images, per_call=3)
    one, _ = whole._gathered_records()
    merged = E.merge_coco_records(parts)
    for k in one:
        assert merged[k].dtype == one[k].dtype and np.array_equal(merged[k], one[k]), k
    npig = E.coco_gt_counts(C.gt_tuples(dicts), C.NUM_CLASSES)
    gt = {d["image_id"]: g for d, g in zip(dicts, C.gt_tuples(dicts))}
    dt = {d["image_id"]: t for d, t in zip(dicts, C.dt_tuples(dets))}
    with np.errstate(invalid="ignore", divide="ignore"):
        ref = C.cached(("prec", name), lambda: E.coco_precision(gt, dt, C.NUM_CLASSES))
    assert np.array_equal(E.coco_accumulate(merged, npig, C.NUM_CLASSES), ref)
