"""cddmsl_proposal_cover (cddmsl_amd/csrc/proposal_recall.hip) against the host walk it restates, evaluation.proposal_cover_host,
BIT FOR BIT: every cover slot of every (limit, range) on the images of tests/proposal_recall_cases.py (which
tests/test_proposal_recall_host.py holds to the reference's own numbers) and on the edge shapes -- batch order, empty sides, the
limit and one either side, the caps and one beyond, equal and NaN logits; every slot written, two runs the same bytes, refused
arguments; then the wiring: the evaluator with ``device`` against without, ``TEST.PROPOSAL_RECALL`` on a tiny detector, and
``ProposalNetwork`` on the detector's weights."""
import ctypes
import os

import numpy as np
import pytest
import torch

import proposal_recall_cases as C

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_CACHE = {}


def _cached(key, fn):
    if key not in _CACHE:
        _CACHE[key] = fn()
    return _CACHE[key]


def _case_images():
    """the case set as (gt f32, bits u8, boxes f32, logits f32) per image"""
    def run():
        from cddmsl_amd import evaluation as E
        items = C.dataset()
        gt = E.proposal_ground_truth([d for d, _, _ in items])
        return [(*gt[d["image_id"]], b, l) for d, b, l in items]
    return _cached("cases", run)


def _host(images, limits, A, key=None):
    """the yardstick: per image cover [L, A, g] from evaluation.proposal_cover_host (once per key)"""
    from cddmsl_amd import evaluation as E
    run = lambda: [E.proposal_cover_host(b, l, g, r, limits, A) for g, r, b, l in images]
    return _cached(("host", key), run) if key is not None else run()


def _gt_dev(images, limits, A):
    from cddmsl_amd import hip
    return hip.ProposalGroundTruth.from_host([(g, r) for g, r, _, _ in images], limits, A, DEV)


def _inputs(images, batch):
    lens = [len(images[i][3]) for i in batch]
    gc = [len(images[i][1]) for i in batch]
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    boxes = up(np.concatenate([images[i][2].reshape(-1, 4) for i in batch] + [np.zeros((0, 4), dtype=np.float32)]).astype(np.float32))
    logits = up(np.concatenate([images[i][3] for i in batch] + [np.zeros(0, dtype=np.float32)]).astype(np.float32))
    off = up(np.concatenate([[0], np.cumsum(lens)]).astype(np.int64))
    coff = up(np.concatenate([[0], np.cumsum(gc)]).astype(np.int64))
    return boxes, logits, off, up(np.asarray(batch, dtype=np.int64)), coff, gc


def _launch(images, limits, A, batch=None, gt=None):
    """one launch over ``batch`` (default: all images, in order) -> (per image cover [L, A, g], over [B])"""
    from cddmsl_amd import hip
    batch = list(range(len(images))) if batch is None else batch
    boxes, logits, off, idx, coff, gc = _inputs(images, batch)
    cover, over = hip.proposal_cover(boxes, logits, off, idx, coff, sum(gc), gt if gt is not None else _gt_dev(images, limits, A))
    torch.cuda.synchronize()
    cover = cover.cpu().numpy()
    st = np.concatenate([[0], np.cumsum(gc)])
    return [cover[:, :, st[j]: st[j + 1]] for j in range(len(batch))], over.cpu().numpy()


def _same(got, ref, what):
    assert got.dtype == ref.dtype == np.float32 and got.shape == ref.shape, what
    assert got.tobytes() == ref.tobytes(), f"{what}: differs at {np.argwhere(got != ref)[:6].tolist()}"


def test_matches_the_host_walk_bit_for_bit_on_the_case_set():
    images = _case_images()
    got, over = _launch(images, C.LIMITS, 8)
    ref = _host(images, C.LIMITS, 8, key="cases")
    assert over.tolist() == [0] * len(images)
    for i, (g, r) in enumerate(zip(got, ref)):
        _same(g, r, f"image {i}")
    allv = np.concatenate([r.reshape(-1) for r in ref])
    assert (allv == -1).any() and (allv == 0).any() and (allv == 1).any() and ((allv > 0) & (allv < 1)).sum() > 100


def test_batch_order_is_free_and_one_call_per_image_equals_the_batch():
    images = _case_images()
    gt = _gt_dev(images, C.LIMITS, 8)
    ref = _host(images, C.LIMITS, 8, key="cases")
    got, over = _launch(images, C.LIMITS, 8, [7, 0, 5], gt=gt)               # B = 3, img_idx out of data-set order
    assert over.tolist() == [0, 0, 0]
    for j, i in enumerate([7, 0, 5]):
        _same(got[j], ref[i], f"image {i} in a batch of three")
    for i in (1, 2, 6, 7, 10):                                               # B = 1: no proposals, one of each, P < G, no boxes, ties
        one, over = _launch(images, C.LIMITS, 8, [i], gt=gt)
        assert over.tolist() == [0]
        _same(one[0], ref[i], f"image {i} alone")
    assert len(images[1][3]) == 0 and len(images[1][1]) > 0 and len(images[7][1]) == 0 and len(images[7][3]) > 0


@pytest.mark.parametrize("limit", [7, 64, 65])
def test_p_at_the_limit_and_one_either_side(limit):
    images = [C.seeded_image(100 + P, P, 9) for P in (limit - 1, limit, limit + 1)] + [C.seeded_image(5, 0, 0), C.seeded_image(6, 3, 0)]
    got, over = _launch(images, (limit, None), 8)
    assert over.tolist() == [0] * 5
    for i, (g, r) in enumerate(zip(got, _host(images, (limit, None), 8))):
        _same(g, r, f"limit {limit}, image {i}")


def test_caps_hand_back_exactly_the_image_beyond_them():
    from cddmsl_amd import hip
    MP, MG = hip.PROPOSAL_COVER_MAX_PROPOSALS, hip.PROPOSAL_COVER_MAX_GT
    assert (MP, MG) == (2048, 512)
    shapes = [(MP, 5), (MP + 1, 5), (40, 7), (12, MG), (12, MG + 1), (130, 3)]
    images = [C.seeded_image(300 + k, P, G, num_bits=2) for k, (P, G) in enumerate(shapes)]
    limits, A = (1000, None), 2
    boxes, logits, off, idx, coff, gc = _inputs(images, list(range(len(images))))
    n = sum(gc)
    cover = torch.full((len(limits), A, n), -77.0, device=DEV, dtype=torch.float32)
    over = torch.full((len(images),), -77, device=DEV, dtype=torch.int32)
    gt = _gt_dev(images, limits, A)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    st = hip.lib().cddmsl_proposal_cover(p(boxes), p(logits), p(off), p(idx), len(images), logits.numel(), p(gt.boxes), p(gt.rng), p(gt.off), gt.n_images,
                                        gt.n_boxes, p(gt.limits), len(limits), A, p(coff), n, p(cover), p(over), hip.stream_ptr())
    torch.cuda.synchronize()
    assert st == 0 and over.tolist() == [0, 1, 0, 0, 1, 0]
    cover = cover.cpu().numpy()
    s = np.concatenate([[0], np.cumsum(gc)])
    ref = _host([im for k, im in enumerate(images) if k not in (1, 4)], limits, A)
    for k, r in zip([0, 2, 3, 5], ref):
        _same(np.ascontiguousarray(cover[:, :, s[k]: s[k + 1]]), r, f"shape {shapes[k]}")
    for k in (1, 4):                                                          # handed back: none of its slots was touched
        assert (cover[:, :, s[k]: s[k + 1]] == -77).all()


def test_equal_logits_rank_stably_and_a_nan_ranks_last():
    gt, rng, p, lg = C.tie_case()
    images = [(gt, rng, p, lg), C.seeded_image(8, 20, 4)]
    limits = (100, 129, None)
    got, over = _launch(images, limits, 8)
    ref = _host(images, limits, 8)
    assert over.tolist() == [0, 0]
    _same(got[0], ref[0], "ties") or _same(got[1], ref[1], "plain")
    assert got[0][2, 0, 0] == 1.0 and got[0][1, 0, 0] < 1.0 and got[0][0, 0, 0] < 1.0      # the NaN proposal is rank 129 of 130


def test_every_slot_is_written_and_nothing_beyond():
    from cddmsl_amd import hip
    images = _case_images()
    batch = [3, 1, 8, 7, 0]
    boxes, logits, off, idx, coff, gc = _inputs(images, batch)
    n, L, A, TAIL = sum(gc), 3, 8, 64
    buf = torch.full((L * A * n + TAIL,), -77.0, device=DEV, dtype=torch.float32)
    over = torch.full((len(batch) + TAIL,), -77, device=DEV, dtype=torch.int32)
    gt = _gt_dev(images, C.LIMITS, A)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    st = hip.lib().cddmsl_proposal_cover(p(boxes), p(logits), p(off), p(idx), len(batch), logits.numel(), p(gt.boxes), p(gt.rng), p(gt.off), gt.n_images,
                                        gt.n_boxes, p(gt.limits), L, A, p(coff), n, p(buf), p(over), hip.stream_ptr())
    torch.cuda.synchronize()
    assert st == 0 and over[: len(batch)].tolist() == [0] * len(batch)
    assert (buf[-TAIL:] == -77).all() and (over[-TAIL:] == -77).all()
    cover = buf[: L * A * n].cpu().numpy().reshape(L, A, n)
    assert not (cover == -77).any()                                           # sentinel gone from every slot
    ref = _host(images, C.LIMITS, 8, key="cases")
    _same(cover, np.concatenate([ref[i] for i in batch], axis=2), "batch")


def test_two_runs_give_identical_bytes():
    from cddmsl_amd import hip
    images = _case_images()
    gt = _gt_dev(images, C.LIMITS, 8)
    boxes, logits, off, idx, coff, gc = _inputs(images, list(range(len(images))))
    first = hip.proposal_cover(boxes, logits, off, idx, coff, sum(gc), gt)
    junk = [torch.full((1 << 18,), v, device=DEV, dtype=torch.float32) for v in (-1.0, 3.5)]      # dirty the allocator's blocks
    del junk
    second = hip.proposal_cover(boxes, logits, off, idx, coff, sum(gc), gt)
    torch.cuda.synchronize()
    for x, y in zip(first, second):
        assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes()


def test_cabi_checks_its_arguments_and_writes_nothing_when_it_refuses():
    from cddmsl_amd import hip
    from cddmsl_amd._lib import HipLibraryError
    images = _case_images()
    batch = [2, 6]
    boxes, logits, off, idx, coff, gc = _inputs(images, batch)
    n = sum(gc)
    gt = _gt_dev(images, C.LIMITS, 8)
    cover = torch.full((3 * 8 * n,), -77.0, device=DEV, dtype=torch.float32)
    over = torch.full((len(batch),), -77, device=DEV, dtype=torch.int32)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    base = dict(boxes=p(boxes), off=p(off), B=len(batch), P=logits.numel(), G=gt.n_boxes, NI=gt.n_images, L=3, A=8, Gb=n, cover=p(cover), over=p(over))

    def call(**kw):
        a = dict(base, **kw)
        return hip.lib().cddmsl_proposal_cover(a["boxes"], p(logits), a["off"], p(idx), a["B"], a["P"], p(gt.boxes), p(gt.rng), p(gt.off), a["NI"], a["G"],
                                              p(gt.limits), a["L"], a["A"], p(coff), a["Gb"], a["cover"], a["over"], hip.stream_ptr())
    bad = [dict(L=0), dict(L=hip.PROPOSAL_COVER_MAX_LIMITS + 1), dict(A=0), dict(A=hip.PROPOSAL_COVER_MAX_RANGES + 1), dict(B=-1), dict(P=-1),
           dict(G=-1), dict(NI=-1), dict(Gb=-1), dict(boxes=ctypes.c_void_p(boxes.data_ptr() + 4)), dict(off=None), dict(over=None),
           dict(cover=None), dict(boxes=None)]
    for kw in bad:
        assert call(**kw) == 1, kw
    torch.cuda.synchronize()
    assert (cover == -77).all() and (over == -77).all()                      # a refused call writes nothing
    assert call(B=0) == 0
    torch.cuda.synchronize()
    assert (cover == -77).all() and (over == -77).all()
    assert call() == 0
    torch.cuda.synchronize()
    ref = _host(images, C.LIMITS, 8, key="cases")
    _same(cover.cpu().numpy().reshape(3, 8, n), np.concatenate([ref[i] for i in batch], axis=2), "after the refusals")
    with pytest.raises(ValueError, match="limits"):
        hip.ProposalGroundTruth.from_host([(g, r) for g, r, _, _ in images], (1, 2, 3, 4, 5), 8, DEV)
    with pytest.raises(HipLibraryError):
        hip.proposal_cover(boxes.cpu(), logits.cpu(), off.cpu(), idx.cpu(), coff.cpu(), n, gt)


@pytest.mark.parametrize("kind", ["coco", "proposal", "voc"])
@pytest.mark.parametrize("n_items", [0, 2])
def test_ground_truth_from_host_packs_empty_and_boxless_items(kind, n_items):
    """the three ground-truth classes' ``from_host`` on no item at all and on two items of which the first has no box: dtype, shape and
    values of every tensor against the numpy built here, ``off``, the image / row count and the box count"""
    from cddmsl_amd import hip
    b64 = np.array([[1.0, 2.0, 30.5, 40.25], [5.0, 6.0, 7.0, 8.0], [0.0, 0.0, 100.0, 50.0]])
    three = {"coco": (b64, np.array([10.0, 2.5, 5000.0]), np.array([False, True, False]), np.array([2, 0, 1], dtype=np.int64)),
             "proposal": (b64.astype(np.float32), np.array([1, 0, 9], dtype=np.uint8)),
             "voc": (b64, np.array([False, True, False]))}[kind]
    items = [tuple(f[:0] for f in three), three][:n_items]
    G, off = 3 * (n_items // 2), [0, 0, 3][: n_items + 1]
    if kind == "coco":
        gt = hip.CocoGroundTruth.from_host(items, [0.5, 0.75], [(0.0, 1e10), (0.0, 1024.0)], DEV)
        got = [gt.xywh, gt.area, gt.crowd, gt.cls]
        want = [(torch.float64, (G, 4)), (torch.float64, (G,)), (torch.uint8, (G,)), (torch.int64, (G,))]
        assert gt.n_images == n_items and gt.thrs.cpu().tolist() == [0.5, 0.75] and gt.rngs.cpu().tolist() == [[0.0, 1e10], [0.0, 1024.0]]
        assert gt.thrs.dtype == gt.rngs.dtype == torch.float64
    elif kind == "proposal":
        gt = hip.ProposalGroundTruth.from_host(items, (100, None, 5000, -3), 4, DEV)
        got, want = [gt.boxes, gt.rng], [(torch.float32, (G, 4)), (torch.uint8, (G,))]
        assert gt.n_images == n_items and gt.n_boxes == G and gt.num_ranges == 4
        assert gt.limits.dtype == torch.int32 and gt.limits.cpu().tolist() == [100, 2048, 2048, 0]       # None and beyond the cap: the cap
    else:
        gt = hip.VocGroundTruth.from_host(items, [0.5, 0.7], DEV)
        got, want = [gt.boxes, gt.difficult], [(torch.float64, (G, 4)), (torch.uint8, (G,))]
        assert gt.n_rows == n_items and gt.n_boxes == G and gt.thrs.dtype == torch.float64 and gt.thrs.cpu().tolist() == [0.5, 0.7]
    assert gt.off.dtype == torch.int64 and gt.off.is_cuda and gt.off.cpu().tolist() == off
    for t, (dtype, shape), field in zip(got, want, three):
        assert t.is_cuda and t.is_contiguous() and t.dtype == dtype and tuple(t.shape) == shape
        assert np.array_equal(t.cpu().numpy(), field[:G].astype(t.cpu().numpy().dtype))


# ------------------------------------------------------------------------------------------------ the evaluator
def _feed(ev, items, per_call):
    from cddmsl_amd.structures import Boxes, Instances
    for s in range(0, len(items), per_call):
        inputs, outputs = [], []
        for d, boxes, logits in items[s: s + per_call]:
            inst = Instances((d["height"], d["width"]))
            inst.proposal_boxes = Boxes(torch.from_numpy(boxes.copy()).to(DEV))
            inst.objectness_logits = torch.from_numpy(logits.copy()).to(DEV)
            inputs.append({"image_id": d["image_id"]}); outputs.append({"proposals": inst})
        ev.process(inputs, outputs)


def _equal_results(a, b):
    assert list(a) == list(b) == ["box_proposals"] and list(a["box_proposals"]) == list(b["box_proposals"])
    for k in a["box_proposals"]:
        x, y = a["box_proposals"][k], b["box_proposals"][k]
        assert type(x) is type(y) is float and (x == y or (x != x and y != y)), (k, x, y)


def test_device_evaluator_equals_the_host_evaluator_including_the_fallback():
    from cddmsl_amd import evaluation as E, hip
    items = list(C.dataset())
    gt, _, p, lg = C.seeded_image(77, hip.PROPOSAL_COVER_MAX_PROPOSALS + 52, 6)          # beyond the cap: the host walks it
    items.append(({"image_id": "big", "height": 2048, "width": 2048,
                   "annotations": [{"bbox": [float(v) for v in b], "category_id": 0, "iscrowd": 0} for b in gt]}, p, lg))
    dicts = [d for d, _, _ in items]

    def host():
        ev = E.ProposalRecallEvaluator(dicts)
        _feed(ev, items, 4)
        return ev.evaluate()
    ref = _cached("host_result", host)
    assert all(0 < v < 100 for v in ref["box_proposals"].values())
    for per_call in (1, 5):
        ev = E.ProposalRecallEvaluator(dicts, device=DEV)
        _feed(ev, items, per_call)
        assert ev._cover == {} and all(e["cover"].is_cuda and e["over"].is_cuda for e in ev._batches)      # nothing came to the host
        rec = ev._device_records()
        assert sum(int(e["over"].sum()) for e in ev._batches) == 1 and len(rec) == len(items)
        _equal_results(ev.evaluate(), ref)
    ev.reset()
    assert all(v != v for v in ev.evaluate()["box_proposals"].values())


# ------------------------------------------------------------------------------------------------ the models
def _cfg(*opts):
    from cddmsl_amd.config import get_cfg
    cfg = get_cfg()
    cfg.merge_from_file(os.path.join(ROOT, "configs", "VOC-Experiments", "faster_rcnn_CLIP_R_50_C4.yaml"))
    cfg.merge_from_list(["MODEL.DEVICE", DEV, "MODEL.RPN.PRE_NMS_TOPK_TEST", 300, "MODEL.RPN.POST_NMS_TOPK_TEST", 50,
                         "MODEL.ROI_HEADS.SCORE_THRESH_TEST", 0.0, "TEST.DETECTIONS_PER_IMAGE", 20, *opts])
    return cfg


def _model(cfg):
    from cddmsl_amd import synthetic
    from cddmsl_amd.modeling import build_model
    model = build_model(cfg)
    own = model.state_dict()
    model.load_state_dict({k: v for k, v in synthetic.make_state_dict(0).items() if k in own}, strict=False)
    return model.eval()


def _inputs_64x96():
    r = np.random.RandomState(3)
    return [{"image": torch.from_numpy(r.randint(0, 256, (3, 64, 96), dtype=np.uint8)), "height": 128, "width": 192, "image_id": f"t{k}"}
            for k in range(2)]


def test_the_switch_adds_proposals_and_leaves_the_detections_bitwise():
    from cddmsl_amd import evaluation as E
    inputs = _inputs_64x96()
    off = _model(_cfg())
    out_off = off(inputs)
    assert all(list(o) == ["instances"] for o in out_off)                    # switch off: no "proposals" key
    cfg = _cfg("TEST.PROPOSAL_RECALL", True)
    on = _model(cfg)
    out_on = on(inputs)
    assert all(list(o) == ["instances", "proposals"] for o in out_on)
    for a, b in zip(out_off, out_on):
        for f in ("pred_boxes", "scores", "pred_classes"):
            x, y = a["instances"].get(f), b["instances"].get(f)
            x, y = getattr(x, "tensor", x), getattr(y, "tensor", y)
            assert x.dtype == y.dtype and torch.equal(x, y), f
        assert b["proposals"].image_size == (128, 192) and 0 < len(b["proposals"]) <= 50
    # a ProposalNetwork on the detector's backbone.* / proposal_generator.* returns the proposals the detector attaches
    pn = _model(_cfg("MODEL.META_ARCHITECTURE", "ProposalNetwork"))
    assert type(pn).__name__ == "ProposalNetwork" and not hasattr(pn, "roi_heads")
    out_pn = pn(inputs)
    for a, b in zip(out_pn, out_on):
        assert list(a) == ["proposals"]
        assert torch.equal(a["proposals"].proposal_boxes.tensor, b["proposals"].proposal_boxes.tensor)
        assert torch.equal(a["proposals"].objectness_logits, b["proposals"].objectness_logits)
    # and box_proposals appears next to the detector's own task, the same with the walk on the device and on the host
    dicts = [{"image_id": i["image_id"], "annotations": [{"bbox": [8.0, 16.0, 100.0, 90.0], "category_id": 0},
                                                         {"bbox": [60.5, 20.0, 180.0, 120.25], "category_id": 1, "area": 900}]} for i in inputs]

    class Counting:
        def reset(self):
            self.n = 0

        def process(self, inputs, outputs):
            self.n += len(outputs)

        def evaluate(self):
            return {"bbox": {"AP": float(self.n)}}

    res = E.inference_on_dataset(on, [[i] for i in inputs], E.with_proposal_recall(Counting(), on, cfg, dicts))
    assert list(res) == ["bbox", "box_proposals"] and res["bbox"] == {"AP": 2.0} and on.training is False
    host = E.ProposalRecallEvaluator(dicts)
    host.process(inputs, out_on)
    _equal_results({"box_proposals": res["box_proposals"]}, host.evaluate())
    only = E.inference_on_dataset(pn, [[i] for i in inputs], E.with_proposal_recall(Counting(), pn, cfg, dicts))
    _equal_results(only, host.evaluate())                                    # a ProposalNetwork reports box_proposals alone
    assert E.with_proposal_recall("ev", off, _cfg(), dicts) == "ev"
