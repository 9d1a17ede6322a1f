"""CPU: proposal recall on the host.  ``evaluation.proposal_cover_host`` + ``proposal_recall_stats`` reproduce the reference's
``_evaluate_box_proposals`` (tests/golden/ref_proposal_recall.npz, written by tests/golden/make_golden_proposal_recall.py from the
reference's own code) BIT FOR BIT -- sorted cover values, num_pos, recalls and ar for all eight named ranges at the limits 100, 1000
and none; the evaluator's dictionary is the fixture's ar x 100; ``DatasetEvaluators`` merges and refuses duplicates; the trainer
refuses a ``ProposalNetwork``; the range-edge and float32-area rules; ``run_eval_only`` prints the ``box_proposals`` line under
``TEST.PROPOSAL_RECALL`` (off: as before; the TTA pass: none; a proposals-only model: that line alone)."""
import math
import os

import numpy as np
import pytest
import torch

import proposal_recall_cases as C
from cddmsl_amd import evaluation as E
from cddmsl_amd.structures import Boxes, Instances

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_proposal_recall.npz")


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@pytest.fixture(scope="module")
def items():
    return C.dataset()


@pytest.fixture(scope="module")
def covers(items):
    """per image: the host walk's cover [3 limits, 8 ranges, g] over the non-crowd boxes"""
    gt = E.proposal_ground_truth([d for d, _, _ in items])
    return [E.proposal_cover_host(b, l, *gt[d["image_id"]], limits=C.LIMITS) for d, b, l in items]


def _outputs(items):
    out = []
    for d, boxes, logits in items:
        inst = Instances((d["height"], d["width"]))
        inst.proposal_boxes = Boxes(torch.from_numpy(boxes.copy()))
        inst.objectness_logits = torch.from_numpy(logits.copy())
        out.append({"proposals": inst})
    return out


def test_cases_are_the_fixtures_inputs(golden, items):
    assert int(golden["n_images"]) == len(items) == 12
    for k, (d, boxes, logits) in enumerate(items):
        assert np.array_equal(golden[f"in/{k}/boxes"], boxes) and np.array_equal(golden[f"in/{k}/logits"], logits)
        assert np.array_equal(golden[f"in/{k}/gt"], np.asarray([a["bbox"] for a in d["annotations"]], dtype=np.float64).reshape(-1, 4))
        assert np.array_equal(golden[f"in/{k}/crowd"], [a["iscrowd"] for a in d["annotations"]])
    assert sorted(len(b) for _, b, _ in items)[-2:] == [1200, 1200] and {0, 1, 99, 100, 101} <= {len(b) for _, b, _ in items}


@pytest.mark.parametrize("a", range(8))
def test_host_walk_reproduces_the_reference(golden, covers, a):
    name = E.PROPOSAL_AREA_NAMES[a]
    for li, limit in enumerate(C.LIMITS):
        st = E.proposal_recall_stats(np.concatenate([c[li, a] for c in covers]))
        key = f"{name}/{limit}"
        assert st["num_pos"] == int(golden[f"num_pos/{key}"]), key
        assert st["gt_overlaps"].numpy().tobytes() == golden[f"gt_overlaps/{key}"].tobytes(), key
        assert st["recalls"].numpy().tobytes() == golden[f"recalls/{key}"].tobytes(), key
        assert np.float32(st["ar"].item()).tobytes() == golden[f"ar/{key}"].tobytes(), key


def test_fixture_covers_the_listed_situations(golden, items, covers):
    # exact ties and an IoU of exactly 1; boxes never reached (P < G); uncounted boxes of an image without proposals
    assert (covers[0][2, 0] == 1.0).sum() >= 2 and (covers[10][2, 0] == 1.0).sum() == 2
    assert (covers[6][2, 0] == 0.0).sum() >= 5 and (covers[1] == -1).all() and covers[7].shape[-1] == 0
    assert (covers[9][:, 0] == 0.0).all() and (covers[9][:, 1] == -1).all()          # nothing overlaps; no small box at all
    # the limits matter: box 0 of images 3..5 is only covered by the lowest-ranked proposal
    assert covers[3][0, 0, 0] > 0.9 and covers[4][0, 0, 0] > 0.9 and covers[5][0, 0, 0] < 0.5 and covers[5][1, 0, 0] > 0.9
    assert (covers[11][1, 0, :3] < 0.5).all() and (covers[11][2, 0, :3] > 0.9).all()
    assert float(golden["ar/all/100"]) < float(golden["ar/all/1000"]) < float(golden["ar/all/None"])


@pytest.mark.parametrize("shard", [1, 5])
def test_evaluator_dictionary_is_the_fixture(golden, items, shard):
    ev = E.ProposalRecallEvaluator([d for d, _, _ in items])
    outs = _outputs(items)
    for k in range(0, len(items), shard):
        ev.process([d for d, _, _ in items[k: k + shard]], outs[k: k + shard])
    res = ev.evaluate()
    assert list(res) == ["box_proposals"]
    assert list(res["box_proposals"]) == ["AR@100", "ARs@100", "ARm@100", "ARl@100", "AR@1000", "ARs@1000", "ARm@1000", "ARl@1000"]
    for limit in (100, 1000):
        for name, suffix in (("all", ""), ("small", "s"), ("medium", "m"), ("large", "l")):
            want = float(torch.from_numpy(golden[f"ar/{name}/{limit}"]).item() * 100)
            assert res["box_proposals"][f"AR{suffix}@{limit}"] == want, (name, limit)
    ev.reset()
    empty = ev.evaluate()["box_proposals"]
    assert all(math.isnan(v) for v in empty.values())            # num_pos == 0: 0 / 0 as in the reference


def test_range_edges_and_float32_areas():
    bits = E.proposal_area_bits([1024, 9216, 1024.00001, 1023.99, 9216.001, 0, 1e10, 16384, 512 ** 2])
    names = lambda b: [n for i, n in enumerate(E.PROPOSAL_AREA_NAMES) if (b >> i) & 1]
    assert names(bits[0]) == ["all", "small", "medium"] and names(bits[1]) == ["all", "medium", "large", "96-128"]
    assert names(bits[2]) == ["all", "small", "medium"]            # 1024.00001 is 1024 after float32
    assert names(bits[3]) == ["all", "small"] and names(bits[4]) == ["all", "large", "96-128"]
    assert names(bits[5]) == ["all", "small"] and names(bits[6]) == ["all", "large", "512-inf"]
    assert names(bits[7]) == ["all", "large", "96-128", "128-256"] and names(bits[8]) == ["all", "large", "256-512", "512-inf"]
    gt = E.proposal_ground_truth([{"image_id": 3, "annotations": [
        {"bbox": [0.0, 0.0, 32.0, 32.0]}, {"bbox": [0.0, 0.0, 32.0, 32.0], "area": 5000.0}, {"bbox": [1.0, 1.0, 9.0, 9.0], "iscrowd": 1}]}])
    boxes, rng = gt["3"]
    assert boxes.dtype == np.float32 and boxes.shape == (2, 4)     # the crowd box is left out
    assert names(rng[0]) == ["all", "small", "medium"] and names(rng[1]) == ["all", "medium"]       # box area, stored area


def test_stable_rank_and_nan_last():
    gt, rng, p, lg = C.tie_case()
    cover = E.proposal_cover_host(p, lg, gt, rng, limits=(100, None), num_ranges=1)
    order = sorted(range(len(lg)), key=lambda i: (math.isnan(lg[i]), -lg[i] if not math.isnan(lg[i]) else 0.0, i))
    assert order[-1] == 5
    want = E.proposal_cover_host(p[order], np.arange(len(lg), 0, -1, dtype=np.float32), gt, rng, limits=(100, None), num_ranges=1)
    assert cover.tobytes() == want.tobytes()
    assert cover[1, 0, 0] == 1.0 and cover[0, 0, 0] < 1.0          # the perfect proposal carries the NaN: only "no limit" reaches it


def test_dataset_evaluators_merge_and_refuse_duplicates():
    class Fixed:
        def __init__(self, res):
            self.res, self.calls = res, []

        def reset(self):
            self.calls.append("reset")

        def process(self, inputs, outputs):
            self.calls.append(("process", inputs, outputs))

        def evaluate(self):
            return self.res

    a, b = Fixed({"bbox": {"AP": 1.0}}), Fixed({"box_proposals": {"AR@100": 2.0}})
    both = E.DatasetEvaluators([a, b])
    both.reset()
    both.process([1], [2])
    assert a.calls == b.calls == ["reset", ("process", [1], [2])]
    assert both.evaluate() == {"bbox": {"AP": 1.0}, "box_proposals": {"AR@100": 2.0}}
    assert E.flatten_results({"set": both.evaluate()}) == {"set/bbox/AP": 1.0, "set/box_proposals/AR@100": 2.0}
    with pytest.raises(ValueError, match="bbox"):
        E.DatasetEvaluators([a, Fixed({"bbox": {"AP": 3.0}})]).evaluate()
    assert E.DatasetEvaluators([Fixed(None), Fixed(None)]).evaluate() is None          # not rank 0


def test_trainer_refuses_a_proposal_network():
    from cddmsl_amd import engine
    from cddmsl_amd.config import get_cfg
    from cddmsl_amd.registry import META_ARCH_REGISTRY
    import cddmsl_amd.modeling  # noqa: F401  (registers)
    assert "ProposalNetwork" in META_ARCH_REGISTRY
    cfg = get_cfg()
    assert cfg.TEST.PROPOSAL_RECALL is False
    cfg.merge_from_list(["MODEL.META_ARCHITECTURE", "ProposalNetwork", "MODEL.DEVICE", "cpu"])
    with pytest.raises(ValueError, match="MODEL.META_ARCHITECTURE"):
        engine.build_trainer(cfg, 1)


class _ToyDetector(torch.nn.Module):
    """two fixed detections per image, and -- when asked -- the same boxes as proposals"""

    def __init__(self, with_proposals):
        super().__init__()
        self.with_proposals = with_proposals

    def forward(self, batched_inputs):
        out = []
        for x in batched_inputs:
            h, w = x["image"].shape[-2:]
            boxes = torch.tensor([[4.0, 2.0, 40.0, 50.0], [1.0, 1.0, w / 2.0, h / 2.0]])
            o = {"instances": Instances((h, w), pred_boxes=Boxes(boxes), scores=torch.tensor([0.9, 0.3]), pred_classes=torch.tensor([1, 4]))}
            if self.with_proposals:
                p = Instances((h, w))
                p.proposal_boxes, p.objectness_logits = Boxes(boxes.clone()), torch.tensor([2.0, -1.0])
                o["proposals"] = p
            out.append(o)
        return out


class _ToyProposalNetwork(_ToyDetector):
    proposals_only = True

    def forward(self, batched_inputs):
        return [{"proposals": o["proposals"]} for o in super().forward(batched_inputs)]


def test_eval_only_reports_box_proposals_under_the_switch(tmp_path, capsys, monkeypatch):
    import argparse
    from cddmsl_amd.config import get_cfg
    from test_data_pipeline import _make_voc
    args = argparse.Namespace(voc_root=_make_voc(str(tmp_path)), voc_split="test", voc_year=2007)

    def cfg(*opts):
        c = get_cfg()
        c.merge_from_list(["MODEL.DEVICE", "cpu", "INPUT.MIN_SIZE_TEST", 0, *opts])
        return c
    plain = E.run_eval_only(_ToyDetector(False), cfg(), args, 0, 1, return_results=True)
    assert list(plain) == ["bbox"] and "box_proposals" not in capsys.readouterr().out          # the switch off: as before
    both = E.run_eval_only(_ToyDetector(True), cfg("TEST.PROPOSAL_RECALL", True), args, 0, 1, return_results=True, prefix="iter 9  ")
    assert list(both) == ["bbox", "box_proposals"] and dict(both["bbox"]) == dict(plain["bbox"])
    lines = capsys.readouterr().out.splitlines()
    assert len(lines) == 2 and all(l.startswith("iter 9  {") for l in lines) and "'box_proposals': {'AR@100'" in lines[1]
    ar = both["box_proposals"]
    assert 0.0 <= ar["AR@100"] <= 100.0 and ar["AR@1000"] == ar["AR@100"]                     # two proposals per image
    assert all(v != v or 0.0 <= v <= 100.0 for v in ar.values())                               # (no large box in these images: NaN)
    assert E.flatten_results({"voc_test": both})["voc_test/box_proposals/AR@1000"] == ar["AR@1000"]
    only = E.run_eval_only(_ToyProposalNetwork(True), cfg(), args, 0, 1, return_results=True)
    assert list(only) == ["box_proposals"] and [only["box_proposals"][k] == v or v != v for k, v in ar.items()] == [True] * 8
    # the TTA pass reports no box_proposals
    from cddmsl_amd.modeling import test_time_augmentation as T

    class Spy(torch.nn.Module):
        def __init__(self, cfg, model, *a, **k):
            super().__init__()
            self.model = model

        def forward(self, batched_inputs):
            return self.model(batched_inputs)

    monkeypatch.setattr(T, "GeneralizedRCNNWithTTA", Spy)
    tta = E.run_eval_only(_ToyDetector(True), cfg("TEST.PROPOSAL_RECALL", True, "TEST.AUG.ENABLED", True), args, 0, 1, return_results=True)
    assert list(tta) == ["bbox", "box_proposals", "bbox_TTA"]


def test_proposal_cover_lives_in_the_main_library():
    """cddmsl_proposal_cover is declared in include/cddmsl_hip.h, exported by libcddmsl_hip.so and typed by _lib.lib() from that header,
    as tests/test_cabi_host.py holds every entry point; no library, loader, header or build table beside them"""
    import ctypes
    import re
    import subprocess
    import __graft_entry__ as g
    g.build()
    from cddmsl_amd import _lib
    L = _lib.lib()
    hdr = re.sub(r"/\*.*?\*/", " ", open(_lib.HEADER_PATH).read(), flags=re.S)
    assert re.findall(r"\bint\s+(cddmsl_proposal_\w+)\s*\(", hdr) == ["cddmsl_proposal_cover"]
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    assert "cddmsl_proposal_cover" in set(re.findall(r"\bT (cddmsl_\w+)", out))
    vp, ci, cl = ctypes.c_void_p, ctypes.c_int, ctypes.c_long
    fn = L.cddmsl_proposal_cover
    assert fn.restype is ctypes.c_int and fn.argtypes == [vp] * 4 + [ci, cl, vp, vp, vp, cl, cl, vp, ci, ci, vp, cl, vp, vp, vp]
    assert not hasattr(_lib, "lib_proposal_recall") and not [n for n in dir(_lib) if n.startswith("PROPOSAL_RECALL_")]
    assert not hasattr(g, "SIDE_LIBS")
    assert not [f for _, _, files in os.walk(os.path.dirname(_lib.HEADER_PATH)) for f in files if f == "cddmsl_proposal_recall.h"]


def test_gather_to_rank0_without_a_process_group_is_the_part_itself():
    part = {"some": "records"}
    got = E.gather_to_rank0(part)
    assert isinstance(got, list) and len(got) == 1 and got[0] is part
