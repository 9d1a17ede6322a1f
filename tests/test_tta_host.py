"""Host side of test-time augmentation: the numpy restatement of Pillow's bilinear resize against the installed Pillow, the host
mapper, the box un-mapping and merge against numpy, the config defaults and the evaluation wiring.  No GPU."""
import argparse
import os

import numpy as np
import pytest
import torch

import pil_resize_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ 1. the restatement is Pillow
@pytest.mark.parametrize("pair", R.PAIRS, ids=lambda p: "%dx%d_to_%dx%d" % (p[0] + p[1]))
def test_restatement_equals_pillow(pair):
    from PIL import Image
    (h, w), (nh, nw) = pair
    img = R.seeded_image(h, w, 1000 * h + w)
    want = np.asarray(Image.fromarray(img).resize((nw, nh), Image.BILINEAR))
    got = R.resize(img, nh, nw)
    assert got.shape == want.shape == (nh, nw, 3) and got.dtype == np.uint8
    assert np.array_equal(got, want)


@pytest.mark.parametrize("pair", R.PAIRS + [((200, 40), (20, 30)), ((150, 210), (97, 136))], ids=lambda p: "%dx%d_to_%dx%d" % (p[0] + p[1]))
def test_kernel_tables_equal_the_restatement(pair):
    """the tables ``hip.tta_views`` uploads (vectorised numpy) are the restatement's scalar-loop tables, entry for entry"""
    from cddmsl_amd import hip
    (h, w), (nh, nw) = pair
    for a, b in ((w, nw), (h, nh)):
        lo, n, k, ks = hip._resample_table(a, b)
        xmin, ns, kk, ks2 = R.coeffs(a, b)
        assert ks == ks2 and k.shape == (b, ks) and lo.dtype == n.dtype == k.dtype == np.int32
        assert np.array_equal(lo, xmin) and np.array_equal(n, ns) and np.array_equal(k, np.array(kk))
        assert (k >= 0).all() and (lo + n <= a).all() and (n <= ks).all()


# ------------------------------------------------------------------------------------------------ 2. the host mapper
def _cfg(*opts):
    from cddmsl_amd.config import get_cfg
    cfg = get_cfg()
    cfg.merge_from_list(["MODEL.DEVICE", "cpu", *opts])
    return cfg


def test_dataset_mapper_tta():
    from cddmsl_amd.modeling import DatasetMapperTTA
    img = R.seeded_image(37, 53, 5)
    d = {"image": torch.from_numpy(np.ascontiguousarray(img.transpose(2, 0, 1))), "height": 74, "width": 106, "image_id": "7"}
    sizes = (24, 37, 64)
    cfg = _cfg("TEST.AUG.MIN_SIZES", sizes, "TEST.AUG.MAX_SIZE", 70)
    out = DatasetMapperTTA(cfg)(d)
    want = R.views(img, sizes, 70, True)
    assert [w[1] for w in want] == [(24, 34, False), (24, 34, True), (37, 53, False), (37, 53, True), (49, 70, False), (49, 70, True)]
    assert len(out) == 6                                                   # (64 -> 64 x 92 exceeds MAX_SIZE 70: 49 x 70; 37 is the identity)
    for o, (pix, (nh, nw, f)) in zip(out, want):
        assert o["transforms"] == (74, 106, 37, 53, nh, nw, f)
        assert o["image"].dtype == torch.uint8 and tuple(o["image"].shape) == (3, nh, nw) and o["image"].is_contiguous()
        assert np.array_equal(o["image"].numpy().transpose(1, 2, 0), pix)
        assert o["height"] == 74 and o["width"] == 106 and o["image_id"] == "7"
    assert np.array_equal(out[2]["image"].numpy(), d["image"].numpy())     # the identity size is the image itself
    assert np.array_equal(out[1]["image"].numpy(), out[0]["image"].numpy()[:, :, ::-1])
    assert tuple(d["image"].shape) == (3, 37, 53) and "transforms" not in d
    half = DatasetMapperTTA(_cfg("TEST.AUG.MIN_SIZES", sizes, "TEST.AUG.MAX_SIZE", 70, "TEST.AUG.FLIP", False))(d)
    assert len(half) == 3 and [h["transforms"][4:] for h in half] == [(24, 34, False), (37, 53, False), (49, 70, False)]
    for hv, i in zip(half, (0, 2, 4)):
        assert torch.equal(hv["image"], out[i]["image"])


# ------------------------------------------------------------------------------------------------ 3. un-mapping + merge
def _views_with_duplicates():
    """four views of a 37x53 image handed for a 74x106 dataset image: plain, its mirror carrying the MIRRORED boxes of the plain view
    (coordinates on a 1/4 grid, so the mirror is exact and the un-mapped boxes are exact duplicates), another scale mirrored, and a
    repeat of the first record with the same boxes and scores (ties: the first index wins)"""
    rs = np.random.RandomState(11)
    records = [(74, 106, 37, 53, 24, 34, False), (74, 106, 37, 53, 24, 34, True), (74, 106, 37, 53, 49, 70, True), (74, 106, 37, 53, 24, 34, False)]

    def boxes(n, nh, nw):
        x = np.sort(rs.randint(0, 4 * nw + 1, (n, 2)), axis=1) / 4.0
        y = np.sort(rs.randint(0, 4 * nh + 1, (n, 2)), axis=1) / 4.0
        return np.stack([x[:, 0], y[:, 0], x[:, 1] + 0.25, y[:, 1] + 0.25], axis=1).astype(np.float32)   # may stick out: the clip is live

    b0 = boxes(40, 24, 34)
    s0 = rs.uniform(0.01, 1.0, 40).astype(np.float32)
    s0[:3] = (0.0, 1e-9, 1e-8)                                             # at or below the 1e-8 threshold: dropped
    c0 = rs.randint(0, 2, 40)
    b1 = b0.copy()
    b1[:, 0], b1[:, 2] = np.float32(34) - b0[:, 2], np.float32(34) - b0[:, 0]
    s1 = rs.uniform(0.01, 1.0, 40).astype(np.float32)
    b2, s2, c2 = boxes(30, 49, 70), rs.uniform(0.01, 1.0, 30).astype(np.float32), rs.randint(0, 2, 30)
    return [(b0, s0, c0), (b1, s1, c0.copy()), (b2, s2, c2), (b0.copy(), s0.copy(), c0.copy())], records


@pytest.mark.parametrize("topk", [20, -1])
def test_unmap_and_merge_equal_numpy(monkeypatch, topk):
    from cddmsl_amd.modeling import roi_heads as RH, test_time_augmentation as T
    from cddmsl_amd.structures import Boxes, Instances
    from oracle import ops as O
    monkeypatch.setattr(RH, "batched_nms", O.batched_nms)                  # the HIP NMS needs the GPU; the oracle's is the CPU statement of it
    per_view, records = _views_with_duplicates()
    outs = [Instances((r[4], r[5]), pred_boxes=Boxes(torch.from_numpy(b)), scores=torch.from_numpy(s), pred_classes=torch.from_numpy(c))
            for (b, s, c), r in zip(per_view, records)]
    for o, (b, _, _), r in zip(outs, per_view, records):                   # the un-mapping alone, view by view
        assert np.array_equal(T.unmap_boxes(o.pred_boxes.tensor, r).numpy(), R.unmap(b, r))
    assert np.array_equal(R.unmap(per_view[0][0], records[0]), R.unmap(per_view[1][0], records[1]))   # exact duplicates across views
    boxes, scores, classes = T.GeneralizedRCNNWithTTA._get_augmented_boxes(outs, records)
    assert boxes.dtype == torch.float32 and boxes.shape == (150, 4) and scores.shape == classes.shape == (150,)
    got = T.merge_detections(boxes, scores, classes, (74, 106), 20, 0.5, topk)
    wb, ws, wc = R.merge(per_view, records, (74, 106), 0.5, topk)
    assert got.image_size == (74, 106)
    assert np.array_equal(got.pred_boxes.tensor.numpy(), wb) and np.array_equal(got.scores.numpy(), ws)
    assert np.array_equal(got.pred_classes.numpy(), wc)
    assert len(ws) == 20 if topk == 20 else 20 < len(ws) < 147
    assert set(wc.tolist()) == {0, 1} and (np.diff(ws) <= 0).all()
    assert wb.min() >= 0 and wb[:, 2].max() <= 106 and wb[:, 3].max() <= 74
    if topk == -1:                                                         # every duplicate collapsed: no box is kept twice in a class
        keyed = {(tuple(b), int(c)) for b, c in zip(wb.tolist(), wc.tolist())}
        assert len(keyed) == len(wb)


# ------------------------------------------------------------------------------------------------ 4. config + evaluation wiring
def test_config_defaults():
    from cddmsl_amd.config import get_cfg
    a = get_cfg().TEST.AUG
    assert a.ENABLED is False and tuple(a.MIN_SIZES) == (400, 500, 600, 700, 800, 900, 1000, 1100, 1200) and a.MAX_SIZE == 4000 and a.FLIP is True
    cfg = get_cfg()
    cfg.merge_from_file(os.path.join(ROOT, "configs", "VOC-Experiments", "faster_rcnn_CLIP_R_50_C4.yaml"))
    assert cfg.TEST.AUG.ENABLED is False and cfg.TEST.DETECTIONS_PER_IMAGE == 100
    cfg.merge_from_list(["TEST.AUG.ENABLED", "True", "TEST.AUG.MIN_SIZES", "(96, 128)"])
    assert cfg.TEST.AUG.ENABLED is True and tuple(cfg.TEST.AUG.MIN_SIZES) == (96, 128) and cfg.TEST.AUG.FLIP is True


class _ToyDetector(torch.nn.Module):
    def forward(self, batched_inputs):
        from cddmsl_amd.structures import Boxes, Instances
        out = []
        for x in batched_inputs:
            h, w = x["image"].shape[-2:]
            i = int(x["image_id"])
            boxes = torch.tensor([[4.0, 2.0, 40.0, 50.0], [1.0, 1.0, w / 2.0, h / 2.0]])
            out.append({"instances": Instances((h, w), pred_boxes=Boxes(boxes), scores=torch.tensor([0.9 - 0.01 * i, 0.3 + 0.02 * i]),
                                               pred_classes=torch.tensor([i % 20, (i + 3) % 20]))})
        return out


def test_eval_only_wiring(tmp_path, monkeypatch, capsys):
    """ENABLED False: today's path, the TTA class is never constructed.  ENABLED True: the plain evaluation, then the same set
    through the TTA class, returned and printed under ``bbox_TTA``"""
    from cddmsl_amd import evaluation
    from cddmsl_amd.modeling import test_time_augmentation as T
    from test_data_pipeline import _make_voc
    base = _make_voc(str(tmp_path))
    args = argparse.Namespace(voc_root=base, voc_split="test", voc_year=2007)
    built = []

    class Spy(torch.nn.Module):
        def __init__(self, cfg, model, *a, **k):
            super().__init__()
            built.append((cfg, model))
            self.model = model

        def forward(self, batched_inputs):
            return self.model(batched_inputs)

    monkeypatch.setattr(T, "GeneralizedRCNNWithTTA", Spy)
    toy = _ToyDetector()
    cfg = _cfg("INPUT.MIN_SIZE_TEST", 0)
    plain = evaluation.run_eval_only(toy, cfg, args, 0, 1, return_results=True)
    assert built == [] and list(plain) == ["bbox"]
    assert "_TTA" not in capsys.readouterr().out
    cfg = _cfg("INPUT.MIN_SIZE_TEST", 0, "TEST.AUG.ENABLED", True)
    both = evaluation.run_eval_only(toy, cfg, args, 0, 1, return_results=True)
    assert len(built) == 1 and built[0][1] is toy and built[0][0] is cfg
    assert list(both) == ["bbox", "bbox_TTA"] and dict(both["bbox"]) == dict(plain["bbox"])
    assert dict(both["bbox_TTA"]) == dict(plain["bbox"])                   # (the spy forwards to the same detector)
    assert "bbox_TTA" in capsys.readouterr().out
    assert evaluation.run_eval_only(toy, cfg, args, 0, 1) == 0


def test_tta_wrapper_refuses_other_models_and_masks():
    from cddmsl_amd.modeling import GeneralizedRCNNWithTTA
    with pytest.raises(AssertionError, match="only supported on GeneralizedRCNN"):
        GeneralizedRCNNWithTTA(_cfg(), _ToyDetector())
