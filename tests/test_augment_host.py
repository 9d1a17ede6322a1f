"""INPUT.CROP, INPUT.MIN_SIZE_TRAIN_SAMPLING "range" and INPUT.RANDOM_FLIP "vertical" in the training mapper (cddmsl_amd/data.py),
against tests/golden/ref_augment.npz -- samples and draw sequences made by the reference's own RandomCrop / ResizeShortestEdge /
RandomFlip / transform_instance_annotations / filter_empty_instances under ``np.random.seed(s)`` (tests/golden/make_golden_augment.py).
The mapper gets ``RandomState(s)`` and has to draw in the reference's order to arrive at the same sample.  CPU only: pictures are
compared byte for byte (both sides resize with the same PIL call), boxes within 1e-4 as tests/test_data_pipeline.py does."""
import os

import numpy as np
import pytest
import torch

from cddmsl_amd import data
from cddmsl_amd.config import get_cfg

G = np.load(os.path.join(os.path.dirname(__file__), "golden", "ref_augment.npz"))
N_SAMPLES = 4
# the settings of the fixture's three draw sequences (make_golden_augment.py SEQUENCES)
SEQUENCES = [(("relative_range", (0.9, 0.9)), tuple(range(480, 801, 32)), "choice", "horizontal"),
             (("absolute_range", (200, 300)), (480, 800), "range", "vertical"),
             (None, (480, 800), "range", "none")]


def _cfg(crop, sizes, sampling, max_size, flip, device_resize=False, fmt="RGB"):
    cfg = get_cfg()
    cfg.merge_from_list(["INPUT.MIN_SIZE_TRAIN", tuple(sizes), "INPUT.MIN_SIZE_TRAIN_SAMPLING", sampling, "INPUT.MAX_SIZE_TRAIN", max_size,
                         "INPUT.RANDOM_FLIP", flip, "INPUT.FORMAT", fmt, "DATALOADER.DEVICE_RESIZE", device_resize])
    if crop is not None:
        cfg.merge_from_list(["INPUT.CROP.ENABLED", True, "INPUT.CROP.TYPE", crop[0], "INPUT.CROP.SIZE", list(crop[1])])
    return cfg


def _png(path, arr):
    from PIL import Image
    Image.fromarray(arr).save(path)
    return path


def _fixture_cfg(n, **kw):
    return _cfg((str(G[f"crop_type{n}"]), G[f"crop_size{n}"].tolist()), G[f"min_sizes{n}"].tolist(), str(G[f"sampling{n}"]),
                int(G[f"max_size{n}"]), str(G[f"flip{n}"]), **kw)


def _fixture_dict(n, tmp_path):
    img = G[f"img{n}"]
    return {"file_name": _png(str(tmp_path / f"a{n}.png"), img), "data_dt_file_name": _png(str(tmp_path / f"t{n}.png"), 255 - img),
            "height": img.shape[0], "width": img.shape[1], "image_id": str(n),
            "annotations": [{"bbox": b.tolist(), "category_id": int(c)} for b, c in zip(G[f"boxes_in{n}"], G[f"classes_in{n}"])]}


def test_config_defaults():
    c = get_cfg().INPUT
    assert c.CROP == {"ENABLED": False, "TYPE": "relative_range", "SIZE": [0.9, 0.9]}
    assert c.MIN_SIZE_TRAIN_SAMPLING == "choice" and c.RANDOM_FLIP == "horizontal"


@pytest.mark.parametrize("n", range(N_SAMPLES))
def test_sample_matches_reference(n, tmp_path):
    """one full sample per crop type: crop -> resize ("choice" / "range") -> flip (vertical on samples 1 and 2), picture, twin, boxes"""
    m = data.DatasetMapper(_fixture_cfg(n), True, np.random.RandomState(int(G[f"seed{n}"])))
    d = _fixture_dict(n, tmp_path)
    out = m(d)
    assert np.array_equal(out["image"].numpy().transpose(1, 2, 0), G[f"final{n}"])
    assert np.array_equal(out["image_trgt"].numpy().transpose(1, 2, 0), G[f"twin_final{n}"])
    assert (out["height"], out["width"]) == G[f"img{n}"].shape[:2]                         # the ORIGINAL image's size
    inst = out["instances"]
    assert inst.image_size == G[f"final{n}"].shape[:2]
    assert inst.gt_boxes.tensor.shape == G[f"boxes_out{n}"].shape
    assert np.allclose(inst.gt_boxes.tensor.numpy(), G[f"boxes_out{n}"], atol=1e-4)
    assert np.array_equal(inst.gt_classes.numpy(), G[f"classes_out{n}"])
    outside = G[f"outside{n}"]
    assert outside.any() and len(inst) == int((~outside).sum())                            # the box outside the window is gone
    assert np.array_equal(inst.gt_classes.numpy(), G[f"classes_in{n}"][~outside])


def test_fixture_covers_the_options():
    kinds = [(str(G[f"crop_type{n}"]), str(G[f"sampling{n}"]), str(G[f"flip{n}"]), int(G[f"flipped{n}"])) for n in range(N_SAMPLES)]
    assert {k[0] for k in kinds} == {"relative", "relative_range", "absolute", "absolute_range"}
    assert {k[1] for k in kinds} == {"choice", "range"}
    assert sum(k[2] == "vertical" and k[3] for k in kinds) >= 2 and any(not k[3] for k in kinds)


def _position_image(h, w):
    """a picture whose pixel (y, x) spells its own position, so that a crop shows its window"""
    yy, xx = np.mgrid[0:h, 0:w]
    return np.stack([yy % 256, xx % 256, (yy // 256) * 16 + xx // 256], axis=2).astype(np.uint8)


@pytest.mark.parametrize("n", range(len(SEQUENCES)))
def test_draw_sequence_matches_reference(n, tmp_path):
    """16 consecutive samples from one RandomState: window, size and flip decision of every sample -- any draw out of order, missing
    or in excess shifts everything behind it"""
    crop, sizes, sampling, flip = SEQUENCES[n]
    # (the device record keeps the cropped picture unresized: its first pixel shows the window's origin)
    m = data.DatasetMapper(_cfg(crop, sizes, sampling, 1333, flip, device_resize=True), True, np.random.RandomState(int(G[f"sequence_seed{n}"])))
    p = _png(str(tmp_path / "z.png"), _position_image(375, 500))
    seen = []
    for _ in range(16):
        out = m({"file_name": p, "height": 375, "width": 500, "image_id": "z", "annotations": []})
        a, rec = out["image"].numpy(), out[data.DEVICE_RESIZE_KEY]
        y0, x0 = int(a[0, 0, 0]) + 256 * (int(a[0, 0, 2]) // 16), int(a[0, 0, 1]) + 256 * (int(a[0, 0, 2]) % 16)
        seen.append((y0, x0, a.shape[0], a.shape[1], rec["size"][0], rec["size"][1], int(rec["flip"] != 0)))
    assert seen == [tuple(r) for r in G[f"sequence{n}"].tolist()]


def test_vertical_flip_draws_match_reference(tmp_path):
    """RandomFlip(vertical=True): the decision is ``uniform() < 0.5``; seen through the box, y -> newh - y with the corners re-sorted"""
    class Rng:                                                      # the size is scripted, the flip draws come from the seeded state
        def __init__(self):
            self.g = np.random.RandomState(123)

        def choice(self, a):
            return a[0]

        def uniform(self):
            return self.g.uniform()

    m = data.DatasetMapper(_cfg(None, (48,), "choice", 100, "vertical"), True, Rng())
    p = _png(str(tmp_path / "v.png"), _position_image(24, 36))
    seen = []
    for _ in range(32):
        out = m({"file_name": p, "height": 24, "width": 36, "image_id": "v", "annotations": [{"bbox": [3.0, 2.0, 9.0, 7.0], "category_id": 1}]})
        img, b = out["image"].numpy(), out["instances"].gt_boxes.tensor[0].tolist()
        assert img.shape == (3, 48, 72)
        flipped = bool(img[0, 0, 0] > img[0, -1, 0])                # plane 0 holds the row index
        assert np.allclose(b, [6.0, 48 - 14.0, 18.0, 48 - 4.0] if flipped else [6.0, 4.0, 18.0, 14.0], atol=1e-4)
        seen.append(flipped)
    assert seen == G["vflip_draws"].tolist() and 0 < sum(seen) < 32


def test_defaults_draw_only_choice_and_uniform(tmp_path):
    """the unchanged-behaviour guard: with the shipped defaults a sample costs one ``choice`` and one ``uniform``, in that order"""
    calls = []

    class TwoDraws:
        def choice(self, a):
            calls.append("choice")
            return a[0]

        def uniform(self):
            calls.append("uniform")
            return 0.75

    cfg = get_cfg()
    cfg.merge_from_list(["INPUT.MIN_SIZE_TRAIN", (40,), "INPUT.MAX_SIZE_TRAIN", 100, "INPUT.FORMAT", "RGB"])
    img = _position_image(24, 36)
    p = _png(str(tmp_path / "d.png"), img)
    out = data.DatasetMapper(cfg, True, TwoDraws())({"file_name": p, "height": 24, "width": 36, "image_id": "d", "annotations": []})
    assert calls == ["choice", "uniform"]
    assert np.array_equal(out["image"].numpy().transpose(1, 2, 0), data.resize_image(img, 40, 60))


def test_test_mapper_ignores_the_training_options(tmp_path):
    """``build_augmentation(cfg, False)``: MIN_SIZE_TEST, "choice", no crop, no flip -- and a scripted rng with ``choice`` alone suffices"""
    class ChoiceOnly:
        def choice(self, a):
            assert list(a) == [32]
            return a[0]

    cfg = _cfg(("absolute", (10, 10)), (480, 800), "range", 1333, "vertical")
    cfg.merge_from_list(["INPUT.MIN_SIZE_TEST", 32, "INPUT.MAX_SIZE_TEST", 100])
    img = _position_image(24, 36)
    p = _png(str(tmp_path / "t.png"), img)
    out = data.DatasetMapper(cfg, False, ChoiceOnly())({"file_name": p, "height": 24, "width": 36, "image_id": "t", "annotations": []})
    assert np.array_equal(out["image"].numpy().transpose(1, 2, 0), data.resize_image(img, 32, 48)) and "instances" not in out
    # ... even where the training mapper refuses the settings
    bad = _cfg(("no_such_type", (10, 10)), (480, 640, 800), "range", 1333, "diagonal")
    data.DatasetMapper(bad, False)


@pytest.mark.parametrize("key,edit", [
    ("INPUT.CROP.TYPE", ["INPUT.CROP.ENABLED", True, "INPUT.CROP.TYPE", "relative_rnage"]),
    ("INPUT.MIN_SIZE_TRAIN_SAMPLING", ["INPUT.MIN_SIZE_TRAIN_SAMPLING", "uniform"]),
    ("INPUT.MIN_SIZE_TRAIN", ["INPUT.MIN_SIZE_TRAIN_SAMPLING", "range", "INPUT.MIN_SIZE_TRAIN", (480, 640, 800)]),
    ("INPUT.MIN_SIZE_TRAIN", ["INPUT.MIN_SIZE_TRAIN_SAMPLING", "range", "INPUT.MIN_SIZE_TRAIN", (800,)]),
    ("INPUT.RANDOM_FLIP", ["INPUT.RANDOM_FLIP", "both"]),
    ("INPUT.RANDOM_FLIP", ["INPUT.RANDOM_FLIP", "Horizontal"])])
def test_refusals_name_the_key(key, edit):
    cfg = get_cfg()
    cfg.merge_from_list(edit)
    with pytest.raises(ValueError, match=key.replace(".", r"\.")):
        data.DatasetMapper(cfg, True)


def test_unknown_crop_type_is_fine_while_crop_is_off():
    cfg = get_cfg()
    cfg.merge_from_list(["INPUT.CROP.TYPE", "whatever"])
    assert data.DatasetMapper(cfg, True).crop_type is None


@pytest.mark.parametrize("n", range(N_SAMPLES))
@pytest.mark.parametrize("fmt", ["RGB", "BGR"])
def test_device_record_carries_the_crop(n, fmt, tmp_path):
    """DATALOADER.DEVICE_RESIZE: the sample holds the cropped [ch, cw, 3] RGB array (a contiguous copy of the window only), tables
    for (crop size -> new size), the flip code 0 / 1 / 2, and the same boxes as the host path"""
    from cddmsl_amd.resample import packed_table
    seed = int(G[f"seed{n}"])
    d = _fixture_dict(n, tmp_path)
    out = data.DatasetMapper(_fixture_cfg(n, device_resize=True, fmt=fmt), True, np.random.RandomState(seed))(d)
    host = data.DatasetMapper(_fixture_cfg(n, fmt=fmt), True, np.random.RandomState(seed))(d)
    y0, x0, ch, cw = G[f"window{n}"].tolist()
    newh, neww = G[f"final{n}"].shape[:2]
    rec = out[data.DEVICE_RESIZE_KEY]
    for k, src in (("image", G[f"img{n}"]), ("image_trgt", 255 - G[f"img{n}"])):
        assert out[k].dtype == torch.uint8 and tuple(out[k].shape) == (ch, cw, 3) and out[k].is_contiguous()
        assert np.array_equal(out[k].numpy(), src[y0:y0 + ch, x0:x0 + cw])
        assert out[k].untyped_storage().nbytes() == ch * cw * 3                                # no view into the whole picture
    assert rec["size"] == (newh, neww) and rec["reverse_channels"] == (fmt == "BGR")
    want_code = {"horizontal": 1, "vertical": 2}[str(G[f"flip{n}"])] if int(G[f"flipped{n}"]) else 0
    assert int(rec["flip"]) == want_code and rec["flip"] in (False, 1, 2)
    for ax, insize, outsize in (("xtab", cw, neww), ("ytab", ch, newh)):
        if insize == outsize:
            assert rec[ax] is None
        else:
            t, ks = packed_table(insize, outsize)
            assert rec[ax][1] == ks and np.array_equal(np.asarray(rec[ax][0]), t)
    assert (out["height"], out["width"]) == G[f"img{n}"].shape[:2]
    assert torch.equal(out["instances"].gt_boxes.tensor, host["instances"].gt_boxes.tensor)
    assert torch.equal(out["instances"].gt_classes, host["instances"].gt_classes) and out["instances"].image_size == (newh, neww)
    # aspect_ratio_batches keeps bucketing by the record's target size
    assert list(data.aspect_ratio_batches(iter([out]), 1)) == [[out]]
