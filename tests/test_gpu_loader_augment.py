"""The flip bit set of cddmsl_resize_batch_u8 (bit 0 mirrors columns, bit 1 rows; cddmsl_amd/csrc/loader_resize.hip) and the
INPUT.CROP / MIN_SIZE_TRAIN_SAMPLING "range" / RANDOM_FLIP "vertical" options through DeviceBatches with DATALOADER.DEVICE_RESIZE on
the GPU.  As in tests/test_gpu_loader_resize.py the kernel tests compare with the numpy restatement of tests/pil_resize_ref.py plus
numpy slicing (tests/loader_augment_cases.py), the loader tests compare the switch on against off; every comparison is exact equality
of bytes, destinations are pre-filled with 0xA5 and every byte outside the items' extents must keep it."""
import os
import sys

import numpy as np
import pytest
import torch

import loader_augment_cases as A
import loader_resize_cases as C
from test_gpu_loader_resize import _launch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def test_all_shapes_every_code():
    """every shape class of loader_resize_cases (several ragged tiles per axis, the recompute path, identity, ...) plus the row-mirror
    edges (newh 1, newh TH + 1, an identity-size copy), each with each of the codes 0..3: item i carries (i + rot) % 4"""
    assert [s[1][0] for s in A.ROW_EDGES[:2]] == [1, 17] and A.ROW_EDGES[2][0] == A.ROW_EDGES[2][1]
    seen = set()
    for rot in range(4):
        cases = A.all_shapes_cases(rot)
        b = A.build(cases)
        seen |= {(n, it[6]) for n, it in enumerate(b["items"])}
        assert all(it[8] < 0 and it[10] < 0 for it, c in zip(b["items"], cases) if c[0].shape[:2] == c[1])     # identity: no tables
        rc, dst = _launch(b)
        assert rc == 0, rot
        C.check(dst, b["want"])
    assert seen == {(n, code) for n in range(len(A.ALL_SHAPES)) for code in range(4)}


def test_store_edges_every_code():
    """output widths 1, 2, 3, 5, 63, 64, 65, 67 with the results shifted by 0..3 bytes inside their slots (row starts on every residue
    modulo 4), every shift with every code: the mirrored row's own address decides the aligned-group / byte-edge split"""
    for srot in range(4):
        for rot in range(4):
            cases = A.store_edge_cases(rot)
            b = A.build(cases, [(i + srot) % 4 for i in range(len(cases))])
            starts = {(off + r * v.shape[2]) % 4 for off, v in b["want"] for r in range(v.shape[0] * v.shape[1])}
            assert starts == {0, 1, 2, 3}
            rc, dst = _launch(b)
            assert rc == 0, (srot, rot)
            C.check(dst, b["want"])


def test_codes_0_and_1_keep_their_bytes():
    """what the library wrote for flip 0 / 1 before the bit set: loader_resize_cases' own expectation, untouched"""
    b = C.build(C.all_shapes_cases())
    assert {it[6] for it in b["items"]} == {0, 1}
    rc, dst = _launch(b)
    assert rc == 0
    C.check(dst, b["want"])


def test_flip_code_out_of_range_is_refused():
    """codes 4 and -1: CDDMSL_ERR_ARG, nothing launched, the destination untouched (also when only the LAST item is wrong)"""
    b = A.build(A.all_shapes_cases(0)[:4])
    for code in (4, -1):
        for n in (0, 3):
            items = list(b["items"])
            items[n] = items[n][:6] + (code,) + items[n][7:]
            rc, dst = _launch(b, items=items)
            assert rc == 1, (code, n)
            assert (dst == C.SENTINEL).all(), (code, n)
    from cddmsl_amd import hip
    dst = torch.full((b["dst_bytes"],), C.SENTINEL, dtype=torch.uint8, device=DEV)
    with pytest.raises(Exception):
        hip.resize_batch_u8(torch.from_numpy(b["src"]).to(DEV), dst, torch.from_numpy(b["tab"]).to(DEV), items)
    assert (dst.cpu().numpy() == C.SENTINEL).all()


# ---------------------------------------------------------------------------------------------------------------- loader
@pytest.fixture(scope="module")
def voc(tmp_path_factory):
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from test_data_pipeline import _make_voc
    return _make_voc(str(tmp_path_factory.mktemp("voc_aug")), n=9)


def _cfg(fmt, on):
    from cddmsl_amd.config import get_cfg
    cfg = get_cfg()
    cfg.merge_from_list(["INPUT.MIN_SIZE_TRAIN", (96, 160), "INPUT.MIN_SIZE_TRAIN_SAMPLING", "range", "INPUT.MAX_SIZE_TRAIN", 224,
                         "INPUT.RANDOM_FLIP", "vertical", "INPUT.CROP.ENABLED", True, "INPUT.CROP.TYPE", "relative_range",
                         "INPUT.CROP.SIZE", [0.6, 0.7], "INPUT.FORMAT", fmt, "SEED", 5, "DATALOADER.DEVICE_RESIZE", on])
    return cfg


@pytest.mark.parametrize("workers,fmt", [(0, "RGB"), (0, "BGR"), (2, "RGB"), (2, "BGR")])
def test_train_loader_on_equals_off(voc, workers, fmt, monkeypatch):
    """six batches of four under crop + size range + vertical flip: the switch on against the host path (this box's Pillow), field
    for field; the kernel's descriptors (seen at the wrapper) show that the comparison met a flipped sample, an unflipped one and a
    crop smaller than its image on both axes"""
    from cddmsl_amd import data, hip
    dicts = data.load_voc_instances(voc, "trainval", dt_data="clipart")
    launches = []
    real = hip.resize_batch_u8
    monkeypatch.setattr(hip, "resize_batch_u8", lambda *a: (launches.append([tuple(it) for it in a[3]]), real(*a))[1])
    off = data.build_detection_train_loader(_cfg(fmt, False), dicts, 4, 0, 1, DEV, num_workers=workers)
    on = data.build_detection_train_loader(_cfg(fmt, True), dicts, 4, 0, 1, DEV, num_workers=workers)
    seen = []                                     # (flip code, cropped (h, w), image (h, w)) per compared sample
    try:
        for n in range(6):
            ba, bb = next(off), next(on)
            assert len(ba) == len(bb) == 4 and len(launches) > n and len(launches[n]) == 8        # image + twin per sample, one launch
            for i, (x, y) in enumerate(zip(ba, bb)):
                assert set(x) == set(y) and data.DEVICE_RESIZE_KEY not in y
                for k in ("image", "image_trgt"):
                    assert y[k].is_cuda and y[k].dtype == torch.uint8 and y[k].shape == x[k].shape
                    assert torch.equal(x[k].cpu(), y[k].cpu()), (n, i, k)
                assert x["image_id"] == y["image_id"] and (x["height"], x["width"]) == (y["height"], y["width"])
                assert x["instances"].image_size == y["instances"].image_size == tuple(y["image"].shape[1:])
                assert torch.equal(x["instances"].gt_boxes.tensor.cpu(), y["instances"].gt_boxes.tensor.cpu())
                assert torch.equal(x["instances"].gt_classes.cpu(), y["instances"].gt_classes.cpu())
                it, tw = launches[n][2 * i], launches[n][2 * i + 1]
                assert it[2:8] == tw[2:8] and it[4:6] == tuple(y["image"].shape[1:]) and it[7] == int(fmt == "BGR")
                seen.append((it[6], it[2:4], (y["height"], y["width"])))
    finally:
        off.close(), on.close()
    # not vacuous: (SEED 5 gives all three for both worker counts; the draws do not depend on the device)
    assert {s[0] for s in seen} == {0, 2}
    assert all(c[0] <= im[0] and c[1] <= im[1] for _, c, im in seen) and any(c[0] < im[0] and c[1] < im[1] for _, c, im in seen)
    assert len({s[1] for s in seen}) > 4                                                           # the windows differ from sample to sample
