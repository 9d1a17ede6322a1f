"""cddmsl_resize_batch_u8 (cddmsl_amd/csrc/loader_resize.hip), hip.resize_batch_u8 and DATALOADER.DEVICE_RESIZE through
DeviceBatches on the GPU.  The kernel tests compare with the numpy restatement of tests/pil_resize_ref.py (tied to Pillow bit for bit
by tests/test_tta_host.py), so they do not depend on the Pillow of the GPU box; the loader tests compare the switch on against off,
i.e. against this box's own Pillow through the existing host path.  Integer arithmetic: every comparison is exact equality of bytes.
Destinations are pre-filled with 0xA5 and every byte outside the items' extents must keep it."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

import loader_resize_cases as C

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _launch(b, items=None, count=None, src_bytes=None, dst_bytes=None, tab_len=None, tab_none=False):
    """one raw C call on a sentinel-filled destination -> (status, destination bytes as numpy)"""
    from cddmsl_amd import hip
    src, tab = torch.from_numpy(b["src"]).to(DEV), torch.from_numpy(b["tab"]).to(DEV)
    dst = torch.full((b["dst_bytes"],), C.SENTINEL, dtype=torch.uint8, device=DEV)
    items = b["items"] if items is None else items
    arr = (hip.ResizeItem * max(len(items), 1))(*[hip.ResizeItem(*it) for it in items])
    rc = hip._L().cddmsl_resize_batch_u8(src.data_ptr(), src.numel() if src_bytes is None else src_bytes, dst.data_ptr(),
                                         dst.numel() if dst_bytes is None else dst_bytes, None if tab_none or not tab.numel() else tab.data_ptr(),
                                         tab.numel() if tab_len is None else tab_len, ctypes.cast(arr, ctypes.c_void_p),
                                         len(items) if count is None else count, hip.stream_ptr())
    torch.cuda.synchronize()
    return rc, dst.cpu().numpy()


def test_one_launch_all_shapes():
    """every shape class, flip alternating, reverse_channels on every third, a pair sharing one table set, in ONE launch; then the same
    items as single-item batches"""
    b = C.build(C.all_shapes_cases())
    assert len(b["items"]) == len(C.ALL_SHAPES) + 1 and b["items"][0][8:] == b["items"][-1][8:] and b["items"][0][8] >= 0
    rc, dst = _launch(b)
    assert rc == 0
    C.check(dst, b["want"])
    for it, w in zip(b["items"], b["want"]):
        rc, one = _launch(b, items=[it])
        assert rc == 0
        C.check(one, [w])
    # the Python wrapper, and more items than one launch takes (two chunks of the descriptor block)
    from cddmsl_amd import hip
    b = C.build((C.all_shapes_cases() * 3)[:36])
    dst = torch.full((b["dst_bytes"],), C.SENTINEL, dtype=torch.uint8, device=DEV)
    hip.resize_batch_u8(torch.from_numpy(b["src"]).to(DEV), dst, torch.from_numpy(b["tab"]).to(DEV), b["items"])
    C.check(dst.cpu().numpy(), b["want"])


def test_store_edges():
    """output widths 1, 2, 3, 5, 63, 64, 65, 67 with results shifted by 0..3 bytes inside their slots: row starts on every residue
    modulo 4, spans shorter than one aligned group, and the 4-byte middle with byte edges on either side"""
    cases = C.store_edge_cases()
    assert sorted(c[1][1] for c in cases) == [1, 2, 3, 5, 63, 64, 65, 67]
    for rot in range(4):
        b = C.build(cases, [(i + rot) % 4 for i in range(len(cases))])
        starts = {(off + r * v.shape[2]) % 4 for off, v in b["want"] for r in range(v.shape[0] * v.shape[1])}
        assert starts == {0, 1, 2, 3}
        rc, dst = _launch(b)
        assert rc == 0
        C.check(dst, b["want"])


def test_refusals():
    """CDDMSL_ERR_ARG and an untouched destination for: a source / destination extent outside its buffer, a changed axis without a
    table, a table on an unchanged axis, a table range outside the table buffer, a non-positive size; count == 0 succeeds"""
    b = C.build(C.all_shapes_cases()[:4])         # item 2 is the identity (no tables), the others change both axes
    it = b["items"]

    def edit(n, **kw):
        names = ("src_off", "dst_off", "h", "w", "newh", "neww", "flip", "reverse_channels", "xtab", "xks", "ytab", "yks")
        t = dict(zip(names, it[n]))
        t.update(kw)
        return it[:n] + [tuple(t[k] for k in names)] + it[n + 1:]

    last_src = it[3][0] + 3 * it[3][2] * it[3][3]
    last_dst = it[3][1] + 3 * it[3][4] * it[3][5]
    xlen = it[3][5] * (2 + it[3][9])
    bad = {"source extent past the buffer": dict(src_bytes=last_src - 1),
           "source offset past the buffer": dict(items=edit(1, src_off=len(b["src"]))),
           "negative source offset": dict(items=edit(1, src_off=-256)),
           "destination extent past the buffer": dict(dst_bytes=last_dst - 1),
           "negative destination offset": dict(items=edit(0, dst_off=-1)),
           "changed x axis without a table": dict(items=edit(0, xtab=-1)),
           "changed y axis without a table": dict(items=edit(1, ytab=-1)),
           "table on an unchanged axis": dict(items=edit(2, xtab=0, xks=3)),
           "tables without a table buffer": dict(tab_none=True),
           "x table range past the table buffer": dict(items=edit(3, xtab=len(b["tab"]) - xlen + 1)),
           "y table past a short table buffer": dict(tab_len=len(b["tab"]) - 1),
           "non-positive ksize": dict(items=edit(0, xks=0)),
           "zero height": dict(items=edit(1, h=0)),
           "negative width": dict(items=edit(1, w=-5)),
           "zero output height": dict(items=edit(3, newh=0)),
           "negative output width": dict(items=edit(3, neww=-1)),
           "negative count": dict(count=-1)}
    for what, kw in bad.items():
        rc, dst = _launch(b, **kw)
        assert rc == 1, what
        assert (dst == C.SENTINEL).all(), what
    rc, dst = _launch(b, count=0)
    assert rc == 0 and (dst == C.SENTINEL).all()
    rc, dst = _launch(b)                          # (the unedited batch is fine)
    assert rc == 0
    C.check(dst, b["want"])


# ---------------------------------------------------------------------------------------------------------------- loaders
@pytest.fixture(scope="module")
def voc(tmp_path_factory):
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from test_data_pipeline import _make_voc
    return _make_voc(str(tmp_path_factory.mktemp("voc")), n=9)


def _cfg(fmt, on):
    from cddmsl_amd.config import get_cfg
    cfg = get_cfg()
    cfg.merge_from_list(["INPUT.MIN_SIZE_TRAIN", (224, 256, 288, 320), "INPUT.MAX_SIZE_TRAIN", 448, "INPUT.MIN_SIZE_TEST", 160,
                         "INPUT.MAX_SIZE_TEST", 224, "INPUT.FORMAT", fmt, "SEED", 5, "DATALOADER.DEVICE_RESIZE", on])
    return cfg


def _same_batches(a, b, n):
    from cddmsl_amd import data
    for _ in range(n):
        ba, bb = next(a), next(b)
        assert len(ba) == len(bb)
        for x, y in zip(ba, bb):
            assert set(x) == set(y) and data.DEVICE_RESIZE_KEY not in y
            for k in ("image", "image_trgt"):
                if k in x or k in y:
                    assert y[k].is_cuda and y[k].dtype == torch.uint8 and y[k].shape == x[k].shape
                    assert torch.equal(x[k].cpu(), y[k].cpu()), k
            assert x["image_id"] == y["image_id"] and (x["height"], x["width"]) == (y["height"], y["width"])
            if "instances" in x:
                assert x["instances"].image_size == y["instances"].image_size == tuple(y["image"].shape[1:])
                assert torch.equal(x["instances"].gt_boxes.tensor.cpu(), y["instances"].gt_boxes.tensor.cpu())
                assert torch.equal(x["instances"].gt_classes.cpu(), y["instances"].gt_classes.cpu())


@pytest.mark.parametrize("workers,fmt", [(0, "RGB"), (0, "BGR"), (2, "RGB"), (2, "BGR")])
def test_train_loader_on_equals_off(voc, workers, fmt):
    """six batches of four, multi-scale + flip: the switch on against the host path (this box's Pillow), field for field"""
    from cddmsl_amd import data
    dicts = data.load_voc_instances(voc, "trainval", dt_data="clipart")
    off = data.build_detection_train_loader(_cfg(fmt, False), dicts, 4, 0, 1, DEV, num_workers=workers)
    on = data.build_detection_train_loader(_cfg(fmt, True), dicts, 4, 0, 1, DEV, num_workers=workers)
    try:
        _same_batches(off, on, 6)
    finally:
        off.close(), on.close()


@pytest.mark.parametrize("fmt", ["RGB", "BGR"])
def test_test_loader_on_equals_off(voc, fmt):
    from cddmsl_amd import data
    dicts = data.load_voc_instances(voc, "test")
    off = data.build_detection_test_loader(_cfg(fmt, False), dicts, batch_size=2, device=DEV)
    on = data.build_detection_test_loader(_cfg(fmt, True), dicts, batch_size=2, device=DEV)
    a, b = list(off), list(on)
    assert len(a) == len(b) == 5
    _same_batches(iter(a), iter(b), 5)


def test_mixed_batch_and_one_copy(voc, monkeypatch):
    """a batch that mixes samples with and without a record goes through ONE host-to-device copy and one kernel call"""
    from cddmsl_amd import data, hip
    dicts = data.load_voc_instances(voc, "trainval", dt_data="clipart")
    on = data.DatasetMapper(_cfg("BGR", True), True, np.random.RandomState(3))
    off = data.DatasetMapper(_cfg("BGR", False), True, np.random.RandomState(3))
    host_on, host_off = [on(d) for d in dicts[:4]], [off(d) for d in dicts[:4]]
    mixed = [host_on[0], host_off[1], host_on[2], host_off[3]]
    calls = []
    real = hip.resize_batch_u8
    monkeypatch.setattr(hip, "resize_batch_u8", lambda *a: (calls.append(len(a[3])), real(*a))[1])
    copies = []
    real_to = torch.Tensor.to

    def counting_to(self, *a, **k):
        if self.is_pinned():
            copies.append(self.numel())
        return real_to(self, *a, **k)

    monkeypatch.setattr(torch.Tensor, "to", counting_to)
    got = list(data.DeviceBatches(iter([mixed]), DEV))
    monkeypatch.undo()
    assert calls == [4] and len(copies) == 1                  # two samples x (image + twin) in one launch; one pinned upload
    for x, y in zip(host_off, got[0]):
        assert data.DEVICE_RESIZE_KEY not in y
        assert torch.equal(x["image"], y["image"].cpu()) and torch.equal(x["image_trgt"], y["image_trgt"].cpu())
        assert torch.equal(x["instances"].gt_boxes.tensor, y["instances"].gt_boxes.tensor.cpu())


def test_drop_in_entry_point_with_device_resize(tmp_path, capsys):
    """tools/train_caption_consistency.py with the options of test_train_checkpoint_eval_on_mini_voc plus DATALOADER.DEVICE_RESIZE
    True: two iterations, checkpoint, --eval-only from it"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import train_caption_consistency as tool
    from test_data_pipeline import _make_voc
    base = _make_voc(str(tmp_path), n=6)
    out = str(tmp_path / "out")
    common = ["--config-file", os.path.join(ROOT, "configs", "VOC-Experiments", "faster_rcnn_CLIP_R_50_C4.yaml"), "--voc-root", base]
    opts = ["SOLVER.IMS_PER_BATCH", "2", "INPUT.MIN_SIZE_TRAIN", "(160,)", "INPUT.MAX_SIZE_TRAIN", "224", "INPUT.MIN_SIZE_TEST", "160",
            "INPUT.MAX_SIZE_TEST", "224", "SOLVER.CHECKPOINT_PERIOD", "2", "OUTPUT_DIR", out, "DATALOADER.NUM_WORKERS", "0",
            "MODEL.RPN.PRE_NMS_TOPK_TRAIN", "300", "MODEL.RPN.POST_NMS_TOPK_TRAIN", "100", "MODEL.RPN.PRE_NMS_TOPK_TEST", "300",
            "MODEL.RPN.POST_NMS_TOPK_TEST", "50", "MODEL.ROI_HEADS.BATCH_SIZE_PER_IMAGE", "32", "TEST.DETECTIONS_PER_IMAGE", "20",
            "DATALOADER.DEVICE_RESIZE", "True"]
    tool.main(tool.default_argument_parser().parse_args(common + ["--dt-data", "clipart", "--max-iter", "2"] + opts))
    ck = os.path.join(out, "model_final.pth")
    assert os.path.exists(ck)
    with pytest.raises(SystemExit) as e:
        tool.main(tool.default_argument_parser().parse_args(common + ["--eval-only"] + opts + ["MODEL.WEIGHTS", ck]))
    assert e.value.code == 0
    assert "'AP50'" in capsys.readouterr().out
