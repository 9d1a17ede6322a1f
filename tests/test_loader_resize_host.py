"""CPU: DATALOADER.DEVICE_RESIZE on the host side -- the mapper with the switch on makes the same draws, boxes, sizes and buckets as
with it off and leaves the decoded image plus a record; the restated Pillow resize (tests/pil_resize_ref.py) of that image, mirrored /
reversed / transposed as the record says, is byte for byte what the host path produces; the record's tables are Pillow's; the table
code loads no library; the default is off; a CPU loader behind the switch is refused.  Exact equality everywhere."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import loader_resize_cases as C  # noqa: E402
import pil_resize_ref as PR  # noqa: E402
from cddmsl_amd import data  # noqa: E402
from cddmsl_amd.config import get_cfg  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cfg(fmt, on):
    cfg = get_cfg()
    cfg.merge_from_list(["INPUT.MIN_SIZE_TRAIN", (224, 256, 288, 320), "INPUT.MAX_SIZE_TRAIN", 448, "INPUT.FORMAT", fmt, "SEED", 7,
                         "DATALOADER.DEVICE_RESIZE", on])
    return cfg


@pytest.fixture(scope="module")
def dicts(tmp_path_factory):
    from test_data_pipeline import _make_voc
    base = _make_voc(str(tmp_path_factory.mktemp("voc")), n=7)
    return data.load_voc_instances(base, "trainval", dt_data="clipart")


@pytest.mark.parametrize("fmt", ["RGB", "BGR"])
def test_mapper_on_equals_mapper_off(dicts, fmt):
    off = data.DatasetMapper(_cfg(fmt, False), True, np.random.RandomState(11))
    on = data.DatasetMapper(_cfg(fmt, True), True, np.random.RandomState(11))
    seen = set()
    a_all, b_all = [], []
    for n in range(14):
        d = dicts[n % len(dicts)]
        a, b = off(d), on(d)
        a_all.append(a), b_all.append(b)
        rec = b[data.DEVICE_RESIZE_KEY]
        assert data.DEVICE_RESIZE_KEY not in a
        newh, neww = rec["size"]
        assert tuple(a["image"].shape) == (3, newh, neww)                                       # the same size draw
        assert rec["reverse_channels"] == (fmt == "BGR")
        for k in ("image", "image_trgt"):
            raw = b[k].numpy()
            assert raw.dtype == np.uint8 and raw.shape == (d["height"], d["width"], 3)          # decoded, nothing else done
            assert np.array_equal(raw, data.read_image(d["file_name" if k == "image" else "data_dt_file_name"], "RGB"))
            assert np.array_equal(C.expected(raw, newh, neww, rec["flip"], rec["reverse_channels"]), a[k].numpy()), (n, k)
        ia, ib = a["instances"], b["instances"]
        assert ia.image_size == ib.image_size == (newh, neww)
        assert torch.equal(ia.gt_boxes.tensor, ib.gt_boxes.tensor) and torch.equal(ia.gt_classes, ib.gt_classes)
        assert all(a[k] == b[k] for k in ("height", "width", "image_id", "file_name"))
        # the flip draw, read off the host path's pixels: the restated resize without / with the mirror
        plain = C.expected(b["image"].numpy(), newh, neww, False, rec["reverse_channels"])
        assert np.array_equal(a["image"].numpy(), plain[:, :, ::-1] if rec["flip"] else plain)
        seen.add((newh, neww, rec["flip"]))
        # the tables are Pillow's, for exactly the axes that change
        for ax, insize, outsize in (("xtab", d["width"], neww), ("ytab", d["height"], newh)):
            if insize == outsize:
                assert rec[ax] is None
                continue
            lo, cnt, k, ks = PR.coeffs(insize, outsize)
            flat, got_ks = rec[ax]
            assert got_ks == ks and flat.dtype == np.int32
            assert np.array_equal(flat, np.concatenate([np.asarray(lo), np.asarray(cnt), np.asarray(k).reshape(-1)]))
    assert {f for _, _, f in seen} == {False, True} and len({s[:2] for s in seen}) >= 3
    # the bucket choice: the same batches, sample for sample
    ba = [[x["image_id"] for x in bt] for bt in data.aspect_ratio_batches(iter(a_all), 2)]
    bb = [[x["image_id"] for x in bt] for bt in data.aspect_ratio_batches(iter(b_all), 2)]
    assert ba == bb and len(ba) >= 4 and sorted(len(x) for x in ba) == [2] * len(ba)


def test_test_mapper_on_equals_off(dicts):
    cfg_off, cfg_on = _cfg("BGR", False), _cfg("BGR", True)
    for c in (cfg_off, cfg_on):
        c.merge_from_list(["INPUT.MIN_SIZE_TEST", 160, "INPUT.MAX_SIZE_TEST", 224])
    a, b = data.DatasetMapper(cfg_off, False)(dicts[0]), data.DatasetMapper(cfg_on, False)(dicts[0])
    rec = b[data.DEVICE_RESIZE_KEY]
    assert rec["flip"] is False and "instances" not in b and rec["size"] == tuple(a["image"].shape[1:])
    assert np.array_equal(C.expected(b["image"].numpy(), *rec["size"], False, True), a["image"].numpy())


def test_default_is_off_and_emits_no_record(dicts):
    cfg = get_cfg()
    assert cfg.DATALOADER.DEVICE_RESIZE is False
    cfg.merge_from_list(["INPUT.MIN_SIZE_TRAIN", (64,), "INPUT.MAX_SIZE_TRAIN", 128])
    out = data.DatasetMapper(cfg, True, np.random.RandomState(0))(dicts[0])
    assert data.DEVICE_RESIZE_KEY not in out and out["image"].shape[0] == 3


def test_table_code_loads_no_library():
    """what a loader worker imports to build the tables: neither the HIP library nor the GPU runtime gets loaded by it"""
    code = ("import sys; sys.path.insert(0, %r)\n"
            "import cddmsl_amd.resample as r\n"
            "t, ks = r.packed_table(375, 800)\n"
            "assert ks == 3 and len(t) == 800 * 5\n"
            "assert 'torch' not in sys.modules and 'cddmsl_amd._lib' not in sys.modules\n"
            "maps = open('/proc/self/maps').read()\n"
            "assert 'libcddmsl_hip' not in maps and 'libamdhip64' not in maps\n"
            "from cddmsl_amd import hip\n"
            "assert hip._resample_table is r.resample_table\n"
            "import cddmsl_amd._lib as L\n"
            "assert L._lib is None\n" % ROOT)
    subprocess.check_call([sys.executable, "-c", code])


def test_cpu_loader_behind_the_switch_is_refused(dicts):
    cfg = _cfg("RGB", True)
    with pytest.raises(ValueError):
        data.build_detection_train_loader(cfg, dicts, per_rank_batch=2, device="cpu", num_workers=0)
    with pytest.raises(ValueError):
        data.build_detection_test_loader(cfg, dicts, batch_size=1, device="cpu")
    next(data.build_detection_train_loader(_cfg("RGB", False), dicts, per_rank_batch=2, device="cpu", num_workers=0))   # off: as before
