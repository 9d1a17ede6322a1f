"""cddmsl_color_jitter_batch_u8 (cddmsl_amd/csrc/color_jitter.hip), hip.color_jitter_batch_u8 and INPUT.COLOR_JITTER through
DeviceBatches on the GPU.  The kernel tests compare with ``augment.color_jitter_u8`` (the host path; tests/test_color_jitter_host.py
holds it to a float64 model and its parameters to the reference), the loader tests compare DATALOADER.DEVICE_RESIZE on against off.
Every comparison is exact equality of bytes.  Buffers are pre-filled with 0xA5 and every byte outside the images must keep it."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from cddmsl_amd import augment

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = 0xA5
WEIGHTS = [1.0, 0.0, 2.5, 0.37, 1.3]
LIGHTS = [[-30.25, -3.5, -200.0], [12.3, -0.4, 7.75]]
ALL4 = [{"brightness": 1.3, "contrast": 0.7, "saturation": 1.4, "lighting": [3.5, -2.25, 9.0]},
        {"brightness": 0.61, "contrast": 1.45, "saturation": 0.2, "lighting": [-13.0, 40.5, 0.125]}]


def _param_sets():
    sets = [{name: w} for name in ("brightness", "contrast", "saturation") for w in WEIGHTS]
    return sets + [{"lighting": v} for v in LIGHTS] + ALL4 + [None, {}]


def _image(h, w, seed):
    img = np.random.RandomState(seed).randint(0, 256, (h, w, 3), dtype=np.uint8)
    img[0, 0] = (255, 0, 3)
    return img


def _layout(images, gaps):
    """CHW images behind one another with ``gaps[i]`` sentinel bytes in front of image i (and gaps[-1] behind the last) -> (buffer, offsets)"""
    assert len(gaps) == len(images) + 1
    parts, offs, pos = [], [], 0
    for img, g in zip(images, gaps):
        parts.append(np.full(g, SENTINEL, np.uint8))
        pos += g
        offs.append(pos)
        parts.append(np.ascontiguousarray(img.transpose(2, 0, 1)).reshape(-1))
        pos += img.size
    parts.append(np.full(gaps[-1], SENTINEL, np.uint8))
    return np.concatenate(parts), offs


def _run_and_check(images, params, bgr, gaps):
    """one wrapper call over the laid-out batch; the whole buffer against the host path, sentinels included -> (bytes, sums)"""
    from cddmsl_amd import hip
    src, offs = _layout(images, gaps)
    want, _ = _layout([augment.color_jitter_u8(im, p, bgr) for im, p in zip(images, params)], gaps)
    buf = torch.from_numpy(src).to(DEV)
    sums = hip.color_jitter_batch_u8(buf, [(o, im.shape[0], im.shape[1], p, bgr) for o, im, p in zip(offs, images, params)])
    got = buf.cpu().numpy()
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{bad.size} bytes differ, first at {bad[:5]} (offsets {offs})"
    return got, sums


@pytest.mark.parametrize("bgr", [False, True])
@pytest.mark.parametrize("shape", [(1, 1), (1, 7), (3, 5), (17, 33), (64, 64)])
def test_kernel_equals_host_path(shape, bgr):
    """each operation alone over the weight set (identity, zero, clipping), negative and positive lighting, all four together, and
    descriptors without an operation, one item each in ONE batch; gaps of 1..23 bytes put the images on every alignment"""
    sets = _param_sets()
    images = [_image(*shape, seed=i) for i in range(len(sets))]
    gaps = [1 + (7 * i) % 23 for i in range(len(sets) + 1)]
    got, sums = _run_and_check(images, sets, bgr, gaps)
    sums = sums.cpu().numpy()
    for i, (im, p) in enumerate(zip(images, sets)):
        if p and "contrast" in p:
            b = augment.color_jitter_u8(im, {"brightness": p["brightness"]}, bgr) if "brightness" in p else im
            assert sums[i] == int(b.sum(dtype=np.int64))
        else:
            assert sums[i] == 0


def test_mixed_sizes_with_twins_at_odd_offsets():
    """three sizes -- 16-byte, 4-byte and byte-wide apply paths, several chunks each pass -- image and twin each, at offsets that are no
    multiples of 4 or 16; more than 32 items, so a second launch pair"""
    shapes = [(80, 120), (50, 66), (37, 29)]
    images, params = [], []
    for rep in range(6):
        for n, (h, w) in enumerate(shapes):
            p = ALL4[(rep + n) % 2] if rep % 3 else {("brightness", "contrast", "saturation")[n]: 0.45 + 0.3 * rep}
            images += [_image(h, w, 10 * rep + n), 255 - _image(h, w, 10 * rep + n)]
            params += [p, dict(p, contrast=1.2) if rep % 2 else p]
    assert len(images) == 36
    gaps = [(5, 3, 9, 1, 7, 2, 11, 6, 13)[i % 9] for i in range(len(images) + 1)]
    src, offs = _layout(images, gaps)
    assert sum(o % 4 != 0 for o in offs) >= 20 and sum(o % 16 != 0 for o in offs) >= 30
    for bgr in (False, True):
        _run_and_check(images, params, bgr, gaps)


def test_no_active_operation_launches_nothing_and_touches_nothing():
    from cddmsl_amd import hip
    images = [_image(9, 13, 1), _image(4, 4, 2)]
    src, offs = _layout(images, [3, 5, 2])
    buf = torch.from_numpy(src).to(DEV)
    assert hip.color_jitter_batch_u8(buf, [(offs[0], 9, 13, None, True), (offs[1], 4, 4, {}, False)]) is None
    assert hip.color_jitter_batch_u8(buf, []) is None
    assert np.array_equal(buf.cpu().numpy(), src)


def test_large_sum_is_exact_and_calls_repeat():
    """512 x 512 of all 255: the sum 200 540 160 is beyond 2^24, where a float32 accumulation stops counting by ones -- any other mean
    than 255 shows in the bytes (0.5 * 254.99 + 127.5 truncates to 254).  Then a random image twice: the same bytes."""
    from cddmsl_amd import hip
    white = np.full((512, 512, 3), 255, np.uint8)
    got, sums = _run_and_check([white], [{"contrast": 0.5}], False, [16, 16])
    assert int(sums[0]) == 200540160 == 3 * 512 * 512 * 255
    assert (got[16:-16] == 255).all()
    img = _image(512, 512, 3)
    src, offs = _layout([img], [7, 9])
    items = [(offs[0], 512, 512, ALL4[0], True)]
    a, b = torch.from_numpy(src).to(DEV), torch.from_numpy(src).to(DEV)
    sa, sb = hip.color_jitter_batch_u8(a, items), hip.color_jitter_batch_u8(b, items)
    assert torch.equal(a, b) and torch.equal(sa, sb)
    want, _ = _layout([augment.color_jitter_u8(img, ALL4[0], True)], [7, 9])
    assert np.array_equal(a.cpu().numpy(), want)


def test_bad_descriptors_are_refused_before_any_launch():
    from cddmsl_amd import hip
    from cddmsl_amd._lib import lib_color_jitter
    img = _image(6, 10, 4)
    src, offs = _layout([img, img], [4, 4, 4])
    good = [augment.descriptor(offs[0], 6, 10, ALL4[0], True), augment.descriptor(offs[1], 6, 10, {"brightness": 0.5}, False)]
    nan = int(np.float32("nan").view(np.int32))

    def call(items, count=None, nbytes=None, with_sums=True, null_buf=False):
        buf = torch.from_numpy(src).to(DEV)
        sums = torch.full((len(items) + 1,), -1, dtype=torch.int64, device=DEV)
        arr = (hip.JitterItem * max(len(items), 1))(*[hip.JitterItem(*it) for it in items])
        rc = lib_color_jitter().cddmsl_color_jitter_batch_u8(None if null_buf else buf.data_ptr(), buf.numel() if nbytes is None else nbytes,
                                                             ctypes.cast(arr, ctypes.c_void_p), len(items) if count is None else count,
                                                             sums.data_ptr() if with_sums else None, hip.stream_ptr())
        return rc, buf.cpu().numpy(), sums.cpu().numpy()

    def edit(i, **kw):
        names = [f[0] for f in hip.JitterItem._fields_]
        it = list(good[i])
        for k, v in kw.items():
            it[names.index(k)] = v
        return [tuple(it) if j == i else g for j, g in enumerate(good)]

    bad = {"offset past the buffer": dict(items=edit(1, off=len(src) - 179)), "negative offset": dict(items=edit(0, off=-1)),
           "short buffer": dict(items=good, nbytes=offs[1] + 179), "zero height": dict(items=edit(1, h=0)),
           "negative width": dict(items=edit(0, w=-3)), "huge size": dict(items=edit(1, h=2 ** 30, w=2 ** 30)),
           "unknown operation bit": dict(items=edit(1, ops=16)), "negative operation set": dict(items=edit(1, ops=-1)),
           "NaN weight": dict(items=edit(1, b_dw=nan)), "NaN lighting": dict(items=edit(0, light_g=nan)),
           "contrast without sums": dict(items=good, with_sums=False), "negative count": dict(items=good, count=-1),
           "null buffer": dict(items=good, null_buf=True)}
    for what, kw in bad.items():
        rc, buf, sums = call(**kw)
        assert rc == 1, what
        assert np.array_equal(buf, src) and (sums == -1).all(), what
    rc, buf, sums = call(good, count=0)
    assert rc == 0 and np.array_equal(buf, src)
    rc, buf, sums = call(good)                                # (the unedited batch is fine)
    want, _ = _layout([augment.color_jitter_u8(img, ALL4[0], True), augment.color_jitter_u8(img, {"brightness": 0.5}, False)], [4, 4, 4])
    assert rc == 0 and np.array_equal(buf, want) and sums[1] == 0 and sums[0] > 0 and sums[2] == -1


# ---------------------------------------------------------------------------------------------------------------- loaders
@pytest.fixture(scope="module")
def voc(tmp_path_factory):
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from test_data_pipeline import _make_voc
    return _make_voc(str(tmp_path_factory.mktemp("voc")), n=4)     # four JPEG pairs of two sizes (80 x 130, 120 x 90)


def _cfg(fmt, on, twin="same", prob=1.0):
    from cddmsl_amd.config import get_cfg
    cfg = get_cfg()
    cfg.merge_from_list(["INPUT.MIN_SIZE_TRAIN", (96, 112, 128, 150), "INPUT.MAX_SIZE_TRAIN", 224, "INPUT.FORMAT", fmt, "SEED", 5,
                         "DATALOADER.DEVICE_RESIZE", on, "INPUT.COLOR_JITTER.ENABLED", True, "INPUT.COLOR_JITTER.PROB", prob,
                         "INPUT.COLOR_JITTER.BRIGHTNESS", (0.6, 1.4), "INPUT.COLOR_JITTER.CONTRAST", (0.5, 1.5),
                         "INPUT.COLOR_JITTER.SATURATION", (0.4, 1.6), "INPUT.COLOR_JITTER.LIGHTING", 25.0, "INPUT.COLOR_JITTER.TWIN", twin])
    return cfg


@pytest.mark.parametrize("fmt,twin,prob", [("BGR", "same", 1.0), ("RGB", "independent", 0.7), ("BGR", "none", 1.0)])
def test_train_loader_device_path_equals_host_path(voc, fmt, twin, prob):
    """six batches of two with jitter on and a seeded mapper: DATALOADER.DEVICE_RESIZE on against off, byte for byte"""
    from cddmsl_amd import data
    dicts = data.load_voc_instances(voc, "trainval", dt_data="clipart")
    off = data.build_detection_train_loader(_cfg(fmt, False, twin, prob), dicts, 2, 0, 1, DEV, num_workers=0)
    on = data.build_detection_train_loader(_cfg(fmt, True, twin, prob), dicts, 2, 0, 1, DEV, num_workers=0)
    plain_cfg = _cfg(fmt, False, twin, 1.0)
    plain_cfg.merge_from_list(["INPUT.COLOR_JITTER.ENABLED", False])
    with_j, without = (data.DatasetMapper(c, True, np.random.RandomState(5))(dicts[0]) for c in (_cfg(fmt, False, twin, 1.0), plain_cfg))
    assert with_j["image"].shape == without["image"].shape and not torch.equal(with_j["image"], without["image"])   # (the block is in force)
    assert torch.equal(with_j["image_trgt"], without["image_trgt"]) == (twin == "none")
    try:
        for _ in range(6):
            ba, bb = next(off), next(on)
            assert len(ba) == len(bb) == 2
            for x, y in zip(ba, bb):
                assert x["image_id"] == y["image_id"] and data.DEVICE_RESIZE_KEY not in y
                for k in ("image", "image_trgt"):
                    assert y[k].is_cuda and y[k].dtype == torch.uint8 and y[k].shape == x[k].shape
                    assert torch.equal(x[k].cpu(), y[k].cpu()), k
                assert torch.equal(x["instances"].gt_boxes.tensor.cpu(), y["instances"].gt_boxes.tensor.cpu())
    finally:
        off.close(), on.close()


def test_batch_without_a_draw_launches_nothing(voc, monkeypatch):
    """PROB 0: no sample draws an operation, so the staging thread makes the resize launch alone; PROB 1: one jitter call per batch"""
    from cddmsl_amd import data, hip
    dicts = data.load_voc_instances(voc, "trainval", dt_data="clipart")
    calls = []
    real = hip.color_jitter_batch_u8
    monkeypatch.setattr(hip, "color_jitter_batch_u8", lambda buf, items: (calls.append(len(items)), real(buf, items))[1])
    for prob, want in ((0.0, []), (1.0, [4])):
        del calls[:]
        m = data.DatasetMapper(_cfg("BGR", True, "same", prob), True, np.random.RandomState(3))
        got = list(data.DeviceBatches(iter([[m(d) for d in dicts[1:3]]]), DEV))
        assert calls == want and len(got) == 1 and got[0][0]["image"].is_cuda
