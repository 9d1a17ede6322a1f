"""cddmsl_tta_view (cddmsl_amd/csrc/tta_views.hip), hip.tta_views and GeneralizedRCNNWithTTA on the GPU, against the numpy
restatement of tests/pil_resize_ref.py (which tests/test_tta_host.py ties to Pillow bit for bit; nothing here depends on the Pillow of
the GPU box except the explicit host-mapper path).  Kernel outputs are compared as RAW BITS with ``hip.preprocess`` of the restated
uint8 view: that covers the padding and the channels 3..Cp; destinations are pre-filled with a NaN bit pattern and the slots the
call does not name must keep it."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

import pil_resize_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLIP_MEAN, CLIP_STD = [0.48145466, 0.4578275, 0.40821073], [0.26862954, 0.26130258, 0.27577711]
STOCK_MEAN, STOCK_STD = [103.530, 116.280, 123.675], [1.0, 1.0, 1.0]
# test 1's shapes; one that spans several workgroup tiles (16 x 64) on both axes at a non-integer ratio; and one whose vertical
# ratio (10) needs more input rows per tile than the kernel stages in LDS, so its tiles take the recompute path
SHAPES = R.PAIRS + [((150, 210), (97, 136)), ((200, 40), (20, 30))]
NAN_BITS = {torch.float32: (torch.int32, 0x7FC00001), torch.bfloat16: (torch.int16, 0x7FC1)}


def _ids(p):
    return "%dx%d_to_%dx%d" % (p[0] + p[1])


@functools.lru_cache(maxsize=None)
def _case(pair):
    """(image uint8 HWC, plain view, mirrored view): computed once per shape, shared and never written"""
    (h, w), (nh, nw) = pair
    img = R.seeded_image(h, w, 1000 * h + w)
    v = R.resize(img, nh, nw)
    out = (img, v, np.ascontiguousarray(v[:, ::-1]))
    for a in out:
        a.setflags(write=False)
    return out


def _chw(a):
    return torch.from_numpy(np.ascontiguousarray(a.transpose(2, 0, 1))).to(DEV)


def _nan_filled(shape, dtype):
    it, bits = NAN_BITS[dtype]
    t = torch.full(shape, bits, dtype=it, device=DEV).view(dtype)
    assert bool(torch.isnan(t).all())
    return t


def _bits(t):
    return t.contiguous().view(NAN_BITS[t.dtype][0])


def _untouched(t):
    return bool((_bits(t) == NAN_BITS[t.dtype][1]).all())


def _tables(insize, outsize):
    """the restatement's tables as device int32 arrays (lo, n, k [out][ksize]) and ksize; no tables for an unchanged axis"""
    if insize == outsize:
        return None, None, None, 0
    xmin, ns, kk, ks = R.coeffs(insize, outsize)
    dev = lambda a: torch.tensor(np.asarray(a, dtype=np.int32)).to(DEV)
    return dev(xmin), dev(ns), dev(np.asarray(kk, np.int32).reshape(-1)), ks


def _p(t):
    return ctypes.c_void_p(t.data_ptr() if t is not None else 0)


def _raw(image, nh, nw, xt, yt, out0, n0, out1, n1, cp, mean3, std3, div255, dtype, over=None):
    from cddmsl_amd import hip
    a = dict(img=_p(image), out0=_p(out0), out1=_p(out1), mean=hip._f3(mean3), std=hip._f3(std3), Hp0=out0.shape[1], Wp0=out0.shape[2], Cp=cp,
             xlo=_p(xt[0]), ylo=_p(yt[0]))
    a.update(over or {})       # overrides of single arguments (the refusal cases)
    rc = hip._L().cddmsl_tta_view(a["img"], image.shape[1], image.shape[2], nh, nw, a["xlo"], _p(xt[1]), _p(xt[2]), xt[3], a["ylo"], _p(yt[1]),
                                  _p(yt[2]), yt[3], a["out0"], n0, a["Hp0"], a["Wp0"], a["out1"], n1,
                                  out1.shape[1] if out1 is not None else 0, out1.shape[2] if out1 is not None else 0, a["Cp"], a["mean"],
                                  a["std"], int(div255), hip.DT[dtype], hip.stream_ptr())
    torch.cuda.synchronize()
    return rc


def _expect(view, Hp, Wp, mean, std, dtype, div255):
    from cddmsl_amd import hip
    return hip.preprocess([_chw(view)], Hp, Wp, mean, std, dtype, div255=div255)[0]


# ------------------------------------------------------------------------------------------------ 5. kernel against the restatement
@pytest.mark.parametrize("div255", [True, False], ids=["clip", "stock"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("pair", SHAPES, ids=_ids)
def test_kernel_equals_the_restatement(pair, dtype, div255):
    """plain view -> slot 0 of a batch of three padded to (newh + 3, neww + 5); mirror -> slot 1 of ANOTHER batch of three padded to
    (newh + 1, neww + 9): the two destinations of a pair that straddles two of the reference's batches"""
    (h, w), (nh, nw) = pair
    img, plain, mirror = _case(pair)
    mean, std = (CLIP_MEAN, CLIP_STD) if div255 else (STOCK_MEAN, STOCK_STD)
    Cp = 8 if dtype == torch.bfloat16 else 4
    out0, out1 = _nan_filled((3, nh + 3, nw + 5, Cp), dtype), _nan_filled((3, nh + 1, nw + 9, Cp), dtype)
    assert _raw(_chw(img), nh, nw, _tables(w, nw), _tables(h, nh), out0, 0, out1, 1, Cp, mean, std, div255, dtype) == 0
    want0, want1 = _expect(plain, nh + 3, nw + 5, mean, std, dtype, div255), _expect(mirror, nh + 1, nw + 9, mean, std, dtype, div255)
    assert torch.equal(_bits(out0[0]), _bits(want0))
    assert torch.equal(_bits(out1[1]), _bits(want1))
    assert _untouched(out0[1:]) and _untouched(out1[0]) and _untouched(out1[2])
    assert not bool(torch.isnan(out0[0]).any()) and bool((out0[0, nh:] == 0).all()) and bool((out0[0, :, nw:] == 0).all())
    assert bool((out0[0, :, :, 3:] == 0).all()) and bool((out1[1, :, :, 3:] == 0).all())


def test_f32_clip_separates_all_levels():
    """what makes bit equality in f32 pin every resampled byte: the 256 levels give 256 different f32 values per channel"""
    from cddmsl_amd import hip
    ramp = torch.arange(256, dtype=torch.uint8).view(1, 1, 256).expand(3, 1, 256).contiguous().to(DEV)
    x = hip.preprocess([ramp], 1, 256, CLIP_MEAN, CLIP_STD, torch.float32)[0, 0, :, :3]
    assert all(len(torch.unique(x[:, c])) == 256 for c in range(3))


def test_plain_view_only_and_same_tensor_pair():
    """out1 NULL: only the plain slot is written.  Both slots in ONE tensor (the usual case inside a batch): slots 1 and 2"""
    pair = ((150, 210), (97, 136))
    (h, w), (nh, nw) = pair
    img, plain, mirror = _case(pair)
    out = _nan_filled((3, nh + 2, nw + 2, 8), torch.bfloat16)
    xt, yt = _tables(w, nw), _tables(h, nh)
    assert _raw(_chw(img), nh, nw, xt, yt, out, 1, None, 0, 8, CLIP_MEAN, CLIP_STD, True, torch.bfloat16) == 0
    want = _expect(plain, nh + 2, nw + 2, CLIP_MEAN, CLIP_STD, torch.bfloat16, True)
    assert torch.equal(_bits(out[1]), _bits(want)) and _untouched(out[0]) and _untouched(out[2])
    assert _raw(_chw(img), nh, nw, xt, yt, out, 1, out, 2, 8, CLIP_MEAN, CLIP_STD, True, torch.bfloat16) == 0
    assert torch.equal(_bits(out[1]), _bits(want)) and _untouched(out[0])
    assert torch.equal(_bits(out[2]), _bits(_expect(mirror, nh + 2, nw + 2, CLIP_MEAN, CLIP_STD, torch.bfloat16, True)))


def test_channel_count_other_than_the_vector():
    """Cp = 5 in f32: the scalar store path, channels 3 and 4 zero"""
    pair = ((37, 53), (24, 34))
    (h, w), (nh, nw) = pair
    img, plain, mirror = _case(pair)
    from cddmsl_amd import hip
    out = _nan_filled((2, nh + 1, nw + 1, 5), torch.float32)
    assert _raw(_chw(img), nh, nw, _tables(w, nw), _tables(h, nh), out, 0, out, 1, 5, CLIP_MEAN, CLIP_STD, True, torch.float32) == 0
    for slot, view in ((0, plain), (1, mirror)):
        want = hip.preprocess([_chw(view)], nh + 1, nw + 1, CLIP_MEAN, CLIP_STD, torch.float32, Cp=5)[0]
        assert torch.equal(_bits(out[slot]), _bits(want))


# ------------------------------------------------------------------------------------------------ 6. refusals
def test_refusals_write_nothing():
    pair = ((37, 53), (24, 34))
    (h, w), (nh, nw) = pair
    img = _chw(_case(pair)[0])
    xt, yt = _tables(w, nw), _tables(h, nh)
    null = ctypes.c_void_p(0)
    for over in (dict(img=null), dict(out0=null), dict(mean=None), dict(std=None), dict(Hp0=nh - 1), dict(Wp0=nw - 1), dict(Cp=2), dict(xlo=null),
                 dict(ylo=null)):
        out0, out1 = _nan_filled((3, nh + 3, nw + 5, 4), torch.float32), _nan_filled((3, nh + 1, nw + 9, 4), torch.float32)
        assert _raw(img, nh, nw, xt, yt, out0, 0, out1, 1, 4, CLIP_MEAN, CLIP_STD, True, torch.float32, over) == 1, over
        assert _untouched(out0) and _untouched(out1), over
    out0, small = _nan_filled((3, nh + 3, nw + 5, 4), torch.float32), _nan_filled((3, nh - 1, nw + 9, 4), torch.float32)
    assert _raw(img, nh, nw, xt, yt, out0, 0, small, 1, 4, CLIP_MEAN, CLIP_STD, True, torch.float32) == 1       # the mirror's slot is too small
    assert _untouched(out0) and _untouched(small)


# ------------------------------------------------------------------------------------------------ 7. hip.tta_views grouping
IMG_HW, MIN_SIZES, MAX_SIZE = (128, 200), (96, 128, 160), 320


@functools.lru_cache(maxsize=None)
def _model_image():
    img = R.seeded_image(IMG_HW[0], IMG_HW[1], 3)
    vs = R.views(img, MIN_SIZES, MAX_SIZE, True)
    img.setflags(write=False)
    return img, vs


def _check_groups(groups, vs, batch_size, mean, std, dtype, div255):
    assert len(groups) == (len(vs) + batch_size - 1) // batch_size
    for g, (t, sizes) in enumerate(groups):
        mine = vs[g * batch_size:(g + 1) * batch_size]
        assert sizes == [(nh, nw) for _, (nh, nw, _) in mine]
        Hp, Wp = max(s[0] for s in sizes), max(s[1] for s in sizes)
        assert tuple(t.shape) == (len(mine), Hp, Wp, 8 if dtype == torch.bfloat16 else 4) and t.dtype == dtype and t.is_contiguous()
        for slot, (pix, _) in enumerate(mine):
            assert torch.equal(_bits(t[slot]), _bits(_expect(pix, Hp, Wp, mean, std, dtype, div255))), (g, slot)


@pytest.mark.parametrize("batch_size", [3, 4])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
def test_tta_views_grouping(batch_size, dtype):
    from cddmsl_amd import hip
    img, vs = _model_image()
    assert [v[1] for v in vs] == [(96, 150, False), (96, 150, True), (128, 200, False), (128, 200, True), (160, 250, False), (160, 250, True)]
    sizes = [v[1][:2] for v in vs[::2]]
    groups = hip.tta_views(_chw(img), sizes, True, CLIP_MEAN, CLIP_STD, dtype, batch_size=batch_size)
    _check_groups(groups, vs, batch_size, CLIP_MEAN, CLIP_STD, dtype, True)
    if batch_size == 3:
        assert [tuple(t.shape[1:3]) for t, _ in groups] == [(128, 200), (160, 250)]
        assert torch.equal(groups[0][0][2, :, :, :3].float(), hip.preprocess([_chw(img)], 128, 200, CLIP_MEAN, CLIP_STD, dtype)[0, :, :, :3].float())
    else:
        assert [tuple(t.shape[1:3]) for t, _ in groups] == [(128, 200), (160, 250)] and [t.shape[0] for t, _ in groups] == [4, 2]
    plain_only = hip.tta_views(_chw(img), sizes, False, STOCK_MEAN, STOCK_STD, dtype, batch_size=batch_size, div255=False)
    _check_groups(plain_only, vs[::2], batch_size, STOCK_MEAN, STOCK_STD, dtype, False)


# ------------------------------------------------------------------------------------------------ 8. model level
def _cfg():
    """the small synthetic model of tests/test_gpu_soft_nms.py::_model, with the TTA keys"""
    from cddmsl_amd.config import get_cfg
    cfg = get_cfg()
    cfg.merge_from_file(os.path.join(ROOT, "configs", "VOC-Experiments", "faster_rcnn_CLIP_R_50_C4.yaml"))
    cfg.merge_from_list(["MODEL.DEVICE", DEV, "INPUT.MIN_SIZE_TEST", 128, "INPUT.MAX_SIZE_TEST", 256, "MODEL.RPN.PRE_NMS_TOPK_TEST", 300,
                         "MODEL.RPN.POST_NMS_TOPK_TEST", 50, "MODEL.ROI_HEADS.SCORE_THRESH_TEST", 0.0, "TEST.DETECTIONS_PER_IMAGE", 20,
                         "TEST.AUG.MIN_SIZES", MIN_SIZES, "TEST.AUG.MAX_SIZE", MAX_SIZE, "TEST.AUG.FLIP", True])
    return cfg


@pytest.fixture(scope="module")
def cfg_model():
    from cddmsl_amd import synthetic
    from cddmsl_amd.modeling import build_model
    cfg = _cfg()
    model = build_model(cfg)
    model.load_state_dict(synthetic.make_state_dict(0), strict=False)
    return cfg, model.eval()


def _np(t):
    return t.detach().cpu().numpy()


def _records(vs):
    return [(256, 400, IMG_HW[0], IMG_HW[1], nh, nw, f) for _, (nh, nw, f) in vs]


def _check_merged(inst, per_view, vs):
    wb, ws, wc = R.merge(per_view, _records(vs), (256, 400), 0.5, 20)
    assert inst.image_size == (256, 400) and len(inst) == len(ws) <= 20 and len(ws) > 0
    assert np.array_equal(_np(inst.pred_boxes.tensor), wb) and np.array_equal(_np(inst.scores), ws)
    assert np.array_equal(_np(inst.pred_classes), wc)


def test_model_with_device_views(cfg_model, monkeypatch):
    """6 views in groups of 3: ``_inference_preprocessed`` sees exactly the tensors of test 7, twice, ``inference`` and the host never
    see a view; the result is the numpy un-mapping + merge of the captured per-view outputs (pre_tfm live: 128x200 handed for 256x400)"""
    from cddmsl_amd.modeling import GeneralizedRCNNWithTTA
    cfg, model = cfg_model
    img, vs = _model_image()
    seen, per_view = [], []
    orig = model._inference_preprocessed

    def spy(images, sizes, *a):
        out = orig(images, sizes, *a)
        seen.append((images.clone(), list(sizes)))
        per_view.extend((_np(o.pred_boxes.tensor), _np(o.scores), _np(o.pred_classes)) for o in out)
        return out

    def no_inference(*a, **k):
        raise AssertionError("the device path does not go through inference / preprocess_image")

    monkeypatch.setattr(model, "_inference_preprocessed", spy)
    monkeypatch.setattr(model, "inference", no_inference)
    tta = GeneralizedRCNNWithTTA(cfg, model)
    assert not tta.training and not model.training
    out = tta([{"image": torch.from_numpy(np.ascontiguousarray(img.transpose(2, 0, 1))), "height": 256, "width": 400}])
    assert len(out) == 1 and list(out[0]) == ["instances"]
    assert len(seen) == 2 and len(per_view) == 6
    _check_groups(seen, vs, 3, model.pixel_mean_list, model.pixel_std_list, model.compute_dtype, model.div_pixel)
    assert sum(len(p[1]) for p in per_view) > 20                           # the merge has something to cut
    _check_merged(out[0]["instances"], per_view, vs)


def test_model_with_the_host_mapper(cfg_model, monkeypatch):
    """``tta_mapper=DatasetMapperTTA(cfg)``: the reference's path -- views from PIL on the host through ``model.inference(group,
    do_postprocess=False)`` -- with the same pixels, and the same kind of result"""
    from cddmsl_amd.modeling import DatasetMapperTTA, GeneralizedRCNNWithTTA
    cfg, model = cfg_model
    img, vs = _model_image()
    calls, per_view = [], []
    orig = model.inference

    def spy(batched_inputs, detected_instances=None, do_postprocess=True):
        out = orig(batched_inputs, detected_instances, do_postprocess=do_postprocess)
        calls.append(([b["image"].clone() for b in batched_inputs], detected_instances, do_postprocess))
        per_view.extend((_np(o.pred_boxes.tensor), _np(o.scores), _np(o.pred_classes)) for o in out)
        return out

    monkeypatch.setattr(model, "inference", spy)
    tta = GeneralizedRCNNWithTTA(cfg, model, tta_mapper=DatasetMapperTTA(cfg))
    out = tta([{"image": torch.from_numpy(np.ascontiguousarray(img.transpose(2, 0, 1))), "height": 256, "width": 400}])
    assert len(calls) == 2 and all(c[1] is None and c[2] is False and len(c[0]) == 3 for c in calls)
    for got, (pix, _) in zip([i for c in calls for i in c[0]], vs):
        assert np.array_equal(_np(got).transpose(1, 2, 0), pix)
    _check_merged(out[0]["instances"], per_view, vs)
