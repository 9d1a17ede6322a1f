"""CPU: INPUT.COLOR_JITTER -- the draws (cddmsl_amd/augment.py::ColorJitter) pinned to the reference's RandomBrightness / RandomContrast /
RandomSaturation / RandomLighting / RandomApply through tests/golden/ref_color_jitter.npz (make_golden_color_jitter.py), the mapper's
behaviour with the block off, TWIN, the canonical arithmetic of ``color_jitter_u8`` against a float64 model, and every ValueError of
``config.check_color_jitter``."""
import os

import numpy as np
import pytest

from cddmsl_amd import augment, data
from cddmsl_amd.config import check_color_jitter, get_cfg

HERE = os.path.dirname(os.path.abspath(__file__))
ALL = {"BRIGHTNESS": (0.6, 1.4), "CONTRAST": (0.5, 1.5), "SATURATION": (0.4, 1.6), "LIGHTING": 40.0}


def _cfg(enabled=True, **kw):
    cfg = get_cfg()
    opts = ["INPUT.COLOR_JITTER.ENABLED", enabled]
    for k, v in kw.items():
        opts += ["INPUT." + k if k in ("FORMAT",) else "INPUT.COLOR_JITTER." + k, v]
    cfg.merge_from_list(opts)
    return cfg


# ---------------------------------------------------------------------------------------------------------------- configuration
def test_defaults_are_off():
    cfg = get_cfg()
    j = cfg.INPUT.COLOR_JITTER
    assert (j.ENABLED, j.PROB, tuple(j.BRIGHTNESS), tuple(j.CONTRAST), tuple(j.SATURATION), j.LIGHTING, j.TWIN) == \
        (False, 1.0, (1.0, 1.0), (1.0, 1.0), (1.0, 1.0), 0.0, "same")
    assert check_color_jitter(cfg) is None
    assert check_color_jitter(_cfg(True, **ALL)) is not None


@pytest.mark.parametrize("key,value", [
    ("BRIGHTNESS", (1.2, 0.8)), ("BRIGHTNESS", (-0.1, 1.0)), ("CONTRAST", (0.5,)), ("CONTRAST", (0.5, float("inf"))),
    ("SATURATION", (float("nan"), 1.0)), ("SATURATION", (0.5, 1.0, 1.5)), ("CONTRAST", ("a", "b")),
    ("LIGHTING", -0.1), ("LIGHTING", float("inf")), ("LIGHTING", float("nan")),
    ("PROB", -0.01), ("PROB", 1.5), ("PROB", float("nan")),
    ("TWIN", "mirror")])
def test_check_names_the_key(key, value):
    with pytest.raises(ValueError, match=r"INPUT\.COLOR_JITTER\." + key):
        check_color_jitter(_cfg(True, **{key: value}))
    with pytest.raises(ValueError, match=r"INPUT\.COLOR_JITTER\." + key):
        data.DatasetMapper(_cfg(True, **{key: value}), True)


@pytest.mark.parametrize("active", [{"SATURATION": (0.5, 1.5)}, {"LIGHTING": 0.1}])
def test_check_channel_order(active):
    with pytest.raises(ValueError, match=r"INPUT\.FORMAT"):
        check_color_jitter(_cfg(True, FORMAT="L", **active))
    assert check_color_jitter(_cfg(False, FORMAT="L", **active)) is None                 # (a disabled block does not judge the format)
    assert check_color_jitter(_cfg(True, FORMAT="L", BRIGHTNESS=(0.5, 1.5), CONTRAST=(0.5, 1.5))) is not None
    for fmt in ("RGB", "BGR"):
        assert check_color_jitter(_cfg(True, FORMAT=fmt, **active)) is not None


# ---------------------------------------------------------------------------------------------------------------- draws against the reference
@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(HERE, "golden", "ref_color_jitter.npz"))


@pytest.mark.parametrize("case", ["all", "contrast", "prob"])
def test_draws_equal_the_reference(golden, case):
    assert case in list(golden["case_names"])
    sp = [float(v) for v in golden[f"{case}/spec"]]
    cj = augment.ColorJitter(check_color_jitter(_cfg(True, PROB=sp[0], BRIGHTNESS=(sp[1], sp[2]), CONTRAST=(sp[3], sp[4]),
                                                      SATURATION=(sp[5], sp[6]), LIGHTING=sp[7], FORMAT="RGB")))
    names = ["brightness", "contrast", "saturation", "lighting"]
    outcomes = set()
    for seed in golden[f"{case}/seeds"]:
        for n in range(3):
            key = f"{case}/{int(seed)}/{n}"
            ops = [names[i] for i in golden[key + "/ops"]]
            params = cj.draw(np.random.RandomState(int(seed)))
            rec = []
            augment.color_jitter_u8(golden[f"img{n}"], params, False, rec)
            outcomes.add(bool(rec))
            assert [r[0] for r in rec] == ops, key
            for i, (name, sw, dw, src) in enumerate(rec):
                ref_sw, ref_dw, ref_src = (golden[f"{key}/{i}/{f}"] for f in ("src_weight", "dst_weight", "src_image"))
                # weights exactly: the doubles the reference hands to BlendTransform, 1 - w and w, are this side's before the float32 rounding
                if name != "lighting":
                    assert float(ref_dw) == params[name] and float(ref_sw) == 1.0 - params[name], key
                assert sw == np.float32(ref_sw) and dw == np.float32(ref_dw), key
                if name == "brightness":
                    assert float(ref_src) == 0.0 and float(src) == 0.0
                elif name == "contrast":                      # image.mean() of the reference (a double), rounded to float32
                    assert ref_src.shape == () and src == np.float32(ref_src), key
                elif name == "lighting":
                    assert ref_src.shape == (3,) and np.array_equal(src, ref_src.astype(np.float32)), key
                    assert np.array_equal(np.asarray(params["lighting"]), ref_src), key
                else:                                         # the grey image: float32 products against the reference's float64 dot
                    assert ref_src.shape == src.shape and np.abs(src - ref_src).max() <= 255 * 2.0 ** -22, key
    assert outcomes == ({True, False} if case == "prob" else {True})


# ---------------------------------------------------------------------------------------------------------------- the mapper
@pytest.fixture(scope="module")
def voc(tmp_path_factory):
    from test_data_pipeline import _make_voc
    return _make_voc(str(tmp_path_factory.mktemp("voc")), n=4)


def _mapper_cfg(enabled, fmt="BGR", **kw):
    cfg = _cfg(enabled, FORMAT=fmt, **kw)
    cfg.merge_from_list(["INPUT.MIN_SIZE_TRAIN", (64, 80, 96), "INPUT.MAX_SIZE_TRAIN", 128])
    return cfg


def _run(cfg, dicts, seed=11):
    m = data.DatasetMapper(cfg, True, np.random.RandomState(seed))
    return [m(d) for d in dicts], m.rng.get_state()


def _same_state(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2:] == b[2:]


@pytest.mark.parametrize("kw", [dict(enabled=False, **ALL), dict(enabled=True), dict(enabled=True, PROB=0.5),
                                dict(enabled=True, BRIGHTNESS=(1, 1), LIGHTING=0)])
def test_block_off_or_inactive_changes_nothing(voc, kw):
    dicts = data.load_voc_instances(voc, "trainval", dt_data="clipart")
    cfg0 = _mapper_cfg(False)
    del cfg0.INPUT["COLOR_JITTER"]                            # a configuration from before the block existed
    want, state0 = _run(cfg0, dicts)
    got, state1 = _run(_mapper_cfg(**kw), dicts)
    assert _same_state(state0, state1)
    for a, b in zip(want, got):
        assert np.array_equal(a["image"].numpy(), b["image"].numpy()) and np.array_equal(a["image_trgt"].numpy(), b["image_trgt"].numpy())
        assert np.array_equal(a["instances"].gt_boxes.tensor.numpy(), b["instances"].gt_boxes.tensor.numpy())


def test_test_mapper_ignores_the_block(voc):
    dicts = data.load_voc_instances(voc, "test")
    a = data.DatasetMapper(_mapper_cfg(True, **ALL), False)(dicts[0])
    b = data.DatasetMapper(_mapper_cfg(False), False)(dicts[0])
    assert np.array_equal(a["image"].numpy(), b["image"].numpy())
    data.DatasetMapper(_mapper_cfg(True, TWIN="mirror"), False)               # (and does not judge it)


@pytest.mark.parametrize("twin", ["same", "independent", "none"])
@pytest.mark.parametrize("fmt", ["RGB", "BGR"])
def test_twin_modes(voc, twin, fmt):
    """the mapper's output against a replay by hand: the geometric draws of a jitter-free mapper, then ColorJitter's on the same stream"""
    dicts = data.load_voc_instances(voc, "trainval", dt_data="clipart")
    cfg = _mapper_cfg(True, fmt, TWIN=twin, PROB=0.8, **ALL)
    got, state = _run(cfg, dicts)
    plain = data.DatasetMapper(_mapper_cfg(False, fmt), True, np.random.RandomState(11))
    cj = augment.ColorJitter(check_color_jitter(cfg))
    changed = 0
    for d, g in zip(dicts, got):
        base = plain(d)                                       # draws the short edge and the flip ...
        p = cj.draw(plain.rng)                                # ... then the image's parameters, then (independent) the twin's
        pt = {"same": p, "independent": None, "none": None}[twin]
        if twin == "independent":
            pt = cj.draw(plain.rng)
        for k, q in (("image", p), ("image_trgt", pt)):
            want = augment.color_jitter_u8(base[k].numpy().transpose(1, 2, 0), q, fmt == "BGR").transpose(2, 0, 1)
            assert np.array_equal(g[k].numpy(), want), (twin, k)
            changed += int(not np.array_equal(want, base[k].numpy()))
        if twin == "none":
            assert np.array_equal(g["image_trgt"].numpy(), base["image_trgt"].numpy())
        assert np.array_equal(g["instances"].gt_boxes.tensor.numpy(), base["instances"].gt_boxes.tensor.numpy())
    assert _same_state(state, plain.rng.get_state())
    assert changed >= (3 if twin == "none" else 6)            # (PROB 0.8 over four samples: most are jittered)


def test_sample_without_twin_draws_once(voc):
    dicts = data.load_voc_instances(voc, "trainval")          # no dt_data: no twins
    cfg = _mapper_cfg(True, TWIN="independent", **ALL)
    got, state = _run(cfg, dicts)
    plain = data.DatasetMapper(_mapper_cfg(False), True, np.random.RandomState(11))
    cj = augment.ColorJitter(check_color_jitter(cfg))
    for d, g in zip(dicts, got):
        base = plain(d)
        want = augment.color_jitter_u8(base["image"].numpy().transpose(1, 2, 0), cj.draw(plain.rng), True).transpose(2, 0, 1)
        assert "image_trgt" not in g and np.array_equal(g["image"].numpy(), want)
    assert _same_state(state, plain.rng.get_state())


def test_device_record_carries_the_draws(voc):
    """DATALOADER.DEVICE_RESIZE: the mapper hands the decoded image on untouched, with the parameters of the host path in its record"""
    dicts = data.load_voc_instances(voc, "trainval", dt_data="clipart")
    cfg = _mapper_cfg(True, TWIN="independent", **ALL)
    cfg.merge_from_list(["DATALOADER.DEVICE_RESIZE", True])
    plain_cfg = _mapper_cfg(False)
    plain_cfg.merge_from_list(["DATALOADER.DEVICE_RESIZE", True])
    m, plain = data.DatasetMapper(cfg, True, np.random.RandomState(4)), data.DatasetMapper(plain_cfg, True, np.random.RandomState(4))
    cj = augment.ColorJitter(check_color_jitter(cfg))
    for d in dicts:
        g, base = m(d), plain(d)
        p, pt = cj.draw(plain.rng), cj.draw(plain.rng)
        assert g[data.DEVICE_RESIZE_KEY]["jitter"] == {"image": p, "image_trgt": pt}
        assert "jitter" not in base[data.DEVICE_RESIZE_KEY]
        assert np.array_equal(g["image"].numpy(), base["image"].numpy()) and g[data.DEVICE_RESIZE_KEY]["size"] == base[data.DEVICE_RESIZE_KEY]["size"]


# ---------------------------------------------------------------------------------------------------------------- arithmetic
def _exact(img, name, value, bgr):
    """the blend in float64 on exact operands -> (floor(clip(v)), v)"""
    x = img.astype(np.float64)
    if name == "lighting":
        vec = np.asarray(value, dtype=np.float64)
        v = x + (vec[::-1] if bgr else vec)
    else:
        if name == "brightness":
            src = 0.0
        elif name == "contrast":
            src = x.mean()
        else:
            r, g, b = (x[..., 2], x[..., 1], x[..., 0]) if bgr else (x[..., 0], x[..., 1], x[..., 2])
            src = (0.299 * r + 0.587 * g + 0.114 * b)[..., None]
        v = (1.0 - value) * src + value * x
    return np.floor(np.clip(v, 0.0, 255.0)), v


WEIGHTS = [1.0, 0.0, 2.5, 0.37, 0.8125, 1.3]


@pytest.mark.parametrize("bgr", [False, True])
@pytest.mark.parametrize("name", ["brightness", "contrast", "saturation"])
@pytest.mark.parametrize("w", WEIGHTS)
def test_blend_against_float64(name, w, bgr):
    """at most 1 off on every byte, equal wherever the double result is at least 2^-10 from an integer (the float32 rounding of three
    operands below 512, relative 2^-24 each, stays far inside that margin)"""
    img = np.random.RandomState(5).randint(0, 256, (37, 29, 3), dtype=np.uint8)
    img[:4, :4] = [[255, 0, 0]]
    got = augment.color_jitter_u8(img, {name: w}, bgr)
    assert got.dtype == np.uint8 and got.shape == img.shape
    want, v = _exact(img, name, w, bgr)
    diff = np.abs(got.astype(np.float64) - want)
    assert diff.max() <= 1
    far = np.abs(v - np.round(v)) >= 2.0 ** -10
    assert (far.any() or w in (0.0, 1.0)) and np.array_equal(got[far], want[far].astype(np.uint8))   # (w 0 / 1 can give integers only; below)
    if w == 1.0:
        assert np.array_equal(got, img)
    if w == 2.5:
        assert (got == 255).any() and ((got == 0).any() or name == "brightness")
    if w == 0.0:
        if name == "brightness":
            assert not got.any()
        elif name == "contrast":
            assert (got == int(img.mean())).all()
        else:
            r, g, b = (img[..., 2], img[..., 1], img[..., 0]) if bgr else (img[..., 0], img[..., 1], img[..., 2])
            f = np.float32
            grey = np.trunc((f(0.299) * r.astype(f) + f(0.587) * g.astype(f)) + f(0.114) * b.astype(f)).astype(np.uint8)
            assert all(np.array_equal(got[..., c], grey) for c in range(3))


@pytest.mark.parametrize("bgr", [False, True])
@pytest.mark.parametrize("vec", [[-30.25, -3.5, -200.0], [12.3, -0.4, 7.75], [300.0, 0.0, -0.001]])
def test_lighting_against_float64(vec, bgr):
    img = np.random.RandomState(6).randint(0, 256, (19, 23, 3), dtype=np.uint8)
    got = augment.color_jitter_u8(img, {"lighting": vec}, bgr)
    want, v = _exact(img, "lighting", vec, bgr)
    assert np.abs(got.astype(np.float64) - want).max() <= 1
    far = np.abs(v - np.round(v)) >= 2.0 ** -10
    assert np.array_equal(got[far], want[far].astype(np.uint8))
    if max(vec) < 0:
        assert all((got[..., c] == 0).any() for c in range(3))          # (every channel clips at 0 somewhere)


def test_chain_reads_the_uint8_result_of_the_step_before():
    img = np.random.RandomState(7).randint(0, 256, (9, 11, 3), dtype=np.uint8)
    p = {"brightness": 1.3, "contrast": 0.7, "saturation": 1.4, "lighting": [3.5, -2.25, 9.0]}
    want = img
    for k in ("brightness", "contrast", "saturation", "lighting"):
        want = augment.color_jitter_u8(want, {k: p[k]}, True)
    assert np.array_equal(augment.color_jitter_u8(img, p, True), want)
    assert np.array_equal(augment.color_jitter_u8(img, None, True), img) and np.array_equal(augment.color_jitter_u8(img, {}, False), img)
    flipped = img[:, ::-1]                                    # a view with a negative stride, as the mapper's flip hands over
    assert np.array_equal(augment.color_jitter_u8(flipped, p, False), augment.color_jitter_u8(np.ascontiguousarray(flipped), p, False))


def test_descriptor_fields():
    p = {"brightness": 1.25, "saturation": 0.1, "lighting": [1.5, -2.0, 0.25]}
    d = augment.descriptor(77, 5, 9, p, True)
    bits = lambda v: int(np.float32(v).view(np.int32))       # noqa: E731
    assert d == (77, 5, 9, augment.BRIGHTNESS | augment.SATURATION | augment.LIGHTING, 1, bits(1.25), bits(-0.25), 0, 0,
                 bits(0.1), bits(np.float32(1.0 - 0.1)), bits(1.5), bits(-2.0), bits(0.25), 0)
    assert augment.descriptor(0, 1, 1, None, False)[3] == 0 and len(d) == 15


# ---------------------------------------------------------------------------------------------------- the raw C-ABI, no GPU needed
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from cddmsl_amd import _lib
    return _lib.lib_color_jitter()


def test_side_library_exports_its_header(lib, tmp_path):
    """libcddmsl_color_jitter.so exports what include/cddmsl_color_jitter.h declares and nothing else; the header is C and its item
    is the 64 bytes hip.JitterItem mirrors"""
    import ctypes
    import re
    import subprocess
    from cddmsl_amd import _lib, hip
    hdr = re.sub(r"/\*.*?\*/", " ", open(_lib.COLOR_JITTER_HEADER_PATH).read(), flags=re.S)
    names = sorted(set(re.findall(r"\bint\s+(cddmsl_\w+)\s*\(", hdr)))
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.COLOR_JITTER_LIB_PATH], text=True)
    assert sorted(set(re.findall(r"\bT (cddmsl_\w+)", out))) == names == ["cddmsl_color_jitter_batch_u8"]
    subprocess.check_call(["gcc", "-std=c99", "-fsyntax-only", "-x", "c", _lib.COLOR_JITTER_HEADER_PATH])
    main = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    assert "cddmsl_color_jitter" not in main
    vp, ci, cl = ctypes.c_void_p, ctypes.c_int, ctypes.c_long
    assert lib.cddmsl_color_jitter_batch_u8.restype is ci and lib.cddmsl_color_jitter_batch_u8.argtypes == [vp, cl, vp, ci, vp, vp]
    members = [m for m, _ in _lib.header_struct(open(_lib.COLOR_JITTER_HEADER_PATH).read(), "cddmsl_jitter_item")]
    assert members == [f[0] for f in hip.JitterItem._fields_] and ctypes.sizeof(hip.JitterItem) == 64
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include "cddmsl_color_jitter.h"\nint main(void) { printf("%zu", sizeof(cddmsl_jitter_item)); return 0; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.dirname(_lib.COLOR_JITTER_HEADER_PATH), str(src), "-o", str(tmp_path / "layout")])
    assert subprocess.check_output([str(tmp_path / "layout")], text=True) == "64"


def test_cabi_argument_errors_return_before_any_hip_call(lib):
    import ctypes
    from cddmsl_amd import hip
    host = (ctypes.c_ubyte * 4096)()                                  # never dereferenced: every call below returns at the checks
    sums = (ctypes.c_long * 4)()
    good = augment.descriptor(16, 10, 12, {"brightness": 0.5, "contrast": 1.5, "lighting": [1.0, 2.0, 3.0]}, True)
    names = [f[0] for f in hip.JitterItem._fields_]
    nan, inf = int(np.float32("nan").view(np.int32)), int(np.float32("inf").view(np.int32))

    def call(nbytes=4096, count=None, with_sums=True, buf=True, **edit):
        it = list(good)
        for k, v in edit.items():
            it[names.index(k)] = v
        arr = (hip.JitterItem * 2)(hip.JitterItem(*augment.descriptor(2000, 3, 3, None, False)), hip.JitterItem(*it))
        return lib.cddmsl_color_jitter_batch_u8(host if buf else None, nbytes, arr, 2 if count is None else count, sums if with_sums else None, None)

    assert call(count=-1) == 1 and call(nbytes=-1) == 1 and call(buf=False) == 1 and call(with_sums=False) == 1
    assert call(h=0) == 1 and call(w=-1) == 1 and call(h=2 ** 30, w=2 ** 30) == 1 and call(ops=16) == 1 and call(ops=-1) == 1
    assert call(off=-1) == 1 and call(off=4096 - 359) == 1 and call(nbytes=16 + 359) == 1 and call(off=4097) == 1
    assert call(b_dw=nan) == 1 and call(b_sw=inf) == 1 and call(c_dw=nan) == 1 and call(c_sw=nan) == 1 and call(light_b=inf) == 1
    assert call(ops=augment.SATURATION, s_dw=nan) == 1
    assert call(count=0) == 0 and lib.cddmsl_color_jitter_batch_u8(None, 0, None, 0, None, None) == 0
    assert call(ops=0, b_dw=nan, light_r=nan) == 0                   # no active operation: members ignored, nothing to launch
