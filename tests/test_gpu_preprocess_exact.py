"""The image-input kernels (cddmsl_amd/csrc/elementwise.hip: cddmsl_preprocess, cddmsl_preprocess_batch, cddmsl_preprocess224,
cddmsl_preprocess224_batch) against the float32 restatements of tests/exact_preprocess.py, compared as RAW BITS in f32 and bf16
(tests/test_preprocess_ref_host.py holds the restatements to float64 ATen bicubic).  The entries are called through the C-ABI into
NaN-filled outputs with one spare image slot, so an unwritten element and a write past the batch both show; the pad channels must be
+0.  Cases (exact_preprocess.CASES224): top != 0, left != 0, the identity geometry (bit-equal to cddmsl_preprocess_batch too),
upscaling, windows across the image / pad / clamp borders, size 224, 33 images (two launches), and Cp = VEC, 3, 5, 16.
On one MI355X every case is bit-equal, both divisions included (102 tests in 2.4 s)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import exact_preprocess as E

pytestmark = pytest.mark.gpu
DEV = "cuda"
ERR_ARG = 1
NAN_BITS = {torch.float32: (torch.int32, 0x7FC00001), torch.bfloat16: (torch.int16, 0x7FC1)}
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16}
BY_NAME = {c["name"]: c for c in E.CASES224}


def _hip():
    from cddmsl_amd import hip
    return hip


def _p(t):
    return ctypes.c_void_p(t.data_ptr() if t is not None else 0)


def _nan_filled(shape, dtype):
    it, bits = NAN_BITS[dtype]
    t = torch.full(shape, bits, dtype=it, device=DEV).view(dtype)
    assert bool(torch.isnan(t).all())
    return t


def _bits(t):
    return t.contiguous().view(NAN_BITS[t.dtype][0])


def _untouched(t):
    return bool((_bits(t) == NAN_BITS[t.dtype][1]).all())


def _assert_bits(got, want, what):
    g, w = _bits(got.cpu()).long(), _bits(want).long()
    if not torch.equal(g, w):
        bad = (g != w)
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements differ, largest distance {int((g - w).abs().max())} ulp, "
                             f"first at {bad.nonzero()[0].tolist()}: got {got.cpu()[tuple(bad.nonzero()[0])]}, want {want[tuple(bad.nonzero()[0])]}")


def _cp(cp, dname):
    return E.VEC[dname] if cp is None else cp


@functools.lru_cache(maxsize=None)
def _case(name):
    """(images uint8 CHW, restatement [N, S, S, 3] float32) of a case: computed once, shared, never written"""
    c = BY_NAME[name]
    imgs = E.case_images(c)
    ref = np.stack([E.preprocess224_f32(im, c["pad"][0], c["pad"][1], c["RH"], c["RW"], c["top"], c["left"], c["size"], E.CLIP_MEAN, E.CLIP_STD)
                    for im in imgs])
    ref.setflags(write=False)
    return imgs, ref


def _dev(imgs):
    return [torch.from_numpy(im).to(DEV) for im in imgs]


def _table(dimgs, null_at=None):
    n = len(dimgs)
    ptrs = (ctypes.c_void_p * n)(*[None if j == null_at else im.data_ptr() for j, im in enumerate(dimgs)])
    hs = (ctypes.c_int * n)(*[int(im.shape[1]) for im in dimgs])
    ws = (ctypes.c_int * n)(*[int(im.shape[2]) for im in dimgs])
    return ptrs, hs, ws


def _batch224(dimgs, out, c, cp, dtype, over=None, null_at=None, hs=None):
    hip = _hip()
    a = dict(Hp=c["pad"][0], Wp=c["pad"][1], RH=c["RH"], RW=c["RW"], top=c["top"], left=c["left"], S=c["size"], Cp=cp)
    a.update(over or {})
    ptrs, h0, ws = _table(dimgs, null_at)
    rc = hip._L().cddmsl_preprocess224_batch(ptrs, hs or h0, ws, len(dimgs), _p(out), a["Hp"], a["Wp"], a["RH"], a["RW"], a["top"], a["left"],
                                             a["S"], a["Cp"], hip._f3(E.CLIP_MEAN), hip._f3(E.CLIP_STD), hip.DT[dtype], hip.stream_ptr())
    torch.cuda.synchronize()
    return rc


# ------------------------------------------------------------------------------------------------ preprocess224
@pytest.mark.parametrize("cp", E.CP, ids=lambda v: "CpVEC" if v is None else f"Cp{v}")
@pytest.mark.parametrize("dname", list(DTYPES))
@pytest.mark.parametrize("name", list(BY_NAME))
def test_preprocess224_batch_bit_equal(name, dname, cp):
    c, dtype, cp = BY_NAME[name], DTYPES[dname], _cp(cp, dname)
    imgs, ref = _case(name)
    dimgs, N, S = _dev(imgs), len(imgs), c["size"]
    out = _nan_filled((N + 1, S, S, cp), dtype)
    assert _batch224(dimgs, out, c, cp, dtype) == 0
    _assert_bits(out[:N], E.to_layout(ref, cp, dtype), f"{name} {dname} Cp={cp}")
    assert _untouched(out[N:]), "the slot past the batch was written"
    # the wrapper computes the same geometry and makes the same call
    via = _hip().preprocess224(dimgs, c["pad"][0], c["pad"][1], E.CLIP_MEAN, E.CLIP_STD, dtype, size=S, Cp=cp)
    assert torch.equal(_bits(via), _bits(out[:N]))


@pytest.mark.parametrize("dname", list(DTYPES))
@pytest.mark.parametrize("name", list(BY_NAME))
def test_preprocess224_single_image_entry_bit_equal(name, dname):
    hip = _hip()
    c, dtype = BY_NAME[name], DTYPES[dname]
    imgs, ref = _case(name)
    imgs, S = imgs[:3], c["size"]
    dimgs = _dev(imgs)
    for cp in (E.VEC[dname], 5):
        out = _nan_filled((len(imgs) + 1, S, S, cp), dtype)
        for n in range(len(imgs) - 1, -1, -1):                  # last slot first: an entry writes its own slot only
            rc = hip._L().cddmsl_preprocess224(_p(dimgs[n]), _p(out), n, imgs[n].shape[1], imgs[n].shape[2], c["pad"][0], c["pad"][1], c["RH"],
                                               c["RW"], c["top"], c["left"], S, cp, hip._f3(E.CLIP_MEAN), hip._f3(E.CLIP_STD), hip.DT[dtype],
                                               hip.stream_ptr())
            torch.cuda.synchronize()
            assert rc == 0
            assert _untouched(out[:n]) and _untouched(out[len(imgs):])
        _assert_bits(out[:len(imgs)], E.to_layout(ref[:len(imgs)], cp, dtype), f"{name} {dname} Cp={cp}")


@pytest.mark.parametrize("dname", list(DTYPES))
def test_identity_geometry_equals_preprocess(dname):
    """Hp = Wp = size: t = 0 on both axes, the weights are exactly (0, 1, 0, 0), and inside each image the bicubic kernel must
    return what the full-resolution kernel returns, bit for bit.  Outside the image the two differ by design: the training path
    pads before it normalises ((0 - m) / s), the inference path after (0)."""
    c, dtype = BY_NAME["identity"], DTYPES[dname]
    imgs, ref = _case("identity")
    dimgs, S = _dev(imgs), c["size"]
    a = _hip().preprocess224(dimgs, S, S, E.CLIP_MEAN, E.CLIP_STD, dtype, size=S).cpu()
    b = _hip().preprocess(dimgs, S, S, E.CLIP_MEAN, E.CLIP_STD, dtype).cpu()
    want = np.stack([E.preprocess_f32(im, S, S, E.CLIP_MEAN, E.CLIP_STD) for im in imgs])
    zero = ((np.float32(0) - np.asarray(E.CLIP_MEAN, np.float32)) / np.asarray(E.CLIP_STD, np.float32)).astype(np.float32)
    pad = E.to_layout(np.broadcast_to(zero, (S, S, 3)).copy(), a.shape[-1], dtype)
    for n, im in enumerate(imgs):
        h, w = im.shape[1:]
        assert torch.equal(_bits(a[n, :h, :w]), _bits(b[n, :h, :w])), n
        outside = torch.ones(S, S, dtype=torch.bool)
        outside[:h, :w] = False
        assert bool((_bits(b[n])[outside] == 0).all()) and torch.equal(_bits(a[n])[outside], _bits(pad)[outside])
        assert np.array_equal(want[n, :h, :w].view(np.int32), np.asarray(ref)[n, :h, :w].view(np.int32))   # and so do the restatements


# ------------------------------------------------------------------------------------------------ preprocess
def _levels_image():
    """[3, 16, 16]: every channel holds all 256 levels, each in another order"""
    rs = np.random.RandomState(5)
    return np.stack([np.arange(256), rs.permutation(256), 255 - np.arange(256)]).astype(np.uint8).reshape(3, 16, 16)


PRE_CASES = {
    "levels": ([_levels_image()], (16, 16)),
    "levels_in_pad": ([_levels_image()], (19, 21)),
    "full_height": ([E.seeded_image(13, 9, 1)], (13, 17)),            # h = Hp, w < Wp
    "full_width": ([E.seeded_image(6, 17, 2)], (13, 17)),             # w = Wp, h < Hp
    "one_pixel": ([E.seeded_image(1, 1, 3)], (1, 1)),
    "one_pixel_in_pad": ([E.seeded_image(1, 1, 4), E.seeded_image(3, 2, 5)], (3, 5)),
    "batch_split": ([E.seeded_image(*((11, 7) if i % 2 else (8, 12)), 60 + i) for i in range(E.PRE_MAX + 1)], (11, 12)),
}


@pytest.mark.parametrize("div255", [True, False], ids=["div255", "raw"])
@pytest.mark.parametrize("dname", list(DTYPES))
@pytest.mark.parametrize("name", list(PRE_CASES))
def test_preprocess_bit_equal(name, dname, div255):
    hip = _hip()
    imgs, (Hp, Wp) = PRE_CASES[name]
    dtype = DTYPES[dname]
    mean, std = (E.CLIP_MEAN, E.CLIP_STD) if div255 else (E.STOCK_MEAN, E.STOCK_STD)
    ref = np.stack([E.preprocess_f32(im, Hp, Wp, mean, std, div255) for im in imgs])
    dimgs, N = _dev(imgs), len(imgs)
    for cp in [_cp(v, dname) for v in E.CP]:
        want = E.to_layout(ref, cp, dtype)
        out = _nan_filled((N + 1, Hp, Wp, cp), dtype)
        ptrs, hs, ws = _table(dimgs)
        rc = hip._L().cddmsl_preprocess_batch(ptrs, hs, ws, N, _p(out), Hp, Wp, cp, hip._f3(mean), hip._f3(std), int(div255), hip.DT[dtype],
                                              hip.stream_ptr())
        torch.cuda.synchronize()
        assert rc == 0
        _assert_bits(out[:N], want, f"batch {name} {dname} Cp={cp}")
        assert _untouched(out[N:])
        one = _nan_filled((min(N, 2) + 1, Hp, Wp, cp), dtype)
        for n in range(min(N, 2) - 1, -1, -1):
            rc = hip._L().cddmsl_preprocess(_p(dimgs[n]), _p(one), n, imgs[n].shape[1], imgs[n].shape[2], Hp, Wp, cp, hip._f3(mean), hip._f3(std),
                                            int(div255), hip.DT[dtype], hip.stream_ptr())
            torch.cuda.synchronize()
            assert rc == 0 and _untouched(one[:n]) and _untouched(one[min(N, 2):])
        _assert_bits(one[:min(N, 2)], want[:min(N, 2)], f"single {name} {dname} Cp={cp}")
    assert torch.equal(_bits(hip.preprocess(dimgs, Hp, Wp, mean, std, dtype, div255=div255)),
                       _bits(E.to_layout(ref, E.VEC[dname], dtype).to(DEV)))


# ------------------------------------------------------------------------------------------------ refusals
@pytest.mark.parametrize("dname", list(DTYPES))
def test_refusals_write_nothing(dname):
    hip = _hip()
    dtype, c = DTYPES[dname], BY_NAME["portrait"]
    imgs, _ = _case("portrait")
    dimgs, N, S, cp = _dev(imgs), len(imgs), c["size"], E.VEC[dname]
    out = _nan_filled((N + 1, S, S, cp), dtype)
    Hp, Wp = c["pad"]
    m, s, st = hip._f3(E.CLIP_MEAN), hip._f3(E.CLIP_STD), hip.stream_ptr()
    tall = (ctypes.c_int * N)(*([Hp + 1] + [im.shape[1] for im in imgs[1:]]))
    assert _batch224(dimgs, out, c, cp, dtype, hs=tall) == ERR_ARG                                   # h > Hp
    assert _batch224(dimgs, out, c, 2, dtype) == ERR_ARG                                             # Cp = 2
    assert _batch224(dimgs, out, c, cp, dtype, over=dict(top=c["RH"] - S + 1)) == ERR_ARG            # top + S > RH
    assert _batch224(dimgs, out, c, cp, dtype, over=dict(left=c["RW"] - S + 1)) == ERR_ARG
    assert _batch224(dimgs, out, c, cp, dtype, null_at=N - 1) == ERR_ARG                             # a null image in the table
    h0, w0 = imgs[0].shape[1:]
    L = hip._L()
    assert L.cddmsl_preprocess224(_p(dimgs[0]), _p(out), 0, Hp + 1, w0, Hp, Wp, c["RH"], c["RW"], c["top"], c["left"], S, cp, m, s,
                                  hip.DT[dtype], st) == ERR_ARG
    assert L.cddmsl_preprocess224(_p(dimgs[0]), _p(out), 0, h0, w0, Hp, Wp, c["RH"], c["RW"], c["top"], c["left"], S, 2, m, s,
                                  hip.DT[dtype], st) == ERR_ARG
    assert L.cddmsl_preprocess224(_p(dimgs[0]), _p(out), 0, h0, w0, Hp, Wp, c["RH"], c["RW"], c["RH"] - S + 1, c["left"], S, cp, m, s,
                                  hip.DT[dtype], st) == ERR_ARG
    torch.cuda.synchronize()
    assert _untouched(out)
    full = _nan_filled((N + 1, Hp, Wp, cp), dtype)
    ptrs, hs, ws = _table(dimgs)
    assert L.cddmsl_preprocess_batch(ptrs, tall, ws, N, _p(full), Hp, Wp, cp, m, s, 1, hip.DT[dtype], st) == ERR_ARG
    assert L.cddmsl_preprocess_batch(ptrs, hs, ws, N, _p(full), Hp, Wp, 2, m, s, 1, hip.DT[dtype], st) == ERR_ARG
    nptrs, _, _ = _table(dimgs, null_at=0)
    assert L.cddmsl_preprocess_batch(nptrs, hs, ws, N, _p(full), Hp, Wp, cp, m, s, 1, hip.DT[dtype], st) == ERR_ARG
    assert L.cddmsl_preprocess(_p(dimgs[0]), _p(full), 0, Hp + 1, w0, Hp, Wp, cp, m, s, 1, hip.DT[dtype], st) == ERR_ARG
    assert L.cddmsl_preprocess(_p(dimgs[0]), _p(full), 0, h0, w0, Hp, Wp, 2, m, s, 1, hip.DT[dtype], st) == ERR_ARG
    torch.cuda.synchronize()
    assert _untouched(full)
