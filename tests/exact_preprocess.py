"""Checker of the image-input kernels (cddmsl_amd/csrc/elementwise.hip: k_preprocess[_batch], k_preprocess224[_batch]).  Imports
without a GPU.  Three things live here:

(a) ``preprocess_f32`` / ``preprocess224_f32``: numpy float32 restatements in the kernels' operation order.  The library is built
    with -ffp-contract=off and IEEE division, so every f32 operation of the kernel is one numpy float32 operation and the kernels
    are held to these BIT FOR BIT (tests/test_gpu_preprocess_exact.py).  bf16 output is round-to-nearest-even of the f32 value.
(b) ``preprocess224_f64``: x/255 -> zero pad -> ATen bicubic (align_corners=False) in float64 -> crop -> normalise, what the
    reference model computes.
(c) ``bound224``: the derived distance allowed between (a) and (b) (tests/test_preprocess_ref_host.py holds (a) to it and shows
    that it rejects the MUTANTS of (a)).

Derivation of (c), u = 2^-24, pixel values v = px/255 in [0, vmax], W the cubic convolution kernel with A = -0.75:
  coordinate  fy = fl(fl((oy+top+0.5) * fl(Hp/RH)) - 0.5): the quotient and the product carry a relative u each of |fy + 0.5|, the
              subtraction u |fy|, so |dfy| <= 3 u (|fy| + 0.5); t = fy - floor(fy) adds at most u.  The interpolant
              sum_k W(fy - k) row_k is C1 in fy (also across a change of floor(fy)), and sum_k |W'(fy - k)| <= 2 * 1.35 + 2 * 0.75
              = 4.2 (|cubic1'| <= 1.35 at x = 0.6, |cubic2'| <= 0.75 at x = 1), so the result moves by at most
              4.2 * (3 (|fy| + 0.5) + 1) u * max_k |row_k|, |row_k| <= sum_b |wx_b| vmax; the same for fx.  This term grows with the
              image size and dominates from a few hundred rows on.
  weights     Horner in f32: cubic1 on [0, 1] has intermediates 1.25, 2.25, 2.25, 2.25, 1 (9 u, later factors x <= 1) and its
              argument 1 - t one rounding (u * 1.35): <= 11 u absolute.  cubic2 on [1, 2] has intermediates 1.5, 3, 4.5, 3.75, 3,
              0.6 amplified by the later factors x <= 2 (6 + 12 + 9 + 7.5 + 3 + 0.6 u) and its argument 2 u * 0.75: <= 40 u.
              An absolute weight error dw moves the result by dw * (4 sum|wx| + 4 sum|wy|) vmax at most.
  sums        one division, two products and 2 * 4 additions per term: 11 u sum |wy| |wx| |v| (x 1.001 for the higher orders).
  normalise   (acc - m) / s with the f32 m, s that (b) uses too: the errors above divided by s, plus 2 u |out|.
"""
import numpy as np
import torch
import torch.nn.functional as F

U = 2.0 ** -24
CLIP_MEAN, CLIP_STD = [0.48145466, 0.4578275, 0.40821073], [0.26862954, 0.26130258, 0.27577711]
STOCK_MEAN, STOCK_STD = [103.530, 116.280, 123.675], [57.375, 57.120, 58.395]
PRE_MAX = 32                        # images per launch of the batched entries (elementwise.hip)
VEC = {"f32": 4, "bf16": 8}         # the channel count at which a pixel is one 16-byte store
DW_SUM, DW_C1, DW_C2, ACC_OPS = 4.2, 11.0, 40.0, 11.0
MUTANTS = ("A=-0.5", "top dropped", "sx/sy swapped", "clamp at h-1", "half-pixel shift")

f32 = np.float32


def geometry(Hp, Wp, size):
    """(RH, RW, top, left) of hip.preprocess224: short side of the padded batch to ``size``, centre crop"""
    if Wp <= Hp:
        RW, RH = size, int(size * Hp / Wp)
    else:
        RH, RW = size, int(size * Wp / Hp)
    return RH, RW, int(round((RH - size) / 2.0)), int(round((RW - size) / 2.0))


def seeded_image(h, w, seed):
    """uint8 [3, h, w], full range, both extremes present"""
    img = np.random.RandomState(seed).randint(0, 256, (3, h, w)).astype(np.uint8)
    img.reshape(-1)[0] = 255
    img.reshape(-1)[-1] = 0
    return img


# ------------------------------------------------------------------------------------------------ (a) f32 restatements
def preprocess_f32(img, Hp, Wp, mean, std, div255=True):
    """[Hp, Wp, 3] float32: ((float)px / div - m) / s inside the image, 0 outside"""
    _, h, w = img.shape
    out = np.zeros((Hp, Wp, 3), f32)
    div = f32(255.0 if div255 else 1.0)
    for c in range(3):
        out[:h, :w, c] = (img[c].astype(f32) / div - f32(mean[c])) / f32(std[c])
    return out


def _cubic1(x, A, one, two, three):
    return ((A + two) * x - (A + three)) * x * x + one


def _cubic2(x, A, four, five, eight):
    return ((A * x - five * A) * x + eight * A) * x - four * A


def _axis(n_out, off, scale, ft, A, shift=0.5):
    """source coordinate, first tap and the four weights of outputs 0..n_out-1 of one axis, in the float type ``ft``"""
    c = lambda v: ft(v)
    f = (np.arange(n_out).astype(ft) + ft(off) + c(shift)) * scale - c(0.5)       # (float)(o + off): small integers, exact
    i = np.floor(f)
    t = (f - i).astype(ft)
    A = c(A)
    w = np.stack([_cubic2(t + c(1), A, c(4), c(5), c(8)), _cubic1(t, A, c(1), c(2), c(3)),
                  _cubic1(c(1) - t, A, c(1), c(2), c(3)), _cubic2(c(2) - t, A, c(4), c(5), c(8))]).astype(ft)
    return f, i.astype(np.int64), w


def preprocess224_formula(img, Hp, Wp, RH, RW, top, left, S, mean, std, ft=f32, mutant=None):
    """[S, S, 3] in the float type ``ft``: the kernel's formula in the kernel's order (ft = float32: restatement (a))"""
    assert mutant is None or mutant in MUTANTS
    _, h, w = img.shape
    sy, sx = ft(Hp) / ft(RH), ft(Wp) / ft(RW)
    if mutant == "sx/sy swapped":
        sy, sx = sx, sy
    A = -0.5 if mutant == "A=-0.5" else -0.75
    shift = 0.0 if mutant == "half-pixel shift" else 0.5
    _, iy, wy = _axis(S, 0 if mutant == "top dropped" else top, sy, ft, A, shift)
    _, ix, wx = _axis(S, left, sx, ft, A, shift)
    cy, cx = (h - 1, w - 1) if mutant == "clamp at h-1" else (Hp - 1, Wp - 1)
    v = img.astype(ft) / ft(255.0)                                                  # [3, h, w]
    acc = np.zeros((3, S, S), ft)
    for a in range(4):
        yy = np.clip(iy - 1 + a, 0, cy)
        r = np.zeros((3, S, S), ft)
        for b in range(4):
            xx = np.clip(ix - 1 + b, 0, cx)
            inside = (yy < h)[:, None] & (xx < w)[None, :]
            tap = v[:, np.minimum(yy, h - 1)[:, None], np.minimum(xx, w - 1)[None, :]]
            r = np.where(inside[None], (r + wx[b][None, None, :] * tap).astype(ft), r)   # an outside tap adds nothing
        acc = (acc + wy[a][None, :, None] * r).astype(ft)
    m, s = np.asarray(mean, f32).astype(ft), np.asarray(std, f32).astype(ft)
    out = (acc - m[:, None, None]) / s[:, None, None]
    return np.ascontiguousarray(out.transpose(1, 2, 0)).astype(ft)


def preprocess224_f32(img, Hp, Wp, RH, RW, top, left, S, mean, std, mutant=None):
    return preprocess224_formula(img, Hp, Wp, RH, RW, top, left, S, mean, std, f32, mutant)


def to_layout(px, Cp, dtype):
    """[.., 3] float32 pixels -> torch [.., Cp] of ``dtype`` with zero pad channels (bf16: RNE of the f32 value)"""
    t = torch.zeros(px.shape[:-1] + (Cp,), dtype=torch.float32)
    t[..., :3] = torch.from_numpy(np.array(px, dtype=f32))            # (a copy: the cached restatements are read-only)
    return t.to(dtype)


# ------------------------------------------------------------------------------------------------ (b) float64 ATen
def preprocess224_f64(img, Hp, Wp, RH, RW, top, left, S, mean, std):
    """[S, S, 3] float64: the reference model's preprocess_image_train on one image of a batch padded to (Hp, Wp)"""
    _, h, w = img.shape
    x = torch.zeros(1, 3, Hp, Wp, dtype=torch.float64)
    x[0, :, :h, :w] = torch.from_numpy(img.astype(np.float64)) / 255.0
    y = F.interpolate(x, size=(RH, RW), mode="bicubic", align_corners=False)[0, :, top:top + S, left:left + S]
    m = torch.from_numpy(np.asarray(mean, f32).astype(np.float64)).view(3, 1, 1)
    s = torch.from_numpy(np.asarray(std, f32).astype(np.float64)).view(3, 1, 1)
    return ((y - m) / s).permute(1, 2, 0).contiguous().numpy()


# ------------------------------------------------------------------------------------------------ (c) the bound
def bound224(img, Hp, Wp, RH, RW, top, left, S, std, out64):
    """[S, S, 3] float64: the distance allowed between (a) and (b) (module docstring)"""
    _, h, w = img.shape
    f64 = np.float64
    fy, iy, wy = _axis(S, top, f64(Hp) / f64(RH), f64, -0.75)
    fx, ix, wx = _axis(S, left, f64(Wp) / f64(RW), f64, -0.75)
    v = img.astype(f64) / 255.0
    vmax = float(v.max())
    swy, swx = np.abs(wy).sum(0), np.abs(wx).sum(0)                                  # [S]
    mag = np.zeros((3, S, S))                                                        # sum |wy| |wx| |v|
    for a in range(4):
        yy = np.clip(iy - 1 + a, 0, Hp - 1)
        for b in range(4):
            xx = np.clip(ix - 1 + b, 0, Wp - 1)
            inside = (yy < h)[:, None] & (xx < w)[None, :]
            tap = v[:, np.minimum(yy, h - 1)[:, None], np.minimum(xx, w - 1)[None, :]]
            mag += np.abs(wy[a])[None, :, None] * np.abs(wx[b])[None, None, :] * np.where(inside[None], tap, 0.0)
    coord = DW_SUM * U * vmax * ((3 * (np.abs(fy) + 0.5) + 1)[:, None] * swx[None, :] + (3 * (np.abs(fx) + 0.5) + 1)[None, :] * swy[:, None])
    weights = max(DW_C1, DW_C2) * U * vmax * 4 * (swx[None, :] + swy[:, None])
    sums = 1.001 * ACC_OPS * U * mag
    s = np.asarray(std, f32).astype(f64)[:, None, None]
    b = (coord[None] + weights[None] + sums) / s
    return b.transpose(1, 2, 0) + 2 * U * np.abs(out64) + 1e-12


# ------------------------------------------------------------------------------------------------ cases
def _c(name, images, pad, size=16, tags=()):
    RH, RW, top, left = geometry(pad[0], pad[1], size)
    return dict(name=name, images=list(images), pad=pad, size=size, RH=RH, RW=RW, top=top, left=left, tags=set(tags))


# (h, w) of each image, the padded batch (Hp, Wp), the crop size.  Every image fits its pad.
CASES224 = [
    _c("portrait", [(45, 30), (40, 31)], (45, 31), tags=["top"]),
    _c("landscape", [(31, 47), (33, 50)], (33, 50), tags=["left"]),
    _c("identity", [(16, 16), (12, 9), (1, 1)], (16, 16), tags=["identity"]),
    _c("upscale", [(9, 11), (11, 8)], (11, 11), tags=["upscale"]),
    # 5 rows in a 40-row pad: windows reach past row 4 (outside the image) and windows are clamped at row 39 (all outside);
    # 39 x 43 in the same pad: one window holds rows 37, 38 (image), 39 (pad) and 40 (clamped to 39)
    _c("short_in_tall_pad", [(5, 30), (39, 43)], (40, 44), tags=["border"]),
    _c("real_size", [(300, 200), (250, 190)], (300, 200), size=224, tags=["size224", "top"]),
    _c("batch_split", [(20, 24), (13, 17)] * 16 + [(20, 24)], (20, 24), tags=["split"]),
]
CP = [None, 3, 5, 16]               # None = VEC of the dtype (one 16-byte store); the others take the scalar store loop
HOST_EXTRA = [                      # host-only geometries of the size where the coordinate term dominates
    _c("host_300", [(280, 300)], (300, 320), size=64, tags=["left"]),
    _c("host_tall", [(333, 120)], (340, 128), size=32, tags=["top"]),
]


def case_images(case):
    return [seeded_image(h, w, 7919 * i + 100 * h + w) for i, (h, w) in enumerate(case["images"])]


def check_case_table():
    """every named class has a case (asserted by the host test)"""
    tags = set().union(*[c["tags"] for c in CASES224])
    assert {"top", "left", "identity", "upscale", "border", "size224", "split"} <= tags, tags
    by = {c["name"]: c for c in CASES224}
    assert by["portrait"]["top"] == 4 and by["portrait"]["left"] == 0
    assert by["landscape"]["left"] == 4 and by["landscape"]["top"] == 0
    c = by["identity"]
    assert c["pad"] == (c["size"], c["size"]) and (c["RH"], c["RW"], c["top"], c["left"]) == (c["size"], c["size"], 0, 0)
    c = by["upscale"]
    assert c["RH"] > c["pad"][0] and c["RW"] > c["pad"][1]
    c = by["batch_split"]
    assert len(c["images"]) == PRE_MAX + 1 and len(set(c["images"])) == 2
    c = by["short_in_tall_pad"]
    Hp, S = c["pad"][0], c["size"]
    _, iy, _ = _axis(S, c["top"], np.float64(Hp) / c["RH"], np.float64, -0.75)
    rows = iy[:, None] - 1 + np.arange(4)[None]
    h0, h1 = c["images"][0][0], c["images"][1][0]
    assert ((rows.min(1) < h0) & (rows.max(1) >= h0)).any() and (rows.max(1) > Hp - 1).any() and (rows.min(1) < 0).any()
    assert ((rows.min(1) < h1) & (np.clip(rows, 0, Hp - 1).max(1) >= h1) & (rows.max(1) > Hp - 1)).any()   # image, pad and clamp at once
    assert by["real_size"]["size"] == 224 and all(c["size"] == 16 for c in CASES224 if c["name"] != "real_size")
    assert CP[0] is None and set(CP[1:]) == {3, 5, 16}
    for c in CASES224 + HOST_EXTRA:
        assert all(h <= c["pad"][0] and w <= c["pad"][1] for h, w in c["images"])
        assert c["top"] + c["size"] <= c["RH"] and c["left"] + c["size"] <= c["RW"]
