"""Pillow's bilinear coefficient tables (ImagingResample, 8 bits per channel) on the host: numpy only.  The kernels that resize on the
device (``cddmsl_tta_view``, ``cddmsl_resize_batch_u8``) only read these tables.  Importing this module loads neither the HIP
library nor anything of the GPU runtime, so a loader worker process can build the tables of its samples."""
import math

import numpy as np

RESAMPLE_BITS = 22          # Pillow's PRECISION_BITS (ImagingResample, 8 bits per channel)
_resample_cache = {}


def resample_table(insize, outsize):
    """Pillow's ``precompute_coeffs`` + ``normalize_coeffs_8bpc`` for the bilinear filter along one axis -> (lo [out], n [out],
    k [out, ksize], ksize), int32: output i reads inputs lo[i] .. lo[i] + n[i] - 1 with the weights k[i, :n[i]] (the rest 0).  Computed in
    double in Pillow's own order of operations -- window from the centre, triangle weight of ``(x + lo - centre + 0.5) * (1 / fs)``, a
    running sum in tap order, one division per tap, ``int(0.5 + w * 2^22)`` -- because another order moves a coefficient by one and
    with it pixels.  The kernel only reads these tables."""
    key = (int(insize), int(outsize))
    if key in _resample_cache:
        return _resample_cache[key]
    scale = key[0] / key[1]
    fs = max(scale, 1.0)
    support = 1.0 * fs                                   # the bilinear filter's support is 1
    ks = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / fs
    center = (np.arange(key[1], dtype=np.float64) + 0.5) * scale
    lo = np.maximum(np.trunc(center - support + 0.5).astype(np.int64), 0)
    hi = np.minimum(np.trunc(center + support + 0.5).astype(np.int64), key[0])
    n = hi - lo
    k = np.zeros((key[1], ks), dtype=np.float64)
    ww = np.zeros(key[1], dtype=np.float64)
    for t in range(ks):
        a = np.abs(((t + lo) - center + 0.5) * ss)
        k[:, t] = np.where((a < 1.0) & (t < n), 1.0 - a, 0.0)
        ww = ww + k[:, t]
    nz = ww != 0.0
    k[nz] = k[nz] / ww[nz, None]
    ki = np.trunc(0.5 + k * float(1 << RESAMPLE_BITS)).astype(np.int32)       # bilinear weights are never negative
    if len(_resample_cache) >= 256:
        _resample_cache.clear()
    _resample_cache[key] = (lo.astype(np.int32), n.astype(np.int32), ki, ks)
    return _resample_cache[key]


def packed_table(insize, outsize):
    """the table of one axis as the kernels' table buffer holds it: (int32 [out * (2 + ksize)] = lo | n | k row-major, ksize)"""
    lo, n, k, ks = resample_table(insize, outsize)
    return np.concatenate([lo, n, k.reshape(-1)]), ks
