"""Batches for ``cddmsl_resize_batch_u8`` and what it must write (imported by tests/test_gpu_loader_resize.py and
tests/test_loader_resize_host.py; not a conftest; numpy only).  The expected bytes come from tests/pil_resize_ref.py -- the restatement
tests/test_tta_host.py ties to the installed Pillow -- so the kernel tests do not depend on the Pillow of the GPU box; the tables the
kernel reads come from the product (cddmsl_amd/resample.py), as in the loader."""
import numpy as np

import pil_resize_ref as PR

SENTINEL = 0xA5

# test 1: every shape class in one launch -- PR.PAIRS (up / down / one axis kept / identity / ksize 9), several tiles per axis at a
# non-integer ratio, and a vertical ratio of 10 whose rows do not fit the LDS buffer (the recompute path)
ALL_SHAPES = list(PR.PAIRS) + [((150, 210), (97, 136)), ((200, 40), (20, 30))]

# test 2: output widths 1, 2, 3, 5, 63, 64, 65, 67 -- (in (h, w), out (newh, neww), flip)
STORE_EDGES = [((8, 8), (8, 1), False), ((16, 9), (7, 3), False), ((9, 4), (9, 2), False), ((11, 10), (6, 5), False),
               ((20, 70), (10, 63), False), ((12, 64), (12, 64), True), ((20, 70), (10, 65), False), ((12, 130), (12, 67), False)]


def expected(img, newh, neww, flip, reverse_channels):
    """uint8 [h, w, 3] -> what the loader's host path makes of it: uint8 [3, newh, neww]"""
    v = PR.resize(img, newh, neww)
    if flip:
        v = v[:, ::-1]
    if reverse_channels:
        v = v[:, :, ::-1]
    return np.ascontiguousarray(v.transpose(2, 0, 1))


def all_shapes_cases():
    """[(image, (newh, neww), flip, reverse_channels)]: flip alternates, reverse_channels on every third, and the last item repeats
    the first item's sizes with another picture (an image and its twin: one table set for both)"""
    shapes = ALL_SHAPES + [ALL_SHAPES[0]]
    return [(PR.seeded_image(h, w, 100 + i), (nh, nw), bool(i % 2), i % 3 == 2) for i, ((h, w), (nh, nw)) in enumerate(shapes)]


def store_edge_cases():
    return [(PR.seeded_image(h, w, 200 + i), (nh, nw), flip, i % 3 == 1) for i, ((h, w), (nh, nw), flip) in enumerate(STORE_EDGES)]


def build(cases, dst_shift=None):
    """-> dict(src uint8 [S], tab int32 [T], items [12-tuples of hip.resize_batch_u8], dst_bytes, want [(dst_off, uint8 [3, newh, neww])]).
    Sources and results sit in 256-byte slots as DeviceBatches lays them out; ``dst_shift[i]`` moves result i inside its slot (the
    slot grows by one unit), so that row starts fall on every residue modulo 4.  Tables are shared by (insize, outsize)."""
    from cddmsl_amd.resample import packed_table
    src, tabs, where, items, want = [], [], {}, [], []
    s_off = d_off = t_off = 0

    def table(insize, outsize):
        nonlocal t_off
        if insize == outsize:
            return -1, 0
        if (insize, outsize) not in where:
            t, ks = packed_table(insize, outsize)
            where[(insize, outsize)] = (t_off, ks)
            tabs.append(t)
            t_off += len(t)
        return where[(insize, outsize)]

    for i, (img, (nh, nw), flip, rev) in enumerate(cases):
        h, w = img.shape[:2]
        shift = dst_shift[i] if dst_shift else 0
        pad = (-img.size) % 256
        src.append(np.concatenate([img.reshape(-1), np.zeros(pad, np.uint8)]))
        items.append((s_off, d_off + shift, h, w, nh, nw, int(flip), int(rev), *table(w, nw), *table(h, nh)))
        want.append((d_off + shift, expected(img, nh, nw, flip, rev)))
        s_off += img.size + pad
        d_off += (3 * nh * nw + shift + 255) // 256 * 256
    return {"src": np.concatenate(src), "tab": np.concatenate(tabs).astype(np.int32) if tabs else np.zeros(0, np.int32), "items": items,
            "dst_bytes": d_off + 256, "want": want}                       # (one more slot behind the last: it must stay untouched)


def check(dst, want):
    """every result equals its expectation and every other byte of ``dst`` (uint8 [dst_bytes]) still holds the sentinel"""
    untouched = np.ones(len(dst), bool)
    for n, (off, v) in enumerate(want):
        got = dst[off:off + v.size].reshape(v.shape)
        assert np.array_equal(got, v), (n, v.shape, int((got != v).sum()), np.argwhere(got != v)[:4].tolist())
        untouched[off:off + v.size] = False
    assert (dst[untouched] == SENTINEL).all(), np.flatnonzero(untouched & (dst != SENTINEL))[:8].tolist()
