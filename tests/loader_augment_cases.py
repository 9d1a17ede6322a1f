"""Batches for ``cddmsl_resize_batch_u8`` with the flip BIT SET (bit 0 mirrors columns, bit 1 rows) and what it must write (imported by
tests/test_gpu_loader_augment.py; not a conftest; numpy only).  Shapes, layout and the sentinel check are those of
tests/loader_resize_cases.py; only the expectation is recomputed here, since ``loader_resize_cases.expected`` knows left-right alone."""
import numpy as np

import loader_resize_cases as C
import pil_resize_ref as PR

# the smallest shapes at which the row mirror alone can go wrong -- (in (h, w), out (newh, neww)):
#   newh = 1: the mirror is the identity;  newh = 17 = TH + 1: the second tile's single row lands on row 0 (and the first tile's rows
#   on 1..16);  an identity-size item: no tables, the copy branch
ROW_EDGES = [((9, 12), (1, 7)), ((40, 30), (17, 21)), ((12, 20), (12, 20))]
ALL_SHAPES = list(C.ALL_SHAPES) + ROW_EDGES


def expected(img, newh, neww, code, reverse_channels):
    """uint8 [h, w, 3] -> uint8 [3, newh, neww]: Pillow's resize, then the mirrors the code's bits ask for"""
    v = PR.resize(img, newh, neww)
    if code & 1:
        v = v[:, ::-1]
    if code & 2:
        v = v[::-1]
    if reverse_channels:
        v = v[:, :, ::-1]
    return np.ascontiguousarray(v.transpose(2, 0, 1))


def all_shapes_cases(rot):
    """[(image, (newh, neww), code, reverse_channels)]: item i carries flip code (i + rot) % 4, reverse_channels on every third"""
    return [(PR.seeded_image(h, w, 300 + i), (nh, nw), (i + rot) % 4, i % 3 == 2) for i, ((h, w), (nh, nw)) in enumerate(ALL_SHAPES)]


def store_edge_cases(rot):
    return [(PR.seeded_image(h, w, 400 + i), (nh, nw), (i + rot) % 4, i % 3 == 1) for i, ((h, w), (nh, nw), _) in enumerate(C.STORE_EDGES)]


def build(cases, dst_shift=None):
    """``loader_resize_cases.build`` (the code rides in the item's flip field as it is) with the expectations recomputed"""
    b = C.build(cases, dst_shift)
    assert [it[6] for it in b["items"]] == [c[2] for c in cases]
    b["want"] = [(off, expected(img, nh, nw, code, rev)) for (off, _), (img, (nh, nw), code, rev) in zip(b["want"], cases)]
    return b
