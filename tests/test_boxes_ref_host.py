"""The numpy references of tests/exact_boxes.py against the CPU oracle and torch on EVERY case of every builder (this is what makes them
fit to judge the kernels of cddmsl_amd/csrc/boxes.hip in tests/test_gpu_boxes_exact.py), a census of the cases (they contain what
they were built to contain), and a negative control: an NMS decision without the division disagrees on every class-a pair."""
from fractions import Fraction

import numpy as np
import pytest
import torch

import exact_boxes as E
from oracle import ops as oo

NMS = {c["name"]: c for c in E.nms_cases()}
THRS = (0.3, 0.5, 0.7)


def _oracle_keep(c, img):
    """oracle NMS on the valid candidates with strictly descending scores, mapped back to positions, cut at max_keep"""
    pos = np.nonzero(c["valid"][img] == 1)[0]
    b = torch.from_numpy(c["boxes"][img][pos])
    k = oo.nms(b, -torch.arange(len(pos), dtype=torch.float32), c["thr"]).numpy()
    return pos[k][:c["max_keep"]].astype(np.int32)


@pytest.mark.parametrize("name", list(NMS))
def test_nms_reference_equals_the_oracle(name):
    c = NMS[name]
    for img in range(c["boxes"].shape[0]):
        assert np.array_equal(E.nms_ref(c["boxes"][img], c["valid"][img], c["thr"], c["max_keep"]), _oracle_keep(c, img)), (name, img)


@pytest.mark.parametrize("name", list(NMS))
def test_anyorder_reference_equals_the_oracle(name):
    boxes, scores = E.anyorder_inputs(NMS[name])
    got = E.anyorder_ref(boxes, scores, NMS[name]["thr"])
    assert np.array_equal(got, oo.nms(torch.from_numpy(boxes), torch.from_numpy(scores), NMS[name]["thr"]).numpy())


@pytest.mark.parametrize("c", E.match_cases(), ids=lambda c: c["name"])
def test_matcher_reference_equals_the_oracle(c):
    m, l = E.matcher_ref(c["gt"], c["preds"], c["thresholds"], c["labels"], c["allow_low_quality"])
    q = oo.pairwise_iou(torch.from_numpy(c["gt"]), torch.from_numpy(c["preds"]))
    om, ol = oo.matcher(q, list(c["thresholds"]), list(c["labels"]), c["allow_low_quality"])
    assert m.dtype == np.int64 and l.dtype == np.int8
    assert np.array_equal(m, om.numpy()) and np.array_equal(l, ol.numpy())


@pytest.mark.parametrize("c", E.match_batched_cases(), ids=lambda c: c["name"])
def test_batched_matcher_reference_equals_the_oracle(c):
    m, l = E.matcher_ref_batched(c["gts"], c["preds"], c["counts"], c["thresholds"], c["labels"], c["allow_low_quality"])
    off = 0
    for n, g in enumerate(c["gts"]):
        cnt = len(c["preds"]) if c["counts"] is None else c["counts"][n]
        p = c["preds"] if c["counts"] is None else c["preds"][off:off + cnt]
        om, ol = oo.matcher(oo.pairwise_iou(torch.from_numpy(g), torch.from_numpy(p)), list(c["thresholds"]), list(c["labels"]),
                            c["allow_low_quality"])
        gm, gl = (m[n], l[n]) if c["counts"] is None else (m[off:off + cnt], l[off:off + cnt])
        off += 0 if c["counts"] is None else cnt
        assert np.array_equal(gm, om.numpy()) and np.array_equal(gl, ol.numpy()), n


@pytest.mark.parametrize("c", E.sort_cases(), ids=lambda c: c["name"])
def test_sort_reference_equals_torch(c):
    s = torch.sort(torch.from_numpy(c["keys"]), descending=True, dim=1, stable=True)
    assert np.array_equal(E.sort_ref(c["keys"]), s.indices.numpy().astype(np.int32))


def test_sort_signed_zero_row():
    """+0.0 and -0.0 are equal scores: the lower index first"""
    assert E.sort_ref(E.sort_cases()[0]["keys"]).tolist() == [[2, 0, 1, 3, 4, 5]]


def test_sort_census():
    cs = E.sort_cases()
    assert {c["keys"].shape[0] for c in cs} == {1, 2, 3, 5, 16, 17}
    assert {c["keys"].shape[1] for c in cs} >= {1, 255, 256, 257, 1000}
    allk = np.concatenate([c["keys"].ravel() for c in cs])
    bits = allk.view(np.uint32)
    assert (bits == 0).any() and (bits == 0x80000000).any() and np.isposinf(allk).any() and np.isneginf(allk).any()
    assert ((bits & 0x7f800000) == 0)[(bits & 0x007fffff) != 0].any(), "no subnormal key"
    assert any((c["keys"] == c["keys"][:, :1]).all() and c["keys"].shape[1] > 1 for c in cs), "no row of equal keys"


# ------------------------------------------------------------------------------------------------------------------ census, NMS
@pytest.mark.parametrize("k", E.DENSE_KEPT)
def test_dense_chunk_keeps_exactly_k(k):
    c = NMS[f"dense_keep{k}"]
    keep = E.nms_ref(c["boxes"][0], c["valid"][0], c["thr"], c["max_keep"])
    assert keep[keep < 64].tolist() == E.dense_slots(k) and len(E.dense_slots(k)) == k
    if k > 1:
        assert 63 in keep                                     # the walk's last bit
    # every candidate of chunk 1 is decided by exactly one row of chunk 0: removed where that row was kept
    assert sorted(set(range(64)) - set((keep[(keep >= 64) & (keep < 128)] - 64).tolist())) == E.dense_slots(k)
    assert not (keep >= 128).any()


def test_ladder_alternates_across_both_chunk_boundaries():
    c = NMS["ladder_odd"]
    keep = set(E.nms_ref(c["boxes"][0], c["valid"][0], c["thr"], 200).tolist())
    assert keep == {0} | set(range(1, 200, 2))
    assert {63, 65, 127, 129} <= keep and not ({64, 128} & keep)      # 63 removes 64, so 64 does not remove 65
    c = NMS["ladder_even"]
    assert set(E.nms_ref(c["boxes"][0], c["valid"][0], c["thr"], 200).tolist()) == set(range(0, 200, 2))


def test_nms_census():
    assert {c["boxes"].shape[1] for c in E.nms_cases()} >= {1, 63, 64, 65, 127, 128, 129, 327}
    assert {c["thr"] for c in E.nms_cases()} == set(THRS)
    big = NMS["clustered_3x327_thr0.5"]["boxes"]
    assert big.shape[0] == 3 and not np.array_equal(big[0], big[1]) and not np.array_equal(big[1], big[2])
    assert set(np.unique(NMS["valid_0_1_2_3x327"]["valid"])) == {0, 1, 2} and not NMS["valid_all_0_n129"]["valid"].any()
    for n in (129, 327):
        full = NMS[f"max_keep{n}_n{n}"]
        c0 = E.kept_in_chunk0(full)
        total = len(E.nms_ref(full["boxes"][0], full["valid"][0], full["thr"], n))
        assert 1 < c0 < total < n                              # max_keep = n is larger than the number of survivors
        assert {f"max_keep{m}_n{n}" for m in (1, c0, c0 + 1, n)} <= set(NMS)
    d = NMS["degenerate_n100"]["boxes"][0]
    assert (d[:, 2] == d[:, 0]).any() and (d[:, 3] == d[:, 1]).any() and (d[:, 2] < d[:, 0]).any()


@pytest.mark.parametrize("name", [n for n in NMS if not n.startswith("degenerate")])
def test_grid_cases_are_exact_in_f32(name):
    """only the division rounds: every other intermediate equals its float64 value, for every pair of the case"""
    for b in NMS[name]["boxes"]:
        assert E.grid_exact(b), name


# ------------------------------------------------------------------------------------------------------------------ threshold pairs
@pytest.mark.parametrize("thr", THRS)
def test_threshold_classes(thr):
    t = E.threshold_cases(thr)
    T = Fraction(float(np.float32(thr)))
    for cls in "abc":
        if cls == "a" and thr in E.CLASS_A_IMPOSSIBLE:
            # no f32 inputs exist (see threshold_cases): the smallest quotient above one half that two f32 values can have
            assert len(t[cls]) == 0 and np.float32(np.nextafter(np.float32(0.5), np.float32(1))) / np.float32(1) > np.float32(0.5)
            continue
        assert len(t[cls]) >= 8, (thr, cls, len(t[cls]))
        assert E.grid_exact(E.spread(t[cls]).reshape(-1, 4))
        for A, B in t[cls]:
            inter, u = E.pair_exact(A, B)
            q = bool(np.float32(float(inter)) / np.float32(float(u)) > np.float32(thr))      # inter, u exact in f32 (grid_exact)
            r = inter - T * u
            if cls == "a":
                assert inter / u > T and not q and inter / u - T <= E.NEAR
            elif cls == "b":
                assert 0 < r < Fraction(2.0e-7) * u and q and inter / u - T <= E.NEAR
            else:
                assert inter / u <= T and not q
            keep = E.nms_ref(np.stack([A, B]), [1, 1], thr, 2)
            assert keep.tolist() == ([0] if cls == "b" else [0, 1])
    if thr == 0.7:
        assert E.pair_exact(*t["a"][0]) == (700, 1000)
    if thr == 0.5:
        i, u = E.pair_exact(*t["c"][0])
        assert 2 * i == u


@pytest.mark.parametrize("thr", [t for t in THRS if t not in E.CLASS_A_IMPOSSIBLE])
def test_a_decision_without_the_division_fails_every_class_a_pair(thr):
    """the negative control: these pairs can see the bug they are there for"""
    for A, B in E.threshold_cases(thr)["a"]:
        p = np.stack([A, B])
        assert E.nms_ref(p, [1, 1], thr, 2, over=E.over_without_division).tolist() == [0]
        assert E.nms_ref(p, [1, 1], thr, 2).tolist() == [0, 1]
    for cls in "bc":                                            # ... and agrees elsewhere: it is the band alone that tells them apart
        for A, B in E.threshold_cases(thr)[cls]:
            p = np.stack([A, B])
            assert np.array_equal(E.nms_ref(p, [1, 1], thr, 2, over=E.over_without_division), E.nms_ref(p, [1, 1], thr, 2))


def test_near_threshold_census():
    """the witness's description of the cases: the threshold cases are near-threshold, the clustered ones are not only that"""
    for thr in THRS:
        clear, near = E.classify_pairs(NMS[f"threshold_b_thr{thr}"]["boxes"][0], thr)
        assert near == 8 and clear == 0
    clear, near = E.classify_pairs(NMS["clustered_3x327_thr0.5"]["boxes"][0], 0.5)
    assert clear > 1000


# ------------------------------------------------------------------------------------------------------------------ matcher census
def test_match_census():
    M = {c["name"]: c for c in E.match_cases()}
    c = M["cut_points_roi_lq0"]
    v = E.iou_match32(c["gt"][0], c["preds"])
    assert v[1] == np.float32(0.5) and v[2] == np.float32(0.7) and v[0] == np.float32(0.3)
    _, lab = E.matcher_ref(c["gt"], c["preds"], c["thresholds"], c["labels"], False)
    assert lab[1] == 1                                        # IoU == 0.5f is not < 0.5: the upper label
    _, lab = E.matcher_ref(c["gt"], c["preds"], E.RPN_T, E.RPN_L, False)
    assert lab[2] == 1 and lab[0] == -1                       # RN(7/10) == 0.7f and RN(3/10) == 0.3f: the upper labels
    c = M["equal_iou_two_boxes"]
    assert E.matcher_ref(c["gt"], c["preds"], c["thresholds"], c["labels"], True)[0].tolist() == [0, 1, 1]
    c = M["tied_row_maximum"]
    assert E.matcher_ref(c["gt"], c["preds"], c["thresholds"], c["labels"], True)[1].tolist() == [1, 1, 1, 0, 1]
    c = M["box_without_overlap_lq1"]
    assert (E.matcher_ref(c["gt"], c["preds"], c["thresholds"], c["labels"], True)[1] == 1).all()
    assert {c["preds"].shape[0] for c in E.match_cases()} >= {255, 256, 257, 1023, 1024, 1025}
    assert {c["gt"].shape[0] for c in E.match_cases()} >= {0, 1, 300}
    b = {c["name"]: c for c in E.match_batched_cases()}["concatenated_lq1"]
    assert tuple(b["counts"]) == (0, 1, 255, 1025, 3000) and tuple(len(g) for g in b["gts"]) == (2, 0, 1, 0, 300)


# ------------------------------------------------------------------------------------------------------------------ decode
@pytest.mark.parametrize("c", E.decode_cases(), ids=lambda c: c["name"])
def test_decode_reference_and_conditions(c):
    d = E.decode_ref(c)
    fin = d["finite"]
    assert int((d["valid"] == 2).sum()) == 3 and not fin[d["valid"] == 2].any()
    assert np.isfinite(d["bound"][fin]).all()
    assert d["ambiguous"].mean() <= E.DECODE_SKIP_CAP                  # (no coordinate is ever excused)
    assert (d["valid"] == 0).any() and (d["valid"] == 1).any()
    total = c["Hf"] * c["Wf"] * c["A"]
    assert c["topk"] in (total, total - 1) and (c["img_hw"][:, 0] <= 16 * c["Hf"]).all() and (c["img_hw"][0] < (16 * c["Hf"], 16 * c["Wf"])).all()
    # the oracle's f32 path is an f32 evaluation of the same expression: it lies within the same bound (this checks the bound, and the
    # float64 reference, before they meet the kernel)
    anchors = torch.from_numpy(E.anchors_ref(c["cell"], c["Hf"], c["Wf"], c["stride"], c["offset"]).astype(np.float32))
    for n in range(2):
        sel = torch.from_numpy(c["order"][n, :c["topk"]].astype(np.int64))
        ob = oo.clip_boxes(oo.apply_deltas(torch.from_numpy(c["deltas"][n])[sel], anchors[sel], c["weights"], c["scale_clamp"]),
                           tuple(int(v) for v in c["img_hw"][n])).numpy().astype(np.float64)
        f = fin[n]
        assert (np.abs(ob[f] - d["boxes"][n][f]) <= d["bound"][n][f]).all()
        assert not np.isfinite(oo.apply_deltas(torch.from_numpy(c["deltas"][n])[sel], anchors[sel], c["weights"], c["scale_clamp"]).numpy()[~f]).all(1).any()
        ov = oo.nonempty(torch.from_numpy(ob), c["min_size"]).numpy()
        chk = f & ~d["ambiguous"][n]
        assert np.array_equal(ov[chk], d["valid"][n][chk] == 1)


def test_anchor_reference_equals_the_oracle():
    cell = E.cell_anchors()
    assert np.array_equal(cell, oo.cell_anchors().numpy())
    for Hf, Wf, off in ((5, 7, 0.0), (12, 17, 0.5)):
        assert np.array_equal(E.anchors_ref(cell, Hf, Wf, 16.0, off).astype(np.float32), oo.grid_anchors(Hf, Wf, 16, off).numpy())
