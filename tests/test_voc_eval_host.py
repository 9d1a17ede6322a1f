"""Host half of the VOC evaluation on the GPU matcher (CPU only): the case sets of tests/voc_match_cases.py hit every rule of
``class_ap``'s walk; the rounding emulation IS the reference's text round trip; ``voc_accumulate`` fed with the host walk's flags is
EXACTLY ``class_ap``; the VOC-family catalog (cddmsl_amd/voc_catalog.py), the multi-set training dicts and how
``run_eval_only_catalog`` treats the VOC config's names; the evaluator without ``device`` returns what it always returned."""
import os

import numpy as np
import pytest

import voc_match_cases as C

SEEDS = (0, 1, 2)


def _walk(seed):
    def run():
        count = {k: 0 for k in C.COUNTERS}
        case = C.random_set(seed)
        return C.instrumented_walk(case, count), count
    return C.cached(("walk", seed), run)


def test_case_sets_hit_every_rule():
    total = {k: 0 for k in C.COUNTERS}
    for seed in SEEDS:
        _, count = _walk(seed)
        print(f"seed {seed}: {count}")
        for k, v in count.items():
            total[k] += v
    assert all(total[k] >= 5 for k in C.COUNTERS), total
    case = C.random_set(0)
    _, _, cls, _ = C.flat_dets(case)
    assert not (cls == C.GT_ONLY).any() and any(o[0] == C.GT_ONLY for objs in case["gt"] for o in objs)       # a class with no detections at all
    assert (cls == C.DT_ONLY).any() and not any(o[0] == C.DT_ONLY for objs in case["gt"] for o in objs)       # a class without positives


def test_rounding_is_the_text_round_trip():
    """``voc_round_boxes`` / ``voc_round_scores`` (and the kernel, which does the same operations) against ``float(f"{v:.1f}")`` /
    ``float(f"{s:.3f}")`` on sampled f32 values and on constructed ties"""
    from cddmsl_amd import evaluation as E
    rng = np.random.RandomState(7)
    ties1 = (np.arange(-400, 4000, dtype=np.float64) / 4.0).astype(np.float32)                   # x.25 / x.75: times 10 ends in .5
    near1 = np.nextafter(ties1, np.float32(np.inf)), np.nextafter(ties1, np.float32(-np.inf))
    v = np.concatenate([rng.uniform(-50, 1400, 100000).astype(np.float32), rng.uniform(-1, 1, 5000).astype(np.float32), ties1, *near1,
                        np.array([0.0, -0.0, 0.04, -0.04, 0.05, -0.05, 1e-30, 16777216.0, 3.0e38, np.inf, -np.inf], dtype=np.float32)])
    assert len(v) >= 100000
    b = np.stack([v, v, v, v], axis=1)
    got = E.voc_round_boxes(b)
    lo = np.array([float(f"{x + 1:.1f}") for x in v])            # x is an np.float32: the + 1 is an f32 addition, as in process()
    hi = np.array([float(f"{x:.1f}") for x in v])
    assert np.array_equal(got[:, 0], lo) and np.array_equal(got[:, 1], lo) and np.array_equal(got[:, 2], hi) and np.array_equal(got[:, 3], hi)
    assert np.array_equal(np.signbit(got[:, 2]), np.signbit(hi))                                 # "-0.0" reads back as -0.0
    ties3 = (np.arange(0, 17, dtype=np.float64) / 16.0).astype(np.float32)                       # odd sixteenths: times 1000 ends in .5
    s = np.concatenate([rng.uniform(0, 1, 100000).astype(np.float32), ties3, np.nextafter(ties3, np.float32(2)), np.nextafter(ties3, np.float32(-1)),
                        (np.arange(0, 2001, dtype=np.float64) / 2000.0).astype(np.float32)])
    want = np.array([float(f"{x:.3f}") for x in s.tolist()])     # process() formats the Python float of the f32
    assert np.array_equal(E.voc_round_scores(s), want)
    assert np.isnan(E.voc_round_scores(np.array([np.nan], dtype=np.float32))[0]) and np.isnan(float(f"{float('nan'):.3f}"))


@pytest.mark.parametrize("use_07", [True, False])
@pytest.mark.parametrize("seed", SEEDS)
def test_accumulate_equals_class_ap(seed, use_07):
    from cddmsl_amd import evaluation as E
    case = C.random_set(seed)
    (tpb, fpb), _ = _walk(seed)
    ref = C.cached(("aps", seed, use_07), lambda: C.class_aps(case, use_07))
    _, s, cls, img = C.flat_dets(case)
    ranked, perm, seg_off, seg_gt = E.voc_segments(cls, img, E.voc_round_scores(s), range(C.NUM_CLASSES), len(case["names"]))
    gts = C.gt_by_class(case)
    nan_classes = 0
    with np.errstate(invalid="ignore", divide="ignore"):
        for k in range(C.NUM_CLASSES):
            npos = sum(int((~d).sum()) for _, d in gts[k].values())
            got = E.voc_accumulate(tpb[ranked[k]], fpb[ranked[k]], npos, use_07)
            assert len(got) == 10
            for g, r in zip(got, ref[k]):
                assert g == r or (g != g and r != r), (k, g, r)
            nan_classes += int(any(r != r for r in ref[k]))
    assert (nan_classes > 0) == (not use_07)           # the class without positives: NaN with the 2012 metric, 0 with the 11-point one
    assert any(0 < r < 1 for row in ref for r in row)
    # the segments: a permutation of the evaluated detections, every (class, image) once, rank order kept inside a segment
    assert sorted(perm.tolist()) == list(range(len(s))) and len(set(seg_gt.tolist())) == len(seg_gt) and seg_off[-1] == len(perm)
    pos = {int(d): i for k in ranked for i, d in enumerate(ranked[k])}
    for a, b_, row in zip(seg_off[:-1], seg_off[1:], seg_gt):
        seg = perm[a:b_]
        assert b_ > a and (cls[seg] == row // len(case["names"])).all() and (img[seg] == row % len(case["names"])).all()
        assert [pos[int(d)] for d in seg] == sorted(pos[int(d)] for d in seg)


# ------------------------------------------------------------------------------------------------ the catalog
TABLE = {
    "voc_2007_trainval": ("VOC2007", "trainval", 2007, None), "voc_2007_train": ("VOC2007", "train", 2007, None),
    "voc_2007_val": ("VOC2007", "val", 2007, None), "voc_2007_test": ("VOC2007", "test", 2007, None),
    "voc_2012_trainval": ("VOC2012", "trainval", 2012, None), "voc_2012_train": ("VOC2012", "train", 2012, None),
    "voc_2012_val": ("VOC2012", "val", 2012, None),
    "voc_clipart_2007_trainval": ("VOC2007", "trainval", 2007, "dt_clipart"), "voc_clipart_2007_train": ("VOC2007", "train", 2007, "dt_clipart"),
    "voc_clipart_2012_trainval": ("VOC2012", "trainval", 2012, "dt_clipart"), "voc_clipart_2012_train": ("VOC2012", "train", 2012, "dt_clipart"),
    "voc_watercolor_2007_trainval": ("VOC2007", "trainval", 2007, "dt_watercolor"), "voc_watercolor_2007_train": ("VOC2007", "train", 2007, "dt_watercolor"),
    "voc_watercolor_2012_trainval": ("VOC2012", "trainval", 2012, "dt_watercolor"), "voc_watercolor_2012_train": ("VOC2012", "train", 2012, "dt_watercolor"),
    "voc_comic_2007_trainval": ("VOC2007", "trainval", 2007, "dt_comic"), "voc_comic_2007_train": ("VOC2007", "train", 2007, "dt_comic"),
    "voc_comic_2012_trainval": ("VOC2012", "trainval", 2012, "dt_comic"), "voc_comic_2012_train": ("VOC2012", "train", 2012, "dt_comic"),
    "Clipart1k_train": ("clipart", "train", 2012, None), "Clipart1k_test": ("clipart", "test", 2012, None),
    "dt_Clipart_2007_trainval": ("dt_clipart/VOC2007", "trainval", 2012, None), "dt_Clipart_2012_trainval": ("dt_clipart/VOC2012", "trainval", 2012, None),
    "Watercolor_train": ("watercolor", "train", 2012, None), "Watercolor_test": ("watercolor", "test", 2012, None),
    "Comic_train": ("comic", "train", 2012, None), "Comic_test": ("comic", "test", 2012, None),
}


def test_catalog_table():
    from cddmsl_amd import voc_catalog as V
    assert sorted(V.ENTRIES) == sorted(TABLE)
    for name, (rel, split, year, dt) in TABLE.items():
        assert V.is_voc_family(name)
        assert V.voc_entry(name, "/d") == ("/d/" + rel, split, year, dt), name
    for other in ("cityscapes_DG_train", "cityscapes_val", "cityscapes_foggy_val", "bdd_100k_val", "voc_2012_test", "no_such_set"):
        assert not V.is_voc_family(other)
    with pytest.raises(KeyError):
        V.voc_entry("bdd_100k_val", "/d")


def test_load_voc_family_and_concatenation(tmp_path):
    from cddmsl_amd import voc_catalog as V
    root = str(tmp_path)
    cases = C.write_family(root)
    a = V.load_voc_family("voc_clipart_2007_trainval", root)
    assert [d["image_id"] for d in a] == cases["VOC2007"]["names"]
    assert [d["file_name"] for d in a] == [f"{root}/VOC2007/JPEGImages/{n}.jpg" for n in cases["VOC2007"]["names"]]
    assert [d["data_dt_file_name"] for d in a] == [f"{root}/VOC2007/../dt_clipart/VOC2007/JPEGImages/{n}.jpg" for n in cases["VOC2007"]["names"]]
    assert all(os.path.exists(d["data_dt_file_name"]) for d in a)
    for d, objs in zip(a, cases["VOC2007"]["gt"]):
        assert [(x["category_id"], x["bbox"]) for x in d["annotations"]] == [(c, [b[0] - 1.0, b[1] - 1.0, float(b[2]), float(b[3])]) for c, _, b in objs]
    assert V.load_voc_family("voc_clipart_2007_trainval", root) is a                         # parsed once per (name, root)
    assert "data_dt_file_name" not in V.load_voc_family("voc_2007_trainval", root)[0]
    both = V.load_train_sets(("voc_clipart_2007_trainval", "voc_clipart_2012_trainval"), root)
    assert [d["image_id"] for d in both] == cases["VOC2007"]["names"] + cases["VOC2012"]["names"]
    assert [d["data_dt_file_name"] for d in both[3:]] == [f"{root}/VOC2012/../dt_clipart/VOC2012/JPEGImages/{n}.jpg" for n in cases["VOC2012"]["names"]]
    swapped = V.load_train_sets(("voc_clipart_2012_trainval", "voc_clipart_2007_trainval"), root)
    assert [d["image_id"] for d in swapped] == cases["VOC2012"]["names"] + cases["VOC2007"]["names"]
    # FILTER_EMPTY_ANNOTATIONS drops an image without annotations, and only with the switch on
    anno = os.path.join(root, "VOC2012", "Annotations", cases["VOC2012"]["names"][1] + ".xml")
    with open(anno) as f:
        text = f.read()
    with open(anno, "w") as f:
        f.write(text[: text.index("<object>")] + "</annotation>")
    V._CACHE.clear()
    names = cases["VOC2012"]["names"]
    assert [d["image_id"] for d in V.load_train_sets(("voc_clipart_2012_trainval",), root, True)] == [names[0], names[2]]
    assert [d["image_id"] for d in V.load_train_sets(("voc_clipart_2012_trainval",), root, False)] == names
    with pytest.raises(ValueError, match="cityscapes_DG_train"):
        V.load_train_sets(("voc_clipart_2007_trainval", "cityscapes_DG_train"), root)
    with pytest.raises(FileNotFoundError, match="dt_comic/VOC2007/JPEGImages"):                # a DG name without its twins: at start-up
        V.load_voc_family("voc_comic_2007_trainval", root)


def _cfg(tests):
    from cddmsl_amd.config import get_cfg
    cfg = get_cfg()
    cfg.merge_from_list(["DATASETS.TEST", tuple(tests), "MODEL.DEVICE", "cpu", "INPUT.MIN_SIZE_TEST", 128, "INPUT.MAX_SIZE_TEST", 160,
                         "MODEL.ROI_HEADS.NUM_CLASSES", 20])
    return cfg


def test_voc_names_skipped_when_the_image_set_is_missing(tmp_path, capsys):
    from cddmsl_amd import evaluation as E
    res = E.run_eval_only_catalog(object(), _cfg(["voc_2007_test", "Comic_test", "no_such_set"]), str(tmp_path), return_results=True, prefix="iter 4  ")
    out = capsys.readouterr().out
    assert res == {}
    assert f"iter 4  skipping voc_2007_test: {tmp_path}/VOC2007/ImageSets/Main/test.txt not found" in out
    assert f"iter 4  skipping Comic_test: {tmp_path}/comic/ImageSets/Main/test.txt not found" in out
    assert "skipping no_such_set: not in the dataset catalog" in out


def _stub_model(cases):
    import torch
    from cddmsl_amd.structures import Boxes, Instances
    dets = {n: d for case in cases for n, d in zip(case["names"], case["dets"])}

    class Stub(torch.nn.Module):
        def forward(self, inputs):
            out = []
            for inp in inputs:
                b, s, c = dets[str(inp["image_id"])]
                out.append({"instances": Instances((128, 160), pred_boxes=Boxes(torch.from_numpy(b)), scores=torch.from_numpy(s), pred_classes=torch.from_numpy(c))})
            return out
    return Stub()


def test_catalog_evaluates_voc_names_on_the_host(tmp_path, capsys, monkeypatch):
    from cddmsl_amd import evaluation as E
    root = str(tmp_path)
    cases = C.write_family(root)
    cfg = _cfg(["voc_2007_test", "Clipart1k_test", "Watercolor_test"])
    model = _stub_model([cases["test"], cases["clipart"]])
    with np.errstate(invalid="ignore", divide="ignore"):
        res = E.run_eval_only_catalog(model, cfg, root, return_results=True)
    out = capsys.readouterr().out
    assert list(res) == ["voc_2007_test", "Clipart1k_test"] and "skipping Watercolor_test" in out
    assert "voc_2007_test: {'AP': " in out and "Clipart1k_test: {'AP': " in out
    for name, case, use_07 in (("voc_2007_test", cases["test"], True), ("Clipart1k_test", cases["clipart"], False)):
        bbox = res[name]["bbox"]
        assert list(bbox) == ["AP", "AP50", "AP75"] + ["AP50-" + n for n in E.VOC_CLASS_NAMES] + ["AP50-present", "AP-present"]
        aps = np.array(C.class_aps(case, use_07)) * 100                 # [K, T]
        present = sorted({o[0] for objs in case["gt"] for o in objs})
        assert bbox["AP50-present"] == float(np.mean(aps[present, 0])) and bbox["AP-present"] == float(np.mean([np.mean(aps[present, t]) for t in range(10)]))
        assert 0 < bbox["AP50-present"] <= 100
    assert not np.isnan(res["voc_2007_test"]["bbox"]["AP"])             # 11-point metric: a class without positives counts 0
    monkeypatch.setattr(E, "num_test_classes", lambda model, cfg: 8)
    with pytest.raises(ValueError, match=r"20 classes.*\b8\b"):
        E.run_eval_only_catalog(model, cfg, root)


@pytest.mark.parametrize("year", [2007, 2012])
def test_host_evaluator_unchanged_without_device(tmp_path, year):
    """``device=None`` (and a CPU device) is the evaluator as it was: text lines, ``class_ap``; the keys it had keep their values"""
    from cddmsl_amd import evaluation as E
    case = C.random_set(1)
    C.write_voc_tree(str(tmp_path), "test", case, E.VOC_CLASS_NAMES)
    res = []
    for dev in (None, "cpu"):
        ev = E.PascalVOCDetectionEvaluator(str(tmp_path), "test", year, device=dev)
        assert ev.device is None
        for inputs, outputs in C.instances_of(case):
            ev.process(inputs, outputs)
        with np.errstate(invalid="ignore", divide="ignore"):
            res.append(ev.evaluate())
            again = ev.evaluate()                                           # the ground truth is cached: same answer
        assert C.same_results(res[-1], again)
    assert C.same_results(res[0], res[1])
    aps = C.cached(("aps", 1, year == 2007), lambda: C.class_aps(case, year == 2007))
    aps = {t: [a[i] * 100 for a in aps] for i, t in enumerate(C.THRS)}      # what evaluate() did before: per threshold a list over classes
    mean = {t: float(np.mean(v)) for t, v in aps.items()}
    old = {"AP": float(np.mean(list(mean.values()))), "AP50": mean[50], "AP75": mean[75]}
    old.update({"AP50-" + n: aps[50][i] for i, n in enumerate(E.VOC_CLASS_NAMES)})
    got = res[0]["bbox"]
    assert list(got)[: len(old)] == list(old)
    assert C.same_results({"bbox": {k: got[k] for k in old}}, {"bbox": old})
    assert np.isnan(got["AP"]) == (year == 2012) and not np.isnan(got["AP-present"]) and not np.isnan(got["AP50-present"])
