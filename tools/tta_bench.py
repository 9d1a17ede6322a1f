#!/usr/bin/env python
"""Test-time augmentation: what making the views costs, on one seeded 800x1333 image with the default TEST.AUG (nine short edges
400..1200 and the mirror of each: 18 views, batches of three).  Medians over ``--reps`` calls after ``--warmup`` calls, every call
ended by a device synchronise (host clock around it):
  (a) ``hip.tta_views``: the views made on the device from the uint8 image already there (table upload + nine launches), also as
      device time between two events;
  (b) what the reference does: ``DatasetMapperTTA`` on the host (18 PIL resizes / mirrors), a pinned host-to-device copy of every
      view, ``hip.preprocess`` per batch of three -- reported in its parts and in total;
  (c) the whole ``GeneralizedRCNNWithTTA`` call on the synthetic-weight model (device views), the same call with the host mapper, and
      for scale 18 plain ``model.inference`` calls on the 800x1333 image.
(a) and (b) are checked to give bit-equal batches before anything is timed.  Prints a table and one JSON line.  Not a test and not
part of bench.py.

    python tools/tta_bench.py [--reps 10] [--warmup 2] [--model-reps 3] [--skip-model] [--dtype bf16]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def medians(fn, reps, warmup):
    """median and min of ``reps`` synchronised calls, in ms"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts)


def device_ms(fn, reps):
    """median device time of one call between two events on the launch stream (the host's share of the call left out)"""
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--model-reps", type=int, default=3)
    ap.add_argument("--skip-model", action="store_true")
    ap.add_argument("--dtype", choices=("bf16", "f32"), default="bf16")
    ap.add_argument("--height", type=int, default=800)
    ap.add_argument("--width", type=int, default=1333)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "tta_bench measures on the GPU; there is no fallback"
    from cddmsl_amd import hip, synthetic
    from cddmsl_amd._lib import to_device_async
    from cddmsl_amd.config import get_cfg
    from cddmsl_amd.modeling import DatasetMapperTTA, GeneralizedRCNNWithTTA, build_model
    from cddmsl_amd.modeling.test_time_augmentation import view_sizes
    dev = "cuda"
    cfg = get_cfg()
    cfg.merge_from_file(os.path.join(ROOT, "configs", "VOC-Experiments", "faster_rcnn_CLIP_R_50_C4.yaml"))
    cfg.merge_from_list(["MODEL.DEVICE", dev, "MODEL.COMPUTE_DTYPE", args.dtype])
    dtype = {"bf16": torch.bfloat16, "f32": torch.float32}[args.dtype]
    mean, std = list(cfg.MODEL.PIXEL_MEAN), list(cfg.MODEL.PIXEL_STD)
    a = cfg.TEST.AUG
    h, w = args.height, args.width
    img_cpu = torch.from_numpy(np.random.RandomState(0).randint(0, 256, (3, h, w), dtype=np.uint8))
    img_dev = img_cpu.to(dev)
    inp = {"image": img_cpu, "height": h, "width": w}
    sizes = view_sizes(h, w, a.MIN_SIZES, a.MAX_SIZE)
    mapper = DatasetMapperTTA(cfg)

    def device_views():
        return hip.tta_views(img_dev, sizes, bool(a.FLIP), mean, std, dtype, 3, div255=True)

    def upload_and_preprocess(views):
        out = []
        for g in range(0, len(views), 3):
            ims = [to_device_async(v["image"], dev) for v in views[g:g + 3]]
            out.append(hip.preprocess(ims, max(i.shape[1] for i in ims), max(i.shape[2] for i in ims), mean, std, dtype, div255=True))
        return out

    def host_views():
        return upload_and_preprocess(mapper(inp))

    got, want = device_views(), host_views()
    torch.cuda.synchronize()
    same = len(got) == len(want) and all(torch.equal(g[0].view(torch.int16), x.view(torch.int16)) for g, x in zip(got, want))
    assert same, "the device views differ from the host mapper's"
    out_bytes = sum(g[0].numel() * g[0].element_size() for g in got)
    views = mapper(inp)
    del got, want
    rows = {"views": len(views), "out_MB": out_bytes / 1e6, "same_pixels": same}
    rows["a_tta_views_ms"], rows["a_tta_views_min_ms"] = medians(device_views, args.reps, args.warmup)
    rows["a_out_GBps"] = out_bytes / 1e6 / rows["a_tta_views_ms"]
    rows["a_device_events_ms"] = device_ms(device_views, args.reps)
    t_map = []
    for _ in range(max(3, args.reps // 2)):
        t0 = time.perf_counter()
        mapper(inp)
        t_map.append((time.perf_counter() - t0) * 1e3)
    rows["b_host_mapper_ms"] = statistics.median(t_map)
    rows["b_h2d_preprocess_ms"], _ = medians(lambda: upload_and_preprocess(views), args.reps, args.warmup)
    rows["b_total_ms"], rows["b_total_min_ms"] = medians(host_views, max(3, args.reps // 2), 1)
    rows["b_over_a"] = rows["b_total_ms"] / rows["a_tta_views_ms"]
    if not args.skip_model:
        model = build_model(cfg)
        model.load_state_dict(synthetic.make_state_dict(0, num_classes=cfg.MODEL.ROI_HEADS.NUM_CLASSES), strict=False)
        model.eval()
        tta_dev, tta_host = GeneralizedRCNNWithTTA(cfg, model), GeneralizedRCNNWithTTA(cfg, model, tta_mapper=mapper)
        dev_inp = {"image": img_dev, "height": h, "width": w}
        rows["c_tta_device_views_ms"], _ = medians(lambda: tta_dev([dev_inp]), args.model_reps, 1)
        rows["c_tta_host_mapper_ms"], _ = medians(lambda: tta_host([inp]), args.model_reps, 1)
        rows["c_18_plain_inference_ms"], _ = medians(lambda: [model.inference([dev_inp]) for _ in range(len(views))], args.model_reps, 1)
    for k, v in rows.items():
        print(f"{k:28s} {v:.3f}" if isinstance(v, float) else f"{k:28s} {v}", flush=True)
    print(json.dumps({"device": torch.cuda.get_device_name(0), "image": [h, w], "dtype": args.dtype, "reps": args.reps,
                      "warmup": args.warmup, "model_reps": args.model_reps, **rows}))


if __name__ == "__main__":
    main()
