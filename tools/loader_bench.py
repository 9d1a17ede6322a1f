#!/usr/bin/env python
"""Does the REAL input pipeline keep up with the step?  (data/build.py:262-308, data/dataset_mapper.py:126-217)

bench.py times the step on synthetic batches already resident in HBM; this tool measures the other side:

  1. writes a VOC-shaped tree of JPEGs (500x375 / 375x500 like VOC2007, 1-5 boxes each) plus the domain-translated twins on the
     box's local disk (PIL; no dataset ships with the repo),
  2. loader alone: samples/s of ``build_detection_train_loader`` (JPEG decode of image + twin, ONE ResizeShortestEdge draw from
     INPUT.MIN_SIZE_TRAIN = 480..800 + flip applied to both, aspect-ratio batches, pinned uint8 -> device) for several
     DATALOADER.NUM_WORKERS,
  3. the training step fed by that loader (multi-scale shapes through the kernel dispatch, the caching allocator and the gradient
     buckets), against the same trainer on synthetic 800x1333 batches: ms/step, samples/s, allocator state after iteration 10
     and at the end.

``--crop [TYPE:A,B]`` / ``--min-size-range`` / ``--flip vertical`` pass INPUT.CROP, MIN_SIZE_TRAIN_SAMPLING "range" and RANDOM_FLIP on.
``--device-resize`` runs 2. and 3. with DATALOADER.DEVICE_RESIZE: the workers only decode, and the staging thread's one kernel launch
per batch (cddmsl_resize_batch_u8) resizes, mirrors and transposes on the GPU -- the same bytes reach the model.
``--color-jitter`` switches INPUT.COLOR_JITTER on with representative ranges (brightness, contrast and saturation in 0.6..1.4, lighting
scale 25.5 = AlexNet's 0.1 on 0..255 pixels, the twin with the same draws): in the workers (numpy) without ``--device-resize``, one more
launch per batch (cddmsl_color_jitter_batch_u8) with it.  ``--kernel-times`` (with ``--device-resize``) stages one batch by hand and
prints the device time of the batch's resize and jitter launches, each timed between events behind a few milliseconds of queued
fills so that no launch latency is inside the window, next to the bytes they move.

usage (GPU box): python tools/loader_bench.py --iters 50 > profiles/r03_loader.txt
"""
import argparse
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def make_voc_tree(root, n, seed=0, year="VOC2007", twin="clipart"):
    """n JPEG pairs + annotations; smooth synthetic pictures (JPEG decode cost depends on content: noise would overstate it)"""
    from PIL import Image
    from cddmsl_amd.evaluation import VOC_CLASS_NAMES
    g = np.random.RandomState(seed)
    base = os.path.join(root, "VOC", year)
    tw = os.path.normpath(os.path.join(base, "..", twin, year))
    for d in (os.path.join(base, "Annotations"), os.path.join(base, "ImageSets", "Main"), os.path.join(base, "JPEGImages"), os.path.join(tw, "JPEGImages")):
        os.makedirs(d, exist_ok=True)
    ids = []
    for i in range(n):
        w, h = (500, 375) if g.rand() < 0.75 else (375, 500)
        fid = f"{i:06d}"
        ids.append(fid)
        yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
        img = np.stack([127 + 100 * np.sin(xx / g.uniform(8, 60) + g.uniform(0, 6)) * np.cos(yy / g.uniform(8, 60)) for _ in range(3)], axis=2)
        img = np.clip(img + g.normal(0, 12, img.shape), 0, 255).astype(np.uint8)
        Image.fromarray(img).save(os.path.join(base, "JPEGImages", fid + ".jpg"), quality=90)
        Image.fromarray(np.clip(img.astype(np.int16) // 32 * 32 + 16, 0, 255).astype(np.uint8)).save(os.path.join(tw, "JPEGImages", fid + ".jpg"), quality=90)
        objs = ""
        for _ in range(g.randint(1, 6)):
            x0, y0 = g.randint(1, w - 80), g.randint(1, h - 80)
            x1, y1 = min(w, x0 + g.randint(40, 300)), min(h, y0 + g.randint(40, 300))
            objs += ("<object><name>%s</name><difficult>0</difficult><bndbox><xmin>%d</xmin><ymin>%d</ymin><xmax>%d</xmax><ymax>%d</ymax></bndbox></object>"
                     % (VOC_CLASS_NAMES[g.randint(0, 20)], x0, y0, x1, y1))
        with open(os.path.join(base, "Annotations", fid + ".xml"), "w") as f:
            f.write(f"<annotation><size><width>{w}</width><height>{h}</height></size>{objs}</annotation>")
    for split in ("trainval", "test"):
        with open(os.path.join(base, "ImageSets", "Main", split + ".txt"), "w") as f:
            f.write("\n".join(ids) + "\n")
    return base


def kernel_times(cfg, dicts, batch, reps=20):
    """one landscape batch through DeviceBatches._stage, `reps` times; the resize and the jitter launch each between two events on the
    staging stream, behind queued fills (the host has long enqueued both launches when the device reaches them)"""
    from cddmsl_amd import data, hip
    assert cfg.DATALOADER.DEVICE_RESIZE, "--kernel-times measures the device path: add --device-resize"
    mapper = data.DatasetMapper(cfg, True, np.random.RandomState(0))
    samples = []
    for d in dicts:
        s = mapper(d)
        if s[data.DEVICE_RESIZE_KEY]["size"][1] > s[data.DEVICE_RESIZE_KEY]["size"][0]:
            samples.append(s)
        if len(samples) == batch:
            break
    db = data.DeviceBatches(iter(()), cfg.MODEL.DEVICE)
    filler = torch.empty(1 << 30, dtype=torch.uint8, device=cfg.MODEL.DEVICE)
    torch.cuda.synchronize()
    events, moved = {"resize": [], "jitter": []}, {}
    real = {"resize": hip.resize_batch_u8, "jitter": hip.color_jitter_batch_u8}

    def timed(name):
        def f(*a):
            if name == "resize":
                for _ in range(4):
                    filler.fill_(1)                        # ~ms of device work in front: both launches below queue up behind it
                moved[name] = sum(3 * it[2] * it[3] + 3 * it[4] * it[5] for it in a[3])
            else:
                moved[name] = sum(3 * h * w * (3 if "contrast" in p else 2) for _, h, w, p, _ in a[1])
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = real[name](*a)
            e1.record()
            events[name].append((e0, e1))
            return out
        return f

    hip.resize_batch_u8, hip.color_jitter_batch_u8 = timed("resize"), timed("jitter")
    try:
        for _ in range(reps + 3):
            db._stage(samples)
            torch.cuda.synchronize()
    finally:
        hip.resize_batch_u8, hip.color_jitter_batch_u8 = real["resize"], real["jitter"]
        db.close()
    sizes = sorted({tuple(s[data.DEVICE_RESIZE_KEY]["size"]) for s in samples})
    print(f"# kernel times, one batch of {len(samples)} pairs ({2 * len(samples)} images, output sizes {sizes[0]} .. {sizes[-1]}), median of {reps} after 3 warm-up batches, behind queued fills")
    for name, evs in events.items():
        if not evs:
            print(f"{name:8s} not launched")
            continue
        ms = sorted(e0.elapsed_time(e1) for e0, e1 in evs[3:])
        med = ms[len(ms) // 2]
        what = "read of the originals + write of the results" if name == "resize" else "read + write of the results, one more read for contrast; sum + apply launches"
        print(f"{name:8s} {med:7.4f} ms (min {ms[0]:.4f}, max {ms[-1]:.4f})   {moved[name] / 1e6:8.1f} MB ({what})   {moved[name] / med / 1e6:7.1f} GB/s")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=256)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--workers", default="0,4,8,12")
    ap.add_argument("--loader-batches", type=int, default=12)
    ap.add_argument("--device-resize", action="store_true", help="DATALOADER.DEVICE_RESIZE: resize / flip on the GPU in the staging thread")
    ap.add_argument("--color-jitter", action="store_true", help="INPUT.COLOR_JITTER: brightness / contrast / saturation / lighting on image and twin")
    ap.add_argument("--kernel-times", action="store_true", help="device time of one batch's resize and jitter launches (needs --device-resize)")
    ap.add_argument("--skip-step", action="store_true", help="loader alone: skip the training-step measurements")
    ap.add_argument("--crop", nargs="?", const="relative_range:0.9,0.9", default=None, metavar="TYPE:A,B",
                    help="INPUT.CROP: RandomCrop in front of the resize, e.g. relative_range:0.9,0.9 (the default with no value) or absolute:300,400")
    ap.add_argument("--min-size-range", action="store_true", help="INPUT.MIN_SIZE_TRAIN_SAMPLING range: any short edge in [min, max] of INPUT.MIN_SIZE_TRAIN")
    ap.add_argument("--flip", choices=("horizontal", "vertical", "none"), default=None, help="INPUT.RANDOM_FLIP")
    args = ap.parse_args()
    import bench
    from cddmsl_amd import data, engine, synthetic
    from cddmsl_amd.evaluation import VOC_CLASS_NAMES
    cfg = bench.make_cfg("bf16")
    cfg.MODEL.DEVICE = "cuda:0"
    cfg.merge_from_list(["DATALOADER.DEVICE_RESIZE", bool(args.device_resize)])
    if args.crop is not None:
        ctype, _, csize = args.crop.partition(":")
        size = [float(v) if ctype.startswith("relative") else int(v) for v in (csize or "0.9,0.9").split(",")]
        cfg.merge_from_list(["INPUT.CROP.ENABLED", True, "INPUT.CROP.TYPE", ctype, "INPUT.CROP.SIZE", size])
    if args.min_size_range:
        cfg.merge_from_list(["INPUT.MIN_SIZE_TRAIN_SAMPLING", "range", "INPUT.MIN_SIZE_TRAIN", (min(cfg.INPUT.MIN_SIZE_TRAIN), max(cfg.INPUT.MIN_SIZE_TRAIN))])
    if args.flip is not None:
        cfg.merge_from_list(["INPUT.RANDOM_FLIP", args.flip])
    if args.color_jitter:
        cfg.merge_from_list(["INPUT.COLOR_JITTER.ENABLED", True, "INPUT.COLOR_JITTER.BRIGHTNESS", (0.6, 1.4), "INPUT.COLOR_JITTER.CONTRAST", (0.6, 1.4),
                             "INPUT.COLOR_JITTER.SATURATION", (0.6, 1.4), "INPUT.COLOR_JITTER.LIGHTING", 25.5])
    engine.limit_host_threads()       # as build_trainer does: the box grants ~16 CPUs, torch's default intra-op pool has one thread per logical CPU
    root = tempfile.mkdtemp(prefix="cddmsl_voc_")
    t0 = time.perf_counter()
    base = make_voc_tree(root, args.images)
    print(f"# synthetic VOC tree: {args.images} JPEG pairs (500x375 / 375x500) under {root}, written in {time.perf_counter() - t0:.1f} s")
    dicts = data.load_voc_instances(base, "trainval", VOC_CLASS_NAMES, dt_data="clipart")
    print(f"# INPUT.MIN_SIZE_TRAIN {tuple(cfg.INPUT.MIN_SIZE_TRAIN)} ({cfg.INPUT.MIN_SIZE_TRAIN_SAMPLING}) max {cfg.INPUT.MAX_SIZE_TRAIN}, flip {cfg.INPUT.RANDOM_FLIP}, crop {(cfg.INPUT.CROP.TYPE, tuple(cfg.INPUT.CROP.SIZE)) if cfg.INPUT.CROP.ENABLED else None}; host: {os.cpu_count()} logical CPUs ({bench.cpu_model_name()})")
    print(f"# DATALOADER.DEVICE_RESIZE {cfg.DATALOADER.DEVICE_RESIZE}; INPUT.COLOR_JITTER {dict(cfg.INPUT.COLOR_JITTER) if cfg.INPUT.COLOR_JITTER.ENABLED else 'off'}")
    if args.kernel_times:
        kernel_times(cfg, dicts, args.batch)
    print("# 1. loader alone (decode 2 JPEGs + resize both + flip + batch + pin + H2D" + (" of the originals + one resize launch per batch" if args.device_resize else "")
          + "), samples/s after 2 warm-up batches")
    rates = {}
    for nw in [int(x) for x in args.workers.split(",")]:
        ld = data.build_detection_train_loader(cfg, dicts, args.batch, 0, 1, cfg.MODEL.DEVICE, num_workers=nw)
        for _ in range(2):
            next(ld)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.loader_batches):
            b = next(ld)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        rates[nw] = args.batch * args.loader_batches / dt
        shapes = sorted({tuple(x["image"].shape[1:]) for x in b})
        st = getattr(ld, "stats", None) or {"batches": 1, "pull_s": 0, "stage_s": 0, "handover_wait_s": 0}
        nb = max(st["batches"], 1)
        print(f"workers {nw:3d}   {rates[nw]:8.1f} samples/s   ({dt / args.loader_batches * 1e3:7.1f} ms per batch of {args.batch}; staging thread per batch: "
              f"{st['pull_s'] / nb * 1e3:.1f} ms pulling samples, {st['stage_s'] / nb * 1e3:.1f} ms pinned copy + H2D enqueue, {st['handover_wait_s'] / nb * 1e3:.1f} ms waiting for the consumer; "
              f"last batch shapes {shapes[:2]}...)")
        ld.close()
        del ld
    best = max(rates, key=rates.get)
    if args.skip_step:
        return

    def run(loader, tag):
        tr = engine.build_trainer(cfg, args.batch, 800, 1333)
        tr.model.load_state_dict(synthetic.make_state_dict(0), strict=False)
        tr.clipcap_model.load_state_dict(synthetic.make_mapper_state_dict(1))
        tr.iter, tr.metrics_period = 20000, 0
        if loader is not None:
            tr.data_loader, tr._data_loader_iter = loader, iter(loader)
        times = []
        for it in range(11):                                   # iterations 0-10: synchronised one by one (start-up behaviour)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            tr.run_step()
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t0)
        mem10 = (torch.cuda.memory_allocated(), torch.cuda.memory_reserved())
        n = max(args.iters - 11, 1)
        t0 = time.perf_counter()
        for it in range(n):                                    # the rest as the trainer runs them: no host synchronisation,
            tr.run_step()                                      # the loader's next() overlaps the previous step on the GPU
        torch.cuda.synchronize()
        med = (time.perf_counter() - t0) / n
        end = (torch.cuda.memory_allocated(), torch.cuda.memory_reserved())
        print(f"{tag:34s} {med * 1e3:7.1f} ms/step = {args.batch / med:6.1f} samples/s over {n} un-synchronised iterations   (iterations 0-10, synchronised: "
              f"{', '.join('%.0f' % (t * 1e3) for t in times)} ms)   reserved after iteration 10: {mem10[1] / 2**30:.1f} GiB, at the end: {end[1] / 2**30:.1f} GiB "
              f"(allocated {mem10[0] / 2**30:.1f} -> {end[0] / 2**30:.1f} GiB)")
        if loader is not None:
            loader.close()
        del tr
        torch.cuda.empty_cache()
        return med

    print(f"# 2. the training step, {args.iters} iterations each")
    s = run(None, "synthetic 800x1333 batches in HBM")
    r = run(data.build_detection_train_loader(cfg, dicts, args.batch, 0, 1, cfg.MODEL.DEVICE, num_workers=best), f"real loader, {best} workers, multi-scale")
    print(f"# the step consumes {args.batch / s:.0f} samples/s on synthetic 800x1333 inputs; the loader delivers {rates[best]:.0f} samples/s with {best} workers "
          f"({rates[best] / (args.batch / s):.1f}x); real-loader step / synthetic step = {r / s:.2f} (multi-scale images are smaller on average: 480-800 short edge)")


if __name__ == "__main__":
    main()
