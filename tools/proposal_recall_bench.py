#!/usr/bin/env python
"""Times proposal recall (ProposalRecallEvaluator, limits 100 and 1000, ranges all / small / medium / large) three ways on a seeded
set of the order of the real test sets:

  device  process() launches hip.proposal_cover per call and keeps everything on the device, evaluate() reads the cover records back
          once -- the evaluator with ``device``
  host    process() copies every image's proposals to the host and runs proposal_cover_host (numpy f32) -- the evaluator without
  torch   the reference's formulation composed from torch ops on the device, written here: per image and per (limit, range)
          ``pairwise_iou`` and the ``max(dim=0)`` / ``max(dim=0)`` / mask loop of _evaluate_box_proposals on GPU tensors, one readback at
          the end.  Timed on the first ``--torch-images`` images (every iteration of its loop is a handful of launches and a
          host-device round trip), its seconds are reported with that image count next to them.

All three see the same proposals (already on the GPU, as the model leaves them).  The two evaluators must return the same dictionary
and the torch walk the same cover values on its images; the tool checks both before it prints.  Every timed window ends in a device
synchronise; the device path is repeated ``--repeats`` times after a warm-up and the median is reported with the spread.  One JSON
line.

    python tools/proposal_recall_bench.py [--images 5000] [--proposals 1000] [--gt-min 3] [--gt-max 40] [--batch 1] [--repeats 5]
                                          [--torch-images 100] [--skip-host] [--skip-torch]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def make_set(n_images, n_props, gt_min, gt_max, seed=0):
    """1280x720 frames; gt_min..gt_max boxes per image of 8..300 pixels a side, ``n_props`` proposals: jittered copies of the boxes
    (about two thirds) plus free ones, distinct logits"""
    rng = np.random.RandomState(seed)
    dicts, props = [], []
    for i in range(n_images):
        n_gt = rng.randint(gt_min, gt_max + 1)
        wh = np.round(np.exp(rng.uniform(np.log(8), np.log(300), (n_gt, 2))) * 4) / 4
        xy = np.round(rng.uniform(0, 1, (n_gt, 2)) * (np.array([1280, 720]) - wh).clip(min=1) * 4) / 4
        anns = [{"bbox": [float(x), float(y), float(x + w), float(y + h)], "area": float(w * h), "iscrowd": int(rng.rand() < 0.05), "category_id": 0}
                for (x, y), (w, h) in zip(xy, wh)]
        dicts.append({"image_id": i, "height": 720, "width": 1280, "annotations": anns})
        src = rng.randint(n_gt, size=n_props)
        b = np.concatenate([xy[src], xy[src] + wh[src]], axis=1) + rng.normal(0, 1, (n_props, 4)) * np.tile(wh[src], 2) * 0.15
        free = rng.rand(n_props) < 0.33
        fxy = rng.uniform(0, 1, (n_props, 2)) * np.array([1200, 640])
        b[free] = np.concatenate([fxy, fxy + rng.uniform(4, 300, (n_props, 2))], axis=1)[free]
        b[:, 2:] = np.maximum(b[:, 2:], b[:, :2] + 1)
        props.append((b.astype(np.float32), (rng.permutation(n_props) * 0.01 - 5.0).astype(np.float32)))
    return dicts, props


def run_evaluator(dicts, dev_props, device, batch):
    from cddmsl_amd.evaluation import ProposalRecallEvaluator
    from cddmsl_amd.structures import Boxes, Instances
    ev = ProposalRecallEvaluator(dicts, device=device)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for s in range(0, len(dicts), batch):
        inputs = [{"image_id": d["image_id"]} for d in dicts[s: s + batch]]
        outputs = []
        for b, lg in dev_props[s: s + batch]:
            inst = Instances((720, 1280))
            inst.proposal_boxes, inst.objectness_logits = Boxes(b), lg
            outputs.append({"proposals": inst})
        ev.process(inputs, outputs)
    t1 = time.perf_counter()          # (device path: the launches are enqueued, not finished -- evaluate()'s readback waits for them)
    res = ev.evaluate()
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    return ev, res, t1 - t0, t2 - t1


def torch_walk(dev_props, gts, limits, num_ranges):
    """the reference's per-image body on device tensors -> per image cover [L, A, g] on the host, after ONE readback"""
    out = []
    for (boxes, logits), (gb, bits) in zip(dev_props, gts):
        G = gb.shape[0]
        cover = -torch.ones((len(limits), num_ranges, G), device=boxes.device)
        if G and len(logits):
            inds = logits.sort(descending=True)[1]
            pb = boxes[inds]
            for li, limit in enumerate(limits):
                kept = pb[:limit] if limit is not None and len(pb) > limit else pb
                for a in range(num_ranges):
                    cols = torch.nonzero((bits >> a) & 1).squeeze(1)
                    g = gb[cols]
                    if len(g) == 0:
                        continue
                    area1, area2 = (kept[:, 2] - kept[:, 0]) * (kept[:, 3] - kept[:, 1]), (g[:, 2] - g[:, 0]) * (g[:, 3] - g[:, 1])
                    wh = torch.min(kept[:, None, 2:], g[:, 2:]) - torch.max(kept[:, None, :2], g[:, :2])
                    wh.clamp_(min=0)
                    inter = wh.prod(dim=2)
                    overlaps = torch.where(inter > 0, inter / (area1[:, None] + area2 - inter), torch.zeros(1, device=inter.device))
                    rec = torch.zeros(len(g), device=boxes.device)
                    for _ in range(min(len(kept), len(g))):
                        max_overlaps, argmax_overlaps = overlaps.max(dim=0)
                        gt_ovr, gt_ind = max_overlaps.max(dim=0)
                        box_ind = argmax_overlaps[gt_ind]
                        rec[gt_ind] = overlaps[box_ind, gt_ind]
                        overlaps[box_ind, :] = -1
                        overlaps[:, gt_ind] = -1
                    cover[li, a, cols] = rec
        out.append(cover)
    host = torch.cat([c.reshape(-1) for c in out]).cpu().numpy() if out else np.zeros(0, dtype=np.float32)
    res, pos = [], 0
    for c in out:
        res.append(host[pos: pos + c.numel()].reshape(c.shape))
        pos += c.numel()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=5000)
    ap.add_argument("--proposals", type=int, default=1000)
    ap.add_argument("--gt-min", type=int, default=3)
    ap.add_argument("--gt-max", type=int, default=40)
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--torch-images", type=int, default=100)
    ap.add_argument("--skip-host", action="store_true")
    ap.add_argument("--skip-torch", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this tool times the MI355X paths: no GPU, no number"
    dicts, props = make_set(a.images, a.proposals, a.gt_min, a.gt_max)
    dev_props = [tuple(torch.from_numpy(x).cuda() for x in p) for p in props]
    out = {"images": a.images, "proposals_per_image": a.proposals, "gt_per_image": [a.gt_min, a.gt_max], "batch": a.batch,
           "limits": [100, 1000], "ranges": 4, "device": torch.cuda.get_device_name(0)}
    try:
        out["sclk_mhz"] = int(torch.cuda.clock_rate())
    except Exception:                                                         # (no SMI library behind torch: the clock stays unnamed)
        out["sclk_mhz"] = None
    run_evaluator(dicts[:16], dev_props[:16], "cuda", a.batch)                # warm-up: library load, first launch, pinned buffers
    tp, te = [], []
    for _ in range(max(a.repeats, 1)):
        ev, dev, p_s, e_s = run_evaluator(dicts, dev_props, "cuda", a.batch)
        tp.append(p_s); te.append(e_s)
    tot = [x + y for x, y in zip(tp, te)]
    out.update(device_process_s=statistics.median(tp), device_evaluate_s=statistics.median(te), device_total_s=statistics.median(tot),
               device_total_min_max_s=[round(min(tot), 4), round(max(tot), 4)], repeats=len(tot))
    out["AR@100"], out["AR@1000"] = dev["box_proposals"]["AR@100"], dev["box_proposals"]["AR@1000"]
    if not a.skip_host:
        _, host, out["host_process_s"], out["host_evaluate_s"] = run_evaluator(dicts, dev_props, None, a.batch)
        out["host_total_s"] = out["host_process_s"] + out["host_evaluate_s"]
        same = list(host["box_proposals"]) == list(dev["box_proposals"]) and all(
            x == y or (x != x and y != y) for x, y in zip(host["box_proposals"].values(), dev["box_proposals"].values()))
        out["results_equal"] = bool(same)
    if not a.skip_torch:
        n = min(a.torch_images, a.images)
        gts = [tuple(torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in ev._gt_list[i]) for i in range(n)]
        torch_walk(dev_props[:2], gts[:2], ev.limits, ev.num_ranges)          # warm-up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        covers = torch_walk(dev_props[:n], gts, ev.limits, ev.num_ranges)
        torch.cuda.synchronize()
        out["torch_device_s"], out["torch_images"] = time.perf_counter() - t0, n
        out["torch_device_s_per_image"] = out["torch_device_s"] / max(n, 1)
        out["device_total_s_per_image"] = out["device_total_s"] / max(a.images, 1)
        rec = ev._device_records()
        # the same multiset of values per (limit, range) and image (with equal IoUs the device's arg-max may name another box)
        out["torch_covers_equal"] = bool(all(np.array_equal(np.sort(c, axis=2), np.sort(rec[i], axis=2)) for i, c in enumerate(covers)))
    print(json.dumps({k: (round(v, 6) if isinstance(v, float) else v) for k, v in out.items()}))
    return 0 if out.get("results_equal", True) and out.get("torch_covers_equal", True) else 1


if __name__ == "__main__":
    sys.exit(main())
