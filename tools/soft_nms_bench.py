#!/usr/bin/env python
"""Soft-NMS speed at evaluation shapes: 1000 proposals x 20 classes (VOC) and x 8 classes (Cityscapes), candidates thresholded at
0.05 and at 0.001, boxes seeded and clustered around a few ground-truth boxes.  Per shape and method (gaussian, linear), ms per call of
  (a) the per-category walk kernel (hip.soft_nms, one launch sequence, no host sync),
  (b) the reference's algorithm on the same device: one pick per iteration on torch ops -- argmax, IoU row, decay, boolean
      compaction, two .item() readbacks (torch_soft_nms below; few repetitions, it is slow),
  (c) for context only, the existing hard batched_nms on the same candidates.
(a) is compared with (b), never with itself; the keep lists of (a) and (b) are compared as a sanity check (linear: equal).  Prints a
table and one JSON line.

    python tools/soft_nms_bench.py [--reps 20] [--torch-reps 1] [--skip-torch]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


def candidates(R, C, thresh, seed, dev, ngt=8, W=1024.0, H=512.0):
    """R proposals jittered around ngt boxes, a class-specific box per class, softmax scores that favour the box's class;
    -> the (proposal, class) pairs above ``thresh`` in row-major order, as fast_rcnn_inference_single_image forms them"""
    r = np.random.RandomState(seed)
    x0, y0 = r.uniform(0, W - 260, ngt), r.uniform(0, H - 200, ngt)
    gt = np.stack([x0, y0, x0 + r.uniform(40, 250, ngt), y0 + r.uniform(40, 190, ngt)], 1)
    gcls = r.randint(C, size=ngt)
    g = r.randint(ngt, size=R)
    prop = gt[g] + r.normal(0, 12.0, (R, 4))
    boxes = prop[:, None, :] + r.normal(0, 3.0, (R, C, 4))
    logits = r.normal(0, 1.0, (R, C + 1))
    logits[np.arange(R), gcls[g]] += r.uniform(0, 6, R)
    p = np.exp(logits)
    p = (p / p.sum(1, keepdims=True))[:, :C]
    pi, ci = np.nonzero(p > thresh)
    t = lambda a, d: torch.from_numpy(np.ascontiguousarray(a.astype(d))).to(dev)
    return t(np.clip(boxes[pi, ci], 0, W), np.float32), t(p[pi, ci], np.float32), t(ci, np.int64)


def torch_soft_nms(boxes, scores, idxs, method, sigma, thr, prune):
    """the reference's walk (one pick per iteration over ALL categories on shifted coordinates) on torch ops of the same device"""
    b = boxes + (idxs.to(boxes) * (boxes.max() + 1))[:, None]
    s, ids = scores.clone(), torch.arange(len(scores), device=boxes.device)
    area = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    out_i, out_s = [], []
    while s.numel():
        t = torch.argmax(s)
        out_i.append(ids[t].item())
        out_s.append(s[t].item())
        wh = (torch.min(b[t, 2:], b[:, 2:]) - torch.max(b[t, :2], b[:, :2])).clamp_(min=0)
        inter = wh[:, 0] * wh[:, 1]
        iou = torch.where(inter > 0, inter / (area[t] + area - inter), torch.zeros_like(inter))
        if method == "linear":
            decay = torch.where(iou > thr, 1 - iou, torch.ones_like(iou))
        elif method == "hard":
            decay = (iou < thr).float()
        else:
            decay = torch.exp(-(iou * iou) / sigma)
        s = s * decay
        live = s > prune
        live[t] = False
        b, s, ids, area = b[live], s[live], ids[live], area[live]
    return torch.tensor(out_i, device=boxes.device), torch.tensor(out_s, device=boxes.device)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--torch-reps", type=int, default=1)
    ap.add_argument("--skip-torch", action="store_true")
    ap.add_argument("--max-keep", type=int, default=100, help="TEST.DETECTIONS_PER_IMAGE, passed to the kernel as its cap")
    args = ap.parse_args()
    from cddmsl_amd import hip
    from cddmsl_amd.modeling.roi_heads import batched_nms
    dev = "cuda"
    rows = []
    for name, C in (("voc", 20), ("cityscapes", 8)):
        for thresh in (0.05, 0.001):
            b, s, i = candidates(1000, C, thresh, 7, dev)
            K = len(s)
            t_hard = timed(lambda: batched_nms(b, s, i, 0.5), args.reps)      # (more than 12 288 candidates: its per-category path)
            for method in ("gaussian", "linear"):
                run = lambda mk: hip.soft_nms(b, s, i, method, 0.5, 0.5, 0.001, mk)
                t_full, t_cap = timed(lambda: run(-1), args.reps), timed(lambda: run(args.max_keep), args.reps)
                keep, ks, nk = run(-1)
                n = int(nk[0])
                row = {"set": name, "classes": C, "thresh": thresh, "K": K, "method": method, "picks": n, "kernel_ms": t_full * 1e3,
                       f"kernel_cap{args.max_keep}_ms": t_cap * 1e3, "hard_batched_nms_ms": t_hard * 1e3}
                if not args.skip_torch:
                    torch_soft_nms(b[:64], s[:64], i[:64], method, 0.5, 0.5, 0.001)        # warm the ops; a full warm-up run costs seconds
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(args.torch_reps):
                        ti, ts = torch_soft_nms(b, s, i, method, 0.5, 0.5, 0.001)
                    torch.cuda.synchronize()
                    t_torch = (time.perf_counter() - t0) / args.torch_reps
                    row.update(torch_loop_ms=t_torch * 1e3, speedup=t_torch / t_full,
                               same_keep=bool(len(ti) == n and torch.equal(ti, keep[:n])),
                               max_score_diff=float((ts - ks[:n]).abs().max()) if len(ti) == n and n else None)
                rows.append(row)
                print({k: (round(v, 4) if isinstance(v, float) else v) for k, v in row.items()}, flush=True)
    print(json.dumps({"device": torch.cuda.get_device_name(0), "reps": args.reps, "torch_reps": args.torch_reps, "rows": rows}))


if __name__ == "__main__":
    main()
