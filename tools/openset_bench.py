#!/usr/bin/env python
"""Open-vocabulary classify-and-select speed at evaluation shapes: R = 1000 regions, D = 1024, K in {20, 80, 1203} classes, score
thresholds 0.05 and 0.001, seeded region features at T = 0.01 (each a mixture of up to 24 class embeddings, so that 0.001 lets tens of
thousands of candidates through at K = 1203 and batched_nms leaves its single pass).  Per shape, ms per call (HIP events, mean of ``--reps``
after a warm-up) of
  (a) the pair hip.openset_logits + hip.openset_select (one readback: the candidate count),
  (b) the closed-set composition on the same inputs: hip.cosine_logits_fwd, torch softmax, threshold, nonzero, gathers, clip -- what
      FastRCNNOutputLayers.forward / predict_probs / fast_rcnn_inference_single_image run up to the NMS (one readback: nonzero).
For K = 1203 also batched_nms_grouped against batched_nms on the selected candidates.  The outputs of (a) and (b) are compared
before any time is printed: same candidate list, up to entries whose score lies within 1e-5 of the threshold (the two evaluate the
softmax in different orders), scores within 1e-4 relative.  Prints a table and one JSON line.

    python tools/openset_bench.py [--reps 20]
"""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def timed(fn, reps):
    fn()
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def inputs(R, K, D, seed, dev, W=1333.0, H=800.0):
    g = np.random.default_rng(seed)
    wn = g.standard_normal((K, D))
    wn = (wn / np.linalg.norm(wn, axis=1, keepdims=True)).astype(np.float32)
    m = min(K, 24)          # every region is a mixture of m classes with nearly equal weights: a few pass 0.05, most of the m pass 0.001
    own = np.argsort(g.random((R, K)), axis=1)[:, :m]
    x = np.zeros((R, D))
    for j in range(m):
        x += (1.0 - g.uniform(0, 0.1, size=(R, 1))) * wn[own[:, j]]
    x = (x + 0.1 * g.standard_normal((R, D)) / math.sqrt(D)).astype(np.float32)
    ngt = 12
    x0, y0 = g.uniform(0, W - 300, ngt), g.uniform(0, H - 250, ngt)
    gt = np.stack([x0, y0, x0 + g.uniform(40, 290, ngt), y0 + g.uniform(40, 240, ngt)], 1)
    boxes = (gt[g.integers(0, ngt, size=R)] + g.normal(0, 12.0, (R, 4))).astype(np.float32)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return t(x), t(wn), t(boxes)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    from cddmsl_amd import hip
    from cddmsl_amd.modeling.roi_heads import batched_nms, batched_nms_grouped
    from cddmsl_amd.structures import Boxes
    dev, R, D, T, H, W = "cuda", 1000, 1024, 0.01, 800, 1333
    rows = []
    for K in (20, 80, 1203):
        x, wn, boxes = inputs(R, K, D, 7, dev)
        for thresh in (0.05, 0.001):
            def pair():
                logits, stats = hip.openset_logits(x, wn, T)
                return hip.openset_select(logits, stats, K, boxes, None, H, W, thresh)

            def closed():
                scores = torch.softmax(hip.cosine_logits_fwd(x, wn, T)[0], dim=-1)[:, :-1]
                b = Boxes(boxes.clone())
                b.clip((H, W))
                mask = scores > thresh
                inds = mask.nonzero()
                return inds, scores[mask], b.tensor[inds[:, 0]]

            prow, pcls, pscore, pbox, _ = pair()
            inds, cscore, cbox = closed()
            # ---- outputs first: the same candidates up to scores at the threshold, then scores and boxes of the common entries
            key_a = (prow.long() * K + pcls.long()).cpu().numpy()
            key_b = (inds[:, 0] * K + inds[:, 1]).cpu().numpy()
            common, ia, ib = np.intersect1d(key_a, key_b, return_indices=True)
            sa, sb = pscore.cpu().numpy(), cscore.cpu().numpy()
            only = np.concatenate([sa[np.setdiff1d(np.arange(len(key_a)), ia)], sb[np.setdiff1d(np.arange(len(key_b)), ib)]])
            assert (np.abs(only - thresh) <= 1e-5).all(), ("candidate lists differ away from the threshold", K, thresh, only[:8])
            assert np.allclose(sa[ia], sb[ib], rtol=1e-4, atol=0), float(np.abs(sa[ia] / sb[ib] - 1).max())
            assert np.array_equal(pbox.cpu().numpy()[ia], cbox.cpu().numpy()[ib])
            row = {"K": K, "thresh": thresh, "candidates": int(len(key_a)), "only_in_one": int(len(only)),
                   "pair_ms": timed(pair, args.reps), "closed_set_composition_ms": timed(closed, args.reps),
                   "logits_ms": timed(lambda: hip.openset_logits(x, wn, T), args.reps),
                   "cosine_logits_fwd_ms": timed(lambda: hip.cosine_logits_fwd(x, wn, T), args.reps)}
            row["speedup"] = row["closed_set_composition_ms"] / row["pair_ms"]
            if K == 1203:
                n = len(key_a)
                cl = pcls.long()
                ka, kb = batched_nms_grouped(pbox, pscore, cl, 0.5), batched_nms(pbox, pscore, cl, 0.5)
                # (above 12 288 candidates batched_nms runs one pass per category on the unshifted boxes; the coordinate trick adds
                # up to K * (W + 1) = 1.6e6 to a coordinate, where f32 is spaced by 0.125: IoUs next to the threshold can fall
                # on the other side -- the same holds for batched_nms' own single pass below 12 288 candidates)
                row["nms_same_keep"] = bool(torch.equal(ka, kb))
                row["nms_kept"] = [int(ka.numel()), int(kb.numel()), int(np.intersect1d(ka.cpu().numpy(), kb.cpu().numpy()).size)]
                row["nms_grouped_ms"] = timed(lambda: batched_nms_grouped(pbox, pscore, cl, 0.5), args.reps)
                row["nms_batched_ms"] = timed(lambda: batched_nms(pbox, pscore, cl, 0.5), max(1, args.reps // 4) if n > 12288 else args.reps)
            rows.append(row)
            print({k: (round(v, 4) if isinstance(v, float) else v) for k, v in row.items()}, flush=True)
    print(json.dumps({"device": torch.cuda.get_device_name(0), "reps": args.reps, "R": R, "D": D, "rows": rows}))


if __name__ == "__main__":
    main()
