#!/usr/bin/env python
"""Box-regression loss speed at the benchmark's sizes: 16 images, 2048 positives (and 2048 negatives) of 16 x 62 250 anchors for the
RPN, 16 x 512 RoIs with 2048 foreground rows at 20 classes for the box head.  Per loss (GIoU, smooth-L1 beta 1/9), ms per call,
forward and backward timed apart, of
  (a) the kernel (hip.rpn_losses_reg / hip.box_reg_loss: one launch per direction; the backward also zero-fills its outputs),
  (b) its torch formulation on the same device (modeling.rpn.box_reg_loss_terms over the gathered rows -- for the RPN without the
      classification half, which (a) includes -- and torch autograd for the backward).
(a) is compared with (b), never with itself; the two losses are compared as a sanity check.  Prints a table and one JSON line.

    python tools/box_loss_bench.py [--reps 50]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def timed(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


def boxes(n, seed, size, dev):
    g = torch.Generator().manual_seed(seed)
    b = torch.rand((n, 4), generator=g) * size
    b[:, 2:] += b[:, :2] + 8
    return b.to(dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    args = ap.parse_args()
    from cddmsl_amd import hip
    from cddmsl_amd.modeling.rpn import SCALE_CLAMP, box_reg_loss_terms
    dev = "cuda"
    g = torch.Generator().manual_seed(1)
    N, A, npos, G = 16, 62250, 2048, 64
    anchors, gt = boxes(A, 2, 1000.0, dev), boxes(G, 3, 1000.0, dev)
    gt_off = (torch.arange(N) * (G // N)).to(dev)
    midx = torch.randint(0, G // N, (N * A,), generator=g).to(dev)
    perm = torch.randperm(N * A, generator=g)
    pos, neg = perm[:npos].to(dev), perm[npos:2 * npos].to(dev)
    logits = torch.randn(N * A, generator=g).to(dev)
    rw, bw = (1.0, 1.0, 1.0, 1.0), (10.0, 10.0, 5.0, 5.0)
    rdeltas = (torch.randn(N * A, 4, generator=g) * torch.tensor([0.1, 0.1, 0.2, 0.2])).to(dev)
    R, K, nfg = 16 * 512, 20, 2048
    src, tgt = boxes(R, 4, 1000.0, dev), boxes(R, 5, 1000.0, dev)
    cls = torch.randint(0, K, (R,), generator=g).to(dev)
    fg = torch.randperm(R, generator=g)[:nfg].sort().values.to(dev)
    bdeltas = torch.randn(R, 4 * K, generator=g).to(dev)
    g2, g1 = torch.tensor([1.0, 1.0], device=dev), torch.ones(1, device=dev)
    img = torch.div(pos, A, rounding_mode="floor")
    rows = []
    for loc, beta in (("giou", 0.0), ("smooth_l1", 1.0 / 9)):
        # ---- RPN
        kargs = (logits, rdeltas, pos, neg, midx, gt, gt_off, anchors, rw, 1.0 / (256 * N), loc, beta, SCALE_CLAMP)
        k_f = timed(lambda: hip.rpn_losses_reg(*kargs), args.reps)
        k_b = timed(lambda: hip.rpn_losses_reg(*kargs, gout=g2), args.reps)

        def rpn_torch(d):
            return box_reg_loss_terms(d[pos], anchors[pos - img * A], gt[midx[pos] + gt_off[img]], rw, loc, beta) / (256 * N)

        t_f = timed(lambda: rpn_torch(rdeltas), args.reps)
        leaf = rdeltas.clone().requires_grad_(True)
        loss = rpn_torch(leaf)
        t_b = timed(lambda: torch.autograd.grad(loss, leaf, retain_graph=True), args.reps)
        rows.append(dict(stage="rpn", loss=loc, beta=beta, rows=npos, kernel_fwd_ms=k_f, kernel_bwd_ms=k_b, torch_fwd_ms=t_f, torch_bwd_ms=t_b,
                         kernel_loss=float(hip.rpn_losses_reg(*kargs)[1]), torch_loss=float(loss.detach())))
        # ---- box head
        kargs = (bdeltas, fg, cls, src, tgt, bw, 1.0 / R, loc, beta, SCALE_CLAMP)
        k_f = timed(lambda: hip.box_reg_loss(*kargs), args.reps)
        k_b = timed(lambda: hip.box_reg_loss(*kargs, gout=g1), args.reps)

        def box_torch(d):
            return box_reg_loss_terms(d.view(-1, K, 4)[fg, cls[fg]], src[fg], tgt[fg], bw, loc, beta) / R

        t_f = timed(lambda: box_torch(bdeltas), args.reps)
        leaf = bdeltas.clone().requires_grad_(True)
        loss = box_torch(leaf)
        t_b = timed(lambda: torch.autograd.grad(loss, leaf, retain_graph=True), args.reps)
        rows.append(dict(stage="box_head", loss=loc, beta=beta, rows=nfg, kernel_fwd_ms=k_f, kernel_bwd_ms=k_b, torch_fwd_ms=t_f, torch_bwd_ms=t_b,
                         kernel_loss=float(hip.box_reg_loss(*kargs)[0]), torch_loss=float(loss.detach())))
    for r in rows:
        print({k: (round(v, 4) if isinstance(v, float) else v) for k, v in r.items()}, flush=True)
    print(json.dumps({"device": torch.cuda.get_device_name(0), "reps": args.reps, "rows": rows}))


if __name__ == "__main__":
    main()
