#!/usr/bin/env python
"""Optimizer-step speed on the real model's trainable parameter list (configs/VOC-Experiments/faster_rcnn_CLIP_R_50_C4.yaml: the
shapes of GeneralizedRCNN's trainable parameters; values are random): hip.sgd_clip_step (the step every shipped config takes)
against hip.sgd_step_groups in each clip mode, with per-tensor lr / weight decay and Nesterov momentum.  The variants alternate
inside one process, one call each per round after a warm-up, each call timed with device events; per variant the median, the
10th and 90th percentile over the rounds and the achieved GB/s of the median.  Bytes come from the shapes: p, m read and written,
g read once (5 N x 4) for none / value, g read twice (6 N x 4) for the norm modes and sgd_clip_step.  Gradients are views packed
back to back into one flat buffer, parameters and momentum buffers separate tensors, as in training.  Prints a table and one JSON line.

    python tools/optimizer_bench.py [--rounds 200] [--warmup 20]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    args = ap.parse_args()
    from cddmsl_amd import hip
    from cddmsl_amd.config import get_cfg
    from cddmsl_amd.modeling.rcnn import GeneralizedRCNN
    from cddmsl_amd.solver import get_default_optimizer_params
    assert torch.cuda.is_available(), "optimizer_bench needs the GPU: a CPU run gives no time"
    cfg = get_cfg()
    cfg.merge_from_file(os.path.join(ROOT, "configs", "VOC-Experiments", "faster_rcnn_CLIP_R_50_C4.yaml"))
    model = GeneralizedRCNN(cfg)                                  # on the CPU: only the shapes and the groups are used
    groups = get_default_optimizer_params(model, base_lr=cfg.SOLVER.BASE_LR, weight_decay=cfg.SOLVER.WEIGHT_DECAY, weight_decay_norm=0.0,
                                          bias_lr_factor=2.0, weight_decay_bias=0.0)
    shapes = [tuple(g["params"][0].shape) for g in groups]
    lrs, wds = [g["lr"] for g in groups], [g["weight_decay"] for g in groups]
    del model
    dev = "cuda"
    gen = torch.Generator(device=dev).manual_seed(1)
    sizes = [int(torch.Size(s).numel()) for s in shapes]
    N = sum(sizes)
    flat_g = torch.randn(N, device=dev, generator=gen) * 1e-2
    ps = [torch.randn(n, device=dev, generator=gen) for n in sizes]
    gs, off = [], 0
    for n in sizes:
        gs.append(flat_g[off:off + n])
        off += n
    ms = [torch.zeros_like(p) for p in ps]
    ws = torch.zeros(len(ps), device=dev)
    mo, clip = cfg.SOLVER.MOMENTUM, 5.0
    variants = [("sgd_clip_step", 6, lambda: hip.sgd_clip_step(ps, gs, ms, ws, 1e-4, mo, 1e-4, clip, False))]
    for name, mode in hip.SGD_CLIP_MODES.items():
        variants.append((f"sgd_step_groups {name}", 6 if mode >= 2 else 5,
                         lambda mode=mode: hip.sgd_step_groups(ps, gs, ms, ws, [lr * 1e-2 for lr in lrs], wds, mo, True, mode, clip, False)))
    times = {name: [] for name, _, _ in variants}
    for r in range(args.warmup + args.rounds):
        for name, _, fn in variants:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if r >= args.warmup:
                times[name].append(e0.elapsed_time(e1))
    assert all(bool(torch.isfinite(p).all()) for p in ps[:4])
    print(f"{len(ps)} tensors, {N} f32 elements ({N * 4 / 1e6:.1f} MB of parameters), {args.rounds} rounds")
    print(f"{'variant':28s} {'median ms':>10s} {'p10':>8s} {'p90':>8s} {'GB/s':>8s}")
    out = {"tensors": len(ps), "elements": N, "rounds": args.rounds, "variants": {}}
    for name, passes, _ in variants:
        t = sorted(times[name])
        med, p10, p90 = t[len(t) // 2], t[len(t) // 10], t[(9 * len(t)) // 10]
        gbs = passes * N * 4 / (med * 1e-3) / 1e9
        print(f"{name:28s} {med:10.4f} {p10:8.4f} {p90:8.4f} {gbs:8.0f}")
        out["variants"][name] = {"ms_median": med, "ms_p10": p10, "ms_p90": p90, "bytes": passes * N * 4, "gb_per_s": gbs}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
