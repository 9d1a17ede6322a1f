#!/usr/bin/env python
"""Optimizer-step speed on the real model's trainable parameter list (configs/VOC-Experiments/faster_rcnn_CLIP_R_50_C4.yaml: the
shapes of GeneralizedRCNN's trainable parameters; values are random): hip.sgd_clip_step (the step every shipped config takes)
against hip.sgd_step_groups in each clip mode, with per-tensor lr / weight decay and Nesterov momentum.  The variants alternate
inside one process, one call each per round after a warm-up, each call timed with device events; per variant the median, the
10th and 90th percentile over the rounds and the achieved GB/s of the median.  Bytes come from the shapes: p, m read and written,
g read once (5 N x 4) for none / value, g read twice (6 N x 4) for the norm modes and sgd_clip_step.  Gradients are views packed
back to back into one flat buffer, parameters and momentum buffers separate tensors, as in training.  Prints a table and one JSON line.
``--average`` times the weight averaging that follows the step under MODEL_EMA instead: hip.weight_average (avg read and written, p
read: 3 N x 4) against ``torch._foreach_lerp_`` on the same tensors (the same expression, one launch per chunk of tensors), next to
the grouped step it follows.  Each is timed twice: as above, on an idle device, where the window between the two events also holds
the host's work to prepare the launch (for the ctypes wrappers the pointer arrays of 63 tensors, tens of microseconds in which the device
waits), and "queued" behind a few milliseconds of matrix products issued just before the first event, so that the launch is
already in the queue when the device gets to it and the window holds the device's time alone -- the situation in training, where
the host runs ahead of the device.  The JSON line also holds the two ratios, from the queued times.

    python tools/optimizer_bench.py [--rounds 200] [--warmup 20] [--average]
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
    ap.add_argument("--average", action="store_true", help="time hip.weight_average against torch._foreach_lerp_ and the grouped step")
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
    if args.average:
        es, et = [p.clone() for p in ps], [p.clone() for p in ps]
        w = 1.0 - 0.999
        variants = [("weight_average", 3, lambda: hip.weight_average(es, ps, w, False)),
                    ("torch._foreach_lerp_", 3, lambda: torch._foreach_lerp_(et, ps, w)),
                    ("weight_average copy", 2, lambda: hip.weight_average(es, ps, 0.0, True)),
                    ("torch._foreach_copy_", 2, lambda: torch._foreach_copy_(et, ps)),
                    ("sgd_step_groups none", 5, lambda: hip.sgd_step_groups(ps, gs, ms, ws, [lr * 1e-2 for lr in lrs], wds, mo, True, 0, clip, False))]
    queued = set()
    if args.average:                                             # every variant a second time, behind work that hides the host's share
        block = torch.randn(8192, 8192, device=dev, generator=gen).bfloat16()
        queued = {name + " queued" for name, _, _ in variants}
        variants = variants + [(name + " queued", passes, fn) for name, passes, fn in variants]
    times = {name: [] for name, _, _ in variants}
    for r in range(args.warmup + args.rounds):
        for name, _, fn in variants:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            if name in queued:
                for _ in range(3):
                    torch.mm(block, block)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if r >= args.warmup:
                times[name].append(e0.elapsed_time(e1))
    assert all(bool(torch.isfinite(p).all()) for p in ps[:4])
    print(f"{len(ps)} tensors, {N} f32 elements ({N * 4 / 1e6:.1f} MB of parameters), {args.rounds} rounds")
    print(f"{'variant':34s} {'median ms':>10s} {'p10':>8s} {'p90':>8s} {'GB/s':>8s}")
    out = {"tensors": len(ps), "elements": N, "rounds": args.rounds, "variants": {}}
    for name, passes, _ in variants:
        t = sorted(times[name])
        med, p10, p90 = t[len(t) // 2], t[len(t) // 10], t[(9 * len(t)) // 10]
        gbs = passes * N * 4 / (med * 1e-3) / 1e9
        print(f"{name:34s} {med:10.4f} {p10:8.4f} {p90:8.4f} {gbs:8.0f}")
        out["variants"][name] = {"ms_median": med, "ms_p10": p10, "ms_p90": p90, "bytes": passes * N * 4, "gb_per_s": gbs}
    if args.average:
        med = {k[:-len(" queued")]: v["ms_median"] for k, v in out["variants"].items() if k in queued}
        out["average_over_foreach_lerp"] = med["weight_average"] / med["torch._foreach_lerp_"]
        out["average_over_step"] = med["weight_average"] / med["sgd_step_groups none"]
        print(f"queued: weight_average / torch._foreach_lerp_ {out['average_over_foreach_lerp']:.3f}, / sgd_step_groups none {out['average_over_step']:.3f}")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
