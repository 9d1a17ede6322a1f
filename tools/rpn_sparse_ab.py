#!/usr/bin/env python
"""The RPN head's backward pass, dense against sparse, inside ONE process: CDDMSL_RPN_SPARSE_BWD alternates 0, 1, 0, 1 (the switch is
read per call), one instrumented step of the bench workload per setting (HIP events around every launch).  Prints the rows of the
head's backward launches under each setting -- launches, ms, algorithmic TFLOP/s and TB/s -- the totals of the kernels that are
booked by name only (relu_bwd, colsum, gemm_nt_batched: the head's share is the difference between the settings), and the sum over
all library kernels.  The second repeat of a setting is the yardstick for the difference between the settings.
usage: python tools/rpn_sparse_ab.py [batch] [--dtype bf16]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402


def _head_row(name, shape, positions, cap):
    if name.startswith("rpn_"):
        return True
    if len(shape) < 3:
        return False
    M, N, K = shape[:3]
    return M in (positions, cap) and (N, K) in ((80, 1024), (1024, 80), (1024, 9216))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("batch", nargs="?", type=int, default=16)
    ap.add_argument("--dtype", default="bf16")
    args = ap.parse_args()
    import bench
    from cddmsl_amd import engine, hip, layers, synthetic
    cfg = bench.make_cfg(args.dtype)
    cfg.MODEL.DEVICE = "cuda:0"
    tr = engine.build_trainer(cfg, args.batch, 800, 1333)
    tr.model.load_state_dict(synthetic.make_state_dict(0), strict=False)
    tr.clipcap_model.load_state_dict(synthetic.make_mapper_state_dict(1))
    tr.iter, tr.metrics_period = 20000, 0
    for setting in ("0", "0", "1", "1"):                      # warm both routes
        os.environ["CDDMSL_RPN_SPARSE_BWD"] = setting
        tr.run_step()
    positions = args.batch * 50 * 83
    for rep, setting in enumerate(["0", "1", "0", "1"]):
        os.environ["CDDMSL_RPN_SPARSE_BWD"] = setting
        torch.cuda.synchronize()
        hip.PROFILE.enable()
        tr.run_step()
        bs = hip.PROFILE.by_shape()
        tot = hip.PROFILE.collect()
        cap = tr.model.proposal_generator.sampled_rows
        print(f"=== CDDMSL_RPN_SPARSE_BWD={setting} repeat {rep // 2 + 1}: {positions} positions, {cap} sampled anchors")
        for (name, shape), (n, ms, fl, by) in sorted(bs.items(), key=lambda kv: str(kv[0])):
            if _head_row(name, shape, positions, cap):
                print(f"  {name:18s} {str(shape):38s} n={n:3d} ms={ms:7.3f} TFLOP/s={fl / ms / 1e9 if ms else 0:8.1f} TB/s={by / ms / 1e9 if ms else 0:6.2f}")
        for k in ("relu_bwd", "colsum", "gemm_nt_batched"):
            if k in tot:
                print(f"  total {k:18s} launches={tot[k]['launches']:3d} ms={tot[k]['ms']:7.3f}")
        print("  all library kernels ms:", round(sum(v["ms"] for v in tot.values()), 3), "launches:", sum(v["launches"] for v in tot.values()))
    print("overflow flags:", [int(f.item()) for f in layers.RPN_SPARSE_OVERFLOW.flags()])


if __name__ == "__main__":
    main()
