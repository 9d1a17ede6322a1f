#!/usr/bin/env python
"""Record every distinct GEMM / convolution launch of one bench-shaped bf16 training step (16 and 32 images of 800x1333, built like
tools/shape_profile.py): a recording shim around ``hip.conv_fwd``, ``hip.conv_wgrad``, ``hip.gemm_nt_batched`` and
``hip.gemm_tn_batched`` notes each call's entry point, full geometry, epilogue flags and the kernel the library picked
(``cddmsl_last_kernel``).  Writes tests/golden/bench_gemm_launches.json, which tests/test_gpu_gemm_exact.py replays in plan-only mode
(dispatch still picks the recorded kernel) and tests/test_exact_bound_host.py checks against the exact-product case table.
A change of dispatch or of the step's shapes must re-record it.  usage: python tools/record_gemm_launches.py [--stock] [--dtype bf16|f32|fp8] [--batches 16 32] [--out F]
With ``--dtype fp8`` the shim also notes ``hip.conv_fwd_fp8``, ``hip.conv_wgrad_fp8`` and ``hip.fp8_dot_nt``, keeps only those and the
``hip.conv_fwd`` calls that write an e4m3 second output (``emit8``), and writes tests/golden/bench_fp8_launches.json (the case table of
tests/fp8_exact_cases.py is checked against it by tests/test_fp8_bound_host.py); the bf16 file is not touched.
With ``--stock`` the step is the stock configuration's instead (configs/PascalVOC-Detection/faster_rcnn_R_50_C4.yaml: Detectron2's
R50-C4 of cddmsl_amd/modeling/resnet.py -- the 7x7 stem, the stride in a block's first 1x1 -- with Res5ROIHeads; one supervised forward
and backward pass of the model in bf16 on the same 800x1333 images, 16 of them unless --batches says otherwise) and the file
tests/golden/stock_gemm_launches.json, same format, read by the same tests.
With ``--dtype f32`` (alone or with ``--stock``) the step runs the f32 instantiations -- the parity path the oracle tests of
tests/test_gpu_e2e.py and tests/test_gpu_golden.py hold to the reference -- on ONE 800x1333 image unless --batches says otherwise (the size
of test_full_size_step_matches_oracle), and the files are tests/golden/bench_gemm_launches_f32.json and stock_gemm_launches_f32.json."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "bench_gemm_launches.json")
OUT_FP8 = os.path.join(ROOT, "tests", "golden", "bench_fp8_launches.json")
OUT_STOCK = os.path.join(ROOT, "tests", "golden", "stock_gemm_launches.json")
OUT_F32 = os.path.join(ROOT, "tests", "golden", "bench_gemm_launches_f32.json")
OUT_STOCK_F32 = os.path.join(ROOT, "tests", "golden", "stock_gemm_launches_f32.json")
STOCK_YAML = os.path.join(ROOT, "configs", "PascalVOC-Detection", "faster_rcnn_R_50_C4.yaml")


def _dt(t):
    return {torch.bfloat16: "bf16", torch.float32: "f32"}[t.dtype]


class Recorder:
    def __init__(self, hip):
        self.hip, self.on, self.calls, self.batch = hip, False, {}, 0
        self.orig = {n: getattr(hip, n) for n in ("conv_fwd", "conv_wgrad", "gemm_nt_batched", "gemm_tn_batched",
                                                     "conv_fwd_fp8", "conv_wgrad_fp8", "fp8_dot_nt")}
        for n in self.orig:
            setattr(hip, n, self._wrap(n))

    def restore(self):
        for n, f in self.orig.items():
            setattr(self.hip, n, f)

    def _note(self, entry, geom, flags, nbytes, kid=None):
        # (kid given: an entry point with one kernel behind it; fp8_dot_nt does not go through the conv / GEMM dispatch: 0)
        kid = int(self.hip._L().cddmsl_last_kernel()) if kid is None else kid
        key = json.dumps([self.batch, entry, geom, flags, kid], sort_keys=True)
        d = self.calls.setdefault(key, {"images": self.batch, "entry": entry, "geometry": geom, "epilogue": flags, "kernel_id": kid,
                                        "kernel": self.hip._CONV_KERNEL.get(kid, "k_fp8_dot_nt" if entry == "fp8_dot_nt" else "?"), "launches": 0, "max_operand_bytes": 0})
        d["launches"] += 1
        d["max_operand_bytes"] = max(d["max_operand_bytes"], int(nbytes))

    def _wrap(self, name):
        f = self.orig[name]
        rec = self

        def conv_fwd(x, w, scale=None, bias=None, residual=None, relu=False, relu_mask=None, stride=1, pad=0, pool=False,
                     out_f32=False, residual_pooled=False, emit8=None, out_spec=None):
            y = f(x, w, scale, bias, residual, relu, relu_mask, stride, pad, pool, out_f32, residual_pooled, emit8, out_spec)
            if rec.on:
                N, H, W, Cin = x.shape
                Cout, KH, KW, _ = w.shape
                res = None if residual is None else ("pooled" if residual_pooled else _dt(residual))
                rec._note("conv_fwd", dict(N=N, H=H, W=W, Cin=Cin, Cout=Cout, KH=KH, KW=KW, stride=stride, pad=pad, pool=bool(pool),
                                           ldy=Cout, dtype=_dt(x)),
                          dict(scale=scale is not None, bias=bias is not None, residual=res, relu=bool(relu),
                               relu_mask=relu_mask is not None, out_f32=bool(out_f32), emit8=emit8 is not None),
                          max(x.numel() * x.element_size(), y.numel() * y.element_size()))
            return y

        def conv_wgrad(x, dy, w_shape, scale=None, stride=1, pad=0, pool=False, out=None):
            r = f(x, dy, w_shape, scale, stride, pad, pool, out)
            if rec.on:
                N, H, W, Cin = x.shape
                Cout, KH, KW, _ = w_shape
                rec._note("conv_wgrad", dict(N=N, H=H, W=W, Cin=Cin, Cout=Cout, KH=KH, KW=KW, stride=stride, pad=pad, pool=bool(pool),
                                             ldd=Cout, dtype=_dt(x)),
                          dict(scale=scale is not None, accumulate=out is not None),
                          max(x.numel() * x.element_size(), dy.numel() * dy.element_size()))
            return r

        def gemm_nt_batched(a, w, c, M, N, K, lda, ldb, ldc, batch, sa, sw, sc, a_off=0, w_off=0, c_off=0, bias=None):
            r = f(a, w, c, M, N, K, lda, ldb, ldc, batch, sa, sw, sc, a_off, w_off, c_off, bias)
            if rec.on:
                rec._note("gemm_nt_batched", dict(M=M, N=N, K=K, lda=lda, ldb=ldb, ldc=ldc, batch=batch, sa=sa, sw=sw, sc=sc, dtype=_dt(a)),
                          dict(bias=bias is not None, out_f32=c.dtype == torch.float32 and a.dtype != torch.float32),
                          max(a.numel() * a.element_size(), c.numel() * c.element_size()))
            return r

        def gemm_tn_batched(a, b, out, M, N, K, lda, ldb, ldo, batch, sa, sb, so, a_off=0, b_off=0, o_off=0, accumulate=False):
            r = f(a, b, out, M, N, K, lda, ldb, ldo, batch, sa, sb, so, a_off, b_off, o_off, accumulate)
            if rec.on:
                rec._note("gemm_tn_batched", dict(M=M, N=N, K=K, lda=lda, ldb=ldb, ldo=ldo, batch=batch, sa=sa, sb=sb, so=so, dtype=_dt(a)),
                          dict(accumulate=bool(accumulate), out=_dt(out)),
                          max(a.numel() * a.element_size(), b.numel() * b.element_size()))
            return r

        def conv_fwd_fp8(x8, w8, scale=None, bias=None, residual=None, relu=False, relu_mask=None, pad=0, out_f32=False, emit8=None):
            y = f(x8, w8, scale, bias, residual, relu, relu_mask, pad, out_f32, emit8)
            if rec.on:
                N, H, W, Cin = x8.shape
                Cout, KH, KW, _ = w8.shape
                rec._note("conv_fwd_fp8", dict(N=N, H=H, W=W, Cin=Cin, Cout=Cout, KH=KH, KW=KW, stride=1, pad=pad, pool=False, ldy=Cout,
                                               dtype="e4m3"),
                          dict(scale=scale is not None, bias=bias is not None, residual=None if residual is None else _dt(residual),
                               relu=bool(relu), relu_mask=relu_mask is not None, out_f32=bool(out_f32), emit8=emit8 is not None),
                          max(x8.numel(), y.numel() * y.element_size()), kid=10)
            return y

        def conv_wgrad_fp8(x8, dy8, w_shape, scale, pad=0, out=None):
            r = f(x8, dy8, w_shape, scale, pad, out)
            if rec.on:
                N, H, W, Cin = x8.shape
                Cout, KH, KW, _ = w_shape
                rec._note("conv_wgrad_fp8", dict(N=N, H=H, W=W, Cin=Cin, Cout=Cout, KH=KH, KW=KW, stride=1, pad=pad, pool=False, ldd=Cout,
                                                 dtype="e4m3"),
                          dict(scale=scale is not None, accumulate=out is not None), max(x8.numel(), dy8.numel()), kid=12)
            return r

        def fp8_dot_nt(a8, b8, alpha=None):
            r = f(a8, b8, alpha)
            if rec.on:
                rec._note("fp8_dot_nt", dict(R=a8.shape[0], N=b8.shape[0], K=a8.shape[1], ldc=b8.shape[0], dtype="e4m3"),
                          dict(alpha=alpha is not None), a8.numel(), kid=0)
            return r

        return locals()[name]


def record_bench(rec, batches, dtype):
    """one bench-shaped training step per batch size, the second one recorded"""
    import bench
    from cddmsl_amd import engine, synthetic
    for batch in batches:
        cfg = bench.make_cfg(dtype)
        cfg.MODEL.DEVICE = "cuda:0"
        tr = engine.build_trainer(cfg, batch, 800, 1333)
        tr.model.load_state_dict(synthetic.make_state_dict(0), strict=False)
        tr.clipcap_model.load_state_dict(synthetic.make_mapper_state_dict(1))
        tr.iter, tr.metrics_period = 20000, 0
        tr.run_step()                      # (first step: lazy weight copies and buffers)
        torch.cuda.synchronize()
        rec.batch, rec.on = batch, True
        tr.run_step()
        torch.cuda.synchronize()
        rec.on = False
        del tr
        torch.cuda.empty_cache()


def record_stock(rec, batches, dtype):
    """one supervised step (forward + backward of the model) of the stock configuration per batch size, the second one recorded"""
    from cddmsl_amd import synthetic
    from cddmsl_amd.config import get_cfg
    from cddmsl_amd.modeling import build_model
    for batch in batches:
        cfg = get_cfg()
        cfg.merge_from_file(STOCK_YAML)
        cfg.merge_from_list(["MODEL.COMPUTE_DTYPE", dtype, "MODEL.DEVICE", "cuda:0"])
        model = build_model(cfg)
        model.load_state_dict(synthetic.make_state_dict_r50(0), strict=False)
        model.train()
        for it in range(2):
            rec.batch, rec.on = batch, it == 1           # (first step: lazy weight copies and buffers)
            model.zero_grad(set_to_none=True)
            sum(model(synthetic.make_batch(batch, 800, 1333, iteration=it)).values()).backward()
            torch.cuda.synchronize()
        rec.on = False
        del model
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=None)
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--stock", action="store_true", help="record the stock R50-C4 configuration's step (bf16 or f32) instead of the bench's")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    fp8 = args.dtype == "fp8"
    f32 = args.dtype == "f32"
    assert not (args.stock and fp8), "--stock records the bf16 or the f32 step"
    args.batches = args.batches or ([1] if f32 else [16] if args.stock else [16, 32])
    args.out = args.out or ((OUT_STOCK_F32 if f32 else OUT_STOCK) if args.stock else OUT_FP8 if fp8 else OUT_F32 if f32 else OUT)
    from cddmsl_amd import hip
    rec = Recorder(hip)
    if args.stock:
        record_stock(rec, args.batches, args.dtype)
    else:
        record_bench(rec, args.batches, args.dtype)
    rec.restore()
    calls = [d for d in rec.calls.values() if not fp8 or d["geometry"]["dtype"] == "e4m3" or d["epilogue"].get("emit8")]
    entries = sorted(calls, key=lambda d: (d["images"], d["entry"], d["kernel_id"], json.dumps(d["geometry"], sort_keys=True),
                                                        json.dumps(d["epilogue"], sort_keys=True)))
    about = "distinct GEMM / convolution launches of one bench-shaped training step (tools/record_gemm_launches.py)"
    if args.stock:
        about = "distinct GEMM / convolution launches of one supervised step of the stock R50-C4 configuration (tools/record_gemm_launches.py --stock)"
    doc = {"about": about, "dtype": args.dtype, "images": args.batches, "entries": entries}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(doc, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(f"{len(entries)} distinct launches -> {args.out}")
    for d in entries:
        print(d["images"], d["entry"], d["kernel"], d["launches"], d["geometry"], d["epilogue"])


if __name__ == "__main__":
    main()
