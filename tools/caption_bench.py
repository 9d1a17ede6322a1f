#!/usr/bin/env python
"""Captioning speed at GPT-2 small geometry (12 x 768, 12 heads, vocabulary 50257) with synthetic weights: ms per decode step and
captions/s at N = 1 / 16 / 64 captions of ``--tokens`` tokens (no stop token) after the 40-row ClipCap prefix, for
  (a) the bf16 path (skinny GEMM, decode attention, LM-head arg-max),
  (b) the same decode with its linears on the conv/GEMM kernel (hip.linear_fwd),
  (c) the reference's algorithm: the full sequence recomputed every step on torch f32 ops (torch_greedy);
and the achieved weight bandwidth of the skinny GEMM at GPT-2's four shapes and of the LM head.  Prints a table and one JSON line.
``--beam-size K`` (K > 1) instead times beam search: ``generate_beam`` with K beams on N captions against greedy ``generate`` at the
same row count N x K, alternated in one process, and ``torch_beam`` (f32, full recompute).

    python tools/caption_bench.py [--tokens 67] [--ns 1,16,64] [--skip-torch] [--beam-size 5 --ns 1,12]
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


def kernel_rates(dec, reps=200):
    from cddmsl_amd import hip
    P = dec._prepared()
    B = P.layers[0]
    rows = []
    for M in (1, 16, 64):
        for name, w, b in (("c_attn", B.w_qkv, B.b_qkv), ("attn.c_proj", B.w_out, B.b_out), ("c_fc", B.w_fc, B.b_fc),
                           ("mlp.c_proj", B.w_proj, B.b_proj)):
            x = torch.randn(M, w.shape[1], device=w.device).to(torch.bfloat16)
            t = timed(lambda: hip.skinny_gemm(x, w, b, epi=0), reps)
            tg = timed(lambda: hip.linear_fwd(x, w, bias=b), reps)
            rows.append({"kernel": "skinny_gemm", "shape": name, "M": M, "N": w.shape[0], "K": w.shape[1], "us": t * 1e6,
                         "TB_s": w.numel() * 2 / t / 1e12, "linear_fwd_us": tg * 1e6})
        h = torch.randn(M, dec.n_embd, device=P.wte.device).to(torch.bfloat16)
        t = timed(lambda: hip.lm_head_argmax(h, P.wte), reps)
        rows.append({"kernel": "lm_head_argmax", "shape": "wte", "M": M, "N": P.wte.shape[0], "K": P.wte.shape[1], "us": t * 1e6,
                     "TB_s": P.wte.numel() * 2 / t / 1e12})
    return rows


def beam_rows(dec, dec32, n, K, T, reps, skip_torch, dev):
    """generate_beam (n captions, K beams) and greedy generate (n * K captions: the same decode-step rows), alternated ``reps`` times"""
    from cddmsl_amd.modeling.gpt2 import torch_beam
    rs = np.random.RandomState(n)
    p = torch.from_numpy((rs.standard_normal((n * K, 40, 768)) * 0.1).astype(np.float32)).to(dev)
    runs = {"beam": lambda t: dec.generate_beam(p[:n], beam_size=K, max_tokens=t), "greedy": lambda t: dec.generate(p, max_tokens=t)}
    acc = {k: [[], []] for k in runs}
    for k, fn in runs.items():                                # warm every shape
        fn(1), fn(T)
    for _ in range(reps):
        for k, fn in runs.items():
            acc[k][0].append(timed(lambda: fn(1), 1))
            acc[k][1].append(timed(lambda: fn(T), 1))
    rows = []
    for k, caps in (("beam", n), ("greedy", n * K)):
        pre, tot = float(np.median(acc[k][0])), float(np.median(acc[k][1]))
        rows.append({"N": caps, "rows": n * K, "route": f"{k} K={K}" if k == "beam" else "greedy", "ms_per_step": (tot - pre) / (T - 1) * 1e3,
                     "prefill_ms": pre * 1e3, "captions_per_s": caps / tot})
    if not skip_torch:
        with torch.no_grad():
            pre = timed(lambda: torch_beam(dec32, p[:n], K, 1), 1)
            tot = timed(lambda: torch_beam(dec32, p[:n], K, T), 1)
        rows.append({"N": n, "rows": n * K, "route": f"torch_beam f32 K={K}", "ms_per_step": (tot - pre) / (T - 1) * 1e3,
                     "prefill_ms": pre * 1e3, "captions_per_s": n / tot})
    return rows


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--tokens", type=int, default=67)
    ap.add_argument("--ns", default="1,16,64")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--skip-torch", action="store_true")
    ap.add_argument("--skip-kernels", action="store_true")
    ap.add_argument("--beam-size", type=int, default=1, help="K > 1: time generate_beam with K beams against greedy generate at N x K rows")
    args = ap.parse_args(argv)
    from cddmsl_amd.modeling.gpt2 import GPT2Decoder, torch_greedy
    from cddmsl_amd.synthetic import make_gpt2_state_dict
    dev = "cuda:0"
    sd = make_gpt2_state_dict(0)
    dec = GPT2Decoder.from_state_dict(sd, torch.bfloat16).to(dev)
    dec32 = GPT2Decoder.from_state_dict(sd, torch.float32).to(dev)
    T = args.tokens
    out = {"tokens": T, "rows": []}
    print(f"{'N':>3} {'route':<28} {'ms/step':>9} {'prefill ms':>10} {'captions/s':>11}")
    if args.beam_size > 1:
        for n in [int(v) for v in args.ns.split(",")]:
            for row in beam_rows(dec, dec32, n, args.beam_size, T, args.reps, args.skip_torch, dev):
                out["rows"].append(row)
                print(f"{row['N']:>3} {row['route']:<28} {row['ms_per_step']:>9.3f} {row['prefill_ms']:>10.2f} {row['captions_per_s']:>11.1f}")
        print(json.dumps(out))
        return
    for n in [int(v) for v in args.ns.split(",")]:
        p = torch.from_numpy((np.random.RandomState(n).standard_normal((n, 40, 768)) * 0.1).astype(np.float32)).to(dev)
        routes = [("a bf16 skinny", dec, "skinny"), ("b bf16 linear_fwd", dec, "gemm")]
        for name, d, lin in routes:
            d.decode_linear = lin
            pre = timed(lambda: d.generate(p, max_tokens=1), args.reps)
            tot = timed(lambda: d.generate(p, max_tokens=T), args.reps)
            row = {"N": n, "route": name, "ms_per_step": (tot - pre) / (T - 1) * 1e3, "prefill_ms": pre * 1e3, "captions_per_s": n / tot}
            out["rows"].append(row)
            print(f"{n:>3} {name:<28} {row['ms_per_step']:>9.3f} {row['prefill_ms']:>10.2f} {row['captions_per_s']:>11.1f}")
        dec.decode_linear = "skinny"
        if not args.skip_torch:
            with torch.no_grad():
                pre = timed(lambda: torch_greedy(dec32, p, max_tokens=1), 1)
                tot = timed(lambda: torch_greedy(dec32, p, max_tokens=T), 1)
            row = {"N": n, "route": "c f32 full recompute (torch)", "ms_per_step": (tot - pre) / (T - 1) * 1e3, "prefill_ms": pre * 1e3,
                   "captions_per_s": n / tot}
            out["rows"].append(row)
            print(f"{n:>3} {row['route']:<28} {row['ms_per_step']:>9.3f} {row['prefill_ms']:>10.2f} {row['captions_per_s']:>11.1f}")
    if not args.skip_kernels:
        out["kernels"] = kernel_rates(dec)
        print(f"{'kernel':<15} {'shape':<12} {'M':>3} {'N':>6} {'K':>5} {'us':>8} {'TB/s':>6} {'linear_fwd us':>14}")
        for r in out["kernels"]:
            print(f"{r['kernel']:<15} {r['shape']:<12} {r['M']:>3} {r['N']:>6} {r['K']:>5} {r['us']:>8.2f} {r['TB_s']:>6.2f} "
                  f"{r.get('linear_fwd_us', float('nan')):>14.2f}")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
