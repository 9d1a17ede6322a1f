#!/usr/bin/env python
"""Times the CLIP text encoder (cddmsl_amd/modeling/text_encoder.py) as tools/extract_concept_features.py uses it:
``encode_prompt_ids`` for C classes x P prompts of synthetic class names, C = 20 (VOC) and 1203 (LVIS), P = 80, on synthetic RN50
weights, in bf16 and f32; against the torch-f32 restatement (``torch_encode_text``, the same function on plain torch ops on the
GPU, full batches at the same truncated T); and truncated (T = max(eot) + 1 per chunk) against full 77-token batches.  Reports
ms, tokens/s (prompt tokens up to and including the EOT) and the fraction of the bf16 MFMA peak taken by the GEMM FLOPs actually
run.  Tokenization (CPU) is timed separately.  One JSON object per line.

usage (GPU box): python tools/text_encoder_bench.py [--classes 20 1203] [--prompts 80] [--reps 3]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

BF16_PEAK = 2.5e15        # MI355X dense bf16 MFMA peak, FLOP/s


def synthetic_prompts(C, P, seed=0):
    """C class names of 1-3 words drawn from a small word list, P templates of 5-9 words: about 18 tokens per prompt"""
    g = torch.Generator().manual_seed(seed)
    words = ("red green small large wooden metal old new toy car bird boat chair table lamp sign light tower bottle cup dog horse "
             "train plane bicycle person rider truck bus motorcycle street house tree flower kite ball phone screen door window").split()
    adj = ("good bad bright dark blurry clean dirty cropped close-up pixelated jpeg corrupted black white plastic cartoon sketch "
           "drawing painting rendering origami toy plushie embroidered tattoo graffiti").split()

    def pick(seq, k):
        return [seq[int(i)] for i in torch.randint(0, len(seq), (k,), generator=g)]

    names = [" ".join(pick(words, 1 + int(torch.randint(0, 3, (1,), generator=g)))) for _ in range(C)]
    templates = [" ".join(["a"] + pick(adj, 1 + int(torch.randint(0, 5, (1,), generator=g))) + ["photo of the {}."]) for _ in range(P)]
    return names, templates


def vocab_file(path, names, templates):
    """a toy BPE vocab in which every word of the prompts merges into one token, as common English words do in CLIP's (the ids
    need not be CLIP's: the weights are synthetic)"""
    import gzip
    merges = []
    for w in sorted(set(" ".join(names + templates).lower().replace("{}", " ").replace(".", " ").split())):
        syms = list(w[:-1]) + [w[-1] + "</w>"]
        while len(syms) > 1:
            m = f"{syms[0]} {syms[1]}"
            if m not in merges:
                merges.append(m)
            syms = [syms[0] + syms[1]] + syms[2:]
    with gzip.open(path, "wt", encoding="utf-8") as f:
        f.write("#version: 0.2\n" + "\n".join(merges) + "\n")


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    best = float("inf")
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        best = min(best, time.perf_counter() - t0)
    return best * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--classes", type=int, nargs="+", default=[20, 1203])
    ap.add_argument("--prompts", type=int, default=80)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--chunk", type=int, default=8192)
    ap.add_argument("--no-torch", action="store_true", help="skip the torch-f32 restatement")
    args = ap.parse_args()
    import tempfile
    from cddmsl_amd.clip_text import BPETokenizer
    from cddmsl_amd.modeling.text_encoder import gemm_flops, load_text_encoder, tokenize_names, torch_encode_text
    dev = torch.device("cuda:0")
    encs = {d: load_text_encoder(synthetic_seed=0, compute_dtype=d).to(dev) for d in (torch.bfloat16, torch.float32)}
    W, L, D = 512, 12, 1024
    for C in args.classes:
        names, templates = synthetic_prompts(C, args.prompts)
        with tempfile.TemporaryDirectory() as td:
            vocab_file(os.path.join(td, "v.gz"), names, templates)
            bpe = BPETokenizer.from_vocab_file(os.path.join(td, "v.gz"))
        t0 = time.perf_counter()
        ids, counts = tokenize_names(names, templates, bpe)
        tok_ms = (time.perf_counter() - t0) * 1e3
        S = ids.shape[0]
        eot = ids.argmax(-1)
        tokens = int((eot + 1).sum())
        # the T each chunk runs at (whole classes per chunk, as encode_prompt_ids does)
        per = max(1, args.chunk // args.prompts) * args.prompts
        t_chunks = [(min(S, s + per) - s, int(eot[s:s + per].max()) + 1) for s in range(0, S, per)]
        flops_trunc = sum(gemm_flops(n, t, W, L, 0) for n, t in t_chunks) + 2 * C * W * D
        flops_full = gemm_flops(S, 77, W, L, 0) + 2 * C * W * D
        rows = {"classes": C, "prompts": args.prompts, "sequences": S, "tokens": tokens, "T_chunks": sorted({t for _, t in t_chunks}),
                "tokenize_ms": round(tok_ms, 1)}
        out = {}
        for name, d in (("bf16", torch.bfloat16), ("f32", torch.float32)):
            enc = encs[d]
            with torch.no_grad():
                ms = timed(lambda: enc.encode_prompt_ids(ids, counts, chunk=args.chunk), args.reps)
                ms_full = timed(lambda: enc.encode_prompt_ids(ids, counts, chunk=args.chunk, truncate=False), max(1, args.reps - 2))
                out[name] = enc.encode_prompt_ids(ids, counts, chunk=args.chunk)
            rows[name] = {"ms": round(ms, 2), "tokens_per_s": round(tokens / ms * 1e3), "gemm_tflop": round(flops_trunc / 1e12, 2),
                          "frac_bf16_peak": round(flops_trunc / (ms * 1e-3) / BF16_PEAK, 4), "ms_full77": round(ms_full, 2),
                          "gemm_tflop_full77": round(flops_full / 1e12, 2), "truncation_speedup": round(ms_full / ms, 2)}
        if not args.no_torch:
            enc = encs[torch.float32]

            def torch_run():
                res = torch.empty((C, D), device=dev)
                pc = args.prompts
                for c0 in range(0, C, per // pc):
                    c1 = min(C, c0 + per // pc)
                    res[c0:c1] = torch_encode_text(enc, ids[c0 * pc:c1 * pc]).view(c1 - c0, pc, D).mean(1)
                return res
            with torch.no_grad():
                ms_t = timed(torch_run, max(1, args.reps - 2))
                ref = torch_run()
            rows["torch_f32"] = {"ms": round(ms_t, 2), "speedup_bf16": round(ms_t / rows["bf16"]["ms"], 2),
                                 "speedup_f32": round(ms_t / rows["f32"]["ms"], 2)}
            for name in ("bf16", "f32"):
                rows[name]["rel_vs_torch_f32"] = float(f"{float((out[name] - ref).abs().max() / ref.abs().max()):.3e}")
        print(json.dumps(rows), flush=True)


if __name__ == "__main__":
    main()
