#!/usr/bin/env python
"""Mapper-training speed at the workload's own size -- batch 40, prefix 40, 40 caption tokens, 8 mapper layers, GPT-2 small (12 x 768,
vocabulary 50257), bf16, synthetic weights: ms per training step of tools/train_clipcap.py's loop and of its parts (the mapper forward +
backward, ``caption_loss`` forward + backward, AdamW), against the same model composed from torch ops under autograd on the same GPU
(``torch_gpt2_logits``, a plain torch mapper, ``F.cross_entropy``, ``torch.optim.AdamW(fused=True)``; bf16 autocast, f32 logits), and
the peak memory of both.  A warm-up, then the median of ``--blocks`` timed blocks of ``--reps`` steps each; the parts are timed with
a synchronisation around each.  Prints a table and one JSON line that names the device.

    python tools/clipcap_train_bench.py [--bs 40] [--blocks 5] [--reps 5] [--skip-torch]
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
import torch.nn.functional as F  # noqa: E402
from torch import nn  # noqa: E402


def median_ms(fn, blocks, reps):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(blocks):
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) / reps * 1e3)
    return float(np.median(out))


class TorchMapper(nn.Module):
    """clipcap.py's TransformerMapper on torch modules, the state dict's names"""

    def __init__(self, sd, dim_clip=1024, d=768, P=40, layers=8):
        super().__init__()
        self.P, self.d, self.nl = P, d, layers
        self.p = nn.ParameterDict({k.replace(".", "/"): nn.Parameter(v.clone()) for k, v in sd.items()})

    def forward(self, x):
        g = lambda k: self.p[k.replace(".", "/")]      # noqa: E731
        n, d, H = x.shape[0], self.d, 8
        h = torch.cat((F.linear(x, g("linear.weight"), g("linear.bias")).view(n, self.P, d), g("prefix_const").unsqueeze(0).expand(n, -1, -1)), 1)
        t = h.shape[1]
        for i in range(self.nl):
            q_ = f"transformer.layers.{i}."
            y = F.layer_norm(h, (d,), g(q_ + "norm1.weight"), g(q_ + "norm1.bias"))
            q = F.linear(y, g(q_ + "attn.to_queries.weight")).view(n, t, H, d // H).transpose(1, 2)
            k, v = F.linear(y, g(q_ + "attn.to_keys_values.weight")).view(n, t, 2, H, d // H).permute(2, 0, 3, 1, 4)
            o = F.scaled_dot_product_attention(q, k, v).transpose(1, 2).reshape(n, t, d)
            h = h + F.linear(o, g(q_ + "attn.project.weight"), g(q_ + "attn.project.bias"))
            y = F.layer_norm(h, (d,), g(q_ + "norm2.weight"), g(q_ + "norm2.bias"))
            h = h + F.linear(F.relu(F.linear(y, g(q_ + "mlp.fc1.weight"), g(q_ + "mlp.fc1.bias"))), g(q_ + "mlp.fc2.weight"), g(q_ + "mlp.fc2.bias"))
        return h[:, self.P:]


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--bs", type=int, default=40)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--skip-torch", action="store_true")
    args = ap.parse_args(argv)
    from cddmsl_amd.modeling import TransformerMapper
    from cddmsl_amd.modeling.gpt2 import GPT2Decoder, torch_gpt2_logits
    from cddmsl_amd.solver import AdamW
    from cddmsl_amd.synthetic import make_gpt2_state_dict, make_mapper_state_dict
    dev, P, L, n = "cuda:0", 40, 40, args.bs
    gsd, msd = make_gpt2_state_dict(0), make_mapper_state_dict(1)
    rs = np.random.RandomState(0)
    x = torch.from_numpy(rs.standard_normal((n, 1024)).astype(np.float32)).to(dev)
    tokens = torch.from_numpy(rs.randint(1, 50257, (n, L))).to(dev)
    tokens[:, 30:] = torch.where(torch.arange(n, device=dev)[:, None] % 2 == 0, tokens[:, 30:], torch.zeros_like(tokens[:, 30:]))   # half padded
    out = {"device": torch.cuda.get_device_name(0), "bs": n, "prefix": P, "tokens": L, "blocks": args.blocks, "reps": args.reps}

    dec = GPT2Decoder.from_state_dict(gsd, torch.bfloat16).to(dev)
    mapper = TransformerMapper(1024, 768, P, P, 8, compute_dtype=torch.bfloat16, trainable=True)
    mapper.load_state_dict(msd)
    mapper.to(dev)
    opt = AdamW(list(mapper.parameters()), lr=2e-5, eps=1e-6, weight_decay=0.0)

    def hip_step():
        opt.zero_grad()
        dec.caption_loss(mapper(x), tokens).backward()
        opt.step()

    def hip_mapper():
        opt.zero_grad()
        mapper(x).sum().backward()

    pre = mapper(x).detach()

    def hip_loss():
        p = pre.clone().requires_grad_(True)
        dec.caption_loss(p, tokens).backward()

    torch.cuda.reset_peak_memory_stats()
    out["hip"] = {"step_ms": median_ms(hip_step, args.blocks, args.reps), "peak_GiB": torch.cuda.max_memory_allocated() / 2 ** 30,
                  "mapper_fwd_bwd_ms": median_ms(hip_mapper, args.blocks, args.reps), "caption_loss_fwd_bwd_ms": median_ms(hip_loss, args.blocks, args.reps),
                  "adamw_ms": median_ms(opt.step, args.blocks, args.reps)}
    if not args.skip_torch:
        del opt
        mapper.cpu()
        dec32 = GPT2Decoder.from_state_dict(gsd, torch.float32).to(dev)
        tm = TorchMapper(msd).to(dev)
        topt = torch.optim.AdamW(tm.parameters(), lr=2e-5, eps=1e-6, weight_decay=0.0, fused=True)
        wte = dec32.wte.weight

        def t_loss(prefix):
            with torch.autocast("cuda", dtype=torch.bfloat16):
                lg = torch_gpt2_logits(dec32, torch.cat((prefix, wte[tokens]), 1), torch.float32)[:, P - 1:-1]
            return F.cross_entropy(lg.float().reshape(-1, lg.shape[-1]), tokens.flatten(), ignore_index=0)

        def t_step():
            topt.zero_grad()
            with torch.autocast("cuda", dtype=torch.bfloat16):
                prefix = tm(x)
            t_loss(prefix.float()).backward()
            topt.step()

        def t_mapper():
            topt.zero_grad()
            with torch.autocast("cuda", dtype=torch.bfloat16):
                tm(x).float().sum().backward()

        def t_l():
            t_loss(pre.clone().requires_grad_(True)).backward()

        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        out["torch"] = {"step_ms": median_ms(t_step, args.blocks, args.reps), "peak_GiB": torch.cuda.max_memory_allocated() / 2 ** 30,
                        "resident_before_GiB": base / 2 ** 30, "mapper_fwd_bwd_ms": median_ms(t_mapper, args.blocks, args.reps),
                        "caption_loss_fwd_bwd_ms": median_ms(t_l, args.blocks, args.reps), "adamw_ms": median_ms(topt.step, args.blocks, args.reps)}
    print(f"{out['device']}: batch {n}, prefix {P}, {L} tokens, bf16; median of {args.blocks} blocks x {args.reps}")
    for k in ("step_ms", "mapper_fwd_bwd_ms", "caption_loss_fwd_bwd_ms", "adamw_ms", "peak_GiB"):
        print(f"{k:<26} hip {out['hip'][k]:>9.3f}" + (f"   torch {out['torch'][k]:>9.3f}" if "torch" in out else ""))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
