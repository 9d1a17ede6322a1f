#!/usr/bin/env python
"""Train the ClipCap mapper (``clip_project``) on the HIP GPT-2 -- ClipCap's ``train.py --only_prefix --mapping_type transformer
--num_layres 8 --prefix_length 40 --prefix_length_clip 40 --is_rn`` (the reference's README, "ClipCap training"):

    python tools/train_clipcap.py --data captions.pt --gpt2-weights gpt2.pt --out-dir out [--prefix run] [--epochs 10] [--bs 40]
        [--lr 2e-5] [--warmup-steps 5000] [--weight-decay 0.0] [--eps 1e-6] [--dtype bf16|f32] [--save-steps 10000]
        [--resume] [--with-gpt] [--init clipcap.pt]

``--data`` is the file tools/parse_captions.py writes; ``--gpt2-weights`` a GPT-2 state dict (a ClipCap file, a transformers
GPT2LMHeadModel file or bare GPT2Model keys).  GPT-2 stays frozen.  Writes ``<out-dir>/<prefix>_latest.pt`` every ``--save-steps``
steps and ``<prefix>-<epoch:03d>.pt`` after every epoch: ``clip_project.*``, what ``MODEL.VISION_TO_LANG_PATH`` and
tools/gen_captions.py read; ``--with-gpt`` adds ``gpt.*`` in transformers' layout (a complete ClipCap file).  ``<prefix>_state.pt``
carries the optimizer state, the step, the epoch position and the shuffle generator for ``--resume``.  ``--init`` starts from a
ClipCap file's ``clip_project.*`` instead of a random mapper.

The defaults are ClipCap's hyper-parameters (AdamW lr 2e-5, 5000 warm-up steps of a linear schedule, batch 40, 10 epochs).  The
optimizer is torch.optim.AdamW's arithmetic: ClipCap used the since-removed ``transformers.AdamW`` (eps 1e-6, weight decay 0), which
added ``eps`` to sqrt(v) BEFORE the bias correction; here ``eps`` sits outside it, as in torch.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def parse(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--data", required=True, help="caption dataset (tools/parse_captions.py)")
    ap.add_argument("--gpt2-weights", required=True, help="GPT-2 state dict file (frozen)")
    ap.add_argument("--out-dir", required=True)
    ap.add_argument("--prefix", default="run", help="checkpoint file name prefix")
    ap.add_argument("--epochs", type=int, default=10)
    ap.add_argument("--bs", type=int, default=40)
    ap.add_argument("--lr", type=float, default=2e-5)
    ap.add_argument("--warmup-steps", type=int, default=5000)
    ap.add_argument("--weight-decay", type=float, default=0.0)
    ap.add_argument("--eps", type=float, default=1e-6)
    ap.add_argument("--dtype", choices=("bf16", "f32"), default="bf16", help="bf16 throughput path or exact-f32 parity path")
    ap.add_argument("--save-steps", type=int, default=10000)
    ap.add_argument("--resume", action="store_true", help="continue from <prefix>_latest.pt + <prefix>_state.pt in --out-dir")
    ap.add_argument("--with-gpt", action="store_true", help="also write gpt.* (a complete ClipCap file)")
    ap.add_argument("--init", default=None, help="ClipCap file whose clip_project.* the mapper starts from")
    ap.add_argument("--prefix-length", type=int, default=40)
    ap.add_argument("--clip-length", type=int, default=40)
    ap.add_argument("--num-layers", type=int, default=8)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--device", default="cuda:0")
    return ap.parse_args(argv)


def main(argv=None):
    args = parse(argv)
    if not torch.cuda.is_available() or torch.device(args.device).type != "cuda":
        raise SystemExit(f"mapper training runs on the MI355X only (HIP kernels, no CPU path); --device {args.device}")
    from cddmsl_amd import clipcap_train as ct
    from cddmsl_amd.modeling import TransformerMapper
    from cddmsl_amd.modeling.gpt2 import load_gpt2

    dtype = torch.bfloat16 if args.dtype == "bf16" else torch.float32
    data = ct.load_dataset(args.data)
    decoder = load_gpt2(args.gpt2_weights, dtype).to(args.device)
    torch.manual_seed(args.seed)
    mapper = TransformerMapper(data["clip_embedding"].shape[1], decoder.n_embd, args.prefix_length, args.clip_length, args.num_layers,
                               compute_dtype=dtype, trainable=True)
    _init_like_torch(mapper)
    if args.init:
        if not os.path.isfile(args.init):
            raise SystemExit(f"--init not found: {args.init!r}")
        ct.load_mapper_weights(mapper, args.init)
    mapper.to(args.device)
    tr = ct.train(data, mapper, decoder, args.out_dir, args.prefix, args.epochs, args.bs, args.lr, args.warmup_steps, args.weight_decay,
                  args.eps, args.save_steps, args.resume, args.with_gpt, args.seed)
    print(f"{tr.global_step} steps; wrote {os.path.join(args.out_dir, args.prefix)}_latest.pt")
    return tr


def _init_like_torch(mapper):
    """the reference builds the mapper from nn.Linear / nn.LayerNorm / randn: their default initialisation"""
    from cddmsl_amd.modeling.clipcap import _Lin
    for m in mapper.modules():
        if isinstance(m, _Lin):
            ref = torch.nn.Linear(m.weight.shape[1], m.weight.shape[0], bias=m.bias is not None)
            with torch.no_grad():
                m.weight.copy_(ref.weight)
                if m.bias is not None:
                    m.bias.copy_(ref.bias)


if __name__ == "__main__":
    main()
