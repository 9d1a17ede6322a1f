#!/usr/bin/env python
"""Concept (class-name) embeddings for ``MODEL.CLIP.TEXT_EMB_PATH`` -- the reference's tools/extract_concept_features.py on this
package's HIP text encoder (cddmsl_amd/modeling/text_encoder.py).

Same command-line shape as the reference (extract_concept_features.sh):

    python tools/extract_concept_features.py --config-file configs/VOC-Experiments/faster_rcnn_CLIP_R_50_C4.yaml \\
        --bpe-vocab bpe_simple_vocab_16e6.txt.gz --templates templates.txt \\
        MODEL.WEIGHTS regionclip_pretrained-cc_rn50.pth INPUT_DIR datasets/custom_concepts OUTPUT_DIR output/concept_feats

reads ``INPUT_DIR/concepts.txt`` (one class name per line), and writes ``OUTPUT_DIR/concept_embeds.pth``: a float32 CPU tensor
[C, D], squeezed as the reference does, of each class's mean over its prompts of the projected EOT features.  The text encoder
comes from ``MODEL.WEIGHTS`` (RegionCLIP ``lang_encoder.*`` or OpenAI CLIP top-level names), or with ``--synthetic-weights SEED``
from ``synthetic.make_text_state_dict`` at the geometry ``MODEL.RESNETS.DEPTH`` implies (50: 512 wide -> 1024, 200 (RN50x4): 640 ->
640).  Neither CLIP's BPE vocabulary nor the template list ships with the package, so both are required inputs.
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

# build_clip_language_encoder (clip_backbone.py:807-877): text width and output dim by ResNet depth
WIDTH = {50: 512, 101: 512, 200: 640}
EMBED = {50: 1024, 101: 512, 200: 640}


def parse(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--config-file", required=True)
    ap.add_argument("--bpe-vocab", required=True, help="CLIP's bpe_simple_vocab_16e6.txt.gz")
    ap.add_argument("--templates", required=True, help="text file, one prompt template per line, '{}' where the name goes")
    ap.add_argument("--dtype", choices=("bf16", "f32"), default="bf16", help="bf16 throughput path or exact-f32 parity path")
    ap.add_argument("--synthetic-weights", type=int, default=None, metavar="SEED", help="seeded synthetic encoder instead of MODEL.WEIGHTS")
    ap.add_argument("--chunk", type=int, default=8192, help="sequences per encoder batch")
    ap.add_argument("opts", nargs=argparse.REMAINDER, help="KEY VALUE config overrides (MODEL.WEIGHTS, INPUT_DIR, OUTPUT_DIR, ...)")
    return ap.parse_args(argv)


def main(argv=None):
    args = parse(argv)
    from cddmsl_amd.clip_text import BPETokenizer, read_templates
    from cddmsl_amd.config import get_cfg
    from cddmsl_amd.modeling.text_encoder import load_text_encoder

    cfg = get_cfg()
    cfg.merge_from_file(args.config_file)
    cfg.merge_from_list(args.opts)
    if "INPUT_DIR" not in cfg:
        raise SystemExit("INPUT_DIR <dir holding concepts.txt> is required")
    device = torch.device(cfg.MODEL.DEVICE)
    if device.type != "cuda" or not torch.cuda.is_available():
        raise SystemExit(f"the text encoder runs on the MI355X only (HIP kernels, no CPU path); MODEL.DEVICE={cfg.MODEL.DEVICE}, "
                         f"GPU available: {torch.cuda.is_available()}")
    dtype = torch.bfloat16 if args.dtype == "bf16" else torch.float32
    with open(os.path.join(cfg.INPUT_DIR, "concepts.txt"), encoding="utf-8") as f:
        names = [ln.strip() for ln in f if ln.strip()]
    templates = read_templates(args.templates)
    bpe = BPETokenizer.from_vocab_file(args.bpe_vocab)
    if args.synthetic_weights is not None:
        depth = cfg.MODEL.RESNETS.DEPTH
        enc = load_text_encoder(synthetic_seed=args.synthetic_weights, compute_dtype=dtype, width=WIDTH[depth], embed_dim=EMBED[depth])
    else:
        if not cfg.MODEL.WEIGHTS:
            raise SystemExit("MODEL.WEIGHTS <checkpoint> (or --synthetic-weights SEED) is required")
        enc = load_text_encoder(cfg.MODEL.WEIGHTS, compute_dtype=dtype)
    enc.to(device)
    t0 = time.perf_counter()
    with torch.no_grad():
        feats = enc.encode_concepts(names, templates, bpe, chunk=args.chunk)
    feats = torch.squeeze(feats).float().cpu().contiguous()
    os.makedirs(cfg.OUTPUT_DIR, exist_ok=True)
    path = os.path.join(cfg.OUTPUT_DIR, "concept_embeds.pth")
    torch.save(feats, path)
    print(f"{len(names)} concepts x {len(templates)} templates -> {tuple(feats.shape)} {args.dtype} in {time.perf_counter() - t0:.2f} s: {path}")
    return path


if __name__ == "__main__":
    main()
