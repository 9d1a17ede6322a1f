#!/usr/bin/env python
"""Captions for images and detected regions -- the reference's gen_captions.py on this package's HIP GPT-2 decoder
(cddmsl_amd/modeling/gpt2.py) and the ClipCap mapper:

    python tools/gen_captions.py --config-file configs/VOC-Experiments/faster_rcnn_CLIP_R_50_C4.yaml --gpt2-vocab encoder.json \\
        [--regions] MODEL.WEIGHTS model_final.pth MODEL.VISION_TO_LANG_PATH coco_prefix.pt INPUT_DIR images OUTPUT_DIR out

Every image of INPUT_DIR (.jpg / .jpeg / .png) is captioned; with ``--regions`` each of its detections too (at most
``--max-regions``, highest score first).  GPT-2 comes from the ClipCap file ``MODEL.VISION_TO_LANG_PATH`` (``gpt.*`` next to
``clip_project.*``) unless ``--gpt2-weights`` names another file.  GPT-2's vocabulary (``encoder.json`` / ``vocab.json``) does not
ship, so it is required.  Writes ``OUTPUT_DIR/captions.json``: per image file name {"caption", "tokens"[, "regions": [{"box",
"class", "score", "caption", "tokens"}]]}.  Greedy decoding stops at ``--stop-token`` (kept) or after ``--max-tokens``.
``--beam-size K`` with K > 1 decodes by length-normalised beam search of width K (ClipCap's other mode; upstream uses 5) and
reports the best beam: each image entry gains "score", the mean log-probability of the caption's tokens, and each region entry the
same as "caption_score" (a region's "score" is its detection score).  K = 1, the default, is the greedy path and its output.
Images are preprocessed as in training (test-loader resize, then the 224x224 image-level path), not with OpenAI CLIP's PIL
preprocessing; captions are not claimed to match the reference's.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

EXTS = (".jpg", ".jpeg", ".png")


def parse(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--config-file", required=True)
    ap.add_argument("--gpt2-vocab", required=True, help="GPT-2's encoder.json / vocab.json (token -> id)")
    ap.add_argument("--gpt2-weights", default=None, help="GPT-2 state dict file (default: the ClipCap file's gpt.* entries)")
    ap.add_argument("--regions", action="store_true", help="also caption each detected region")
    ap.add_argument("--max-regions", type=int, default=10)
    ap.add_argument("--max-tokens", type=int, default=67)
    ap.add_argument("--stop-token", default=".")
    ap.add_argument("--beam-size", type=int, default=1, help="beam width 1..8; 1 = greedy decoding")
    ap.add_argument("--dtype", choices=("bf16", "f32"), default="bf16", help="bf16 throughput path or exact-f32 parity path")
    ap.add_argument("--batch", type=int, default=32, help="images per embedding batch")
    ap.add_argument("opts", nargs=argparse.REMAINDER, help="KEY VALUE config overrides (MODEL.WEIGHTS, INPUT_DIR, OUTPUT_DIR, ...)")
    return ap.parse_args(argv)


def _need_file(path, what):
    if not path or not os.path.isfile(path):
        raise SystemExit(f"{what} not found: {path!r}")


def main(argv=None):
    args = parse(argv)
    from cddmsl_amd.config import get_cfg
    cfg = get_cfg()
    cfg.merge_from_file(args.config_file)
    cfg.merge_from_list(args.opts)
    if not 1 <= args.beam_size <= 8:
        raise SystemExit(f"--beam-size {args.beam_size} outside 1..8")
    _need_file(args.gpt2_vocab, "--gpt2-vocab")
    _need_file(cfg.MODEL.WEIGHTS, "MODEL.WEIGHTS")
    _need_file(cfg.MODEL.get("VISION_TO_LANG_PATH", ""), "MODEL.VISION_TO_LANG_PATH")
    if args.gpt2_weights is not None:
        _need_file(args.gpt2_weights, "--gpt2-weights")
    if "INPUT_DIR" not in cfg or not os.path.isdir(cfg.INPUT_DIR):
        raise SystemExit(f"INPUT_DIR <dir of images> not found: {cfg.get('INPUT_DIR')!r}")
    device = torch.device(cfg.MODEL.DEVICE)
    if device.type != "cuda" or not torch.cuda.is_available():
        raise SystemExit(f"captioning runs on the MI355X only (HIP kernels, no CPU path); MODEL.DEVICE={cfg.MODEL.DEVICE}")

    from cddmsl_amd.captioning import caption_images, caption_regions
    from cddmsl_amd.checkpoint import DetectionCheckpointer
    from cddmsl_amd.data import read_image
    from cddmsl_amd.gpt2_text import GPT2Vocab
    from cddmsl_amd.modeling import TransformerMapper, build_model
    from cddmsl_amd.modeling.gpt2 import GPT2Decoder, load_gpt2

    dtype = torch.bfloat16 if args.dtype == "bf16" else torch.float32
    cfg.merge_from_list(["MODEL.COMPUTE_DTYPE", args.dtype])
    vocab = GPT2Vocab(args.gpt2_vocab)
    stop_id = vocab.token_id(args.stop_token) if args.stop_token else None
    model = build_model(cfg)
    DetectionCheckpointer(model).load(cfg.MODEL.WEIGHTS)
    model.eval()
    cc = torch.load(cfg.MODEL.VISION_TO_LANG_PATH, map_location="cpu", weights_only=True)
    mapper = TransformerMapper(1024, 768, 40, 40, 8, compute_dtype=dtype)
    mapper.load_state_dict({k[len("clip_project."):]: v for k, v in cc.items() if k.startswith("clip_project.")})
    mapper.to(model.device).eval()
    decoder = load_gpt2(args.gpt2_weights, dtype) if args.gpt2_weights else GPT2Decoder.from_state_dict(cc, dtype)
    if decoder.vocab_size > len(vocab):
        raise SystemExit(f"--gpt2-vocab has {len(vocab)} entries, GPT-2 has {decoder.vocab_size}")
    decoder.to(model.device)

    names = sorted(f for f in os.listdir(cfg.INPUT_DIR) if f.lower().endswith(EXTS))
    images = [read_image(os.path.join(cfg.INPUT_DIR, f), cfg.INPUT.FORMAT) for f in names]
    t0 = time.perf_counter()
    beam = args.beam_size if args.beam_size > 1 else None
    caps = caption_images(model, mapper, decoder, images, cfg, vocab, args.max_tokens, stop_id, args.batch, beam_size=beam)
    result = {n: c for n, c in zip(names, caps)}
    if args.regions:
        regions = caption_regions(model, mapper, decoder, images, cfg, vocab, args.max_regions, args.max_tokens, stop_id, beam_size=beam)
        for n, regs in zip(names, regions):
            result[n]["regions"] = regs
    os.makedirs(cfg.OUTPUT_DIR, exist_ok=True)
    path = os.path.join(cfg.OUTPUT_DIR, "captions.json")
    with open(path, "w", encoding="utf-8") as f:
        json.dump(result, f, indent=1, ensure_ascii=False)
    print(f"{len(names)} images{' + regions' if args.regions else ''} captioned ({args.dtype}) in {time.perf_counter() - t0:.2f} s: {path}")
    return path


if __name__ == "__main__":
    main()
