#!/usr/bin/env python
"""Build the caption dataset that tools/train_clipcap.py trains on -- ClipCap's (patched) parse_coco.py on this package's encoder:

    python tools/parse_captions.py --config-file configs/VOC-Experiments/faster_rcnn_CLIP_R_50_C4.yaml --captions train_caption.json \\
        --images DIR --gpt2-vocab encoder.json --gpt2-merges vocab.bpe MODEL.WEIGHTS model.pth OUTPUT captions.pt

``--captions`` is ClipCap's list of {"image_id", "caption"}; an image is looked up in ``--images`` as ``<image_id>`` itself, with
.jpg / .jpeg / .png appended, or as COCO's ``COCO_train2014_<id:012d>.jpg`` / ``COCO_val2014_<id:012d>.jpg`` / ``<id:012d>.jpg``.
Every image is embedded once by ``captioning.image_embeddings`` -- the preprocessing tools/gen_captions.py uses (test-loader resize,
then the 224x224 image-level path), not OpenAI CLIP's PIL preprocessing: no parity with ClipCap's own embeddings is claimed.  The
captions are tokenised by ``GPT2Vocab.encode``.  Writes OUTPUT: the dataset file of cddmsl_amd/clipcap_train.py (``clip_embedding``,
``caption_embedding``, ``tokens``, ``captions``), which loads with ``weights_only=True``.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

EXTS = ("", ".jpg", ".jpeg", ".png")


def parse(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--config-file", required=True)
    ap.add_argument("--captions", required=True, help="json list of {image_id, caption}")
    ap.add_argument("--images", required=True, help="directory of the images")
    ap.add_argument("--gpt2-vocab", required=True, help="GPT-2's encoder.json / vocab.json (token -> id)")
    ap.add_argument("--gpt2-merges", required=True, help="GPT-2's vocab.bpe / merges.txt")
    ap.add_argument("--batch", type=int, default=32, help="images per embedding batch")
    ap.add_argument("opts", nargs=argparse.REMAINDER, help="KEY VALUE config overrides (MODEL.WEIGHTS, OUTPUT, ...)")
    return ap.parse_args(argv)


def find_image(root, image_id):
    names = [str(image_id) + e for e in EXTS]
    if str(image_id).isdigit():
        n = int(image_id)
        names += [f"COCO_train2014_{n:012d}.jpg", f"COCO_val2014_{n:012d}.jpg", f"{n:012d}.jpg"]
    for name in names:
        p = os.path.join(root, name)
        if os.path.isfile(p):
            return p
    raise SystemExit(f"image {image_id!r} not found in {root!r} (tried {names})")


def main(argv=None):
    args = parse(argv)
    from cddmsl_amd.config import get_cfg
    cfg = get_cfg()
    cfg.merge_from_file(args.config_file)
    opts = list(args.opts)
    out = None
    if "OUTPUT" in opts:                               # (the output file is this tool's own key, not the config's)
        i = opts.index("OUTPUT")
        out = opts[i + 1]
        del opts[i:i + 2]
    cfg.merge_from_list(opts)
    if not out:
        raise SystemExit("OUTPUT <dataset file> is required")
    for path, what in ((args.captions, "--captions"), (args.gpt2_vocab, "--gpt2-vocab"), (args.gpt2_merges, "--gpt2-merges"),
                       (cfg.MODEL.WEIGHTS, "MODEL.WEIGHTS")):
        if not path or not os.path.isfile(path):
            raise SystemExit(f"{what} not found: {path!r}")
    if not os.path.isdir(args.images):
        raise SystemExit(f"--images <dir> not found: {args.images!r}")
    device = torch.device(cfg.MODEL.DEVICE)
    if device.type != "cuda" or not torch.cuda.is_available():
        raise SystemExit(f"the image encoder runs on the MI355X only (HIP kernels, no CPU path); MODEL.DEVICE={cfg.MODEL.DEVICE}")

    from cddmsl_amd import clipcap_train as ct
    from cddmsl_amd.captioning import image_embeddings
    from cddmsl_amd.checkpoint import DetectionCheckpointer
    from cddmsl_amd.data import read_image
    from cddmsl_amd.gpt2_text import GPT2Vocab
    from cddmsl_amd.modeling import build_model

    with open(args.captions, encoding="utf-8") as f:
        items = json.load(f)
    vocab = GPT2Vocab(args.gpt2_vocab, merges=args.gpt2_merges)
    model = build_model(cfg)
    DetectionCheckpointer(model).load(cfg.MODEL.WEIGHTS)
    model.eval()

    row_of, paths = {}, []
    for it in items:
        if it["image_id"] not in row_of:
            row_of[it["image_id"]] = len(paths)
            paths.append(find_image(args.images, it["image_id"]))
    embs = []
    with torch.no_grad():
        for i in range(0, len(paths), args.batch):
            imgs = [read_image(p, cfg.INPUT.FORMAT) for p in paths[i:i + args.batch]]
            embs.append(image_embeddings(model, imgs, cfg).cpu())
    emb = torch.cat(embs) if embs else torch.empty((0, 0))
    captions = [it["caption"] for it in items]
    ct.save_dataset(out, emb, torch.tensor([row_of[it["image_id"]] for it in items], dtype=torch.int64),
                    [vocab.encode(c) for c in captions], captions)
    print(f"{len(captions)} captions of {len(paths)} images: {out}")
    return out


if __name__ == "__main__":
    main()
