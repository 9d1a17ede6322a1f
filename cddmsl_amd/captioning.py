"""Captions of images and detected regions: an image or region embedding -> the ClipCap mapper's 40 prefix rows -> GPT-2 greedy
decoding (the reference's gen_captions.py), or with ``beam_size`` length-normalised beam search (ClipCap's other mode), of which
the best beam and its score are reported.

* Images: each image is resized as the test loader resizes it (shortest edge ``INPUT.MIN_SIZE_TEST``, longest at most
  ``INPUT.MAX_SIZE_TEST``), then ``preprocess224`` -> backbone -> attention pool: the embedding the image-level consistency branch
  trains on.
* Regions: the detector's inference, and the attention-pool embeddings of the proposals the kept detections came from (the
  reference's tools/extract_region_features.py), at most ``max_regions`` per image, highest score first.  Boxes are in
  original-image coordinates.

This is the training's preprocessing, not OpenAI CLIP's PIL preprocessing that the reference's gen_captions.py applies to whole
images: no parity with the latter is claimed.
"""
from typing import Dict, List, Optional

import numpy as np
import torch

from . import hip
from .data import resize_image, shortest_edge_size
from .gpt2_text import GPT2Vocab


def _resized(img_u8: np.ndarray, cfg) -> torch.Tensor:
    h, w = img_u8.shape[:2]
    nh, nw = shortest_edge_size(h, w, cfg.INPUT.MIN_SIZE_TEST, cfg.INPUT.MAX_SIZE_TEST)
    return torch.from_numpy(np.ascontiguousarray(resize_image(img_u8, nh, nw).transpose(2, 0, 1)))


def _captions(decoder, mapper, emb, max_tokens, stop_id, vocab: Optional[GPT2Vocab], beam_size: Optional[int] = None):
    prefix = mapper(emb.float())                                            # [n, 40, 768] f32
    scores = None
    if beam_size is None:
        tokens, lengths = decoder.generate(prefix, max_tokens=max_tokens, stop_id=stop_id)
    else:
        tokens, lengths, scores = decoder.generate_beam(prefix, beam_size=beam_size, max_tokens=max_tokens, stop_id=stop_id)
        tokens, lengths, scores = tokens[:, 0], lengths[:, 0], scores[:, 0].cpu().tolist()      # the best beam
    tokens, lengths = tokens.cpu(), lengths.cpu()
    out = []
    for i, (t, n) in enumerate(zip(tokens, lengths.tolist())):
        ids = t[:n].tolist()
        out.append({"tokens": ids, "caption": vocab.decode(ids) if vocab is not None else None})
        if scores is not None:
            out[-1]["score"] = float(scores[i])
    return out


@torch.no_grad()
def image_embeddings(model, images_u8: List[np.ndarray], cfg) -> torch.Tensor:
    """[n, D] f32: resize (test loader) -> preprocess224 -> backbone -> attention pool, one image at a time through the resize"""
    xs = []
    for img in images_u8:
        t = _resized(img, cfg).to(model.device)
        xs.append(hip.preprocess224([t], t.shape[-2], t.shape[-1], model.pixel_mean_list, model.pixel_std_list, model.compute_dtype))
    return model._encode(model.backbone, torch.cat(xs)).float()


@torch.no_grad()
def caption_images(model, mapper, decoder, images_u8: List[np.ndarray], cfg, vocab: Optional[GPT2Vocab] = None, max_tokens=67,
                   stop_id: Optional[int] = None, batch=32, beam_size: Optional[int] = None) -> List[Dict]:
    """one {"caption", "tokens"} per image (HWC uint8 in the model's INPUT.FORMAT); with ``beam_size`` the best beam of a beam
    search of that width and its "score" (the mean log-probability of its tokens)"""
    out = []
    for i in range(0, len(images_u8), batch):
        out += _captions(decoder, mapper, image_embeddings(model, images_u8[i:i + batch], cfg), max_tokens, stop_id, vocab, beam_size)
    return out


@torch.no_grad()
def caption_regions(model, mapper, decoder, images_u8: List[np.ndarray], cfg, vocab: Optional[GPT2Vocab] = None, max_regions=10,
                    max_tokens=67, stop_id: Optional[int] = None, beam_size: Optional[int] = None) -> List[List[Dict]]:
    """per image a list of {"box" [x0, y0, x1, y1] in original-image pixels, "class", "score", "caption", "tokens"}, highest score
    first, at most ``max_regions``; with ``beam_size`` the captions are the best beams, each with its "caption_score" ("score" is
    the detection's)"""
    out = []
    for img in images_u8:
        inp = {"image": _resized(img, cfg), "height": img.shape[0], "width": img.shape[1]}
        inst = model.inference_with_region_embeddings([inp])[0]["instances"]
        order = torch.argsort(inst.scores, descending=True)[:max_regions]
        regs = []
        if len(order):
            emb = inst.region_embeds[order]
            caps = _captions(decoder, mapper, emb, max_tokens, stop_id, vocab, beam_size)
            boxes, cls, sc = inst.pred_boxes.tensor[order].cpu(), inst.pred_classes[order].cpu(), inst.scores[order].cpu()
            for b, c, s, cap in zip(boxes.tolist(), cls.tolist(), sc.tolist(), caps):
                if "score" in cap:                       # "score" stays the detection's
                    cap["caption_score"] = cap.pop("score")
                regs.append({"box": b, "class": int(c), "score": float(s), **cap})
        out.append(regs)
    return out
