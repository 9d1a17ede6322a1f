"""Generates tests/golden/ref_text_encoder.npz by running the REFERENCE's own tokenizer and text encoder (read from /root/reference,
never copied): ``SimpleTokenizer`` + ``pre_tokenize`` (detectron2/data/datasets/clip_prompt_utils.py) and
``CLIPLangEncoder.encode_text`` (detectron2/modeling/backbone/clip_backbone.py:732-868) at full geometry (12 x 512, 8 heads,
77 tokens, vocab 49408) with ``synthetic.make_text_state_dict(0)``.  ``ftfy.fix_text`` is stubbed as the identity (every fixture
string is ASCII, which ftfy leaves alone).  Runs only in the build container; what travels:

  templates                 the reference's 80 prompt templates (get_prompt_templates)
  names                     one entry per class, synonyms joined with '|'
  ids / nprompt             [C, Pmax, 77] uint16 ``pre_tokenize`` ids of each class (P = synonyms x 80 rows, then zero rows up to
                            Pmax) and each class's P
  merge_a/merge_b/merge_rank/merge_id   the BPE merges those encodings applied, in rank order, with their CLIP rank and id
  vocab_tok / vocab_id      every symbol id the encodings produced (byte symbols included) and the two specials
  enc_ids / enc_out         24 sequences [24, 77] and encode_text's output [24, 1024] f32
  mean_classes / mean_out   a few classes and the mean of encode_text over their first 8 templates [k, 1024] f32
No weights are stored (make_text_state_dict(0) regenerates them).

usage:  python tests/golden/make_golden_text.py
"""
import importlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden  # noqa: E402  (stubs, package bypass, repository on sys.path)

VOC = ["aeroplane", "bicycle", "bird", "boat", "bottle", "bus", "car", "cat", "chair", "cow", "diningtable", "dog", "horse",
       "motorbike", "person", "pottedplant", "sheep", "sofa", "train", "tvmonitor"]
CITY = ["person", "rider", "car", "truck", "bus", "train", "motorcycle", "bicycle"]
SYNONYMS = [["traffic light", "stop light"], ["tv", "television", "tv monitor"], ["sofa", "couch"]]
AWKWARD = ["traffic light", "a+b,c", "route 66 sign", "people's car", "o'clock tower", "it's a dog's life", "3d printer",
           "hot-air balloon", "&amp; sign",
           "an extremely long and overly detailed description of a small red wooden toy fire engine with a ladder and two tiny "
           "plastic firefighters sitting on top of it near the old town square fountain, parked beside a bakery that sells warm "
           "bread, sweet cakes and fresh coffee every single morning of the week while pigeons wander around the cobbled street and children chase them, laughing loudly under the bright blue summer sky"]


def main():
    make_golden.setup()
    make_golden._pkg("detectron2.data.datasets", "detectron2/data/datasets")
    importlib.import_module("ftfy").fix_text = lambda s: s
    cpu = importlib.import_module("detectron2.data.datasets.clip_prompt_utils")
    cb = importlib.import_module("detectron2.modeling.backbone.clip_backbone")
    from cddmsl_amd import synthetic

    # record the merges BPE applies: the chosen bigram is the one tested with `in self.bpe_ranks`
    applied = set()

    class Ranks(dict):
        def __contains__(self, k):
            hit = dict.__contains__(self, k)
            if hit:
                applied.add(k)
            return hit

    orig_init = cpu.SimpleTokenizer.__init__

    def init(self, *a, **k):
        orig_init(self, *a, **k)
        self.bpe_ranks = Ranks(self.bpe_ranks)
    cpu.SimpleTokenizer.__init__ = init

    templates = cpu.get_prompt_templates()
    classes = [[n] for n in VOC] + [[n] for n in CITY] + SYNONYMS + [[n] for n in AWKWARD]
    per = [cpu.pre_tokenize([c if len(c) > 1 else c[0]])[0] for c in classes]      # [P_c, 77] each
    Pmax = max(p.shape[0] for p in per)
    ids = np.full((len(classes), Pmax, 77), 0, np.int64)
    for i, p in enumerate(per):
        ids[i, :p.shape[0]] = p.numpy()
    nprompt = np.array([p.shape[0] for p in per], np.int64)

    tok = cpu.SimpleTokenizer()
    used = set(int(v) for v in np.unique(ids))
    vocab = {tok.decoder[i]: i for i in sorted(used)}
    merges = sorted(applied, key=lambda m: tok.bpe_ranks[m])
    # every merge result that was applied must be in the token table too (intermediate symbols are)
    for a, b in merges:
        vocab.setdefault(a + b, tok.encoder[a + b])
        vocab.setdefault(a, tok.encoder[a])
        vocab.setdefault(b, tok.encoder[b])

    # encode_text at full geometry
    sd = synthetic.make_text_state_dict(0)
    enc = cb.CLIPLangEncoder(1024, 224, [3, 4, 6, 3], 64, None, 77, 49408, 512, 8, 12, ["res5"], 2)
    enc.load_state_dict(sd, strict=True)
    enc.eval()
    flat = [(c, p) for c in range(len(classes)) for p in range(nprompt[c])]
    pick = [flat[(k * 997) % len(flat)] for k in range(20)] + [(len(classes) - 1, 0), (len(classes) - 1, 5), (20, 3), (0, 0)]
    enc_ids = np.stack([ids[c, p] for c, p in pick])
    mean_classes = np.array([0, 15, 27, 28, 31], np.int64)     # aeroplane, pottedplant, bicycle (Cityscapes), traffic light | stop light, traffic light
    with torch.no_grad():
        enc_out = enc.encode_text(torch.from_numpy(enc_ids)).numpy().astype(np.float32)
        mean_out = np.stack([enc.encode_text(torch.from_numpy(ids[c, :8])).mean(0).numpy() for c in mean_classes]).astype(np.float32)

    names = np.array(["|".join(c) for c in classes])
    np.savez_compressed(os.path.join(HERE, "ref_text_encoder.npz"),
                        templates=np.array(templates), names=names, nprompt=nprompt, ids=ids.astype(np.uint16),
                        merge_a=np.array([m[0] for m in merges]), merge_b=np.array([m[1] for m in merges]),
                        merge_rank=np.array([tok.bpe_ranks[m] for m in merges], np.int64),
                        merge_id=np.array([tok.encoder[m[0] + m[1]] for m in merges], np.int64),
                        vocab_tok=np.array(list(vocab.keys())), vocab_id=np.array(list(vocab.values()), np.int64),
                        enc_ids=enc_ids.astype(np.int64), enc_out=enc_out, mean_classes=mean_classes, mean_out=mean_out)
    print("text encoder fixture:", len(classes), "classes,", len(merges), "merges,", len(vocab), "symbols,",
          "eot max", int(ids.argmax(-1).max()), "cut", int((ids[..., -1] != 0).sum()), "|out| max", float(np.abs(enc_out).max()))


if __name__ == "__main__":
    main()
