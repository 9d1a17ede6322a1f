"""Training the ClipCap mapper (``clip_project``) against the frozen GPT-2 -- the reference's README "ClipCap training" section:
ClipCap's ``train.py --only_prefix --mapping_type transformer --num_layres 8 --prefix_length 40 --prefix_length_clip 40 --is_rn``,
whose loop also sits in the reference's clipcap.py (``ClipCaptionModel.forward``, ``ClipCaptionPrefix``, ``pad_captions``, ``train``).

One step: ``prefix = mapper(clip_embedding)`` -> ``GPT2Decoder.caption_loss(prefix, tokens)`` -> backward -> AdamW at the schedule's
learning rate.  GPT-2 stays frozen; only ``clip_project.*`` is written (``--with-gpt`` adds GPT-2 for a complete ClipCap file).

Dataset file (``save_dataset`` / ``load_dataset``): a ``torch.save`` dict of tensors and strings that loads with
``weights_only=True`` -- ClipCap's parse_coco.py writes a pickle of the same four entries:
  ``clip_embedding``     [N, D] f32     one row per image
  ``caption_embedding``  [M] int64      the image row of each caption
  ``tokens``             [M, Lmax] int64, GPT-2 ids, padded with -1
  ``captions``           M strings

Conventions (ClipCap's): a caption is cut to ``max_seq_len = min(int(mean + 10 std), max)`` tokens of the lengths in the file (here
also capped so that prefix + tokens <= 128 positions, the attention kernels' limit) and padded with -1, which becomes token 0;
token 0 is ignored by the loss wherever it stands.  Batches are a shuffle of the captions with the incomplete last batch dropped.
"""
import os
from typing import Dict, Iterator, List, Optional

import torch

from .modeling.clipcap import TransformerMapper
from .modeling.gpt2 import GPT2Decoder
from .solver import AdamW, linear_warmup_schedule

MAX_POSITIONS = 128          # prefix + caption tokens: GPT2Decoder.caption_loss's limit
DATASET_KEYS = ("clip_embedding", "caption_embedding", "tokens", "captions")


# ---------------------------------------------------------------------------------------------------------------- dataset file
def save_dataset(path: str, clip_embedding: torch.Tensor, caption_embedding: torch.Tensor, token_lists: List[List[int]],
                 captions: List[str]):
    M = len(captions)
    assert len(token_lists) == M and caption_embedding.numel() == M and clip_embedding.dim() == 2
    Lmax = max((len(t) for t in token_lists), default=0)
    tokens = torch.full((M, max(Lmax, 1)), -1, dtype=torch.int64)
    for i, t in enumerate(token_lists):
        tokens[i, :len(t)] = torch.tensor(t, dtype=torch.int64)
    torch.save({"clip_embedding": clip_embedding.detach().float().cpu().contiguous(),
                "caption_embedding": caption_embedding.detach().to(torch.int64).cpu().contiguous(),
                "tokens": tokens, "captions": [str(c) for c in captions]}, path)


def load_dataset(path: str) -> Dict:
    if not os.path.isfile(path):
        raise FileNotFoundError(f"caption dataset not found: {path}")
    d = torch.load(path, map_location="cpu", weights_only=True)
    missing = [k for k in DATASET_KEYS if k not in d]
    if missing:
        raise KeyError(f"{path}: not a caption dataset, missing {missing}")
    emb, own, tok = d["clip_embedding"], d["caption_embedding"], d["tokens"]
    if emb.dim() != 2 or emb.dtype != torch.float32 or own.dtype != torch.int64 or tok.dtype != torch.int64 or tok.dim() != 2:
        raise ValueError(f"{path}: clip_embedding [N, D] f32, caption_embedding [M] int64, tokens [M, Lmax] int64 expected")
    if own.numel() != tok.shape[0] or len(d["captions"]) != tok.shape[0]:
        raise ValueError(f"{path}: caption_embedding, tokens and captions disagree on the number of captions")
    if own.numel() and (int(own.min()) < 0 or int(own.max()) >= emb.shape[0]):
        raise ValueError(f"{path}: caption_embedding points outside clip_embedding")
    return d


def token_lengths(tokens: torch.Tensor) -> torch.Tensor:
    """tokens [M, Lmax] padded with -1 -> the number of tokens of each caption"""
    return (tokens >= 0).sum(dim=1)


def choose_max_seq_len(lengths: torch.Tensor, prefix_length: int, positions: int = MAX_POSITIONS) -> int:
    """ClipCap's rule ``min(int(mean + 10 std), max)`` over the caption lengths (std as ``torch.std``: unbiased; 0 for a single
    caption), capped so that ``prefix_length + max_seq_len <= positions``; at least 1"""
    ln = lengths.float()
    std = float(ln.std()) if ln.numel() > 1 else 0.0
    L = min(int(float(ln.mean()) + std * 10), int(ln.max()))
    return max(1, min(L, positions - prefix_length))


def pad_tokens(tokens: torch.Tensor, max_seq_len: int) -> torch.Tensor:
    """``pad_captions``: rows [.., L] padded with -1 -> [.., max_seq_len], cut or padded, every -1 turned into token 0"""
    L = tokens.shape[-1]
    if L >= max_seq_len:
        out = tokens[..., :max_seq_len].clone()
    else:
        out = torch.cat((tokens, torch.full((*tokens.shape[:-1], max_seq_len - L), -1, dtype=tokens.dtype)), dim=-1)
    out[out < 0] = 0
    return out


def epoch_batches(num_captions: int, batch_size: int, generator: torch.Generator) -> List[torch.Tensor]:
    """one epoch's batches: a shuffle drawn from ``generator``, the incomplete last batch dropped (DataLoader(shuffle, drop_last))"""
    perm = torch.randperm(num_captions, generator=generator)
    return [perm[i:i + batch_size] for i in range(0, num_captions - batch_size + 1, batch_size)]


# ---------------------------------------------------------------------------------------------------------------- checkpoints
_CONV1D = ("attn.c_attn.weight", "attn.c_proj.weight", "mlp.c_fc.weight", "mlp.c_proj.weight")


def gpt_entries(decoder: GPT2Decoder) -> Dict[str, torch.Tensor]:
    """``gpt.transformer.*`` + ``gpt.lm_head.weight`` in transformers' layout (Conv1D weights [in, out], the head tied to wte)"""
    out = {}
    for k, v in decoder.state_dict().items():
        v = v.detach().cpu()
        out["gpt.transformer." + k] = v.t().contiguous() if k.endswith(_CONV1D) else v.clone()
    out["gpt.lm_head.weight"] = out["gpt.transformer.wte.weight"].clone()
    return out


def clipcap_state(mapper: TransformerMapper, decoder: Optional[GPT2Decoder] = None) -> Dict[str, torch.Tensor]:
    """the ClipCap file: ``clip_project.*`` (what the detector's trainer and tools/gen_captions.py read), with ``decoder`` also GPT-2"""
    out = {"clip_project." + k: v.detach().cpu().clone() for k, v in mapper.state_dict().items()}
    if decoder is not None:
        out.update(gpt_entries(decoder))
    return out


def load_mapper_weights(mapper: TransformerMapper, path: str):
    sd = torch.load(path, map_location="cpu", weights_only=True)
    mapper.load_state_dict({k[len("clip_project."):]: v for k, v in sd.items() if k.startswith("clip_project.")})


# ---------------------------------------------------------------------------------------------------------------- the loop
class MapperTrainer:
    """the training state: mapper (trainable), frozen decoder, AdamW, the warm-up schedule's position and the shuffle generator"""

    def __init__(self, mapper: TransformerMapper, decoder: GPT2Decoder, lr=2e-5, warmup_steps=5000, total_steps=1,
                 weight_decay=0.0, eps=1e-6, betas=(0.9, 0.999), seed=0):
        assert mapper.trainable, "TransformerMapper(..., trainable=True)"
        self.mapper, self.decoder = mapper, decoder
        self.optimizer = AdamW(list(mapper.parameters()), lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)
        self.base_lr, self.warmup_steps, self.total_steps = float(lr), int(warmup_steps), int(total_steps)
        self.global_step, self.epoch, self.batch_in_epoch = 0, 0, 0
        self.generator = torch.Generator().manual_seed(seed)
        self.epoch_generator_state = self.generator.get_state()       # the generator as the current epoch's shuffle found it

    def lr_now(self) -> float:
        return self.base_lr * linear_warmup_schedule(self.global_step, self.warmup_steps, self.total_steps)

    def step(self, clip_embedding: torch.Tensor, tokens: torch.Tensor) -> float:
        """one optimisation step on a batch (clip_embedding [bs, D] f32, tokens [bs, L] int64 with 0 for the pads) -> the loss"""
        dev = self.decoder.wte.weight.device
        self.optimizer.lr = self.lr_now()
        self.optimizer.zero_grad()
        prefix = self.mapper(clip_embedding.to(dev, torch.float32))
        loss = self.decoder.caption_loss(prefix, tokens.to(dev))
        loss.backward()
        self.optimizer.step()
        self.global_step += 1
        return float(loss.detach())

    # -- files
    def save(self, out_dir: str, prefix: str, epoch_file: Optional[int] = None, with_gpt=False):
        """``<prefix>_latest.pt`` (+ ``<prefix>-<epoch:03d>.pt``) and the sidecar ``<prefix>_state.pt`` for ``resume``"""
        os.makedirs(out_dir, exist_ok=True)
        state = clipcap_state(self.mapper, self.decoder if with_gpt else None)
        torch.save(state, os.path.join(out_dir, f"{prefix}_latest.pt"))
        if epoch_file is not None:
            torch.save(state, os.path.join(out_dir, f"{prefix}-{epoch_file:03d}.pt"))
        torch.save({"optimizer": self.optimizer.state_dict(), "global_step": self.global_step, "epoch": self.epoch,
                    "batch_in_epoch": self.batch_in_epoch, "generator": self.generator.get_state(),
                    "epoch_generator": self.epoch_generator_state, "base_lr": self.base_lr, "warmup_steps": self.warmup_steps,
                    "total_steps": self.total_steps}, os.path.join(out_dir, f"{prefix}_state.pt"))

    def resume(self, out_dir: str, prefix: str):
        """restores the weights of ``<prefix>_latest.pt`` and, from the sidecar, the moments, step counts, schedule position,
        epoch position and generator state"""
        load_mapper_weights(self.mapper, os.path.join(out_dir, f"{prefix}_latest.pt"))
        s = torch.load(os.path.join(out_dir, f"{prefix}_state.pt"), map_location="cpu", weights_only=True)
        self.optimizer.load_state_dict(s["optimizer"])
        self.global_step, self.epoch, self.batch_in_epoch = int(s["global_step"]), int(s["epoch"]), int(s["batch_in_epoch"])
        self.base_lr, self.warmup_steps, self.total_steps = float(s["base_lr"]), int(s["warmup_steps"]), int(s["total_steps"])
        self.generator.set_state(s["generator"])
        self.epoch_generator_state = s["epoch_generator"]

    def batches(self, num_captions: int, batch_size: int) -> Iterator[torch.Tensor]:
        """the rest of the current epoch's batches; after a ``resume`` inside an epoch, that epoch's own shuffle from where it stopped"""
        if self.batch_in_epoch == 0:
            self.epoch_generator_state = self.generator.get_state()
            order = epoch_batches(num_captions, batch_size, self.generator)
        else:
            g = torch.Generator()
            g.set_state(self.epoch_generator_state)
            order = epoch_batches(num_captions, batch_size, g)
        for idx in order[self.batch_in_epoch:]:
            yield idx
            self.batch_in_epoch += 1
        self.batch_in_epoch = 0
        self.epoch += 1


def train(data: Dict, mapper: TransformerMapper, decoder: GPT2Decoder, out_dir: str, prefix="run", epochs=10, bs=40, lr=2e-5,
          warmup_steps=5000, weight_decay=0.0, eps=1e-6, save_steps=10000, resume=False, with_gpt=False, seed=0, log=print, log_every=100) -> MapperTrainer:
    """ClipCap's ``train`` on a loaded dataset; returns the trainer (its ``global_step`` is the number of steps taken in all)"""
    P = mapper.prefix_const.shape[0]
    L = choose_max_seq_len(token_lengths(data["tokens"]), P)
    tokens = pad_tokens(data["tokens"], L)
    M = tokens.shape[0]
    per_epoch = M // bs
    if per_epoch == 0:
        raise ValueError(f"{M} captions do not fill one batch of {bs}")
    tr = MapperTrainer(mapper, decoder, lr, warmup_steps, epochs * per_epoch, weight_decay, eps, seed=seed)
    if resume:
        tr.resume(out_dir, prefix)
    while tr.epoch < epochs:
        epoch = tr.epoch
        for idx in tr.batches(M, bs):
            loss = tr.step(data["clip_embedding"][data["caption_embedding"][idx]], tokens[idx])
            if tr.global_step % save_steps == 0:
                tr.batch_in_epoch += 1                     # the sidecar points at the next batch
                tr.save(out_dir, prefix, with_gpt=with_gpt)
                tr.batch_in_epoch -= 1
            if tr.global_step % log_every == 0 or tr.global_step == 1:
                log(f"epoch {epoch} step {tr.global_step} loss {loss:.4f} lr {tr.optimizer.lr:.3e}")
        tr.save(out_dir, prefix, epoch_file=epoch, with_gpt=with_gpt)
    return tr
