"""CLIP text encoder (frozen) -- RegionCLIP's ``CLIPLangEncoder`` (detectron2/modeling/backbone/clip_backbone.py:732-877, residual
block :273-317), the tower behind ``MODEL.CLIP.TEXT_EMB_PATH``: tools/extract_concept_features.py averages its projected EOT
features over a class's prompts.  Parameter names are the reference's (``token_embedding.weight``, ``positional_embedding``,
``transformer.resblocks.{i}.{ln_1, attn.in_proj_weight, attn.in_proj_bias, attn.out_proj, ln_2, mlp.c_fc, mlp.c_proj}.*``,
``ln_final.*``, ``text_projection``); the geometry comes from the tensors, so RN50 (width 512, 8 heads, 1024 out) and RN50x4
(640, 10, 640) load alike, from RegionCLIP files (``lang_encoder.*``) or OpenAI CLIP files (top level).

Forward only: the token + positional embedding, the layers on ``causal_stack.prefill`` with QuickGELU (its bf16 throughput path, or
its exact-f32 parity path with ``compute_dtype=torch.float32``), then ln_final and the projection of the EOT rows.

Truncation.  The mask lets position i attend to keys j <= i only, so no position <= the EOT depends on any later position, and
the only rows read out (one per sequence, at the EOT) come out the same whether the batch runs at 77 tokens or cut to
``T = max(eot) + 1`` (every layer is row-wise except attention, and attention of row i reads rows <= i).  Every batch therefore runs
at that T: prompts are 10-20 tokens, about 4x less work than 77.  On the HIP kernels each row is computed independently of T (the
attention kernel walks key tiles 0 .. i's tile whatever t is; LayerNorm, QuickGELU and the embedding are per row).

The last layer is run in full: an EOT-rows-only last layer (as the mapper's ``_last_token_layer``) would save at most 1/24 of the
GEMM work here and was not built.
"""
import re
from functools import partial
from typing import Dict, List, Optional, Sequence

import torch
from torch import nn

from .. import hip, layers
from .._lib import require_cuda
from ..clip_text import BPETokenizer, concept_prompts, tokenize_prompts
from .causal_stack import HEAD_DIM, FrozenCausalStack, Layer, _Prepared, f32, gemm_weight, prefill


class _Attn(nn.Module):
    """nn.MultiheadAttention's parameters (in_proj_weight / in_proj_bias rows: q | k | v, out_proj)"""

    def __init__(self, w):
        super().__init__()
        self.in_proj_weight = nn.Parameter(torch.empty(3 * w, w))
        self.in_proj_bias = nn.Parameter(torch.empty(3 * w))
        self.out_proj = nn.Linear(w, w)


class _Mlp(nn.Module):
    def __init__(self, w):
        super().__init__()
        self.c_fc, self.c_proj = nn.Linear(w, 4 * w), nn.Linear(4 * w, w)


class ResidualAttentionBlock(nn.Module):
    def __init__(self, w):
        super().__init__()
        self.attn, self.ln_1, self.mlp, self.ln_2 = _Attn(w), nn.LayerNorm(w), _Mlp(w), nn.LayerNorm(w)


class _Transformer(nn.Module):
    def __init__(self, w, n):
        super().__init__()
        self.resblocks = nn.ModuleList([ResidualAttentionBlock(w) for _ in range(n)])


class CLIPTextEncoder(FrozenCausalStack):
    def __init__(self, width=512, layers=12, embed_dim=1024, vocab_size=49408, context_length=77, compute_dtype=torch.bfloat16):
        super().__init__()
        assert width % HEAD_DIM == 0, width
        self.width, self.heads, self.context_length, self.compute_dtype = width, width // HEAD_DIM, context_length, compute_dtype
        self.token_embedding = nn.Embedding(vocab_size, width)
        self.positional_embedding = nn.Parameter(torch.empty(context_length, width))
        self.transformer = _Transformer(width, layers)
        self.ln_final = nn.LayerNorm(width)
        self.text_projection = nn.Parameter(torch.empty(width, embed_dim))
        for p in self.parameters():
            p.requires_grad = False

    # ---------------------------------------------------------------- construction / loading
    @staticmethod
    def geometry(state: Dict[str, torch.Tensor], prefix: str = "") -> dict:
        """constructor arguments read off a state dict whose encoder keys start with ``prefix``"""
        tok = state[prefix + "token_embedding.weight"]
        pat = re.compile("^" + re.escape(prefix) + r"transformer\.resblocks\.(\d+)\.")
        n = len({m.group(1) for m in map(pat.match, state.keys()) if m})
        return dict(width=tok.shape[1], layers=n, embed_dim=state[prefix + "text_projection"].shape[1], vocab_size=tok.shape[0],
                    context_length=state[prefix + "positional_embedding"].shape[0])

    @classmethod
    def from_state_dict(cls, state: Dict[str, torch.Tensor], compute_dtype=torch.bfloat16):
        """a state dict with exactly the encoder's own names"""
        enc = cls(**cls.geometry(state), compute_dtype=compute_dtype)
        enc.load_state_dict(state, strict=True)
        return enc

    @classmethod
    def from_checkpoint(cls, ckpt: Dict[str, torch.Tensor], compute_dtype=torch.bfloat16):
        """the encoder inside a detector / CLIP checkpoint: RegionCLIP keeps it under ``lang_encoder.*``, OpenAI CLIP at the top
        level.  Names are matched by ``checkpoint.convert_clip_state`` (longest dotted suffix) against ``lang_encoder.<name>``."""
        from ..checkpoint import convert_clip_state
        prefix = next((p for p in ("lang_encoder.", "") if p + "token_embedding.weight" in ckpt), None)
        if prefix is None:
            raise KeyError("checkpoint holds no CLIP text encoder (no 'lang_encoder.token_embedding.weight' / 'token_embedding.weight')")
        enc = cls(**cls.geometry(ckpt, prefix), compute_dtype=compute_dtype)
        own = {"lang_encoder." + k: v for k, v in enc.state_dict().items()}
        conv, pairs = convert_clip_state(own, ckpt)
        missing = sorted(k for k in own if k not in pairs)
        if missing:
            raise KeyError(f"text encoder tensors missing from the checkpoint: {missing[:8]}{' ...' if len(missing) > 8 else ''}")
        enc.load_state_dict({k[len("lang_encoder."):]: conv[k] for k in own}, strict=True)
        enc.matched = pairs
        return enc

    def _prepare(self):
        w, f = partial(gemm_weight, dtype=self.compute_dtype), f32
        blocks = [Layer(f(b.ln_1.weight), f(b.ln_1.bias), w(b.attn.in_proj_weight), f(b.attn.in_proj_bias),
                        w(b.attn.out_proj.weight), f(b.attn.out_proj.bias), f(b.ln_2.weight), f(b.ln_2.bias),
                        w(b.mlp.c_fc.weight), f(b.mlp.c_fc.bias), w(b.mlp.c_proj.weight), f(b.mlp.c_proj.bias))
                  for b in self.transformer.resblocks]
        return _Prepared(blocks, tok=w(self.token_embedding.weight), pos=f(self.positional_embedding), ln_w=f(self.ln_final.weight),
                         ln_b=f(self.ln_final.bias), proj=w(self.text_projection.detach().t()))         # proj [D, W]

    # ---------------------------------------------------------------- forward
    def _check_ids(self, ids):
        """-> (eot positions [n] on ids' device, the T the batch runs at); rejects ids outside the vocabulary"""
        assert ids.dim() == 2 and ids.dtype == torch.int64 and ids.shape[1] <= self.context_length, ids.shape
        eot = ids.argmax(dim=-1)                          # first maximum: the EOT id is the largest CLIP id (encode_text)
        stats = torch.stack([eot.max(), ids.min(), ids.max()]).tolist() if ids.numel() else [0, 0, 0]
        if stats[1] < 0 or stats[2] >= self.token_embedding.num_embeddings:
            raise ValueError(f"token ids outside [0, {self.token_embedding.num_embeddings}): {stats[1]} .. {stats[2]}")
        return eot, stats[0] + 1

    def encode_text(self, ids, truncate=True, group=1):
        """ids [n, <= 77] int64 (CPU or device) -> [n // group, D] f32: ``encode_text`` (clip_backbone.py:849-868), the projected
        ln_final feature of each sequence's EOT row (first argmax of its ids).  ``group`` > 1 averages each ``group`` consecutive
        sequences' ln_final features BEFORE the projection (the mean commutes with it), so the projection runs on n // group rows.
        ``truncate``: run at T = max(eot) + 1 (same value, see the module docstring) instead of the full width of ids."""
        dev = self.positional_embedding.device
        require_cuda(self.positional_embedding)
        n = ids.shape[0]
        assert n % group == 0, (n, group)
        eot, t = self._check_ids(ids)
        if not truncate:
            t = ids.shape[1]
        ids = ids[:, :t].to(dev, non_blocking=True).contiguous()
        eot = eot.to(dev)
        x = self._residual_stream(ids)
        P = self._prepared()
        rows = torch.arange(n, device=dev, dtype=torch.int64) * t + eot
        pooled = layers.text_pool(x, rows, P.ln_w, P.ln_b, group, out_dtype=self.compute_dtype)
        return hip.linear_fwd(pooled, P.proj, out_f32=True)

    def _residual_stream(self, ids):
        """ids [n, t] on the device -> the residual stream after the last block, [n*t, W] f32"""
        P = self._prepared()
        n, t = ids.shape
        return prefill(P.layers, layers.text_embed(ids, P.tok, P.pos), n, t, self.heads, self.compute_dtype, hip.quick_gelu_)

    def encode_prompt_ids(self, ids, counts: Sequence[int], chunk=8192, truncate=True):
        """ids [S, 77] int64 (CPU), the prompts of class c being ``counts[c]`` consecutive rows -> [C, D] f32, the mean over each
        class's prompts of the projected EOT features.  At most about ``chunk`` sequences are in flight at a time."""
        dev = self.positional_embedding.device
        C = len(counts)
        assert sum(counts) == ids.shape[0] and min(counts, default=1) > 0
        out = torch.empty((C, self.text_projection.shape[1]), device=dev, dtype=torch.float32)
        if len(set(counts)) <= 1:
            # one prompt count P: whole classes per chunk, the class mean taken in text_pool before the projection
            Pc = counts[0] if C else 1
            per = max(1, chunk // Pc)
            for c0 in range(0, C, per):
                c1 = min(C, c0 + per)
                out[c0:c1] = self.encode_text(ids[c0 * Pc:c1 * Pc], truncate=truncate, group=Pc)
            return out
        # synonym lists of different lengths: per-sequence features, then the per-class mean
        seg = torch.repeat_interleave(torch.arange(C), torch.tensor(counts)).to(dev)
        out.zero_()
        for s0 in range(0, ids.shape[0], chunk):
            s1 = min(ids.shape[0], s0 + chunk)
            out.index_add_(0, seg[s0:s1], self.encode_text(ids[s0:s1], truncate=truncate))
        return out / torch.tensor(counts, device=dev, dtype=torch.float32).unsqueeze(1)

    def encode_concepts(self, names, templates: Sequence[str], bpe: BPETokenizer, chunk=8192, truncate=True):
        """tools/extract_concept_features.py: for every class (a name or a list of synonyms) the mean over its prompts
        (synonyms x templates, ``prompt_engineering``) of the UNNORMALISED projected EOT features -> [C, D] f32"""
        ids, counts = tokenize_names(names, templates, bpe)
        return self.encode_prompt_ids(ids, counts, chunk=chunk, truncate=truncate)


def tokenize_names(names, templates, bpe):
    """-> (ids [S, 77] int64, prompts per class)"""
    prompts: List[str] = []
    counts = []
    for n in names:
        p = concept_prompts(n, templates)
        prompts += p
        counts.append(len(p))
    return tokenize_prompts(prompts, bpe), counts


def torch_encode_text(enc: CLIPTextEncoder, ids, dtype=torch.float32, truncate=True):
    """The reference's ``encode_text`` restated on plain torch ops in ``dtype`` on the encoder's device -- the yardstick the tests
    and tools/text_encoder_bench.py compare against.  Never called by the encoder itself (that would be a silent fallback)."""
    dev = enc.positional_embedding.device
    ids = ids.to(dev)
    eot = ids.argmax(dim=-1)
    t = int(eot.max()) + 1 if truncate else ids.shape[1]
    ids = ids[:, :t]
    n, W, H = ids.shape[0], enc.width, enc.heads

    def lin(x, m):
        return x @ m.weight.to(dtype).t() + m.bias.to(dtype)

    def ln(x, m):
        return torch.nn.functional.layer_norm(x, (W,), m.weight.to(dtype), m.bias.to(dtype), 1e-5)

    x = enc.token_embedding.weight.to(dtype)[ids] + enc.positional_embedding.to(dtype)[:t]
    mask = torch.full((t, t), float("-inf"), device=dev, dtype=dtype).triu_(1)
    for b in enc.transformer.resblocks:
        y = ln(x, b.ln_1)
        qkv = y @ b.attn.in_proj_weight.to(dtype).t() + b.attn.in_proj_bias.to(dtype)
        q, k, v = qkv.view(n, t, 3, H, HEAD_DIM).permute(2, 0, 3, 1, 4)
        att = torch.softmax((q @ k.transpose(-1, -2)) * HEAD_DIM ** -0.5 + mask, dim=-1)
        x = x + lin((att @ v).permute(0, 2, 1, 3).reshape(n, t, W), b.attn.out_proj)
        h = lin(ln(x, b.ln_2), b.mlp.c_fc)
        x = x + lin(h * torch.sigmoid(1.702 * h), b.mlp.c_proj)
    x = ln(x, enc.ln_final)
    return x[torch.arange(n, device=dev), eot] @ enc.text_projection.to(dtype)


def load_text_encoder(path: Optional[str] = None, synthetic_seed: Optional[int] = None, compute_dtype=torch.bfloat16, **geometry):
    """the encoder from a checkpoint file (``MODEL.WEIGHTS``) or from ``synthetic.make_text_state_dict(seed, **geometry)``"""
    if synthetic_seed is not None:
        from ..synthetic import make_text_state_dict
        return CLIPTextEncoder.from_state_dict(make_text_state_dict(synthetic_seed, **geometry), compute_dtype)
    from ..checkpoint import read_state
    return CLIPTextEncoder.from_checkpoint(read_state(path)["model"], compute_dtype)


def gemm_flops(n_seq: int, t: int, width: int, layers_: int, embed_dim: int) -> float:
    """the encoder's GEMM FLOPs for n_seq sequences run at t tokens (2 M N K per linear; attention's q k^T and p v excluded)"""
    per_layer = 2 * n_seq * t * (3 * width * width + width * width + 8 * width * width)
    return float(layers_ * per_layer + 2 * n_seq * width * embed_dim)
