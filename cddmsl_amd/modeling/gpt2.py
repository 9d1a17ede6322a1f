"""GPT-2 decoder (frozen) for ClipCap captioning -- ``ClipCaptionModel.gpt`` (detectron2/modeling/backbone/clipcap/clipcap.py) with
the reference's ``generate2`` loop (clipcap.py:732-790, used by gen_captions.py): the 40 prefix rows of ``TransformerMapper`` are
GPT-2's input embeddings, then tokens are appended one at a time.

Greedy decoding.  ``generate2`` filters the logits with top-p before its arg-max; the top-p filter keeps the most probable token
by construction, so the arg-max of the filtered logits is the arg-max of the raw logits: greedy decoding is exactly what it
computes.  ``generate`` keeps a KV cache instead of recomputing the whole sequence every step (``torch_gpt2_logits`` /
``torch_greedy`` restate the recomputing loop for tests and tools/caption_bench.py).

Parameters follow GPT-2's names (``wte``, ``wpe``, ``h.{i}.{ln_1, attn.c_attn, attn.c_proj, ln_2, mlp.c_fc, mlp.c_proj}``, ``ln_f``),
but the linear weights are stored [out, in] (GPT-2's Conv1D stores [in, out]; they are transposed once at load).  The LM head is
tied to ``wte``.  The geometry comes from the tensors; heads = n_embd / 64 for every GPT-2 size.

Beam search.  ClipCap's other decoding mode (``inference(prefix, use_beam_search=True)``, clipcap.py:196-205; the reference names
``generate_beam`` there and defines it nowhere) is ``generate_beam``: length-normalised beam search of width B <= 8.  Every live
beam offers the B largest logits of its row (within a beam the key is monotone in the logit, so these are all it can contribute), a
stopped beam offers itself; the B candidates with the largest ``sum of log-probabilities / length`` survive, ties to the lower
(beam, token).  The prefix is prefilled once per caption and shared by its beams; the cache of the generated positions is never
reordered: an ancestry table [rows, T - 1] says which beam slot wrote each step of a beam's history, the selection kernel permutes
that table (and the token history) instead of the cache, and the attention kernel reads keys and values through it.
``torch_beam`` restates the semantics with a full recompute on torch ops.

Two paths, as in the text encoder:
* bf16 throughput path, f32 residual stream.  Prefill (prefix rows): ``causal_stack.prefill`` with gelu_new, which also fills the
  KV cache.  Decode step (one row per caption): skinny GEMM (M <= 64 rows) with bias / residual / gelu_new
  epilogues, decode attention over the KV cache, ln_f + the LM-head arg-max kernel (the logits are never written).  Beam search:
  the same step on captions x B rows with ``decode_attention_beam``, the LM-head top-B + log-sum-exp kernel and ``beam_step``.
* exact-f32 parity path (``compute_dtype=torch.float32``): the f32 GEMM instantiation for every linear, attention and the LM head
  on torch f32 ops (no f32 kernel exists for them); beam search gathers its caches through the same ancestry table, takes the top B
  by a stable descending sort and selects with the same ``beam_step`` kernel.
"""
import os
import re
from functools import partial
from typing import Dict, Optional

import torch
from torch import nn

from .. import hip, layers
from .._lib import require_cuda
from .causal_stack import HEAD_DIM, FrozenCausalStack, Layer, _Prepared, f32, gemm_weight, prefill

MAX_ROWS = 64            # decode-step rows per chunk: the skinny GEMM's and the LM head's M bound
MAX_BEAMS = 8            # beam_step holds a caption's B x B candidates in one wave
_IGNORED = re.compile(r"^h\.\d+\.attn\.(bias|masked_bias)$")     # the causal-mask buffers older transformers files carry


class _Lin(nn.Module):
    def __init__(self, i, o):
        super().__init__()
        self.weight = nn.Parameter(torch.empty(o, i))       # [out, in]
        self.bias = nn.Parameter(torch.empty(o))


class _Attn(nn.Module):
    def __init__(self, e):
        super().__init__()
        self.c_attn, self.c_proj = _Lin(e, 3 * e), _Lin(e, e)


class _Mlp(nn.Module):
    def __init__(self, e):
        super().__init__()
        self.c_fc, self.c_proj = _Lin(e, 4 * e), _Lin(4 * e, e)


class _Block(nn.Module):
    def __init__(self, e):
        super().__init__()
        self.ln_1, self.attn, self.ln_2, self.mlp = nn.LayerNorm(e), _Attn(e), nn.LayerNorm(e), _Mlp(e)


class GPT2Decoder(FrozenCausalStack):
    def __init__(self, n_layer=12, n_embd=768, vocab_size=50257, n_positions=1024, compute_dtype=torch.bfloat16, eps=1e-5):
        super().__init__()
        assert n_embd % HEAD_DIM == 0, n_embd
        self.n_embd, self.heads, self.n_positions, self.compute_dtype, self.eps = n_embd, n_embd // HEAD_DIM, n_positions, compute_dtype, eps
        self.wte = nn.Embedding(vocab_size, n_embd)
        self.wpe = nn.Embedding(n_positions, n_embd)
        self.h = nn.ModuleList([_Block(n_embd) for _ in range(n_layer)])
        self.ln_f = nn.LayerNorm(n_embd, eps=eps)
        for p in self.parameters():
            p.requires_grad = False
        # decode-step linears: "skinny" (the M <= 64 kernel) or "gemm" (the conv/GEMM kernel, hip.linear_fwd): a measurement switch
        self.decode_linear = os.environ.get("CDDMSL_GPT2_DECODE_LINEAR", "skinny")

    @property
    def vocab_size(self):
        return self.wte.num_embeddings

    # ---------------------------------------------------------------- loading
    @classmethod
    def from_state_dict(cls, state: Dict[str, torch.Tensor], compute_dtype=torch.bfloat16):
        """GPT-2 from a ClipCap file (``gpt.transformer.*`` + ``gpt.lm_head.weight``; the other entries, ``clip_project.*``, are
        not GPT-2's and are skipped), a transformers ``GPT2LMHeadModel`` file (``transformer.*`` + ``lm_head.weight``) or bare
        ``GPT2Model`` keys.  Conv1D weights [in, out] are transposed; ``lm_head.weight`` must equal ``wte.weight`` (tied)."""
        if "gpt.transformer.wte.weight" in state:
            body, head = "gpt.transformer.", "gpt.lm_head.weight"
            own = {k for k in state if k.startswith("gpt.")}
        elif "transformer.wte.weight" in state:
            body, head, own = "transformer.", "lm_head.weight", set(state)
        elif "wte.weight" in state:
            body, head, own = "", "lm_head.weight", set(state)
        else:
            raise KeyError("no GPT-2 weights: none of 'gpt.transformer.wte.weight', 'transformer.wte.weight', 'wte.weight' is present")
        sd = {k[len(body):]: v for k, v in state.items() if k in own and k.startswith(body)}
        unexpected = sorted(k for k in own if not k.startswith(body) and k != head)
        pat = re.compile(r"^h\.(\d+)\.")
        n_layer = len({m.group(1) for m in map(pat.match, sd) if m})
        wte, wpe = sd["wte.weight"], sd.get("wpe.weight")
        if wpe is None:
            raise KeyError(f"GPT-2 tensors missing: ['{body}wpe.weight']")
        dec = cls(n_layer, wte.shape[1], wte.shape[0], wpe.shape[0], compute_dtype=compute_dtype)
        expected = set(dec.state_dict())
        missing = sorted(body + k for k in expected if k not in sd)
        unexpected += sorted(body + k for k in sd if k not in expected and not _IGNORED.match(k))
        if missing or unexpected:
            raise KeyError(f"GPT-2 state dict does not match: missing {missing[:8]}{' ...' if len(missing) > 8 else ''}, "
                           f"unexpected {unexpected[:8]}{' ...' if len(unexpected) > 8 else ''}")
        own_sd = {}
        for k in expected:
            v = sd[k]
            if re.match(r"^h\.\d+\.(attn\.c_attn|attn\.c_proj|mlp\.c_fc|mlp\.c_proj)\.weight$", k):
                v = v.t()                                                   # Conv1D [in, out] -> [out, in]
            if tuple(v.shape) != tuple(dec.state_dict()[k].shape):
                raise ValueError(f"{body + k}: shape {tuple(sd[k].shape)} does not fit GPT-2 with n_embd {dec.n_embd}")
            own_sd[k] = v.contiguous()
        if head in state and not torch.equal(state[head].to(wte.dtype), wte):
            raise ValueError(f"{head} differs from {body}wte.weight: only a tied LM head is supported")
        dec.load_state_dict(own_sd, strict=True)
        return dec

    def _prepare(self):
        w, f = partial(gemm_weight, dtype=self.compute_dtype), f32
        blocks = [Layer(f(b.ln_1.weight), f(b.ln_1.bias), w(b.attn.c_attn.weight), f(b.attn.c_attn.bias),
                        w(b.attn.c_proj.weight), f(b.attn.c_proj.bias), f(b.ln_2.weight), f(b.ln_2.bias),
                        w(b.mlp.c_fc.weight), f(b.mlp.c_fc.bias), w(b.mlp.c_proj.weight), f(b.mlp.c_proj.bias))
                  for b in self.h]
        return _Prepared(blocks, wte=w(self.wte.weight), wpe=f(self.wpe.weight), ln_w=f(self.ln_f.weight), ln_b=f(self.ln_f.bias))

    # ---------------------------------------------------------------- generation
    @torch.no_grad()
    def generate(self, prefix_embeds, max_tokens=67, stop_id: Optional[int] = None, return_logits=False, check_every=4):
        """prefix_embeds [N, P, n_embd] f32 -> (tokens [N, max_tokens] int64, lengths [N] int64[, logits [N, steps, V] f32]).
        Greedy decoding with a KV cache.  A sequence ends after it emits ``stop_id`` (kept in it); the batch ends when every
        sequence has ended (tested every ``check_every`` steps) or after ``max_tokens``.  Entries at and after ``lengths[n]``
        are -1; a sequence's tokens do not depend on the other sequences of the batch.  Batches above 64 rows run in chunks of
        64.  ``return_logits``: the logits of every step run (the LM head's optional output on the bf16 path)."""
        require_cuda(self.wte.weight)
        dev = self.wte.weight.device
        N, P, E = prefix_embeds.shape
        assert E == self.n_embd and max_tokens >= 1
        if P + max_tokens - 1 > min(self.n_positions, 1024) or (self.compute_dtype == torch.bfloat16 and P > 128):
            raise ValueError(f"prefix {P} + {max_tokens} tokens does not fit n_positions {self.n_positions}")
        prefix_embeds = prefix_embeds.to(dev, torch.float32).contiguous()
        Pm = self._prepared()                        # once per call: the key walks every parameter
        toks, lens, logs = [], [], []
        for c0 in range(0, N, MAX_ROWS):
            t, lg = self._generate_chunk(Pm, prefix_embeds[c0:c0 + MAX_ROWS], max_tokens, stop_id, return_logits, check_every)
            toks.append(t)
            logs.append(lg)
        tokens = torch.cat(toks) if toks else torch.empty((0, max_tokens), dtype=torch.int64, device=dev)
        tokens, lengths = finish_tokens(tokens, stop_id)
        if not return_logits:
            return tokens, lengths
        steps = max(lg.shape[1] for lg in logs) if logs else 0
        logits = torch.full((N, steps, self.vocab_size), float("nan"), device=dev)
        r = 0
        for lg in logs:
            logits[r:r + lg.shape[0], :lg.shape[1]] = lg
            r += lg.shape[0]
        return tokens, lengths, logits

    def _generate_chunk(self, Pm, prefix, max_tokens, stop_id, want_logits, check_every):
        T = self.compute_dtype
        n, P, E = prefix.shape
        H, scale = self.heads, HEAD_DIM ** -0.5
        dev = prefix.device
        Lmax = P + max_tokens - 1
        kc = torch.empty((len(Pm.layers), n, Lmax, E), device=dev, dtype=T)
        vc = torch.empty_like(kc)
        tokens = torch.full((n, max_tokens), -1, device=dev, dtype=torch.int64)
        logits = [] if want_logits else None

        # prefill: the P prefix rows of every sequence, their keys and values into the cache
        x = prefill(Pm.layers, layers.prefix_position_embed(prefix, Pm.wpe), n, P, H, T, hip.gelu_new_, self.eps, kv=(kc, vc))
        x = x.view(n, P, E)[:, P - 1].contiguous()
        self._head(Pm, x, tokens[:, 0], logits)

        def attend(li, qkv):
            if T == torch.bfloat16:
                return layers.decode_attention(qkv, kc[li], vc[li], L, H, scale)
            q3 = qkv.view(n, 3, H, HEAD_DIM)
            kc[li, :, L - 1] = qkv[:, E:2 * E]
            vc[li, :, L - 1] = qkv[:, 2 * E:]
            kk = kc[li, :, :L].view(n, L, H, HEAD_DIM).transpose(1, 2)          # [n, H, L, 64]
            vv = vc[li, :, :L].view(n, L, H, HEAD_DIM).transpose(1, 2)
            att = torch.softmax((q3[:, 0].unsqueeze(2) @ kk.transpose(-1, -2)) * scale, dim=-1)   # [n, H, 1, L]
            return (att @ vv).reshape(n, E).contiguous()

        xb = torch.empty((n, E), device=dev, dtype=torch.float32)
        for s in range(1, max_tokens):
            if stop_id is not None and s % check_every == 0 and bool((tokens[:, :s] == stop_id).any(dim=1).all()):
                break
            L = P + s
            x = self._decode_step(Pm, layers.token_position_embed(tokens[:, s - 1], Pm.wte, Pm.wpe, L - 1, out=xb), attend)
            self._head(Pm, x, tokens[:, s], logits)
        return tokens, (torch.stack(logits, dim=1) if want_logits else None)

    def _decode_step(self, Pm, x, attend):
        """one decode step: the rows x [rows, E] f32 (one per sequence) through every layer -> [rows, E] f32.  ``attend(li, qkv)`` is
        layer li's attention of this step's c_attn output over its cache (which it also extends) -> o [rows, E]."""
        T = self.compute_dtype
        for li, B in enumerate(Pm.layers):
            y = hip.layernorm_fwd(x, B.ln1_w, B.ln1_b, T, self.eps)[0]
            if T == torch.bfloat16 and self.decode_linear == "skinny":
                qkv = layers.skinny_linear(y, B.w_qkv, B.b_qkv)
                o = attend(li, qkv)
                x = layers.skinny_linear(o, B.w_out, B.b_out, residual=x, out=x)
                y = hip.layernorm_fwd(x, B.ln2_w, B.ln2_b, T, self.eps)[0]
                h = layers.skinny_linear(y, B.w_fc, B.b_fc, gelu=True)
                x = layers.skinny_linear(h, B.w_proj, B.b_proj, residual=x, out=x)
                continue
            qkv = hip.linear_fwd(y, B.w_qkv, bias=B.b_qkv)
            o = attend(li, qkv)
            x = hip.linear_fwd(o, B.w_out, bias=B.b_out, residual=x, out_f32=True)
            y = hip.layernorm_fwd(x, B.ln2_w, B.ln2_b, T, self.eps)[0]
            h = hip.gelu_new_(hip.linear_fwd(y, B.w_fc, bias=B.b_fc))
            x = hip.linear_fwd(h, B.w_proj, bias=B.b_proj, residual=x, out_f32=True)
        return x

    def _head(self, Pm, x, out_ids, logits):
        """ln_f + the tied LM head's arg-max of rows x [n, E] f32 into out_ids (a strided column of the token buffer)"""
        y = hip.layernorm_fwd(x, Pm.ln_w, Pm.ln_b, self.compute_dtype, self.eps)[0]
        if self.compute_dtype == torch.bfloat16:
            r = hip.lm_head_argmax(y, Pm.wte, ids=out_ids, logits=logits is not None)
            if logits is not None:
                logits.append(r[1])
            return
        lg = y @ Pm.wte.t()
        out_ids.copy_(lg.argmax(dim=1))
        if logits is not None:
            logits.append(lg)

    # ---------------------------------------------------------------- training the mapper against the frozen decoder
    _train = None

    def _train_weights(self):
        """the frozen linears as ``layers.PreparedWeight`` (forward and input-gradient copies in the compute dtype) plus the LM head's
        table, ``wte`` with zero rows up to a multiple of 8 (the GEMMs' row alignment); rebuilt when a parameter or the dtype changes"""
        key = (self.compute_dtype, tuple((p.data_ptr(), p._version) for p in self.parameters()))
        if self._train is None or self._train[0] != key:
            pw = lambda m: layers.PreparedWeight(m.weight, None, frozen=True)
            V, E = self.wte.weight.shape
            head = torch.zeros((V + 7) // 8 * 8, E, device=self.wte.weight.device, dtype=torch.float32)
            head[:V] = self.wte.weight.detach()
            self._train = (key, [(pw(b.attn.c_attn), pw(b.attn.c_proj), pw(b.mlp.c_fc), pw(b.mlp.c_proj)) for b in self.h],
                           layers.PreparedWeight(head, None, frozen=True))
        return self._train[1], self._train[2]

    def caption_loss(self, prefix_embeds, tokens):
        """ClipCap's training loss (clipcap.py ``ClipCaptionModel.forward`` + ``train``): prefix_embeds [n, P, n_embd] f32 (the
        mapper's output, the only input that gets a gradient) and tokens [n, L] int64 (0 where padded) -> the mean cross-entropy of
        predicting tokens[:, j] from row P - 1 + j, over the tokens that are not 0, as a 0-dim f32 tensor.

        The input is ``cat(prefix, wte[tokens]) + wpe[0 .. P+L)`` through the frozen blocks and ``ln_f``; the LM head runs for rows
        P-1 .. P+L-2 only: the reference's ``logits[:, prefix_length - 1:-1]`` against ``tokens.flatten()`` with ``ignore_index=0``.
        Token id 0 is both the pad and a real token ("!"); it stays ignored wherever it stands, as in the reference.

        The reference also passes an ``attention_mask`` that hides the pads.  Pads sit at the tail of a caption, and under the
        causal mask a row sees only the rows before it, so no row that is scored (each predicts a real token, hence stands before
        every pad) ever sees one: the mask changes nothing at the scored rows and is not formed here.

        P + L <= 128 (the fused attention kernels' limit).  bf16 path: attention forward and backward on the fused causal kernels;
        exact-f32 path (``compute_dtype=torch.float32``): attention on torch f32 ops, everything else on the same kernels.
        Raises ``ValueError`` when every token is 0."""
        require_cuda(self.wte.weight)
        dev, T = self.wte.weight.device, self.compute_dtype
        n, P, E = prefix_embeds.shape
        L = tokens.shape[1]
        t = P + L
        assert E == self.n_embd and tokens.shape[0] == n and tokens.dtype == torch.int64 and P >= 1 and L >= 1
        if t > min(self.n_positions, 128):
            raise ValueError(f"prefix {P} + {L} tokens exceeds {min(self.n_positions, 128)} positions")
        if int(tokens.min()) < 0 or int(tokens.max()) >= self.vocab_size:
            raise ValueError("token ids outside [0, vocab_size)")
        Pm = self._prepared()
        blocks, head = self._train_weights()
        H, scale = self.heads, HEAD_DIM ** -0.5
        tokens = tokens.to(dev)
        x = torch.cat((prefix_embeds.to(dev, torch.float32), self.wte.weight.detach()[tokens]), dim=1) + Pm.wpe[:t]
        x = x.view(n * t, E)
        mask = None
        for B, (w_qkv, w_out, w_fc, w_proj) in zip(Pm.layers, blocks):
            y, xs = layers.layer_norm_skip(x, B.ln1_w, B.ln1_b, T, self.eps)
            qkv = layers.linear(y, w_qkv, B.b_qkv, train_w=False)
            if T == torch.bfloat16:
                o = layers.causal_attention_grad(qkv, t, H, scale)
            else:
                if mask is None:
                    mask = torch.full((t, t), float("-inf"), device=dev).triu_(1)
                q, k, v = qkv.view(n, t, 3, H, HEAD_DIM).permute(2, 0, 3, 1, 4)
                att = torch.softmax((q @ k.transpose(-1, -2)) * scale + mask, dim=-1)
                o = (att @ v).permute(0, 2, 1, 3).reshape(n * t, E).contiguous()
            x = layers.linear(o, w_out, B.b_out, out_f32=True, train_w=False, residual=xs)
            y, xs = layers.layer_norm_skip(x, B.ln2_w, B.ln2_b, T, self.eps)
            h = layers.gelu_new(layers.linear(y, w_fc, B.b_fc, train_w=False))
            x = layers.linear(h, w_proj, B.b_proj, out_f32=True, train_w=False, residual=xs)
        rows = x.view(n, t, E)[:, P - 1:t - 1].reshape(n * L, E)
        y = layers.layer_norm(rows, Pm.ln_w, Pm.ln_b, T, self.eps)
        return layers.lm_head_cross_entropy(y, head, tokens.reshape(n * L), self.vocab_size, 0)


    # ---------------------------------------------------------------- beam search
    @torch.no_grad()
    def generate_beam(self, prefix_embeds, beam_size=5, max_tokens=67, stop_id: Optional[int] = None, check_every=4):
        """prefix_embeds [N, P, n_embd] f32 -> (tokens [N, B, max_tokens] int64, lengths [N, B] int64, scores [N, B] f32), B =
        ``beam_size`` <= 8: length-normalised beam search (the module docstring has the rule), a caption's beams sorted by score =
        sum of the tokens' log-probabilities / length, best first, ties to the lower beam.  A beam ends after it emits ``stop_id``
        (kept in it); decoding ends when every beam of the chunk has ended (tested every ``check_every`` steps) or after
        ``max_tokens``.  Entries at and after a beam's length are -1; a caption's result does not depend on the other captions.
        Chunks hold 64 // B captions.  ``beam_size=1`` gives ``generate``'s tokens."""
        require_cuda(self.wte.weight)
        dev = self.wte.weight.device
        N, P, E = prefix_embeds.shape
        assert E == self.n_embd and max_tokens >= 1
        if not 1 <= beam_size <= min(MAX_BEAMS, self.vocab_size):
            raise ValueError(f"beam_size {beam_size} outside 1..{min(MAX_BEAMS, self.vocab_size)}")
        if P + max_tokens - 1 > min(self.n_positions, 1024) or (self.compute_dtype == torch.bfloat16 and P > 128):
            raise ValueError(f"prefix {P} + {max_tokens} tokens does not fit n_positions {self.n_positions}")
        prefix_embeds = prefix_embeds.to(dev, torch.float32).contiguous()
        Pm = self._prepared()
        per = MAX_ROWS // beam_size
        outs = [self._beam_chunk(Pm, prefix_embeds[c0:c0 + per], beam_size, max_tokens, stop_id, check_every) for c0 in range(0, N, per)]
        if not outs:
            return (torch.empty((0, beam_size, max_tokens), dtype=torch.int64, device=dev),
                    torch.empty((0, beam_size), dtype=torch.int64, device=dev), torch.empty((0, beam_size), device=dev))
        return tuple(torch.cat(v) for v in zip(*outs))

    def _beam_chunk(self, Pm, prefix, B, max_tokens, stop_id, check_every):
        T = self.compute_dtype
        n, P, E = prefix.shape
        rows, H, scale, nl = n * B, self.heads, HEAD_DIM ** -0.5, len(Pm.layers)
        dev = prefix.device
        pk = torch.empty((nl, n, P, E), device=dev, dtype=T)                 # the prefix's keys / values: per caption, shared by its beams
        pv = torch.empty_like(pk)
        gk = torch.empty((nl, rows, max(max_tokens - 1, 1), E), device=dev, dtype=T)   # generated positions: written once, never moved
        gv = torch.empty_like(gk)
        cur, nxt = hip.BeamState(n, B, max_tokens, dev), hip.BeamState(n, B, max_tokens, dev)

        x = prefill(Pm.layers, layers.prefix_position_embed(prefix, Pm.wpe), n, P, H, T, hip.gelu_new_, self.eps, kv=(pk, pv))
        x = x.view(n, P, E)[:, P - 1].contiguous()
        hip.beam_step(*self._head_topk(Pm, x, B), nxt, cur, 0, stop_id)      # step 0: one row per caption

        cap = torch.arange(rows, device=dev) // B                            # (exact-f32 path) a row's caption, its first row
        base, steps = (cap * B).unsqueeze(1), torch.arange(max(max_tokens - 1, 1), device=dev)

        def attend(li, qkv):
            if T == torch.bfloat16:
                return layers.decode_attention_beam(qkv, pk[li], pv[li], gk[li], gv[li], cur.anc, L, B, H, scale)
            t = L - 1 - P                                                    # this step's generated position
            gk[li, :, t] = qkv[:, E:2 * E]
            gv[li, :, t] = qkv[:, 2 * E:]
            own = base + cur.anc[:, :t].long()                               # [rows, t]: the row that holds step j of this beam's history
            kk = torch.cat([pk[li][cap], gk[li][own, steps[:t]], qkv[:, None, E:2 * E]], 1).view(rows, L, H, HEAD_DIM).transpose(1, 2)
            vv = torch.cat([pv[li][cap], gv[li][own, steps[:t]], qkv[:, None, 2 * E:]], 1).view(rows, L, H, HEAD_DIM).transpose(1, 2)
            att = torch.softmax((qkv.view(rows, 3, H, HEAD_DIM)[:, 0].unsqueeze(2) @ kk.transpose(-1, -2)) * scale, dim=-1)
            return (att @ vv).reshape(rows, E).contiguous()

        xb = torch.empty((rows, E), device=dev, dtype=torch.float32)
        for s in range(1, max_tokens):
            if stop_id is not None and s % check_every == 0 and bool(cur.stop.all()):
                break
            L = P + s
            x = self._decode_step(Pm, layers.token_position_embed(cur.next_tok, Pm.wte, Pm.wpe, L - 1, out=xb), attend)
            hip.beam_step(*self._head_topk(Pm, x, B), cur, nxt, s, stop_id)
            cur, nxt = nxt, cur
        scores = cur.sum / cur.len.float()
        order = torch.sort(scores, dim=1, descending=True, stable=True).indices
        tokens = cur.hist.long().gather(1, order.unsqueeze(2).expand(n, B, max_tokens))
        return tokens, cur.len.long().gather(1, order), scores.gather(1, order)

    def _head_topk(self, Pm, x, B):
        """ln_f + the tied LM head of rows x [m, E] f32 -> (vals [m, B] f32, idx [m, B] int32, logZ [m] f32): each row's B largest
        logits (larger value, then lower index) and its log-sum-exp"""
        y = hip.layernorm_fwd(x, Pm.ln_w, Pm.ln_b, self.compute_dtype, self.eps)[0]
        if self.compute_dtype == torch.bfloat16:
            return hip.lm_head_topk(y, Pm.wte, B)
        lg = y @ Pm.wte.t()
        top = torch.sort(lg, dim=1, descending=True, stable=True)
        return top.values[:, :B].contiguous(), top.indices[:, :B].to(torch.int32).contiguous(), torch.logsumexp(lg, dim=1)


def finish_tokens(tokens, stop_id: Optional[int]):
    """tokens [N, T] as generated (-1 where a step was not run) -> (tokens with every entry after a sequence's stop token set to -1,
    lengths [N]): a sequence's length runs to its first ``stop_id`` inclusive, else to its first -1 or T"""
    N, T = tokens.shape
    pos = torch.arange(T, device=tokens.device).expand(N, T)
    end = torch.where(tokens < 0, pos, torch.full_like(pos, T)).min(dim=1).values
    if stop_id is not None:
        hit = torch.where(tokens == stop_id, pos + 1, torch.full_like(pos, T)).min(dim=1).values
        end = torch.minimum(end, hit)
    out = torch.where(pos < end.unsqueeze(1), tokens, torch.full_like(tokens, -1))
    return out, end


def torch_gpt2_logits(dec: GPT2Decoder, embeds, dtype=torch.float32):
    """GPT-2's forward restated on plain torch ops: input embeddings [N, T, E] -> logits [N, T, V] (wpe[0..T-1] added, causal
    attention, tied LM head).  The yardstick of the tests and tools/caption_bench.py; never called by the decoder itself."""
    dev = dec.wte.weight.device
    x = embeds.to(dev, dtype)
    N, T, E = x.shape
    H = dec.heads

    def lin(v, m):
        return v @ m.weight.to(dtype).t() + m.bias.to(dtype)

    def ln(v, m):
        return torch.nn.functional.layer_norm(v, (E,), m.weight.to(dtype), m.bias.to(dtype), dec.eps)

    x = x + dec.wpe.weight.to(dtype)[:T]
    mask = torch.full((T, T), float("-inf"), device=dev, dtype=dtype).triu_(1)
    for b in dec.h:
        q, k, v = lin(ln(x, b.ln_1), b.attn.c_attn).view(N, T, 3, H, HEAD_DIM).permute(2, 0, 3, 1, 4)
        att = torch.softmax((q @ k.transpose(-1, -2)) * HEAD_DIM ** -0.5 + mask, dim=-1)
        x = x + lin((att @ v).permute(0, 2, 1, 3).reshape(N, T, E), b.attn.c_proj)
        h = lin(ln(x, b.ln_2), b.mlp.c_fc)
        h = 0.5 * h * (1.0 + torch.tanh(0.7978845608028654 * (h + 0.044715 * h ** 3)))
        x = x + lin(h, b.mlp.c_proj)
    return ln(x, dec.ln_f) @ dec.wte.weight.to(dtype).t()


def torch_greedy(dec: GPT2Decoder, prefix, max_tokens=67, stop_id: Optional[int] = None, dtype=torch.float32):
    """the reference's loop (generate2 without its top-p filter, which never removes the arg-max): the full sequence recomputed
    every step -> (tokens [N, max_tokens] int64 (-1 after a stop), lengths [N], per-step last-row logits [N, steps, V])"""
    dev = dec.wte.weight.device
    emb = prefix.to(dev, dtype)
    N = emb.shape[0]
    toks, logs = [], []
    done = torch.zeros(N, dtype=torch.bool, device=dev)
    for _ in range(max_tokens):
        lg = torch_gpt2_logits(dec, emb, dtype)[:, -1]
        t = lg.argmax(dim=1)
        toks.append(t)
        logs.append(lg)
        if stop_id is not None:
            done |= t == stop_id
            if bool(done.all()):
                break
        emb = torch.cat([emb, dec.wte.weight.to(dtype)[t].unsqueeze(1)], dim=1)
    tokens = torch.full((N, max_tokens), -1, dtype=torch.int64, device=dev)
    tokens[:, :len(toks)] = torch.stack(toks, dim=1)
    tokens, lengths = finish_tokens(tokens, stop_id)
    return tokens, lengths, torch.stack(logs, dim=1)


def torch_beam(dec: GPT2Decoder, prefix, beam_size=5, max_tokens=67, stop_id: Optional[int] = None, dtype=torch.float32):
    """``generate_beam``'s rule restated with the full sequence recomputed every step on plain torch ops (any device) -> (tokens
    [N, B, max_tokens] int64, lengths [N, B], scores [N, B] f32, gaps [N, steps] f32).  The logits are computed in ``dtype``, the
    selection in f32.  ``gaps[n, s]`` is the distance between the B-th and the (B+1)-th key of step s (inf when there is no
    (B+1)-th candidate): where it is small, another summation order may select differently.  Every beam offers B + 1 tokens here so
    that the (B+1)-th key is the true one; the B survivors are the same as with B tokens per beam."""
    dev = dec.wte.weight.device
    B, T, V = beam_size, max_tokens, dec.vocab_size
    N, P, E = prefix.shape
    K1 = min(B + 1, V)
    stop = -1 if stop_id is None else int(stop_id)
    wte = dec.wte.weight.to(dtype)
    inf = torch.tensor(float("inf"), device=dev)

    def top(lg):                                       # [..., V] f32 -> the K1 largest (larger value, then lower index), log-sum-exp
        st = torch.sort(lg, dim=-1, descending=True, stable=True)
        return st.values[..., :K1], st.indices[..., :K1], torch.logsumexp(lg, dim=-1)

    # step 0: the last prefix row's B best tokens
    vals, idx, logZ = top(torch_gpt2_logits(dec, prefix.to(dev, dtype), dtype)[:, -1].float())
    logp = vals - logZ.unsqueeze(1)
    bsum, blen = logp[:, :B].clone(), torch.ones((N, B), dtype=torch.int64, device=dev)
    hist = torch.full((N, B, T), -1, dtype=torch.int64, device=dev)
    hist[:, :, 0] = idx[:, :B]
    stopped = idx[:, :B] == stop
    gaps = [logp[:, B - 1] - logp[:, B] if K1 > B else inf.expand(N)]
    emb = prefix.to(dev, dtype).unsqueeze(1).expand(N, B, P, E)
    feed = torch.where(stopped, torch.full_like(idx[:, :B], max(stop, 0)), idx[:, :B])
    ar = torch.arange(N, device=dev).unsqueeze(1)
    for s in range(1, T):
        if bool(stopped.all()):
            break
        emb = torch.cat([emb, wte[feed].unsqueeze(2)], dim=2)                           # [N, B, P + s, E]
        vals, idx, logZ = top(torch_gpt2_logits(dec, emb.reshape(N * B, P + s, E), dtype)[:, -1].float().view(N, B, V))
        csum = bsum.unsqueeze(2) + (vals - logZ.unsqueeze(2))                           # [N, B, K1]
        clen = (blen + 1).unsqueeze(2).expand(N, B, K1).clone()
        valid = torch.ones((N, B, K1), dtype=torch.bool, device=dev)
        tok = idx.clone()
        # a stopped beam offers itself once, as token column 0
        first = torch.zeros(K1, dtype=torch.bool, device=dev)
        first[0] = True
        sb = stopped.unsqueeze(2)
        csum = torch.where(sb, bsum.unsqueeze(2).expand_as(csum), csum)
        clen = torch.where(sb, blen.unsqueeze(2).expand_as(clen), clen)
        tok = torch.where(sb, torch.zeros_like(tok), tok)
        valid &= ~sb | first
        key = csum / clen.float()
        flat = torch.arange(B, device=dev).view(1, B, 1) * V + tok
        key = torch.where(valid, key, -inf).view(N, B * K1)
        flat = torch.where(valid, flat, torch.full_like(flat, B * V)).view(N, B * K1)
        o1 = torch.sort(flat, dim=1, stable=True).indices                               # lower flat index first among equal keys
        o2 = torch.sort(key.gather(1, o1), dim=1, descending=True, stable=True).indices
        order = o1.gather(1, o2)                                                        # [N, B * K1], best first
        kbest, vbest = key.gather(1, order), valid.view(N, B * K1).gather(1, order)
        gaps.append(torch.where(vbest[:, B], kbest[:, B - 1] - kbest[:, B], inf) if B * K1 > B else inf.expand(N))
        win = order[:, :B]
        src = win // K1
        wtok, was = tok.view(N, B * K1).gather(1, win), stopped.gather(1, src)
        bsum, blen = csum.reshape(N, B * K1).gather(1, win), clen.reshape(N, B * K1).gather(1, win)
        hist = hist[ar, src]
        hist[:, :, s] = torch.where(was, torch.full_like(wtok, -1), wtok)
        stopped = was | (wtok == stop)
        emb = emb[ar, src]
        feed = torch.where(stopped, torch.full_like(wtok, max(stop, 0)), wtok)
    scores = bsum / blen.float()
    order = torch.sort(scores, dim=1, descending=True, stable=True).indices
    return hist[ar, order], blen.gather(1, order), scores.gather(1, order), torch.stack(gaps, dim=1)


def load_gpt2(path: str, compute_dtype=torch.bfloat16) -> GPT2Decoder:
    """GPT-2 from a file holding a ClipCap / transformers / bare state dict (``torch.load``; a ``{"model": ...}`` wrapper is opened)"""
    if not os.path.isfile(path):
        raise FileNotFoundError(f"GPT-2 weights not found: {path}")
    state = torch.load(path, map_location="cpu", weights_only=True)
    if isinstance(state, dict) and "model" in state and isinstance(state["model"], dict):
        state = state["model"]
    return GPT2Decoder.from_state_dict(state, compute_dtype)
