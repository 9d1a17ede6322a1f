"""What a frozen, forward-only, pre-LayerNorm causal transformer layer is -- shared by the CLIP text encoder (text_encoder.py) and the
GPT-2 decoder's prefill (gpt2.py): the prepared per-layer weights, their cache, and the loop over the layers.  Heads are 64 wide.

Two paths:
* bf16 throughput path: f32 residual stream; LayerNorm kernel -> bf16 GEMM operand; q | k | v GEMM; fused causal attention kernel;
  out-projection and c_proj add the f32 residual in the GEMM epilogue; the tower's activation kernel in place on the c_fc output;
* exact-f32 parity path (``dtype=torch.float32``): the f32 GEMM instantiation, attention on torch f32 ops (the fused kernel is
  bf16-only).
"""
from typing import NamedTuple

import torch
from torch import nn

from .. import hip, layers

HEAD_DIM = 64


class Layer(NamedTuple):
    """one block's device copies: GEMM weights ``w_*`` [N, K] in the compute dtype, biases ``b_*`` / LayerNorm affines ``ln*`` f32"""
    ln1_w: torch.Tensor
    ln1_b: torch.Tensor
    w_qkv: torch.Tensor      # [3W, W], rows q | k | v
    b_qkv: torch.Tensor
    w_out: torch.Tensor
    b_out: torch.Tensor
    ln2_w: torch.Tensor
    ln2_b: torch.Tensor
    w_fc: torch.Tensor       # [4W, W]
    b_fc: torch.Tensor
    w_proj: torch.Tensor     # [W, 4W]
    b_proj: torch.Tensor


def gemm_weight(t, dtype):
    """f32 master [N, K] -> compute-dtype GEMM operand (cddmsl_weight_prep)"""
    t = t.detach().float().contiguous()
    return hip.weight_prep(t.view(t.shape[0], 1, 1, t.shape[1]), None, dtype, True, False)[0].view(t.shape)


def f32(t):
    return t.detach().float().contiguous()


class _Prepared:
    """a tower's device copies: ``layers`` (one Layer per block) and, as attributes, the tables and final LayerNorm it names itself"""

    def __init__(self, blocks, **own):
        self.layers = list(blocks)
        self.__dict__.update(own)


class FrozenCausalStack(nn.Module):
    """base of the two towers: ``_prepared()`` caches the ``_Prepared`` that the subclass's ``_prepare()`` builds for
    ``self.compute_dtype`` until that dtype or a parameter (its storage or its version) changes"""
    _prep = None

    def _prepared(self) -> _Prepared:
        key = (self.compute_dtype, tuple((p.data_ptr(), p._version) for p in self.parameters()))
        if self._prep is None or self._prep[0] != key:
            self._prep = (key, self._prepare())
        return self._prep[1]


def prefill(blocks, x, n, t, heads, dtype, act_, eps=1e-5, kv=None):
    """the residual stream x [n*t, W] f32 (n sequences of t rows) through every Layer of ``blocks`` -> [n*t, W] f32.  ``act_`` is the
    in-place activation on the c_fc output (hip.quick_gelu_ / hip.gelu_new_).  ``kv`` = (kc, vc), each [len(blocks), n, >= t, W] in
    ``dtype``: layer li's keys and values of the t rows are copied to kc[li, :, :t] / vc[li, :, :t] (GPT-2's cache)."""
    W, scale = x.shape[1], HEAD_DIM ** -0.5
    mask = None
    for li, L in enumerate(blocks):
        y = hip.layernorm_fwd(x, L.ln1_w, L.ln1_b, dtype, eps)[0]
        qkv = hip.linear_fwd(y, L.w_qkv, bias=L.b_qkv)                                  # [n*t, 3W] in dtype
        if kv is not None:
            q3 = qkv.view(n, t, 3, W)
            kv[0][li, :, :t] = q3[:, :, 1]
            kv[1][li, :, :t] = q3[:, :, 2]
        if dtype == torch.bfloat16:
            o = layers.causal_attention(qkv, t, heads, scale)
        else:
            # exact-f32 parity path: the same arithmetic on torch ops
            if mask is None:
                mask = torch.full((t, t), float("-inf"), device=x.device).triu_(1)
            q, k, v = qkv.view(n, t, 3, heads, HEAD_DIM).permute(2, 0, 3, 1, 4)
            att = torch.softmax((q @ k.transpose(-1, -2)) * scale + mask, dim=-1)
            o = (att @ v).permute(0, 2, 1, 3).reshape(n * t, W).contiguous()
        x = hip.linear_fwd(o, L.w_out, bias=L.b_out, residual=x, out_f32=True)          # x + out_proj(o): residual in the epilogue
        y = hip.layernorm_fwd(x, L.ln2_w, L.ln2_b, dtype, eps)[0]
        h = act_(hip.linear_fwd(y, L.w_fc, bias=L.b_fc))                                # [n*t, 4W] in dtype
        x = hip.linear_fwd(h, L.w_proj, bias=L.b_proj, residual=x, out_f32=True)
    return x
