"""GPT-2 small / medium / large causal language model (pre-LN decoder, tied head).

Parameter-for-parameter equivalent to HF ``GPT2LMHeadModel`` (124,439,808 parameters for small).  The
blocks are ``ViTLayer``'s wiring -- fused QKV, residual adds in the output GEMMs' epilogues, the
residual-stream gradient bridged into the LayerNorm backwards -- with causal attention
(``ops.attention(..., causal=True)``: the tiled kernels' CAUSAL instances, which skip the tiles
above the diagonal).  The head is the token embedding (tied, no bias) and, with labels, the fused
vocabulary head + loss (``ops.linear_cross_entropy``): the ``[B S, vocab]`` logits exist once.

Labels are NOT shifted here: ``labels[b, s]`` is the token at ``s + 1`` (-100 at the last position
and wherever ``s + 1`` is padding), as ``data.SyntheticTokens(causal_lm=True)`` builds them.

``activation_function="gelu"`` (default) is the exact erf GELU the fused GELU / dGELU GEMM epilogues
compute; ``"gelu_new"`` (HF's tanh form, what the released checkpoints were trained with) runs
unfused: fc1 without activation, ``F.gelu(approximate="tanh")``, fc2.

What stays on ATen in a training step: the position-embedding add (``wte(ids) + wpe[:S]``: one
broadcast add forward, one batch sum + slice backward) and, with ``attention_mask``, the
``(1 - mask) * -10000`` key bias; with ``"gelu_new"`` the tanh GELU and its backward.
"""
from __future__ import annotations

from dataclasses import dataclass

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import ops
from ..ops.bridge import GradBridge
from .layers import Dropout, Embedding, LayerNorm, Linear


@dataclass
class GPT2Config:
    vocab_size: int = 50257
    n_positions: int = 1024
    n_embd: int = 768
    n_layer: int = 12
    n_head: int = 12
    layer_norm_epsilon: float = 1e-5
    resid_pdrop: float = 0.1
    embd_pdrop: float = 0.1
    attn_pdrop: float = 0.1
    initializer_range: float = 0.02
    activation_function: str = "gelu"       # "gelu" (erf, fused) | "gelu_new" (tanh, unfused)


class GPT2Block(nn.Module):
    def __init__(self, c: GPT2Config):
        super().__init__()
        H, std = c.n_embd, c.initializer_range
        if c.activation_function not in ("gelu", "gelu_new"):
            raise ValueError(f"activation_function {c.activation_function!r}: 'gelu' or 'gelu_new'")
        self.num_heads = c.n_head
        self.attn_dropout = c.attn_pdrop
        self.tanh_gelu = c.activation_function == "gelu_new"
        self.ln_1 = LayerNorm(H, c.layer_norm_epsilon)
        self.qkv = Linear(H, 3 * H, init_std=std)
        self.attn_out = Linear(H, H, init_std=std)
        self.ln_2 = LayerNorm(H, c.layer_norm_epsilon)
        self.fc1 = Linear(H, 4 * H, act=None if self.tanh_gelu else "gelu", init_std=std)
        self.fc2 = Linear(4 * H, H, init_std=std)
        self.dropout = Dropout(c.resid_pdrop)
        for lin in (self.qkv, self.attn_out, self.fc1, self.fc2):
            nn.init.zeros_(lin.bias)

    def _mlp(self, y, **kw):
        if self.tanh_gelu:
            return self.fc2(F.gelu(self.fc1(y), approximate="tanh"), **kw)
        return self.fc2(self.fc1(y), fuse_dgelu=True, **kw)

    def forward(self, h, mask=None):
        bridged = torch.is_grad_enabled() and h.requires_grad
        b1 = GradBridge() if bridged else None
        y = self.ln_1(h, grad_from=b1)
        ctx = ops.attention(self.qkv(y), self.num_heads, mask, self.attn_dropout, self.training, causal=True)
        if self.dropout.p > 0.0 and self.training:
            h = h + self.dropout(self.attn_out(ctx))
            return h + self.dropout(self._mlp(self.ln_2(h)))
        # no residual dropout: both residual adds ride the output GEMMs' epilogues and the residual
        # stream's gradient reaches each LayerNorm backward through a bridge (as in ViTLayer)
        h = self.attn_out(ctx, residual=h, residual_grad_to=b1)
        b2 = GradBridge() if bridged else None
        y = self.ln_2(h, grad_from=b2)
        return self._mlp(y, residual=h, residual_grad_to=b2)


class GPT2LMHeadModel(nn.Module):
    def __init__(self, c: GPT2Config):
        super().__init__()
        if c.n_embd % c.n_head:
            raise ValueError("n_embd must be a multiple of n_head")
        self.config = c
        self.wte = Embedding(c.vocab_size, c.n_embd, c.initializer_range)
        self.wpe = Embedding(c.n_positions, c.n_embd, c.initializer_range)
        self.drop = Dropout(c.embd_pdrop)
        self.h = nn.ModuleList([GPT2Block(c) for _ in range(c.n_layer)])
        self.ln_f = LayerNorm(c.n_embd, c.layer_norm_epsilon)
        # HF scales the residual projections' init by 1 / sqrt(2 n_layer)
        for blk in self.h:
            for lin in (blk.attn_out, blk.fc2):
                nn.init.normal_(lin.weight, 0.0, c.initializer_range / (2 * c.n_layer) ** 0.5)

    # ZeRO-1 gather waits (parallel/ddp.py): the root's forward reads both tables directly
    _ddl_direct_reads = ("wte", "wpe")

    def forward(self, input_ids, attention_mask=None, token_type_ids=None, labels=None):
        """``token_type_ids`` is ignored (GPT-2 has none): it keeps the training loop's
        ``(input_ids, attention_mask, token_type_ids, labels)`` call form.
        Returns ``(loss, None)`` with labels -- the fused head never hands out the logits -- and the
        ``[B, S, vocab]`` logits without."""
        B, S = input_ids.shape
        if S > self.config.n_positions:
            raise ValueError(f"sequence length {S} exceeds n_positions {self.config.n_positions}")
        mask_bias = None
        if attention_mask is not None:
            mask_bias = (1.0 - attention_mask.float()) * -10000.0
        h = self.drop(self.wte(input_ids) + self.wpe.weight[:S].unsqueeze(0))
        for blk in self.h:
            h = blk(h, mask_bias)
        h = self.ln_f(h)
        if labels is not None:
            loss = ops.linear_cross_entropy(h.reshape(-1, h.shape[-1]), self.wte.weight, None, labels.reshape(-1),
                                            -100, defer_weight_ready=True)
            return loss, None
        return ops.linear(h, self.wte.weight, None)


def _make(dropout: float, activation_function: str, **kw) -> GPT2LMHeadModel:
    return GPT2LMHeadModel(GPT2Config(resid_pdrop=dropout, embd_pdrop=dropout, attn_pdrop=dropout,
                                      activation_function=activation_function, **kw))


def gpt2(dropout: float = 0.1, activation_function: str = "gelu", **kw) -> GPT2LMHeadModel:
    return _make(dropout, activation_function, **kw)


def gpt2_medium(dropout: float = 0.1, activation_function: str = "gelu", **kw) -> GPT2LMHeadModel:
    d = dict(n_embd=1024, n_layer=24, n_head=16)
    d.update(kw)
    return _make(dropout, activation_function, **d)


def gpt2_large(dropout: float = 0.1, activation_function: str = "gelu", **kw) -> GPT2LMHeadModel:
    d = dict(n_embd=1280, n_layer=36, n_head=20)
    d.update(kw)
    return _make(dropout, activation_function, **d)


def gpt2_tiny(dropout: float = 0.1, activation_function: str = "gelu", **kw) -> GPT2LMHeadModel:
    """2 layers, hidden 128, 2 heads (head dim 64), vocabulary 1000: the GPT-2 code path at test size."""
    d = dict(n_embd=128, n_layer=2, n_head=2, vocab_size=1000, n_positions=128)
    d.update(kw)
    return _make(dropout, activation_function, **d)


# ------------------------------------------------------------ HF conversion
# HF GPT-2 linears are ``Conv1D``: weight [in, out] (ours: [out, in]); ``c_attn`` is the fused QKV
# in our [q | k | v] order; ``lm_head.weight`` is the tied ``wte``; ``attn.bias`` /
# ``attn.masked_bias`` are HF's causal-mask buffers.
_HF_LINEAR = {"attn.c_attn": "qkv", "attn.c_proj": "attn_out", "mlp.c_fc": "fc1", "mlp.c_proj": "fc2"}
_HF_NORM = {"ln_1": "ln_1", "ln_2": "ln_2"}


def from_hf_state_dict(sd: dict, num_layers: int) -> dict:
    """HF ``GPT2LMHeadModel`` state dict -> this model's."""
    out = {"wte.weight": sd["transformer.wte.weight"], "wpe.weight": sd["transformer.wpe.weight"],
           "ln_f.weight": sd["transformer.ln_f.weight"], "ln_f.bias": sd["transformer.ln_f.bias"]}
    if "lm_head.weight" in sd and not torch.equal(sd["lm_head.weight"], sd["transformer.wte.weight"]):
        raise ValueError("lm_head.weight is not tied to transformer.wte.weight: this model shares the two")
    for i in range(num_layers):
        p = f"transformer.h.{i}."
        for hf, ours in _HF_LINEAR.items():
            out[f"h.{i}.{ours}.weight"] = sd[p + hf + ".weight"].t().contiguous()
            out[f"h.{i}.{ours}.bias"] = sd[p + hf + ".bias"]
        for hf, ours in _HF_NORM.items():
            for t in ("weight", "bias"):
                out[f"h.{i}.{ours}.{t}"] = sd[p + f"{hf}.{t}"]
    return out


def to_hf_state_dict(sd: dict, num_layers: int) -> dict:
    out = {"transformer.wte.weight": sd["wte.weight"], "transformer.wpe.weight": sd["wpe.weight"],
           "transformer.ln_f.weight": sd["ln_f.weight"], "transformer.ln_f.bias": sd["ln_f.bias"],
           "lm_head.weight": sd["wte.weight"]}
    for i in range(num_layers):
        p = f"transformer.h.{i}."
        for hf, ours in _HF_LINEAR.items():
            out[p + hf + ".weight"] = sd[f"h.{i}.{ours}.weight"].t().contiguous()
            out[p + hf + ".bias"] = sd[f"h.{i}.{ours}.bias"]
        for hf, ours in _HF_NORM.items():
            for t in ("weight", "bias"):
                out[p + f"{hf}.{t}"] = sd[f"h.{i}.{ours}.{t}"]
    return out
