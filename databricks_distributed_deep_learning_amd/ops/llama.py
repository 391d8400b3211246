"""The Llama family's memory-bound ops: RMSNorm, RoPE + grouped-query pack, SwiGLU.

``rms_norm``   ``y = x * rsqrt(mean(x^2) + eps) * w`` over the last axis (no mean subtraction, no bias).
``rope_qkv``   the fused projection ``[B, S, (H + 2 Hkv) D]`` (``[q heads | k heads | v heads]``) -> the packed
               ``[B, S, 3 H D]`` that ``ops.attention`` takes: q and k rotated by their position (HF's
               half-split convention), every k / v head repeated to its ``G = H / Hkv`` query heads.
``swiglu``     ``[gate | up]`` of one fused Linear -> ``silu(gate) * up``.

Each has a plain differentiable torch reference (CPU, fp32 / fp64, ``DDL_NATIVE=off``, shapes the
kernels do not cover); bf16 GPU tensors take the HIP kernels of ``csrc/kernels/llama.hip``.
"""
from __future__ import annotations

from typing import Optional

import torch
import torch.nn.functional as F

from . import _lib

_LOW = (torch.bfloat16, torch.float16)


def _compute_dtype(t: torch.Tensor) -> torch.dtype:
    return torch.float32 if t.dtype in _LOW else t.dtype


# ------------------------------------------------------------------ RMSNorm
def rms_norm_reference(x: torch.Tensor, weight: torch.Tensor, eps: float) -> torch.Tensor:
    ct = _compute_dtype(x)
    xf = x.to(ct)
    y = xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + eps) * weight.to(ct)
    return y.to(x.dtype)


def rms_norm(x: torch.Tensor, weight: torch.Tensor, eps: float, grad_from=None) -> torch.Tensor:
    """``grad_from``: a :class:`ops.bridge.GradBridge` holding the gradient of ``x`` from its other
    consumer (the block's residual branch); the backward adds it to this norm's input gradient in
    the same pass (``layer_norm``'s contract)."""
    if _lib.use_native(x, weight) and x.dtype == torch.bfloat16:
        from . import _native_llama
        if _native_llama.rms_norm_supported(x):
            return _native_llama.rms_norm(x, weight, eps, grad_from)
    from .bridge import join
    return rms_norm_reference(join(x, grad_from), weight, eps)


# ------------------------------------------------------------------ RoPE + GQA pack
def rope_table(n_positions: int, theta: float, head_dim: int = 64, device=None) -> torch.Tensor:
    """fp32 ``[n_positions, head_dim]``: row s is ``[cos(s f_i) | sin(s f_i)]``, ``i < head_dim / 2``,
    ``f_i = theta^(-2 i / head_dim)`` in fp32 and the angle their fp32 product, as HF computes them."""
    if head_dim % 2:
        raise ValueError("head_dim must be even")
    inv_freq = 1.0 / (theta ** (torch.arange(0, head_dim, 2, dtype=torch.int64).float() / head_dim))
    ang = torch.arange(n_positions, dtype=torch.int64).float()[:, None] * inv_freq[None, :]
    table = torch.cat([ang.cos(), ang.sin()], 1)
    return table if device is None else table.to(device)


def _rope_check(qkv, table, num_heads, num_kv_heads, positions=None):
    if qkv.dim() != 3:
        raise ValueError("rope_qkv takes the fused projection [B, S, (H + 2 Hkv) D]")
    if num_kv_heads < 1 or num_heads % num_kv_heads:
        raise ValueError(f"num_heads {num_heads} must be a multiple of num_kv_heads {num_kv_heads}")
    W = qkv.shape[2]
    if W % (num_heads + 2 * num_kv_heads):
        raise ValueError(f"width {W} is no multiple of num_heads + 2 num_kv_heads")
    D = W // (num_heads + 2 * num_kv_heads)
    if table.dim() != 2 or table.shape[1] != D:
        raise ValueError(f"table must be [n_positions, {D}], got {tuple(table.shape)}")
    if positions is None:
        if qkv.shape[1] > table.shape[0]:
            raise ValueError(f"sequence length {qkv.shape[1]} exceeds the rotary table's {table.shape[0]} positions")
    elif positions.dtype != torch.int32 or positions.shape != qkv.shape[:2]:
        raise ValueError(f"positions must be int32 {tuple(qkv.shape[:2])}, got {positions.dtype} "
                         f"{tuple(positions.shape)}")
    return D


def rope_qkv_reference(qkv: torch.Tensor, table: torch.Tensor, num_heads: int, num_kv_heads: int,
                       positions: Optional[torch.Tensor] = None) -> torch.Tensor:
    D = _rope_check(qkv, table, num_heads, num_kv_heads, positions)
    B, S, _ = qkv.shape
    H, Hkv, half = num_heads, num_kv_heads, D // 2
    ct = _compute_dtype(qkv)
    x = qkv.to(ct).view(B, S, H + 2 * Hkv, D)
    if positions is None:
        cos = table[:S, :half].to(ct).view(1, S, 1, half)
        sin = table[:S, half:].to(ct).view(1, S, 1, half)
    else:
        if B * S and not (0 <= int(positions.min()) and int(positions.max()) < table.shape[0]):
            raise ValueError(f"positions must lie in [0, {table.shape[0]}), the rotary table's rows")
        row = table[positions.long()].to(ct)                    # [B, S, D]
        cos, sin = row[:, :, None, :half], row[:, :, None, half:]

    def rot(t):
        a, b = t[..., :half], t[..., half:]
        return torch.cat([a * cos - b * sin, b * cos + a * sin], -1)

    q = rot(x[:, :, :H])
    k = rot(x[:, :, H:H + Hkv]).repeat_interleave(H // Hkv, 2)
    v = x[:, :, H + Hkv:].repeat_interleave(H // Hkv, 2)
    return torch.stack([q, k, v], 2).reshape(B, S, 3 * H * D).to(qkv.dtype)


def rope_qkv(qkv: torch.Tensor, table: torch.Tensor, num_heads: int, num_kv_heads: int,
             positions: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``positions`` (int32 ``[B, S]``, packed rows): token (b, s) is rotated by table row
    ``positions[b, s]`` in place of row s, forward and backward.  A value outside the table is a
    ``ValueError`` on the reference path; on the native path it is the caller's contract
    (``ops.doc_bounds`` checks ``position_ids`` once per batch: a valid one never passes s)."""
    D = _rope_check(qkv, table, num_heads, num_kv_heads, positions)
    if _lib.use_native(qkv, table, positions) and qkv.dtype == torch.bfloat16 and table.dtype == torch.float32:
        from . import _native_llama
        if _native_llama.rope_qkv_supported(num_heads, num_kv_heads, D):
            return _native_llama.rope_qkv(qkv, table, num_heads, num_kv_heads, positions)
    return rope_qkv_reference(qkv, table, num_heads, num_kv_heads, positions)


# ------------------------------------------------------------------ SwiGLU
def swiglu_reference(gu: torch.Tensor) -> torch.Tensor:
    if gu.shape[-1] % 2:
        raise ValueError("swiglu takes [gate | up]: an even last dimension")
    ct = _compute_dtype(gu)
    g, u = gu.to(ct).chunk(2, -1)
    return (F.silu(g) * u).to(gu.dtype)


def swiglu(gu: torch.Tensor) -> torch.Tensor:
    if gu.shape[-1] % 2:
        raise ValueError("swiglu takes [gate | up]: an even last dimension")
    if _lib.use_native(gu) and gu.dtype == torch.bfloat16:
        from . import _native_llama
        if _native_llama.swiglu_supported(gu):
            return _native_llama.swiglu(gu)
    return swiglu_reference(gu)
