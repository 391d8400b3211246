"""Grouped-query single-query attention over a rotated KV cache and its cache fill
(csrc/kernels/attn_decode_gqa.hip).

No autograd: generation runs under ``torch.no_grad()``.  ``lens`` stays on the device; the launch
grid follows from ``max_len`` (the host's bound on ``lens + 1``) alone, so no call synchronises.
"""
from __future__ import annotations

import math

import torch

from . import _lib
from ._lib import F as CF, I, L, P

_lib.register({
    "ddl_attn_decode_gqa_supported": [I, I],
    "ddl_attn_decode_gqa_nsplit": [I, I, I],
    "ddl_attn_decode_gqa_chunk": [I, I, I],
    "ddl_attn_decode_gqa_ws": [I, I, I, I],
    "ddl_attn_decode_gqa": [P, P, P, P, P, P, P, I, I, I, I, I, L, CF, P],
    "ddl_kv_cache_fill_gqa": [P, P, P, I, I, I, I, I, P],
})


def supported(num_heads: int, num_kv_heads: int) -> bool:
    """The decode kernel has an instance for this group size (G in 1, 2, 3, 4, 8)."""
    return bool(_lib.fn("ddl_attn_decode_gqa_supported")(num_heads, num_kv_heads))


def plan(B: int, Hkv: int, max_len: int):
    """(nsplit, chunk): the key splits of the launch and the positions each covers."""
    return (_lib.fn("ddl_attn_decode_gqa_nsplit")(B, Hkv, max_len),
            _lib.fn("ddl_attn_decode_gqa_chunk")(B, Hkv, max_len))


def _check_cache(cache_k, cache_v, B, Hkv):
    if cache_k.shape != cache_v.shape or cache_k.dim() != 4 or cache_k.shape[0] != B or cache_k.shape[1] != Hkv \
            or cache_k.shape[3] != 64:
        raise ValueError(f"cache must be [B={B}, Hkv={Hkv}, C, 64] for keys and values, got {tuple(cache_k.shape)} / "
                         f"{tuple(cache_v.shape)}")
    if not (cache_k.is_contiguous() and cache_v.is_contiguous()):
        raise ValueError("cache tensors must be contiguous")


def attention_decode_gqa(qkv_new, table, cache_k, cache_v, lens, num_heads, num_kv_heads, max_len):
    B, H, Hkv = qkv_new.shape[0], num_heads, num_kv_heads
    _check_cache(cache_k, cache_v, B, Hkv)
    C = cache_k.shape[2]
    if lens.dtype != torch.int32 or lens.shape != (B,) or not lens.is_contiguous():
        raise ValueError("lens must be a contiguous int32 [B] tensor")
    qkv_new, table = qkv_new.contiguous(), table.contiguous()
    out = torch.empty(B, H * 64, dtype=qkv_new.dtype, device=qkv_new.device)
    wsf = _lib.fn("ddl_attn_decode_gqa_ws")
    wsf.restype = L
    n_ws = wsf(B, H, Hkv, max_len)
    ws = torch.empty(n_ws, dtype=torch.float32, device=qkv_new.device) if n_ws else None
    _lib.call("ddl_attn_decode_gqa", qkv_new.data_ptr(), table.data_ptr(), cache_k.data_ptr(), cache_v.data_ptr(),
              lens.data_ptr(), out.data_ptr(), _lib.p(ws), B, H, Hkv, C, max_len, table.shape[0],
              1.0 / math.sqrt(64))
    return out


def kv_cache_fill_gqa(packed, cache_k, cache_v, num_heads, num_kv_heads):
    B, S, _ = packed.shape
    _check_cache(cache_k, cache_v, B, num_kv_heads)
    packed = packed.contiguous()
    _lib.call("ddl_kv_cache_fill_gqa", packed.data_ptr(), cache_k.data_ptr(), cache_v.data_ptr(), B, S, num_heads,
              num_kv_heads, cache_k.shape[2])
