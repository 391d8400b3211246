"""Grouped-query chunk attention over a rotated KV cache with the chunk's rotation and the append
(csrc/kernels/attn_extend_gqa.hip).

No autograd: generation runs under ``torch.no_grad()``.  ``lens`` and ``new_lens`` stay on the device; the
launch grid follows from the batch, the KV heads, the group size and the chunk length alone, so no call
synchronises.
"""
from __future__ import annotations

import math

import torch

from . import _lib
from ._lib import F as CF, I, L, P
from ._native_attn_decode_gqa import _check_cache

_lib.register({
    "ddl_attn_extend_gqa_supported": [I, I],
    "ddl_attn_extend_gqa_tile": [I, I, I],
    "ddl_attn_extend_gqa": [P, P, P, P, P, P, P, I, I, I, I, I, I, L, CF, P],
})


def supported(num_heads: int, num_kv_heads: int) -> bool:
    """The extend kernel has an instance for this group size (the decode kernel's set)."""
    return bool(_lib.fn("ddl_attn_extend_gqa_supported")(num_heads, num_kv_heads))


def tile(T: int, num_heads: int, num_kv_heads: int) -> int:
    """Queries per workgroup the launch uses for a chunk of ``T`` tokens (0 without an instance)."""
    return _lib.fn("ddl_attn_extend_gqa_tile")(T, num_heads, num_kv_heads)


def attention_extend_gqa(qkv_new, table, cache_k, cache_v, lens, num_heads, num_kv_heads, max_len, new_lens=None):
    B, T, H, Hkv = qkv_new.shape[0], qkv_new.shape[1], num_heads, num_kv_heads
    _check_cache(cache_k, cache_v, B, Hkv)
    C = cache_k.shape[2]
    for name, t in (("lens", lens), ("new_lens", new_lens)):
        if t is not None and (t.dtype != torch.int32 or t.shape != (B,) or not t.is_contiguous()):
            raise ValueError(f"{name} must be a contiguous int32 [B] tensor")
    qkv_new, table = qkv_new.contiguous(), table.contiguous()
    out = torch.empty(B, T, H * 64, dtype=qkv_new.dtype, device=qkv_new.device)
    _lib.call("ddl_attn_extend_gqa", qkv_new.data_ptr(), table.data_ptr(), cache_k.data_ptr(), cache_v.data_ptr(),
              lens.data_ptr(), _lib.p(new_lens), out.data_ptr(), B, T, H, Hkv, C, max_len, table.shape[0],
              1.0 / math.sqrt(64))
    return out
