"""Chunk attention over a KV cache with the append (csrc/kernels/attn_extend.hip).

No autograd: generation runs under ``torch.no_grad()``.  ``lens`` and ``new_lens`` stay on the device; the
launch grid follows from the batch, the heads and the chunk length alone, so no call synchronises.
"""
from __future__ import annotations

import math

import torch

from . import _lib
from ._lib import F as CF, I, P
from ._native_attn_decode import _check_cache

_lib.register({
    "ddl_attn_extend": [P, P, P, P, P, P, I, I, I, I, I, CF, P],
})


def attention_extend(qkv_new, cache_k, cache_v, lens, num_heads, max_len, new_lens=None):
    B, T, H = qkv_new.shape[0], qkv_new.shape[1], num_heads
    _check_cache(cache_k, cache_v, B, H)
    C = cache_k.shape[2]
    for name, t in (("lens", lens), ("new_lens", new_lens)):
        if t is not None and (t.dtype != torch.int32 or t.shape != (B,) or not t.is_contiguous()):
            raise ValueError(f"{name} must be a contiguous int32 [B] tensor")
    qkv_new = qkv_new.contiguous()
    out = torch.empty(B, T, H * 64, dtype=qkv_new.dtype, device=qkv_new.device)
    _lib.call("ddl_attn_extend", qkv_new.data_ptr(), cache_k.data_ptr(), cache_v.data_ptr(), lens.data_ptr(),
              _lib.p(new_lens), out.data_ptr(), B, T, H, C, max_len, 1.0 / math.sqrt(64))
    return out
