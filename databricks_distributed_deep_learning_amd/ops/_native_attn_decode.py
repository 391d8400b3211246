"""Single-query attention over a KV cache and the cache fill (csrc/kernels/attn_decode.hip).

No autograd: generation runs under ``torch.no_grad()``.  ``lens`` stays on the device; the launch
grid follows from ``max_len`` (the host's bound on ``lens + 1``) alone, so no call synchronises.
"""
from __future__ import annotations

import math

import torch

from . import _lib
from ._lib import F as CF, I, L, P

_lib.register({
    "ddl_attn_decode_nsplit": [I, I, I],
    "ddl_attn_decode_chunk": [I, I, I],
    "ddl_attn_decode_ws": [I, I, I],
    "ddl_attn_decode": [P, P, P, P, P, P, I, I, I, I, CF, P],
    "ddl_kv_cache_fill": [P, P, P, I, I, I, I, P],
})


def plan(B: int, H: int, max_len: int):
    """(nsplit, chunk): the key splits of the launch and the positions each covers."""
    return _lib.fn("ddl_attn_decode_nsplit")(B, H, max_len), _lib.fn("ddl_attn_decode_chunk")(B, H, max_len)


def _check_cache(cache_k, cache_v, B, H):
    if cache_k.shape != cache_v.shape or cache_k.dim() != 4 or cache_k.shape[0] != B or cache_k.shape[1] != H \
            or cache_k.shape[3] != 64:
        raise ValueError(f"cache must be [B={B}, H={H}, C, 64] for keys and values, got {tuple(cache_k.shape)} / "
                         f"{tuple(cache_v.shape)}")
    if not (cache_k.is_contiguous() and cache_v.is_contiguous()):
        raise ValueError("cache tensors must be contiguous")


def attention_decode(qkv_new, cache_k, cache_v, lens, num_heads, max_len):
    B, H = qkv_new.shape[0], num_heads
    _check_cache(cache_k, cache_v, B, H)
    C = cache_k.shape[2]
    if lens.dtype != torch.int32 or lens.shape != (B,) or not lens.is_contiguous():
        raise ValueError("lens must be a contiguous int32 [B] tensor")
    qkv_new = qkv_new.contiguous()
    out = torch.empty(B, H * 64, dtype=qkv_new.dtype, device=qkv_new.device)
    wsf = _lib.fn("ddl_attn_decode_ws")
    wsf.restype = L
    n_ws = wsf(B, H, max_len)
    ws = torch.empty(n_ws, dtype=torch.float32, device=qkv_new.device) if n_ws else None
    _lib.call("ddl_attn_decode", qkv_new.data_ptr(), cache_k.data_ptr(), cache_v.data_ptr(), lens.data_ptr(),
              out.data_ptr(), _lib.p(ws), B, H, C, max_len, 1.0 / math.sqrt(64))
    return out


def kv_cache_fill(qkv, cache_k, cache_v, num_heads):
    B, S, _ = qkv.shape
    _check_cache(cache_k, cache_v, B, num_heads)
    qkv = qkv.contiguous()
    _lib.call("ddl_kv_cache_fill", qkv.data_ptr(), cache_k.data_ptr(), cache_v.data_ptr(), B, S, num_heads,
              cache_k.shape[2])
