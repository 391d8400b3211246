"""Attention over a KV cache with the append -- one new token (csrc/kernels/attn_decode.hip) or a chunk of them
(csrc/kernels/attn_extend.hip) -- and the cache fill after a prefill; for GPT-2's packed projection and, with a
rotary ``table``, for the Llama family's grouped-query cache of rotated keys.

No autograd: generation runs under ``torch.no_grad()``.  ``lens`` and ``new_lens`` stay on the device; the launch
grids follow from the shapes and from ``max_len`` (the host's bound on ``lens``) alone, so no call synchronises.
"""
from __future__ import annotations

import math

import torch

from . import _lib
from ._lib import F as CF, I, L, P
from .attention import _check_lens

_lib.register({
    "ddl_attn_decode_nsplit": [I, I, I],
    "ddl_attn_decode_chunk": [I, I, I],
    "ddl_attn_decode_ws": [I, I, I],
    "ddl_attn_decode": [P, P, P, P, P, P, I, I, I, I, CF, P],
    "ddl_kv_cache_fill": [P, P, P, I, I, I, I, P],
    "ddl_attn_extend": [P, P, P, P, P, P, I, I, I, I, I, CF, P],
    "ddl_attn_decode_gqa_supported": [I, I],
    "ddl_attn_decode_gqa_nsplit": [I, I, I],
    "ddl_attn_decode_gqa_chunk": [I, I, I],
    "ddl_attn_decode_gqa_ws": [I, I, I, I],
    "ddl_attn_decode_gqa": [P, P, P, P, P, P, P, I, I, I, I, I, L, CF, P],
    "ddl_kv_cache_fill_gqa": [P, P, P, I, I, I, I, I, P],
    "ddl_attn_extend_gqa_supported": [I, I],
    "ddl_attn_extend_gqa_tile": [I, I, I],
    "ddl_attn_extend_gqa": [P, P, P, P, P, P, P, I, I, I, I, I, I, L, CF, P],
})

_SCALE = 1.0 / math.sqrt(64)


def plan(B: int, H: int, max_len: int):
    """(nsplit, chunk) of ``attention_decode``: the key splits of the launch and the positions each covers."""
    return _lib.fn("ddl_attn_decode_nsplit")(B, H, max_len), _lib.fn("ddl_attn_decode_chunk")(B, H, max_len)


def plan_gqa(B: int, Hkv: int, max_len: int):
    """(nsplit, chunk) of ``attention_decode_gqa``."""
    return (_lib.fn("ddl_attn_decode_gqa_nsplit")(B, Hkv, max_len),
            _lib.fn("ddl_attn_decode_gqa_chunk")(B, Hkv, max_len))


def supported(num_heads: int, num_kv_heads: int) -> bool:
    """The rotary kernels have an instance for this group size (G in 1, 2, 3, 4, 8).  Decode and extend are built
    for the same set and ``ops.attention`` routes a model's cache through both, so one answer serves both: a group
    size either kernel lacks takes the reference for the whole cache, never for one of the two paths alone."""
    return bool(_lib.fn("ddl_attn_decode_gqa_supported")(num_heads, num_kv_heads)
                and _lib.fn("ddl_attn_extend_gqa_supported")(num_heads, num_kv_heads))


def tile(T: int, num_heads: int, num_kv_heads: int) -> int:
    """Queries per workgroup ``attention_extend_gqa`` uses for a chunk of ``T`` tokens (0 without an instance)."""
    return _lib.fn("ddl_attn_extend_gqa_tile")(T, num_heads, num_kv_heads)


def _check_cache(cache_k, cache_v, B, heads, name="H"):
    if cache_k.shape != cache_v.shape or cache_k.dim() != 4 or cache_k.shape[0] != B or cache_k.shape[1] != heads \
            or cache_k.shape[3] != 64:
        raise ValueError(f"cache must be [B={B}, {name}={heads}, C, 64] for keys and values, got "
                         f"{tuple(cache_k.shape)} / {tuple(cache_v.shape)}")
    if not (cache_k.is_contiguous() and cache_v.is_contiguous()):
        raise ValueError("cache tensors must be contiguous")


def _workspace(ws_fn: str, dev, *args):
    """The fp32 partials buffer of a split decode launch (None with one split)."""
    f = _lib.fn(ws_fn)
    f.restype = L
    n = f(*args)
    return torch.empty(n, dtype=torch.float32, device=dev) if n else None


def attention_decode(qkv_new, cache_k, cache_v, lens, num_heads, max_len):
    B, H = qkv_new.shape[0], num_heads
    _check_cache(cache_k, cache_v, B, H)
    _check_lens(B, lens)
    qkv_new = qkv_new.contiguous()
    out = torch.empty(B, H * 64, dtype=qkv_new.dtype, device=qkv_new.device)
    ws = _workspace("ddl_attn_decode_ws", qkv_new.device, B, H, max_len)
    _lib.call("ddl_attn_decode", qkv_new.data_ptr(), cache_k.data_ptr(), cache_v.data_ptr(), lens.data_ptr(),
              out.data_ptr(), _lib.p(ws), B, H, cache_k.shape[2], max_len, _SCALE)
    return out


def attention_decode_gqa(qkv_new, table, cache_k, cache_v, lens, num_heads, num_kv_heads, max_len):
    B, H, Hkv = qkv_new.shape[0], num_heads, num_kv_heads
    _check_cache(cache_k, cache_v, B, Hkv, "Hkv")
    _check_lens(B, lens)
    qkv_new, table = qkv_new.contiguous(), table.contiguous()
    out = torch.empty(B, H * 64, dtype=qkv_new.dtype, device=qkv_new.device)
    ws = _workspace("ddl_attn_decode_gqa_ws", qkv_new.device, B, H, Hkv, max_len)
    _lib.call("ddl_attn_decode_gqa", qkv_new.data_ptr(), table.data_ptr(), cache_k.data_ptr(), cache_v.data_ptr(),
              lens.data_ptr(), out.data_ptr(), _lib.p(ws), B, H, Hkv, cache_k.shape[2], max_len, table.shape[0],
              _SCALE)
    return out


def attention_extend(qkv_new, cache_k, cache_v, lens, num_heads, max_len, new_lens=None):
    B, T, H = qkv_new.shape[0], qkv_new.shape[1], num_heads
    _check_cache(cache_k, cache_v, B, H)
    _check_lens(B, lens, new_lens)
    qkv_new = qkv_new.contiguous()
    out = torch.empty(B, T, H * 64, dtype=qkv_new.dtype, device=qkv_new.device)
    _lib.call("ddl_attn_extend", qkv_new.data_ptr(), cache_k.data_ptr(), cache_v.data_ptr(), lens.data_ptr(),
              _lib.p(new_lens), out.data_ptr(), B, T, H, cache_k.shape[2], max_len, _SCALE)
    return out


def attention_extend_gqa(qkv_new, table, cache_k, cache_v, lens, num_heads, num_kv_heads, max_len, new_lens=None):
    B, T, H, Hkv = qkv_new.shape[0], qkv_new.shape[1], num_heads, num_kv_heads
    _check_cache(cache_k, cache_v, B, Hkv, "Hkv")
    _check_lens(B, lens, new_lens)
    qkv_new, table = qkv_new.contiguous(), table.contiguous()
    out = torch.empty(B, T, H * 64, dtype=qkv_new.dtype, device=qkv_new.device)
    _lib.call("ddl_attn_extend_gqa", qkv_new.data_ptr(), table.data_ptr(), cache_k.data_ptr(), cache_v.data_ptr(),
              lens.data_ptr(), _lib.p(new_lens), out.data_ptr(), B, T, H, Hkv, cache_k.shape[2], max_len,
              table.shape[0], _SCALE)
    return out


def kv_cache_fill(qkv, cache_k, cache_v, num_heads):
    B, S, _ = qkv.shape
    _check_cache(cache_k, cache_v, B, num_heads)
    qkv = qkv.contiguous()
    _lib.call("ddl_kv_cache_fill", qkv.data_ptr(), cache_k.data_ptr(), cache_v.data_ptr(), B, S, num_heads,
              cache_k.shape[2])


def kv_cache_fill_gqa(packed, cache_k, cache_v, num_heads, num_kv_heads):
    B, S, _ = packed.shape
    _check_cache(cache_k, cache_v, B, num_kv_heads, "Hkv")
    packed = packed.contiguous()
    _lib.call("ddl_kv_cache_fill_gqa", packed.data_ptr(), cache_k.data_ptr(), cache_v.data_ptr(), B, S, num_heads,
              num_kv_heads, cache_k.shape[2])
