"""Attention over a KV cache with the append -- one new token (csrc/kernels/attn_decode.hip) or a chunk of them
(csrc/kernels/attn_extend.hip) -- and the cache fill after a prefill; for GPT-2's packed projection and, with a
rotary ``table``, for the Llama family's grouped-query cache of rotated keys.

Head dimension 64 throughout, except the rotary kernels, which also have head-dim-128 instances (Llama-2-7B,
Llama-3-8B, Mistral-7B): decode and the cache fill in csrc/kernels/attn_decode_d128.hip, extend in
csrc/kernels/attn_extend_d128.hip.  ``attention_decode_gqa``, ``attention_extend_gqa`` and ``kv_cache_fill_gqa``
read D from the cache; GPT-2's non-rotary ops are D = 64 only (no GPT-2 has another head size), and there are
no other head dimensions.

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
    "ddl_attn_decode_gqa_supported_hd": [I, I, I],
    "ddl_attn_decode_gqa_ws_hd": [I, I, I, I, I],
    "ddl_attn_decode_gqa_d128": [P, P, P, P, P, P, P, I, I, I, I, I, L, CF, P],
    "ddl_kv_cache_fill_gqa_d128": [P, P, P, I, I, I, I, I, P],
    "ddl_attn_extend_gqa_d128_supported": [I, I],
    "ddl_attn_extend_gqa_d128_tile": [I, I, I],
    "ddl_attn_extend_gqa_d128": [P, P, P, P, P, P, P, I, I, I, I, I, I, L, CF, P],
    "ddl_attn_extend_gqa_d128_nsplit": [I, I, I, I, I],
    "ddl_attn_extend_gqa_d128_ws": [I, I, I, I],
    "ddl_attn_extend_gqa_d128_split": [P, P, P, P, P, P, P, P, I, I, I, I, I, I, I, L, CF, P],
    "ddl_attn_decode_gqa_d128_fp8_supported": [I, I, I],
    "ddl_attn_decode_gqa_d128_fp8": [P, P, P, P, P, P, P, P, P, I, I, I, I, I, L, CF, P],
    "ddl_kv_cache_fill_gqa_d128_fp8": [P, P, P, P, P, I, I, I, I, I, P],
    "ddl_attn_extend_gqa_d128_fp8_supported": [I, I],
    "ddl_attn_extend_gqa_d128_fp8": [P, P, P, P, P, P, P, P, P, I, I, I, I, I, I, L, CF, P],
})

_SCALE = 1.0 / math.sqrt(64)
DECODE_HEAD_DIMS = (64, 128)        # of attention_decode_gqa, attention_extend_gqa and kv_cache_fill_gqa


def plan(B: int, H: int, max_len: int):
    """(nsplit, chunk) of ``attention_decode``: the key splits of the launch and the positions each covers."""
    return _lib.fn("ddl_attn_decode_nsplit")(B, H, max_len), _lib.fn("ddl_attn_decode_chunk")(B, H, max_len)


def plan_gqa(B: int, Hkv: int, max_len: int):
    """(nsplit, chunk) of ``attention_decode_gqa``, at either head dimension: the plan follows from B, Hkv and
    ``max_len`` alone (a chunk is a multiple of 32 positions: of the 32 key groups of a D = 64 workgroup and of
    the 16 of a D = 128 one)."""
    return (_lib.fn("ddl_attn_decode_gqa_nsplit")(B, Hkv, max_len),
            _lib.fn("ddl_attn_decode_gqa_chunk")(B, Hkv, max_len))


def plan_extend(B: int, T: int, num_heads: int, num_kv_heads: int, max_len: int, head_dim: int = 128) -> int:
    """Key splits ``attention_extend_gqa`` uses by default: from the shapes and ``max_len`` alone, like
    ``plan_gqa``.  1 is the one launch: at head dim 64 (no split there), without an instance for the group size,
    and for every ``max_len`` below 448.  More than 1 when the one launch's ``ceil(T / tile) Hkv B`` workgroups
    are fewer than two per CU over a long cache: each split walks ``ceil(max_len / nsplit)`` keys rounded up to 32."""
    if head_dim != 128:
        return 1
    return _lib.fn("ddl_attn_extend_gqa_d128_nsplit")(B, T, num_heads, num_kv_heads, max_len)


def supported(num_heads: int, num_kv_heads: int, head_dim: int = 64) -> bool:
    """The D = 64 pair of rotary kernels has an instance for this group size (G in 1, 2, 3, 4, 8).  Decode and
    extend are built for the same set and ``ops.attention`` routes a model's cache through both, so at head dim 64
    one answer serves both: a group size either kernel lacks takes the reference for the whole cache, never for
    one of the two paths alone.  This is about that pair only: at any other ``head_dim`` the answer is False.  The
    head-dim-128 kernels are separate files and answer for themselves: ask ``supported_decode`` and
    ``supported_extend``."""
    return bool(head_dim == 64 and _lib.fn("ddl_attn_decode_gqa_supported")(num_heads, num_kv_heads)
                and _lib.fn("ddl_attn_extend_gqa_supported")(num_heads, num_kv_heads))


def supported_decode(num_heads: int, num_kv_heads: int, head_dim: int = 64) -> bool:
    """What ``attention_decode_gqa`` takes natively.  Head dim 64: ``supported``'s answer (decode never goes
    native without extend).  Head dim 128: the decode kernel's own.  A cache may be appended to by a native kernel
    and by a reference (another dtype, a prefill), which is sound: all append keys rotated in fp32 and rounded
    once to bf16 and bit-copied values, and all read the same ``[B, Hkv, C, D]`` layout of rotated keys, so any
    continues a cache another wrote.  A kernel may contract ``a c - b s`` into an FMA where torch rounds the two
    products, so an appended key element can differ by one bf16 ulp between a kernel and a reference."""
    if head_dim == 64:
        return supported(num_heads, num_kv_heads)
    return bool(_lib.fn("ddl_attn_decode_gqa_supported_hd")(num_heads, num_kv_heads, head_dim))


def supported_extend(num_heads: int, num_kv_heads: int, head_dim: int = 64) -> bool:
    """What ``attention_extend_gqa`` takes natively.  Head dim 64: ``supported``'s answer.  Head dim 128: the
    head-dim-128 extend kernel's own."""
    if head_dim == 64:
        return supported(num_heads, num_kv_heads)
    return bool(head_dim == 128 and _lib.fn("ddl_attn_extend_gqa_d128_supported")(num_heads, num_kv_heads))


def supported_decode_fp8(num_heads: int, num_kv_heads: int, head_dim: int = 128) -> bool:
    """What ``attention_decode_gqa_fp8`` and ``kv_cache_fill_gqa_fp8`` take natively: head dim 128 and the bf16
    kernel's group sizes (csrc/kernels/attn_decode_d128_fp8.hip)."""
    return bool(_lib.fn("ddl_attn_decode_gqa_d128_fp8_supported")(num_heads, num_kv_heads, head_dim))


def supported_extend_fp8(num_heads: int, num_kv_heads: int, head_dim: int = 128) -> bool:
    """What ``attention_extend_gqa_fp8`` takes natively: head dim 128 and the bf16 kernel's group sizes
    (csrc/kernels/attn_extend_d128_fp8.hip).  Its query tile is the bf16 kernel's: ``tile(..., head_dim=128)``
    answers for both; its cache tile is 64 keys."""
    return bool(head_dim == 128 and _lib.fn("ddl_attn_extend_gqa_d128_fp8_supported")(num_heads, num_kv_heads))


def tile(T: int, num_heads: int, num_kv_heads: int, head_dim: int = 64) -> int:
    """Queries per workgroup ``attention_extend_gqa`` uses for a chunk of ``T`` tokens (0 without an instance)."""
    if head_dim not in DECODE_HEAD_DIMS:
        return 0
    return _lib.fn("ddl_attn_extend_gqa_tile" if head_dim == 64 else "ddl_attn_extend_gqa_d128_tile")(
        T, num_heads, num_kv_heads)


def _check_cache(cache_k, cache_v, B, heads, name="H", dims=(64,)):
    """-> the head dimension, one of ``dims``."""
    if cache_k.shape != cache_v.shape or cache_k.dim() != 4 or cache_k.shape[0] != B or cache_k.shape[1] != heads \
            or cache_k.shape[3] not in dims:
        raise ValueError(f"cache must be [B={B}, {name}={heads}, C, {' or '.join(map(str, dims))}] for keys and "
                         f"values, got {tuple(cache_k.shape)} / {tuple(cache_v.shape)}")
    if not (cache_k.is_contiguous() and cache_v.is_contiguous()):
        raise ValueError("cache tensors must be contiguous")
    return cache_k.shape[3]


def _workspace(ws_fn: str, dev, *args):
    """The fp32 partials buffer of a split launch (None with one split)."""
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
    D = _check_cache(cache_k, cache_v, B, Hkv, "Hkv", DECODE_HEAD_DIMS)
    if qkv_new.shape[1] != (H + 2 * Hkv) * D or table.shape[1] != D:
        raise ValueError(f"qkv_new must be [B, (H + 2 Hkv) {D}] and table [n_positions, {D}], got "
                         f"{tuple(qkv_new.shape)} / {tuple(table.shape)}")
    _check_lens(B, lens)
    qkv_new, table = qkv_new.contiguous(), table.contiguous()
    out = torch.empty(B, H * D, dtype=qkv_new.dtype, device=qkv_new.device)
    ws = _workspace("ddl_attn_decode_gqa_ws_hd", qkv_new.device, B, H, Hkv, max_len, D)
    _lib.call("ddl_attn_decode_gqa" if D == 64 else "ddl_attn_decode_gqa_d128", qkv_new.data_ptr(), table.data_ptr(),
              cache_k.data_ptr(), cache_v.data_ptr(), lens.data_ptr(), out.data_ptr(), _lib.p(ws), B, H, Hkv,
              cache_k.shape[2], max_len, table.shape[0], 1.0 / math.sqrt(D))
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


def attention_extend_gqa(qkv_new, table, cache_k, cache_v, lens, num_heads, num_kv_heads, max_len, new_lens=None,
                         key_splits=None):
    """``key_splits``: None for ``plan_extend``'s answer, 1 for the one launch, n >= 2 for that many key splits and
    the merge launch (head dim 128 only; head dim 64 has the one launch)."""
    B, T, H, Hkv = qkv_new.shape[0], qkv_new.shape[1], num_heads, num_kv_heads
    D = _check_cache(cache_k, cache_v, B, Hkv, "Hkv", DECODE_HEAD_DIMS)
    if qkv_new.shape[2] != (H + 2 * Hkv) * D or table.shape[1] != D:
        raise ValueError(f"qkv_new must be [B, T, (H + 2 Hkv) {D}] and table [n_positions, {D}], got "
                         f"{tuple(qkv_new.shape)} / {tuple(table.shape)}")
    _check_lens(B, lens, new_lens)
    qkv_new, table = qkv_new.contiguous(), table.contiguous()
    out = torch.empty(B, T, H * D, dtype=qkv_new.dtype, device=qkv_new.device)
    nsplit = 1 if D == 64 else (plan_extend(B, T, H, Hkv, max_len) if key_splits is None else key_splits)
    if nsplit > 1:
        ws = _workspace("ddl_attn_extend_gqa_d128_ws", qkv_new.device, B, T, H, nsplit)
        _lib.call("ddl_attn_extend_gqa_d128_split", qkv_new.data_ptr(), table.data_ptr(), cache_k.data_ptr(),
                  cache_v.data_ptr(), lens.data_ptr(), _lib.p(new_lens), out.data_ptr(), _lib.p(ws), nsplit, B, T, H,
                  Hkv, cache_k.shape[2], max_len, table.shape[0], 1.0 / math.sqrt(D))
        return out
    _lib.call("ddl_attn_extend_gqa" if D == 64 else "ddl_attn_extend_gqa_d128", qkv_new.data_ptr(), table.data_ptr(),
              cache_k.data_ptr(), cache_v.data_ptr(), lens.data_ptr(), _lib.p(new_lens), out.data_ptr(), B, T, H, Hkv,
              cache_k.shape[2], max_len, table.shape[0], 1.0 / math.sqrt(D))
    return out


def kv_cache_fill(qkv, cache_k, cache_v, num_heads):
    B, S, _ = qkv.shape
    _check_cache(cache_k, cache_v, B, num_heads)
    qkv = qkv.contiguous()
    _lib.call("ddl_kv_cache_fill", qkv.data_ptr(), cache_k.data_ptr(), cache_v.data_ptr(), B, S, num_heads,
              cache_k.shape[2])


def kv_cache_fill_gqa(packed, cache_k, cache_v, num_heads, num_kv_heads):
    B, S, _ = packed.shape
    D = _check_cache(cache_k, cache_v, B, num_kv_heads, "Hkv", DECODE_HEAD_DIMS)
    if packed.shape[2] != 3 * num_heads * D:
        raise ValueError(f"packed must be rope_qkv's [B, S, 3 H {D}], got {tuple(packed.shape)}")
    packed = packed.contiguous()
    _lib.call("ddl_kv_cache_fill_gqa" if D == 64 else "ddl_kv_cache_fill_gqa_d128", packed.data_ptr(), cache_k.data_ptr(), cache_v.data_ptr(), B, S, num_heads,
              num_kv_heads, cache_k.shape[2])


def attention_decode_gqa_fp8(qkv_new, table, cache_k, cache_v, scale_k, scale_v, lens, num_heads, num_kv_heads,
                             max_len):
    """The caller (``ops.attention``) has checked the shapes, dtypes and contiguity of the four cache tensors."""
    B, H, Hkv = qkv_new.shape[0], num_heads, num_kv_heads
    qkv_new, table = qkv_new.contiguous(), table.contiguous()
    out = torch.empty(B, H * 128, dtype=qkv_new.dtype, device=qkv_new.device)
    ws = _workspace("ddl_attn_decode_gqa_ws_hd", qkv_new.device, B, H, Hkv, max_len, 128)    # the bf16 kernel's plan
    _lib.call("ddl_attn_decode_gqa_d128_fp8", qkv_new.data_ptr(), table.data_ptr(), cache_k.data_ptr(),
              cache_v.data_ptr(), scale_k.data_ptr(), scale_v.data_ptr(), lens.data_ptr(), out.data_ptr(), _lib.p(ws),
              B, H, Hkv, cache_k.shape[2], max_len, table.shape[0], 1.0 / math.sqrt(128))
    return out


def kv_cache_fill_gqa_fp8(packed, cache_k, cache_v, scale_k, scale_v, num_heads, num_kv_heads):
    B, S, _ = packed.shape
    packed = packed.contiguous()
    _lib.call("ddl_kv_cache_fill_gqa_d128_fp8", packed.data_ptr(), cache_k.data_ptr(), cache_v.data_ptr(),
              scale_k.data_ptr(), scale_v.data_ptr(), B, S, num_heads, num_kv_heads, cache_k.shape[2])


def attention_extend_gqa_fp8(qkv_new, table, cache_k, cache_v, scale_k, scale_v, lens, num_heads, num_kv_heads, max_len,
                             new_lens=None):
    """The caller (``ops.attention``) has checked the shapes, dtypes, contiguity and alignment of the four cache
    tensors."""
    B, T, H, Hkv = qkv_new.shape[0], qkv_new.shape[1], num_heads, num_kv_heads
    _check_lens(B, lens, new_lens)
    qkv_new, table = qkv_new.contiguous(), table.contiguous()
    out = torch.empty(B, T, H * 128, dtype=qkv_new.dtype, device=qkv_new.device)
    _lib.call("ddl_attn_extend_gqa_d128_fp8", qkv_new.data_ptr(), table.data_ptr(), cache_k.data_ptr(),
              cache_v.data_ptr(), scale_k.data_ptr(), scale_v.data_ptr(), lens.data_ptr(), _lib.p(new_lens),
              out.data_ptr(), B, T, H, Hkv, cache_k.shape[2], max_len, table.shape[0], 1.0 / math.sqrt(128))
    return out
