"""Multi-head self-attention core (kernel families K14/K15).

Input is the packed QKV projection ``[B, S, 3·H·D]`` exactly as the fused QKV
GEMM writes it (no permute/copy), output is ``[B, S, H·D]`` ready for the
output projection.  ``mask`` is an optional additive key bias ``[B, S]`` (0 for
keep, large negative for padding), the HF extended-attention-mask convention.
``causal=True`` additionally hides every key after the query's own position
(autoregressive decoders); the key bias adds on top of it.
"""
from __future__ import annotations

import math
import warnings
from typing import Optional

import torch
import torch.nn.functional as F

from . import _lib

_warned_mask_doc = False


def doc_bounds(position_ids: torch.Tensor):
    """Document bounds of packed rows from HF-style ``position_ids`` (int ``[B, S]``): every row starts at 0
    and every further entry is the previous one plus 1, or 0 where a new document starts (``ValueError``
    otherwise).  Returns ``(doc_start, doc_end)``, int32 ``[B, S]`` on the same device: the row index of the
    first token of each token's document (``i - position_ids[b, i]``) and the exclusive end of that document.
    ``ops.attention(..., causal=True, doc_start=...)`` takes the first, or the pair as it is.

    The check reads the device once (a host synchronisation), so call it once per batch, not per layer."""
    pos = position_ids
    if pos.dim() != 2 or pos.dtype not in (torch.int32, torch.int64) or pos.shape[1] < 1:
        raise ValueError(f"position_ids must be an int32 / int64 [B, S >= 1] tensor, got {pos.dtype} "
                         f"{tuple(pos.shape)}")
    B, S = pos.shape
    ok = (pos[:, 0] == 0).all() & ((pos[:, 1:] == pos[:, :-1] + 1) | (pos[:, 1:] == 0)).all()
    if not bool(ok):
        raise ValueError("position_ids must start every row at 0 and continue with previous + 1, or 0 where a "
                         "new document starts")
    ar = torch.arange(S, device=pos.device)
    doc_start = (ar[None, :] - pos).to(torch.int32).contiguous()
    # the end of token i's document: the first start after i, S without one
    nxt = torch.where(pos == 0, ar[None, :], torch.full_like(pos, S))
    nxt = torch.cat([nxt[:, 1:], torch.full_like(nxt[:, :1], S)], 1)
    doc_end = nxt.flip(1).cummin(1).values.flip(1).to(torch.int32).contiguous()
    return doc_start, doc_end


def _doc_pair(doc_start, qkv):
    """``doc_start`` as ``ops.attention`` takes it -- the int32 ``[B, S]`` tensor or ``doc_bounds``' pair, on
    ``qkv``'s device -- as ``(doc_start, doc_end or None)``."""
    B, S = qkv.shape[:2]
    ds, de = doc_start if isinstance(doc_start, (tuple, list)) else (doc_start, None)
    for t in (ds, de):
        if t is not None and (t.dtype != torch.int32 or t.shape != (B, S) or t.device != qkv.device):
            raise ValueError(f"doc_start must be int32 [B={B}, S={S}] on {qkv.device}, got {t.dtype} "
                             f"{tuple(t.shape)} on {t.device}")
    return ds, de


def attention_reference(qkv: torch.Tensor, num_heads: int, mask: Optional[torch.Tensor] = None,
                        dropout_p: float = 0.0, training: bool = False, causal: bool = False,
                        doc_start=None) -> torch.Tensor:
    B, S, three_hd = qkv.shape
    hd = three_hd // 3
    D = hd // num_heads
    q, k, v = qkv.view(B, S, 3, num_heads, D).permute(2, 0, 3, 1, 4).unbind(0)
    attn_mask = None
    if mask is not None:
        attn_mask = mask.view(B, 1, 1, S).to(q.dtype if q.is_cuda else torch.float32)
    tri = None
    if causal:      # -inf above the diagonal, [S, S]
        tri = torch.full((S, S), float("-inf"), device=q.device, dtype=torch.float32).triu(1)
    if doc_start is not None:
        if not causal:
            raise ValueError("doc_start masks packed causal rows: it needs causal=True")
        ds = _doc_pair(doc_start, qkv)[0]
        # -inf on the keys before the query's document as well, [B, 1, S, S]
        before = torch.arange(S, device=q.device).view(1, 1, 1, S) < ds.view(B, 1, S, 1)
        tri = tri.expand(B, 1, S, S).masked_fill(before, float("-inf"))
    if q.is_cuda:
        if tri is not None:     # one combined mask (SDPA takes either is_causal or attn_mask)
            attn_mask = tri.to(q.dtype) if attn_mask is None else attn_mask + tri.to(q.dtype)
        o = F.scaled_dot_product_attention(q, k, v, attn_mask=attn_mask,
                                           dropout_p=dropout_p if training else 0.0)
    else:
        qf, kf, vf = q.float(), k.float(), v.float()
        s = qf @ kf.transpose(-1, -2) / math.sqrt(D)
        if attn_mask is not None:
            s = s + attn_mask.float()
        if tri is not None:
            s = s + tri
        p = torch.softmax(s, -1)
        if training and dropout_p > 0:
            p = F.dropout(p, dropout_p, True)
        o = (p @ vf).to(q.dtype)
    return o.permute(0, 2, 1, 3).reshape(B, S, hd)


def attention(qkv: torch.Tensor, num_heads: int, mask: Optional[torch.Tensor] = None,
              dropout_p: float = 0.0, training: bool = False, *, causal: bool = False,
              doc_start=None) -> torch.Tensor:
    """``doc_start`` (with ``causal=True``): packed rows.  int32 ``[B, S]`` on the tensors' device, the row
    index of the first token of each token's document; query i then sees key j iff
    ``doc_start[b, i] <= j <= i``.  ``ops.doc_bounds`` builds it from ``position_ids``, and only what it
    returns is supported: non-decreasing along a row with ``doc_start[b, i] <= i``.  That is not checked here
    (it would cost a host synchronisation per layer); the kernels take their loop bounds from a workgroup's
    first row, so a tensor that breaks it is memory-safe but gives other results than the reference.  The
    ``(doc_start, doc_end)`` pair may be passed as it is, which spares the native path deriving the ends on
    every call.  There is no native kernel for ``mask`` together with ``doc_start``: that combination takes
    the reference composition, an ``[B, 1, S, S]`` mask per call, and warns once (in a packed row the unused
    tail is a document of its own whose labels are -100, so no key bias is needed)."""
    if doc_start is not None and not causal:
        raise ValueError("doc_start masks packed causal rows: it needs causal=True")
    if _lib.use_native(qkv):
        if doc_start is None:
            from . import _native_attention
            return _native_attention.attention(qkv, num_heads, mask, dropout_p if training else 0.0, causal)
        ds, de = _doc_pair(doc_start, qkv)
        if mask is None:
            from . import _native_attention
            return _native_attention.attention(qkv, num_heads, None, dropout_p if training else 0.0, True,
                                               doc=(ds, de))
        global _warned_mask_doc
        if not _warned_mask_doc:
            _warned_mask_doc = True
            warnings.warn("ops.attention: a key bias (attention_mask) together with doc_start has no HIP kernel and "
                          "runs the reference attention with an [B, 1, S, S] mask; packed rows need no "
                          "attention_mask", RuntimeWarning, stacklevel=2)
    return attention_reference(qkv, num_heads, mask, dropout_p, training, causal=causal, doc_start=doc_start)


# ------------------------------------------------------------------ decode (one new token per sequence, KV cache)
# cache_k / cache_v: [B, H, C, D], C the capacity in positions; lens: int32 [B], the valid positions of
# each batch row (on the tensors' device: nothing here reads it on the host).  qkv_new is the new token's
# packed [B, 3·H·D] projection.  For row b with n = lens[b] the query attends to cached keys 0..n-1 and
# to the new key, and the new K / V rows are stored to cache[b, :, n].  lens is NOT changed: every layer
# of a decode step shares it and the caller adds 1 once per step.  max_len is the host's upper bound on
# n + 1 (it sizes the launch); positions past n never reach the output, whatever they hold.
def _no_autograd(name, *tensors):
    if any(t.requires_grad for t in tensors):
        raise RuntimeError(f"{name} has no autograd: call it under torch.no_grad() on detached tensors")


def _check_lens(B, lens, new_lens=None):
    for name, t in (("lens", lens), ("new_lens", new_lens)):
        if t is not None and (t.dtype != torch.int32 or t.shape != (B,) or not t.is_contiguous()):
            raise ValueError(f"{name} must be a contiguous int32 [B] tensor")


def _decode_bounds(cache_k, max_len):
    """``max_len`` bounds ``lens + 1`` and must fit the cache."""
    if max_len > cache_k.shape[2]:
        raise ValueError(f"max_len {max_len} exceeds the cache capacity {cache_k.shape[2]}")
    if max_len < 1:
        raise ValueError("max_len counts the new token: at least 1")


def _extend_bounds(cache_k, max_len, T):
    """``max_len`` bounds ``lens``; the chunk's ``T`` tokens come on top and must fit the cache."""
    if max_len < 0:
        raise ValueError("max_len bounds lens: at least 0")
    if max_len + T > cache_k.shape[2]:
        raise ValueError(f"max_len {max_len} + the chunk's {T} tokens exceeds the cache capacity {cache_k.shape[2]}")


def _decode_guard(qkv_new, cache_k, cache_v, max_len):
    _no_autograd("attention_decode", qkv_new, cache_k, cache_v)
    _decode_bounds(cache_k, max_len)


def attention_decode_reference(qkv_new: torch.Tensor, cache_k: torch.Tensor, cache_v: torch.Tensor,
                               lens: torch.Tensor, num_heads: int, max_len: int) -> torch.Tensor:
    _decode_guard(qkv_new, cache_k, cache_v, max_len)
    B, three_hd = qkv_new.shape
    D = three_hd // (3 * num_heads)
    q, k, v = qkv_new.view(B, 3, num_heads, D).unbind(1)
    n = lens.long()
    bi = torch.arange(B, device=qkv_new.device)
    cache_k[bi, :, n] = k.to(cache_k.dtype)
    cache_v[bi, :, n] = v.to(cache_v.dtype)
    ct = torch.float64 if qkv_new.dtype == torch.float64 else torch.float32
    live = torch.arange(max_len, device=qkv_new.device).view(1, 1, max_len) <= n.view(B, 1, 1)      # [B, 1, L]
    kk, vv = cache_k[:, :, :max_len].to(ct), cache_v[:, :, :max_len].to(ct)
    s = (q.to(ct).unsqueeze(2) @ kk.transpose(-1, -2)).squeeze(2) / math.sqrt(D)       # [B, H, L]
    # selects, not multiplies: a dead position may hold any bit pattern
    p = torch.softmax(torch.where(live, s, torch.full_like(s, float("-inf"))), -1)
    vv = torch.where(live.unsqueeze(-1), vv, torch.zeros_like(vv))
    o = (p.unsqueeze(2) @ vv).squeeze(2)                                               # [B, H, D]
    return o.reshape(B, num_heads * D).to(qkv_new.dtype)


def attention_decode(qkv_new: torch.Tensor, cache_k: torch.Tensor, cache_v: torch.Tensor, lens: torch.Tensor,
                     num_heads: int, max_len: int) -> torch.Tensor:
    """Single-query attention over the cache, with the append; returns ``[B, H·D]``."""
    _decode_guard(qkv_new, cache_k, cache_v, max_len)
    if (_lib.use_native(qkv_new, cache_k, cache_v, lens) and qkv_new.dtype == torch.bfloat16
            and cache_k.dtype == torch.bfloat16 and cache_v.dtype == torch.bfloat16
            and qkv_new.shape[1] == 3 * 64 * num_heads):
        from . import _native_attn_cache
        return _native_attn_cache.attention_decode(qkv_new, cache_k, cache_v, lens, num_heads, max_len)
    return attention_decode_reference(qkv_new, cache_k, cache_v, lens, num_heads, max_len)


def kv_cache_fill_reference(qkv: torch.Tensor, cache_k: torch.Tensor, cache_v: torch.Tensor, num_heads: int) -> None:
    B, S, three_hd = qkv.shape
    D = three_hd // (3 * num_heads)
    _, k, v = qkv.view(B, S, 3, num_heads, D).permute(2, 0, 3, 1, 4).unbind(0)
    cache_k[:, :, :S] = k.to(cache_k.dtype)
    cache_v[:, :, :S] = v.to(cache_v.dtype)


def kv_cache_fill(qkv: torch.Tensor, cache_k: torch.Tensor, cache_v: torch.Tensor, num_heads: int) -> None:
    """After a prefill: the K and V thirds of the packed ``[B, S, 3·H·D]`` projection into cache positions
    0..S-1 (rows past a sequence's own length too: they are dead by ``lens``)."""
    _no_autograd("kv_cache_fill", qkv, cache_k, cache_v)
    if qkv.shape[1] > cache_k.shape[2]:
        raise ValueError(f"sequence length {qkv.shape[1]} exceeds the cache capacity {cache_k.shape[2]}")
    if (_lib.use_native(qkv, cache_k, cache_v) and qkv.dtype == torch.bfloat16 and cache_k.dtype == torch.bfloat16
            and cache_v.dtype == torch.bfloat16 and qkv.shape[2] == 3 * 64 * num_heads):
        from . import _native_attn_cache
        return _native_attn_cache.kv_cache_fill(qkv, cache_k, cache_v, num_heads)
    return kv_cache_fill_reference(qkv, cache_k, cache_v, num_heads)


# ------------------------------------------------------------------ extend (a chunk of T new tokens per sequence)
# qkv_new is the chunk's packed [B, T, 3·H·D] projection.  For row b with n = lens[b] and t = new_lens[b]
# (T without new_lens; 1 <= t <= T: rows are right-padded), query i < t attends to cached keys 0..n-1 and
# to chunk keys 0..i -- read from qkv_new, never from the cache -- and output rows i >= t are zeros.  The
# K / V rows of chunk positions i < t are stored to cache[b, :, n+i]; nothing else in the cache changes.
# (A caller that must pass a row with no real token -- GPT2LMHeadModel.extend with new_lens[b] == 0 -- hands
# it t = 1: that row's dead position n then does change; it stays dead as long as the caller does not
# advance lens for it.)
# lens is NOT changed (every layer shares it; the caller adds new_lens once).  max_len is the host's
# upper bound on lens; max_len + T must fit the capacity.
def _extend_guard(qkv_new, cache_k, cache_v, max_len):
    _no_autograd("attention_extend", qkv_new, cache_k, cache_v)
    if qkv_new.dim() != 3 or qkv_new.shape[1] < 1:
        raise ValueError(f"qkv_new must be [B, T >= 1, 3·H·D], got {tuple(qkv_new.shape)}")
    _extend_bounds(cache_k, max_len, qkv_new.shape[1])


def attention_extend_reference(qkv_new: torch.Tensor, cache_k: torch.Tensor, cache_v: torch.Tensor,
                               lens: torch.Tensor, num_heads: int, max_len: int,
                               new_lens: Optional[torch.Tensor] = None) -> torch.Tensor:
    _extend_guard(qkv_new, cache_k, cache_v, max_len)
    B, T, three_hd = qkv_new.shape
    D = three_hd // (3 * num_heads)
    dev = qkv_new.device
    q, k, v = qkv_new.view(B, T, 3, num_heads, D).permute(2, 0, 3, 1, 4).unbind(0)     # [B, H, T, D]
    n = lens.long().clamp(0, max_len)
    t = torch.full_like(n, T) if new_lens is None else new_lens.long().clamp(1, T)
    ct = torch.float64 if qkv_new.dtype == torch.float64 else torch.float32
    i = torch.arange(T, device=dev)
    qlive = i.view(1, T) < t.view(B, 1)                                                # [B, T]
    # keys: the cache's first max_len positions (live while < n), then the chunk (live while <= the query)
    live = torch.cat([(torch.arange(max_len, device=dev).view(1, 1, max_len) < n.view(B, 1, 1)).expand(B, T, max_len),
                      (i.view(1, 1, T) <= i.view(1, T, 1)).expand(B, T, T)], 2).unsqueeze(1)    # [B, 1, T, L + T]
    kk = torch.cat([cache_k[:, :, :max_len].to(ct), k.to(ct)], 2)
    vv = torch.cat([cache_v[:, :, :max_len].to(ct), v.to(ct)], 2)
    s = q.to(ct) @ kk.transpose(-1, -2) / math.sqrt(D)                                 # [B, H, T, L + T]
    # selects, not multiplies: a dead position (and a padded chunk row) may hold any bit pattern
    p = torch.softmax(torch.where(live, s, torch.full_like(s, float("-inf"))), -1)
    vlive = torch.cat([torch.arange(max_len, device=dev).view(1, max_len) < n.view(B, 1), qlive], 1)   # [B, L + T]
    vv = torch.where(vlive.view(B, 1, -1, 1), vv, torch.zeros_like(vv))
    o = torch.where(qlive.view(B, 1, T, 1), p @ vv, torch.zeros((), dtype=ct, device=dev))
    # the append: chunk position i < t of row b to cache position n + i
    bi, ii = torch.nonzero(qlive, as_tuple=True)
    cache_k[bi, :, n[bi] + ii] = k.to(cache_k.dtype)[bi, :, ii]
    cache_v[bi, :, n[bi] + ii] = v.to(cache_v.dtype)[bi, :, ii]
    return o.permute(0, 2, 1, 3).reshape(B, T, num_heads * D).to(qkv_new.dtype)


def attention_extend(qkv_new: torch.Tensor, cache_k: torch.Tensor, cache_v: torch.Tensor, lens: torch.Tensor,
                     num_heads: int, max_len: int, new_lens: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Causal attention of a chunk of new tokens over the cache plus the chunk, with the append; returns
    ``[B, T, H·D]``."""
    _extend_guard(qkv_new, cache_k, cache_v, max_len)
    if (_lib.use_native(qkv_new, cache_k, cache_v, lens, new_lens) and qkv_new.dtype == torch.bfloat16
            and cache_k.dtype == torch.bfloat16 and cache_v.dtype == torch.bfloat16
            and qkv_new.shape[2] == 3 * 64 * num_heads):
        from . import _native_attn_cache
        return _native_attn_cache.attention_extend(qkv_new, cache_k, cache_v, lens, num_heads, max_len, new_lens)
    return attention_extend_reference(qkv_new, cache_k, cache_v, lens, num_heads, max_len, new_lens)


# ------------------------------------------------------------------ grouped-query decode (rotated KV cache)
# The Llama family's cache: cache_k / cache_v [B, Hkv, C, D] hold ROTATED keys for the Hkv key / value heads
# (never expanded to the H query heads).  qkv_new [B, (H + 2 Hkv) D] is the new token's fused, UNROTATED
# projection [q heads | k heads | v heads] and table the fp32 [n_pos, D] of ops.rope_table.  For row b with
# n = lens[b] the query heads and the new key are rotated by table row n (HF half-split pairs, computed in
# fp32 -- fp64 for fp64 inputs -- and rounded once to the input dtype: what ops.rope_qkv hands a full
# forward); the G = H / Hkv query heads of KV head j attend to its cached keys 0..n-1 and to the new key, and
# the rotated key and the value are stored to cache[b, :, n].  lens is NOT changed; max_len is the host's
# upper bound on n + 1 and must fit both the cache and the table.
def _gqa_heads(num_heads, num_kv_heads):
    if num_kv_heads < 1 or num_heads < 1 or num_heads % num_kv_heads:
        raise ValueError(f"num_heads {num_heads} must be a multiple of num_kv_heads {num_kv_heads}")


def _check_gqa_cache(cache_k, cache_v, B, num_kv_heads, D):
    if (cache_k.shape != cache_v.shape or cache_k.dim() != 4 or cache_k.shape[0] != B
            or cache_k.shape[1] != num_kv_heads or cache_k.shape[3] != D):
        raise ValueError(f"cache must be [B={B}, Hkv={num_kv_heads}, C, {D}] for keys and values, got "
                         f"{tuple(cache_k.shape)} / {tuple(cache_v.shape)}")
    if not (cache_k.is_contiguous() and cache_v.is_contiguous()):
        raise ValueError("cache tensors must be contiguous")


def _decode_gqa_guard(qkv_new, table, cache_k, cache_v, lens, num_heads, num_kv_heads, max_len):
    _no_autograd("attention_decode_gqa", qkv_new, table, cache_k, cache_v)
    _gqa_heads(num_heads, num_kv_heads)
    W = num_heads + 2 * num_kv_heads
    if qkv_new.dim() != 2 or qkv_new.shape[1] % W or (qkv_new.shape[1] // W) % 2:
        raise ValueError(f"qkv_new must be [B, (H + 2 Hkv)·D] with D even, got {tuple(qkv_new.shape)}")
    B, D = qkv_new.shape[0], qkv_new.shape[1] // W
    _check_gqa_cache(cache_k, cache_v, B, num_kv_heads, D)
    if table.dim() != 2 or table.shape[1] != D:
        raise ValueError(f"table must be [n_positions, {D}], got {tuple(table.shape)}")
    _check_lens(B, lens)
    _decode_bounds(cache_k, max_len)
    if max_len > table.shape[0]:
        raise ValueError(f"max_len {max_len} exceeds the rotary table's {table.shape[0]} positions")
    return D


def attention_decode_gqa_reference(qkv_new: torch.Tensor, table: torch.Tensor, cache_k: torch.Tensor,
                                   cache_v: torch.Tensor, lens: torch.Tensor, num_heads: int, num_kv_heads: int,
                                   max_len: int) -> torch.Tensor:
    D = _decode_gqa_guard(qkv_new, table, cache_k, cache_v, lens, num_heads, num_kv_heads, max_len)
    B, H, Hkv, half = qkv_new.shape[0], num_heads, num_kv_heads, D // 2
    G = H // Hkv
    dev = qkv_new.device
    ct = torch.float64 if qkv_new.dtype == torch.float64 else torch.float32
    n = lens.long()
    x = qkv_new.to(ct).view(B, H + 2 * Hkv, D)
    row = table[n].to(ct)                                                              # [B, D]
    cos, sin = row[:, None, :half], row[:, None, half:]

    def rot(t):
        a, b = t[..., :half], t[..., half:]
        return torch.cat([a * cos - b * sin, b * cos + a * sin], -1)

    # rounded once to the input dtype: the operands a full forward sees after rope_qkv
    q = rot(x[:, :H]).to(qkv_new.dtype)
    k = rot(x[:, H:H + Hkv]).to(qkv_new.dtype)
    v = qkv_new.view(B, H + 2 * Hkv, D)[:, H + Hkv:]
    bi = torch.arange(B, device=dev)
    cache_k[bi, :, n] = k.to(cache_k.dtype)
    cache_v[bi, :, n] = v.to(cache_v.dtype)
    live = torch.arange(max_len, device=dev).view(1, 1, 1, max_len) <= n.view(B, 1, 1, 1)
    kk, vv = cache_k[:, :, :max_len].to(ct), cache_v[:, :, :max_len].to(ct)            # [B, Hkv, L, D]
    s = q.to(ct).view(B, Hkv, G, D) @ kk.transpose(-1, -2) / math.sqrt(D)              # [B, Hkv, G, L]
    # selects, not multiplies: a dead position may hold any bit pattern
    p = torch.softmax(torch.where(live, s, torch.full_like(s, float("-inf"))), -1)
    vv = torch.where(live.squeeze(1).unsqueeze(-1), vv, torch.zeros_like(vv))
    return (p @ vv).reshape(B, H * D).to(qkv_new.dtype)


def attention_decode_gqa(qkv_new: torch.Tensor, table: torch.Tensor, cache_k: torch.Tensor, cache_v: torch.Tensor,
                         lens: torch.Tensor, num_heads: int, num_kv_heads: int, max_len: int) -> torch.Tensor:
    """Grouped-query single-query attention over the rotated cache, with the new token's rotation and the
    append; returns ``[B, H·D]``."""
    D = _decode_gqa_guard(qkv_new, table, cache_k, cache_v, lens, num_heads, num_kv_heads, max_len)
    if (_lib.use_native(qkv_new, table, cache_k, cache_v, lens) and qkv_new.dtype == torch.bfloat16
            and cache_k.dtype == torch.bfloat16 and cache_v.dtype == torch.bfloat16
            and table.dtype == torch.float32 and D == 64):
        from . import _native_attn_cache as N
        if N.supported(num_heads, num_kv_heads):
            return N.attention_decode_gqa(qkv_new, table, cache_k, cache_v, lens, num_heads, num_kv_heads, max_len)
    return attention_decode_gqa_reference(qkv_new, table, cache_k, cache_v, lens, num_heads, num_kv_heads, max_len)


def _fill_gqa_guard(packed, cache_k, cache_v, num_heads, num_kv_heads):
    _no_autograd("kv_cache_fill_gqa", packed, cache_k, cache_v)
    _gqa_heads(num_heads, num_kv_heads)
    if packed.dim() != 3 or packed.shape[2] % (3 * num_heads):
        raise ValueError(f"packed must be rope_qkv's [B, S, 3·H·D], got {tuple(packed.shape)}")
    D = packed.shape[2] // (3 * num_heads)
    _check_gqa_cache(cache_k, cache_v, packed.shape[0], num_kv_heads, D)
    if packed.shape[1] > cache_k.shape[2]:
        raise ValueError(f"sequence length {packed.shape[1]} exceeds the cache capacity {cache_k.shape[2]}")
    return D


def kv_cache_fill_gqa_reference(packed: torch.Tensor, cache_k: torch.Tensor, cache_v: torch.Tensor, num_heads: int,
                                num_kv_heads: int) -> None:
    D = _fill_gqa_guard(packed, cache_k, cache_v, num_heads, num_kv_heads)
    B, S, _ = packed.shape
    G = num_heads // num_kv_heads
    _, k, v = packed.view(B, S, 3, num_heads, D)[:, :, :, ::G].permute(2, 0, 3, 1, 4).unbind(0)
    cache_k[:, :, :S] = k.to(cache_k.dtype)
    cache_v[:, :, :S] = v.to(cache_v.dtype)


def kv_cache_fill_gqa(packed: torch.Tensor, cache_k: torch.Tensor, cache_v: torch.Tensor, num_heads: int,
                      num_kv_heads: int) -> None:
    """After a prefill: from ``rope_qkv``'s packed ``[B, S, 3·H·D]`` (keys already rotated, every KV head
    repeated to its G query-head slots) the first slot of every group goes to cache positions 0..S-1 of
    ``[B, Hkv, C, D]`` (rows past a sequence's own length too: they are dead by ``lens``).  A bit copy."""
    D = _fill_gqa_guard(packed, cache_k, cache_v, num_heads, num_kv_heads)
    if (_lib.use_native(packed, cache_k, cache_v) and packed.dtype == torch.bfloat16
            and cache_k.dtype == torch.bfloat16 and cache_v.dtype == torch.bfloat16 and D == 64):
        from . import _native_attn_cache as N
        return N.kv_cache_fill_gqa(packed, cache_k, cache_v, num_heads, num_kv_heads)
    return kv_cache_fill_gqa_reference(packed, cache_k, cache_v, num_heads, num_kv_heads)


# ------------------------------------------------------------------ grouped-query extend (rotated KV cache)
# A chunk of T new tokens per sequence against the Llama family's cache.  qkv_new [B, T, (H + 2 Hkv) D] is the
# chunk's fused, UNROTATED projection and table the fp32 [n_pos, D] of ops.rope_table.  For row b with
# n = lens[b] (clamped to 0 .. max_len) and t = new_lens[b] (clamped to 1 .. T; T without new_lens: rows are
# right-padded), chunk token i < t has its H query heads and Hkv key heads rotated by table row n + i (HF
# half-split pairs, computed in fp32 -- fp64 for fp64 inputs -- and rounded once to the input dtype: what
# ops.rope_qkv hands a full forward).  Query i of head h attends to cached keys 0..n-1 of KV head h / G and to
# the rotated chunk keys 0..i of that head; output rows i >= t are zeros.  The rotated key and the value of
# chunk positions i < t are stored to cache[b, :, n+i]; nothing else in the cache changes.  (A caller that must
# pass a row with no real token hands it t = 1, as for attention_extend.)  lens and new_lens are NOT changed;
# max_len is the host's upper bound on lens, and max_len + T must fit both the cache and the table.
def _extend_gqa_guard(qkv_new, table, cache_k, cache_v, lens, num_heads, num_kv_heads, max_len, new_lens):
    _no_autograd("attention_extend_gqa", qkv_new, table, cache_k, cache_v)
    _gqa_heads(num_heads, num_kv_heads)
    W = num_heads + 2 * num_kv_heads
    if qkv_new.dim() != 3 or qkv_new.shape[1] < 1 or qkv_new.shape[2] % W or (qkv_new.shape[2] // W) % 2:
        raise ValueError(f"qkv_new must be [B, T >= 1, (H + 2 Hkv)·D] with D even, got {tuple(qkv_new.shape)}")
    B, T, D = qkv_new.shape[0], qkv_new.shape[1], qkv_new.shape[2] // W
    _check_gqa_cache(cache_k, cache_v, B, num_kv_heads, D)
    if table.dim() != 2 or table.shape[1] != D:
        raise ValueError(f"table must be [n_positions, {D}], got {tuple(table.shape)}")
    _check_lens(B, lens, new_lens)
    _extend_bounds(cache_k, max_len, T)
    if max_len + T > table.shape[0]:
        raise ValueError(f"max_len {max_len} + the chunk's {T} tokens exceeds the rotary table's {table.shape[0]} "
                         f"positions")
    return D


def attention_extend_gqa_reference(qkv_new: torch.Tensor, table: torch.Tensor, cache_k: torch.Tensor,
                                   cache_v: torch.Tensor, lens: torch.Tensor, num_heads: int, num_kv_heads: int,
                                   max_len: int, new_lens: Optional[torch.Tensor] = None) -> torch.Tensor:
    D = _extend_gqa_guard(qkv_new, table, cache_k, cache_v, lens, num_heads, num_kv_heads, max_len, new_lens)
    B, T, _ = qkv_new.shape
    H, Hkv, half = num_heads, num_kv_heads, D // 2
    G = H // Hkv
    dev = qkv_new.device
    ct = torch.float64 if qkv_new.dtype == torch.float64 else torch.float32
    n = lens.long().clamp(0, max_len)
    t = torch.full_like(n, T) if new_lens is None else new_lens.long().clamp(1, T)
    i = torch.arange(T, device=dev)
    qlive = i.view(1, T) < t.view(B, 1)                                                # [B, T]
    # a padded column rotates by its row's last real position (its result is dropped: the table stays in bounds)
    pos = n.view(B, 1) + torch.minimum(i.view(1, T), t.view(B, 1) - 1)
    x = qkv_new.view(B, T, H + 2 * Hkv, D)
    row = table[pos].to(ct)                                                            # [B, T, D]
    cos, sin = row[:, :, None, :half], row[:, :, None, half:]

    def rot(u):
        a, b = u[..., :half], u[..., half:]
        return torch.cat([a * cos - b * sin, b * cos + a * sin], -1)

    # rounded once to the input dtype: the operands a full forward sees after rope_qkv
    q = rot(x[:, :, :H].to(ct)).to(qkv_new.dtype).permute(0, 2, 1, 3)                   # [B, H, T, D]
    k = rot(x[:, :, H:H + Hkv].to(ct)).to(qkv_new.dtype).permute(0, 2, 1, 3)            # [B, Hkv, T, D]
    v = x[:, :, H + Hkv:].permute(0, 2, 1, 3)
    # keys: the cache's first max_len positions (live while < n), then the chunk (live while <= the query)
    clive = torch.arange(max_len, device=dev).view(1, max_len) < n.view(B, 1)          # [B, L]
    live = torch.cat([clive.view(B, 1, max_len).expand(B, T, max_len),
                      (i.view(1, 1, T) <= i.view(1, T, 1)).expand(B, T, T)], 2).view(B, 1, 1, T, max_len + T)
    kk = torch.cat([cache_k[:, :, :max_len].to(ct), k.to(ct)], 2)                      # [B, Hkv, L + T, D]
    vv = torch.cat([cache_v[:, :, :max_len].to(ct), v.to(ct)], 2)
    s = q.to(ct).reshape(B, Hkv, G, T, D) @ kk.unsqueeze(2).transpose(-1, -2) / math.sqrt(D)
    # selects, not multiplies: a dead position (and a padded chunk row) may hold any bit pattern
    p = torch.softmax(torch.where(live, s, torch.full_like(s, float("-inf"))), -1)
    vlive = torch.cat([clive, qlive], 1)                                               # [B, L + T]
    vv = torch.where(vlive.view(B, 1, -1, 1), vv, torch.zeros_like(vv))
    o = torch.where(qlive.view(B, 1, 1, T, 1), p @ vv.unsqueeze(2), torch.zeros((), dtype=ct, device=dev))
    # the append: chunk position i < t of row b to cache position n + i
    bi, ii = torch.nonzero(qlive, as_tuple=True)
    cache_k[bi, :, n[bi] + ii] = k.to(cache_k.dtype)[bi, :, ii]
    cache_v[bi, :, n[bi] + ii] = v.to(cache_v.dtype)[bi, :, ii]
    return o.reshape(B, H, T, D).permute(0, 2, 1, 3).reshape(B, T, H * D).to(qkv_new.dtype)


def attention_extend_gqa(qkv_new: torch.Tensor, table: torch.Tensor, cache_k: torch.Tensor, cache_v: torch.Tensor,
                         lens: torch.Tensor, num_heads: int, num_kv_heads: int, max_len: int,
                         new_lens: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Grouped-query causal attention of a chunk of new tokens over the rotated cache plus the chunk, with the
    chunk's rotation and the append; returns ``[B, T, H·D]``."""
    D = _extend_gqa_guard(qkv_new, table, cache_k, cache_v, lens, num_heads, num_kv_heads, max_len, new_lens)
    if (_lib.use_native(qkv_new, table, cache_k, cache_v, lens, new_lens) and qkv_new.dtype == torch.bfloat16
            and cache_k.dtype == torch.bfloat16 and cache_v.dtype == torch.bfloat16
            and table.dtype == torch.float32 and D == 64):
        from . import _native_attn_cache as N
        if N.supported(num_heads, num_kv_heads):
            return N.attention_extend_gqa(qkv_new, table, cache_k, cache_v, lens, num_heads, num_kv_heads, max_len,
                                          new_lens)
    return attention_extend_gqa_reference(qkv_new, table, cache_k, cache_v, lens, num_heads, num_kv_heads, max_len,
                                          new_lens)
