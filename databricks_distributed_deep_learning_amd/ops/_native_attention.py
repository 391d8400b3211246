"""Fused multi-head attention on MFMA (csrc/kernels/attention.hip), with autograd.

Reads the packed QKV projection in place and writes the packed dQKV gradient, so
no head split / merge copies exist on either pass.  Head dim 64 (BERT-base/large,
ViT-B/16); other head dims use the reference path.
"""
from __future__ import annotations

import math

import torch

from . import _lib
from ._lib import F as CF, I, L, P, U64
from ._native_elementwise import new_seed

_lib.register({
    "ddl_attn_fwd": [P, P, P, P, I, I, I, CF, CF, U64, P, P],
    "ddl_attn_bwd": [P, P, P, P, P, P, P, I, I, I, CF, CF, P, P, P],
    "ddl_attn_dmask_words": [I, I, I],
    # causal (query i attends to keys j <= i): the tiled kernels' CAUSAL instances for every S
    "ddl_attn_causal_fwd": [P, P, P, P, I, I, I, CF, CF, U64, P, P],
    "ddl_attn_causal_bwd": [P, P, P, P, P, P, P, I, I, I, CF, CF, P, P, P],
    # packed rows (doc_start[b, i] <= j <= i): their DOC instances; the causal arguments + doc_start, doc_end
    "ddl_attn_doc_fwd": [P, P, P, P, I, I, I, CF, CF, U64, P, P, P, P],
    "ddl_attn_doc_bwd": [P, P, P, P, P, P, P, I, I, I, CF, CF, P, P, P, P, P],
})

# the backward also writes column sums of dQKV, from which the QKV Linear takes its bias gradient
# instead of another pass over dQKV


def doc_end_from_start(doc_start):
    """The exclusive end of each token's document from the non-decreasing ``doc_start`` ``[B, S]``: the
    first index whose document starts later.  Stays on the device."""
    return torch.searchsorted(doc_start, doc_start, right=True).to(torch.int32)


class _Attention(torch.autograd.Function):
    @staticmethod
    def forward(ctx, qkv, num_heads, mask, p_drop, causal=False, doc_start=None, doc_end=None):
        qkv = qkv.contiguous()
        B, S, three_hd = qkv.shape
        H = num_heads
        D = three_hd // (3 * H)
        scale = 1.0 / math.sqrt(D)
        out = torch.empty(B, S, H * D, dtype=qkv.dtype, device=qkv.device)
        lse = torch.empty(B, H, S, dtype=torch.float32, device=qkv.device)
        m = None if mask is None else mask.to(torch.float32).reshape(B, S).contiguous()
        seed = new_seed() if p_drop > 0 else 0
        # dropout: the forward draws the keep decisions and stores them as bits (1 per score);
        # the backward reads them instead of regenerating them
        dmask = None
        if p_drop > 0:
            fn = _lib.fn("ddl_attn_dmask_words")
            fn.restype = L
            dmask = torch.empty(fn(B, S, H), dtype=torch.int32, device=qkv.device)
        if doc_start is not None:
            _lib.call("ddl_attn_doc_fwd", qkv.data_ptr(), 0, out.data_ptr(), lse.data_ptr(), B, S, H, scale,
                      float(p_drop), seed, _lib.p(dmask), doc_start.data_ptr(), doc_end.data_ptr())
        else:
            _lib.call("ddl_attn_causal_fwd" if causal else "ddl_attn_fwd", qkv.data_ptr(), _lib.p(m), out.data_ptr(), lse.data_ptr(), B, S, H, scale,
                      float(p_drop), seed, _lib.p(dmask))
        ctx.meta = (B, S, H, scale, float(p_drop), seed, bool(causal))
        ctx.save_for_backward(qkv, out, lse, m, dmask, doc_start, doc_end)
        return out

    @staticmethod
    def backward(ctx, dout):
        qkv, out, lse, m, dmask, doc_start, doc_end = ctx.saved_tensors
        B, S, H, scale, p_drop, seed, causal = ctx.meta
        dout = dout.contiguous()
        delta = torch.empty(B, H, S, dtype=torch.float32, device=qkv.device)
        dqkv = torch.empty_like(qkv)
        # QKV bias gradient rows: per batch (single-workgroup kernels) or per batch and 16-row group
        # (tiled backward kernels: 64-row workgroups of 4 waves)
        tiled_rows = B * 4 * -(-S // 64)
        cs = torch.empty(tiled_rows, 3 * H * 64, dtype=torch.float32, device=qkv.device)
        if doc_start is not None:
            name = "ddl_attn_doc_bwd"
            rc = _lib.fn(name)(qkv.data_ptr(), out.data_ptr(), dout.data_ptr(), lse.data_ptr(), 0,
                               delta.data_ptr(), dqkv.data_ptr(), B, S, H, scale, p_drop, _lib.p(dmask),
                               _lib.p(cs), doc_start.data_ptr(), doc_end.data_ptr(), _lib.stream())
        else:
            name = "ddl_attn_causal_bwd" if causal else "ddl_attn_bwd"
            rc = _lib.fn(name)(qkv.data_ptr(), out.data_ptr(), dout.data_ptr(), lse.data_ptr(), _lib.p(m),
                                         delta.data_ptr(), dqkv.data_ptr(), B, S, H, scale, p_drop, _lib.p(dmask),
                                         _lib.p(cs), _lib.stream())
        if rc not in (0, 2) or (causal and rc != 2):     # causal: always the tiled-row form
            raise RuntimeError(f"native kernel {name} failed with HIP error {rc}")
        # rides on the gradient: the producing Linear's bias gradient = column sums of these rows
        # (the version guards against autograd accumulating another gradient into dqkv)
        dqkv._ddl_colsum_rows = (cs[:tiled_rows] if rc == 2 else cs[:B], dqkv._version)
        return dqkv, None, None, None, None, None, None


def attention(qkv, num_heads, mask, dropout_p, causal=False, doc=None):
    """``doc``: ``(doc_start, doc_end or None)``, int32 ``[B, S]`` (packed rows; causal, no key bias)."""
    B, S, three_hd = qkv.shape
    if qkv.dtype != torch.bfloat16 or three_hd != 3 * 64 * num_heads:
        from .attention import attention_reference
        return attention_reference(qkv, num_heads, mask, dropout_p, dropout_p > 0, causal=causal,
                                   doc_start=None if doc is None else doc[0])
    if doc is None:
        return _Attention.apply(qkv, num_heads, mask, float(dropout_p), bool(causal))
    if mask is not None or not causal:
        raise ValueError("the document-masked kernels are causal and take no key bias")
    ds = doc[0].contiguous()
    de = doc_end_from_start(ds) if doc[1] is None else doc[1].contiguous()
    return _Attention.apply(qkv, num_heads, None, float(dropout_p), True, ds, de)
