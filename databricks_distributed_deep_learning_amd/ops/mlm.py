"""Masked-LM pretraining ops: the row gather at the masked positions and the fused vocabulary head.

``gather_rows`` picks the ``B * P`` hidden rows the MLM head predicts from, so the head's GEMMs and its
``[rows, vocab]`` logits cover 76 rows per sequence instead of 512.  ``linear_cross_entropy`` is the
decoder GEMM and the loss as one op: on the GPU the logits exist once, 8-padded, and their gradient
overwrites them (``_native_mlm._LinearCE``).
"""
from __future__ import annotations

from typing import Optional

import torch

from . import _lib
from .loss import cross_entropy


def gather_rows(h: torch.Tensor, positions: torch.Tensor, labels: Optional[torch.Tensor] = None,
                ignore_index: int = -100) -> torch.Tensor:
    """``out[i] = h[positions[i]]`` for ``h [R, D]`` and ``positions [n]``; or, for ``h [B, S, D]`` and
    ``positions [B, P]`` (positions inside each sequence), ``out[b * P + j] = h[b, positions[b, j]]``
    -- the flat row index is formed inside the kernel, with no index arithmetic on the host or in
    separate launches.  Returns ``[n, D]``.

    ``labels`` (one per slot): a slot whose label equals ``ignore_index`` is a padded prediction slot.
    It still receives its row in the forward, but it is a constant to autograd: the backward drops its
    incoming gradient, so a padded slot that points at a row a valid slot also uses (padding
    conventionally points at position 0) cannot disturb that row's gradient.

    The positions of the VALID slots must be unique within a batch: the backward stores each slot's
    gradient into its row (zero fill, then plain stores: no atomics, no sort), so two valid slots on
    one row would keep only one of the two gradients."""
    per_seq = seq_len = 0
    if h.dim() == 3:
        if positions.dim() != 2 or positions.shape[0] != h.shape[0]:
            raise ValueError("gather_rows: h [B, S, D] takes positions [B, P]")
        per_seq, seq_len = positions.shape[1], h.shape[1]
        h = h.reshape(-1, h.shape[-1])
    elif h.dim() != 2 or positions.dim() != 1:
        raise ValueError("gather_rows: h [R, D] takes positions [n]")
    if labels is not None:
        labels = labels.reshape(-1)
        if labels.numel() != positions.numel():
            raise ValueError("gather_rows: one label per position")
    if _lib.use_native(h) and h.shape[1] % 8 == 0 and h.dtype in (torch.bfloat16, torch.float32):
        from . import _native_mlm
        return _native_mlm.gather_rows(h, positions, labels, ignore_index, per_seq, seq_len)
    pos = positions
    if per_seq:
        pos = positions + torch.arange(positions.shape[0], device=positions.device)[:, None] * seq_len
    out = h.index_select(0, pos.reshape(-1))
    if labels is not None:
        out = torch.where((labels != ignore_index)[:, None], out, out.detach())
    return out


def linear_cross_entropy(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor],
                         labels: torch.Tensor, ignore_index: int = -100, return_logits: bool = False,
                         defer_weight_ready: bool = False):
    """Mean cross-entropy of ``x W^T + b`` (``x [..., K]``, ``weight [V, K]``) against ``labels`` over
    the rows whose label is not ``ignore_index`` (0 when there is none, see ``cross_entropy``).
    Returns the fp32 scalar loss; with ``return_logits`` also the ``[M, V]`` logits (detached).

    ``defer_weight_ready``: ``weight`` is also an embedding table of the same graph (tied decoder).
    The head then adds its share to the weight's gradient slot without reporting the slot to the
    gradient reducer; the embedding backward, which runs last, reports it once both shares are in."""
    if _lib.use_native(x):
        from . import _native_mlm
        if _native_mlm.head_ok(x, weight, bias):
            return _native_mlm.linear_cross_entropy(x, weight, bias, labels, ignore_index, return_logits,
                                                    defer_weight_ready)
    from .linear import linear
    logits = linear(x.reshape(-1, x.shape[-1]), weight, bias)
    loss = cross_entropy(logits, labels.reshape(-1), ignore_index=ignore_index)
    return (loss, logits.detach()) if return_logits else loss
