"""Softmax cross-entropy (K10) and inference softmax + top-k (K11).

``softmax_topk`` reproduces the reference's post-processing: softmax over the
1000 logits then the 5 best classes (``notebooks/cv/onnx_experiments.py:85-100``
for ORT, ``:174-178`` for PyTorch).
"""
from __future__ import annotations

from typing import Optional

import torch
import torch.nn.functional as F

from . import _lib


def cross_entropy(logits: torch.Tensor, labels: torch.Tensor, ignore_index: Optional[int] = None) -> torch.Tensor:
    """Mean softmax cross-entropy, fp32 math, returns an fp32 scalar.

    ``ignore_index``: rows whose label equals it take no part (the mean is over the other rows).
    The one deliberate difference from ``F.cross_entropy``: when EVERY row is ignored the loss is 0
    with a zero gradient, not NaN -- a NaN here would go straight into the fp32 master weights.
    ``None`` (default) is the path without ignored targets, unchanged."""
    if ignore_index is None:
        if _lib.use_native(logits):
            from . import _native_loss
            return _native_loss.cross_entropy(logits, labels)
        return F.cross_entropy(logits.float(), labels)
    if _lib.use_native(logits) and logits.dim() == 2 and logits.dtype in (torch.bfloat16, torch.float32) \
            and logits.numel() > 0:
        from . import _native_mlm
        return _native_mlm.cross_entropy_ignore(logits, labels, ignore_index)
    x = logits if logits.dtype == torch.float64 else logits.float()
    total = F.cross_entropy(x, labels, ignore_index=ignore_index, reduction="sum")
    return total / (labels != ignore_index).sum().clamp(min=1)


def softmax_topk(logits: torch.Tensor, k: int = 5):
    """Returns (probabilities, top-k values, top-k indices) over the last axis.

    On the GPU one HIP kernel does both (softmax_topk_k in elementwise.hip: one block
    per row, probabilities staged in LDS, k block-wide argmax rounds)."""
    if _lib.use_native(logits) and logits.dtype in (torch.bfloat16, torch.float32) and \
            logits.shape[-1] <= 4096 and 1 <= k <= logits.shape[-1]:
        from ._lib import call, dcode, p as ptr
        x = logits.contiguous()
        C = x.shape[-1]
        B = x.numel() // C
        probs = torch.empty(B, C, dtype=torch.float32, device=x.device)
        v = torch.empty(B, k, dtype=torch.float32, device=x.device)
        i = torch.empty(B, k, dtype=torch.int64, device=x.device)
        call("ddl_softmax_topk", dcode(x), ptr(x), B, C, k, ptr(probs), ptr(v), ptr(i))
        lead = x.shape[:-1]
        return probs.view(*lead, C), v.view(*lead, k), i.view(*lead, k)
    p = torch.softmax(logits.float(), dim=-1)
    v, i = torch.topk(p, k, dim=-1)
    return p, v, i
