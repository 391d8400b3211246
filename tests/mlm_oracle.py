"""An independent reference for the kernels of ``csrc/kernels/mlm_loss.hip``: cross-entropy with ignored
targets (row log-sum-exp, the mean over the valid rows, the scaled gradient), the fused vocabulary head
around it, and the row gather / scatter at the masked positions.

Everything here is device-agnostic torch written out from the formulas: no ``F.cross_entropy``, nothing
from ``ops/``.  Each reference takes a ``dtype``, as in ``norm_oracle`` / ``elementwise_oracle``:

``torch.float64``  the oracle: exact arithmetic on the (already rounded) inputs, nothing rounded.
``torch.float32``  the emulation: fp32 arithmetic, every stored tensor rounded once to the logits' dtype,
                   fp32 side outputs (lse, row losses, loss, 1 / n_valid) left in fp32.

The bound is ``norm_oracle.bound``.
"""
from __future__ import annotations

import math
from types import SimpleNamespace

import torch

from elementwise_oracle import _softmax  # noqa: F401  (shared, not copied)
from norm_oracle import _rounder, bound  # noqa: F401


def valid_rows(labels, ignore_index: int, C: int):
    """A row takes part when its label is not ``ignore_index`` and lies in [0, C)."""
    return (labels != ignore_index) & (labels >= 0) & (labels < C)


LOG2E_F32 = float(torch.tensor(math.log2(math.e), dtype=torch.float32))


def _exp_bwd(a, dtype):
    """``exp(a)`` of the backward.  The emulation carries one named rounding more than ``torch.exp``:
    ``ce_bwd_k`` takes ``__expf(a)``, which is ``exp2(a * log2(e))`` with the product rounded to fp32 --
    at a = -20 that product alone is 1e-6 relative, next to the 1e-6 of rounding ``x - lse``."""
    return torch.exp(a) if dtype == torch.float64 else torch.exp2(a * LOG2E_F32)


def ce_ignore_ref(logits, labels, ignore_index: int, upstream: float, dtype, store_dtype=None):
    """Mean cross-entropy over the valid rows of ``logits [M, C]`` and its gradient.

    The emulation's mean is the sum of its fp32 row losses, taken exactly and rounded once: the row
    losses are what fp32 side outputs lose, and a mean over them is entitled to one more rounding.  (An
    fp32 running sum adds roundings of its own, which depend on the order of the rows and as often
    cancel the row losses' errors as add to them: no yardstick for a scalar.)

    Returns lse and row_loss per row (meaningful on ``valid`` rows only), valid, n_valid,
    ``loss = sum(valid row losses) / n_valid`` (0 when there is none), ``inv_n = 1 / n_valid`` (0 when
    there is none) and ``dlogits = (exp(x - lse) - onehot) * (upstream * inv_n)`` with exact zeros on
    the other rows.  The emulation forms ``upstream * inv_n`` first, in fp32, and rounds the product of
    the two factors once to ``store_dtype`` (default: the dtype of ``logits``)."""
    rnd = _rounder(store_dtype or logits.dtype, dtype)
    x = logits.to(dtype)
    M, C = x.shape
    valid = valid_rows(labels, ignore_index, C)
    n_valid = int(valid.sum())
    _, m, s = _softmax(x)
    lse = (m + torch.log(s)).squeeze(-1)
    col = torch.where(valid, labels, torch.zeros_like(labels)).view(-1, 1)
    row_loss = lse - x.gather(1, col).squeeze(1)
    zero = torch.zeros((), dtype=dtype, device=x.device)
    one = torch.ones((), dtype=dtype, device=x.device)
    inv_n = one / n_valid if n_valid else zero
    loss = (torch.where(valid, row_loss, zero).double().sum() / n_valid).to(dtype) if n_valid else zero
    scale = torch.tensor(upstream, dtype=torch.float32, device=x.device).to(dtype) * inv_n
    onehot = torch.zeros_like(x).scatter_(1, col, 1.0)
    dl = torch.where(valid.view(-1, 1), (_exp_bwd(x - lse.view(-1, 1), dtype) - onehot) * scale, zero)
    return SimpleNamespace(lse=lse, row_loss=row_loss, valid=valid, n_valid=n_valid, loss=loss, inv_n=inv_n,
                           dlogits=rnd(dl))


def head_ref(x, w, b, labels, ignore_index: int, upstream: float, dtype):
    """``logits = x W^T + b`` (``b`` may be None), ``ce_ignore_ref`` on them, and ``dx = dl W``,
    ``dW = dl^T x``, ``db = colsum(dl)``.  The emulation rounds the logits to the dtype of ``x`` before
    the loss reads them, and its GEMMs and column sums read the rounded ``dl``; each result is rounded
    once."""
    st = x.dtype
    rnd = _rounder(st, dtype)
    xf, wf = x.to(dtype), w.to(dtype)
    logits = xf @ wf.t()
    if b is not None:
        logits = logits + b.to(dtype)
    logits = rnd(logits)
    ce = ce_ignore_ref(logits, labels, ignore_index, upstream, dtype, store_dtype=st)
    dl = ce.dlogits.to(dtype)
    return SimpleNamespace(logits=logits, ce=ce, loss=ce.loss, dx=rnd(dl @ wf), dW=rnd(dl.t() @ xf),
                           db=None if b is None else rnd(dl.sum(0)))


def slot_rows(pos, P: int = 0, S: int = 0):
    """The flat row of every slot: ``pos[t]``, or ``(t // P) * S + pos[t]`` for positions per sequence."""
    pos = pos.reshape(-1)
    if P > 0:
        pos = pos + (torch.arange(pos.numel(), device=pos.device) // P) * S
    return pos


def gather_ref(h, pos, P: int = 0, S: int = 0):
    """``out[t] = h[row(t)]`` for ``h [R, D]``; a row outside [0, R) gives zeros."""
    R = h.shape[0]
    rows = slot_rows(pos, P, S)
    ok = (rows >= 0) & (rows < R)
    out = torch.zeros(rows.numel(), h.shape[1], dtype=h.dtype, device=h.device)
    out[ok] = h[rows[ok]]
    return out


def scatter_ref(dy, pos, labels, ignore_index: int, R: int, P: int = 0, S: int = 0):
    """``dh [R, D]``: zeros, then ``dh[row(t)] = dy[t]`` for every slot whose label is not
    ``ignore_index`` (``labels=None``: every slot) and whose row lies in [0, R)."""
    rows = slot_rows(pos, P, S)
    ok = (rows >= 0) & (rows < R)
    if labels is not None:
        ok = ok & (labels.reshape(-1) != ignore_index)
    dh = torch.zeros(R, dy.shape[1], dtype=dy.dtype, device=dy.device)
    dh[rows[ok]] = dy[ok]
    return dh
