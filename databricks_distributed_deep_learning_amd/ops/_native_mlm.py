"""Masked-LM bindings (csrc/kernels/mlm_loss.hip): cross-entropy with ignored targets, the
masked-position row gather / scatter and the fused vocabulary head.

The loss is split into a forward kernel (row log-sum-exp + row loss, then a fixed-order mean over
the valid rows that also leaves 1 / n_valid on the device) and a backward kernel that writes
``(softmax - onehot) * g / n_valid`` in one read and one write of the logits -- in place for the
fused head, whose [tokens, roundup(V, 8)] logits buffer is the only vocabulary-wide tensor it ever
allocates.
"""
from __future__ import annotations

import torch

from . import _native_elementwise as E
from ._lib import I, L, P, call, dcode, grad_ready, grad_sink, p, register
from ._native_gemm import MODE_NN, MODE_NT, MODE_TN, gemm
from ._native_linear import _padded

register({
    "ddl_ce_lse": [I, P, L, L, I, P, L, P, P, P, P, P],
    "ddl_ce_bwd": [I, P, L, L, I, P, L, P, P, P, P, P],
    "ddl_gather_rows": [I, P, P, P, L, L, I, L, L, P],
    "ddl_scatter_rows": [I, P, P, P, L, P, L, L, I, L, L, P],
})


def _lse(y: torch.Tensor, M: int, ld: int, C: int, labels: torch.Tensor, ignore_index: int):
    """(loss, lse [M], 1 / n_valid) of the rows of ``y`` ([M, ld], columns [0, C) valid)."""
    dev = y.device
    lse = torch.empty(M, dtype=torch.float32, device=dev)
    row = torch.empty(M, dtype=torch.float32, device=dev)
    loss = torch.empty((), dtype=torch.float32, device=dev)
    inv_n = torch.empty(1, dtype=torch.float32, device=dev)
    call("ddl_ce_lse", dcode(y), p(y), M, ld, C, p(labels), ignore_index, p(lse), p(row), p(loss), p(inv_n))
    return loss, lse, inv_n


def _bwd(y, M, ld, C, labels, ignore_index, lse, g, inv_n, dst) -> None:
    call("ddl_ce_bwd", dcode(y), p(y), M, ld, C, p(labels), ignore_index, p(lse), p(g), p(inv_n), p(dst))


class _CEIgnore(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, labels, ignore_index):
        M, C = logits.shape
        ld = (C + 7) // 8 * 8
        x = logits.contiguous()
        if ld != C or x.data_ptr() % 16:
            # rows padded to 8 columns (pad columns are never read as logits)
            x = E.copy2d(torch.empty(M, ld, dtype=x.dtype, device=x.device), x, ld, M, ld, C, M, C)
        labels = labels.contiguous().to(torch.int64)
        loss, lse, inv_n = _lse(x, M, ld, C, labels, ignore_index)
        ctx.save_for_backward(x, labels, lse, inv_n)
        ctx.dims = (M, C, ld, ignore_index)
        return loss

    @staticmethod
    def backward(ctx, g):
        x, labels, lse, inv_n = ctx.saved_tensors
        M, C, ld, ignore_index = ctx.dims
        g = g.contiguous().float()
        dl = torch.empty_like(x)          # the caller owns the logits: a fresh buffer
        _bwd(x, M, ld, C, labels, ignore_index, lse, g, inv_n, dl)
        if ld != C:
            dl = E.copy2d(torch.empty(M, C, dtype=dl.dtype, device=dl.device), dl, C, M, C, ld, M, C)
        return dl, None, None


def cross_entropy_ignore(logits, labels, ignore_index: int):
    return _CEIgnore.apply(logits, labels, int(ignore_index))


class _GatherRows(torch.autograd.Function):
    @staticmethod
    def forward(ctx, h, positions, labels, ignore_index, P_, S_):
        h = h.contiguous()
        R, D = h.shape
        pos = positions.contiguous().to(torch.int64)
        n = pos.numel()
        out = torch.empty(n, D, dtype=h.dtype, device=h.device)
        call("ddl_gather_rows", dcode(h), p(h), p(pos), p(out), n, R, D, P_, S_)
        lab = None if labels is None else labels.contiguous().to(torch.int64)
        ctx.save_for_backward(pos, lab)
        ctx.dims = (n, R, D, int(ignore_index), P_, S_)
        return out

    @staticmethod
    def backward(ctx, dy):
        pos, lab = ctx.saved_tensors
        n, R, D, ignore_index, P_, S_ = ctx.dims
        dy = dy.contiguous()
        dh = torch.empty(R, D, dtype=dy.dtype, device=dy.device)
        call("ddl_scatter_rows", dcode(dy), p(dy), p(pos), p(lab), ignore_index, p(dh), n, R, D, P_, S_)
        return dh, None, None, None, None, None


def gather_rows(h2d, positions, labels, ignore_index, per_seq: int = 0, seq_len: int = 0):
    return _GatherRows.apply(h2d, positions, labels, ignore_index, int(per_seq), int(seq_len))


def head_ok(x, w, b) -> bool:
    return (x.dtype == torch.bfloat16 and w.dtype == torch.bfloat16 and (b is None or b.dtype == w.dtype)
            and x.shape[-1] % 8 == 0 and x.numel() > 0 and w.dim() == 2)


class _LinearCE(torch.autograd.Function):
    """loss = CE(x W^T + b, labels) with the logits kept in ONE [M, roundup(V, 8)] buffer: written by
    the NT GEMM, read once by ``ddl_ce_lse``, overwritten by ``ddl_ce_bwd`` with their own gradient,
    which the dgrad (NN) and wgrad (TN) GEMMs and the bias column sums then read as is (its pad
    columns are exact zeros).  The in-place backward makes the graph single-use."""

    @staticmethod
    def forward(ctx, x, w, b, labels, ignore_index, return_logits, defer_weight_ready):
        K, V = x.shape[-1], w.shape[0]
        Np = (V + 7) // 8 * 8
        x2 = x.reshape(-1, K)
        if not x2.is_contiguous():
            x2 = x2.contiguous()
        M = x2.shape[0]
        if Np != V:
            wp, bp = _padded(w, b, Np)
        else:
            wp, bp = w.contiguous(), b
        y = torch.empty(M, Np, dtype=x.dtype, device=x.device)
        gemm(MODE_NT, x2, K, wp, K, y, Np, M, Np, K, bias=bp)
        labels = labels.reshape(-1).contiguous().to(torch.int64)
        loss, lse, inv_n = _lse(y, M, Np, V, labels, ignore_index)
        ctx.save_for_backward(x2, wp, y, labels, lse, inv_n)
        ctx.w_param, ctx.b_param = w, b
        ctx.dims = (M, K, V, Np, ignore_index)
        ctx.xshape = x.shape
        ctx.defer_weight_ready = defer_weight_ready
        ctx.done = False
        if not return_logits:
            ctx.inplace = True
            return loss
        # the caller keeps these logits: a copy when the buffer is padded, else the buffer itself,
        # which the backward then leaves alone
        ctx.inplace = Np != V
        logits = y if Np == V else E.copy2d(torch.empty(M, V, dtype=y.dtype, device=y.device), y, V, M, V, Np, M, V)
        ctx.mark_non_differentiable(logits)
        return loss, logits

    @staticmethod
    def backward(ctx, g, *_):
        if ctx.done and ctx.inplace:
            raise RuntimeError("linear_cross_entropy: the backward overwrites the logits in place and "
                               "runs once per forward")
        ctx.done = True
        x2, wp, y, labels, lse, inv_n = ctx.saved_tensors
        M, K, V, Np, ignore_index = ctx.dims
        g = g.contiguous().float()
        dl = y if ctx.inplace else torch.empty_like(y)
        _bwd(y, M, Np, V, labels, ignore_index, lse, g, inv_n, dl)
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty(M, K, dtype=x2.dtype, device=x2.device)
            gemm(MODE_NN, dl, Np, wp, K, dx, K, M, K, Np)
            dx = dx.view(ctx.xshape)
        if ctx.needs_input_grad[1]:
            sink = grad_sink(ctx.w_param)
            if sink is not None and sink.dtype != wp.dtype:
                sink = None
            if Np == V and sink is not None:
                gemm(MODE_TN, dl, Np, x2, K, sink, K, V, K, M, accumulate=True)
            else:
                dwp = torch.empty(Np, K, dtype=wp.dtype, device=wp.device)
                gemm(MODE_TN, dl, Np, x2, K, dwp, K, Np, K, M)
                if sink is not None:
                    E.add_into(sink.view(-1), dwp[:V].reshape(-1))     # rows 0..V-1: contiguous
                else:
                    dw = dwp[:V]
            # a weight tied to an embedding table: the embedding backward, the last producer of this
            # gradient in the step, reports it (parallel/ddp.py: one report, after both shares)
            if sink is not None and not ctx.defer_weight_ready:
                grad_ready(ctx.w_param)
        if ctx.b_param is not None and ctx.needs_input_grad[2]:
            dbp = torch.empty(Np, dtype=wp.dtype, device=wp.device)
            E.colsum(dl, dbp)
            sink = grad_sink(ctx.b_param)
            if sink is not None and sink.dtype == dbp.dtype:
                E.add_into(sink.view(-1), dbp[:V])
                grad_ready(ctx.b_param)
            else:
                db = dbp[:V]
        return dx, dw, db, None, None, None, None


def linear_cross_entropy(x, w, b, labels, ignore_index, return_logits, defer_weight_ready):
    return _LinearCE.apply(x, w, b, labels, int(ignore_index), bool(return_logits), bool(defer_weight_ready))
