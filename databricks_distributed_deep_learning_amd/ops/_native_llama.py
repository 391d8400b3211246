"""Autograd bindings for the HIP RMSNorm / RoPE + GQA pack / SwiGLU kernels (csrc/kernels/llama.hip).
All of them bf16 only."""
from __future__ import annotations

import torch

from . import _lib
from ._lib import F, I, L, P, call, p

_lib.register({
    "ddl_rmsnorm_supported": [I],
    "ddl_rmsnorm_fwd": [P, P, P, P, L, I, F, P],
    "ddl_rmsnorm_bwd_nblk": [L],
    "ddl_rmsnorm_bwd": [P, P, P, P, P, P, P, P, L, I, P],
    "ddl_rope_qkv_supported": [I, I, I],
    "ddl_rope_qkv_fwd": [P, P, P, L, L, I, I, L, P],
    "ddl_rope_qkv_bwd": [P, P, P, L, L, I, I, L, P],
    # explicit positions (packed rows): the same + pos int32 [B, S]
    "ddl_rope_qkv_pos_fwd": [P, P, P, P, L, L, I, I, L, P],
    "ddl_rope_qkv_pos_bwd": [P, P, P, P, L, L, I, I, L, P],
    "ddl_swiglu_supported": [L, I],
    "ddl_swiglu_fwd": [P, P, L, I, P],
    "ddl_swiglu_bwd": [P, P, P, L, I, P],
})


# ------------------------------------------------------------------ RMSNorm
class _RMSNorm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, eps, grad_from=None):
        ctx.grad_from = grad_from
        x = x.contiguous()
        H = x.shape[-1]
        rows = x.numel() // H
        rstd = torch.empty(rows, dtype=torch.float32, device=x.device)
        y = torch.empty_like(x)
        call("ddl_rmsnorm_fwd", p(x), p(weight), p(y), p(rstd), rows, H, float(eps))
        ctx.save_for_backward(x, weight, rstd)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, weight, rstd = ctx.saved_tensors
        dy = dy.contiguous()
        H = x.shape[-1]
        rows = x.numel() // H
        # x's gradient from its other consumer (the residual branch, handed over by that Linear's
        # backward): added in the same pass, before dx's one rounding
        add = ctx.grad_from.take() if ctx.grad_from is not None else None
        ctx.grad_from = None
        if add is not None:
            add = add.reshape(x.shape)
            if not add.is_contiguous() or add.dtype != x.dtype:
                add = add.contiguous().to(x.dtype)
        dx = torch.empty_like(x)
        dw = torch.empty_like(weight)
        if rows == 0:
            return dx, dw.zero_(), None, None
        nblk = _lib.fn("ddl_rmsnorm_bwd_nblk")(rows)
        part = torch.empty(nblk * H, dtype=torch.float32, device=x.device)
        call("ddl_rmsnorm_bwd", p(dy), p(x), p(weight), p(rstd), p(add), p(dx), p(part), p(dw), rows, H)
        return dx, dw, None, None


def rms_norm_supported(x: torch.Tensor) -> bool:
    return x.dim() >= 1 and bool(_lib.fn("ddl_rmsnorm_supported")(x.shape[-1]))


def rms_norm(x, weight, eps, grad_from=None):
    if weight.dtype != x.dtype:
        weight = weight.to(x.dtype)
    return _RMSNorm.apply(x, weight.contiguous(), eps, grad_from)


# ------------------------------------------------------------------ RoPE + GQA pack
class _RopeQKV(torch.autograd.Function):
    @staticmethod
    def forward(ctx, qkv, table, H, Hkv, positions=None):
        qkv = qkv.contiguous()
        table = table.contiguous()
        B, S, _ = qkv.shape
        out = torch.empty(B, S, 3 * H * 64, dtype=qkv.dtype, device=qkv.device)
        if positions is not None:
            positions = positions.contiguous()
            if B * S:
                call("ddl_rope_qkv_pos_fwd", p(qkv), p(table), p(out), p(positions), B, S, H, Hkv, table.shape[0])
        elif B * S:
            call("ddl_rope_qkv_fwd", p(qkv), p(table), p(out), B, S, H, Hkv, table.shape[0])
        ctx.dims = (B, S, H, Hkv)
        ctx.save_for_backward(table, positions)
        return out

    @staticmethod
    def backward(ctx, dout):
        table, positions = ctx.saved_tensors
        B, S, H, Hkv = ctx.dims
        dout = dout.contiguous()
        din = torch.empty(B, S, (H + 2 * Hkv) * 64, dtype=dout.dtype, device=dout.device)
        if positions is not None:
            if B * S:
                call("ddl_rope_qkv_pos_bwd", p(dout), p(table), p(din), p(positions), B, S, H, Hkv, table.shape[0])
        elif B * S:
            call("ddl_rope_qkv_bwd", p(dout), p(table), p(din), B, S, H, Hkv, table.shape[0])
        return din, None, None, None, None


def rope_qkv_supported(H: int, Hkv: int, head_dim: int) -> bool:
    return bool(_lib.fn("ddl_rope_qkv_supported")(H, Hkv, head_dim))


def rope_qkv(qkv, table, H, Hkv, positions=None):
    if positions is None:
        return _RopeQKV.apply(qkv, table, H, Hkv)
    return _RopeQKV.apply(qkv, table, H, Hkv, positions)


# ------------------------------------------------------------------ SwiGLU
class _SwiGLU(torch.autograd.Function):
    @staticmethod
    def forward(ctx, gu):
        gu = gu.contiguous()
        I2 = gu.shape[-1]
        rows = gu.numel() // I2
        z = torch.empty(*gu.shape[:-1], I2 // 2, dtype=gu.dtype, device=gu.device)
        call("ddl_swiglu_fwd", p(gu), p(z), rows, I2 // 2)
        ctx.save_for_backward(gu)
        return z

    @staticmethod
    def backward(ctx, dz):
        gu, = ctx.saved_tensors
        dz = dz.contiguous()
        I2 = gu.shape[-1]
        dgu = torch.empty_like(gu)
        call("ddl_swiglu_bwd", p(gu), p(dz), p(dgu), gu.numel() // I2, I2 // 2)
        return dgu


def swiglu_supported(gu: torch.Tensor) -> bool:
    I2 = gu.shape[-1]
    return gu.dim() >= 1 and I2 % 2 == 0 and I2 > 0 and \
        bool(_lib.fn("ddl_swiglu_supported")(gu.numel() // I2, I2 // 2))


def swiglu(gu):
    return _SwiGLU.apply(gu)
