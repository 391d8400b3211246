"""An independent reference for the RMSNorm, RoPE + GQA pack and SwiGLU kernels (a helper, not a test).

Device-agnostic torch written out from the formulas, nothing imported from ``ops/``.  As in
``norm_oracle.py`` each reference runs at two precisions:

``dtype=torch.float64``  the oracle: exact arithmetic on the (already rounded) inputs.
``dtype=torch.float32``  the emulation: the precision the kernels are entitled to -- fp32 arithmetic,
                         every stored tensor rounded once to the dtype of the input, fp32 side outputs
                         (``rstd``) left in fp32.
"""
from __future__ import annotations

from types import SimpleNamespace

import torch


def _rounder(store_dtype, dtype):
    if dtype == torch.float64:
        return lambda t: t
    return lambda t: t.to(store_dtype)


def table_ref(n_positions: int, theta: float, head_dim: int = 64) -> torch.Tensor:
    """fp64 ``[n, head_dim]`` rows ``[cos | sin]`` of ``pos * inv_freq``, ``inv_freq`` the fp32 values
    ``theta^(-2i/head_dim)`` (the frequencies ARE fp32 numbers in HF; the angle and sin / cos are exact)."""
    inv_freq = (1.0 / (theta ** (torch.arange(0, head_dim, 2, dtype=torch.int64).float() / head_dim))).double()
    ang = torch.arange(n_positions, dtype=torch.float64)[:, None] * inv_freq[None, :]
    return torch.cat([ang.cos(), ang.sin()], 1)


def rms_ref(x, w, eps, dy, add, dtype):
    """y = x * rstd * w, rstd = 1 / sqrt(mean(x^2) + eps) over the last axis, and the backward:
    g = dy * w, dx = rstd * (g - xhat * mean(g * xhat)) (+ add), dw = sum_rows(dy * xhat)."""
    rnd = _rounder(x.dtype, dtype)
    H = x.shape[-1]
    xf, wf, dyf = x.to(dtype), w.to(dtype), dy.to(dtype)
    rstd = 1.0 / torch.sqrt((xf * xf).sum(-1, keepdim=True) / H + eps)
    xh = xf * rstd
    y = xh * wf
    g = dyf * wf
    m = (g * xh).sum(-1, keepdim=True) / H
    dx = rstd * (g - xh * m)
    if add is not None:
        dx = dx + add.to(dtype).reshape(dx.shape)
    dw_raw = (dyf * xh).reshape(-1, H).sum(0)
    return SimpleNamespace(y=rnd(y), rstd=rstd.reshape(-1), dx=rnd(dx), dw=rnd(dw_raw))


def rope_ref(qkv, table, H, Hkv, dout, dtype):
    """``qkv [B, S, (H + 2 Hkv) D]`` -> ``out [B, S, 3 H D]`` and, from ``dout`` of that shape, ``din``.
    Written per head with explicit indices: query head h reads input head h; key / value head g lands in
    query-head slots g G .. g G + G - 1; the backward sums those slots and un-rotates the sum."""
    rnd = _rounder(qkv.dtype, dtype)
    B, S, W = qkv.shape
    D = W // (H + 2 * Hkv)
    half, G = D // 2, H // Hkv
    x = qkv.to(dtype).reshape(B, S, H + 2 * Hkv, D)
    cos = table[:S, :half].to(dtype).reshape(1, S, half)
    sin = table[:S, half:].to(dtype).reshape(1, S, half)

    def rot(t, sgn):
        a, b = t[..., :half], t[..., half:]
        return torch.cat([a * cos - sgn * b * sin, b * cos + sgn * a * sin], -1)

    out = torch.zeros(B, S, 3, H, D, dtype=dtype, device=qkv.device)
    for h in range(H):
        out[:, :, 0, h] = rot(x[:, :, h], 1.0)
    for g in range(Hkv):
        kr = rot(x[:, :, H + g], 1.0)
        for r in range(G):
            out[:, :, 1, g * G + r] = kr
            out[:, :, 2, g * G + r] = x[:, :, H + Hkv + g]
    din = None
    if dout is not None:
        d = dout.to(dtype).reshape(B, S, 3, H, D)
        din = torch.zeros(B, S, H + 2 * Hkv, D, dtype=dtype, device=qkv.device)
        for h in range(H):
            din[:, :, h] = rot(d[:, :, 0, h], -1.0)
        for g in range(Hkv):
            dk = d[:, :, 1, g * G]
            dv = d[:, :, 2, g * G]
            for r in range(1, G):
                dk = dk + d[:, :, 1, g * G + r]
                dv = dv + d[:, :, 2, g * G + r]
            din[:, :, H + g] = rot(dk, -1.0)
            din[:, :, H + Hkv + g] = dv
        din = rnd(din.reshape(B, S, W))
    return SimpleNamespace(out=rnd(out.reshape(B, S, 3 * H * D)), din=din)


def swiglu_ref(gu, dz, dtype):
    """z = gate * sig(gate) * up; dgate = dz * up * sig * (1 + gate * (1 - sig)); dup = dz * gate * sig."""
    rnd = _rounder(gu.dtype, dtype)
    I = gu.shape[-1] // 2
    g, u = gu[..., :I].to(dtype), gu[..., I:].to(dtype)
    sig = 1.0 / (1.0 + torch.exp(-g))
    z = g * sig * u
    dgu = None
    if dz is not None:
        d = dz.to(dtype)
        dgu = rnd(torch.cat([d * u * sig * (1.0 + g * (1.0 - sig)), d * (g * sig)], -1))
    return SimpleNamespace(z=rnd(z), dgu=dgu)
