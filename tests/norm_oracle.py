"""An independent reference for the LayerNorm / BatchNorm kernels, and the bound the oracle tests share.

Everything here is device-agnostic torch written out from the formulas: no ``F.layer_norm``, no
``F.batch_norm``, nothing from ``ops/norm.py``.  Each reference runs at two precisions:

``dtype=torch.float64``  the oracle (``ref64``): exact arithmetic on the (already rounded) inputs.
``dtype=torch.float32``  the emulation (``emu``): the precision the kernels are entitled to -- fp32
                         arithmetic and statistics, every stored tensor rounded once to the dtype of
                         ``x``, fp32 side outputs (mean, rstd, column sums) left in fp32.  The column
                         sums of dx are taken over the *rounded* dx, as ``ln_bwd_k`` takes them.

``bound`` then allows a kernel ``M`` times the emulation's own distance from the oracle plus half an ulp
of the output format, in the max and in the rms norm.
"""
from __future__ import annotations

import math
from types import SimpleNamespace
from typing import Optional

import torch

from test_kernels_gpu import _hash_keep  # noqa: F401  (the dropout keep mask: not re-derived here)


# ---------------------------------------------------------------------------- helpers
def _rounder(store_dtype, dtype):
    """Rounds a ``dtype`` tensor to the stored format (emulation) or leaves it alone (oracle)."""
    if dtype == torch.float64:
        return lambda t: t
    return lambda t: t.to(store_dtype)


def keep_mask(seed: int, shape, p: float, device) -> torch.Tensor:
    """The keep bits the fused-dropout kernels draw for ``seed`` over a tensor of ``shape``."""
    n = 1
    for s in shape:
        n *= s
    return _hash_keep(seed, n, p).to(device).view(*shape)


# ---------------------------------------------------------------------------- LayerNorm
def ln_ref(x, g, b, eps, res, keep, p, dy, add, dtype):
    """LayerNorm over the last axis of ``h = x * keep / (1 - p) + res`` and its backward.

    ``res``: None, the shape of ``x``, or one leading row block (``[1, S, H]`` against ``[B, S, H]``);
    ``keep``: None or a bool tensor (fused dropout with probability ``p``); ``add``: None or the
    gradient of ``x`` from its other consumer.  Returns y, mean, rstd (per row), dx (through the mask,
    plus ``add``), dres (not masked; summed over the batch for a broadcast residual), dgamma, dbeta
    and dxsum, the column sums of dx.  ``dgamma_raw`` / ``dbeta_raw`` are the sums before their one
    rounding (what an accumulating gradient slot adds to its old value)."""
    st = x.dtype
    rnd = _rounder(st, dtype)
    H = x.shape[-1]
    xf, gf, bf, dyf = x.to(dtype), g.to(dtype), b.to(dtype), dy.to(dtype)
    kf = None if keep is None else keep.to(dtype) / (1.0 - p)
    h = xf if kf is None else xf * kf
    if res is not None:
        h = h + res.to(dtype)
    mean = h.sum(-1, keepdim=True) / H
    c = h - mean
    var = (c * c).sum(-1, keepdim=True) / H
    rstd = 1.0 / torch.sqrt(var + eps)
    xh = c * rstd
    y = xh * gf + bf
    gy = dyf * gf
    m1 = gy.sum(-1, keepdim=True) / H
    m2 = (gy * xh).sum(-1, keepdim=True) / H
    dh = rstd * (gy - m1 - xh * m2)                    # gradient of h
    dx = dh if kf is None else dh * kf
    if add is not None:
        dx = dx + add.to(dtype).reshape(dx.shape)
    dx = rnd(dx)
    dres = None
    if res is not None:
        dres = rnd(dh)
        if res.shape != x.shape:                       # broadcast over the leading dimension
            dres = rnd(dres.to(dtype).reshape(-1, *res.shape[1:]).sum(0, keepdim=True).reshape(res.shape))
    dgamma_raw = (dyf * xh).reshape(-1, H).sum(0)
    dbeta_raw = dyf.reshape(-1, H).sum(0)
    dxsum = dx.to(dtype).reshape(-1, H).sum(0)
    return SimpleNamespace(y=rnd(y), mean=mean.reshape(-1), rstd=rstd.reshape(-1), dx=dx, dres=dres,
                           dgamma=rnd(dgamma_raw), dbeta=rnd(dbeta_raw), dgamma_raw=dgamma_raw,
                           dbeta_raw=dbeta_raw, dxsum=dxsum)


# ---------------------------------------------------------------------------- BatchNorm
def bn_ref(x, g, b, eps, relu, res, dy, dtype):
    """Training-mode BatchNorm over every axis but the last (+ residual) (+ ReLU) and its backward,
    two-pass statistics.  ``relu``: False, True (the mask is this run's own ``y > 0``) or a bool
    tensor of the shape of ``x`` that IS the mask.  Returns y, mean, var (biased), var_unbiased, dx,
    dres, dgamma, dbeta, z (the pre-activation) and mask."""
    st = x.dtype
    rnd = _rounder(st, dtype)
    C = x.shape[-1]
    xf = x.to(dtype).reshape(-1, C)
    M = xf.shape[0]
    gf, bf, dyf = g.to(dtype), b.to(dtype), dy.to(dtype).reshape(-1, C)
    mean = xf.sum(0) / M
    c = xf - mean
    var = (c * c).sum(0) / M
    var_u = var * (M / (M - 1.0)) if M > 1 else var
    invstd = 1.0 / torch.sqrt(var + eps)
    xh = c * invstd
    z = xh * gf + bf
    if res is not None:
        z = z + res.to(dtype).reshape(-1, C)
    if relu is False:
        y, mask = rnd(z), None
    else:
        y = rnd(torch.clamp_min(z, 0.0))
        mask = (y > 0) if relu is True else relu.reshape(-1, C)
    dz = dyf if mask is None else dyf * mask.to(dtype)
    dbeta_raw = dz.sum(0)
    dgamma_raw = (dz * xh).sum(0)
    dx = gf * invstd * (dz - dbeta_raw / M - xh * (dgamma_raw / M))
    return SimpleNamespace(y=y.reshape(x.shape), mean=mean, var=var, var_unbiased=var_u,
                           dx=rnd(dx).reshape(x.shape), dres=None if res is None else rnd(dz).reshape(x.shape),
                           dgamma=rnd(dgamma_raw), dbeta=rnd(dbeta_raw), z=z.reshape(x.shape),
                           mask=None if mask is None else mask.reshape(x.shape))


def bn_running(mean, var_unbiased, momentum, dtype, rm0=0.0, rv0=1.0):
    """The running statistics after one training step from (rm0, rv0), in ``dtype``."""
    m = torch.tensor(momentum, dtype=torch.float32).to(dtype)       # the kernels take a float momentum
    return (1 - m) * rm0 + m * mean.to(dtype), (1 - m) * rv0 + m * var_unbiased.to(dtype)


def bn_eval_ref(x, g, b, rm, rv, eps, relu, res, dtype):
    """BatchNorm with frozen statistics (+ residual) (+ ReLU): y and the pre-activation z."""
    rnd = _rounder(x.dtype, dtype)
    xf = x.to(dtype)
    scale = g.to(dtype) / torch.sqrt(rv.to(dtype) + eps)
    z = (xf - rm.to(dtype)) * scale + b.to(dtype)
    if res is not None:
        z = z + res.to(dtype)
    y = torch.clamp_min(z, 0.0) if relu else z
    return SimpleNamespace(y=rnd(y), z=z)


# ---------------------------------------------------------------------------- the bound
_MANT = {torch.bfloat16: 8, torch.float32: 24, torch.float64: 53}


def half_ulp(v: float, dtype) -> float:
    """Half the spacing of ``dtype`` numbers at ``|v|``."""
    v = abs(float(v))
    return 0.0 if not v > 0 else 2.0 ** (math.floor(math.log2(v)) - _MANT[dtype])


def _rms(t: torch.Tensor) -> float:
    return float(t.pow(2).mean().sqrt())


def figures(got, ref64, emu, dtype):
    """(kernel error, emulation error, half-ulp term) in the max form and in the rms form."""
    ref = ref64.double()
    d, e = (got.double() - ref).abs(), (emu.double() - ref).abs()
    return ((float(d.max()), float(e.max()), half_ulp(float(ref.abs().max()), dtype)),
            (_rms(d), _rms(e), half_ulp(_rms(ref), dtype)))


def bound(got, ref64, emu, dtype, M, label: str = "", fails: Optional[list] = None):
    """Asserts, per tensor,
        max|got - ref64| <= M * max|emu - ref64| + 1/2 ulp_dtype(max|ref64|)
        rms(got - ref64) <= M * rms(emu - ref64) + 1/2 ulp_dtype(rms(ref64))
    after printing both ratios ((error - ulp term) / emulation error).  With ``fails`` the messages
    are appended there instead, so that a case prints every tensor before it fails.  Returns the two
    ratios."""
    assert got.shape == ref64.shape == emu.shape, f"{label}: shapes {tuple(got.shape)} {tuple(ref64.shape)}"
    assert bool(torch.isfinite(got.double()).all()), f"{label}: non-finite values"
    (kmax, emax, hmax), (krms, erms, hrms) = figures(got, ref64, emu, dtype)

    def ratio(k, h, e):
        return (k - h) / e if e > 0 else (0.0 if k <= h else float("inf"))
    rmax, rrms = ratio(kmax, hmax, emax), ratio(krms, hrms, erms)
    print(f"RATIO {label} max={rmax:.3f} rms={rrms:.3f} kmax={kmax:.3e} emax={emax:.3e} hmax={hmax:.3e} "
          f"krms={krms:.3e} erms={erms:.3e} hrms={hrms:.3e}")
    msgs = []
    if not kmax <= M * emax + hmax:
        msgs.append(f"{label}: max err {kmax:.3e} > {M} * {emax:.3e} + {hmax:.3e}")
    if not krms <= M * erms + hrms:
        msgs.append(f"{label}: rms err {krms:.3e} > {M} * {erms:.3e} + {hrms:.3e}")
    if fails is not None:
        fails.extend(msgs)
    else:
        assert not msgs, "; ".join(msgs)
    return rmax, rrms


def forward_tol(ref64, emu, dtype, M) -> float:
    """The right-hand side of the max inequality (the half width of the ReLU exclusion band)."""
    (_, emax, hmax), _ = figures(emu, ref64, emu, dtype)
    return M * emax + hmax


def relu_band(z64, t: float):
    """(inside, share): the elements whose oracle pre-activation lies within ``t`` of zero -- the
    only ones whose ReLU side the kernel's rounding may decide -- and their share of the tensor."""
    inside = z64.abs() <= t
    return inside, float(inside.double().mean())
