"""An independent reference for the kernels of ``csrc/kernels/elementwise.hip``: GELU, dropout, column
sums, softmax cross-entropy / top-k, NHWC pooling, embedding and the flat glue.

Everything here is device-agnostic torch written out from the formulas: nothing from ``ops/``, no
``F.gelu`` / ``F.max_pool2d`` / ``F.cross_entropy`` / ``F.embedding`` / ``torch.topk``.  Each reference
takes a ``dtype``, as in ``norm_oracle``:

``torch.float64``  the oracle: exact arithmetic on the (already rounded) inputs, nothing rounded.
``torch.float32``  the emulation: fp32 arithmetic, every stored tensor rounded once to the dtype of the
                   input, fp32 side outputs (row losses, probabilities, column partials) left in fp32.

The bound is ``norm_oracle.bound``; ``shrink`` folds a derived per-element allowance (the erf
approximation's documented error) into it.
"""
from __future__ import annotations

import math
from types import SimpleNamespace

import torch

from norm_oracle import _rounder, bound, forward_tol, half_ulp  # noqa: F401  (shared, not copied)
from test_kernels_gpu import _hash_keep  # the dropout keep mask: not re-derived here

ERF_ABS_ERR = 1.5e-7          # Abramowitz & Stegun 7.1.26, the kernels' erf: |error| <= 1.5e-7
SQRT2 = math.sqrt(2.0)
INV_SQRT_2PI = 1.0 / math.sqrt(2.0 * math.pi)


def shrink(got, ref64, allow):
    """``got`` with each element moved towards the oracle by ``allow`` (>= 0, elementwise): bounding the
    result allows every element its own extra error on top of the measured yardstick."""
    d = got.double() - ref64.double()
    return ref64.double() + torch.sign(d) * torch.clamp_min(d.abs() - allow.double(), 0.0)


# ---------------------------------------------------------------------------- GELU, tanh
def _gelu(z):
    return 0.5 * z * torch.special.erfc(-z / SQRT2)


def _gelu_grad(z):
    return 0.5 * torch.special.erfc(-z / SQRT2) + z * torch.exp(-0.5 * z * z) * INV_SQRT_2PI


def gelu_ref(z, dtype):
    """erf-form GELU ``z Phi(z)``, with Phi through erfc so that the negative tail is not cancelled."""
    return _rounder(z.dtype, dtype)(_gelu(z.to(dtype)))


def gelu_grad_ref(z, dtype):
    """``Phi(z) + z phi(z)`` (not rounded: a factor, never stored)."""
    return _gelu_grad(z.to(dtype))


def gelu_bwd_ref(dy, z, dtype, out=None, out_dtype=None, accumulate=False):
    """``dz = dy gelu'(z)`` and the column sums of the *rounded* dz (``gelu_bwd_colsum_k``), optionally
    added to ``out`` and rounded to ``out_dtype``."""
    rnd = _rounder(z.dtype, dtype)
    dz = rnd(dy.to(dtype) * _gelu_grad(z.to(dtype)))
    o = SimpleNamespace(dz=dz, colsum=None)
    if z.dim() == 2 and out_dtype is not None:
        o.colsum = colsum_ref(dz, dtype, out, out_dtype, accumulate)
    return o


def tanh_bwd_ref(dy, y, dtype):
    yf = y.to(dtype)
    return _rounder(y.dtype, dtype)(dy.to(dtype) * (1.0 - yf * yf))


# ---------------------------------------------------------------------------- dropout
def keep_bits(x, seed: int, p: float):
    return _hash_keep(seed, x.numel(), p).to(x.device).view(x.shape)


def dropout_ref(x, seed: int, p: float, dtype, keep=None):
    """``x keep / (1 - p)`` with the kernels' keep bits; ``p`` is the fp32 value the kernel receives."""
    keep = keep_bits(x, seed, p) if keep is None else keep
    xf = x.to(dtype)
    y = torch.where(keep, xf / (1.0 - torch.tensor(p, dtype=dtype)), torch.zeros((), dtype=dtype, device=x.device))
    return SimpleNamespace(y=_rounder(x.dtype, dtype)(y), keep=keep)


# ---------------------------------------------------------------------------- column sums
def colsum_ref(x, dtype, out=None, out_dtype=None, accumulate=False):
    """``out[c] (+)= sum_r x[r, c]``, rounded once to ``out_dtype`` in the emulation."""
    s = x.to(dtype).sum(0)
    if accumulate:
        s = s + out.to(dtype)
    return _rounder(out_dtype if out_dtype is not None else x.dtype, dtype)(s)


# ---------------------------------------------------------------------------- softmax cross-entropy / top-k
def _softmax(x):
    m = x.max(-1, keepdim=True).values
    e = torch.exp(x - m)
    s = e.sum(-1, keepdim=True)
    return e / s, m, s


def ce_ref(logits, labels, upstream: float, dtype):
    """Mean-reduced softmax cross-entropy: per-row loss, mean loss, ``(softmax - onehot) / B`` and that
    scaled by the upstream scalar.  The emulation rounds the gradient twice, as ``softmax_ce_k`` (which
    stores it) and ``scale_k`` (which rescales the stored tensor) do."""
    rnd = _rounder(logits.dtype, dtype)
    x = logits.to(dtype)
    B, C = x.shape
    p, m, s = _softmax(x)
    row = (m + torch.log(s)).squeeze(-1) - x.gather(1, labels.view(-1, 1)).squeeze(1)
    onehot = torch.zeros_like(x).scatter_(1, labels.view(-1, 1), 1.0)
    dl = rnd((p - onehot) / B)
    return SimpleNamespace(row_loss=row, loss=row.sum() / B, dlogits=dl, dscaled=rnd(dl.to(dtype) * upstream))


def topk_ref(logits, k: int, dtype):
    """Softmax probabilities and the k largest: ordered by value, then by lower index (a stable
    descending sort of the fp64 logits, whatever ``dtype`` the probabilities are computed in)."""
    x = logits.to(dtype)
    p = _softmax(x)[0]
    order = torch.sort(logits.double(), dim=-1, descending=True, stable=True).indices[..., :k]
    return SimpleNamespace(probs=p, values=p.gather(-1, order), indices=order)


# ---------------------------------------------------------------------------- NHWC max-pool
def pool_shape(H, W, K, S, pad):
    return (H + 2 * pad - K) // S + 1, (W + 2 * pad - K) // S + 1


def _taps(a, K, S, pad):
    """Yields (tap, window values [N, P, Q, C], in-bounds [1, P, Q, 1], rows, columns) in (r, s) order."""
    N, H, W, C = a.shape
    P, Q = pool_shape(H, W, K, S, pad)
    dev = a.device
    for r in range(K):
        hs = torch.arange(P, device=dev) * S - pad + r
        vh = (hs >= 0) & (hs < H)
        for s in range(K):
            ws = torch.arange(Q, device=dev) * S - pad + s
            vw = (ws >= 0) & (ws < W)
            v = a[:, hs.clamp(0, H - 1)][:, :, ws.clamp(0, W - 1)]
            yield r * K + s, v, (vh[:, None] & vw[None, :])[None, :, :, None], (hs, vh), (ws, vw)


def _select(a, K, S, pad):
    """Window maximum and recorded tap: the first tap in (r, s) order among equal maxima; a NaN takes
    over (the last NaN tap is recorded); an all ``-inf`` window records its first in-bounds tap."""
    N, H, W, C = a.shape
    P, Q = pool_shape(H, W, K, S, pad)
    best = torch.full((N, P, Q, C), float("-inf"), dtype=a.dtype, device=a.device)
    arg = torch.full((N, P, Q, C), -1, dtype=torch.int64, device=a.device)
    for tap, v, valid, _, _ in _taps(a, K, S, pad):
        arg = torch.where(valid & (arg < 0), tap, arg)
        take = valid & ((v > best) | torch.isnan(v))
        best = torch.where(take, v, best)
        arg = torch.where(take, tap, arg)
    return best, arg


def maxpool_bwd_ref(dy, arg, shape, K, S, pad, dtype):
    """Each output's gradient goes to the input its recorded tap names; sums in ``dtype``."""
    N, H, W, C = shape
    dx = torch.zeros(N, H, W, C, dtype=dtype, device=dy.device)
    g = dy.to(dtype)
    probe = torch.zeros(N, H, W, 1, dtype=dtype, device=dy.device)
    for tap, _, _, (hs, vh), (ws, vw) in _taps(probe, K, S, pad):
        c = torch.where(arg == tap, g, torch.zeros((), dtype=dtype, device=dy.device))[:, vh][:, :, vw]
        dx[:, hs[vh][:, None], ws[vw][None, :]] += c       # distinct inputs inside one tap
    return _rounder(dy.dtype, dtype)(dx)


def maxpool_ref(x, K, S, pad, dy, dtype):
    """y (a selection: exact in any dtype), the recorded tap and dx."""
    best, arg = _select(x.double(), K, S, pad)
    return SimpleNamespace(y=best.to(x.dtype), idx=arg, dx=maxpool_bwd_ref(dy, arg, x.shape, K, S, pad, dtype))


def pack_mask(mask):
    """bool [..] -> bytes: bit j of byte e / 8 for flat element e."""
    w = (1 << torch.arange(8, device=mask.device)).to(torch.int64)
    return (mask.reshape(-1, 8).to(torch.int64) * w).sum(1).to(torch.uint8)


def unpack_mask(bits, shape):
    w = torch.arange(8, device=bits.device)
    return ((bits.view(-1, 1).to(torch.int64) >> w) & 1).bool().view(shape)


def bn_relu_maxpool_ref(x, scale, shift, dtype):
    """``maxpool3x3/2(relu(x scale + shift))`` over the activations rounded to the dtype of ``x``
    (emulation; the oracle rounds nothing).  Returns y, the tap, the ReLU mask, the pre-activation z,
    the activation a, and the best / second-best value of every window (second = -inf for a
    one-tap window)."""
    rnd = _rounder(x.dtype, dtype)
    z = x.to(dtype) * scale.to(dtype) + shift.to(dtype)
    a = rnd(torch.clamp_min(z, 0.0)).to(dtype)
    best, arg = _select(a, 3, 2, 1)
    ninf = torch.full((), float("-inf"), dtype=dtype, device=x.device)
    win = torch.stack([torch.where(valid, v, ninf) for _, v, valid, _, _ in _taps(a, 3, 2, 1)])
    top2 = torch.sort(win, dim=0, descending=True).values[:2]
    return SimpleNamespace(y=rnd(best), idx=arg, mask=z > 0, z=z, a=a, best=top2[0], second=top2[1], win=win)


# ---------------------------------------------------------------------------- global average pool
def avgpool_ref(x, dy, dtype):
    rnd = _rounder(x.dtype, dtype)
    N, H, W, C = x.shape
    y = rnd(x.to(dtype).reshape(N, H * W, C).sum(1) / (H * W))
    dx = rnd((dy.to(dtype) / (H * W)).view(N, 1, 1, C).expand(N, H, W, C).contiguous())
    return SimpleNamespace(y=y, dx=dx)


# ---------------------------------------------------------------------------- embedding
def embedding_ref(ids, w, dy, dtype, sink=None):
    """Gather, and the table's gradient as an ``index_add_`` in ``dtype`` (added to ``sink`` if given)."""
    V, D = w.shape
    dw = torch.zeros(V, D, dtype=dtype, device=w.device).index_add_(0, ids.reshape(-1), dy.reshape(-1, D).to(dtype))
    if sink is not None:
        dw = dw + sink.to(dtype)
    return SimpleNamespace(y=w[ids], dw=_rounder(w.dtype, dtype)(dw))


# ---------------------------------------------------------------------------- flat glue
def acc_ref(acc, g, first: bool, dtype):
    """``acc32 = g`` (first) or ``acc32 += g``: an fp32 side output."""
    return g.to(dtype) if first else acc.to(dtype) + g.to(dtype)


def acc_f32_ref(dst, src, dtype):
    return _rounder(dst.dtype, dtype)(dst.to(dtype) + src.to(dtype))


def rows_add_row_ref(a, v, dtype):
    return _rounder(a.dtype, dtype)(a.to(dtype) + v.to(dtype).view(1, -1))
