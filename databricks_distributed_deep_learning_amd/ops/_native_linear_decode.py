"""Linear layer at M <= 16 rows (csrc/kernels/linear_decode.hip): a decode step's GEMMs.

No autograd.  The weight is read in its [N, K] layout, any N (the 50257-row tied head included).
"""
from __future__ import annotations

import ctypes

import torch

from . import _lib
from ._lib import I, L, P

_lib.register({
    "ddl_linear_small_m_plan": [I, I, P],
    "ddl_linear_small_m_ws": [I, I, I],
    "ddl_linear_small_m": [P, P, P, P, P, P, I, I, I, I, P],
})

MAX_M = 16


def plan(N: int, K: int):
    """(weight tiles per wave, workgroups over N, K splits, 64-deep k steps per wave): wave ``w`` of K
    split ``s`` covers k steps ``[(4 s + w) per, (4 s + w + 1) per)``."""
    out = (ctypes.c_int * 4)()
    _lib.fn("ddl_linear_small_m_plan")(N, K, ctypes.cast(out, ctypes.c_void_p))
    return tuple(out)


def linear_small_m(x2, w, b, act, residual2):
    """x2 [M, K], residual2 [M, N] or None, all bf16 and contiguous; returns [M, N]."""
    M, K = x2.shape
    N = w.shape[0]
    y = torch.empty(M, N, dtype=x2.dtype, device=x2.device)
    wsf = _lib.fn("ddl_linear_small_m_ws")
    wsf.restype = L
    n_ws = wsf(M, N, K)
    ws = torch.empty(n_ws, dtype=torch.float32, device=x2.device) if n_ws else None
    _lib.call("ddl_linear_small_m", x2.data_ptr(), w.data_ptr(), _lib.p(b), _lib.p(residual2), y.data_ptr(), _lib.p(ws),
              M, N, K, 1 if act == "gelu" else 0)
    return y
