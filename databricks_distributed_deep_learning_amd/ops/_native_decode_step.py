"""The decode step's glue kernels (csrc/kernels/decode_step.hip): embedding add and token selection.

No autograd, no host sync: every launch argument is a shape or a pointer, the step's state is read and
written on the device, so the launches can be captured once and replayed.
"""
from __future__ import annotations

import torch

from . import _lib
from ._lib import I, L, P

_lib.register({
    "ddl_next_token_lds": [I],
    "ddl_next_token": [P, I, I, P, I, P, P, P, P, P, I, P],
    "ddl_next_token_ex": [P, I, I, P, I, P, I, P, I, P, P, P, P, P, I, P],
    "ddl_decode_embed": [P, P, P, P, P, I, I, I, I],
})


def row_in_lds(V: int) -> bool:
    """Whether ``next_token`` keeps a row of V logits in LDS (else it re-reads the row from memory)."""
    f = _lib.fn("ddl_next_token_lds")
    f.restype = L
    return f(V) > 0


def decode_embed(tok, lens, wte, wpe):
    B, E = tok.shape[0], wte.shape[1]
    h = torch.empty(B, E, dtype=wte.dtype, device=wte.device)
    _lib.call("ddl_decode_embed", tok.data_ptr(), lens.data_ptr(), wte.data_ptr(), wpe.data_ptr(), h.data_ptr(), B, E,
              wte.shape[0], wpe.shape[0])
    return h


def next_token(logits, u, params, step, done, out, tokens_out, lens):
    B, V = logits.shape
    _lib.call("ddl_next_token", logits.data_ptr(), B, V, _lib.p(u), 0 if u is None else u.shape[0], _lib.p(params),
              _lib.p(step), _lib.p(done), out.data_ptr(), _lib.p(tokens_out),
              0 if tokens_out is None else tokens_out.shape[1], _lib.p(lens))
    return out


def next_token_ex(logits, u, params, history, history_lens, step, done, out, tokens_out, lens):
    """``params`` int32 ``[5]`` or ``[8]``; the penalty counts ``history`` / ``tokens_out[:, :step]`` on rows that
    fit LDS (``row_in_lds``) -- a longer row's logits come here already penalised."""
    B, V = logits.shape
    _lib.call("ddl_next_token_ex", logits.data_ptr(), B, V, _lib.p(u), 0 if u is None else u.shape[0],
              params.data_ptr(), params.shape[0], _lib.p(history), 0 if history is None else history.shape[1],
              _lib.p(history_lens), _lib.p(step), _lib.p(done), out.data_ptr(), _lib.p(tokens_out),
              0 if tokens_out is None else tokens_out.shape[1], _lib.p(lens))
    return out
