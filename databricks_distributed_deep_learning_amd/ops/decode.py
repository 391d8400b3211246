"""The glue of a generation step: the embedding add and the choice of the next token.

``decode_embed(tok, lens, wte, wpe)``: ``h[b] = wte[tok[b]] + wpe[lens[b]]``, added in fp32 and rounded once.

``next_token(logits, ...)``: one token per row of ``logits [B, V]``.

* Greedy (``u=None``, or ``params[4] == 0``): the argmax, ties to the lowest index.
* Sampling, given one uniform number per row, ``u`` in [0, 1): with ``x`` the row, the kept set is every
  column whose logit is >= the ``top_k``-th largest value (ties at that value are all kept; no ``top_k``,
  or ``top_k >= V``: every column), ``w_j = exp((x_j - max x) * inv_temperature)`` in fp32 over the kept
  set, ``W`` their sum; the token is the lowest kept index whose inclusive prefix sum of ``w`` (in index
  order) exceeds ``u * W``, or the last kept index if rounding leaves none.  A pure function of
  ``(logits, u)``: the randomness is the caller's.
* Optional state, each tensor updated in place when given: ``step`` (int32 ``[B]``, the row of ``u
  [T, B]`` to read and the column of ``tokens_out [B, T']`` to write; one counter per batch row, all equal;
  0 without it), ``done`` (bool ``[B]``: a done row gets ``pad``; then ``done |= token == eos``), ``out``
  (int64 ``[B]``: receives the tokens -- the next step's input), ``tokens_out``, ``lens`` (int32 ``[B]``,
  ``+= 1``: a KV cache's lengths).  ``step += 1`` last.

The settings travel in a small device tensor (``next_token_params``), so that a captured launch serves any
of them; the keyword scalars build one on the fly when ``params`` is not given.
"""
from __future__ import annotations

import struct
from typing import Optional

import torch

from . import _lib


def next_token_params(inv_temperature: float = 1.0, top_k: Optional[int] = None, eos_token_id: Optional[int] = None,
                      pad_token_id: Optional[int] = None, sample: bool = True, device=None) -> torch.Tensor:
    """int32 ``[5]``: inv_temperature's fp32 bits, top_k (0: none), eos (-1: none), pad, sample flag."""
    bits = struct.unpack("<i", struct.pack("<f", float(inv_temperature)))[0]
    pad = pad_token_id if pad_token_id is not None else (eos_token_id if eos_token_id is not None else 0)
    return torch.tensor([bits, 0 if top_k is None else int(top_k), -1 if eos_token_id is None else int(eos_token_id),
                         int(pad), int(bool(sample))], dtype=torch.int32, device=device)


def _unpack_params(params: torch.Tensor):
    bits, top_k, eos, pad, sample = params.tolist()
    return struct.unpack("<f", struct.pack("<i", bits))[0], top_k, eos, pad, bool(sample)


def decode_embed_reference(tok: torch.Tensor, lens: torch.Tensor, wte: torch.Tensor, wpe: torch.Tensor) -> torch.Tensor:
    ct = torch.float64 if wte.dtype == torch.float64 else torch.float32
    return (wte[tok].to(ct) + wpe[lens.long()].to(ct)).to(wte.dtype)


def decode_embed(tok: torch.Tensor, lens: torch.Tensor, wte: torch.Tensor, wpe: torch.Tensor) -> torch.Tensor:
    """``tok`` int64 ``[B]``, ``lens`` int32 ``[B]`` (both read on the device), tables ``[V, E]`` / ``[P, E]``
    -> ``[B, E]``."""
    if tok.dim() != 1 or lens.shape != tok.shape or wte.dim() != 2 or wpe.dim() != 2 or wte.shape[1] != wpe.shape[1]:
        raise ValueError(f"decode_embed: tok {tuple(tok.shape)}, lens {tuple(lens.shape)}, wte {tuple(wte.shape)}, "
                         f"wpe {tuple(wpe.shape)}")
    if (_lib.use_native(tok, lens, wte, wpe) and wte.dtype == torch.bfloat16 and wpe.dtype == torch.bfloat16
            and tok.dtype == torch.int64 and lens.dtype == torch.int32 and wte.shape[1] % 8 == 0
            and all(t.is_contiguous() for t in (tok, lens, wte, wpe))
            and wte.data_ptr() % 16 == 0 and wpe.data_ptr() % 16 == 0):
        from . import _native_decode_step
        return _native_decode_step.decode_embed(tok, lens, wte, wpe)
    return decode_embed_reference(tok, lens, wte, wpe)


def next_token_reference(logits, u, params, step, done, out, tokens_out, lens):
    B, V = logits.shape
    inv_t, top_k, eos, pad, sample = _unpack_params(params)
    x = logits.float()
    if u is None or not sample:
        tok = x.argmax(-1)
    else:
        row = 0 if step is None else int(step[0])
        ub = u[min(max(row, 0), u.shape[0] - 1)].double()
        kept = torch.ones_like(x, dtype=torch.bool)
        if 0 < top_k < V:
            kept = x >= x.topk(top_k, -1).values[:, -1:]
        w = torch.where(kept, torch.exp((x - x.max(-1, keepdim=True).values) * inv_t), torch.zeros_like(x))
        c = w.double().cumsum(-1)
        hit = kept & (c > ub[:, None] * c[:, -1:])
        last = V - 1 - kept.flip(-1).int().argmax(-1)
        tok = torch.where(hit.any(-1), hit.int().argmax(-1), last)
    if done is not None:
        tok = torch.where(done, torch.full_like(tok, pad), tok)
        if eos >= 0:
            done |= tok == eos
    out.copy_(tok)
    if tokens_out is not None and step is not None:
        col = int(step[0])
        if 0 <= col < tokens_out.shape[1]:
            tokens_out[:, col] = tok
    elif tokens_out is not None and tokens_out.shape[1] > 0:
        tokens_out[:, 0] = tok
    if step is not None:
        step += 1
    if lens is not None:
        lens += 1
    return out


def next_token(logits: torch.Tensor, *, u: Optional[torch.Tensor] = None, inv_temperature: float = 1.0,
               top_k: Optional[int] = None, eos_token_id: Optional[int] = None, pad_token_id: Optional[int] = None,
               params: Optional[torch.Tensor] = None, step: Optional[torch.Tensor] = None,
               done: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None,
               tokens_out: Optional[torch.Tensor] = None, lens: Optional[torch.Tensor] = None) -> torch.Tensor:
    """See the module docstring.  ``u``: fp32 ``[T, B]`` (or ``[B]``); returns ``out`` (allocated if None)."""
    if logits.dim() != 2 or logits.shape[1] < 1:
        raise ValueError(f"logits must be [B, V], got {tuple(logits.shape)}")
    B, V = logits.shape
    dev = logits.device
    if top_k is not None and top_k < 1:
        raise ValueError("top_k must be at least 1")
    if not inv_temperature > 0:
        raise ValueError("inv_temperature must be positive")
    if u is not None:
        if u.dim() == 1:
            u = u.unsqueeze(0)
        if u.dtype != torch.float32 or u.dim() != 2 or u.shape[1] != B or u.shape[0] < 1 or not u.is_contiguous():
            raise ValueError(f"u must be contiguous fp32 [T, {B}] (or [{B}]), got {u.dtype} {tuple(u.shape)}")
    for name, t, dt, shape in (("step", step, torch.int32, (B,)), ("done", done, torch.bool, (B,)),
                               ("out", out, torch.int64, (B,)), ("lens", lens, torch.int32, (B,)),
                               ("params", params, torch.int32, (5,))):
        if t is not None and (t.dtype != dt or tuple(t.shape) != shape or not t.is_contiguous() or t.device != dev):
            raise ValueError(f"{name} must be a contiguous {dt} {shape} tensor on {dev}, got {t.dtype} "
                             f"{tuple(t.shape)} on {t.device}")
    if tokens_out is not None and (tokens_out.dtype != torch.int64 or tokens_out.dim() != 2 or tokens_out.shape[0] != B
                                   or tokens_out.shape[1] < 1 or not tokens_out.is_contiguous()
                                   or tokens_out.device != dev):
        raise ValueError(f"tokens_out must be a contiguous int64 [{B}, T] tensor on {dev}")
    if params is None:
        params = next_token_params(inv_temperature, top_k, eos_token_id, pad_token_id, True, dev)
    if out is None:
        out = torch.empty(B, dtype=torch.int64, device=dev)
    if _lib.use_native(logits, u) and logits.dtype == torch.bfloat16 and logits.is_contiguous():
        from . import _native_decode_step
        return _native_decode_step.next_token(logits, u, params, step, done, out, tokens_out, lens)
    return next_token_reference(logits, u, params, step, done, out, tokens_out, lens)
