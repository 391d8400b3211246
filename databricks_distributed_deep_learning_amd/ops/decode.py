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
* Further settings, in the order they apply (HF's): ``repetition_penalty`` r > 0, before anything else and
  for greedy too: ``x_j <- x_j / r`` if ``x_j > 0`` else ``x_j * r``, in fp32 from the original logit and
  rounded once to the logits' dtype, for every distinct column id in the row's history,
  ``history[b, :history_lens[b]]`` (int64 ``[B, Lh]``, int32 ``[B]`` clamped to ``0 .. Lh``) plus
  ``tokens_out[b, :step[b]]`` when both are given; ids outside ``[0, V)`` do not count.  Then top-k as
  above; then ``top_p`` in (0, 1]: with ``W`` the mass of the top-k set, column j stays iff the mass of the
  columns with a strictly larger value is ``< p * W`` (the kept set is ``x >= T`` for the largest value ``T``
  with ``mass(x >= T) >= p * W``: ties at the cut are all kept, the maximum always); then ``min_p`` in
  [0, 1): column j stays iff ``(x_j - max x) * inv_temperature >= log(min_p)`` in fp32.  The kept set is the
  intersection; the weights and the prefix-sum rule are as above.
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


def _f32_bits(v: float) -> int:
    return struct.unpack("<i", struct.pack("<f", float(v)))[0]


def _bits_f32(bits: int) -> float:
    return struct.unpack("<f", struct.pack("<i", bits))[0]


def check_filters(top_p, min_p, repetition_penalty) -> None:
    if top_p is not None and not 0 < top_p <= 1:
        raise ValueError("top_p must be in (0, 1]")
    if min_p is not None and not 0 <= min_p < 1:
        raise ValueError("min_p must be in [0, 1)")
    if repetition_penalty is not None and not repetition_penalty > 0:
        raise ValueError("repetition_penalty must be positive")


def next_token_params(inv_temperature: float = 1.0, top_k: Optional[int] = None, eos_token_id: Optional[int] = None,
                      pad_token_id: Optional[int] = None, sample: bool = True, device=None, *,
                      top_p: Optional[float] = None, min_p: Optional[float] = None,
                      repetition_penalty: Optional[float] = None) -> torch.Tensor:
    """int32 ``[5]``: inv_temperature's fp32 bits, top_k (0: none), eos (-1: none), pad, sample flag.  With any
    of ``top_p`` / ``min_p`` / ``repetition_penalty``: int32 ``[8]``, the same five, then the fp32 bits of
    top_p (1.0: off), min_p (0.0: off) and repetition_penalty (1.0: off)."""
    pad = pad_token_id if pad_token_id is not None else (eos_token_id if eos_token_id is not None else 0)
    v = [_f32_bits(inv_temperature), 0 if top_k is None else int(top_k),
         -1 if eos_token_id is None else int(eos_token_id), int(pad), int(bool(sample))]
    if top_p is not None or min_p is not None or repetition_penalty is not None:
        v += [_f32_bits(1.0 if top_p is None else top_p), _f32_bits(0.0 if min_p is None else min_p),
              _f32_bits(1.0 if repetition_penalty is None else repetition_penalty)]
    return torch.tensor(v, dtype=torch.int32, device=device)


def _unpack_params(params: torch.Tensor):
    """(inv_t, top_k, eos, pad, sample, top_p, min_p, repetition_penalty), the last three neutral for ``[5]``."""
    v = params.tolist()
    ext = [_bits_f32(w) for w in v[5:8]] if len(v) == 8 else [1.0, 0.0, 1.0]
    return (_bits_f32(v[0]), v[1], v[2], v[3], bool(v[4]), *ext)


def penalise_logits(logits: torch.Tensor, r, history, history_lens, tokens_out, step) -> torch.Tensor:
    """A copy of ``logits [B, V]`` with the repetition penalty ``r`` (a number, or an fp32 tensor of one element
    on the logits' device) on every column id of ``history[b, :history_lens[b]]`` and ``tokens_out[b,
    :step[b]]``.  The counts are read on the device: no host sync, so a graph capture can hold it."""
    B, V = logits.shape
    dev = logits.device
    hit = torch.zeros(B, V + 1, dtype=torch.bool, device=dev)       # column V: the entries that do not count
    for ids, n in ((history, history_lens), (tokens_out, step) if step is not None else (None, None)):
        if ids is None or ids.shape[1] == 0:
            continue
        ids = ids.long()
        live = (ids >= 0) & (ids < V)
        if n is not None:
            live &= torch.arange(ids.shape[1], device=dev)[None, :] < n[:, None]
        hit.scatter_(1, torch.where(live, ids, torch.full_like(ids, V)), True)
    if not torch.is_tensor(r):      # (a tensor: a GPU division by a host number multiplies by its reciprocal)
        r = torch.tensor(float(r), dtype=torch.float32, device=dev)
    x = logits.float()
    return torch.where(hit[:, :V], torch.where(x > 0, x / r, x * r).to(logits.dtype), logits)


def sampling_kept(x: torch.Tensor, inv_t: float, top_k=None, top_p: float = 1.0, min_p: float = 0.0) -> torch.Tensor:
    """fp32 ``x [B, V]`` -> bool ``[B, V]``: the columns top-k, top-p and min-p all keep (module docstring)."""
    V = x.shape[-1]
    kept = torch.ones_like(x, dtype=torch.bool)
    xmax = x.max(-1, keepdim=True).values
    if top_k is not None and 0 < top_k < V:
        kept = x >= x.topk(top_k, -1).values[:, -1:]
    if top_p < 1.0:
        xs = torch.where(kept, x, torch.full_like(x, float("-inf"))).sort(-1, descending=True).values
        c = torch.exp((xs - xmax) * inv_t).double().cumsum(-1)
        # the mass strictly above a value: the exclusive sum at the first column of its run of equal values
        first = torch.searchsorted(-xs, -xs, right=False)
        above = torch.cat([torch.zeros_like(c[:, :1]), c[:, :-1]], -1).gather(-1, first)
        n = (above < top_p * c[:, -1:]).sum(-1, keepdim=True).clamp(min=1)
        kept = kept & (x >= xs.gather(-1, n - 1))
    if min_p > 0.0:
        kept = kept & ((x - xmax) * inv_t >= torch.log(torch.tensor(min_p, dtype=torch.float32, device=x.device)))
    return kept


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


def next_token_reference(logits, u, params, step, done, out, tokens_out, lens, history=None, history_lens=None):
    B, V = logits.shape
    inv_t, top_k, eos, pad, sample, top_p, min_p, pen = _unpack_params(params)
    if pen != 1.0:
        logits = penalise_logits(logits, pen, history, history_lens, tokens_out, step)
    x = logits.float()
    if u is None or not sample:
        tok = x.argmax(-1)
    else:
        row = 0 if step is None else int(step[0])
        ub = u[min(max(row, 0), u.shape[0] - 1)].double()
        kept = sampling_kept(x, inv_t, top_k, top_p, min_p)
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
               tokens_out: Optional[torch.Tensor] = None, lens: Optional[torch.Tensor] = None,
               top_p: Optional[float] = None, min_p: Optional[float] = None,
               repetition_penalty: Optional[float] = None, history: Optional[torch.Tensor] = None,
               history_lens: Optional[torch.Tensor] = None) -> torch.Tensor:
    """See the module docstring.  ``u``: fp32 ``[T, B]`` (or ``[B]``); ``params``: int32 ``[5]`` or ``[8]``
    (``next_token_params``); returns ``out`` (allocated if None)."""
    if logits.dim() != 2 or logits.shape[1] < 1:
        raise ValueError(f"logits must be [B, V], got {tuple(logits.shape)}")
    B, V = logits.shape
    dev = logits.device
    if top_k is not None and top_k < 1:
        raise ValueError("top_k must be at least 1")
    if not inv_temperature > 0:
        raise ValueError("inv_temperature must be positive")
    check_filters(top_p, min_p, repetition_penalty)
    if u is not None:
        if u.dim() == 1:
            u = u.unsqueeze(0)
        if u.dtype != torch.float32 or u.dim() != 2 or u.shape[1] != B or u.shape[0] < 1 or not u.is_contiguous():
            raise ValueError(f"u must be contiguous fp32 [T, {B}] (or [{B}]), got {u.dtype} {tuple(u.shape)}")
    n_params = 8 if params is not None and params.dim() == 1 and params.shape[0] == 8 else 5
    for name, t, dt, shape in (("step", step, torch.int32, (B,)), ("done", done, torch.bool, (B,)),
                               ("out", out, torch.int64, (B,)), ("lens", lens, torch.int32, (B,)),
                               ("params", params, torch.int32, (n_params,)),
                               ("history_lens", history_lens, torch.int32, (B,))):
        if t is not None and (t.dtype != dt or tuple(t.shape) != shape or not t.is_contiguous() or t.device != dev):
            raise ValueError(f"{name} must be a contiguous {dt} {shape} tensor on {dev}, got {t.dtype} "
                             f"{tuple(t.shape)} on {t.device}")
    for name, t in (("tokens_out", tokens_out), ("history", history)):
        if t is not None and (t.dtype != torch.int64 or t.dim() != 2 or t.shape[0] != B or t.shape[1] < 1
                              or not t.is_contiguous() or t.device != dev):
            raise ValueError(f"{name} must be a contiguous int64 [{B}, T] tensor on {dev}")
    if history_lens is not None and history is None:
        raise ValueError("history_lens needs history")
    if params is None:
        params = next_token_params(inv_temperature, top_k, eos_token_id, pad_token_id, True, dev, top_p=top_p,
                                   min_p=min_p, repetition_penalty=repetition_penalty)
    if out is None:
        out = torch.empty(B, dtype=torch.int64, device=dev)
    if _lib.use_native(logits, u) and logits.dtype == torch.bfloat16 and logits.is_contiguous():
        from . import _native_decode_step
        if params.shape[0] == 5 and history is None:
            return _native_decode_step.next_token(logits, u, params, step, done, out, tokens_out, lens)
        if params.shape[0] == 8 and not _native_decode_step.row_in_lds(V):
            # the kernel penalises rows it holds in LDS; a longer row here, from the settings on the device
            logits = penalise_logits(logits, params[7:8].view(torch.float32), history, history_lens, tokens_out, step)
        return _native_decode_step.next_token_ex(logits, u, params, history, history_lens, step, done, out,
                                                 tokens_out, lens)
    return next_token_reference(logits, u, params, step, done, out, tokens_out, lens, history, history_lens)
