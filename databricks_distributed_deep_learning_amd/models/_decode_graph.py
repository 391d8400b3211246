"""A decode session: the static state of a generation loop and its step, captured once.

The step is one linear chain on one stream -- the model's ``_session_logits`` (GPT-2: ``ops.decode_embed``,
every block's ``decode``, ``ln_f`` and the head ``ops.linear_small_m``; Llama: the ``embed_tokens`` gather,
every block's ``decode``, ``norm`` and the head), with the attention launch bound fixed at the cache capacity
(so the grid is the same at every step; rows past ``lens`` are still never loaded), then ``ops.next_token``,
which also advances the cache lengths and the step counter -- and it reads and writes only the session's own
tensors, so on the GPU it is captured into a ``torch.cuda.CUDAGraph`` and replayed: one host call per token
instead of about a hundred.  Off the GPU (or without the native kernels) the same step runs eagerly.

What a model hands the session: ``_session_weight()`` (its token embedding: device and dtype of the
state, part of the key), ``_session_cache(batch, capacity, device)`` and ``_session_logits(tok_cur, cache)``
(the step up to the ``[B, vocab]`` logits, at ``len_bound = cache.capacity``, not advancing the lengths).
"""
from __future__ import annotations

import weakref

import torch

from .. import ops

_sessions: "weakref.WeakKeyDictionary" = weakref.WeakKeyDictionary()     # model -> its DecodeSession


def round_capacity(need: int, n_positions: int) -> int:
    """``need`` positions rounded up to a multiple of 128, capped at ``n_positions``."""
    return min((need + 127) // 128 * 128, n_positions)


def _key(model, batch: int, capacity: int, graph: bool, ext: bool = False):
    w = model._session_weight()
    return (batch, capacity, w.device, w.dtype, graph, ext, tuple(p.data_ptr() for p in model.parameters()))


def session_for(model, batch: int, capacity: int, graph: bool, ext: bool = False) -> "DecodeSession":
    """The model's session for this shape: rebuilt when the batch, the capacity, the device, the dtype or
    the address of any parameter baked into the captured step has changed.  ``ext``: a session whose step
    also serves top-p, min-p and a repetition penalty (another launch in the captured step, so part of the
    key); without it the step is the one it always was."""
    key = _key(model, batch, capacity, graph, ext)
    s = _sessions.get(model)
    if s is None or s.key != key:
        s = None
        _sessions.pop(model, None)          # (frees the old session's cache before the new one is allocated)
        s = _sessions[model] = DecodeSession(model, batch, capacity, graph, key, ext)
    return s


def current_session(model):
    return _sessions.get(model)


class DecodeSession:
    WARMUP = 2

    def __init__(self, model, batch: int, capacity: int, graph: bool, key=None, ext: bool = False):
        dev = model._session_weight().device
        self.key = key
        self._model = weakref.ref(model)
        self.batch, self.capacity = batch, capacity
        self.cache = model._session_cache(batch, capacity, dev)
        self.tok_cur = torch.zeros(batch, dtype=torch.int64, device=dev)
        self.done = torch.zeros(batch, dtype=torch.bool, device=dev)
        self.step = torch.zeros(batch, dtype=torch.int32, device=dev)
        self.u = torch.zeros(capacity, batch, dtype=torch.float32, device=dev)
        self.tokens_out = torch.zeros(batch, capacity, dtype=torch.int64, device=dev)
        # the settings, int32 [8]; a session without ``ext`` hands its step the first five, as ever
        self.ext = ext
        self.params = ops.next_token_params(device=dev, top_p=1.0)
        self.history = torch.zeros(batch, capacity, dtype=torch.int64, device=dev) if ext else None
        self.history_lens = torch.zeros(batch, dtype=torch.int32, device=dev) if ext else None
        self.captures = 0
        self.graph = None
        if graph:
            self._capture()

    def _state(self):
        return (self.cache.lens, self.tok_cur, self.done, self.step, self.tokens_out)

    def _select(self, logits, lens):
        if self.ext:
            ops.next_token(logits, u=self.u, params=self.params, step=self.step, done=self.done, out=self.tok_cur,
                           tokens_out=self.tokens_out, lens=lens, history=self.history,
                           history_lens=self.history_lens)
        else:
            ops.next_token(logits, u=self.u, params=self.params[:5], step=self.step, done=self.done,
                           out=self.tok_cur, tokens_out=self.tokens_out, lens=lens)

    def _step(self):
        self._select(self._model()._session_logits(self.tok_cur, self.cache), self.cache.lens)

    def _capture(self):
        # the warm-up really executes (on a side stream, as export.GraphRunner's): it writes dead cache rows,
        # which get rewritten, and advances the state, which is put back -- or lens would walk off the cache
        saved = [t.clone() for t in self._state()]
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s), torch.no_grad():
            for _ in range(min(self.WARMUP, self.capacity)):
                self._step()
        torch.cuda.current_stream().wait_stream(s)
        for t, v in zip(self._state(), saved):
            t.copy_(v)
        self.graph = torch.cuda.CUDAGraph()
        with torch.no_grad(), torch.cuda.graph(self.graph):
            self._step()
        self.captures += 1

    def begin(self, params: torch.Tensor, u=None, history=None, history_lens=None):
        """Before a generation: fresh counters and flags, this call's settings (int32 ``[5]``, or ``[8]`` on
        an ``ext`` session) and uniform numbers, and the prompts the repetition penalty counts (``history
        [B, S0]`` with ``history_lens``: ``ext`` sessions only; none: no prompt counts)."""
        if not self.ext and (params.shape[0] != 5 or history is not None):
            raise ValueError("top_p, min_p, repetition_penalty and history need a session made with ext=True")
        self.done.zero_()
        self.step.zero_()
        self.params[:params.shape[0]].copy_(params)
        if params.shape[0] == 5:
            self.params[5:].copy_(ops.next_token_params(top_p=1.0)[5:])
        if self.ext:
            self.history_lens.zero_()
            if history is not None:
                self.history[:, :history.shape[1]].copy_(history)
                if history_lens is None:
                    self.history_lens.fill_(history.shape[1])
                else:
                    self.history_lens.copy_(history_lens)
        if u is not None:
            self.u[:u.shape[0]].copy_(u)

    def first_token(self, logits: torch.Tensor):
        """From the prefill's logits, by the step's own kernel; prefill has already set the lengths."""
        self._select(logits, None)

    def advance(self):
        if self.graph is not None:
            self.graph.replay()
        else:
            with torch.no_grad():
                self._step()
