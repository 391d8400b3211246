"""GPT-2 small / medium / large causal language model (pre-LN decoder, tied head).

Parameter-for-parameter equivalent to HF ``GPT2LMHeadModel`` (124,439,808 parameters for small).  The
blocks are ``ViTLayer``'s wiring -- fused QKV, residual adds in the output GEMMs' epilogues, the
residual-stream gradient bridged into the LayerNorm backwards -- with causal attention
(``ops.attention(..., causal=True)``: the tiled kernels' CAUSAL instances, which skip the tiles
above the diagonal).  The head is the token embedding (tied, no bias) and, with labels, the fused
vocabulary head + loss (``ops.linear_cross_entropy``): the ``[B S, vocab]`` logits exist once.

Labels are NOT shifted here: ``labels[b, s]`` is the token at ``s + 1`` (-100 at the last position
and wherever ``s + 1`` is padding), as ``data.SyntheticTokens(causal_lm=True)`` builds them.

``activation_function="gelu"`` (default) is the exact erf GELU the fused GELU / dGELU GEMM epilogues
compute; ``"gelu_new"`` (HF's tanh form, what the released checkpoints were trained with) runs
unfused: fc1 without activation, ``F.gelu(approximate="tanh")``, fc2.

What stays on ATen in a training step: the position-embedding add (``wte(ids) + wpe[:S]``: one
broadcast add forward, one batch sum + slice backward) and, with ``attention_mask``, the
``(1 - mask) * -10000`` key bias; with ``"gelu_new"`` the tanh GELU and its backward.

Generation (``generate``): ``prefill`` runs the causal forward once over the right-padded prompts, copies
every layer's keys and values into a ``KVCache`` and applies the head to each sequence's last row only;
``decode_step`` then feeds one token per sequence through ``GPT2Block.decode``: single-query attention
over the cache (``ops.attention_decode``, which also appends the new key / value) and the M <= 16
weight-streaming linears (``ops.linear_small_m``).  The cache lengths live on the device, so a step
launches without a host sync; sampling (temperature, top-k, multinomial) is plain torch on the
``[B, vocab]`` logits.  ``generate(use_graph=True)`` runs the step from a decode session instead
(``models/_decode_graph.py``): ``ops.decode_embed`` and ``ops.next_token`` replace the ATen glue and the
sampling, the attention launch bound is the cache capacity at every step, and the step is captured once into
a hipGraph and replayed per token.

``extend`` appends a chunk of T tokens per sequence to a cache that already holds something
(``ops.attention_extend``: the chunk's queries over the cached keys plus, causally, the chunk's own; it appends
too).  ``generate(prefix=cache)`` starts from a copy of a prefilled cache (``KVCache.copy_prefix_``: a shared
system prompt is computed once) and ``generate(prefill_chunk=k)`` consumes the prompt k columns at a time.
"""
from __future__ import annotations

from dataclasses import dataclass

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import ops
from ..ops.bridge import GradBridge
from . import _generate as G
from .layers import Dropout, Embedding, LayerNorm, Linear


@dataclass
class GPT2Config:
    vocab_size: int = 50257
    n_positions: int = 1024
    n_embd: int = 768
    n_layer: int = 12
    n_head: int = 12
    layer_norm_epsilon: float = 1e-5
    resid_pdrop: float = 0.1
    embd_pdrop: float = 0.1
    attn_pdrop: float = 0.1
    initializer_range: float = 0.02
    activation_function: str = "gelu"       # "gelu" (erf, fused) | "gelu_new" (tanh, unfused)


class KVCache:
    """Keys and values of every layer, ``data [L, 2, B, H, C, D]`` (C: capacity in positions), the valid
    length of each batch row on the device (``lens``, int32 ``[B]``) and ``max_len``, the host's upper
    bound on ``lens`` -- what sizes the decode launches, so no step reads ``lens`` back."""

    def __init__(self, data: torch.Tensor, lens: torch.Tensor):
        self.data, self.lens = data, lens
        self.capacity = data.shape[4]
        self.max_len = 0

    @classmethod
    def allocate(cls, model: "GPT2LMHeadModel", batch: int, capacity: int, device=None, dtype=None) -> "KVCache":
        c = model.config
        if not 1 <= capacity <= c.n_positions:
            raise ValueError(f"capacity {capacity} must be in 1 .. n_positions ({c.n_positions})")
        w = model.wte.weight
        device = w.device if device is None else device
        data = torch.empty(c.n_layer, 2, batch, c.n_head, capacity, c.n_embd // c.n_head,
                           dtype=w.dtype if dtype is None else dtype, device=device)
        return cls(data, torch.zeros(batch, dtype=torch.int32, device=device))

    def k(self, layer: int) -> torch.Tensor:
        return self.data[layer, 0]

    def v(self, layer: int) -> torch.Tensor:
        return self.data[layer, 1]

    def copy_prefix_(self, src: "KVCache") -> "KVCache":
        """Start this cache from ``src``'s contents: positions ``< src.max_len`` of every layer, ``lens`` and
        ``max_len``.  ``src`` has this cache's batch or batch 1 (one prefix shared by every row), its dtype and
        its device (nothing is converted or moved silently); it is only read.  Rows of ``src`` may have unequal
        ``lens``: ``src.max_len``, their bound, is what is copied and what ``generate`` counts against
        ``n_positions``."""
        L, _, B, H, C, D = self.data.shape
        Ls, _, Bs, Hs, _, Ds = src.data.shape
        if (Ls, Hs, Ds) != (L, H, D):
            raise ValueError(f"prefix cache has {Ls} layers of {Hs} heads x {Ds}, this one {L} of {H} x {D}")
        if Bs not in (1, B):
            raise ValueError(f"prefix cache batch {Bs} must be 1 or {B}")
        if src.data.dtype != self.data.dtype or src.data.device != self.data.device:
            raise ValueError(f"prefix cache is {src.data.dtype} on {src.data.device}, this one {self.data.dtype} on "
                             f"{self.data.device}")
        if src.max_len > C:
            raise ValueError(f"prefix length {src.max_len} exceeds the cache capacity {C}")
        n = src.max_len
        self.data[:, :, :, :, :n].copy_(src.data[:, :, :, :, :n])
        self.lens.copy_(src.lens)
        self.max_len = n
        return self


class GPT2Block(nn.Module):
    def __init__(self, c: GPT2Config):
        super().__init__()
        H, std = c.n_embd, c.initializer_range
        if c.activation_function not in ("gelu", "gelu_new"):
            raise ValueError(f"activation_function {c.activation_function!r}: 'gelu' or 'gelu_new'")
        self.num_heads = c.n_head
        self.attn_dropout = c.attn_pdrop
        self.tanh_gelu = c.activation_function == "gelu_new"
        self.ln_1 = LayerNorm(H, c.layer_norm_epsilon)
        self.qkv = Linear(H, 3 * H, init_std=std)
        self.attn_out = Linear(H, H, init_std=std)
        self.ln_2 = LayerNorm(H, c.layer_norm_epsilon)
        self.fc1 = Linear(H, 4 * H, act=None if self.tanh_gelu else "gelu", init_std=std)
        self.fc2 = Linear(4 * H, H, init_std=std)
        self.dropout = Dropout(c.resid_pdrop)
        for lin in (self.qkv, self.attn_out, self.fc1, self.fc2):
            nn.init.zeros_(lin.bias)

    def _mlp(self, y, **kw):
        if self.tanh_gelu:
            return self.fc2(F.gelu(self.fc1(y), approximate="tanh"), **kw)
        return self.fc2(self.fc1(y), fuse_dgelu=True, **kw)

    def forward(self, h, mask=None, doc=None):
        """``doc`` (packed rows): ``ops.doc_bounds``' pair."""
        bridged = torch.is_grad_enabled() and h.requires_grad
        b1 = GradBridge() if bridged else None
        y = self.ln_1(h, grad_from=b1)
        if doc is None:
            ctx = ops.attention(self.qkv(y), self.num_heads, mask, self.attn_dropout, self.training, causal=True)
        else:
            ctx = ops.attention(self.qkv(y), self.num_heads, mask, self.attn_dropout, self.training, causal=True,
                                doc_start=doc)
        if self.dropout.p > 0.0 and self.training:
            h = h + self.dropout(self.attn_out(ctx))
            return h + self.dropout(self._mlp(self.ln_2(h)))
        # no residual dropout: both residual adds ride the output GEMMs' epilogues and the residual
        # stream's gradient reaches each LayerNorm backward through a bridge (as in ViTLayer)
        h = self.attn_out(ctx, residual=h, residual_grad_to=b1)
        b2 = GradBridge() if bridged else None
        y = self.ln_2(h, grad_from=b2)
        return self._mlp(y, residual=h, residual_grad_to=b2)

    def prefill(self, h, mask, cache: KVCache, layer: int):
        """The inference forward (no dropout) that also copies this layer's keys / values into the cache."""
        qkv = self.qkv(self.ln_1(h))
        ops.kv_cache_fill(qkv, cache.k(layer), cache.v(layer), self.num_heads)
        h = self.attn_out(ops.attention(qkv, self.num_heads, mask, 0.0, False, causal=True), residual=h)
        return self._mlp(self.ln_2(h), residual=h)

    def decode(self, h_new, cache: KVCache, layer: int, len_bound=None):
        """One new token per sequence, ``h_new [B, E]``, against the cache (which gains its key / value).
        ``len_bound``: the bound on ``lens + 1`` that sizes the attention launch (default ``max_len + 1``)."""
        lin = ops.linear_small_m
        qkv = lin(self.ln_1(h_new), self.qkv.weight, self.qkv.bias)
        ctx = ops.attention_decode(qkv, cache.k(layer), cache.v(layer), cache.lens, self.num_heads,
                                   cache.max_len + 1 if len_bound is None else len_bound)
        return self._small_m_tail(ctx, h_new)

    def _small_m_tail(self, ctx, h):
        """Output projection and MLP of a block on M <= 16 rows (``ops.linear_small_m``)."""
        lin = ops.linear_small_m
        h = lin(ctx, self.attn_out.weight, self.attn_out.bias, residual=h)
        y = self.ln_2(h)
        if self.tanh_gelu:
            z = F.gelu(lin(y, self.fc1.weight, self.fc1.bias), approximate="tanh")
        else:
            z = lin(y, self.fc1.weight, self.fc1.bias, act="gelu")
        return lin(z, self.fc2.weight, self.fc2.bias, residual=h)

    def extend(self, h, cache: KVCache, layer: int, new_lens=None, len_bound=None):
        """A chunk of new tokens per sequence, ``h [B, T, E]``, against the cache, which gains the keys /
        values of each row's first ``new_lens`` (default T) tokens: ``prefill`` with ``ops.attention_extend``
        in place of attention + fill.  ``len_bound``: the bound on ``lens`` (default ``max_len``).  With
        ``B T <= 16`` the linears are the weight-streaming ones of ``decode``."""
        small = h.shape[0] * h.shape[1] <= 16
        y = self.ln_1(h)
        qkv = ops.linear_small_m(y, self.qkv.weight, self.qkv.bias) if small else self.qkv(y)
        ctx = ops.attention_extend(qkv, cache.k(layer), cache.v(layer), cache.lens, self.num_heads,
                                   cache.max_len if len_bound is None else len_bound, new_lens)
        if small:
            return self._small_m_tail(ctx, h)
        h = self.attn_out(ctx, residual=h)
        return self._mlp(self.ln_2(h), residual=h)


class GPT2LMHeadModel(nn.Module):
    def __init__(self, c: GPT2Config):
        super().__init__()
        if c.n_embd % c.n_head:
            raise ValueError("n_embd must be a multiple of n_head")
        self.config = c
        self.wte = Embedding(c.vocab_size, c.n_embd, c.initializer_range)
        self.wpe = Embedding(c.n_positions, c.n_embd, c.initializer_range)
        self.drop = Dropout(c.embd_pdrop)
        self.h = nn.ModuleList([GPT2Block(c) for _ in range(c.n_layer)])
        self.ln_f = LayerNorm(c.n_embd, c.layer_norm_epsilon)
        # HF scales the residual projections' init by 1 / sqrt(2 n_layer)
        for blk in self.h:
            for lin in (blk.attn_out, blk.fc2):
                nn.init.normal_(lin.weight, 0.0, c.initializer_range / (2 * c.n_layer) ** 0.5)

    # ZeRO-1 gather waits (parallel/ddp.py): the root's forward reads both tables directly
    _ddl_direct_reads = ("wte", "wpe")

    def forward(self, input_ids, attention_mask=None, token_type_ids=None, labels=None, position_ids=None):
        """``token_type_ids`` is ignored (GPT-2 has none): it keeps the training loop's
        ``(input_ids, attention_mask, token_type_ids, labels)`` call form.
        Returns ``(loss, None)`` with labels -- the fused head never hands out the logits -- and the
        ``[B, S, vocab]`` logits without.

        ``position_ids`` (int ``[B, S]``, HF's packed-sequence convention: 0 at the first token of every
        document, previous + 1 otherwise) makes each row several documents: ``wpe`` is read at these
        positions and no token attends across a boundary.  The caller sets the label of each document's last
        token to -100."""
        B, S = input_ids.shape
        if S > self.config.n_positions:
            raise ValueError(f"sequence length {S} exceeds n_positions {self.config.n_positions}")
        mask_bias = None
        if attention_mask is not None:
            mask_bias = (1.0 - attention_mask.float()) * -10000.0
        if position_ids is None:
            h = self.drop(self.wte(input_ids) + self.wpe.weight[:S].unsqueeze(0))
            for blk in self.h:
                h = blk(h, mask_bias)
        else:
            if position_ids.shape != input_ids.shape or position_ids.device != input_ids.device:
                raise ValueError(f"position_ids {tuple(position_ids.shape)} on {position_ids.device} must match "
                                 f"input_ids {(B, S)} on {input_ids.device}")
            doc = ops.doc_bounds(position_ids)          # checked once per batch: positions < S <= n_positions
            h = self.drop(self.wte(input_ids) + self.wpe(position_ids))
            for blk in self.h:
                h = blk(h, mask_bias, doc)
        h = self.ln_f(h)
        if labels is not None:
            loss = ops.linear_cross_entropy(h.reshape(-1, h.shape[-1]), self.wte.weight, None, labels.reshape(-1),
                                            -100, defer_weight_ready=True)
            return loss, None
        return ops.linear(h, self.wte.weight, None)

    # ------------------------------------------------------------ generation
    def prefill(self, input_ids, lens, cache: KVCache):
        """Right-padded prompts ``[B, S]`` of lengths ``lens`` (int ``[B]``, on the device) -> the next-token
        logits ``[B, vocab]`` of each sequence's last token; fills ``cache`` and sets its lengths.  The head
        runs on those B rows only: the ``[B, S, vocab]`` logits never exist."""
        B, S = input_ids.shape
        if S > cache.capacity:
            raise ValueError(f"prompt length {S} exceeds the cache capacity {cache.capacity}")
        with torch.no_grad():
            lens = lens.to(device=input_ids.device, dtype=torch.int32)
            keep = torch.arange(S, device=input_ids.device)[None, :] < lens[:, None]
            mask_bias = (1.0 - keep.float()) * -10000.0
            h = self.wte(input_ids) + self.wpe.weight[:S].unsqueeze(0)
            for i, blk in enumerate(self.h):
                h = blk.prefill(h, mask_bias, cache, i)
            last = h[torch.arange(B, device=h.device), (lens - 1).long()]
            cache.lens.copy_(lens)
            cache.max_len = S
            return ops.linear_small_m(self.ln_f(last), self.wte.weight, None)

    def extend(self, input_ids, cache: KVCache, new_lens=None, all_logits: bool = False):
        """``input_ids [B, T]``: the tokens at positions ``cache.lens + 0 .. T-1`` of each sequence, right-padded
        to T, of which row b's first ``new_lens[b]`` are real (int ``[B]`` on the device; default T) -> the
        next-token logits ``[B, vocab]`` at each row's last new token (the head runs on those B rows only), or
        with ``all_logits`` the ``[B, T, vocab]`` logits of every column (padded ones are meaningless).  Every
        layer appends the real tokens' keys / values; then ``cache.lens += new_lens`` and ``cache.max_len +=
        T``.  From an empty cache this is ``prefill``.

        ``new_lens[b] == 0`` is allowed: the row is handed one dead column (the attention wants at least one
        query per row), whose key / value land at position ``lens[b]`` -- which stays dead, since the row's
        length does not advance, and is overwritten by the row's next real token.  Its logits are meaningless."""
        B, T = input_ids.shape
        if T < 1:
            raise ValueError("extend needs at least one column")
        if cache.max_len + T > cache.capacity:
            raise ValueError(f"max_len {cache.max_len} + {T} new columns exceeds the cache capacity {cache.capacity}")
        with torch.no_grad():
            dev = input_ids.device
            adv = q_lens = None
            if new_lens is not None:
                adv = new_lens.to(device=dev, dtype=torch.int32).clamp(0, T)
                q_lens = adv.clamp(min=1)
            # positions lens + i, read on the device; a padded column's may pass the table: clamped
            pos = cache.lens.long()[:, None] + torch.arange(T, device=dev)[None, :]
            h = self.wte(input_ids) + self.wpe(pos.clamp(max=self.config.n_positions - 1))
            for i, blk in enumerate(self.h):
                h = blk.extend(h, cache, i, q_lens)
            if all_logits:
                logits = ops.linear(self.ln_f(h), self.wte.weight, None)
            else:
                last = h[:, -1] if q_lens is None else h[torch.arange(B, device=dev), (q_lens - 1).long()]
                logits = ops.linear_small_m(self.ln_f(last), self.wte.weight, None)
            cache.lens += T if adv is None else adv
            cache.max_len += T
            return logits

    def _consume_prompt(self, ids, cnt, cache: KVCache, prefix=None, prefill_chunk=None):
        """The right-padded prompts ``ids [B, S0]`` of lengths ``cnt`` into ``cache`` -> each row's next-token
        logits.  Neither option: ``prefill``.  Otherwise the cache starts from ``prefix`` (or empty) and takes
        the prompt through ``extend`` in chunks of ``prefill_chunk`` columns (default: all at once).  A row
        whose prompt ended before a chunk passes ``new_lens = 0`` there (see ``extend``) and keeps the logits
        of the chunk that held its last token."""
        if prefix is None and prefill_chunk is None:
            return self.prefill(ids, cnt, cache)
        if prefix is not None:
            cache.copy_prefix_(prefix)
        else:
            cache.lens.zero_()
            cache.max_len = 0
        S0 = ids.shape[1]
        step = S0 if prefill_chunk is None else prefill_chunk
        logits = None
        for c0 in range(0, S0, step):
            T = min(step, S0 - c0)
            new = self.extend(ids[:, c0:c0 + T], cache, (cnt - c0).clamp(0, T))
            logits = new if logits is None else torch.where((cnt > c0)[:, None], new, logits)
        return logits

    def decode_step(self, tokens, cache: KVCache, len_bound=None):
        """``tokens [B]``: the token at position ``cache.lens`` of each sequence -> the next-token logits
        ``[B, vocab]``.  Every layer appends to the cache; the lengths advance once, after the last.
        ``len_bound`` (default ``cache.max_len + 1``): the bound on ``lens + 1`` handed to the attention
        launches; with ``cache.capacity`` every step launches the same grid (positions past ``lens`` are
        still never loaded)."""
        if cache.max_len + 1 > cache.capacity:
            raise ValueError(f"max_len {cache.max_len + 1} exceeds the cache capacity {cache.capacity}")
        if len_bound is not None and not cache.max_len + 1 <= len_bound <= cache.capacity:
            raise ValueError(f"len_bound {len_bound} must be in max_len + 1 ({cache.max_len + 1}) .. the cache "
                             f"capacity ({cache.capacity})")
        with torch.no_grad():
            h = self.wte(tokens) + self.wpe(cache.lens.long())
            for i, blk in enumerate(self.h):
                h = blk.decode(h, cache, i, len_bound)
            cache.lens += 1
            cache.max_len += 1
            return ops.linear_small_m(self.ln_f(h), self.wte.weight, None)

    @torch.no_grad()
    def generate(self, input_ids, attention_mask=None, max_new_tokens: int = 20, do_sample: bool = False,
                 temperature: float = 1.0, top_k=None, eos_token_id=None, pad_token_id=None, generator=None,
                 use_graph: bool = False, prefix: KVCache = None, prefill_chunk: int = None, top_p=None, min_p=None,
                 repetition_penalty=None):
        """Greedy (argmax) or sampled (temperature, then top-k, then multinomial) continuation of
        ``input_ids [B, S_in]`` -> ``[B, S_in + n_new]``: each row as given, then its generated tokens, with
        ``pad_token_id`` (default ``eos_token_id``) after the first ``eos_token_id``.  ``attention_mask``
        rows must each be one contiguous run of ones (left- or right-padded).  Always eval semantics (no
        dropout).  Stops early once every row has produced ``eos_token_id``: that check is the only host
        sync of a step and is made only when ``eos_token_id`` is given.

        ``use_graph=True``: the decode step runs from a session cached on the model
        (``models/_decode_graph.py``): its state lives on the device, tokens are chosen by
        ``ops.next_token``, and on a GPU with the native kernels and bf16 parameters the whole step is one
        captured graph, replayed once per token (captured on the first call of a shape; rebuilt when the
        batch, the rounded cache capacity or a parameter's storage changes).  Elsewhere the same loop runs
        eagerly through the reference ops.  Greedy output equals ``use_graph=False``'s.  With ``do_sample``
        the tokens follow ``ops.next_token``'s definition from one ``torch.rand(max_new_tokens, B,
        generator=generator)`` drawn before the loop: the same distribution as the ``torch.multinomial``
        path, but NOT its token stream for a given generator.  The eos check syncs only every 16 steps; the
        result is trimmed to the length ``use_graph=False`` returns.

        ``top_p`` (nucleus), ``min_p`` and ``repetition_penalty`` are ``ops.next_token``'s, applied in HF's
        order (penalty, temperature, top-k, top-p, min-p) and defined by value, so ties at a cut are kept;
        the penalty counts a row's prompt and its generated tokens (not the tokens of a ``prefix`` cache), and
        applies to greedy too.  Left at None, every path gives the tokens it gave without them.

        ``prefix``: a ``KVCache`` (of batch B, or of batch 1 and shared by every row) that already holds the
        tokens before ``input_ids``, e.g. a system prompt prefilled once: it is copied into this call's own
        cache, never modified, and the prompt is consumed by ``extend`` on top of it.  ``prefill_chunk``: the
        prompt is consumed in chunks of that many columns through ``extend`` (the first one included), which
        bounds the prompt's activations by the chunk.  Without either, the prompt goes through ``prefill``."""
        B, S_in = input_ids.shape
        G.check_sampling(max_new_tokens, do_sample, temperature, top_k, top_p, min_p, repetition_penalty)
        ext = top_p is not None or min_p is not None or repetition_penalty is not None
        if prefill_chunk is not None and prefill_chunk < 1:
            raise ValueError("prefill_chunk must be at least 1")
        P0 = 0 if prefix is None else prefix.max_len
        if P0 + S_in + max_new_tokens > self.config.n_positions:
            raise ValueError(f"{'prefix + ' if prefix is not None else ''}S_in + max_new_tokens = "
                             f"{P0 + S_in + max_new_tokens} exceeds n_positions {self.config.n_positions}")
        dev = input_ids.device
        ids, cnt, S0 = G.compact_prompts(input_ids, attention_mask)
        if pad_token_id is None:
            pad_token_id = eos_token_id
        need = P0 + S0 + max_new_tokens
        was_training = self.training
        self.eval()
        try:
            if use_graph:
                from ._decode_graph import round_capacity, session_for
                sess = session_for(self, B, round_capacity(need, self.config.n_positions),
                                   G.use_graph_for(self.wte.weight), ext)
                new = G.session_loop(sess, lambda cache: self._consume_prompt(ids, cnt, cache, prefix, prefill_chunk),
                                     B, dev, max_new_tokens, do_sample, temperature, top_k, eos_token_id,
                                     pad_token_id, generator, top_p, min_p, repetition_penalty,
                                     ids if ext else None, cnt if ext else None)
            else:
                cache = KVCache.allocate(self, B, need, dev)
                logits = self._consume_prompt(ids, cnt, cache, prefix, prefill_chunk)
                new = G.token_loop(logits, lambda tok: self.decode_step(tok, cache), max_new_tokens, do_sample,
                                   temperature, top_k, eos_token_id, pad_token_id, generator, top_p, min_p,
                                   repetition_penalty, ids, cnt)
        finally:
            self.train(was_training)
        return torch.cat([input_ids, new.to(input_ids.dtype)], 1)

    @property
    def decode_session(self):
        """The session ``generate(use_graph=True)`` last used on this model (None before the first)."""
        from ._decode_graph import current_session
        return current_session(self)

    # what a decode session (models/_decode_graph.py) asks of its model
    def _session_weight(self):
        return self.wte.weight

    def _session_cache(self, batch, capacity, device):
        return KVCache.allocate(self, batch, capacity, device)

    def _session_logits(self, tok_cur, cache: KVCache):
        h = ops.decode_embed(tok_cur, cache.lens, self.wte.weight, self.wpe.weight)
        for i, blk in enumerate(self.h):
            h = blk.decode(h, cache, i, len_bound=cache.capacity)
        return ops.linear_small_m(self.ln_f(h), self.wte.weight, None)


def _make(dropout: float, activation_function: str, **kw) -> GPT2LMHeadModel:
    return GPT2LMHeadModel(GPT2Config(resid_pdrop=dropout, embd_pdrop=dropout, attn_pdrop=dropout,
                                      activation_function=activation_function, **kw))


def gpt2(dropout: float = 0.1, activation_function: str = "gelu", **kw) -> GPT2LMHeadModel:
    return _make(dropout, activation_function, **kw)


def gpt2_medium(dropout: float = 0.1, activation_function: str = "gelu", **kw) -> GPT2LMHeadModel:
    d = dict(n_embd=1024, n_layer=24, n_head=16)
    d.update(kw)
    return _make(dropout, activation_function, **d)


def gpt2_large(dropout: float = 0.1, activation_function: str = "gelu", **kw) -> GPT2LMHeadModel:
    d = dict(n_embd=1280, n_layer=36, n_head=20)
    d.update(kw)
    return _make(dropout, activation_function, **d)


def gpt2_tiny(dropout: float = 0.1, activation_function: str = "gelu", **kw) -> GPT2LMHeadModel:
    """2 layers, hidden 128, 2 heads (head dim 64), vocabulary 1000: the GPT-2 code path at test size."""
    d = dict(n_embd=128, n_layer=2, n_head=2, vocab_size=1000, n_positions=128)
    d.update(kw)
    return _make(dropout, activation_function, **d)


# ------------------------------------------------------------ HF conversion
# HF GPT-2 linears are ``Conv1D``: weight [in, out] (ours: [out, in]); ``c_attn`` is the fused QKV
# in our [q | k | v] order; ``lm_head.weight`` is the tied ``wte``; ``attn.bias`` /
# ``attn.masked_bias`` are HF's causal-mask buffers.
_HF_LINEAR = {"attn.c_attn": "qkv", "attn.c_proj": "attn_out", "mlp.c_fc": "fc1", "mlp.c_proj": "fc2"}
_HF_NORM = {"ln_1": "ln_1", "ln_2": "ln_2"}


def from_hf_state_dict(sd: dict, num_layers: int) -> dict:
    """HF ``GPT2LMHeadModel`` state dict -> this model's."""
    out = {"wte.weight": sd["transformer.wte.weight"], "wpe.weight": sd["transformer.wpe.weight"],
           "ln_f.weight": sd["transformer.ln_f.weight"], "ln_f.bias": sd["transformer.ln_f.bias"]}
    if "lm_head.weight" in sd and not torch.equal(sd["lm_head.weight"], sd["transformer.wte.weight"]):
        raise ValueError("lm_head.weight is not tied to transformer.wte.weight: this model shares the two")
    for i in range(num_layers):
        p = f"transformer.h.{i}."
        for hf, ours in _HF_LINEAR.items():
            out[f"h.{i}.{ours}.weight"] = sd[p + hf + ".weight"].t().contiguous()
            out[f"h.{i}.{ours}.bias"] = sd[p + hf + ".bias"]
        for hf, ours in _HF_NORM.items():
            for t in ("weight", "bias"):
                out[f"h.{i}.{ours}.{t}"] = sd[p + f"{hf}.{t}"]
    return out


def to_hf_state_dict(sd: dict, num_layers: int) -> dict:
    out = {"transformer.wte.weight": sd["wte.weight"], "transformer.wpe.weight": sd["wpe.weight"],
           "transformer.ln_f.weight": sd["ln_f.weight"], "transformer.ln_f.bias": sd["ln_f.bias"],
           "lm_head.weight": sd["wte.weight"]}
    for i in range(num_layers):
        p = f"transformer.h.{i}."
        for hf, ours in _HF_LINEAR.items():
            out[p + hf + ".weight"] = sd[f"h.{i}.{ours}.weight"].t().contiguous()
            out[p + hf + ".bias"] = sd[f"h.{i}.{ours}.bias"]
        for hf, ours in _HF_NORM.items():
            for t in ("weight", "bias"):
                out[p + f"{hf}.{t}"] = sd[f"h.{i}.{ours}.{t}"]
    return out
