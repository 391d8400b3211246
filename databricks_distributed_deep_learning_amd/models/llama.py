"""Llama-family causal language model: RMSNorm, rotary positions, grouped-query attention, SwiGLU, no biases.

Parameter-for-parameter equivalent to HF ``LlamaForCausalLM`` (SmolLM-135M: 134,515,008 parameters); the
q / k / v projections are stored fused (``qkv``, rows ``[q | k | v]``) and so are gate / up (``gate_up``).
The blocks are ``GPT2Block``'s no-dropout wiring -- residual adds in the output GEMMs' epilogues, the
residual-stream gradient bridged into each RMSNorm backward -- with ``ops.rms_norm`` for the norms,
``ops.rope_qkv`` between the projection and ``ops.attention(causal=True)`` (it rotates q and k and repeats each
k / v head to its query heads, so the attention kernels see the packed ``[B, S, 3 H D]`` they were written for)
and ``ops.swiglu`` between the two MLP GEMMs.  The head is the token embedding (tied) or a separate bias-free
``lm_head`` and, with labels, the fused vocabulary head + loss (``ops.linear_cross_entropy``).

Labels are NOT shifted here (the GPT-2 convention): ``labels[b, s]`` is the token at ``s + 1``.

Head dimension 64 takes the native kernels; any other even head dimension runs through the references of
``ops.rope_qkv`` and ``ops.attention``.

Generation (``generate``, GPT-2's contract): ``prefill`` runs the causal forward once over the right-padded
prompts, copies every layer's rotated keys and its values into a ``LlamaKVCache`` -- ``[L, 2, B, Hkv, C, D]``:
the Hkv key / value heads, never expanded to the H query heads -- and applies the head to each sequence's last
row only; ``decode_step`` then feeds one token per sequence through ``LlamaBlock.decode``: the M <= 16
weight-streaming linears (``ops.linear_small_m``) and ``ops.attention_decode_gqa``, which rotates the new
token's queries and key by the row's own position, scores every cached row once against the G query heads of
its group and appends.  ``generate(use_graph=True)`` runs the step from a decode session
(``models/_decode_graph.py``): captured once into a hipGraph and replayed per token.

``extend`` adds a chunk of T tokens per sequence to a cache that already holds something
(``ops.attention_extend_gqa``: the chunk is rotated by each row's own positions inside the attention kernel --
there is no position embedding to add); ``generate(prefix=...)`` starts from a copy of a prefilled cache and
``prefill(chunk=...)`` consumes a prompt through ``extend`` in chunks.

Not covered: ``generate(prefill_chunk=...)`` (chunked prompt consumption is on ``prefill``), ``rope_scaling``,
sliding-window attention, biased projections.
"""
from __future__ import annotations

from dataclasses import dataclass

import torch
import torch.nn as nn

from .. import ops
from ..ops.bridge import GradBridge
from . import _generate as G
from .layers import Embedding, Linear


@dataclass
class LlamaConfig:
    vocab_size: int = 49152
    hidden_size: int = 576
    intermediate_size: int = 1536
    num_hidden_layers: int = 30
    num_attention_heads: int = 9
    num_key_value_heads: int = 3
    max_position_embeddings: int = 2048
    rms_norm_eps: float = 1e-5
    rope_theta: float = 10000.0
    tie_word_embeddings: bool = True
    initializer_range: float = 0.02


class RMSNorm(nn.Module):
    def __init__(self, d: int, eps: float = 1e-5):
        super().__init__()
        self.d, self.eps = d, eps
        self.weight = nn.Parameter(torch.ones(d))

    def forward(self, x, grad_from=None):
        return ops.rms_norm(x, self.weight, self.eps, grad_from=grad_from)

    def extra_repr(self):
        return f"{self.d}, eps={self.eps}"


class LlamaKVCache:
    """Rotated keys and values of every layer, ``data [L, 2, B, Hkv, C, D]`` (C: capacity in positions), the
    valid length of each batch row on the device (``lens``, int32 ``[B]``) and ``max_len``, the host's upper
    bound on ``lens`` -- what sizes the decode launches, so no step reads ``lens`` back."""

    def __init__(self, data: torch.Tensor, lens: torch.Tensor):
        self.data, self.lens = data, lens
        self.capacity = data.shape[4]
        self.max_len = 0

    @classmethod
    def allocate(cls, model: "LlamaForCausalLM", batch: int, capacity: int, device=None,
                 dtype=None) -> "LlamaKVCache":
        c = model.config
        if not 1 <= capacity <= c.max_position_embeddings:
            raise ValueError(f"capacity {capacity} must be in 1 .. max_position_embeddings "
                             f"({c.max_position_embeddings})")
        w = model.embed_tokens.weight
        device = w.device if device is None else device
        data = torch.empty(c.num_hidden_layers, 2, batch, c.num_key_value_heads, capacity,
                           c.hidden_size // c.num_attention_heads, dtype=w.dtype if dtype is None else dtype,
                           device=device)
        return cls(data, torch.zeros(batch, dtype=torch.int32, device=device))

    def k(self, layer: int) -> torch.Tensor:
        return self.data[layer, 0]

    def v(self, layer: int) -> torch.Tensor:
        return self.data[layer, 1]

    def copy_prefix_(self, src: "LlamaKVCache") -> "LlamaKVCache":
        """Start this cache from ``src``'s contents: positions ``< src.max_len`` of every layer, ``lens`` and
        ``max_len``.  ``src`` has this cache's batch or batch 1 (one prefix shared by every row), its dtype and
        its device (nothing is converted or moved silently); it is only read.  Rows of ``src`` may have unequal
        ``lens``: ``src.max_len``, their bound, is what is copied and what ``generate`` counts against
        ``max_position_embeddings``."""
        L, _, B, H, C, D = self.data.shape
        Ls, _, Bs, Hs, _, Ds = src.data.shape
        if (Ls, Hs, Ds) != (L, H, D):
            raise ValueError(f"prefix cache has {Ls} layers of {Hs} KV heads x {Ds}, this one {L} of {H} x {D}")
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


class LlamaBlock(nn.Module):
    def __init__(self, c: LlamaConfig):
        super().__init__()
        E, std = c.hidden_size, c.initializer_range
        self.num_heads, self.num_kv_heads = c.num_attention_heads, c.num_key_value_heads
        D = E // self.num_heads
        self.input_layernorm = RMSNorm(E, c.rms_norm_eps)
        self.qkv = Linear(E, (self.num_heads + 2 * self.num_kv_heads) * D, bias=False, init_std=std)
        self.o_proj = Linear(self.num_heads * D, E, bias=False, init_std=std)
        self.post_attention_layernorm = RMSNorm(E, c.rms_norm_eps)
        self.gate_up = Linear(E, 2 * c.intermediate_size, bias=False, init_std=std)
        self.down_proj = Linear(c.intermediate_size, E, bias=False, init_std=std)

    def forward(self, h, table, mask=None, positions=None, doc=None):
        """``positions`` / ``doc`` (packed rows): the int32 rotary positions and ``ops.doc_bounds``' pair."""
        bridged = torch.is_grad_enabled() and h.requires_grad
        b1 = GradBridge() if bridged else None
        y = self.input_layernorm(h, grad_from=b1)
        if doc is None:
            qkv = ops.rope_qkv(self.qkv(y), table, self.num_heads, self.num_kv_heads)
            ctx = ops.attention(qkv, self.num_heads, mask, 0.0, self.training, causal=True)
        else:
            qkv = ops.rope_qkv(self.qkv(y), table, self.num_heads, self.num_kv_heads, positions=positions)
            ctx = ops.attention(qkv, self.num_heads, mask, 0.0, self.training, causal=True, doc_start=doc)
        h = self.o_proj(ctx, residual=h, residual_grad_to=b1)
        b2 = GradBridge() if bridged else None
        y = self.post_attention_layernorm(h, grad_from=b2)
        return self.down_proj(ops.swiglu(self.gate_up(y)), residual=h, residual_grad_to=b2)

    def prefill(self, h, table, mask, cache: LlamaKVCache, layer: int):
        """The inference forward that also copies this layer's rotated keys and its values into the cache."""
        qkv = ops.rope_qkv(self.qkv(self.input_layernorm(h)), table, self.num_heads, self.num_kv_heads)
        ops.kv_cache_fill_gqa(qkv, cache.k(layer), cache.v(layer), self.num_heads, self.num_kv_heads)
        h = self.o_proj(ops.attention(qkv, self.num_heads, mask, 0.0, False, causal=True), residual=h)
        return self.down_proj(ops.swiglu(self.gate_up(self.post_attention_layernorm(h))), residual=h)

    def decode(self, h_new, table, cache: LlamaKVCache, layer: int, len_bound=None):
        """One new token per sequence, ``h_new [B, E]``, against the cache (which gains its rotated key and
        its value).  ``len_bound``: the bound on ``lens + 1`` that sizes the attention launch (default
        ``max_len + 1``)."""
        lin = ops.linear_small_m
        qkv = lin(self.input_layernorm(h_new), self.qkv.weight, None)
        ctx = ops.attention_decode_gqa(qkv, table, cache.k(layer), cache.v(layer), cache.lens, self.num_heads,
                                       self.num_kv_heads, cache.max_len + 1 if len_bound is None else len_bound)
        return self._small_m_tail(ctx, h_new)

    def _small_m_tail(self, ctx, h):
        """Output projection and MLP of a block on M <= 16 rows (``ops.linear_small_m``)."""
        lin = ops.linear_small_m
        h = lin(ctx, self.o_proj.weight, None, residual=h)
        z = ops.swiglu(lin(self.post_attention_layernorm(h), self.gate_up.weight, None))
        return lin(z, self.down_proj.weight, None, residual=h)

    def extend(self, h, table, cache: LlamaKVCache, layer: int, new_lens=None, len_bound=None):
        """A chunk of new tokens per sequence, ``h [B, T, E]``, against the cache, which gains the rotated keys
        and the values of each row's first ``new_lens`` (default T) tokens: ``prefill`` with
        ``ops.attention_extend_gqa`` in place of rope + attention + fill.  ``len_bound``: the bound on ``lens``
        (default ``max_len``).  With ``B T <= 16`` the linears are the weight-streaming ones of ``decode``."""
        small = h.shape[0] * h.shape[1] <= 16
        y = self.input_layernorm(h)
        qkv = ops.linear_small_m(y, self.qkv.weight, None) if small else self.qkv(y)
        ctx = ops.attention_extend_gqa(qkv, table, cache.k(layer), cache.v(layer), cache.lens, self.num_heads,
                                       self.num_kv_heads, cache.max_len if len_bound is None else len_bound,
                                       new_lens)
        if small:
            return self._small_m_tail(ctx, h)
        h = self.o_proj(ctx, residual=h)
        return self.down_proj(ops.swiglu(self.gate_up(self.post_attention_layernorm(h))), residual=h)


class LlamaForCausalLM(nn.Module):
    def __init__(self, c: LlamaConfig):
        super().__init__()
        if c.hidden_size % c.num_attention_heads:
            raise ValueError("hidden_size must be a multiple of num_attention_heads")
        if c.num_key_value_heads < 1 or c.num_attention_heads % c.num_key_value_heads:
            raise ValueError("num_attention_heads must be a multiple of num_key_value_heads")
        D = c.hidden_size // c.num_attention_heads
        if D % 2:
            raise ValueError("the head dimension must be even (rotary pairs)")
        self.config = c
        self.embed_tokens = Embedding(c.vocab_size, c.hidden_size, c.initializer_range)
        self.layers = nn.ModuleList([LlamaBlock(c) for _ in range(c.num_hidden_layers)])
        self.norm = RMSNorm(c.hidden_size, c.rms_norm_eps)
        self.lm_head = None
        if not c.tie_word_embeddings:
            self.lm_head = Linear(c.hidden_size, c.vocab_size, bias=False, init_std=c.initializer_range)
        self.register_buffer("rope_table", ops.rope_table(c.max_position_embeddings, c.rope_theta, D),
                             persistent=False)

    # ZeRO-1 gather waits (parallel/ddp.py): the root's forward reads the embedding and the head's weight
    # directly
    @property
    def _ddl_direct_reads(self):
        return ("embed_tokens",) if self.lm_head is None else ("embed_tokens", "lm_head")

    def _apply(self, fn, recurse=True):
        # the rotary table stays fp32 when the module is cast to bf16
        super()._apply(fn, recurse)
        if self.rope_table.dtype != torch.float32:
            c = self.config
            self.rope_table = ops.rope_table(c.max_position_embeddings, c.rope_theta,
                                             c.hidden_size // c.num_attention_heads, self.rope_table.device)
        return self

    def head_weight(self) -> torch.Tensor:
        return self.embed_tokens.weight if self.lm_head is None else self.lm_head.weight

    def forward(self, input_ids, attention_mask=None, token_type_ids=None, labels=None, position_ids=None):
        """``token_type_ids`` is ignored: it keeps the training loop's ``(input_ids, attention_mask,
        token_type_ids, labels)`` call form.  Returns ``(loss, None)`` with labels -- the fused head never
        hands out the logits -- and the ``[B, S, vocab]`` logits without.

        ``position_ids`` (int ``[B, S]``, HF's packed-sequence convention: 0 at the first token of every
        document, previous + 1 otherwise) makes each row several documents: rotary positions restart and no
        token attends across a boundary.  The caller sets the label of each document's last token to -100."""
        B, S = input_ids.shape
        if S > self.config.max_position_embeddings:
            raise ValueError(f"sequence length {S} exceeds max_position_embeddings "
                             f"{self.config.max_position_embeddings}")
        mask_bias = None
        if attention_mask is not None:
            mask_bias = (1.0 - attention_mask.float()) * -10000.0
        h = self.embed_tokens(input_ids)
        if position_ids is None:
            for blk in self.layers:
                h = blk(h, self.rope_table, mask_bias)
        else:
            if position_ids.shape != input_ids.shape or position_ids.device != input_ids.device:
                raise ValueError(f"position_ids {tuple(position_ids.shape)} on {position_ids.device} must match "
                                 f"input_ids {(B, S)} on {input_ids.device}")
            doc = ops.doc_bounds(position_ids)          # checked once per batch: positions < S <= the table's rows
            positions = position_ids.to(torch.int32).contiguous()
            for blk in self.layers:
                h = blk(h, self.rope_table, mask_bias, positions, doc)
        h = self.norm(h)
        w = self.head_weight()
        if labels is not None:
            loss = ops.linear_cross_entropy(h.reshape(-1, h.shape[-1]), w, None, labels.reshape(-1), -100,
                                            defer_weight_ready=self.lm_head is None)
            return loss, None
        return ops.linear(h, w, None)

    # ------------------------------------------------------------ generation
    def prefill(self, input_ids, lens, cache: LlamaKVCache, chunk: int = None):
        """Right-padded prompts ``[B, S]`` of lengths ``lens`` (int ``[B]``, on the device) -> the next-token
        logits ``[B, vocab]`` of each sequence's last token; fills ``cache`` and sets its lengths.  The head
        runs on those B rows only: the ``[B, S, vocab]`` logits never exist.

        ``chunk``: the prompt is consumed from an empty cache through ``extend`` in chunks of that many
        columns, which bounds the prompt's activations by the chunk.  A row whose prompt ended before a chunk
        passes ``new_lens = 0`` there and keeps the logits of the chunk that held its last token;
        ``cache.max_len`` ends at S either way."""
        B, S = input_ids.shape
        if S > cache.capacity:
            raise ValueError(f"prompt length {S} exceeds the cache capacity {cache.capacity}")
        if chunk is not None:
            if chunk < 1:
                raise ValueError("chunk must be at least 1")
            with torch.no_grad():
                cache.lens.zero_()
                cache.max_len = 0
                return self._extend_chunks(input_ids, lens.to(device=input_ids.device, dtype=torch.int32), cache,
                                           chunk)
        with torch.no_grad():
            lens = lens.to(device=input_ids.device, dtype=torch.int32)
            keep = torch.arange(S, device=input_ids.device)[None, :] < lens[:, None]
            mask_bias = (1.0 - keep.float()) * -10000.0
            h = self.embed_tokens(input_ids)
            for i, blk in enumerate(self.layers):
                h = blk.prefill(h, self.rope_table, mask_bias, cache, i)
            last = h[torch.arange(B, device=h.device), (lens - 1).long()]
            cache.lens.copy_(lens)
            cache.max_len = S
            return ops.linear_small_m(self.norm(last), self.head_weight(), None)

    def extend(self, input_ids, cache: LlamaKVCache, new_lens=None, all_logits: bool = False):
        """``input_ids [B, T]``: the tokens at positions ``cache.lens + 0 .. T-1`` of each sequence, right-padded
        to T, of which row b's first ``new_lens[b]`` are real (int ``[B]`` on the device; default T) -> the
        next-token logits ``[B, vocab]`` at each row's last new token (the head runs on those B rows only), or
        with ``all_logits`` the ``[B, T, vocab]`` logits of every column (padded ones are meaningless).  Every
        layer appends the real tokens' rotated keys and their values; then ``cache.lens += new_lens`` and
        ``cache.max_len += T``.  From an empty cache this is ``prefill``.  Positions enter only through the
        rotary table rows the attention kernel reads (``lens[b] + i``, on the device).

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
            h = self.embed_tokens(input_ids)
            for i, blk in enumerate(self.layers):
                h = blk.extend(h, self.rope_table, cache, i, q_lens)
            if all_logits:
                logits = ops.linear(self.norm(h), self.head_weight(), None)
            else:
                last = h[:, -1] if q_lens is None else h[torch.arange(B, device=dev), (q_lens - 1).long()]
                logits = ops.linear_small_m(self.norm(last), self.head_weight(), None)
            cache.lens += T if adv is None else adv
            cache.max_len += T
            return logits

    def _extend_chunks(self, ids, cnt, cache: LlamaKVCache, step: int):
        """The right-padded prompts ``ids [B, S0]`` of lengths ``cnt`` on top of what ``cache`` holds, through
        ``extend`` in chunks of ``step`` columns -> each row's next-token logits (those of the chunk that held
        its last token; a row whose prompt ended before a chunk passes ``new_lens = 0`` there)."""
        S0 = ids.shape[1]
        logits = None
        for c0 in range(0, S0, step):
            T = min(step, S0 - c0)
            new = self.extend(ids[:, c0:c0 + T], cache, (cnt - c0).clamp(0, T))
            logits = new if logits is None else torch.where((cnt > c0)[:, None], new, logits)
        return logits

    def _consume_prompt(self, ids, cnt, cache: LlamaKVCache, prefix=None):
        """The right-padded prompts into ``cache`` -> each row's next-token logits: ``prefill``, or with
        ``prefix`` a copy of it extended by the whole prompt."""
        if prefix is None:
            return self.prefill(ids, cnt, cache)
        cache.copy_prefix_(prefix)
        return self._extend_chunks(ids, cnt, cache, ids.shape[1])

    def decode_step(self, tokens, cache: LlamaKVCache, len_bound=None):
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
            logits = self._step_logits(tokens, cache, len_bound)
            cache.lens += 1
            cache.max_len += 1
            return logits

    def _step_logits(self, tokens, cache: LlamaKVCache, len_bound):
        h = self.embed_tokens(tokens)
        for i, blk in enumerate(self.layers):
            h = blk.decode(h, self.rope_table, cache, i, len_bound)
        return ops.linear_small_m(self.norm(h), self.head_weight(), None)

    @torch.no_grad()
    def generate(self, input_ids, attention_mask=None, max_new_tokens: int = 20, do_sample: bool = False,
                 temperature: float = 1.0, top_k=None, eos_token_id=None, pad_token_id=None, generator=None,
                 use_graph: bool = False, prefix: LlamaKVCache = None, top_p=None, min_p=None,
                 repetition_penalty=None):
        """Greedy (argmax) or sampled (temperature, then top-k, then multinomial) continuation of
        ``input_ids [B, S_in]`` -> ``[B, S_in + n_new]``: ``GPT2LMHeadModel.generate``'s contract.  Each row
        as given, then its generated tokens, with ``pad_token_id`` (default ``eos_token_id``) after the first
        ``eos_token_id``.  ``attention_mask`` rows must each be one contiguous run of ones (left- or
        right-padded); the prompts are compacted to right-padded, so row b's rotary positions start at 0 --
        what HF's ``position_ids`` from the mask give.  Always eval semantics.  Stops early once every row has
        produced ``eos_token_id``: that check is the only host sync of a step and is made only when
        ``eos_token_id`` is given.

        ``use_graph=True``: the decode step runs from a session cached on the model
        (``models/_decode_graph.py``): state on the device, tokens chosen by ``ops.next_token``, and on a GPU
        with the native kernels and bf16 parameters the whole step is one captured graph, replayed once per
        token (captured on the first call of a shape; rebuilt when the batch, the rounded cache capacity or a
        parameter's storage changes).  Elsewhere the same loop runs eagerly.  Greedy output equals
        ``use_graph=False``'s; with ``do_sample`` the tokens follow ``ops.next_token``'s definition from one
        ``torch.rand(max_new_tokens, B, generator=generator)`` drawn before the loop.  The eos check syncs
        only every 16 steps; the result is trimmed to the length ``use_graph=False`` returns.

        ``top_p`` (nucleus), ``min_p`` and ``repetition_penalty`` are ``ops.next_token``'s, applied in HF's
        order (penalty, temperature, top-k, top-p, min-p) and defined by value, so ties at a cut are kept;
        the penalty counts a row's prompt and its generated tokens (not the tokens of a ``prefix`` cache), and
        applies to greedy too.  Left at None, every path gives the tokens it gave without them.

        ``prefix``: a ``LlamaKVCache`` (of batch B, or of batch 1 and shared by every row) that already holds
        the tokens before ``input_ids``, e.g. a system prompt prefilled once: it is copied into this call's
        own cache (the session's, under ``use_graph``), never modified, and the prompt is consumed by
        ``extend`` on top of it, so row b's prompt starts at rotary position ``prefix.lens[b]``."""
        B, S_in = input_ids.shape
        G.check_sampling(max_new_tokens, do_sample, temperature, top_k, top_p, min_p, repetition_penalty)
        ext = top_p is not None or min_p is not None or repetition_penalty is not None
        n_pos = self.config.max_position_embeddings
        P0 = 0 if prefix is None else prefix.max_len
        if P0 + S_in + max_new_tokens > n_pos:
            raise ValueError(f"{'prefix + ' if prefix is not None else ''}S_in + max_new_tokens = "
                             f"{P0 + S_in + max_new_tokens} exceeds max_position_embeddings {n_pos}")
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
                sess = session_for(self, B, round_capacity(need, n_pos),
                                   G.use_graph_for(self.embed_tokens.weight), ext)
                new = G.session_loop(sess, lambda cache: self._consume_prompt(ids, cnt, cache, prefix), B, dev,
                                     max_new_tokens, do_sample, temperature, top_k, eos_token_id, pad_token_id,
                                     generator, top_p, min_p, repetition_penalty, ids if ext else None,
                                     cnt if ext else None)
            else:
                cache = LlamaKVCache.allocate(self, B, need, dev)
                new = G.token_loop(self._consume_prompt(ids, cnt, cache, prefix),
                                   lambda tok: self.decode_step(tok, cache), max_new_tokens, do_sample,
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
        return self.embed_tokens.weight

    def _session_cache(self, batch, capacity, device):
        return LlamaKVCache.allocate(self, batch, capacity, device)

    def _session_logits(self, tok_cur, cache: LlamaKVCache):
        return self._step_logits(tok_cur, cache, cache.capacity)


def _make(**kw) -> LlamaForCausalLM:
    return LlamaForCausalLM(LlamaConfig(**kw))


def llama_tiny(**kw) -> LlamaForCausalLM:
    """2 layers, hidden 128, 2 heads over 1 KV head (head dim 64), vocabulary 1000: the code path at test size."""
    d = dict(hidden_size=128, num_hidden_layers=2, num_attention_heads=2, num_key_value_heads=1,
             intermediate_size=352, vocab_size=1000, max_position_embeddings=256)
    d.update(kw)
    return _make(**d)


def smollm_135m(**kw) -> LlamaForCausalLM:
    return _make(**kw)


def smollm_360m(**kw) -> LlamaForCausalLM:
    d = dict(hidden_size=960, num_hidden_layers=32, num_attention_heads=15, num_key_value_heads=5,
             intermediate_size=2560)
    d.update(kw)
    return _make(**d)


def smollm_1p7b(**kw) -> LlamaForCausalLM:
    d = dict(hidden_size=2048, num_hidden_layers=24, num_attention_heads=32, num_key_value_heads=32,
             intermediate_size=8192)
    d.update(kw)
    return _make(**d)


# ------------------------------------------------------------ HF conversion
# HF keeps q_proj / k_proj / v_proj and gate_proj / up_proj apart ([out, in] each, as here): their rows
# concatenate into ``qkv.weight`` and ``gate_up.weight``.
_HF_SAME = {"self_attn.o_proj": "o_proj", "mlp.down_proj": "down_proj", "input_layernorm": "input_layernorm",
            "post_attention_layernorm": "post_attention_layernorm"}


def check_hf_config(hf_config) -> None:
    """Raises ``ValueError`` for an HF ``LlamaConfig`` (object or dict) this model does not cover."""
    get = _getter(hf_config)
    # (recent HF versions keep rope_theta in the same dict, with rope_type "default": that is no scaling)
    scaling = get("rope_scaling") or get("rope_parameters")
    if scaling is not None:
        kind = scaling.get("rope_type", scaling.get("type"))
        if kind not in (None, "default") or "factor" in scaling:
            raise ValueError(f"rope_scaling ({kind}) is not supported")
    if get("attention_bias", False) or get("mlp_bias", False):
        raise ValueError("biased projections (attention_bias / mlp_bias) are not supported")


def _getter(hf_config):
    return hf_config.get if isinstance(hf_config, dict) else (lambda k, d=None: getattr(hf_config, k, d))


def config_from_hf(hf_config) -> LlamaConfig:
    """This model's config from an HF ``LlamaConfig`` (object, or the dict of its ``config.json``)."""
    check_hf_config(hf_config)
    get = _getter(hf_config)
    E, H = get("hidden_size"), get("num_attention_heads")
    if get("head_dim") not in (None, E // H):
        raise ValueError("head_dim must be hidden_size / num_attention_heads")
    theta = get("rope_theta")
    if theta is None:
        theta = (get("rope_parameters") or get("rope_scaling") or {}).get("rope_theta", 10000.0)
    return LlamaConfig(vocab_size=get("vocab_size"), hidden_size=E, intermediate_size=get("intermediate_size"),
                       num_hidden_layers=get("num_hidden_layers"), num_attention_heads=H,
                       num_key_value_heads=get("num_key_value_heads") or H,
                       max_position_embeddings=get("max_position_embeddings"), rms_norm_eps=get("rms_norm_eps"),
                       rope_theta=float(theta), tie_word_embeddings=bool(get("tie_word_embeddings", False)),
                       initializer_range=get("initializer_range", 0.02))


def from_hf_state_dict(sd: dict, config: LlamaConfig, hf_config=None) -> dict:
    """HF ``LlamaForCausalLM`` state dict -> this model's (``config``: this model's)."""
    if hf_config is not None:
        check_hf_config(hf_config)
    if any(k.endswith(".bias") for k in sd):
        raise ValueError("biased projections (attention_bias / mlp_bias) are not supported")
    emb = sd["model.embed_tokens.weight"]
    head = sd.get("lm_head.weight")
    out = {"embed_tokens.weight": emb, "norm.weight": sd["model.norm.weight"]}
    if config.tie_word_embeddings:
        if head is not None and not torch.equal(head, emb):
            raise ValueError("tie_word_embeddings is set but lm_head.weight differs from model.embed_tokens.weight")
    else:
        if head is None:
            raise ValueError("tie_word_embeddings is not set but the state dict has no lm_head.weight")
        out["lm_head.weight"] = head
    for i in range(config.num_hidden_layers):
        p, o = f"model.layers.{i}.", f"layers.{i}."
        out[o + "qkv.weight"] = torch.cat([sd[p + f"self_attn.{n}_proj.weight"] for n in "qkv"], 0)
        out[o + "gate_up.weight"] = torch.cat([sd[p + "mlp.gate_proj.weight"], sd[p + "mlp.up_proj.weight"]], 0)
        for hf, ours in _HF_SAME.items():
            out[o + ours + ".weight"] = sd[p + hf + ".weight"]
    return out


def to_hf_state_dict(sd: dict, config: LlamaConfig) -> dict:
    c = config
    D = c.hidden_size // c.num_attention_heads
    nq, nkv = c.num_attention_heads * D, c.num_key_value_heads * D
    out = {"model.embed_tokens.weight": sd["embed_tokens.weight"], "model.norm.weight": sd["norm.weight"],
           "lm_head.weight": sd["embed_tokens.weight"] if c.tie_word_embeddings else sd["lm_head.weight"]}
    for i in range(c.num_hidden_layers):
        p, o = f"model.layers.{i}.", f"layers.{i}."
        q, k, v = sd[o + "qkv.weight"].split([nq, nkv, nkv], 0)
        out[p + "self_attn.q_proj.weight"], out[p + "self_attn.k_proj.weight"] = q.contiguous(), k.contiguous()
        out[p + "self_attn.v_proj.weight"] = v.contiguous()
        g, u = sd[o + "gate_up.weight"].chunk(2, 0)
        out[p + "mlp.gate_proj.weight"], out[p + "mlp.up_proj.weight"] = g.contiguous(), u.contiguous()
        for hf, ours in _HF_SAME.items():
            out[p + hf + ".weight"] = sd[o + ours + ".weight"]
    return out
