"""What the causal LMs' ``generate`` share: the argument checks, the prompt compaction and the two token loops.

A model's ``generate`` checks its own position limit, compacts the prompts, switches to eval, consumes the
prompt into a cache (its own business: ``prefill``, or the ``extend`` paths) and hands the resulting
next-token logits to ``token_loop`` (one ``decode_step`` per token, sampling in plain torch) or
``session_loop`` (the step of a decode session, ``models/_decode_graph.py``).
"""
from __future__ import annotations

import torch

from .. import ops
from ..ops.decode import check_filters, penalise_logits, sampling_kept


def check_sampling(max_new_tokens: int, do_sample: bool, temperature: float, top_k, top_p=None, min_p=None,
                   repetition_penalty=None) -> None:
    if max_new_tokens < 1:
        raise ValueError("max_new_tokens must be at least 1")
    if do_sample and not temperature > 0:
        raise ValueError("temperature must be positive")
    if top_k is not None and top_k < 1:
        raise ValueError("top_k must be at least 1")
    check_filters(top_p, min_p, repetition_penalty)


def compact_prompts(input_ids: torch.Tensor, attention_mask):
    """``(ids [B, S0], cnt int32 [B], S0)``: the prompts right-padded, row b's tokens at columns
    ``0 .. cnt[b]-1`` (so its positions start at 0, whichever side it was padded on), ``S0 = max cnt``.
    ``attention_mask`` rows must each be one contiguous, non-empty run of ones."""
    B, S_in = input_ids.shape
    dev = input_ids.device
    ar = torch.arange(S_in, device=dev)[None, :]
    if attention_mask is None:
        return input_ids, torch.full((B,), S_in, dtype=torch.int32, device=dev), S_in
    m = attention_mask.to(dev) != 0
    cnt = m.sum(1)
    first = m.int().argmax(1)
    run = (ar >= first[:, None]) & (ar < (first + cnt)[:, None])
    if not bool(((run == m).all(1) & (cnt > 0)).all()):
        raise ValueError("each attention_mask row must be one contiguous, non-empty run of ones")
    # compact to right-padded: row b's tokens move to columns 0 .. cnt[b]-1
    ids = input_ids.gather(1, (first[:, None] + ar).clamp(max=S_in - 1))
    ids = torch.where(ar < cnt[:, None], ids, torch.zeros_like(ids))
    S0 = int(cnt.max())
    return ids[:, :S0].contiguous(), cnt.int(), S0


def token_loop(logits, decode_step, max_new_tokens, do_sample, temperature, top_k, eos_token_id, pad_token_id,
               generator, top_p=None, min_p=None, repetition_penalty=None, history=None,
               history_lens=None) -> torch.Tensor:
    """From the prompt's next-token ``logits [B, vocab]``: choose a token, ``decode_step(tok)`` -> the next
    logits, until ``max_new_tokens`` or every row has produced ``eos_token_id`` -> the new tokens ``[B, n]``.
    ``top_p`` / ``min_p`` / ``repetition_penalty`` as ``ops.next_token`` defines them (by value, ties kept), the
    penalty over the prompt (``history [B, S0]``, ``history_lens``) and the tokens generated so far."""
    done = torch.zeros(logits.shape[0], dtype=torch.bool, device=logits.device)
    new = []
    for i in range(max_new_tokens):
        if repetition_penalty is not None and repetition_penalty != 1.0:
            logits = penalise_logits(logits, repetition_penalty, history, history_lens,
                                     torch.stack(new, 1) if new else None,
                                     torch.full_like(done, len(new), dtype=torch.int32))
        if do_sample and (top_p is not None or min_p is not None):
            x = logits.float()
            kept = sampling_kept(x, float(torch.tensor(1.0 / temperature, dtype=torch.float32)), top_k,
                                 1.0 if top_p is None else top_p, 0.0 if min_p is None else min_p)
            z = torch.where(kept, x / temperature, torch.full_like(x, float("-inf")))
            tok = torch.multinomial(torch.softmax(z, -1), 1, generator=generator).squeeze(1)
        elif do_sample:
            z = logits.float() / temperature
            if top_k is not None and top_k < z.shape[-1]:
                kth = z.topk(top_k, -1).values[:, -1:]
                z = torch.where(z < kth, torch.full_like(z, float("-inf")), z)
            tok = torch.multinomial(torch.softmax(z, -1), 1, generator=generator).squeeze(1)
        else:
            tok = logits.argmax(-1)
        if eos_token_id is not None:
            tok = torch.where(done, torch.full_like(tok, pad_token_id), tok)
            done = done | (tok == eos_token_id)
        new.append(tok)
        if i + 1 == max_new_tokens or (eos_token_id is not None and bool(done.all())):
            break
        logits = decode_step(tok)       # finished rows keep decoding (on pad tokens)
    return torch.stack(new, 1)


def use_graph_for(weight: torch.Tensor) -> bool:
    """A session on this embedding weight captures its step: a GPU with the native kernels and bf16."""
    from ..ops import _lib
    return weight.device.type == "cuda" and weight.dtype == torch.bfloat16 and _lib.use_native(weight)


def session_loop(sess, consume_prompt, batch, device, max_new_tokens, do_sample, temperature, top_k, eos_token_id,
                 pad_token_id, generator, top_p=None, min_p=None, repetition_penalty=None, history=None,
                 history_lens=None) -> torch.Tensor:
    """``token_loop`` on a decode session: ``consume_prompt(sess.cache)`` -> the prompt's logits, the first
    token by the step's own kernel, then one ``advance`` per token -> the new tokens ``[B, n]``.  The three
    further settings need a session made for them (``session_for(..., ext=True)``), which also takes the
    prompts (``history [B, S0]``, ``history_lens``) the penalty counts."""
    u = None
    if do_sample:
        u = torch.rand(max_new_tokens, batch, generator=generator,
                       device=device if generator is None else generator.device).to(device)
    sess.begin(ops.next_token_params(1.0 / temperature if do_sample else 1.0, top_k, eos_token_id, pad_token_id,
                                     do_sample, device, top_p=top_p, min_p=min_p,
                                     repetition_penalty=repetition_penalty), u, history, history_lens)
    sess.first_token(consume_prompt(sess.cache))
    n = 1
    while n < max_new_tokens:
        sess.advance()
        n += 1
        if eos_token_id is not None and n % 16 == 0 and bool(sess.done.all()):
            break
    new = sess.tokens_out[:, :n].clone()
    if eos_token_id is not None:
        # what the per-step check returns: through the step in which the last row emitted eos
        is_eos = new == eos_token_id
        if bool(is_eos.any(1).all()):
            new = new[:, :int(is_eos.int().argmax(1).max()) + 1]
    return new
