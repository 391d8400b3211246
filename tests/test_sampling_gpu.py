"""``ops.next_token`` with ``top_p``, ``min_p`` and ``repetition_penalty`` on the GPU (``ddl_next_token_ex``,
csrc/kernels/decode_step.hip): the cases, the fp64 oracle and the margins behind the exact-token requirement are
those of tests/test_sampling_cpu.py, run here against the HIP kernel.  V = 90001 exceeds what the kernel keeps
in LDS: its other loader, and for the penalty the op's own pass over the logits.

The models: gpt2_tiny and llama_tiny in bf16 with the prompts of their generate tests.  The captured session
must give, bit for bit, the tokens of the same step run eagerly through ``ops.next_token`` with the same ``u``,
history and state (the way tests/test_gpt2_graph_gpu.py compares).
"""
import pytest
import torch

from conftest import gpu_device
from test_sampling_cpu import (TOP_P_CASES, run_min_p, run_penalty_greedy, run_penalty_sampled, run_penalty_value,
                               run_top_p, run_top_p_edges, run_unchanged_and_bookkeeping)

from databricks_distributed_deep_learning_amd import ops
from databricks_distributed_deep_learning_amd.models import KVCache, LlamaKVCache, cast_params, llama_tiny
from databricks_distributed_deep_learning_amd.models._decode_graph import round_capacity

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("V,B,temperature,k,target", TOP_P_CASES)
def test_top_p(V, B, temperature, k, target):
    run_top_p(V, B, temperature, k, target, gpu_device())


@pytest.mark.parametrize("V", [1000, 50257, 90001])
def test_top_p_edges(V):
    run_top_p_edges(V, gpu_device())


@pytest.mark.parametrize("V,B,temperature", [(7, 3, 1.0), (1000, 3, 0.7), (1000, 1, 1.5), (50257, 3, 1.0),
                                             (90001, 3, 0.7)])
def test_min_p(V, B, temperature):
    run_min_p(V, B, temperature, gpu_device())


@pytest.mark.parametrize("V", [7, 1000, 50257, 90001])
def test_penalty(V):
    dev = gpu_device()
    run_penalty_greedy(V, dev)
    run_penalty_value(V, dev)
    run_penalty_sampled(V, dev)


def test_unchanged_and_bookkeeping():
    run_unchanged_and_bookkeeping(gpu_device())


# ------------------------------------------------------------------ the models
def _family(name, dev):
    if name == "gpt2":
        from test_gpt2_graph_gpu import _plain
        from test_gpt2_generate_gpu import _tokens
        model = _plain(dev)
        return model, _tokens()[0], KVCache, model.config.n_positions
    from test_llama_generate_gpu import _tokens
    torch.manual_seed(3)        # (not that file's decisive model: a sampled token has to depend on u)
    model = cast_params(llama_tiny().eval().to(dev), torch.bfloat16)
    return model, _tokens()[0], LlamaKVCache, model.config.max_position_embeddings


def _padded(prompts, dev):
    S = max(len(r) for r in prompts)
    ids, mask, comp = (torch.zeros(len(prompts), S, dtype=torch.long) for _ in range(3))
    for b, r in enumerate(prompts):     # left-padded: generate compacts
        ids[b, S - len(r):], mask[b, S - len(r):] = r, 1
        comp[b, :len(r)] = r
    return ids.to(dev), mask.to(dev), comp.to(dev)


def _eager(model, cache_cls, prompts, steps, cap, dev, u, sample, **settings):
    """prefill, then per token ``ops.next_token`` (with the prompts as history and its own tokens_out / step)
    and ``decode_step(len_bound=capacity)``: the session's step, launch by launch."""
    B = len(prompts)
    _, _, comp = _padded(prompts, dev)
    cnt = torch.tensor([len(r) for r in prompts], dtype=torch.int32, device=dev)
    cache = cache_cls.allocate(model, B, cap)
    logits = model.prefill(comp, cnt, cache)
    step = torch.zeros(B, dtype=torch.int32, device=dev)
    toks = torch.zeros(B, cap, dtype=torch.long, device=dev)
    prm = ops.next_token_params(settings.pop("inv_temperature", 1.0), settings.pop("top_k", None), sample=sample,
                                device=dev, **settings)
    for t in range(steps):
        tok = ops.next_token(logits, u=u, params=prm, history=comp, history_lens=cnt, tokens_out=toks, step=step)
        if t + 1 < steps:
            logits = model.decode_step(tok, cache, len_bound=cache.capacity)
    return toks[:, :steps].cpu()


@pytest.mark.parametrize("name", ["gpt2", "llama"])
def test_generate_with_the_new_settings(name):
    dev = gpu_device()
    model, prompts, cache_cls, n_pos = _family(name, dev)
    ids, mask, _ = _padded(prompts, dev)
    S, STEPS = ids.shape[1], 6
    cap = round_capacity(S + STEPS, n_pos)
    kw = dict(attention_mask=mask, max_new_tokens=STEPS, do_sample=True, temperature=0.8, top_k=50, top_p=0.9,
              min_p=0.02, repetition_penalty=1.3)
    a = model.generate(ids, use_graph=True, generator=torch.Generator().manual_seed(11), **kw)
    sess = model.decode_session
    assert sess.ext and sess.graph is not None and sess.captures == 1 and sess.capacity == cap
    b = model.generate(ids, use_graph=True, generator=torch.Generator().manual_seed(11), **kw)
    c = model.generate(ids, use_graph=True, generator=torch.Generator().manual_seed(12), **kw)
    assert model.decode_session is sess and sess.captures == 1
    assert torch.equal(a, b) and not torch.equal(a, c) and torch.equal(a[:, :S], ids)
    u = torch.zeros(cap, len(prompts))
    u[:STEPS] = torch.rand(STEPS, len(prompts), generator=torch.Generator().manual_seed(11))
    want = _eager(model, cache_cls, prompts, STEPS, cap, dev, u.to(dev), True, inv_temperature=1.0 / 0.8, top_k=50,
                  top_p=0.9, min_p=0.02, repetition_penalty=1.3)
    assert torch.equal(a[:, S:].cpu(), want)
    e = model.generate(ids, generator=torch.Generator(device=dev).manual_seed(11), **kw)        # the eager loop runs
    assert e.shape == a.shape and torch.equal(e[:, :S], ids)

    # greedy with a huge penalty: no row repeats a token of its prompt or of its continuation; the session's
    # tokens are the eager step's
    greedy = model.generate(ids, attention_mask=mask, max_new_tokens=STEPS, use_graph=True, repetition_penalty=1e4)
    assert model.decode_session is sess and sess.captures == 1
    want = _eager(model, cache_cls, prompts, STEPS, cap, dev, None, False, repetition_penalty=1e4)
    assert torch.equal(greedy[:, S:].cpu(), want)
    for out in (greedy, model.generate(ids, attention_mask=mask, max_new_tokens=STEPS, repetition_penalty=1e4)):
        for bi, r in enumerate(prompts):
            new = out[bi, S:].tolist()
            assert len(set(new)) == STEPS and not set(new) & set(r.tolist()), (name, bi, new)

    # without the settings: the session of old (no ext), and its tokens
    kw = dict(attention_mask=mask, max_new_tokens=STEPS, do_sample=True, temperature=0.8, top_k=50, use_graph=True)
    old = model.generate(ids, generator=torch.Generator().manual_seed(11), **kw)
    sess_old = model.decode_session
    assert sess_old is not sess and not sess_old.ext
    same = model.generate(ids, generator=torch.Generator().manual_seed(11), top_p=None, min_p=None,
                          repetition_penalty=None, **kw)
    neutral = model.generate(ids, generator=torch.Generator().manual_seed(11), top_p=1.0, min_p=0.0,
                             repetition_penalty=1.0, **kw)
    assert torch.equal(same, old) and torch.equal(neutral, old)
    for bad in (dict(top_p=0.0), dict(top_p=1.5), dict(min_p=-0.1), dict(min_p=1.0), dict(repetition_penalty=0.0)):
        with pytest.raises(ValueError, match=next(iter(bad))):
            model.generate(ids, attention_mask=mask, max_new_tokens=2, use_graph=True, **bad)
