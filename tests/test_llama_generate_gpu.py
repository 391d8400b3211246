"""Llama-family generation on the GPU (bf16, native kernels): prefill + grouped-query KV-cache decode steps
against an fp64 copy of the model, greedy ``generate`` against decoding by full re-forward, and the graph
session.

Models: ``llama_tiny`` (2 heads over 1 KV head: G = 2) and a G = 3 variant (hidden 192, 3 heads, 1 KV head).
B = 2 with prompt lengths {5, 65}; 6 decode steps, teacher-forced on a fixed token sequence so that a flipped
near-tie cannot cascade.  The fp64 copy (`forward64`) is plain torch on the CPU from the model's bf16 weights
and its fp32 rotary table, each sequence alone and unpadded.

Step logits: the prefill's and each decode step's ``[B, vocab]`` logits are bounded, in the form of
tests/test_attention_edges_gpu.py (`check`, M = 2, max and rms), by M x the error of the EXISTING native full
``forward`` at the same positions against the same fp64 copy, plus half a bf16 ulp: the yardstick is the
training-time forward path, not the code under test.

Greedy tokens: ``generate`` is repeatable and equals both the fp64 greedy continuation and the native
re-forward arm, on a model whose every fp64 top-2 gap on that continuation exceeds 20 x the measured decode
logit error (asserted).  As in tests/test_gpt2_generate_gpu.py the (tied) token embedding is scaled by 5, which
makes the last token's own logit dominate.  Under RMSNorm the scale of the residual stream cancels inside the
blocks, but the final norm's output still points along 5 x the token's embedding plus the blocks' O(1)
contributions, so the tied head favours that token.  The scale was checked on the CPU before any GPU run, with
the reference ops in bf16 standing in for the kernels: gap / error 219 (G = 2) and 202 (G = 3) at scale 5.

``use_graph=True``: tokens equal the eager loop's at the same launch bound bitwise, one capture serves the
calls of a shape, and a different batch rebuilds the session.

Measured on an MI355X: against the native forward's error as the yardstick, with the ulp term subtracted the
largest ratios are 0.104 (max form; G = 2, decode step 1) and 0.382 (rms form; G = 3, prefill); as plain decode
error / forward error 1.10 (max; G = 2, decode step 0) and 1.07 (rms; G = 2, decode step 3), so M = 2 holds as
it stands.  The largest decode logit errors are 3.49e-2 (G = 2) and 6.17e-2 (G = 3) and the smallest fp64 top-2
gaps 7.53 and 13.3: 216 x in both.
"""
import math

import pytest
import torch
import torch.nn.functional as F

from conftest import gpu_device
from test_attention_edges_gpu import M, check  # noqa: F401

from databricks_distributed_deep_learning_amd import ops
from databricks_distributed_deep_learning_amd.models import LlamaKVCache, cast_params, llama_tiny
from databricks_distributed_deep_learning_amd.models._decode_graph import round_capacity

pytestmark = pytest.mark.gpu

LENS = [5, 65]
STEPS = 6
MODEL_SEED = 0
EMB_SCALE = 5.0
VARIANTS = {"G2": dict(), "G3": dict(hidden_size=192, num_attention_heads=3, num_key_value_heads=1)}
_cache = {}


def _model(dev, variant, dtype=torch.bfloat16):
    torch.manual_seed(MODEL_SEED)
    model = llama_tiny(**VARIANTS[variant]).eval()
    with torch.no_grad():       # see the module docstring: what makes the greedy continuation decisive
        model.embed_tokens.weight.mul_(EMB_SCALE)
    model = model.to(dev)
    cast_params(model, dtype)
    return model


def _tokens():
    g = torch.Generator().manual_seed(77)
    prompts = [torch.randint(0, 1000, (n,), generator=g) for n in LENS]
    forced = torch.randint(0, 1000, (len(LENS), STEPS), generator=g)
    return prompts, forced


def forward64(model, ids):
    """fp64 logits [S, vocab] of one unpadded sequence from the model's (bf16) weights and fp32 table."""
    c = model.config
    p = {k: v.detach().double().cpu() for k, v in model.state_dict().items()}
    H, Hkv, eps = c.num_attention_heads, c.num_key_value_heads, c.rms_norm_eps
    D = c.hidden_size // H
    S = ids.shape[0]
    tab = model.rope_table[:S].double().cpu()
    cos, sin = tab[:, None, :D // 2], tab[:, None, D // 2:]

    def rms(x, w):
        return x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps) * w

    def rot(t):
        a, b = t[..., :D // 2], t[..., D // 2:]
        return torch.cat([a * cos - b * sin, b * cos + a * sin], -1)

    h = p["embed_tokens.weight"][ids]
    ar = torch.arange(S)
    for i in range(c.num_hidden_layers):
        g = lambda name: p[f"layers.{i}.{name}.weight"]     # noqa: E731
        x = (rms(h, g("input_layernorm")) @ g("qkv").t()).view(S, H + 2 * Hkv, D)
        q = rot(x[:, :H]).permute(1, 0, 2)
        k = rot(x[:, H:H + Hkv]).repeat_interleave(H // Hkv, 1).permute(1, 0, 2)
        v = x[:, H + Hkv:].repeat_interleave(H // Hkv, 1).permute(1, 0, 2)
        s = (q @ k.transpose(-1, -2)) / math.sqrt(D)
        s = s.masked_fill(ar[None, :] > ar[:, None], -math.inf)
        ctx = (torch.softmax(s, -1) @ v).permute(1, 0, 2).reshape(S, -1)
        h = h + ctx @ g("o_proj").t()
        gate, up = (rms(h, g("post_attention_layernorm")) @ g("gate_up").t()).chunk(2, -1)
        h = h + (F.silu(gate) * up) @ g("down_proj").t()
    return rms(h, p["norm.weight"]) @ p["embed_tokens.weight"].t()


def _decode_logits(model, prompts, forced, dev):
    """[STEPS + 1, B, vocab]: the prefill's logits, then each teacher-forced decode step's."""
    S = max(LENS)
    ids = torch.zeros(len(LENS), S, dtype=torch.long)
    for b, r in enumerate(prompts):
        ids[b, :len(r)] = r
    cache = LlamaKVCache.allocate(model, len(LENS), S + STEPS)
    out = [model.prefill(ids.to(dev), torch.tensor(LENS, dtype=torch.int32, device=dev), cache)]
    for t in range(STEPS):
        out.append(model.decode_step(forced[:, t].to(dev), cache))
    assert cache.lens.tolist() == [n + STEPS for n in LENS]
    return torch.stack(out).float().cpu()


def _shared(dev, variant):
    """Computed once per variant: the decode logits, the fp64 copy's and the existing native forward's,
    [STEPS + 1, B, V]."""
    if variant not in _cache:
        model = _model(dev, variant)
        prompts, forced = _tokens()
        got = _decode_logits(model, prompts, forced, dev)
        ref, fwd = [], []
        with torch.no_grad():
            for b, r in enumerate(prompts):
                full = torch.cat([r, forced[b]])
                rows = slice(len(r) - 1, len(r) + STEPS)
                ref.append(forward64(model, full)[rows])
                fwd.append(model(full[None].to(dev))[0, rows].float().cpu())
        _cache[variant] = (model, got, torch.stack(ref, 1), torch.stack(fwd, 1))
    return _cache[variant]


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_step_logits_against_fp64_copy(variant):
    dev = gpu_device()
    _, got, ref, fwd = _shared(dev, variant)
    fails = []
    for t in range(STEPS + 1):
        check(fails, f"{variant} " + ("prefill logits" if t == 0 else f"decode step {t - 1} logits"), got[t], ref[t],
              fwd[t])
    assert not fails, "\n".join(fails)


def _padded(prompts):
    S = max(LENS)
    ids, mask = torch.zeros(len(LENS), S, dtype=torch.long), torch.zeros(len(LENS), S, dtype=torch.long)
    for b, r in enumerate(prompts):     # left-padded: generate compacts
        ids[b, S - len(r):], mask[b, S - len(r):] = r, 1
    return ids, mask


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_greedy_generate_equals_reforward(variant):
    dev = gpu_device()
    model, got, ref, _ = _shared(dev, variant)
    err = (got.double() - ref).abs().max().item()
    prompts, _ = _tokens()
    want, gap = [], math.inf
    for r in prompts:           # the fp64 greedy continuation and its smallest top-2 gap
        seq = r.clone()
        for _ in range(STEPS):
            lg = forward64(model, seq)[-1]
            top = lg.topk(2).values
            gap = min(gap, (top[0] - top[1]).item())
            seq = torch.cat([seq, lg.argmax()[None]])
        want.append(seq[len(r):])
    want = torch.stack(want)
    print(f"{variant}: measured decode logit error {err:.4e}, smallest fp64 top-2 gap {gap:.4e} ({gap / err:.1f} x)")
    assert gap >= 20 * err

    S = max(LENS)
    ids, mask = _padded(prompts)
    a = model.generate(ids.to(dev), attention_mask=mask.to(dev), max_new_tokens=STEPS)
    b2 = model.generate(ids.to(dev), attention_mask=mask.to(dev), max_new_tokens=STEPS)
    assert torch.equal(a, b2)
    assert torch.equal(a[:, :S].cpu(), ids) and torch.equal(a[:, S:].cpu(), want)
    with torch.no_grad():               # the re-forward arm: a full native forward per token
        for bi, r in enumerate(prompts):
            seq = r.clone().to(dev)
            for _ in range(STEPS):
                seq = torch.cat([seq, model(seq[None])[0, -1].argmax()[None]])
            assert torch.equal(seq[len(r):].cpu(), want[bi])


def _eager_loop(model, prompts, steps, dev, capacity, u=None, **sampling):
    """prefill, then ``decode_step(len_bound=capacity)`` per token -> tokens [B, steps]: the session's step,
    launch by launch."""
    S = max(LENS)
    comp = torch.zeros(len(prompts), S, dtype=torch.long)
    for b, r in enumerate(prompts):
        comp[b, :len(r)] = r
    cache = LlamaKVCache.allocate(model, len(prompts), capacity)
    logits = model.prefill(comp.to(dev), torch.tensor([len(r) for r in prompts], dtype=torch.int32, device=dev), cache)
    toks = []
    for t in range(steps):
        toks.append(logits.argmax(-1) if u is None else ops.next_token(logits, u=u[t].contiguous(), **sampling))
        if t + 1 < steps:
            logits = model.decode_step(toks[-1], cache, len_bound=cache.capacity)
    return torch.stack(toks, 1).cpu()


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_graph_session(variant):
    """Replayed tokens equal the eager loop's at the same launch bound (the cache capacity) bitwise, greedy and
    sampled; one capture serves the calls of a shape; another batch rebuilds the session."""
    dev = gpu_device()
    model = _shared(dev, variant)[0]
    prompts, _ = _tokens()
    ids, mask = _padded(prompts)
    ids, mask = ids.to(dev), mask.to(dev)
    S = ids.shape[1]
    cap = round_capacity(S + STEPS, model.config.max_position_embeddings)

    want = _eager_loop(model, prompts, STEPS, dev, cap)
    a = model.generate(ids, attention_mask=mask, max_new_tokens=STEPS, use_graph=True)
    sess = model.decode_session
    assert sess is not None and sess.graph is not None and sess.captures == 1 and sess.capacity == cap
    assert sess.cache.data.shape[3] == model.config.num_key_value_heads
    assert a.shape == (len(LENS), S + STEPS) and torch.equal(a[:, :S], ids)
    assert torch.equal(a[:, S:].cpu(), want)
    b = model.generate(ids, attention_mask=mask, max_new_tokens=STEPS, use_graph=True)
    assert model.decode_session is sess and sess.captures == 1      # replayed, not captured again
    assert torch.equal(a, b)
    assert sess.cache.lens.tolist() == [n + STEPS - 1 for n in LENS]
    assert torch.equal(a, model.generate(ids, attention_mask=mask, max_new_tokens=STEPS))   # the decisive model

    u = torch.rand(STEPS, len(LENS), generator=torch.Generator().manual_seed(3)).to(dev)
    want_s = _eager_loop(model, prompts, STEPS, dev, cap, u, inv_temperature=1.0 / 0.8, top_k=50)
    got_s = model.generate(ids, attention_mask=mask, max_new_tokens=STEPS, use_graph=True, do_sample=True,
                           temperature=0.8, top_k=50, generator=torch.Generator().manual_seed(3))
    assert model.decode_session is sess and sess.captures == 1
    assert torch.equal(got_s[:, S:].cpu(), want_s)

    one = model.generate(ids[1:], attention_mask=mask[1:], max_new_tokens=STEPS, use_graph=True)
    assert model.decode_session is not sess and model.decode_session.batch == 1
    assert torch.equal(one[0, S:].cpu(), _eager_loop(model, prompts[1:], STEPS, dev, cap)[0])
