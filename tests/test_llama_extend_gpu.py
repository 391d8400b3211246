"""Llama ``extend`` / ``generate(prefix=...)`` / ``prefill(chunk=...)`` on the GPU (bf16, native kernels), in the
form of tests/test_gpt2_extend_gpu.py and tests/test_llama_generate_gpu.py, whose models (``llama_tiny``, G = 2,
and the G = 3 variant, token embedding scaled by 5), fp64 copy (`forward64`) and tolerance it uses.

Step logits: two sequences of 56 and 24 tokens go through ``prefill`` of (5, 3) tokens, ``extend`` of T = 33 with
``new_lens`` (33, 20) and ``all_logits``, ``extend`` of T = 17 with ``new_lens`` (17, 0) -- row 1 sits out -- and
``extend`` of T = 1 (B T <= 16: the weight-streaming linears).  Every real row of logits is bounded, in the form
of tests/test_attention_edges_gpu.py (`check`, M = 2, max and rms), by M x the error of the EXISTING native full
``forward`` at the same positions against the same fp64 copy, plus half a bf16 ulp.

Greedy tokens: ``generate(prefix=...)`` over a shared 40-token prefix equals ``generate`` on the concatenated
prompts and the fp64 greedy continuation, eagerly and under graph replay, on a model whose every fp64 top-2 gap
on that continuation exceeds 20 x the measured extend logit error (asserted: the near-tie cap of
tests/test_llama_generate_gpu.py, checked on the reference arm).

Measured on an MI355X: against the native forward's error as the yardstick, with the ulp term subtracted the
largest ratios are 0.067 (max form; G = 2, all_logits row 0) and 0.368 (rms form; G = 3, chunked prefill row
1); as plain extend error / forward error 1.07 (max; G = 2, extend T = 1) and 1.07 (rms; G = 2, chunked
prefill), so M = 2 holds as it stands.  The largest extend logit errors are 3.35e-2 (G = 2) and 6.20e-2 (G = 3)
and the smallest fp64 top-2 gaps 8.70 and 13.3: 260 x and 214 x.
"""
import math

import pytest
import torch

from conftest import gpu_device
from test_attention_edges_gpu import M, check  # noqa: F401
from test_llama_generate_gpu import VARIANTS, _model, forward64

from databricks_distributed_deep_learning_amd.models import LlamaKVCache

pytestmark = pytest.mark.gpu

TOTAL = [56, 24]
FIRST, SECOND, THIRD = [5, 3], [33, 20], [17, 0]
STEPS = 6
_cache = {}


def _i32(v, dev):
    return torch.tensor(v, dtype=torch.int32, device=dev)


def _seqs():
    g = torch.Generator().manual_seed(78)
    return [torch.randint(0, 1000, (n,), generator=g) for n in TOTAL]


def _chunk(seqs, start, lens, T):
    out = torch.full((len(seqs), T), 7, dtype=torch.long)       # pad content must not matter
    for b, s in enumerate(seqs):
        out[b, :lens[b]] = s[start[b]:start[b] + lens[b]]
    return out


def _shared(dev, variant):
    """Once per variant: the model, [(label, got [n, V], positions (b, s) ...)] of the extend path, and per
    sequence the fp64 copy's and the existing native forward's logits [S, V]."""
    if variant in _cache:
        return _cache[variant]
    model = _model(dev, variant)
    seqs = _seqs()
    cache = LlamaKVCache.allocate(model, 2, 64)
    model.prefill(_chunk(seqs, [0, 0], FIRST, 5).to(dev), _i32(FIRST, dev), cache)
    at = list(FIRST)
    rows = []
    mid = model.extend(_chunk(seqs, at, SECOND, 33).to(dev), cache, _i32(SECOND, dev), all_logits=True)
    assert mid.shape == (2, 33, 1000) and cache.lens.tolist() == [38, 23] and cache.max_len == 38
    for b in range(2):
        rows.append((f"all_logits row {b}", mid[b, :SECOND[b]].float().cpu(), b, slice(at[b], at[b] + SECOND[b])))
    at = [a + s for a, s in zip(at, SECOND)]
    lg = model.extend(_chunk(seqs, at, THIRD, 17).to(dev), cache, _i32(THIRD, dev))
    assert lg.shape == (2, 1000) and cache.lens.tolist() == [55, 23] and cache.max_len == 55
    rows.append(("extend T=17, row 0", lg[0:1].float().cpu(), 0, slice(54, 55)))
    at = [a + s for a, s in zip(at, THIRD)]
    lg = model.extend(_chunk(seqs, at, [1, 1], 1).to(dev), cache)
    assert cache.lens.tolist() == TOTAL and cache.max_len == 56
    for b in range(2):
        rows.append((f"extend T=1, row {b}", lg[b:b + 1].float().cpu(), b, slice(TOTAL[b] - 1, TOTAL[b])))
    with torch.no_grad():
        ref = [forward64(model, s) for s in seqs]
        fwd = [model(s[None].to(dev))[0].float().cpu() for s in seqs]
    _cache[variant] = (model, rows, ref, fwd)
    return _cache[variant]


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_extend_logits_against_fp64_copy(variant):
    dev = gpu_device()
    _, rows, ref, fwd = _shared(dev, variant)
    fails = []
    for label, got, b, sl in rows:
        check(fails, f"{variant} {label}", got, ref[b][sl], fwd[b][sl])
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_chunked_prefill_equals_prefill_path(variant):
    """``prefill(chunk=16)`` of right-padded prompts (56, 24): logits within the same bound, the same lengths."""
    dev = gpu_device()
    model, _, ref, fwd = _shared(dev, variant)
    seqs = _seqs()
    ids = _chunk(seqs, [0, 0], TOTAL, 56).to(dev)
    cache = LlamaKVCache.allocate(model, 2, 56)
    got = model.prefill(ids, _i32(TOTAL, dev), cache, chunk=16).float().cpu()
    assert cache.lens.tolist() == TOTAL and cache.max_len == 56
    fails = []
    for b in range(2):
        sl = slice(TOTAL[b] - 1, TOTAL[b])
        check(fails, f"{variant} chunked prefill row {b}", got[b:b + 1], ref[b][sl], fwd[b][sl])
    assert not fails, "\n".join(fails)


def _left_padded(tails):
    S = max(len(t) for t in tails)
    ids, mask = torch.zeros(len(tails), S, dtype=torch.long), torch.zeros(len(tails), S, dtype=torch.long)
    for b, r in enumerate(tails):
        ids[b, S - len(r):], mask[b, S - len(r):] = r, 1
    return ids, mask


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_greedy_generate_with_prefix(variant):
    dev = gpu_device()
    model, rows, ref, _ = _shared(dev, variant)
    err = max((got.double() - ref[b][sl]).abs().max().item() for _, got, b, sl in rows)
    g = torch.Generator().manual_seed(79)
    head = torch.randint(0, 1000, (40,), generator=g)
    tails = [torch.randint(0, 1000, (n,), generator=g) for n in (30, 9)]
    want, gap = [], math.inf
    for t in tails:             # the fp64 greedy continuation and its smallest top-2 gap
        seq = torch.cat([head, t])
        for _ in range(STEPS):
            lg = forward64(model, seq)[-1]
            top = lg.topk(2).values
            gap = min(gap, (top[0] - top[1]).item())
            seq = torch.cat([seq, lg.argmax()[None]])
        want.append(seq[-STEPS:])
    want = torch.stack(want)
    print(f"{variant}: measured extend logit error {err:.4e}, smallest fp64 top-2 gap {gap:.4e} ({gap / err:.1f} x)")
    assert gap >= 20 * err

    prefix = LlamaKVCache.allocate(model, 1, 40)
    model.prefill(head[None].to(dev), _i32([40], dev), prefix)
    before = prefix.data.clone()
    ids, mask = _left_padded(tails)
    whole, wmask = _left_padded([torch.cat([head, t]) for t in tails])
    for use_graph in (False, True):
        ref_run = model.generate(whole.to(dev), attention_mask=wmask.to(dev), max_new_tokens=STEPS, use_graph=use_graph)
        assert torch.equal(ref_run[:, -STEPS:].cpu(), want), use_graph
        out = model.generate(ids.to(dev), attention_mask=mask.to(dev), max_new_tokens=STEPS, prefix=prefix,
                             use_graph=use_graph)
        assert torch.equal(out[:, :ids.shape[1]].cpu(), ids) and torch.equal(out[:, -STEPS:].cpu(), want), use_graph
        if use_graph:
            sess = model.decode_session
            assert sess is not None and sess.graph is not None
            assert sess.cache.lens.tolist() == [40 + 30 + STEPS - 1, 40 + 9 + STEPS - 1]
    assert torch.equal(prefix.data, before) and prefix.lens.tolist() == [40] and prefix.max_len == 40


def test_value_errors():
    dev = gpu_device()
    model = _shared(dev, "G2")[0]
    prefix = LlamaKVCache.allocate(model, 1, 7)
    model.prefill(torch.zeros(1, 7, dtype=torch.long, device=dev), _i32([7], dev), prefix)
    c = LlamaKVCache.allocate(model, 1, 12)
    c.copy_prefix_(prefix)
    ids = torch.zeros(1, 200, dtype=torch.long, device=dev)
    with pytest.raises(ValueError, match="capacity"):
        model.extend(ids[:, :6], c)
    model.extend(ids[:, :5], c)         # 7 + 5 fills it
    with pytest.raises(ValueError, match="max_position_embeddings"):
        model.generate(ids, max_new_tokens=50, prefix=prefix)      # 7 + 200 + 50 > 256
    with pytest.raises(ValueError, match="float32"):
        LlamaKVCache.allocate(model, 1, 12, dtype=torch.float32).copy_prefix_(prefix)
