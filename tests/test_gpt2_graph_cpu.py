"""``generate(use_graph=True)`` and ``decode_step(len_bound=...)`` on the CPU (fp32, reference ops): the
session loop run eagerly must return what ``generate()`` returns.  The model, prompts and horizon are those of
tests/test_gpt2_generate_cpu.py, whose seeds keep every greedy step's top-2 gap above 1e-3 (asserted there).
"""
import pytest
import torch

from test_gpt2_generate_cpu import LENS, NEW, _model, _prompts

from databricks_distributed_deep_learning_amd.models import KVCache
from databricks_distributed_deep_learning_amd.models._decode_graph import round_capacity


@pytest.mark.parametrize("side", ["right", "left"])
def test_use_graph_equals_generate_greedy(side):
    model = _model(0)
    ids, mask, _ = _prompts(1, side)
    want = model.generate(ids, attention_mask=mask, max_new_tokens=NEW)
    got = model.generate(ids, attention_mask=mask, max_new_tokens=NEW, use_graph=True)
    assert got.dtype == want.dtype and torch.equal(got, want)
    sess = model.decode_session
    assert sess.graph is None and sess.captures == 0 and sess.capacity == 128 and sess.batch == 3
    assert sess.cache.lens.tolist() == [n + NEW - 1 for n in LENS] and sess.step.tolist() == [NEW] * 3
    assert torch.equal(model.generate(ids, attention_mask=mask, max_new_tokens=NEW, use_graph=True), want)
    assert model.decode_session is sess         # same shape: the same session
    model.train()
    assert torch.equal(model.generate(ids[:2], attention_mask=mask[:2], max_new_tokens=3, use_graph=True),
                       model.generate(ids[:2], attention_mask=mask[:2], max_new_tokens=3))
    assert model.training and model.decode_session is not sess


def test_capacity_rounding():
    assert [round_capacity(n, 1024) for n in (1, 128, 129, 1000, 1024)] == [128, 128, 256, 1024, 1024]
    assert round_capacity(71, 100) == 100


def test_use_graph_eos_shape_and_pad():
    model = _model(0)
    ids, mask, rows = _prompts(1, "right")
    horizon = 40            # past the 16-step interval of the session loop's eos check
    free = model.generate(ids, attention_mask=mask, max_new_tokens=horizon)[:, ids.shape[1]:]
    eos = int(free[0, 3])
    for kw in (dict(eos_token_id=eos, pad_token_id=999), dict(eos_token_id=eos)):
        want = model.generate(ids, attention_mask=mask, max_new_tokens=horizon, **kw)
        got = model.generate(ids, attention_mask=mask, max_new_tokens=horizon, use_graph=True, **kw)
        assert torch.equal(got, want)
    # one row, finished after a few tokens: trimmed to where the per-step check stops
    want = model.generate(rows[0][None], max_new_tokens=horizon, eos_token_id=eos, pad_token_id=999)
    got = model.generate(rows[0][None], max_new_tokens=horizon, eos_token_id=eos, pad_token_id=999, use_graph=True)
    assert want.shape[1] < LENS[0] + 16 and int(want[0, -1]) == eos and torch.equal(got, want)


def test_use_graph_sampling():
    model = _model(0)
    ids, mask, _ = _prompts(1, "left")
    kw = dict(attention_mask=mask, max_new_tokens=8, do_sample=True, temperature=0.7, top_k=20, use_graph=True)
    a = model.generate(ids, generator=torch.Generator().manual_seed(11), **kw)
    b = model.generate(ids, generator=torch.Generator().manual_seed(11), **kw)
    c = model.generate(ids, generator=torch.Generator().manual_seed(12), **kw)
    assert torch.equal(a, b) and not torch.equal(a, c)
    greedy = model.generate(ids, attention_mask=mask, max_new_tokens=8)
    k1 = model.generate(ids, attention_mask=mask, max_new_tokens=8, do_sample=True, top_k=1, use_graph=True,
                        generator=torch.Generator().manual_seed(3))
    assert torch.equal(k1, greedy) and not torch.equal(a, greedy)


def test_len_bound():
    model = _model(0)
    ids, _, _ = _prompts(1, "right")
    lens = torch.tensor(LENS, dtype=torch.int32)
    outs = []
    for bound in (None, "default", 20):
        cache = KVCache.allocate(model, 3, 20)
        logits = model.prefill(ids, lens, cache)
        for _ in range(3):
            lb = cache.max_len + 1 if bound == "default" else bound
            logits = model.decode_step(logits.argmax(-1), cache, len_bound=lb)
        assert cache.lens.tolist() == [n + 3 for n in LENS] and cache.max_len == max(LENS) + 3
        outs.append(logits)
    assert torch.equal(outs[0], outs[1])            # the default is max_len + 1
    torch.testing.assert_close(outs[2], outs[0], atol=1e-5, rtol=1e-5)
    with pytest.raises(ValueError, match="len_bound"):
        model.decode_step(logits.argmax(-1), cache, len_bound=cache.max_len)
    with pytest.raises(ValueError, match="len_bound"):
        model.decode_step(logits.argmax(-1), cache, len_bound=21)


def test_value_errors_with_use_graph():
    model = _model(0)
    ids = torch.randint(0, 1000, (2, 6))
    with pytest.raises(ValueError, match="n_positions"):
        model.generate(ids, max_new_tokens=128 - 6 + 1, use_graph=True)
    with pytest.raises(ValueError, match="temperature"):
        model.generate(ids, max_new_tokens=2, do_sample=True, temperature=0.0, use_graph=True)
    with pytest.raises(ValueError, match="top_k"):
        model.generate(ids, max_new_tokens=2, top_k=0, use_graph=True)
    with pytest.raises(ValueError, match="contiguous"):
        model.generate(ids, attention_mask=torch.tensor([[1, 0, 1, 1, 1, 1], [1] * 6]), max_new_tokens=2, use_graph=True)
    assert model.generate(ids, max_new_tokens=128 - 6, use_graph=True).shape == (2, 128)
