"""GPT-2 ``extend`` / ``generate(prefix=..., prefill_chunk=...)`` on the CPU (gpt2_tiny, fp32, reference ops)."""
import pytest
import torch

from databricks_distributed_deep_learning_amd.models import KVCache, gpt2_tiny

WTE_SCALE = 5.0     # as tests/test_gpt2_generate_gpu.py: the last token's own logit dominates, no near-ties


@pytest.fixture(scope="module")
def model():
    torch.manual_seed(0)
    m = gpt2_tiny(dropout=0.0).eval()
    with torch.no_grad():
        m.wte.weight.mul_(WTE_SCALE)
    return m


def _ids(*shape, seed=1):
    return torch.randint(0, 1000, shape, generator=torch.Generator().manual_seed(seed))


def _i32(v):
    return torch.tensor(v, dtype=torch.int32)


def test_extend_from_empty_equals_prefill(model):
    ids, lens = _ids(2, 9), _i32([9, 4])
    a, b = KVCache.allocate(model, 2, 16), KVCache.allocate(model, 2, 16)
    a.data.zero_(), b.data.zero_()
    want = model.prefill(ids, lens, a)
    got = model.extend(ids, b, lens)
    torch.testing.assert_close(got, want, rtol=1e-4, atol=1e-4)
    assert b.lens.tolist() == [9, 4] and b.max_len == a.max_len == 9
    for r, n in enumerate([9, 4]):      # (prefill also copies the padded columns; extend leaves them alone)
        torch.testing.assert_close(b.data[:, :, r, :, :n], a.data[:, :, r, :, :n], rtol=1e-4, atol=1e-4)
    assert (b.data[:, :, 1, :, 4:] == 0).all()


def test_prefill_extend_extend_equals_prefill(model):
    ids = _ids(2, 66, seed=2)
    full = KVCache.allocate(model, 2, 66)
    want = model.prefill(ids, _i32([66, 66]), full)
    c = KVCache.allocate(model, 2, 70)
    model.prefill(ids[:, :5], _i32([5, 5]), c)
    mid = model.extend(ids[:, 5:65], c, all_logits=True)
    got = model.extend(ids[:, 65:], c)
    assert c.lens.tolist() == [66, 66] and c.max_len == 66 and mid.shape == (2, 60, 1000)
    torch.testing.assert_close(got, want, rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(mid, model(ids)[:, 5:65], rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(c.data[..., :66, :], full.data, rtol=1e-4, atol=1e-4)


def _prompts(model):
    """A shared 7-token prefix (batch-1 cache) and two continuations of 20 and 9 tokens."""
    head = _ids(1, 7, seed=3)
    tails = [_ids(20, seed=4), _ids(9, seed=5)]
    prefix = KVCache.allocate(model, 1, 7)
    model.prefill(head, _i32([7]), prefix)
    return head, tails, prefix


def _padded(tails, left):
    S = max(len(t) for t in tails)
    ids, mask = torch.zeros(len(tails), S, dtype=torch.long), torch.zeros(len(tails), S, dtype=torch.long)
    for b, t in enumerate(tails):
        sl = slice(S - len(t), S) if left else slice(0, len(t))
        ids[b, sl], mask[b, sl] = t, 1
    return ids, mask


@pytest.mark.parametrize("left", [False, True], ids=["right-padded", "left-padded"])
@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "session"])
def test_generate_with_prefix_and_chunks(model, left, use_graph):
    head, tails, prefix = _prompts(model)
    new = 5
    want = [model.generate(torch.cat([head[0], t])[None], max_new_tokens=new)[0, -new:] for t in tails]
    want = torch.stack(want)
    ids, mask = _padded(tails, left)
    before, lens_before = prefix.data.clone(), prefix.lens.clone()
    for kw in (dict(prefix=prefix), dict(prefix=prefix, prefill_chunk=8)):
        out = model.generate(ids, attention_mask=mask, max_new_tokens=new, use_graph=use_graph, **kw)
        assert torch.equal(out[:, :ids.shape[1]], ids) and torch.equal(out[:, ids.shape[1]:], want), kw
    assert torch.equal(prefix.data, before) and torch.equal(prefix.lens, lens_before) and prefix.max_len == 7
    # chunked prefill alone: the whole prompt (prefix tokens included) through extend, 16 columns at a time
    whole = [torch.cat([head[0], t]) for t in tails]
    ids, mask = _padded(whole, left)
    out = model.generate(ids, attention_mask=mask, max_new_tokens=new, use_graph=use_graph, prefill_chunk=16)
    assert torch.equal(out[:, ids.shape[1]:], want)


def test_copy_prefix(model):
    _, _, prefix = _prompts(model)
    c = KVCache.allocate(model, 3, 12)
    c.data.fill_(7.0)
    assert c.copy_prefix_(prefix) is c
    assert c.lens.tolist() == [7, 7, 7] and c.max_len == 7
    assert all(torch.equal(c.data[:, :, b, :, :7], prefix.data[:, :, 0]) for b in range(3))
    assert (c.data[..., 7:, :] == 7.0).all()
    with pytest.raises(ValueError, match="capacity"):
        KVCache.allocate(model, 1, 6).copy_prefix_(prefix)
    with pytest.raises(ValueError, match="batch"):
        c.copy_prefix_(KVCache.allocate(model, 2, 12))
    with pytest.raises(ValueError, match="float64"):
        KVCache.allocate(model, 3, 12, dtype=torch.float64).copy_prefix_(prefix)
    other = gpt2_tiny(dropout=0.0, n_layer=1)
    with pytest.raises(ValueError, match="layers"):
        KVCache.allocate(other, 3, 12).copy_prefix_(prefix)
    wide = gpt2_tiny(dropout=0.0, n_embd=256, n_head=4)
    with pytest.raises(ValueError, match="heads"):
        KVCache.allocate(wide, 3, 12).copy_prefix_(prefix)


def test_value_errors(model):
    _, _, prefix = _prompts(model)
    c = KVCache.allocate(model, 1, 12)
    c.copy_prefix_(prefix)
    with pytest.raises(ValueError, match="capacity"):
        model.extend(_ids(1, 6), c)
    model.extend(_ids(1, 5), c)         # 7 + 5 fills it
    with pytest.raises(ValueError, match="n_positions"):
        model.generate(_ids(1, 100), max_new_tokens=22, prefix=prefix)      # 7 + 100 + 22 > 128
    model.generate(_ids(1, 100), max_new_tokens=21, prefix=prefix)
    with pytest.raises(ValueError, match="prefill_chunk"):
        model.generate(_ids(1, 4), max_new_tokens=1, prefill_chunk=0)
