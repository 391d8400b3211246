"""Llama ``extend`` / ``prefill(chunk=...)`` / ``generate(prefix=...)`` on the CPU (llama_tiny, fp32, reference
ops), in the form of tests/test_gpt2_extend_cpu.py and tests/test_llama_generate_cpu.py.

The greedy arms are compared with decoding by full re-forward, each sequence alone and unpadded (all the model
could do before it had a cache).  Seeds are fixed so that every step's top-2 logit gap on that arm exceeds 1e-3
(asserted), far above the 1e-4 to which the arms' logits agree.
"""
import pytest
import torch

from databricks_distributed_deep_learning_amd.models import LlamaKVCache, llama_tiny

NEW = 5


def _model(seed=0, **kw):
    torch.manual_seed(seed)
    # a wider init than the default 0.02: the logits of a random tiny model are otherwise nearly flat
    return llama_tiny(initializer_range=0.2, **kw).eval()


@pytest.fixture(scope="module")
def model():
    return _model(0)


def _ids(*shape, seed=1):
    return torch.randint(0, 1000, shape, generator=torch.Generator().manual_seed(seed))


def _i32(v):
    return torch.tensor(v, dtype=torch.int32)


def _reforward_greedy(model, rows, steps):
    """Greedy decoding by full re-forward, each sequence alone: tokens [B, steps]; asserts the top-2 gap."""
    toks, gap = [], float("inf")
    with torch.no_grad():
        for r in rows:
            seq, t_row = r.clone(), []
            for _ in range(steps):
                lg = model(seq[None])[0, -1]
                top2 = lg.topk(2).values
                gap = min(gap, (top2[0] - top2[1]).item())
                t_row.append(lg.argmax())
                seq = torch.cat([seq, t_row[-1][None]])
            toks.append(torch.stack(t_row))
    print(f"min top-2 gap on the re-forward arm: {gap:.4e}")
    assert gap > 1e-3
    return torch.stack(toks)


def test_extend_from_empty_equals_prefill(model):
    ids, lens = _ids(2, 9), _i32([9, 4])
    a, b = LlamaKVCache.allocate(model, 2, 16), LlamaKVCache.allocate(model, 2, 16)
    a.data.zero_(), b.data.zero_()
    want = model.prefill(ids, lens, a)
    got = model.extend(ids, b, lens)
    torch.testing.assert_close(got, want, rtol=1e-4, atol=1e-4)
    assert b.lens.tolist() == [9, 4] and b.max_len == a.max_len == 9
    for r, n in enumerate([9, 4]):      # (prefill also copies the padded columns; extend leaves them alone)
        torch.testing.assert_close(b.data[:, :, r, :, :n], a.data[:, :, r, :, :n], rtol=1e-4, atol=1e-4)
    assert (b.data[:, :, 1, :, 4:] == 0).all()


def test_prefill_extend_extend_equals_prefill(model):
    """Unequal lengths throughout and a row that sits out the last chunk (``new_lens == 0``)."""
    ids = _ids(3, 40, seed=2)
    total = [40, 23, 31]
    full = LlamaKVCache.allocate(model, 3, 40)
    want = model.prefill(ids, _i32(total), full)
    c = LlamaKVCache.allocate(model, 3, 48)
    c.data.zero_()
    first, second = [5, 3, 4], [25, 20, 20]                       # then 10, 0, 7
    comp = torch.zeros(3, 40, dtype=torch.long)
    model.prefill(ids[:, :5], _i32(first), c)
    chunk2 = torch.stack([torch.cat([ids[b, first[b]:first[b] + second[b]],
                                     comp[b, :25 - second[b]]]) for b in range(3)])
    mid = model.extend(chunk2, c, _i32(second), all_logits=True)
    assert c.lens.tolist() == [30, 23, 24] and c.max_len == 30 and mid.shape == (3, 25, 1000)
    done = [first[b] + second[b] for b in range(3)]
    third = [total[b] - done[b] for b in range(3)]
    assert third == [10, 0, 7]
    chunk3 = torch.stack([torch.cat([ids[b, done[b]:total[b]], comp[b, :10 - third[b]]]) for b in range(3)])
    got = model.extend(chunk3, c, _i32(third))
    assert c.lens.tolist() == total and c.max_len == 40
    # the row that sat out keeps its earlier logits: those of its last real column of the middle chunk
    torch.testing.assert_close(got[[0, 2]], want[[0, 2]], rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(mid[1, second[1] - 1], want[1], rtol=1e-4, atol=1e-4)
    # all_logits rows are forward's
    for b in range(3):
        fwd = model(ids[b:b + 1, :total[b]])[0]
        torch.testing.assert_close(mid[b, :second[b]], fwd[first[b]:done[b]], rtol=1e-4, atol=1e-4)
    for b, n in enumerate(total):       # the live rows of the cache
        torch.testing.assert_close(c.data[:, :, b, :, :n], full.data[:, :, b, :, :n], rtol=1e-4, atol=1e-4)


@pytest.mark.parametrize("k", [1, 4, 7, 64])
def test_chunked_prefill_equals_prefill(model, k):
    """k = 7 does not divide the 18 columns; k = 64 is one chunk.  Row 1's prompt ends before the later chunks."""
    ids, lens = _ids(2, 18, seed=6), _i32([18, 6])
    a, b = LlamaKVCache.allocate(model, 2, 20), LlamaKVCache.allocate(model, 2, 20)
    want = model.prefill(ids, lens, a)
    b.lens.fill_(3)                     # whatever it held before: chunked prefill starts from empty
    b.max_len = 3
    got = model.prefill(ids, lens, b, chunk=k)
    torch.testing.assert_close(got, want, rtol=1e-4, atol=1e-4)
    assert b.lens.tolist() == [18, 6] and b.max_len == a.max_len == 18
    for r, n in enumerate([18, 6]):
        torch.testing.assert_close(b.data[:, :, r, :, :n], a.data[:, :, r, :, :n], rtol=1e-4, atol=1e-4)
    with pytest.raises(ValueError, match="chunk"):
        model.prefill(ids, lens, b, chunk=0)


def _prompts(model, batch):
    """A 7-token prefix (one shared batch-1 cache, or a batch-2 cache of unequal lengths 7 and 4) and two
    continuations of 20 and 9 tokens."""
    heads = [_ids(7, seed=3), _ids(7, seed=3)] if batch == 1 else [_ids(7, seed=3), _ids(4, seed=7)]
    tails = [_ids(20, seed=4), _ids(9, seed=5)]
    prefix = LlamaKVCache.allocate(model, batch, 7)
    if batch == 1:
        model.prefill(heads[0][None], _i32([7]), prefix)
    else:
        hp = torch.zeros(2, 7, dtype=torch.long)
        hp[0], hp[1, :4] = heads[0], heads[1]
        model.prefill(hp, _i32([7, 4]), prefix)
    return heads, tails, prefix


def _padded(tails, left):
    S = max(len(t) for t in tails)
    ids, mask = torch.full((len(tails), S), 7, dtype=torch.long), torch.zeros(len(tails), S, dtype=torch.long)
    for b, t in enumerate(tails):
        sl = slice(S - len(t), S) if left else slice(0, len(t))
        ids[b, sl], mask[b, sl] = t, 1
    return ids, mask


@pytest.fixture(scope="module")
def prefix_cases(model):
    out = {}
    for batch in (1, 2):
        heads, tails, _ = _prompts(model, batch)
        out[batch] = _reforward_greedy(model, [torch.cat([h, t]) for h, t in zip(heads, tails)], NEW)
    return out


@pytest.mark.parametrize("left", [False, True], ids=["right-padded", "left-padded"])
@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "session"])
@pytest.mark.parametrize("batch", [1, 2], ids=["shared-prefix", "batch-prefix"])
def test_generate_with_prefix(model, prefix_cases, batch, left, use_graph):
    heads, tails, prefix = _prompts(model, batch)
    want = prefix_cases[batch]
    # ... which is also what generate gives on the concatenated prompts
    whole, wmask = _padded([torch.cat([h, t]) for h, t in zip(heads, tails)], left)
    out = model.generate(whole, attention_mask=wmask, max_new_tokens=NEW, use_graph=use_graph)
    assert torch.equal(out[:, whole.shape[1]:], want)
    ids, mask = _padded(tails, left)
    before, lens_before = prefix.data.clone(), prefix.lens.clone()
    out = model.generate(ids, attention_mask=mask, max_new_tokens=NEW, use_graph=use_graph, prefix=prefix)
    assert torch.equal(out[:, :ids.shape[1]], ids) and torch.equal(out[:, ids.shape[1]:], want)
    assert torch.equal(prefix.data, before) and torch.equal(prefix.lens, lens_before) and prefix.max_len == 7


def test_generate_prefix_group_of_three_untied():
    """G = 3 with a separate lm_head."""
    model = _model(3, hidden_size=192, num_attention_heads=3, num_key_value_heads=1, tie_word_embeddings=False)
    ids = _ids(2, 11, seed=5)
    want = _reforward_greedy(model, list(ids), NEW)
    prefix = LlamaKVCache.allocate(model, 2, 4)
    model.prefill(ids[:, :4], _i32([4, 4]), prefix)
    for use_graph in (False, True):
        out = model.generate(ids[:, 4:], max_new_tokens=NEW, prefix=prefix, use_graph=use_graph)
        assert torch.equal(out[:, 7:], want)
    c = LlamaKVCache.allocate(model, 2, 11)
    full = LlamaKVCache.allocate(model, 2, 11)
    torch.testing.assert_close(model.prefill(ids, _i32([11, 11]), c, chunk=4),
                               model.prefill(ids, _i32([11, 11]), full), rtol=1e-4, atol=1e-4)


def test_copy_prefix(model):
    _, _, prefix = _prompts(model, 1)
    c = LlamaKVCache.allocate(model, 3, 12)
    c.data.fill_(7.0)
    assert c.copy_prefix_(prefix) is c
    assert c.lens.tolist() == [7, 7, 7] and c.max_len == 7
    assert all(torch.equal(c.data[:, :, b, :, :7], prefix.data[:, :, 0]) for b in range(3))
    assert (c.data[..., 7:, :] == 7.0).all()
    with pytest.raises(ValueError, match="capacity"):
        LlamaKVCache.allocate(model, 1, 6).copy_prefix_(prefix)
    with pytest.raises(ValueError, match="batch"):
        c.copy_prefix_(LlamaKVCache.allocate(model, 2, 12))
    with pytest.raises(ValueError, match="float64"):
        LlamaKVCache.allocate(model, 3, 12, dtype=torch.float64).copy_prefix_(prefix)
    other = llama_tiny(num_hidden_layers=1)
    with pytest.raises(ValueError, match="layers"):
        LlamaKVCache.allocate(other, 3, 12).copy_prefix_(prefix)
    wide = llama_tiny(hidden_size=256, num_attention_heads=4, num_key_value_heads=2)
    with pytest.raises(ValueError, match="heads"):
        LlamaKVCache.allocate(wide, 3, 12).copy_prefix_(prefix)


def test_value_errors(model):
    _, _, prefix = _prompts(model, 1)
    c = LlamaKVCache.allocate(model, 1, 12)
    c.copy_prefix_(prefix)
    with pytest.raises(ValueError, match="capacity"):
        model.extend(_ids(1, 6), c)
    with pytest.raises(ValueError, match="at least one column"):
        model.extend(_ids(1, 0), c)
    model.extend(_ids(1, 5), c)         # 7 + 5 fills it
    assert c.lens.tolist() == [12] and c.max_len == 12
    with pytest.raises(ValueError, match="max_position_embeddings"):
        model.generate(_ids(1, 200), max_new_tokens=50, prefix=prefix)      # 7 + 200 + 50 > 256
    model.generate(_ids(1, 200), max_new_tokens=49, prefix=prefix)
