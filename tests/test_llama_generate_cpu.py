"""Llama-family generation on the CPU (reference paths): the grouped-query decode reference against a
composition of the references that existed before it, the cache fill, the host guards, and the model --
prefill + decode_step against the full forward, greedy generate against decoding by full re-forward (with and
without a decode session), eos / pad, sampling -- and GPT-2's ``generate`` across the move of its prompt
compaction and token loops into ``models/_generate.py``.

The re-forward arm runs each sequence alone and unpadded through ``LlamaForCausalLM.forward`` (all the model
could do before it had a cache).  Seeds are fixed so that every step's top-2 logit gap on that arm exceeds
1e-3 (asserted), far above the 1e-4 to which the two arms' logits agree.
"""
import pytest
import torch

from databricks_distributed_deep_learning_amd import ops
from databricks_distributed_deep_learning_amd.models import LlamaKVCache, gpt2_tiny, llama_tiny
from databricks_distributed_deep_learning_amd.ops.attention import (attention_decode_gqa_reference,
                                                                   attention_decode_reference,
                                                                   kv_cache_fill_gqa_reference)
from databricks_distributed_deep_learning_amd.ops.llama import rope_qkv_reference

LENS = [1, 5, 9]
NEW = 10


# ------------------------------------------------------------------ the decode reference
@pytest.mark.parametrize("G", [1, 2, 3])
def test_decode_gqa_reference_is_rope_then_decode(G):
    """fp64: per batch row, ``rope_qkv_reference`` on the row as a length-1 sequence with ``table[n:n+1]``, then
    ``attention_decode_reference`` over the cache expanded by ``repeat_interleave(G)``."""
    B, Hkv, D, C = 3, 2, 16, 12
    H = Hkv * G
    lens = [0, C - 1, 5]
    g = torch.Generator().manual_seed(G)
    qkv = torch.randn(B, (H + 2 * Hkv) * D, generator=g, dtype=torch.float64)
    ck0 = torch.randn(B, Hkv, C, D, generator=g, dtype=torch.float64)
    cv0 = torch.randn(B, Hkv, C, D, generator=g, dtype=torch.float64)
    table = ops.rope_table(C, 10000.0, D).double()
    lt = torch.tensor(lens, dtype=torch.int32)

    ck, cv = ck0.clone(), cv0.clone()
    out = attention_decode_gqa_reference(qkv, table, ck, cv, lt, H, Hkv, C)
    assert out.shape == (B, H * D) and lt.tolist() == lens
    wk, wv = ck0.clone(), cv0.clone()
    for b, n in enumerate(lens):
        packed = rope_qkv_reference(qkv[b].view(1, 1, -1), table[n:n + 1], H, Hkv).view(1, 3 * H * D)
        ek = ck0[b:b + 1].repeat_interleave(G, 1).contiguous()
        ev = cv0[b:b + 1].repeat_interleave(G, 1).contiguous()
        want = attention_decode_reference(packed, ek, ev, lt[b:b + 1], H, C)
        assert (out[b] - want[0]).abs().max().item() <= 1e-12
        # position n of each KV head holds the rotated key and the value
        _, k, v = packed.view(3, H, D).unbind(0)
        assert torch.equal(ck[b, :, n], k[::G]) and torch.equal(cv[b, :, n], v[::G])
        wk[b, :, n], wv[b, :, n] = k[::G], v[::G]
    # ... and every other cache element is unchanged
    assert torch.equal(ck, wk) and torch.equal(cv, wv)
    # the public op routes CPU tensors to the reference; a dead tail of NaN cannot reach the output
    ck, cv = ck0.clone(), cv0.clone()
    for b, n in enumerate(lens):
        ck[b, :, n:], cv[b, :, n:] = float("nan"), float("nan")
    assert torch.equal(ops.attention_decode_gqa(qkv, table, ck, cv, lt, H, Hkv, C), out)


def test_decode_gqa_reference_rounds_rotated_operands_once():
    """bf16: the appended key is the fp32 rotation rounded once -- rope_qkv_reference's bits."""
    B, H, Hkv, D, C = 2, 4, 2, 64, 8
    g = torch.Generator().manual_seed(0)
    qkv = torch.randn(B, (H + 2 * Hkv) * D, generator=g).bfloat16()
    ck, cv = torch.zeros(B, Hkv, C, D).bfloat16(), torch.zeros(B, Hkv, C, D).bfloat16()
    table = ops.rope_table(C, 10000.0, D)
    lens = [3, 7]
    ops.attention_decode_gqa(qkv, table, ck, cv, torch.tensor(lens, dtype=torch.int32), H, Hkv, C)
    for b, n in enumerate(lens):
        packed = rope_qkv_reference(qkv[b].view(1, 1, -1), table[n:n + 1], H, Hkv).view(3, H, D)
        assert torch.equal(ck[b, :, n], packed[1, ::2]) and torch.equal(cv[b, :, n], packed[2, ::2])


@pytest.mark.parametrize("G", [1, 3])
def test_kv_cache_fill_gqa_reference(G):
    B, S, Hkv, D, C = 2, 5, 2, 16, 8
    H = Hkv * G
    proj = torch.randn(B, S, (H + 2 * Hkv) * D)
    packed = rope_qkv_reference(proj, ops.rope_table(S, 10000.0, D), H, Hkv)
    ck, cv = torch.full((B, Hkv, C, D), -3.0), torch.full((B, Hkv, C, D), -3.0)
    ops.kv_cache_fill_gqa(packed, ck, cv, H, Hkv)
    p5 = packed.view(B, S, 3, H, D)
    for j in range(Hkv):
        assert torch.equal(ck[:, j, :S], p5[:, :, 1, j * G]) and torch.equal(cv[:, j, :S], p5[:, :, 2, j * G])
    assert (ck[:, :, S:] == -3.0).all() and (cv[:, :, S:] == -3.0).all()
    ck2, cv2 = torch.zeros_like(ck), torch.zeros_like(cv)
    kv_cache_fill_gqa_reference(packed, ck2, cv2, H, Hkv)
    assert torch.equal(ck2[:, :, :S], ck[:, :, :S]) and torch.equal(cv2[:, :, :S], cv[:, :, :S])


def test_host_guards():
    B, H, Hkv, D, C = 2, 4, 2, 16, 4
    ck, cv = torch.zeros(B, Hkv, C, D), torch.zeros(B, Hkv, C, D)
    lens = torch.zeros(B, dtype=torch.int32)
    qkv = torch.randn(B, (H + 2 * Hkv) * D)
    table = ops.rope_table(8, 10000.0, D)
    ops.attention_decode_gqa(qkv, table, ck, cv, lens, H, Hkv, C)
    with pytest.raises(ValueError, match="capacity"):
        ops.attention_decode_gqa(qkv, table, ck, cv, lens, H, Hkv, C + 1)
    with pytest.raises(ValueError, match="at least 1"):
        ops.attention_decode_gqa(qkv, table, ck, cv, lens, H, Hkv, 0)
    with pytest.raises(ValueError, match="rotary table"):
        ops.attention_decode_gqa(qkv, table[:3], ck, cv, lens, H, Hkv, C)
    with pytest.raises(ValueError, match="multiple of num_kv_heads"):
        ops.attention_decode_gqa(torch.randn(B, 7 * D), table, torch.zeros(B, 3, C, D), torch.zeros(B, 3, C, D), lens,
                                 4, 3, C)
    with pytest.raises(RuntimeError, match="autograd"):
        ops.attention_decode_gqa(qkv.clone().requires_grad_(), table, ck, cv, lens, H, Hkv, 1)
    with pytest.raises(ValueError, match="cache must be"):
        ops.attention_decode_gqa(qkv, table, torch.zeros(B, H, C, D), torch.zeros(B, H, C, D), lens, H, Hkv, C)
    with pytest.raises(ValueError, match="contiguous"):
        big = torch.zeros(B, Hkv, C, 2 * D)
        ops.attention_decode_gqa(qkv, table, big[..., :D], big[..., D:], lens, H, Hkv, C)
    with pytest.raises(ValueError, match="lens"):
        ops.attention_decode_gqa(qkv, table, ck, cv, lens.long(), H, Hkv, C)
    packed = torch.randn(B, C + 1, 3 * H * D)
    with pytest.raises(ValueError, match="capacity"):
        ops.kv_cache_fill_gqa(packed, ck, cv, H, Hkv)
    with pytest.raises(ValueError, match="multiple of num_kv_heads"):
        ops.kv_cache_fill_gqa(packed[:, :2], ck, cv, H, 3)
    with pytest.raises(RuntimeError, match="autograd"):
        ops.kv_cache_fill_gqa(packed[:, :2].clone().requires_grad_(), ck, cv, H, Hkv)


# ------------------------------------------------------------------ the model
def _model(seed=0, **kw):
    torch.manual_seed(seed)
    # a wider init than the default 0.02: the logits of a random tiny model are otherwise nearly flat
    return llama_tiny(initializer_range=0.2, **kw).eval()


def _prompts(seed, side, vocab=1000):
    """input_ids [3, 9], attention_mask, and the bare prompts."""
    g = torch.Generator().manual_seed(seed)
    S = max(LENS)
    rows = [torch.randint(0, vocab, (n,), generator=g) for n in LENS]
    ids = torch.full((len(LENS), S), 7, dtype=torch.long)      # pad content must not matter
    mask = torch.zeros(len(LENS), S, dtype=torch.long)
    for b, r in enumerate(rows):
        sl = slice(0, len(r)) if side == "right" else slice(S - len(r), S)
        ids[b, sl] = r
        mask[b, sl] = 1
    return ids, mask, rows


def _reforward_greedy(model, rows, steps):
    """Greedy decoding by full re-forward, each sequence alone: tokens [B, steps], logits [B, steps, V]."""
    toks, logs = [], []
    with torch.no_grad():
        for r in rows:
            seq, t_row, l_row = r.clone(), [], []
            for _ in range(steps):
                lg = model(seq[None])[0, -1]
                l_row.append(lg)
                t_row.append(lg.argmax())
                seq = torch.cat([seq, t_row[-1][None]])
            toks.append(torch.stack(t_row))
            logs.append(torch.stack(l_row))
    return torch.stack(toks), torch.stack(logs)


@pytest.fixture(scope="module")
def greedy_case():
    model = _model(0)
    _, _, rows = _prompts(1, "right")
    want, want_logits = _reforward_greedy(model, rows, NEW)
    top2 = want_logits.topk(2, -1).values
    gap = (top2[..., 0] - top2[..., 1]).min().item()
    print(f"min top-2 gap on the re-forward arm: {gap:.4e}")
    assert gap > 1e-3
    return model, want, want_logits


def test_prefill_and_decode_step_logits_equal_forward(greedy_case):
    """Unequal prompt lengths; teacher-forced on the re-forward arm's tokens."""
    model, want, want_logits = greedy_case
    _, _, rows = _prompts(1, "right")
    S = max(LENS)
    comp = torch.zeros(3, S, dtype=torch.long)
    for b, r in enumerate(rows):
        comp[b, :len(r)] = r
    cache = LlamaKVCache.allocate(model, 3, S + NEW)
    assert cache.data.shape == (2, 2, 3, 1, S + NEW, 64) and cache.capacity == S + NEW
    logits = model.prefill(comp, torch.tensor(LENS, dtype=torch.int32), cache)
    assert logits.shape == (3, 1000)
    for t in range(NEW):
        err = (logits - want_logits[:, t]).abs().max().item()
        assert err < 1e-4, (t, err)
        if t + 1 < NEW:
            logits = model.decode_step(want[:, t], cache)
    assert cache.lens.tolist() == [n + NEW - 1 for n in LENS] and cache.max_len == S + NEW - 1


@pytest.mark.parametrize("use_graph", [False, True], ids=["loop", "session"])
@pytest.mark.parametrize("side", ["right", "left"])
def test_greedy_generate_equals_reforward(greedy_case, side, use_graph):
    """Left padding goes through generate's mask path: the rows are compacted, positions start at 0."""
    model, want, _ = greedy_case
    ids, mask, _ = _prompts(1, side)
    out = model.generate(ids, attention_mask=mask, max_new_tokens=NEW, use_graph=use_graph)
    assert out.shape == (3, ids.shape[1] + NEW) and out.dtype == torch.long
    assert torch.equal(out[:, :ids.shape[1]], ids)          # each row as given, padding included
    assert torch.equal(out[:, ids.shape[1]:], want)
    if use_graph:
        sess = model.decode_session
        assert sess is not None and sess.graph is None and sess.cache.data.shape[3] == 1     # eager, Hkv heads
        model.generate(ids, attention_mask=mask, max_new_tokens=NEW, use_graph=True)
        assert model.decode_session is sess


def test_generate_group_of_three_untied_and_training_mode():
    """G = 3 with a separate lm_head, no mask; eval semantics whatever ``model.training`` says."""
    model = _model(3, hidden_size=192, num_attention_heads=3, num_key_value_heads=1, tie_word_embeddings=False)
    g = torch.Generator().manual_seed(5)
    ids = torch.randint(0, 1000, (2, 6), generator=g)
    want, _ = _reforward_greedy(model, list(ids), 5)
    model.train()
    assert torch.equal(model.generate(ids, max_new_tokens=5)[:, 6:], want)
    assert torch.equal(model.generate(ids, max_new_tokens=5, use_graph=True)[:, 6:], want)
    assert model.training


@pytest.mark.parametrize("use_graph", [False, True], ids=["loop", "session"])
def test_eos_pads_and_exits_early(greedy_case, use_graph):
    model, free, _ = greedy_case
    ids, mask, rows = _prompts(1, "right")
    # a token that row 0 produces first at some step and the other rows never do within the horizon
    step = next(i for i in range(1, NEW - 1) if int(free[0, i]) not in free[0, :i].tolist()
                and all(int(free[0, i]) not in free[b].tolist() for b in (1, 2)))
    eos = int(free[0, step])
    out = model.generate(ids, attention_mask=mask, max_new_tokens=NEW, eos_token_id=eos, pad_token_id=999,
                         use_graph=use_graph)
    new = out[:, ids.shape[1]:]
    assert new.shape[1] == NEW
    assert torch.equal(new[0, :step + 1], free[0, :step + 1]) and (new[0, step + 1:] == 999).all()
    assert torch.equal(new[1:], free[1:])           # the finished row does not disturb the others
    out = model.generate(ids, attention_mask=mask, max_new_tokens=NEW, eos_token_id=eos, use_graph=use_graph)
    assert (out[0, ids.shape[1] + step + 1:] == eos).all()          # pad defaults to eos
    # every row finished: the loop stops there
    one = model.generate(rows[0][None], max_new_tokens=NEW, eos_token_id=eos, pad_token_id=999, use_graph=use_graph)
    assert one.shape == (1, LENS[0] + step + 1) and int(one[0, -1]) == eos


@pytest.mark.parametrize("use_graph", [False, True], ids=["loop", "session"])
def test_sampling_repeatable_and_top_k_1_is_greedy(greedy_case, use_graph):
    model = greedy_case[0]
    ids, mask, _ = _prompts(1, "left")
    kw = dict(attention_mask=mask, max_new_tokens=8, do_sample=True, temperature=0.7, top_k=20, use_graph=use_graph)
    a = model.generate(ids, generator=torch.Generator().manual_seed(11), **kw)
    b = model.generate(ids, generator=torch.Generator().manual_seed(11), **kw)
    c = model.generate(ids, generator=torch.Generator().manual_seed(12), **kw)
    assert torch.equal(a, b) and not torch.equal(a, c)
    greedy = model.generate(ids, attention_mask=mask, max_new_tokens=8)
    k1 = model.generate(ids, attention_mask=mask, max_new_tokens=8, do_sample=True, top_k=1, use_graph=use_graph,
                        generator=torch.Generator().manual_seed(3))
    assert torch.equal(k1, greedy)
    assert not torch.equal(a, greedy)


def test_generate_value_errors():
    model = _model(0)
    ids = torch.randint(0, 1000, (2, 6))
    with pytest.raises(ValueError, match="contiguous"):
        model.generate(ids, attention_mask=torch.tensor([[1, 0, 1, 1, 1, 1], [1, 1, 1, 1, 1, 1]]), max_new_tokens=2)
    with pytest.raises(ValueError, match="max_position_embeddings"):
        model.generate(ids, max_new_tokens=256 - 6 + 1)
    with pytest.raises(ValueError, match="max_new_tokens"):
        model.generate(ids, max_new_tokens=0)
    with pytest.raises(ValueError, match="temperature"):
        model.generate(ids, do_sample=True, temperature=0.0)
    with pytest.raises(TypeError):
        model.generate(ids, prefill_chunk=2)            # not offered for this family
    cache = LlamaKVCache.allocate(model, 2, 7)
    logits = model.prefill(ids, torch.tensor([6, 6], dtype=torch.int32), cache)
    model.decode_step(logits.argmax(-1), cache)         # position 6: the last slot
    with pytest.raises(ValueError, match="capacity"):
        model.decode_step(logits.argmax(-1), cache)
    with pytest.raises(ValueError, match="capacity"):
        LlamaKVCache.allocate(model, 2, 257)
    with pytest.raises(ValueError, match="capacity"):
        model.prefill(torch.zeros(2, 8, dtype=torch.long), torch.tensor([8, 8], dtype=torch.int32), cache)


# ------------------------------------------------------------------ GPT-2 across the helper refactor
# Computed with the commit before models/_generate.py existed (gpt2_tiny(dropout=0, initializer_range=0.2) under
# torch.manual_seed(0); prompts torch.randint(0, 1000, (3, 9)) from Generator seed 1; row 0 left-padded to one
# token, row 1 right-padded to five, row 2 full).
GPT2_GREEDY = [[951, 843, 830, 316, 326, 326, 826, 326], [294, 441, 538, 819, 826, 826, 981, 17],
               [395, 826, 284, 726, 726, 397, 397, 410]]
GPT2_SAMPLE = [[777, 835, 310, 998, 838, 838, 748, 326], [276, 749, 642, 826, 310, 168, 718, 497],
               [820, 397, 630, 726, 726, 397, 397, 155]]
GPT2_SAMPLE_SESSION = [[217, 217, 372, 826, 310, 397, 758, 441], [294, 441, 168, 326, 538, 168, 845, 845],
                       [872, 572, 483, 630, 432, 754, 826, 744]]
GPT2_EOS = [[951, 843, 830, 316, 999, 999, 999, 999], [294, 441, 538, 819, 826, 826, 981, 17],
            [395, 826, 284, 726, 726, 397, 397, 410]]


def test_gpt2_generate_is_unchanged_by_the_shared_helpers():
    torch.manual_seed(0)
    model = gpt2_tiny(dropout=0.0, initializer_range=0.2).eval()
    ids = torch.randint(0, 1000, (3, 9), generator=torch.Generator().manual_seed(1))
    mask = torch.ones(3, 9, dtype=torch.long)
    mask[0, :8] = 0
    mask[1, 5:] = 0
    for use_graph in (False, True):
        out = model.generate(ids, attention_mask=mask, max_new_tokens=8, use_graph=use_graph)
        assert out[:, 9:].tolist() == GPT2_GREEDY
        out = model.generate(ids, attention_mask=mask, max_new_tokens=8, eos_token_id=316, pad_token_id=999,
                             use_graph=use_graph)
        assert out[:, 9:].tolist() == GPT2_EOS
    kw = dict(attention_mask=mask, max_new_tokens=8, do_sample=True, temperature=0.7, top_k=20)
    out = model.generate(ids, generator=torch.Generator().manual_seed(11), **kw)
    assert out[:, 9:].tolist() == GPT2_SAMPLE
    out = model.generate(ids, generator=torch.Generator().manual_seed(11), use_graph=True, **kw)
    assert out[:, 9:].tolist() == GPT2_SAMPLE_SESSION
