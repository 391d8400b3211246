"""GPT-2 generation on the CPU (fp32, reference paths): the cached decode against greedy decoding by
full re-forward, the decode-attention reference against an explicit fp64 softmax (append, dead tail),
eos / pad handling, sampling, the host-side guards and the HF checkpoint layout.

The re-forward arm runs each sequence alone and unpadded through ``GPT2LMHeadModel.forward`` (what the
model could do before it had a cache).  Seeds are fixed so that every step's top-2 logit gap on that arm
exceeds 1e-3 (asserted), far above the 1e-4 to which the two arms' logits agree, so the token comparison
cannot hinge on a near-tie.
"""
import math

import pytest
import torch

from databricks_distributed_deep_learning_amd import ops
from databricks_distributed_deep_learning_amd.models import KVCache, gpt2_tiny
from databricks_distributed_deep_learning_amd.models.gpt2 import from_hf_state_dict, to_hf_state_dict
from databricks_distributed_deep_learning_amd.ops.attention import (attention_decode_reference,
                                                                   kv_cache_fill_reference)

LENS = [1, 5, 9]
NEW = 12


def _model(seed=0, **kw):
    torch.manual_seed(seed)
    # a wider init than the default 0.02: the logits of a random tiny model are otherwise nearly flat
    return gpt2_tiny(dropout=0.0, initializer_range=0.2, **kw).eval()


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


# ------------------------------------------------------------------ cached vs re-forward
@pytest.mark.parametrize("side", ["right", "left"])
def test_greedy_cached_equals_reforward(side):
    model = _model(0)
    ids, mask, rows = _prompts(1, side)
    want, want_logits = _reforward_greedy(model, rows, NEW)
    top2 = want_logits.topk(2, -1).values
    gap = (top2[..., 0] - top2[..., 1]).min().item()
    print(f"min top-2 gap on the re-forward arm: {gap:.4e}")
    assert gap > 1e-3

    out = model.generate(ids, attention_mask=mask, max_new_tokens=NEW)
    assert out.shape == (3, ids.shape[1] + NEW) and out.dtype == torch.long
    assert torch.equal(out[:, :ids.shape[1]], ids)          # each row as given, padding included
    assert torch.equal(out[:, ids.shape[1]:], want)

    # per-step logits: prefill + decode_step on the right-padded compaction, teacher-forced on `want`
    S = max(LENS)
    comp = torch.zeros(3, S, dtype=torch.long)
    for b, r in enumerate(rows):
        comp[b, :len(r)] = r
    cache = KVCache.allocate(model, 3, S + NEW)
    logits = model.prefill(comp, torch.tensor(LENS, dtype=torch.int32), cache)
    assert logits.shape == (3, 1000)
    for t in range(NEW):
        err = (logits - want_logits[:, t]).abs().max().item()
        assert err < 1e-4, (t, err)
        if t + 1 < NEW:
            logits = model.decode_step(want[:, t], cache)
    assert cache.lens.tolist() == [n + NEW - 1 for n in LENS] and cache.max_len == S + NEW - 1


def test_generate_without_mask_and_in_training_mode():
    """No mask: every row is a full prompt.  Eval semantics whatever ``model.training`` says."""
    model = _model(3)
    g = torch.Generator().manual_seed(5)
    ids = torch.randint(0, 1000, (2, 6), generator=g)
    want, _ = _reforward_greedy(model, list(ids), 5)
    assert torch.equal(model.generate(ids, max_new_tokens=5)[:, 6:], want)
    torch.manual_seed(0)
    noisy = gpt2_tiny(dropout=0.5, initializer_range=0.2)
    noisy.load_state_dict(model.state_dict())
    noisy.train()
    assert torch.equal(noisy.generate(ids, max_new_tokens=5)[:, 6:], want)
    assert noisy.training


def test_gelu_new_decode_matches_reforward():
    model = _model(4, activation_function="gelu_new")
    ids, mask, rows = _prompts(2, "left")
    want, _ = _reforward_greedy(model, rows, 6)
    assert torch.equal(model.generate(ids, attention_mask=mask, max_new_tokens=6)[:, ids.shape[1]:], want)


# ------------------------------------------------------------------ decode attention reference
def _explicit64(qkv_new, ck, cv, lens, H):
    B, D = qkv_new.shape[0], qkv_new.shape[1] // (3 * H)
    q, k, v = qkv_new.double().view(B, 3, H, D).unbind(1)
    out = torch.empty(B, H, D, dtype=torch.float64)
    for b in range(B):
        n = int(lens[b])
        for h in range(H):
            keys = torch.cat([ck[b, h, :n].double(), k[b, h][None]])
            vals = torch.cat([cv[b, h, :n].double(), v[b, h][None]])
            p = torch.softmax(keys @ q[b, h] / math.sqrt(D), 0)
            out[b, h] = p @ vals
    return out.reshape(B, H * D)


@pytest.mark.parametrize("lens", [[0, 3], [7, 0], [15, 9]])
def test_attention_decode_reference(lens):
    B, H, D, C = 2, 2, 16, 16
    g = torch.Generator().manual_seed(sum(lens))
    qkv = torch.randn(B, 3 * H * D, generator=g)
    ck0, cv0 = torch.randn(B, H, C, D, generator=g), torch.randn(B, H, C, D, generator=g)
    lt = torch.tensor(lens, dtype=torch.int32)
    want = _explicit64(qkv, ck0, cv0, lens, H)
    outs = []
    for fill in (None, 0.0, float("nan")):      # the dead tail as drawn, zeros, NaN
        ck, cv = ck0.clone(), cv0.clone()
        if fill is not None:
            for b, n in enumerate(lens):
                ck[b, :, n:] = fill
                cv[b, :, n:] = fill
        gk, gv = ck.clone(), cv.clone()
        out = attention_decode_reference(qkv, ck, cv, lt, H, max(lens) + 1)
        outs.append(out)
        torch.testing.assert_close(out.double(), want, atol=1e-5, rtol=1e-5)
        # append: cache[b, :, n_b] is the new K / V row, every other element is untouched
        _, k, v = qkv.view(B, 3, H, D).unbind(1)
        for b, n in enumerate(lens):
            assert torch.equal(ck[b, :, n], k[b]) and torch.equal(cv[b, :, n], v[b])
            gk[b, :, n], gv[b, :, n] = k[b], v[b]
        assert torch.equal(ck.view(torch.int32), gk.view(torch.int32))
        assert torch.equal(cv.view(torch.int32), gv.view(torch.int32))
        assert lt.tolist() == lens
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
    # a bound above n + 1 changes nothing; the public op routes CPU tensors to the reference
    ck, cv = ck0.clone(), cv0.clone()
    assert torch.equal(ops.attention_decode(qkv, ck, cv, lt, H, C), outs[0])
    if lens[0] == 0:    # a softmax over one key is exactly 1
        assert torch.equal(outs[0][0], qkv.view(B, 3, H * D)[0, 2])


def test_kv_cache_fill_reference():
    B, S, H, D, C = 2, 5, 2, 16, 8
    qkv = torch.randn(B, S, 3 * H * D)
    ck, cv = torch.full((B, H, C, D), -3.0), torch.full((B, H, C, D), -3.0)
    ops.kv_cache_fill(qkv, ck, cv, H)
    _, k, v = qkv.view(B, S, 3, H, D).permute(2, 0, 3, 1, 4).unbind(0)
    assert torch.equal(ck[:, :, :S], k) and torch.equal(cv[:, :, :S], v)
    assert (ck[:, :, S:] == -3.0).all() and (cv[:, :, S:] == -3.0).all()
    ck2, cv2 = torch.zeros_like(ck), torch.zeros_like(cv)
    kv_cache_fill_reference(qkv, ck2, cv2, H)
    assert torch.equal(ck2[:, :, :S], k)


def test_linear_small_m_reference_path():
    x, w, b, r = torch.randn(3, 16), torch.randn(5, 16), torch.randn(5), torch.randn(3, 5)
    assert torch.equal(ops.linear_small_m(x, w, b, "gelu"), ops.linear(x, w, b, "gelu"))
    assert torch.equal(ops.linear_small_m(x, w, b, residual=r), ops.linear(x, w, b, residual=r))


# ------------------------------------------------------------------ eos, sampling
def test_eos_pads_and_exits_early():
    model = _model(0)
    ids, mask, rows = _prompts(1, "right")
    free = model.generate(ids, attention_mask=mask, max_new_tokens=NEW)[:, ids.shape[1]:]
    # a token that row 0 produces at step 3 and the other rows never do within the horizon
    eos = int(free[0, 3])
    assert eos not in free[0, :3].tolist() and all(eos not in free[b].tolist() for b in (1, 2))
    out = model.generate(ids, attention_mask=mask, max_new_tokens=NEW, eos_token_id=eos, pad_token_id=999)
    new = out[:, ids.shape[1]:]
    assert new.shape[1] == NEW
    assert torch.equal(new[0, :4], free[0, :4]) and (new[0, 4:] == 999).all()
    assert torch.equal(new[1:], free[1:])           # the finished row does not disturb the others
    # pad defaults to eos
    out = model.generate(ids, attention_mask=mask, max_new_tokens=NEW, eos_token_id=eos)
    assert (out[0, ids.shape[1] + 4:] == eos).all()
    # every row finished: the loop stops there
    one = model.generate(rows[0][None], max_new_tokens=NEW, eos_token_id=eos, pad_token_id=999)
    assert one.shape == (1, LENS[0] + 4) and int(one[0, -1]) == eos


def test_sampling_repeatable_and_top_k_1_is_greedy():
    model = _model(0)
    ids, mask, _ = _prompts(1, "left")
    kw = dict(attention_mask=mask, max_new_tokens=8, do_sample=True, temperature=0.7, top_k=20)
    a = model.generate(ids, generator=torch.Generator().manual_seed(11), **kw)
    b = model.generate(ids, generator=torch.Generator().manual_seed(11), **kw)
    c = model.generate(ids, generator=torch.Generator().manual_seed(12), **kw)
    assert torch.equal(a, b) and not torch.equal(a, c)
    greedy = model.generate(ids, attention_mask=mask, max_new_tokens=8)
    k1 = model.generate(ids, attention_mask=mask, max_new_tokens=8, do_sample=True, top_k=1,
                        generator=torch.Generator().manual_seed(3))
    assert torch.equal(k1, greedy)
    assert not torch.equal(a, greedy)


# ------------------------------------------------------------------ guards
def test_value_errors():
    model = _model(0)
    ids = torch.randint(0, 1000, (2, 6))
    for bad in ([[1, 0, 1, 1, 1, 1], [1, 1, 1, 1, 1, 1]], [[0, 0, 0, 0, 0, 0], [1, 1, 1, 1, 1, 1]],
                [[0, 1, 1, 0, 0, 1], [1, 1, 1, 1, 1, 1]]):
        with pytest.raises(ValueError, match="contiguous"):
            model.generate(ids, attention_mask=torch.tensor(bad), max_new_tokens=2)
    with pytest.raises(ValueError, match="n_positions"):
        model.generate(ids, max_new_tokens=128 - 6 + 1)
    model.generate(ids[:, :2], max_new_tokens=2)
    # capacity: the bound on n + 1 may not exceed C, checked on the host
    B, H, D, C = 2, 2, 16, 4
    ck, cv = torch.zeros(B, H, C, D), torch.zeros(B, H, C, D)
    lens = torch.zeros(B, dtype=torch.int32)
    with pytest.raises(ValueError, match="capacity"):
        ops.attention_decode(torch.randn(B, 3 * H * D), ck, cv, lens, H, C + 1)
    cache = KVCache.allocate(model, 2, 7)
    logits = model.prefill(ids, torch.tensor([6, 6], dtype=torch.int32), cache)
    model.decode_step(logits.argmax(-1), cache)         # position 6: the last slot
    with pytest.raises(ValueError, match="capacity"):
        model.decode_step(logits.argmax(-1), cache)
    with pytest.raises(ValueError, match="capacity"):
        KVCache.allocate(model, 2, 129)
    with pytest.raises(RuntimeError, match="autograd"):
        ops.attention_decode(torch.randn(B, 3 * H * D, requires_grad=True), ck, cv, lens, H, 1)


# ------------------------------------------------------------------ HF layout
def test_hf_round_trip_generates_the_same_tokens():
    model = _model(0)
    ids, mask, _ = _prompts(1, "right")
    want = model.generate(ids, attention_mask=mask, max_new_tokens=6)
    hf = to_hf_state_dict(model.state_dict(), 2)
    assert hf["transformer.h.0.attn.c_attn.weight"].shape == (128, 384)     # Conv1D: [in, out]
    torch.manual_seed(9)
    other = gpt2_tiny(dropout=0.0).eval()
    other.load_state_dict(from_hf_state_dict(hf, 2))
    assert torch.equal(other.generate(ids, attention_mask=mask, max_new_tokens=6), want)
