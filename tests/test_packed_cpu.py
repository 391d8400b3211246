"""Packed-sequence pretraining on the reference path (CPU): ``ops.doc_bounds``, the document mask of
``attention_reference``, ``rope_qkv(positions=...)``, ``position_ids`` in the Llama and GPT-2 models, the
loader's ``docs_per_row`` and the training loop.

Model comparisons run in fp32 (the reference attention computes in fp32 whatever it is given).  A packed row
and its documents alone do the same arithmetic on the same numbers except for the order of fp32 sums (and
exact zeros added where a key is masked), so the tolerance is rtol 1e-4 / atol 1e-5 on O(0.1 .. 1) logits
and O(1e-2) gradients: a few hundred fp32 roundings (6e-8 each) through two layers, with room to spare, and
four orders of magnitude below what a leaked key or a run-on position changes (asserted: the unpacked
forward of the same ids differs by more than 1e-3).
"""
import copy
import math

import pytest
import torch

from databricks_distributed_deep_learning_amd import ops
from databricks_distributed_deep_learning_amd.data import SyntheticTokens
from databricks_distributed_deep_learning_amd.ops.attention import attention_reference
from databricks_distributed_deep_learning_amd.ops.llama import rope_qkv_reference


def positions_of(starts, S):
    """position_ids [len(starts), S] from per-row lists of document start indices (each begins with 0)."""
    pos = torch.empty(len(starts), S, dtype=torch.long)
    for b, st in enumerate(starts):
        assert st[0] == 0 and list(st) == sorted(set(st)) and st[-1] < S
        first = torch.zeros(S, dtype=torch.long)
        for s in st:
            first[s:] = s
        pos[b] = torch.arange(S) - first
    return pos


def spans(st, S):
    return list(zip(st, list(st[1:]) + [S]))


# ------------------------------------------------------------------ doc_bounds
def test_doc_bounds_values():
    S = 12
    starts = [[0, 1, 2, 7], [0], [0, 11]]
    pos = positions_of(starts, S)
    for p in (pos, pos.to(torch.int32)):
        ds, de = ops.doc_bounds(p)
        assert ds.dtype == de.dtype == torch.int32 and ds.shape == de.shape == (3, S)
        for b, st in enumerate(starts):
            for a, e in spans(st, S):
                assert (ds[b, a:e] == a).all() and (de[b, a:e] == e).all()
    # a changed tensor gives changed bounds (nothing is kept between calls)
    pos[1, 5:] = torch.arange(S - 5)
    ds2, de2 = ops.doc_bounds(pos)
    assert ds2[1, 4] == 0 and de2[1, 4] == 5 and ds2[1, 5] == 5 and de2[1, 5] == S


@pytest.mark.parametrize("bad", [
    torch.tensor([[1, 2, 3]]),                   # a row that does not start at 0
    torch.tensor([[0, 1, 3]]),                   # a jump
    torch.tensor([[0, 1, 1]]),                   # a repeat
    torch.tensor([[0, 1, 2], [0, -1, 0]]),       # a negative entry
    torch.tensor([[0, 2, 3]]),                   # a document that starts at 2
    torch.tensor([0, 1, 2]),                     # not [B, S]
    torch.tensor([[0.0, 1.0]]),                  # not an integer tensor
])
def test_doc_bounds_rejects(bad):
    with pytest.raises(ValueError):
        ops.doc_bounds(bad)


# ------------------------------------------------------------------ attention_reference
@pytest.mark.parametrize("S,starts", [(11, [[0, 4, 5], [0]]), (70, [[0, 1, 2, 3, 64], [0, 63, 65]])])
def test_attention_reference_doc_mask(S, starts):
    H, D = 2, 16
    g = torch.Generator().manual_seed(S)
    qkv = torch.randn(len(starts), S, 3 * H * D, generator=g)
    ds, de = ops.doc_bounds(positions_of(starts, S))
    for arg in (ds, (ds, de)):
        out = ops.attention(qkv, H, None, 0.0, False, causal=True, doc_start=arg)
        for b, st in enumerate(starts):
            for a, e in spans(st, S):
                alone = attention_reference(qkv[b:b + 1, a:e], H, causal=True)
                torch.testing.assert_close(out[b:b + 1, a:e], alone, rtol=1e-5, atol=1e-6)
    # the first token of a document sees itself alone: out = its v
    v = qkv.view(len(starts), S, 3, H * D)[:, :, 2]
    for b, st in enumerate(starts):
        torch.testing.assert_close(out[b, st], v[b, st], rtol=1e-6, atol=1e-6)
    # the key bias composes on top
    bias = torch.zeros(len(starts), S)
    bias[:, S - 2] = -10000.0
    both = ops.attention(qkv, H, bias, 0.0, False, causal=True, doc_start=ds)
    a, e = spans(starts[0], S)[-1]
    alone = attention_reference(qkv[:1, a:e], H, bias[:1, a:e], causal=True)
    torch.testing.assert_close(both[:1, a:e], alone, rtol=1e-5, atol=1e-6)


def test_doc_start_needs_causal():
    qkv = torch.randn(1, 5, 3 * 16)
    ds = torch.zeros(1, 5, dtype=torch.int32)
    for fn in (ops.attention, attention_reference):
        with pytest.raises(ValueError, match="causal"):
            fn(qkv, 1, None, 0.0, False, causal=False, doc_start=ds)
    with pytest.raises(ValueError, match="int32"):
        ops.attention(qkv, 1, None, 0.0, False, causal=True, doc_start=ds.long())


# ------------------------------------------------------------------ rope_qkv(positions=...)
@pytest.mark.parametrize("H,Hkv", [(2, 2), (4, 2), (9, 3)])
def test_rope_positions_reference(H, Hkv):
    B, S, D = 2, 70, 64
    g = torch.Generator().manual_seed(H)
    table = ops.rope_table(128, 10000.0, D)
    x = torch.randn(B, S, (H + 2 * Hkv) * D, generator=g, dtype=torch.float64)
    dy = torch.randn(B, S, 3 * H * D, generator=g, dtype=torch.float64)

    def run(xx, pos):
        xx = xx.clone().requires_grad_(True)
        y = ops.rope_qkv(xx, table, H, Hkv) if pos is None else ops.rope_qkv(xx, table, H, Hkv, positions=pos)
        y.backward(dy)
        return y.detach(), xx.grad

    # arange is the call without the argument, bit for bit
    ar = torch.arange(S, dtype=torch.int32).expand(B, S).contiguous()
    y0, g0 = run(x, None)
    y1, g1 = run(x, ar)
    assert torch.equal(y0, y1) and torch.equal(g0, g1)
    # a packed row is, per document slice, that document rotated alone
    starts = [[0, 1, 33, 64], [0, 69]]
    pos = positions_of(starts, S).to(torch.int32)
    yp, gp = run(x, pos)
    for b, st in enumerate(starts):
        for a, e in spans(st, S):
            xa = x[b:b + 1, a:e].clone().requires_grad_(True)
            ya = ops.rope_qkv(xa, table, H, Hkv)
            ya.backward(dy[b:b + 1, a:e])
            assert torch.equal(yp[b:b + 1, a:e], ya.detach()) and torch.equal(gp[b:b + 1, a:e], xa.grad)
    assert not torch.equal(yp, y0)
    # S may pass the table as long as the positions stay inside it; a position outside is an error
    small = ops.rope_table(40, 10000.0, D)
    pos40 = positions_of([[0, 35], [0, 31, 62]], S).to(torch.int32)
    assert torch.equal(rope_qkv_reference(x, small, H, Hkv, pos40), rope_qkv_reference(x, table, H, Hkv, pos40))
    with pytest.raises(ValueError, match="positions"):
        ops.rope_qkv(x, small, H, Hkv, positions=ar)
    with pytest.raises(ValueError, match="positions"):
        ops.rope_qkv(x, table, H, Hkv, positions=ar - 1)
    with pytest.raises(ValueError, match="int32"):
        ops.rope_qkv(x, table, H, Hkv, positions=ar.long())


# ------------------------------------------------------------------ models: packed against alone
def _tiny(kind):
    from databricks_distributed_deep_learning_amd.models import gpt2_tiny, llama_tiny
    torch.manual_seed(0)
    return llama_tiny() if kind == "llama" else gpt2_tiny(dropout=0.0)


def _packed_labels(ids, starts):
    """next-token labels, -100 at the last token of every document"""
    B, S = ids.shape
    lab = torch.full_like(ids, -100)
    lab[:, :-1] = ids[:, 1:]
    for b, st in enumerate(starts):
        for s in st[1:]:
            lab[b, s - 1] = -100
    return lab


@pytest.mark.parametrize("kind", ["llama", "gpt2"])
def test_model_packed_equals_documents_alone(kind):
    S = 40
    starts = [[0, 1, 14, 30], [0, 25]]
    g = torch.Generator().manual_seed(3)
    ids = torch.randint(0, 1000, (2, S), generator=g)
    pos = positions_of(starts, S)
    labels = _packed_labels(ids, starts)
    model = _tiny(kind)

    # ---- logits
    model.eval()
    with torch.no_grad():
        packed = model(ids, position_ids=pos)
        plain = model(ids)
        for b, st in enumerate(starts):
            for a, e in spans(st, S):
                alone = model(ids[b:b + 1, a:e])
                torch.testing.assert_close(packed[b:b + 1, a:e], alone, rtol=1e-4, atol=1e-5)
        # position_ids=None is the call as it was; arange packs one document per row: the same numbers
        assert torch.equal(plain, model(ids, None, None, None))
        one = model(ids, position_ids=torch.arange(S).expand(2, S).contiguous())
        torch.testing.assert_close(one, plain, rtol=1e-4, atol=1e-5)
        assert (packed - plain).abs().max() > 1e-3          # packing is no rounding matter

    # ---- loss and gradients: the target-count-weighted mean of the documents' own losses
    model.train()
    ref = copy.deepcopy(model)
    loss, _ = model(ids, None, None, labels, position_ids=pos)
    loss.backward()
    n_all = int((labels != -100).sum())
    total = 0.0
    for b, st in enumerate(starts):
        for a, e in spans(st, S):
            n = e - a - 1                                   # a one-token document has no target
            assert n == int((labels[b, a:e] != -100).sum())
            if n:
                ld, _ = ref(ids[b:b + 1, a:e], None, None, labels[b:b + 1, a:e])
                total = total + ld * (n / n_all)
    total.backward()
    torch.testing.assert_close(loss, total.detach(), rtol=1e-5, atol=1e-6)
    for (name, p), (_, q) in zip(model.named_parameters(), ref.named_parameters()):
        assert p.grad is not None and q.grad is not None, name
        torch.testing.assert_close(p.grad, q.grad, rtol=1e-4, atol=1e-6, msg=lambda m: f"{name}: {m}")


@pytest.mark.parametrize("kind", ["llama", "gpt2"])
def test_model_rejects_bad_position_ids(kind):
    model = _tiny(kind).eval()
    ids = torch.randint(0, 1000, (1, 6))
    with pytest.raises(ValueError):
        model(ids, position_ids=torch.tensor([[0, 1, 2, 4, 5, 6]]))
    with pytest.raises(ValueError):
        model(ids, position_ids=torch.zeros(1, 5, dtype=torch.long))


# ------------------------------------------------------------------ loader
def test_loader_docs_per_row():
    kw = dict(batch_size=3, seq_len=37, vocab_size=500, seed=5, pool=3, causal_lm=True)
    base = SyntheticTokens(**kw)
    zero = SyntheticTokens(docs_per_row=0, **kw)
    for a, b in zip(base.pool, zero.pool):
        assert a.keys() == b.keys() and "position_ids" not in b
        assert all(torch.equal(a[k], b[k]) for k in ("input_ids", "labels")) and b["attention_mask"] is None
    for k in (1, 4, 37):
        ld = SyntheticTokens(docs_per_row=k, **kw)
        for a, b in zip(base.pool, ld.pool):
            assert torch.equal(a["input_ids"], b["input_ids"])
            pos = b["position_ids"]
            ds, de = ops.doc_bounds(pos)                    # raises unless the convention holds
            assert ((pos == 0).sum(1) == k).all()
            last = de.long() - 1 == torch.arange(37)[None, :]
            assert torch.equal(b["labels"] == -100, (a["labels"] == -100) | last)
            assert torch.equal(b["labels"][~last], a["labels"][~last])
    # padded rows keep their -100
    pad = dict(kw, pad_fraction=0.3)
    a, b = SyntheticTokens(**pad).pool[0], SyntheticTokens(docs_per_row=4, **pad).pool[0]
    last = ops.doc_bounds(b["position_ids"])[1].long() - 1 == torch.arange(37)[None, :]
    assert torch.equal(a["attention_mask"], b["attention_mask"])
    assert torch.equal(b["labels"] == -100, (a["labels"] == -100) | last)
    # the cuts differ between rows and between pool entries
    ld = SyntheticTokens(docs_per_row=4, **kw)
    assert not torch.equal(ld.pool[0]["position_ids"][0], ld.pool[0]["position_ids"][1])
    assert not torch.equal(ld.pool[0]["position_ids"], ld.pool[1]["position_ids"])
    with pytest.raises(ValueError, match="docs_per_row"):
        SyntheticTokens(docs_per_row=38, **kw)
    with pytest.raises(ValueError, match="causal_lm"):
        SyntheticTokens(batch_size=2, seq_len=8, docs_per_row=2)


def test_loader_resume_replays_packed_batches():
    kw = dict(batch_size=2, seq_len=16, vocab_size=100, seed=9, pool=3, causal_lm=True, docs_per_row=3)
    a = SyntheticTokens(**kw)
    for _ in range(4):
        a.next()
    st = a.state_dict()
    b = SyntheticTokens(**kw)
    b.load_state_dict(st)
    for _ in range(5):
        x, y = a.next(), b.next()
        assert all(torch.equal(x[k], y[k]) for k in ("input_ids", "labels", "position_ids"))


# ------------------------------------------------------------------ config, loop
def test_packed_preset_and_override():
    from databricks_distributed_deep_learning_amd.config import TrainConfig, apply_overrides, get_preset
    c, p = get_preset("llama_pretrain"), get_preset("llama_pretrain_packed")
    assert c.docs_per_row == 0 and p.docs_per_row == 8 and p == c.replace(docs_per_row=8)
    assert TrainConfig().docs_per_row == 0
    assert apply_overrides(c, ["--docs-per-row=4"], {}).docs_per_row == 4
    assert apply_overrides(c, [], {"DDL_DOCS_PER_ROW": "2"}).docs_per_row == 2


def test_llama_tiny_trains_packed_on_cpu():
    from databricks_distributed_deep_learning_amd.config import get_preset
    from databricks_distributed_deep_learning_amd.training.loop import Trainer
    cfg = get_preset("llama_pretrain_packed", model="llama_tiny", batch_size=4, seq_len=32, steps=2, warmup_steps=0,
                     dtype="fp32", backend="gloo", native="off", log_every=1, lr=3e-3, synthetic_pool=1,
                     docs_per_row=3)
    t = Trainer(cfg)
    b = t.loader.pool[0]
    assert ((b["position_ids"] == 0).sum(1) == 3).all()
    seen = []
    fwd = t.model.forward
    t.model.forward = lambda *a, **k: (seen.append(k.get("position_ids")), fwd(*a, **k))[1]
    losses = []
    out = t.run(callback=lambda step, loss: losses.append(loss))
    t.close()
    assert seen and all(p is b["position_ids"] for p in seen)
    assert out["steps"] == 2 and all(math.isfinite(x) for x in losses)
    assert len(losses) == 2 and losses[1] <= losses[0], losses
