"""BERT masked-LM pretraining on the reference (CPU, fp32) paths: the ops with ignored targets, the
tied-decoder model, its HF state-dict mapping, the synthetic MLM batches and the preset."""
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

from databricks_distributed_deep_learning_amd import ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------ cross_entropy(ignore_index)
def test_cross_entropy_ignore_matches_torch():
    torch.manual_seed(0)
    x = torch.randn(9, 11, requires_grad=True)
    xr = x.detach().clone().requires_grad_(True)
    y = torch.tensor([3, -100, 10, 0, -100, 5, 5, -100, 1])
    loss = ops.cross_entropy(x, y, ignore_index=-100)
    ref = F.cross_entropy(xr, y, ignore_index=-100)
    torch.testing.assert_close(loss, ref)
    (loss * 2).backward()
    (ref * 2).backward()
    torch.testing.assert_close(x.grad, xr.grad)
    assert x.grad[1].abs().max() == 0


def test_cross_entropy_all_ignored_is_zero():
    x = torch.randn(4, 7, requires_grad=True)
    loss = ops.cross_entropy(x, torch.full((4,), -100), ignore_index=-100)
    assert loss.item() == 0.0
    loss.backward()
    assert x.grad.abs().max().item() == 0.0 and torch.isfinite(x.grad).all()


def test_cross_entropy_ignore_gradcheck():
    torch.manual_seed(1)
    x = torch.randn(4, 7, dtype=torch.float64, requires_grad=True)
    y = torch.tensor([2, -100, 6, 0])
    assert torch.autograd.gradcheck(lambda t: ops.cross_entropy(t, y, ignore_index=-100), (x,))


def test_cross_entropy_without_ignore_index_unchanged():
    torch.manual_seed(2)
    x = torch.randn(6, 10)
    y = torch.randint(0, 10, (6,))
    a = ops.cross_entropy(x, y)
    assert torch.equal(a, F.cross_entropy(x.float(), y))
    assert torch.equal(a, ops.cross_entropy(x, y, ignore_index=None))


# ------------------------------------------------------------------ gather_rows
def _gather_case(dtype=torch.float64):
    torch.manual_seed(3)
    h = torch.randn(10, 8, dtype=dtype, requires_grad=True)
    pos = torch.tensor([0, 4, 7, 9, 0, 0])            # slots 4, 5: padding, aliasing row 0 of slot 0
    lab = torch.tensor([5, 1, 2, 3, -100, -100])
    return h, pos, lab


def test_gather_rows_gradcheck_with_aliasing_padded_slot():
    h, pos, lab = _gather_case()
    out = ops.gather_rows(h, pos, lab, -100)
    assert torch.equal(out, h[pos])                    # every slot receives its row, padded ones too
    # as a function of h the VALID slots are differentiable; the padded ones are constants
    assert torch.autograd.gradcheck(lambda t: ops.gather_rows(t, pos, lab, -100)[lab != -100], (h,))
    dy = torch.randn(6, 8, dtype=h.dtype)
    out.backward(dy)
    want = torch.zeros_like(h)
    want[pos[:4]] = dy[:4]
    assert torch.equal(h.grad, want)                   # row 0 holds slot 0's gradient alone


def test_gather_rows_per_sequence_positions():
    torch.manual_seed(4)
    h = torch.randn(3, 5, 8)
    pos = torch.tensor([[0, 4], [2, 3], [1, 0]])
    out = ops.gather_rows(h, pos)
    want = torch.stack([h[b, pos[b, j]] for b in range(3) for j in range(2)])
    assert torch.equal(out, want)


# ------------------------------------------------------------------ linear_cross_entropy
@pytest.mark.parametrize("V", [16, 18])
def test_linear_cross_entropy_matches_composition(V):
    torch.manual_seed(5)
    x = torch.randn(7, 8, requires_grad=True)
    w = torch.randn(V, 8, requires_grad=True)
    b = torch.randn(V, requires_grad=True)
    y = torch.randint(0, V, (7,))
    y[2] = -100
    y[0] = V - 1
    loss, logits = ops.linear_cross_entropy(x, w, b, y, -100, return_logits=True)
    xr, wr, br = (t.detach().clone().requires_grad_(True) for t in (x, w, b))
    ref_logits = F.linear(xr, wr, br)
    ref = F.cross_entropy(ref_logits, y, ignore_index=-100)
    torch.testing.assert_close(loss, ref)
    torch.testing.assert_close(logits, ref_logits.detach())
    assert not logits.requires_grad
    loss.backward()
    ref.backward()
    for got, want in ((x.grad, xr.grad), (w.grad, wr.grad), (b.grad, br.grad)):
        torch.testing.assert_close(got, want)
    torch.testing.assert_close(ops.linear_cross_entropy(x, w, b, y), ref)


# ------------------------------------------------------------------ model
def _tiny():
    from databricks_distributed_deep_learning_amd.models import bert_tiny_pretraining
    torch.manual_seed(6)
    return bert_tiny_pretraining(dropout=0.0)


def test_pretraining_decoder_is_tied_and_registered_once():
    m = _tiny()
    assert m.decoder_weight is m.bert.embeddings.word_embeddings.weight
    names = [n for n, p in m.named_parameters() if p is m.decoder_weight]
    assert names == ["bert.embeddings.word_embeddings.weight"]
    assert len({id(p) for p in m.parameters()}) == len(list(m.parameters()))
    assert m.mlm_bias.shape == (m.config.vocab_size,)


def test_pretraining_positions_path_equals_dense_labels_path():
    m = _tiny()
    B, S, P, V = 3, 32, 6, m.config.vocab_size
    g = torch.Generator().manual_seed(7)
    ids = torch.randint(0, V, (B, S), generator=g)
    mask = torch.ones(B, S, dtype=torch.int64)
    mask[1, 28:] = 0
    pos = torch.stack([torch.randperm(28, generator=g)[:P].sort().values for _ in range(B)])
    lab = torch.randint(0, V, (B, P), generator=g)
    lab[0, 4:] = -100                                  # padded slots: position 0, which row 2 also predicts
    pos[0, 4:] = 0
    pos[2, 0] = 0
    nsp = torch.randint(0, 2, (B,), generator=g)
    dense = torch.full((B, S), -100, dtype=torch.int64)
    for b in range(B):
        for j in range(P):
            if lab[b, j] != -100:
                dense[b, pos[b, j]] = lab[b, j]

    def grads(**kw):
        m.zero_grad(set_to_none=True)
        loss, (mlm_logits, nsp_logits) = m(ids, mask, None, next_sentence_label=nsp, **kw)
        assert mlm_logits is None and nsp_logits.shape == (B, 2)
        loss.backward()
        return loss.detach(), {n: p.grad.clone() for n, p in m.named_parameters()}

    l1, g1 = grads(masked_lm_positions=pos, masked_lm_labels=lab)
    l2, g2 = grads(masked_lm_labels=dense)
    torch.testing.assert_close(l1, l2, atol=1e-5, rtol=1e-5)
    assert set(g1) == set(g2) == {n for n, _ in m.named_parameters()}
    for n in g1:
        torch.testing.assert_close(g1[n], g2[n], atol=1e-5, rtol=1e-4, msg=lambda s, n=n: f"{n}: {s}")
    # inference: no labels -> logits of the gathered rows, no loss
    with torch.no_grad():
        loss, (mlm_logits, _) = m(ids, mask, None, masked_lm_positions=pos)
    assert loss is None and mlm_logits.shape == (B * P, V)


def test_pretraining_hf_state_dict_round_trip():
    from databricks_distributed_deep_learning_amd.models import bert, bert_tiny
    m = _tiny()
    sd = m.state_dict()
    L = m.config.num_hidden_layers
    hf = bert.to_hf_state_dict(sd, L)
    for k in ("cls.predictions.transform.dense.weight", "cls.predictions.transform.LayerNorm.bias",
              "cls.predictions.bias", "cls.predictions.decoder.weight", "cls.seq_relationship.weight"):
        assert k in hf, k
    assert torch.equal(hf["cls.predictions.decoder.weight"], sd["bert.embeddings.word_embeddings.weight"])
    back = bert.from_hf_state_dict(hf, L)
    assert set(back) == set(sd)
    assert all(torch.equal(back[k], sd[k]) for k in sd)
    m.load_state_dict(back)
    # an untied decoder cannot be represented: refused on import
    hf["cls.predictions.decoder.weight"] = hf["cls.predictions.decoder.weight"] + 1
    with pytest.raises(ValueError):
        bert.from_hf_state_dict(hf, L)
    # the classification model's mapping is what it was: no head keys appear
    c = bert_tiny()
    csd = c.state_dict()
    chf = bert.to_hf_state_dict(csd, 2)
    assert not any(k.startswith("cls.") for k in chf)
    cback = bert.from_hf_state_dict(chf, 2)
    assert set(cback) == set(csd) and all(torch.equal(cback[k], csd[k]) for k in csd)


def test_pretraining_base_parameter_count():
    from databricks_distributed_deep_learning_amd.models import build_model, count_params
    with torch.device("meta"):
        m = build_model("bert_base_pretraining")
    assert count_params(m) == 110_106_428


# ------------------------------------------------------------------ data, preset, notebook
def test_synthetic_tokens_mlm_targets():
    from databricks_distributed_deep_learning_amd.data import SyntheticTokens
    B, S, P, V = 5, 40, 9, 300
    ld = SyntheticTokens(B, S, V, pool=3, pad_fraction=0.5, mlm_predictions=P)
    for _ in range(3):
        b = ld.next()
        pos, lab, nsp = b["masked_lm_positions"], b["masked_lm_labels"], b["next_sentence_label"]
        assert pos.shape == lab.shape == (B, P) and nsp.shape == (B,)
        lens = b["attention_mask"].sum(1)
        valid = lab != -100
        assert valid.any(dim=1).all()                              # a target in every row
        assert ((lab[valid] >= 0) & (lab[valid] < V)).all()
        assert ((pos >= 0) & (pos < lens[:, None])).all()            # inside the unpadded length
        for r in range(B):
            pv = pos[r][valid[r]]
            assert pv.unique().numel() == pv.numel()
            k = int(valid[r].sum())
            assert valid[r, :k].all() and not valid[r, k:].any()      # padding is trailing
        assert ((nsp == 0) | (nsp == 1)).all()
    plain = SyntheticTokens(B, S, V, pool=2, pad_fraction=0.5)
    zero = SyntheticTokens(B, S, V, pool=2, pad_fraction=0.5, mlm_predictions=0)
    for _ in range(2):
        a, z = plain.next(), zero.next()
        assert set(a) == set(z) == {"input_ids", "attention_mask", "labels"}
        assert all(torch.equal(a[k], z[k]) for k in a)


def test_pretrain_preset_smoke_step():
    from databricks_distributed_deep_learning_amd.config import get_preset
    from databricks_distributed_deep_learning_amd.training.loop import Trainer
    full = get_preset("bert_large_pretrain")
    lamb = get_preset("bert_large_lamb")
    assert (full.model, full.seq_len, full.mlm_predictions) == ("bert_large_pretraining", 512, 76)
    assert full.resolved_optimizer == "lamb" and full.resolved_task == "nlp"
    same = {k: v for k, v in full.to_dict().items() if k not in ("model", "mlm_predictions")}
    assert same == {k: v for k, v in lamb.to_dict().items() if k not in ("model", "mlm_predictions")}
    cfg = get_preset("bert_large_pretrain", model="bert_tiny_pretraining", batch_size=2, seq_len=16,
                     mlm_predictions=4, vocab_size=1024, steps=1, warmup_steps=0, grad_accum=2, dtype="fp32",
                     backend="gloo", native="off", log_every=0, optimizer="lamb")
    t = Trainer(cfg)
    loss = t.train_step()
    assert torch.isfinite(loss).all()


def test_pretraining_notebook_smoke():
    nb = os.path.join(ROOT, "notebooks/nlp/bert_pretraining.py")
    src = open(nb).read()
    assert src.startswith("# Databricks notebook source") and "# COMMAND ----------" in src
    env = dict(os.environ, DDL_NOTEBOOK_SMOKE="1", PYTHONPATH=ROOT, CUDA_VISIBLE_DEVICES="")
    for k in ("MASTER_PORT", "RANK", "WORLD_SIZE", "LOCAL_RANK", "LOCAL_WORLD_SIZE"):
        env.pop(k, None)            # a process group of this process must not name the child's port
    r = subprocess.run([sys.executable, nb], env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "'final_loss': " in r.stdout and "nan" not in r.stdout.lower()
