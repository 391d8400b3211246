"""GPT-2 causal LM on the CPU: the causal attention reference, HF parity and checkpoint conversion,
the shifted next-token labels of the synthetic loader, the preset and a short training run."""
import math

import pytest
import torch

from databricks_distributed_deep_learning_amd import ops
from databricks_distributed_deep_learning_amd.ops.attention import attention_reference


# ------------------------------------------------------------------ causal reference
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("S", [1, 5, 64, 65])
def test_attention_reference_causal_matches_fp64_triangular_softmax(S, masked):
    B, H, D = 2, 2, 16
    g = torch.Generator().manual_seed(S)
    qkv = torch.randn(B, S, 3 * H * D, generator=g)
    mask = None
    if masked:      # hide the last keys of row 1 (key 0 stays: every query keeps one visible key)
        mask = torch.zeros(B, S)
        mask[1, max(1, S // 2):] = -10000.0
    got = attention_reference(qkv, H, mask, causal=True)
    q, k, v = qkv.double().view(B, S, 3, H, D).permute(2, 0, 3, 1, 4).unbind(0)
    s = q @ k.transpose(-1, -2) / math.sqrt(D)
    if mask is not None:
        s = s + mask.double().view(B, 1, 1, S)
    ar = torch.arange(S)
    s = s.masked_fill(ar[None, :] > ar[:, None], -math.inf)
    want = (torch.softmax(s, -1) @ v).permute(0, 2, 1, 3).reshape(B, S, H * D)
    torch.testing.assert_close(got.double(), want, atol=1e-5, rtol=1e-5)
    # the public op takes the keyword and routes CPU tensors to the reference
    assert torch.equal(ops.attention(qkv, H, mask, causal=True), got)
    if S > 1:   # and the mask is not a no-op
        assert not torch.allclose(got, attention_reference(qkv, H, mask), atol=1e-3)


# ------------------------------------------------------------------ HF parity
@pytest.mark.parametrize("act", ["gelu", "gelu_new"])
def test_gpt2_matches_hf_random_init(act):
    transformers = pytest.importorskip("transformers")
    from databricks_distributed_deep_learning_amd.models.gpt2 import GPT2Config, GPT2LMHeadModel, \
        from_hf_state_dict, to_hf_state_dict
    hc = transformers.GPT2Config(vocab_size=100, n_positions=32, n_embd=64, n_layer=2, n_head=4,
                                 resid_pdrop=0.0, embd_pdrop=0.0, attn_pdrop=0.0, activation_function=act)
    torch.manual_seed(0)
    hf = transformers.GPT2LMHeadModel(hc).eval()
    ours = GPT2LMHeadModel(GPT2Config(vocab_size=100, n_positions=32, n_embd=64, n_layer=2, n_head=4,
                                      resid_pdrop=0.0, embd_pdrop=0.0, attn_pdrop=0.0,
                                      activation_function=act)).eval()
    sd = hf.state_dict()
    missing, unexpected = ours.load_state_dict(from_hf_state_dict(sd, 2), strict=False)
    assert not missing and not unexpected, (missing, unexpected)
    ids = torch.randint(0, 100, (2, 11))
    mask = torch.ones(2, 11, dtype=torch.long)
    mask[1, 8:] = 0
    # our labels are already shifted (labels[b, s] = token s + 1); HF shifts its own
    hf_labels = ids.masked_fill(mask == 0, -100)
    labels = torch.full_like(ids, -100)
    labels[:, :-1] = hf_labels[:, 1:]
    with torch.no_grad():
        ref = hf(input_ids=ids, attention_mask=mask, labels=hf_labels)
        got = ours(ids, mask)
        loss, none = ours(ids, mask, None, labels)
    assert none is None
    keep = mask.bool()      # HF's rows at padded positions attend differently (-inf vs -10000): not compared
    torch.testing.assert_close(got[keep], ref.logits[keep], atol=1e-4, rtol=1e-4)
    torch.testing.assert_close(loss, ref.loss, atol=1e-4, rtol=1e-4)
    back = to_hf_state_dict(from_hf_state_dict(sd, 2), 2)
    mine = {k: v for k, v in sd.items() if not k.endswith((".attn.bias", ".attn.masked_bias"))}
    assert set(back) == set(mine)
    for k, v in back.items():
        assert torch.equal(v, mine[k]), k


def test_gpt2_factories_and_tied_head():
    from databricks_distributed_deep_learning_amd.models import build_model, count_params
    with torch.device("meta"):
        m = build_model("gpt2")
    assert count_params(m) == 124_439_808       # HF GPT2LMHeadModel (gpt2), tied head counted once
    c = m.config
    assert (c.vocab_size, c.n_positions, c.n_embd, c.n_layer, c.n_head) == (50257, 1024, 768, 12, 12)
    assert c.layer_norm_epsilon == 1e-5 and c.initializer_range == 0.02 and c.activation_function == "gelu"
    with torch.device("meta"):
        for name, want in (("gpt2_medium", (1024, 24, 16)), ("gpt2_large", (1280, 36, 20))):
            cc = build_model(name).config
            assert (cc.n_embd, cc.n_layer, cc.n_head) == want and cc.n_embd // cc.n_head == 64
    t = build_model("gpt2_tiny", dropout=0.0)
    tc = t.config
    assert (tc.n_layer, tc.n_embd, tc.n_head, tc.vocab_size, tc.n_positions) == (2, 128, 2, 1000, 128)
    assert not any(n.startswith("lm_head") for n, _ in t.named_parameters())
    ids = torch.randint(0, 1000, (2, 9))
    assert t.eval()(ids).shape == (2, 9, 1000)


# ------------------------------------------------------------------ data, preset, training
def test_synthetic_tokens_causal_lm_labels():
    from databricks_distributed_deep_learning_amd.data import SyntheticTokens
    B, S, V = 6, 40, 300
    ld = SyntheticTokens(B, S, V, pool=3, pad_fraction=0.5, causal_lm=True)
    from_padding = 0
    for b in ld.pool:
        ids, mask, lab = b["input_ids"], b["attention_mask"], b["labels"]
        assert lab.shape == (B, S) and lab.dtype == ids.dtype
        assert (lab[:, -1] == -100).all()
        nxt = mask[:, 1:].bool()
        assert torch.equal(lab[:, :-1][nxt], ids[:, 1:][nxt])
        assert (lab[:, :-1][~nxt] == -100).all()
        from_padding += int((~nxt).sum())
    assert from_padding > 0
    full = SyntheticTokens(B, S, V, pool=2, causal_lm=True)
    for b in full.pool:
        assert b["attention_mask"] is None
        assert torch.equal(b["labels"][:, :-1], b["input_ids"][:, 1:]) and (b["labels"][:, -1] == -100).all()
    # the flag draws nothing: ids and masks are those of a loader without it, and False changes nothing
    for pf in (0.0, 0.5):
        plain = SyntheticTokens(B, S, V, pool=3, pad_fraction=pf)
        off = SyntheticTokens(B, S, V, pool=3, pad_fraction=pf, causal_lm=False)
        on = SyntheticTokens(B, S, V, pool=3, pad_fraction=pf, causal_lm=True)
        for a, z, c in zip(plain.pool, off.pool, on.pool):
            assert set(a) == set(z)
            for k in a:
                assert (a[k] is None and z[k] is None) or torch.equal(a[k], z[k])
            assert torch.equal(a["input_ids"], c["input_ids"])
            assert (a["attention_mask"] is None and c["attention_mask"] is None) or \
                torch.equal(a["attention_mask"], c["attention_mask"])


def test_gpt2_pretrain_preset():
    from databricks_distributed_deep_learning_amd.config import get_preset
    c = get_preset("gpt2_pretrain")
    assert c.resolved_task == "nlp" and c.resolved_optimizer == "adamw"
    assert (c.model, c.seq_len, c.dtype, c.dropout, c.batch_size) == ("gpt2", 1024, "bf16", 0.1, 16)
    assert c.replace(optimizer="auto").resolved_optimizer == "adamw"


def test_gpt2_tiny_trains_on_cpu():
    from databricks_distributed_deep_learning_amd.config import get_preset
    from databricks_distributed_deep_learning_amd.training.loop import Trainer
    cfg = get_preset("gpt2_pretrain", model="gpt2_tiny", batch_size=4, seq_len=32, steps=6, warmup_steps=0,
                     dtype="fp32", backend="gloo", native="off", log_every=1, lr=3e-3, dropout=0.0,
                     synthetic_pool=1, pad_fraction=0.25)
    t = Trainer(cfg)
    assert t.task == "nlp" and t.loader.pool[0]["labels"].shape == (4, 32)
    losses = []
    out = t.run(callback=lambda step, loss: losses.append(loss))
    t.close()
    assert out["steps"] == 6 and math.isfinite(out["final_loss"])
    assert len(losses) == 6 and losses[-1] < losses[0], losses
