"""The Llama-family model on the CPU: HF parity and checkpoint conversion over the grouped-query head
configurations, the factories' parameter counts, the preset and a short training run."""
import math

import pytest
import torch

from databricks_distributed_deep_learning_amd.models import llama as ML


def _hf_config(transformers, heads, kv, tied, **kw):
    d = dict(vocab_size=100, hidden_size=128, intermediate_size=352, num_hidden_layers=2,
             num_attention_heads=heads, num_key_value_heads=kv, max_position_embeddings=64, rms_norm_eps=1e-5,
             rope_theta=10000.0, tie_word_embeddings=tied, attention_bias=False, mlp_bias=False)
    d.update(kw)
    return transformers.LlamaConfig(**d)


# ------------------------------------------------------------------ HF parity
@pytest.mark.parametrize("tied", [True, False], ids=["tied", "untied"])
@pytest.mark.parametrize("heads,kv", [(2, 2), (2, 1), (4, 2)])
def test_llama_matches_hf_random_init(heads, kv, tied):
    transformers = pytest.importorskip("transformers")
    hc = _hf_config(transformers, heads, kv, tied)
    torch.manual_seed(0)
    hf = transformers.LlamaForCausalLM(hc).eval()
    with torch.no_grad():       # norm weights away from their all-ones init: a swapped pair would show
        for n, p in hf.named_parameters():
            if n.endswith("norm.weight"):
                p.copy_(torch.rand_like(p) + 0.5)
    c = ML.config_from_hf(hc)
    assert (c.num_attention_heads, c.num_key_value_heads, c.tie_word_embeddings) == (heads, kv, tied)
    ours = ML.LlamaForCausalLM(c).eval()
    sd = hf.state_dict()
    missing, unexpected = ours.load_state_dict(ML.from_hf_state_dict(sd, c, hc), strict=False)
    assert not missing and not unexpected, (missing, unexpected)
    assert "rope_table" not in ours.state_dict()            # a non-persistent buffer
    assert (ours.lm_head is None) == tied
    ids = torch.randint(0, 100, (2, 11))
    mask = torch.ones(2, 11, dtype=torch.long)
    mask[1, 8:] = 0                                          # right-padded
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
    # the round trip is exact
    back = ML.to_hf_state_dict(ML.from_hf_state_dict(sd, c), c)
    assert set(back) == set(sd)
    for k, v in back.items():
        assert torch.equal(v, sd[k]), k
    again = ML.from_hf_state_dict(ML.to_hf_state_dict(ours.state_dict(), c), c)
    assert set(again) == set(ours.state_dict())
    for k, v in ours.state_dict().items():
        assert torch.equal(again[k], v), k


def test_llama_conversion_errors():
    c = ML.LlamaConfig(vocab_size=50, hidden_size=64, intermediate_size=96, num_hidden_layers=1,
                       num_attention_heads=1, num_key_value_heads=1, max_position_embeddings=16)
    torch.manual_seed(1)
    sd = ML.to_hf_state_dict(ML.LlamaForCausalLM(c).state_dict(), c)
    assert set(ML.from_hf_state_dict(sd, c)) == set(ML.LlamaForCausalLM(c).state_dict())
    base = dict(hidden_size=64, num_attention_heads=1, rope_scaling=None, attention_bias=False, mlp_bias=False)
    ML.check_hf_config(base)
    ML.check_hf_config(dict(base, rope_scaling={"rope_type": "default", "rope_theta": 1e4}))
    with pytest.raises(ValueError, match="rope_scaling"):
        ML.from_hf_state_dict(sd, c, dict(base, rope_scaling={"rope_type": "llama3", "factor": 32.0}))
    with pytest.raises(ValueError, match="rope_scaling"):
        ML.check_hf_config(dict(base, rope_scaling={"type": "linear", "factor": 2.0}))
    with pytest.raises(ValueError, match="bias"):
        ML.from_hf_state_dict(sd, c, dict(base, attention_bias=True))
    with pytest.raises(ValueError, match="bias"):
        ML.from_hf_state_dict(sd, c, dict(base, mlp_bias=True))
    with pytest.raises(ValueError, match="bias"):       # the tensors say so even where no config does
        ML.from_hf_state_dict(dict(sd, **{"model.layers.0.self_attn.q_proj.bias": torch.zeros(64)}), c)
    # tied flag against the tensors
    other = dict(sd, **{"lm_head.weight": sd["lm_head.weight"] + 1})
    with pytest.raises(ValueError, match="tie_word_embeddings"):
        ML.from_hf_state_dict(other, c)
    untied = ML.LlamaConfig(**{**c.__dict__, "tie_word_embeddings": False})
    assert torch.equal(ML.from_hf_state_dict(other, untied)["lm_head.weight"], other["lm_head.weight"])
    headless = {k: v for k, v in sd.items() if k != "lm_head.weight"}
    with pytest.raises(ValueError, match="tie_word_embeddings"):
        ML.from_hf_state_dict(headless, untied)
    assert "lm_head.weight" not in ML.from_hf_state_dict(headless, c)      # tied: the head is the embedding


# ------------------------------------------------------------------ factories
_FACTORIES = {"llama_tiny": (128, 2, 2, 1, 352, 1000, 256), "smollm_135m": (576, 30, 9, 3, 1536, 49152, 2048),
              "smollm_360m": (960, 32, 15, 5, 2560, 49152, 2048), "smollm_1p7b": (2048, 24, 32, 32, 8192, 49152, 2048)}


@pytest.mark.parametrize("name", sorted(_FACTORIES))
def test_llama_factories(name):
    from databricks_distributed_deep_learning_amd.models import available_models, build_model, count_params
    assert name in available_models()
    with torch.device("meta"):
        m = build_model(name, dropout=0.3)           # ignored: the family has no dropout
    c = m.config
    E, L, H, Hkv, I, V, P = _FACTORIES[name]
    assert (c.hidden_size, c.num_hidden_layers, c.num_attention_heads, c.num_key_value_heads, c.intermediate_size,
            c.vocab_size, c.max_position_embeddings) == _FACTORIES[name]
    assert c.tie_word_embeddings and c.rope_theta == 1e4 and c.rms_norm_eps == 1e-5 and E // H == 64
    n = count_params(m)
    # embedding + per layer (qkv, o, gate_up, down, two norms) + final norm
    assert n == V * E + L * (E * (H + 2 * Hkv) * 64 + H * 64 * E + 3 * E * I + 2 * E) + E
    if name == "smollm_135m":
        assert n == 134_515_008
    assert not any(k.startswith("lm_head") for k, _ in m.named_parameters())
    assert not any(k.endswith(".bias") for k, _ in m.named_parameters())
    transformers = pytest.importorskip("transformers")
    hc = _hf_config(transformers, H, Hkv, True, vocab_size=V, hidden_size=E, intermediate_size=I,
                    num_hidden_layers=L, max_position_embeddings=P)
    with torch.device("meta"):
        hf = transformers.LlamaForCausalLM(hc)
    assert n == sum(p.numel() for p in hf.parameters())


def test_llama_tiny_forward_shapes_and_untied_head():
    from databricks_distributed_deep_learning_amd.models import llama_tiny
    t = llama_tiny().eval()
    ids = torch.randint(0, 1000, (2, 9))
    assert t(ids).shape == (2, 9, 1000)
    with pytest.raises(ValueError, match="max_position_embeddings"):
        t(torch.zeros(1, 257, dtype=torch.long))
    u = llama_tiny(tie_word_embeddings=False)
    assert u.lm_head is not None and u.lm_head.bias is None and u.lm_head.weight.shape == (1000, 128)
    # a head dimension other than 64 runs (through the reference ops)
    o = llama_tiny(hidden_size=64, num_attention_heads=4, num_key_value_heads=2).eval()
    assert o.rope_table.shape == (256, 16) and o(ids).shape == (2, 9, 1000)
    # a cast to bf16 leaves the rotary table in fp32
    assert llama_tiny().bfloat16().rope_table.dtype == torch.float32


# ------------------------------------------------------------------ preset, training
def test_llama_pretrain_preset():
    from databricks_distributed_deep_learning_amd.config import get_preset
    c = get_preset("llama_pretrain")
    assert c.resolved_task == "nlp" and c.resolved_optimizer == "adamw"
    assert (c.model, c.seq_len, c.batch_size, c.dtype, c.optimizer, c.vocab_size) == \
        ("smollm_135m", 2048, 8, "bf16", "adamw", 49152)
    for name in ("llama_tiny", "smollm_360m"):
        r = c.replace(model=name, optimizer="auto")
        assert r.resolved_task == "nlp" and r.resolved_optimizer == "adamw"


def test_llama_tiny_trains_on_cpu():
    from databricks_distributed_deep_learning_amd.config import get_preset
    from databricks_distributed_deep_learning_amd.training.loop import Trainer
    cfg = get_preset("llama_pretrain", model="llama_tiny", batch_size=4, seq_len=32, steps=6, warmup_steps=0,
                     dtype="fp32", backend="gloo", native="off", log_every=1, lr=3e-3, synthetic_pool=1,
                     pad_fraction=0.25)
    t = Trainer(cfg)
    assert t.task == "nlp" and t.loader.pool[0]["labels"].shape == (4, 32)
    b = t.loader.pool[0]                                  # causal-LM labels: the next token
    nxt = b["attention_mask"][:, 1:].bool()
    assert torch.equal(b["labels"][:, :-1][nxt], b["input_ids"][:, 1:][nxt])
    losses = []
    out = t.run(callback=lambda step, loss: losses.append(loss))
    t.close()
    assert out["steps"] == 6 and math.isfinite(out["final_loss"])
    assert len(losses) == 6 and losses[-1] < losses[0], losses
