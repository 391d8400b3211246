"""The Llama-family model on the GPU: the native bf16 ``llama_tiny`` (two query heads over one key / value
head; RMSNorm, RoPE + GQA pack and SwiGLU kernels, causal attention, fused vocabulary head on the tied
embedding, bridged blocks) against the same weights run through the reference ops in fp32 on the CPU, with
and without padding, and one repeatable native training step.

Tolerance: ``tests/test_gpt2_gpu.py``'s band -- per parameter the native error against fp32 stays within
``2.0 * e_t16 + 0.05`` of stock bf16's, the mean within ``1.25 * mean_t16 + 0.02``, the loss within
``3 * |t16 - ref| + 5e-2 * max(1, |ref|)``; stock bf16 is the same model through the reference ops on the GPU.
"""
import copy

import pytest
import torch

from conftest import gpu_device
from test_models_gpu import _grads, _rel

pytestmark = pytest.mark.gpu


def _tiny():
    from databricks_distributed_deep_learning_amd.models import llama_tiny
    torch.manual_seed(0)
    m = llama_tiny().train()                 # hidden 128, 2 heads over 1 KV head: head dim 64, G = 2
    with torch.no_grad():                    # norm weights away from their all-ones init
        for n, p in m.named_parameters():
            if n.endswith("norm.weight"):
                p.copy_(torch.rand_like(p) + 0.5)
    return m


def _batch(S, padded):
    g = torch.Generator().manual_seed(S)
    ids = torch.randint(0, 1000, (2, S), generator=g)
    mask = None
    labels = torch.full_like(ids, -100)
    labels[:, :-1] = ids[:, 1:]
    if padded:      # ragged lengths; labels are -100 wherever the next position is padding
        lens = torch.tensor([S, S - 37])
        mask = (torch.arange(S)[None, :] < lens[:, None]).long()
        labels[:, :-1] = ids[:, 1:].masked_fill(mask[:, 1:] == 0, -100)
    return ids, mask, labels


def _cpu_fp32(model, ids, mask, labels):
    m = copy.deepcopy(model).float()
    loss, _ = m(ids, mask, None, labels)
    loss.backward()
    return loss.detach().float(), {n: p.grad.detach().float() for n, p in m.named_parameters()}


@pytest.mark.parametrize("padded", [False, True])
@pytest.mark.parametrize("S", [96, 200])
def test_llama_native_vs_cpu_fp32(S, padded, monkeypatch):
    dev = gpu_device()
    from databricks_distributed_deep_learning_amd.models.layers import cast_params
    from databricks_distributed_deep_learning_amd.ops import _native_llama as NL
    model = _tiny()
    ids, mask, labels = _batch(S, padded)
    ref_loss, ref = _cpu_fp32(model, ids, mask, labels)
    d_ids, d_mask, d_labels = ids.to(dev), None if mask is None else mask.to(dev), labels.to(dev)
    # the native arm must run the new kernels, the stock arm must not
    calls = {"rms": 0, "rope": 0, "swiglu": 0}
    for key, name in (("rms", "rms_norm"), ("rope", "rope_qkv"), ("swiglu", "swiglu")):
        def counted(*a, _f=getattr(NL, name), _k=key, **k):
            calls[_k] += 1
            return _f(*a, **k)
        monkeypatch.setattr(NL, name, counted)

    def run(mod):
        loss, none = mod(d_ids, d_mask, None, d_labels)
        assert none is None
        return loss.float()

    t_loss, t16 = _grads(cast_params(copy.deepcopy(model), torch.bfloat16).to(dev), run, "off")
    assert calls == {"rms": 0, "rope": 0, "swiglu": 0}
    loss, got = _grads(cast_params(copy.deepcopy(model), torch.bfloat16).to(dev), run, "auto")
    assert calls == {"rms": 5, "rope": 2, "swiglu": 2}       # 2 layers x 2 norms + the final norm
    ref_loss, t_loss, loss = ref_loss.item(), t_loss.item(), loss.item()
    print(f"LLAMA S={S} padded={padded} loss native={loss:.5f} stock-bf16={t_loss:.5f} cpu-fp32={ref_loss:.5f}")
    assert abs(loss - ref_loss) <= 3 * abs(t_loss - ref_loss) + 5e-2 * max(1.0, abs(ref_loss))
    assert set(got) == set(ref) == set(t16)         # the tied embedding included, once
    for n, gr in got.items():
        assert torch.isfinite(gr).all(), f"{n}: non-finite gradient"
    e_nat = {n: _rel(got[n].cpu(), ref[n]) for n in ref}
    e_t16 = {n: _rel(t16[n].cpu(), ref[n]) for n in ref}
    print("LLAMA worst native/stock:", max((e_nat[n], e_t16[n], n) for n in ref))
    bad = {n: (round(e_nat[n], 3), round(e_t16[n], 3)) for n in ref if e_nat[n] > 2.0 * e_t16[n] + 0.05}
    assert not bad, bad
    mean_nat, mean_t16 = sum(e_nat.values()) / len(e_nat), sum(e_t16.values()) / len(e_t16)
    assert mean_nat <= 1.25 * mean_t16 + 0.02, (mean_nat, mean_t16)
    # the tied table's gradient has both shares: the head's (every row) and the embedding's
    assert got["embed_tokens.weight"].abs().sum(1).count_nonzero().item() == 1000


def test_llama_all_ignored_row_has_finite_gradients():
    """a sequence whose labels are all -100 (and whose tail is padding) contributes no NaN"""
    dev = gpu_device()
    from databricks_distributed_deep_learning_amd.models.layers import cast_params
    m = cast_params(_tiny(), torch.bfloat16).to(dev)
    assert m.rope_table.dtype == torch.float32 and m.rope_table.is_cuda
    ids, mask, labels = _batch(96, True)
    labels[1] = -100
    loss, _ = m(ids.to(dev), mask.to(dev), None, labels.to(dev))
    loss.backward()
    assert torch.isfinite(loss)
    for n, p in m.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), n


def test_llama_tiny_native_train_step_repeatable(monkeypatch):
    gpu_device()
    from databricks_distributed_deep_learning_amd.config import get_preset
    from databricks_distributed_deep_learning_amd.ops import _native_gemm
    from databricks_distributed_deep_learning_amd.training.loop import Trainer
    # both runs take the committed / default kernel plans (no in-model tuning on rotating candidates)
    monkeypatch.setattr(_native_gemm, "_ONLINE_ENV", "0")
    runs = []
    for _ in range(2):
        t = Trainer(get_preset("llama_pretrain", model="llama_tiny", batch_size=2, seq_len=128, steps=1,
                               warmup_steps=0, log_every=0, pad_fraction=0.25))
        assert t.cfg.resolved_optimizer == "adamw" and t.task == "nlp"
        out = t.run()
        torch.cuda.synchronize()
        runs.append((torch.tensor(out["final_loss"]), t.arena.flat.float().clone()))
        del t
    assert torch.isfinite(runs[0][0]).all()
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
