"""GPT-2 on the GPU: the native bf16 model (causal attention kernels, fused vocabulary head on the tied
embedding, bridged pre-LN blocks) against the same weights run through the reference ops in fp32 on the
CPU, with and without padding, and one repeatable native training step.

Tolerance: the band of tests/test_models_gpu.py's BERT / ViT comparison (`_compare`): per parameter the
native error against fp32 stays within `2.0 * e_t16 + 0.05` of stock bf16's (its line 58), the mean
within `1.25 * mean_t16 + 0.02` (line 62), the loss within `3 * |t16 - ref| + 5e-2 * max(1, |ref|)`
(lines 50-51); stock bf16 is the same model through the reference ops on the GPU.
"""
import copy

import pytest
import torch

from conftest import gpu_device
from test_models_gpu import _grads, _rel

pytestmark = pytest.mark.gpu


def _tiny():
    from databricks_distributed_deep_learning_amd.models import gpt2_tiny
    torch.manual_seed(0)
    return gpt2_tiny(dropout=0.0, n_positions=256).train()      # hidden 128, 2 heads: head dim 64


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
def test_gpt2_native_vs_cpu_fp32(S, padded):
    dev = gpu_device()
    from databricks_distributed_deep_learning_amd.models.layers import cast_params
    model = _tiny()
    ids, mask, labels = _batch(S, padded)
    ref_loss, ref = _cpu_fp32(model, ids, mask, labels)
    d_ids, d_mask, d_labels = ids.to(dev), None if mask is None else mask.to(dev), labels.to(dev)

    def run(mod):
        loss, none = mod(d_ids, d_mask, None, d_labels)
        assert none is None
        return loss.float()

    t_loss, t16 = _grads(cast_params(copy.deepcopy(model), torch.bfloat16).to(dev), run, "off")
    loss, got = _grads(cast_params(copy.deepcopy(model), torch.bfloat16).to(dev), run, "auto")
    ref_loss, t_loss, loss = ref_loss.item(), t_loss.item(), loss.item()
    print(f"GPT2 S={S} padded={padded} loss native={loss:.5f} stock-bf16={t_loss:.5f} cpu-fp32={ref_loss:.5f}")
    assert abs(loss - ref_loss) <= 3 * abs(t_loss - ref_loss) + 5e-2 * max(1.0, abs(ref_loss))
    assert set(got) == set(ref) == set(t16)         # the tied embedding included, once
    for n, gr in got.items():
        assert torch.isfinite(gr).all(), f"{n}: non-finite gradient"
    e_nat = {n: _rel(got[n].cpu(), ref[n]) for n in ref}
    e_t16 = {n: _rel(t16[n].cpu(), ref[n]) for n in ref}
    print("GPT2 worst native/stock:", max((e_nat[n], e_t16[n], n) for n in ref))
    bad = {n: (round(e_nat[n], 3), round(e_t16[n], 3)) for n in ref if e_nat[n] > 2.0 * e_t16[n] + 0.05}
    assert not bad, bad
    mean_nat, mean_t16 = sum(e_nat.values()) / len(e_nat), sum(e_t16.values()) / len(e_t16)
    assert mean_nat <= 1.25 * mean_t16 + 0.02, (mean_nat, mean_t16)
    # the tied table's gradient has both shares: the head's (every row) and the embedding's
    assert got["wte.weight"].abs().sum(1).count_nonzero().item() == 1000


def test_gpt2_all_ignored_row_has_finite_gradients():
    """a sequence whose labels are all -100 (and whose tail is padding) contributes no NaN"""
    dev = gpu_device()
    from databricks_distributed_deep_learning_amd.models.layers import cast_params
    m = cast_params(_tiny(), torch.bfloat16).to(dev)
    ids, mask, labels = _batch(96, True)
    labels[1] = -100
    loss, _ = m(ids.to(dev), mask.to(dev), None, labels.to(dev))
    loss.backward()
    assert torch.isfinite(loss)
    for n, p in m.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), n


def test_gpt2_tiny_native_train_step_repeatable(monkeypatch):
    gpu_device()
    from databricks_distributed_deep_learning_amd.config import get_preset
    from databricks_distributed_deep_learning_amd.ops import _native_gemm
    from databricks_distributed_deep_learning_amd.training.loop import Trainer
    # both runs take the committed / default kernel plans (no in-model tuning on rotating candidates)
    monkeypatch.setattr(_native_gemm, "_ONLINE_ENV", "0")
    runs = []
    for _ in range(2):
        t = Trainer(get_preset("gpt2_pretrain", model="gpt2_tiny", batch_size=2, seq_len=128, steps=1,
                               warmup_steps=0, log_every=0, pad_fraction=0.25))
        assert t.cfg.resolved_optimizer == "adamw"
        out = t.run()
        torch.cuda.synchronize()
        runs.append((torch.tensor(out["final_loss"]), t.arena.flat.float().clone()))
        del t
    assert torch.isfinite(runs[0][0]).all()
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
