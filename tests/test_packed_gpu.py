"""Packed rows through the whole model on the HIP kernels (GPU only): ``llama_tiny`` and GPT-2 tiny in
bf16, S = 193 with three documents per row (starts 70 / 129 and 64 / 150: mid-tile, one past a tile edge and
on one), loss and parameter gradients of the native path against the reference ops (``native=off``) on the
same packed batch.

Bound: M = 2 times the error of the UNPACKED native forward and backward against its own reference on the
same ids -- the code path as it was before ``position_ids`` existed -- measured in the same test.  Both
errors are taken as the largest over four seeded batches (a single scalar loss difference is one draw of a
random sign-and-size), the gradient error as the relative L2 distance over all parameters.

Measured on an MI355X, packed error / unpacked error: llama_tiny loss 0.89 (6.7e-5 / 7.5e-5), gradients 0.97
(6.6e-3 / 6.8e-3); GPT-2 tiny loss 0.98 (1.10e-4 / 1.13e-4), gradients 1.02 (6.0e-3 / 5.9e-3).
"""
import pytest
import torch

from conftest import gpu_device

pytestmark = pytest.mark.gpu

M = 2.0
B, S = 2, 193
STARTS = [[0, 70, 129], [0, 64, 150]]
SEEDS = [1, 2, 3, 4]


def _model(kind, dev):
    from databricks_distributed_deep_learning_amd.models import cast_params, gpt2_tiny, llama_tiny
    torch.manual_seed(0)
    m = llama_tiny() if kind == "llama" else gpt2_tiny(dropout=0.0, n_positions=256)
    m = m.to(dev)
    cast_params(m, torch.bfloat16)
    return m.train()


def _batch(seed, dev):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(0, 1000, (B, S), generator=g)
    plain = torch.full_like(ids, -100)
    plain[:, :-1] = ids[:, 1:]
    packed = plain.clone()
    pos = torch.empty(B, S, dtype=torch.long)
    for b, st in enumerate(STARTS):
        first = torch.zeros(S, dtype=torch.long)
        for s in st:
            first[s:] = s
            if s:
                packed[b, s - 1] = -100
        pos[b] = torch.arange(S) - first
    return ids.to(dev), plain.to(dev), packed.to(dev), pos.to(dev)


def _loss_and_grads(model, mode, ids, labels, pos, last_hidden=None):
    from databricks_distributed_deep_learning_amd import ops
    ops.set_native_mode(mode)
    model.zero_grad(set_to_none=True)
    handle = None
    if last_hidden is not None:
        final = model.norm if hasattr(model, "norm") else model.ln_f

        def keep(_, __, out):
            out.retain_grad()
            last_hidden.append(out)
        handle = final.register_forward_hook(keep)
    if pos is None:
        loss, _ = model(ids, None, None, labels)
    else:
        loss, _ = model(ids, None, None, labels, position_ids=pos)
    loss.backward()
    torch.cuda.synchronize()
    if handle is not None:
        handle.remove()
    return loss.detach().double(), [p.grad.detach().double() for p in model.parameters()]


def _errors(model, ids, labels, pos):
    ln, gn = _loss_and_grads(model, "auto", ids, labels, pos)
    lr, gr = _loss_and_grads(model, "off", ids, labels, pos)
    num = sum((a - b).pow(2).sum() for a, b in zip(gn, gr)).sqrt().item()
    den = sum(b.pow(2).sum() for b in gr).sqrt().item()
    return abs((ln - lr).item()), num / den


@pytest.mark.parametrize("kind", ["llama", "gpt2"])
def test_packed_model_native_against_reference(kind):
    dev = gpu_device()
    model = _model(kind, dev)
    plain_err, packed_err = [], []
    for seed in SEEDS:
        ids, plain, packed, pos = _batch(seed, dev)
        plain_err.append(_errors(model, ids, plain, None))          # the yardstick: the unpacked path
        packed_err.append(_errors(model, ids, packed, pos))
    yl, yg = max(e[0] for e in plain_err), max(e[1] for e in plain_err)
    pl, pg = max(e[0] for e in packed_err), max(e[1] for e in packed_err)
    print(f"PACKED {kind}: loss error packed {pl:.3e} unpacked {yl:.3e} ratio {pl / yl:.3f}; "
          f"gradient error packed {pg:.3e} unpacked {yg:.3e} ratio {pg / yg:.3f}")
    assert yl > 0 and yg > 0
    assert pl <= M * yl, f"loss error {pl:.3e} > {M} * {yl:.3e}"
    assert pg <= M * yg, f"gradient error {pg:.3e} > {M} * {yg:.3e}"


@pytest.mark.parametrize("kind", ["llama", "gpt2"])
def test_paths_agree_on_the_tokens_that_carry_loss(kind):
    """The gradient that reaches the final norm's output is zero exactly at the tokens whose label is -100 --
    every document's last token -- and nowhere else, on the native path and with native=off alike."""
    dev = gpu_device()
    model = _model(kind, dev)
    ids, _, packed, pos = _batch(SEEDS[0], dev)
    want = packed != -100
    assert int((~want).sum()) == B * len(STARTS[0])
    for mode in ("auto", "off"):
        hs = []
        _loss_and_grads(model, mode, ids, packed, pos, last_hidden=hs)
        got = hs[0].grad.float().abs().sum(-1).reshape(B, S) != 0
        assert torch.equal(got, want), mode
