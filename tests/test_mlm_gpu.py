"""BERT masked-LM pretraining on the GPU: the loss / gather kernels of csrc/kernels/mlm_loss.hip, the
fused vocabulary head, the pretraining model against the stock path, and the tied decoder weight
under the gradient reducer."""
import copy
import os

import pytest
import torch
import torch.nn.functional as F

from conftest import gpu_device

pytestmark = pytest.mark.gpu


def _close(a, b, atol, rtol=0.0, what=""):
    a, b = a.float(), b.float()
    err = (a - b).abs().max().item()
    tol = atol + rtol * b.abs().max().item()
    print(f"{what}: max err {err:.3e} tol {tol:.3e}")
    assert err <= tol, f"{what}: max err {err:.3e} > tol {tol:.3e}"


def _fro(a, b):
    """Relative Frobenius-norm error of a against b."""
    a, b = a.double(), b.double()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def _log(line: str) -> None:
    print(line)
    path = os.environ.get("DDL_MLM_LOG")          # the measurement log of a profiling run
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


# ------------------------------------------------------------------ CE kernels
def _labels(M, C, pattern, dev):
    g = torch.Generator().manual_seed(M * 7 + C)
    y = torch.randint(0, C, (M,), generator=g)
    y[min(1, M - 1)] = C - 1
    if pattern == "mixed":
        y[::3] = -100
    elif pattern == "all":
        y[:] = -100
    return y.to(dev)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("M,C,ld", [(5, 8, 8), (64, 1000, 1000), (7, 30522, 30528), (3, 32776, 32776)])
def test_ce_kernels(M, C, ld, dtype):
    """ddl_ce_lse / ddl_ce_bwd on [M, ld] rows with C valid columns (the last shape is past the
    register-resident width) against F.cross_entropy on the fp32 copy of the valid columns; the
    tolerances are test_kernels_gpu.test_cross_entropy's, the incoming gradient is 2 as there."""
    dev = gpu_device()
    from databricks_distributed_deep_learning_amd import ops
    from databricks_distributed_deep_learning_amd.ops import _native_mlm as N
    torch.manual_seed(0)
    x = torch.full((M, ld), float("inf"), device=dev, dtype=dtype)      # pad columns: +inf, never used
    x[:, :C] = (torch.randn(M, C, device=dev) * 3).to(dtype)
    g = torch.full((), 2.0, device=dev)
    for pattern in ("mixed", "all", "none"):
        y = _labels(M, C, pattern, dev)
        assert pattern == "all" or bool((y == C - 1).any())
        xr = x[:, :C].float().clone().requires_grad_(True)
        if pattern == "all":
            ref_loss, ref_grad = torch.zeros((), device=dev), torch.zeros(M, C, device=dev)
        else:
            ref_loss = F.cross_entropy(xr, y, ignore_index=-100)
            (ref_loss * 2).backward()
            ref_grad = xr.grad
        runs = []
        for _ in range(2):
            loss, lse, inv_n = N._lse(x, M, ld, C, y, -100)
            dl = torch.empty_like(x)
            N._bwd(x, M, ld, C, y, -100, lse, g, inv_n, dl)
            inplace = x.clone()
            N._bwd(inplace, M, ld, C, y, -100, lse, g, inv_n, inplace)
            assert torch.equal(dl, inplace), "in-place backward differs"
            runs.append((loss.clone(), dl))
        assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1]), "not repeatable"
        loss, dl = runs[0]
        assert loss.dtype == torch.float32
        _close(loss, ref_loss.detach(), 1e-3 if dtype == torch.bfloat16 else 1e-5, 1e-3, f"loss {pattern}")
        _close(dl[:, :C], ref_grad, 1e-3, 1e-2, f"grad {pattern}")
        assert torch.isfinite(dl).all()
        if bool((y == -100).any()):
            assert dl[y == -100].abs().max().item() == 0.0, "ignored rows of the gradient are not exact zeros"
        if ld > C:
            assert dl[:, C:].abs().max().item() == 0.0, "pad columns of the gradient are not exact zeros"
        # the public op on the unpadded logits: the same kernels (through an 8-padded copy when C % 8)
        xc = x[:, :C].contiguous().requires_grad_(True)
        l2 = ops.cross_entropy(xc, y, ignore_index=-100)
        assert torch.equal(l2.detach(), loss)
        (l2 * 2).backward()
        assert torch.equal(xc.grad, dl[:, :C])


# ------------------------------------------------------------------ gather / scatter
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("D", [128, 1024])
def test_gather_scatter_rows(D, dtype):
    dev = gpu_device()
    from databricks_distributed_deep_learning_amd import ops
    torch.manual_seed(1)
    R, n = 96, 12
    h = torch.randn(R, D, device=dev).to(dtype).requires_grad_(True)
    pos = torch.tensor([0, 95, 17, 33, 64, 1, 50, 80, 0, 0, 0, 0], device=dev)     # 4 padded slots on row 0
    lab = torch.tensor([4, 9, 2, 7, 7, 1, 3, 8, -100, -100, -100, -100], device=dev)
    out = ops.gather_rows(h, pos, lab, -100)
    assert torch.equal(out, h.detach()[pos])
    dy = torch.randn(n, D, device=dev).to(dtype)
    out.backward(dy)
    want = torch.zeros(R, D, device=dev, dtype=dtype)
    want[pos[:8]] = dy[:8]
    assert torch.equal(h.grad, want)
    # positions per sequence ([B, P] into [B, S, D]): the flat index is formed in the kernel
    h3 = h.detach().reshape(4, 24, D).requires_grad_(True)
    p2 = torch.tensor([[0, 23, 5], [7, 0, 0], [1, 2, 3], [22, 0, 0]], device=dev)
    l2 = torch.tensor([[1, 2, 3], [4, -100, -100], [5, 6, 7], [8, 9, -100]], device=dev)
    o2 = ops.gather_rows(h3, p2, l2, -100)
    flat = (p2 + torch.arange(4, device=dev)[:, None] * 24).reshape(-1)
    assert torch.equal(o2, h.detach()[flat])
    dy2 = torch.randn(12, D, device=dev).to(dtype)
    o2.backward(dy2)
    keep = (l2 != -100).reshape(-1)
    want2 = torch.zeros(R, D, device=dev, dtype=dtype)
    want2[flat[keep]] = dy2[keep]
    assert torch.equal(h3.grad.reshape(R, D), want2)


# ------------------------------------------------------------------ fused head
def _head_case(M, K, V, dev):
    g = torch.Generator().manual_seed(M * 31 + V)
    x = torch.randn(M, K, generator=g).bfloat16().to(dev)
    w = (torch.randn(V, K, generator=g) * 0.1).bfloat16().to(dev)
    b = (torch.randn(V, generator=g) * 0.1).bfloat16().to(dev)
    y = torch.randint(0, V, (M,), generator=g)
    y[::3] = -100
    y[1] = V - 1
    return x, w, b, y.to(dev)


def _arm(x, w, b, y, how):
    x, w, b = (t.detach().clone().requires_grad_(True) for t in (x, w, b))
    if how == "fp32":
        xf, wf, bf = x.float(), w.float(), b.float()
        loss = F.cross_entropy(F.linear(xf, wf, bf), y, ignore_index=-100)
    elif how == "stock":
        loss = F.cross_entropy(F.linear(x, w, b).float(), y, ignore_index=-100)
    else:
        from databricks_distributed_deep_learning_amd import ops
        loss = ops.linear_cross_entropy(x, w, b, y, -100)
    loss.backward()
    return {"loss": loss.detach().float(), "dx": x.grad.float(), "dW": w.grad.float(), "db": b.grad.float()}


@pytest.mark.parametrize("M", [10, 130])
@pytest.mark.parametrize("V", [1000, 1002])
def test_linear_cross_entropy(M, V):
    """The fused head against an fp32 reference on the same bf16-rounded inputs.  The bound is
    measured here: the error of the stock bf16 arm (bf16 F.linear, .float(), F.cross_entropy)
    against the same reference, times 2 -- the factor covers a different summation order, not a
    different algorithm -- in relative Frobenius norm per tensor."""
    dev = gpu_device()
    x, w, b, y = _head_case(M, 128, V, dev)
    ref = _arm(x, w, b, y, "fp32")
    stock = _arm(x, w, b, y, "stock")
    got = _arm(x, w, b, y, "native")
    again = _arm(x, w, b, y, "native")
    bad = []
    for k in ("loss", "dx", "dW", "db"):
        e_nat, e_stock = _fro(got[k], ref[k]), _fro(stock[k], ref[k])
        _log(f"linear_cross_entropy M={M} K=128 V={V} {k}: native {e_nat:.3e} stock-bf16 {e_stock:.3e}")
        if not e_nat <= 2 * e_stock:
            bad.append((k, e_nat, e_stock))
        assert torch.equal(got[k], again[k]), f"{k} not repeatable"
    assert not bad, bad


def test_linear_cross_entropy_logits_and_gradient_slots():
    """return_logits hands out the unpadded logits and leaves them alone; under a reducer the
    weight gradient goes into its slot (rows 0..V-1 only: the next arena entry stays untouched)."""
    dev = gpu_device()
    import torch.nn as nn
    from databricks_distributed_deep_learning_amd import ops
    from databricks_distributed_deep_learning_amd.optim import ParamArena
    from databricks_distributed_deep_learning_amd.parallel.ddp import DataParallel
    M, K = 130, 128
    for V in (1000, 1002):
        x, w, b, y = _head_case(M, K, V, dev)
        ref = _arm(x, w, b, y, "native")

        class Head(nn.Module):
            def __init__(self):
                super().__init__()
                self.after = nn.Parameter(torch.zeros(1024, device=dev, dtype=torch.bfloat16))   # follows w
                self.w = nn.Parameter(w.clone())
                self.b = nn.Parameter(b.clone())

        m = Head()
        arena = ParamArena(list(m.named_parameters()))
        names = [e.name for e in arena.entries]
        ew, ea = arena.entries[names.index("w")], arena.entries[names.index("after")]
        assert ea.offset == ew.offset + V * K          # no gap: a leaked pad row would land in `after`
        dp = DataParallel(m, arena, broadcast_init=False, comm="torch")
        dp.zero_grad()
        xg = x.clone().requires_grad_(True)
        loss, logits = ops.linear_cross_entropy(xg, m.w, m.b, y, -100, return_logits=True)
        keep = logits.clone()
        want_logits = F.linear(x.float(), w.float(), b.float())
        assert logits.shape == (M, V) and not logits.requires_grad
        _close(logits, want_logits, 0.0, 2.0 ** -7, "logits")       # the bf16 store rounds by 2^-9; 4x margin
        loss.backward()
        flat = dp.finish()
        torch.cuda.synchronize()
        assert torch.equal(logits, keep), "returned logits were overwritten by the backward"
        assert torch.equal(loss.detach().float(), ref["loss"])
        assert torch.equal(xg.grad.float(), ref["dx"])
        # (accumulating into the slot may take another split-K plan than a fresh output: bf16 rounding)
        assert _fro(flat[ew.offset:ew.offset + V * K].view(V, K).float(), ref["dW"]) <= 2.0 ** -8
        assert torch.equal(m.b.grad.float(), ref["db"])
        assert flat[ea.offset:ea.offset + 1024].abs().max().item() == 0.0
        dp.close()


# ------------------------------------------------------------------ model
def _batch(dev, V, B=3, S=32, P=6):
    g = torch.Generator().manual_seed(11)
    ids = torch.randint(0, V // 2, (B, S), generator=g)             # inputs: lower half of the vocabulary
    mask = torch.ones(B, S)
    mask[1, 28:] = 0
    pos = torch.stack([torch.randperm(28, generator=g)[:P].sort().values for _ in range(B)])
    lab = torch.randint(V // 2, V, (B, P), generator=g)             # targets: upper half
    lab[0, 4:] = -100
    pos[0, 4:] = 0
    pos[2, 0] = 0
    nsp = torch.randint(0, 2, (B,), generator=g)
    return tuple(t.to(dev) for t in (ids, mask, pos, lab, nsp))


def test_bert_pretraining_native_vs_reference():
    dev = gpu_device()
    from test_models_gpu import _compare
    from databricks_distributed_deep_learning_amd.models import bert_tiny_pretraining
    torch.manual_seed(0)
    m = bert_tiny_pretraining(dropout=0.0).to(dev).train()
    ids, mask, pos, lab, nsp = _batch(dev, m.config.vocab_size)

    def run(mod):
        loss, (mlm_logits, nsp_logits) = mod(ids, mask, None, pos, lab, nsp)
        assert mlm_logits is None
        return loss.float()

    names = ["bert.embeddings.word_embeddings.weight", "mlm_dense.weight", "mlm_dense.bias", "mlm_ln.weight",
             "mlm_ln.bias", "mlm_bias", "seq_relationship.weight", "seq_relationship.bias"]
    assert set(names) <= set(dict(m.named_parameters()))
    _compare(m, run, names)


# ------------------------------------------------------------------ tied weight under the reducer
def _reducer_setup(dev, passes=1):
    from databricks_distributed_deep_learning_amd.models import bert_tiny_pretraining, cast_params
    from databricks_distributed_deep_learning_amd.optim import ParamArena
    from databricks_distributed_deep_learning_amd.parallel.ddp import DataParallel
    torch.manual_seed(0)
    m32 = bert_tiny_pretraining(dropout=0.0).to(dev).train()
    m = cast_params(copy.deepcopy(m32), torch.bfloat16)
    arena = ParamArena(list(m.named_parameters()))
    dp = DataParallel(m, arena, bucket_mb=0.05, first_bucket_mb=0.01, broadcast_init=False, comm="torch",
                      backward_passes_per_step=passes)
    assert len(dp.buckets) > 2
    e = next(e for e in arena.entries if e.name == "bert.embeddings.word_embeddings.weight")
    return m32, m, arena, dp, e


def _autograd_word_grad(model, batch):
    from databricks_distributed_deep_learning_amd import ops
    ids, mask, pos, lab, nsp = batch
    ops.set_native_mode("off")
    try:
        model.zero_grad(set_to_none=True)
        model(ids, mask, None, pos, lab, nsp)[0].backward()
        return model.bert.embeddings.word_embeddings.weight.grad.float().clone()
    finally:
        ops.set_native_mode("auto")


def test_tied_weight_through_reducer():
    """The decoder's wgrad (early in backward) and the embedding backward (last) both land in the
    word embedding's gradient slot, and the slot is reported to the reducer once per pass, after the
    second of them."""
    dev = gpu_device()
    from databricks_distributed_deep_learning_amd.models import cast_params
    m32, m, arena, dp, e = _reducer_setup(dev)
    batch = _batch(dev, m.config.vocab_size)
    ids, mask, pos, lab, nsp = batch
    ref = _autograd_word_grad(m32, batch)
    stock = _autograd_word_grad(cast_params(copy.deepcopy(m32), torch.bfloat16), batch)
    w = m.bert.embeddings.word_embeddings.weight
    slot = arena.grad[e.offset:e.offset + e.numel].view(e.shape)
    reports = []
    inner = w._ddl_grad_ready
    w._ddl_grad_ready = lambda: (reports.append(slot.clone()), inner())

    def step(n_backward):
        dp.zero_grad()
        for _ in range(n_backward):
            m(ids, mask, None, pos, lab, nsp)[0].backward()
        flat = dp.finish()
        torch.cuda.synchronize()
        return flat[e.offset:e.offset + e.numel].view(e.shape).clone()

    one = step(1)
    assert len(reports) == 1, f"{len(reports)} reports of the tied weight in one backward"
    assert torch.equal(reports[0], one), "the slot changed after it was reported"
    e_nat, e_stock = _fro(one, ref), _fro(stock, ref)
    _log(f"tied word-embedding gradient (bert_tiny_pretraining): native {e_nat:.3e} stock-bf16 {e_stock:.3e}")
    assert e_nat <= 2 * e_stock
    label_row = int(lab[lab != -100][0])
    input_row = int(ids[0, 5])
    assert not bool((ids == label_row).any()) and not bool((lab == input_row).any())
    assert one[label_row].abs().max().item() > 0 and one[input_row].abs().max().item() > 0
    assert torch.equal(step(1), one), "not repeatable"
    dp.close()

    # two accumulated passes: communicated on the second arrival, the slot holds both passes
    _, m, arena, dp, e = _reducer_setup(dev, passes=2)
    launched = []
    launch = dp._launch
    dp._launch = lambda b: (launched.append(len(reports)), launch(b))
    w = m.bert.embeddings.word_embeddings.weight
    slot = arena.grad[e.offset:e.offset + e.numel].view(e.shape)
    reports.clear()
    inner2 = w._ddl_grad_ready
    w._ddl_grad_ready = lambda: (reports.append(slot.clone()), inner2())
    two = step(2)
    assert len(reports) == 2
    assert launched and min(launched) >= 1, "a bucket was launched during the first of two passes"
    # per pass the slot takes at most two bf16-rounded adds of same-sign-or-smaller magnitude: 2 * 2^-9
    assert _fro(two, 2 * one.float()) <= 2.0 ** -7
    assert torch.equal(step(2), two), "not repeatable"
    dp.close()


def test_tied_weight_eager_optimizer_step():
    dev = gpu_device()
    from databricks_distributed_deep_learning_amd.optim import FlatAdamW
    _, m, arena, dp, e = _reducer_setup(dev)
    ids, mask, pos, lab, nsp = _batch(dev, m.config.vocab_size)
    opt = FlatAdamW(arena, lr=1e-3)
    before = arena.flat.float().clone()
    dp.zero_grad()
    opt.begin_step()
    dp.set_eager(lambda g, lo, hi: opt.step_range(g, 1.0, lo, hi))
    loss = m(ids, mask, None, pos, lab, nsp)[0]
    loss.backward()                     # raises if the tied weight reports twice with the eager optimizer on
    dp.finish()
    opt.end_step()
    torch.cuda.synchronize()
    after = arena.flat.float()
    assert torch.isfinite(after).all() and torch.isfinite(loss).all()
    w0 = before[e.offset:e.offset + e.numel]
    assert not torch.equal(after[e.offset:e.offset + e.numel], w0), "the word embedding was not updated"
    dp.close()
