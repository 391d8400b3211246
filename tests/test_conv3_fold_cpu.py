"""The Python hand-over of the fused conv3 / bn3 backward (ops/bridge.py Conv3Fold, the hint the
convolution leaves and the BatchNorm keeps), exercised without the native kernels."""
import pytest
import torch

from databricks_distributed_deep_learning_amd.ops import bridge as B


def _triple():
    dz = torch.randn(4, 256).bfloat16()
    x = torch.randn(4, 256).bfloat16()
    return dz, x, torch.zeros(256), torch.ones(256), torch.zeros(3 * 256)


def test_park_take_hands_over_once_and_clears():
    h = B.Conv3Fold()
    assert h.take() is None
    t = _triple()
    h.park(*t)
    got = h.take()
    assert all(a is b for a, b in zip(got, t))
    assert h.parked is None and h.take() is None


def test_double_park_is_an_error():
    h = B.Conv3Fold()
    h.park(*_triple())
    with pytest.raises(RuntimeError):
        h.park(*_triple())


def test_is_parked_means_the_very_tensor():
    t = _triple()
    dz = t[0]
    assert B.Conv3Fold.is_parked(t, dz)
    assert B.Conv3Fold.is_parked(t, dz.view(2, 2, 256))          # same storage, same size
    assert not B.Conv3Fold.is_parked(t, dz.clone())              # autograd summed into a new tensor
    assert not B.Conv3Fold.is_parked(t, dz[:2])                  # same pointer, another size
    assert not B.Conv3Fold.is_parked(t, dz + 0)


def test_conv_leaves_no_hint_off_the_gpu_or_with_the_switch_off(monkeypatch):
    from databricks_distributed_deep_learning_amd.ops import _native_conv as NC
    x = torch.randn(1, 4, 4, 64).bfloat16()
    w = torch.randn(256, 1, 1, 64).bfloat16()
    assert not NC._conv3_fold_ok(x, w, 1, 0)                      # not a GPU tensor
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
    assert NC._conv3_fold_ok(x, w, 1, 0)
    assert not NC._conv3_fold_ok(x, w, 2, 0)
    assert not NC._conv3_fold_ok(x.float(), w, 1, 0)
    assert not NC._conv3_fold_ok(x, torch.randn(512, 1, 1, 64).bfloat16(), 1, 0)
    assert not NC._conv3_fold_ok(x.transpose(1, 2), w, 1, 0)
    monkeypatch.setattr(B, "CONV3_FUSED", False)
    assert not NC._conv3_fold_ok(x, w, 1, 0)


def test_batchnorm_keeps_the_hint_only_for_the_tensor_it_saves():
    from databricks_distributed_deep_learning_amd.ops import _native_norm as NN
    x = torch.randn(1, 4, 4, 256).bfloat16().requires_grad_(True)
    assert NN._conv3_hint(x) is None                             # no convolution left one
    hint = B.Conv3Fold()
    x._ddl_c3 = hint
    assert NN._conv3_hint(x) is hint
    y = x.detach()
    y._ddl_c3 = hint
    assert NN._conv3_hint(y) is None                             # its gradient is not asked for
    z = x.transpose(1, 2)
    z._ddl_c3 = hint
    assert NN._conv3_hint(z) is None                             # the BatchNorm would save a copy
    f = torch.randn(1, 4, 4, 256, requires_grad=True)
    f._ddl_c3 = hint
    assert NN._conv3_hint(f) is None                             # fp32 is unchanged


# ------------------------------------------------------------------ the hand-over itself, on the CPU
# _bn_backward and _Conv.backward run for real; the native entry points they reach are replaced by
# small torch implementations working on the same raw pointers.
import ctypes
from types import SimpleNamespace

C3, CIN, MROWS = 256, 64, 12


def _at(ptr, n, dtype):
    size = n * torch.empty(0, dtype=dtype).element_size()
    return torch.frombuffer((ctypes.c_char * size).from_address(ptr), dtype=dtype)


class _Native:
    """Torch stand-ins for the C entry points the hand-over calls (the stream argument is absent,
    as in ``_lib.call``)."""

    def __init__(self):
        self.calls = []

    def call(self, name, *a):
        self.calls.append(name)
        fn = getattr(self, name, None)
        if fn is not None:
            fn(*a)

    def fn(self, name):
        return {"ddl_bn_bwd_nblk": lambda M, C: 4}[name]

    @staticmethod
    def _coef(part, nrows, invstd, gamma, M, C, dgamma, dbeta, coef, acc):
        rows = _at(part, nrows * 2 * C, torch.float32).view(nrows, 2, C).sum(0)
        g = _at(gamma, C, torch.bfloat16).float()
        _at(coef, 3 * C, torch.float32).copy_(torch.cat([g * _at(invstd, C, torch.float32), rows[0] / M, rows[1] / M]))
        for ptr, v in ((dgamma, rows[1]), (dbeta, rows[0])):
            out = _at(ptr, C, torch.bfloat16)
            out.copy_((out.float() if acc else 0) + v)

    @staticmethod
    def _apply(dz, x, mean, istd, coef, M, C, dx):
        k1, mb, mg = _at(coef, 3 * C, torch.float32).view(3, C)
        xh = (_at(x, M * C, torch.bfloat16).float().view(M, C) - _at(mean, C, torch.float32)) * _at(istd, C, torch.float32)
        out = k1 * (_at(dz, M * C, torch.bfloat16).float().view(M, C) - mb - xh * mg)
        _at(dx, M * C, torch.bfloat16).copy_(out.bfloat16().view(-1))

    def ddl_bn_bwd_coef_from_partials(self, dt, part, nrows, ws, ws_n, invstd, gamma, M, C, dgamma, dbeta, coef, acc):
        self._coef(part, nrows, invstd, gamma, M, C, dgamma, dbeta, coef, acc)

    def ddl_bn_bwd_apply_coef(self, dt, dz, x, mean, istd, coef, M, C, dx):
        self._apply(dz, x, mean, istd, coef, M, C, dx)

    def ddl_bn_bwd_from_partials(self, dt, part, nrows, ws, ws_n, dz, x, mean, invstd, gamma, M, C, dgamma, dbeta,
                                 coef, dx, dres, acc):
        self._coef(part, nrows, invstd, gamma, M, C, dgamma, dbeta, coef, acc)
        self._apply(dz, x, mean, invstd, coef, M, C, dx)


@pytest.fixture()
def native(monkeypatch):
    from databricks_distributed_deep_learning_amd.ops import _lib, _native_norm as NN
    n = _Native()
    monkeypatch.setattr(_lib, "call", n.call)
    monkeypatch.setattr(NN, "call", n.call)
    monkeypatch.setattr(_lib, "fn", n.fn)
    monkeypatch.setattr(NN, "_group_sum", lambda row, group: None)
    return n


def _bn_case(hint=True, given=True, group=None):
    """A bn3-like BatchNorm backward: (ctx, dz, x, mask, weight, stats, the BNBackward hint)."""
    torch.manual_seed(3)
    x = torch.randn(1, 1, MROWS, C3).bfloat16()
    dz = torch.randn(1, 1, MROWS, C3).bfloat16()
    weight = (torch.rand(C3) + 0.5).bfloat16()
    stats = torch.stack([torch.randn(C3) * 0.1, torch.rand(C3) + 0.5, torch.ones(C3), torch.zeros(C3)]).contiguous()
    bnb = None
    if given:
        bnb = B.BNBackward(x, None, stats[0], stats[1])
        nrows = 3
        xh = (x.float().view(MROWS, C3) - stats[0]) * stats[1]
        d = dz.float().view(MROWS, C3)
        part = torch.zeros(nrows * 2 * C3 + 2 * C3)
        rows = part[:nrows * 2 * C3].view(nrows, 2, C3)
        for r in range(nrows):                         # the sums split over three "workgroups"
            sl = slice(r * 4, r * 4 + 4)
            rows[r, 0], rows[r, 1] = d[sl].sum(0), (d[sl] * xh[sl]).sum(0)
        bnb.set(dz, part, nrows)
    ctx = SimpleNamespace(bnb=bnb, group=group, has_res=True, relu=True, params=(weight, weight.clone()), bridge=None,
                          c3=B.Conv3Fold() if hint else None, m_total=MROWS)
    return ctx, dz, x, weight, stats


def _expected_dx3(dz, x, weight, stats):
    d, xv = dz.float().view(MROWS, C3), x.float().view(MROWS, C3)
    xh = (xv - stats[0]) * stats[1]
    return (weight.float() * stats[1]) * (d - d.mean(0) - xh * (d * xh).mean(0))


def test_bn_backward_folds_with_hint_and_given_sums_and_no_group(native):
    from databricks_distributed_deep_learning_amd.ops import _native_norm as NN
    ctx, dz, x, weight, stats = _bn_case()
    hint = ctx.c3
    dx, dgamma, dbeta, dres = NN._bn_backward(ctx, dz, x, None, weight, stats)
    assert dx is dz and dres is dz                               # dz itself, no apply pass, no copy
    assert "ddl_bn_bwd_coef_from_partials" in native.calls
    assert not {"ddl_bn_bwd_from_partials", "ddl_bn_bwd", "ddl_bn_bwd_apply_coef"} & set(native.calls)
    pdz, px, pmean, pistd, coef = hint.parked
    assert pdz is dz and px is x
    d = dz.float().view(MROWS, C3)
    xh = (x.float().view(MROWS, C3) - stats[0]) * stats[1]
    torch.testing.assert_close(coef.view(3, C3)[1], d.mean(0), rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(coef.view(3, C3)[2], (d * xh).mean(0), rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(dbeta.float(), d.sum(0), rtol=2e-2, atol=2e-2)      # bf16 parameters
    torch.testing.assert_close(dgamma.float(), (d * xh).sum(0), rtol=2e-2, atol=2e-2)


@pytest.mark.parametrize("why", ["no hint", "no given sums", "SyncBN group"])
def test_bn_backward_does_not_fold_otherwise(native, why):
    from databricks_distributed_deep_learning_amd.ops import _native_norm as NN
    ctx, dz, x, weight, stats = _bn_case(hint=why != "no hint", given=why != "no given sums",
                                         group=object() if why == "SyncBN group" else None)
    hint = ctx.c3
    dx, _, _, dres = NN._bn_backward(ctx, dz, x, None if why != "no given sums" else torch.zeros(1), weight, stats)
    assert dx is not dz and "ddl_bn_bwd_coef_from_partials" not in native.calls
    assert hint is None or hint.parked is None
    want = {"no hint": "ddl_bn_bwd_from_partials", "no given sums": "ddl_bn_bwd", "SyncBN group": "ddl_bn_bwd_finish"}
    assert want[why] in native.calls
    if why == "no hint":
        torch.testing.assert_close(dx.float().view(MROWS, C3), _expected_dx3(dz, x, weight, stats), rtol=2e-2,
                                   atol=2e-2)


def _conv_case(monkeypatch, fused_covers=True):
    """conv3's backward after a folding bn3: (ctx, hint, dz, dx3 the apply pass would write, log)."""
    from databricks_distributed_deep_learning_amd.ops import _native_conv as NC, _native_norm as NN
    bctx, dz, x3, weight, stats = _bn_case()
    hint = bctx.c3
    NN._bn_backward(bctx, dz, x3, None, weight, stats)
    assert hint.parked is not None
    a2 = torch.randn(1, 1, MROWS, CIN).bfloat16()
    w = (torch.randn(C3, 1, 1, CIN) * 0.1).bfloat16()
    log = SimpleNamespace(fused=[], dgrad=[], wgrad=[])

    def fused(parked, x, w_, bnb, param, sink):
        log.fused.append(parked)
        return (torch.zeros_like(x), torch.zeros_like(w_)) if fused_covers else None

    def dgrad(dy, w_, x_shape, stride, pad, residual=None, bnb=None, param=None):
        log.dgrad.append(dy)
        return torch.zeros(x_shape, dtype=dy.dtype)

    def wgrad(dy, x, w_shape, stride, pad, out=None):
        log.wgrad.append(dy)
        return torch.zeros(w_shape, dtype=dy.dtype)

    monkeypatch.setattr(NC, "_conv3_bwd_fused", fused)
    monkeypatch.setattr(NC, "_dgrad", dgrad)
    monkeypatch.setattr(NC, "_wgrad", wgrad)
    ctx = SimpleNamespace(saved_tensors=(a2, w), needs_input_grad=(True, True, False, False, False, False, False),
                          c3=hint, bnb=object(), bridge=None, grad_to=None, w_param=w, stride=1, pad=0)
    dx3 = _expected_dx3(dz, x3, weight, stats).bfloat16().view(1, 1, MROWS, C3)
    return ctx, hint, dz, dx3, log


def test_conv_backward_runs_fused_only_for_the_very_tensor(native, monkeypatch):
    from databricks_distributed_deep_learning_amd.ops import _native_conv as NC
    ctx, hint, dz, dx3, log = _conv_case(monkeypatch)
    NC._Conv.backward(ctx, dz)
    assert len(log.fused) == 1 and log.fused[0][0] is dz and not log.dgrad and not log.wgrad
    assert hint.parked is None and "ddl_bn_bwd_apply_coef" not in native.calls


def test_conv_backward_corrects_a_gradient_that_is_not_the_parked_dz(native, monkeypatch):
    from databricks_distributed_deep_learning_amd.ops import _native_conv as NC
    ctx, hint, dz, dx3, log = _conv_case(monkeypatch)
    extra = torch.randn_like(dz.float())
    summed = (dz.float() + extra).bfloat16()                    # a second consumer: autograd's new tensor
    NC._Conv.backward(ctx, summed)
    assert not log.fused and hint.parked is None
    assert "ddl_bn_bwd_apply_coef" in native.calls
    want = (summed - dz) + dx3                                   # - dz + dx3, in the gradient's own dtype
    assert torch.equal(log.dgrad[0], want) and log.wgrad[0] is log.dgrad[0]
    torch.testing.assert_close(log.dgrad[0].float(), extra + dx3.float(), rtol=0, atol=0.0625)


def test_conv_backward_materialises_when_the_fused_kernel_does_not_cover(native, monkeypatch):
    from databricks_distributed_deep_learning_amd.ops import _native_conv as NC
    ctx, hint, dz, dx3, log = _conv_case(monkeypatch, fused_covers=False)
    NC._Conv.backward(ctx, dz)
    assert len(log.fused) == 1 and hint.parked is None
    torch.testing.assert_close(log.dgrad[0].float(), dx3.float(), rtol=0, atol=2.0 ** -7 * dx3.float().abs().max().item())
    assert log.dgrad[0].data_ptr() != dz.data_ptr()


def test_conv_backward_without_a_parked_gradient_is_the_ordinary_path(native, monkeypatch):
    from databricks_distributed_deep_learning_amd.ops import _native_conv as NC
    ctx, hint, dz, dx3, log = _conv_case(monkeypatch)
    hint.take()                                                  # the BatchNorm ran its own apply pass
    NC._Conv.backward(ctx, dz)
    assert not log.fused and log.dgrad[0] is dz and "ddl_bn_bwd_apply_coef" not in native.calls
