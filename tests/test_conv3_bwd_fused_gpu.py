"""Fused conv3 / bn3 backward (csrc/kernels/conv3_bwd.hip): bn3's backward apply, conv3's dgrad with
bn2's backward reduction, and conv3's wgrad in one streaming pass, against

  * an fp32 PyTorch reference of the unfused math.  The bound is not a chosen number: the unfused
    native path (apply kernel, streaming dgrad, wgrad GEMM) is measured against the same reference at
    the same shapes and the fused path gets twice that error -- the summation order of dW (its
    per-workgroup chunks coincide with the unfused kernel's only at some M) is the only intended
    difference;
  * the unfused native path itself: dz2 bitwise (same dx3 image, same k order), dW and the sums
    within the bound above;
  * itself (bitwise repeatable);
  * at module level, a pair of bottleneck blocks with the switch on and off, a conv3 output with a
    second consumer (the correction path), and two consecutive steps (nothing stays parked).

M = 40 is less than two 32-row tiles (a ragged one), 64 * 3 + 17 ends on a ragged tile, and
256 * 64 * 2 + 5 gives every workgroup several tiles so the three-image ring wraps.  Workgroups walk
the row chunks of the unfused streaming dgrad, so the statistics rows are bitwise equal too.
"""
import functools

import pytest
import torch

from databricks_distributed_deep_learning_amd.ops import _lib
from databricks_distributed_deep_learning_amd.ops import bridge as B

pytestmark = pytest.mark.gpu

CO, CI = 256, 64
MS = [40, 64 * 3 + 17, 256 * 64 * 2 + 5]


def _inputs(M):
    g = torch.Generator(device="cuda").manual_seed(1234 + M)
    rn = lambda *s: torch.randn(*s, device="cuda", generator=g)       # noqa: E731
    ru = lambda *s: torch.rand(*s, device="cuda", generator=g)        # noqa: E731
    d = dict(M=M)
    d["dz"] = rn(M, CO).bfloat16()
    d["x3"] = (rn(M, CO) * 1.5 + 0.3).bfloat16()
    d["mean3"], d["istd3"] = rn(CO) * 0.3, ru(CO) + 0.5
    gamma3 = ru(CO) + 0.5
    # [gamma * istd | mean(dz) | mean(dz * xhat)] as the finalize would leave them
    d["coef"] = torch.cat([gamma3 * d["istd3"], rn(CO) * 0.05, rn(CO) * 0.05]).contiguous()
    d["a2"] = rn(M, CI).clamp_min(0).bfloat16()
    d["x2"] = (rn(M, CI) * 0.8 - 0.1).bfloat16()
    d["mean2"], d["istd2"] = rn(CI) * 0.2, ru(CI) + 0.5
    bits = ru(M * CI) > 0.5
    d["bits"] = bits.view(M, CI)
    d["mask"] = (bits.view(-1, 8).to(torch.uint8) << torch.arange(8, device="cuda", dtype=torch.uint8)).sum(1).to(
        torch.uint8)
    d["w"] = (rn(CO, 1, 1, CI) * 0.1).bfloat16()
    return d


def _reference(d):
    """fp32: apply, 1x1 dgrad with the masked bn2 reduction, wgrad."""
    k1, mb, mg = d["coef"].view(3, CO)
    xh3 = (d["x3"].float() - d["mean3"]) * d["istd3"]
    dx3 = k1 * (d["dz"].float() - mb - xh3 * mg)
    w = d["w"].float().view(CO, CI)
    dz2 = (dx3 @ w) * d["bits"].float()
    xh2 = (d["x2"].float() - d["mean2"]) * d["istd2"]
    return dict(dz2=dz2, s=dz2.sum(0), q=(dz2 * xh2).sum(0), dw=dx3.t() @ d["a2"].float())


def _bnb(d, mask=True):
    M = d["M"]
    return B.BNBackward(d["x2"].view(1, 1, M, CI), d["mask"] if mask else None, d["mean2"], d["istd2"])


def _sums(hint):
    rows = hint.nrows
    st = hint.part[:rows * 2 * CI].view(rows, 2, CI).double().sum(0).float()
    return st[0], st[1], hint.part[:rows * 2 * CI].clone()


def _unfused(d, mask=True, sink=None):
    from databricks_distributed_deep_learning_amd.ops import _native_conv as NC
    M = d["M"]
    dx3 = torch.empty_like(d["x3"])
    _lib.call("ddl_bn_bwd_apply_coef", 1, d["dz"].data_ptr(), d["x3"].data_ptr(), d["mean3"].data_ptr(),
              d["istd3"].data_ptr(), d["coef"].data_ptr(), M, CO, dx3.data_ptr())
    hint = _bnb(d, mask)
    dy = dx3.view(1, 1, M, CO)
    dz2 = NC._dgrad(dy, d["w"], (1, 1, M, CI), 1, 0, bnb=hint)
    assert hint.dz is dz2, "the unfused dgrad did not run the BN-backward epilogue"
    dw = NC._wgrad(dy, d["a2"].view(1, 1, M, CI), d["w"].shape, 1, 0, out=sink)
    s, q, rows = _sums(hint)
    torch.cuda.synchronize()
    return dict(dz2=dz2.view(M, CI), s=s, q=q, rows=rows, dw=dw.view(CO, CI), dx3=dx3)


def _fused(d, mask=True, sink=None):
    from databricks_distributed_deep_learning_amd.ops import _native_conv as NC
    M = d["M"]
    hint = _bnb(d, mask)
    parked = (d["dz"], d["x3"], d["mean3"], d["istd3"], d["coef"])
    out = NC._conv3_bwd_fused(parked, d["a2"].view(1, 1, M, CI), d["w"], hint, None, sink)
    assert out is not None, "shape not covered"
    dz2, dw = out
    assert (dw is None) == (sink is not None)
    dw = sink if dw is None else dw
    s, q, rows = _sums(hint)
    torch.cuda.synchronize()
    return dict(dz2=dz2.view(M, CI), s=s, q=q, rows=rows, dw=dw.view(CO, CI))


@functools.lru_cache(maxsize=None)
def _case(M):
    d = _inputs(M)
    return d, _reference(d), _unfused(d), _fused(d)


def _err(got, ref):
    return ((got.float() - ref).abs().max() / ref.abs().max().clamp_min(1e-30)).item()


@pytest.mark.parametrize("M", MS)
def test_fused_against_fp32_reference_within_twice_the_unfused_error(M):
    d, ref, unf, fus = _case(M)
    for k in ("dz2", "s", "q", "dw"):
        eu, ef = _err(unf[k], ref[k]), _err(fus[k], ref[k])
        print(f"conv3_bwd M={M} {k}: unfused err {eu:.3e} fused err {ef:.3e}")
        assert ef <= 2 * eu, (k, eu, ef)


@pytest.mark.parametrize("M", MS)
def test_fused_against_unfused_native(M):
    d, ref, unf, fus = _case(M)
    assert torch.equal(fus["dz2"], unf["dz2"]), "dz2 must be bitwise what the unfused path gives"
    assert torch.equal(fus["rows"], unf["rows"]), "same row chunks, same per-lane order: the same statistics rows"
    for k in ("s", "q", "dw"):
        bound = 2 * _err(unf[k], ref[k]) * ref[k].abs().max().item()
        diff = (fus[k].float() - unf[k].float()).abs().max().item()
        print(f"conv3_bwd M={M} {k}: |fused - unfused| {diff:.3e} bound {bound:.3e}")
        assert diff <= bound, (k, diff, bound)


@pytest.mark.parametrize("M", MS)
def test_fused_is_bitwise_repeatable(M):
    d, _, _, fus = _case(M)
    again = _fused(d)
    for k in ("dz2", "rows", "dw"):
        assert torch.equal(fus[k], again[k]), k


def test_fp32_gradient_sink_is_accumulated_into():
    """The path a training step takes: dW added into a pre-filled fp32 gradient sink."""
    d, ref, _, _ = _case(MS[1])
    g = torch.Generator(device="cuda").manual_seed(5)
    fill = torch.randn(CO, 1, 1, CI, device="cuda", generator=g) * ref["dw"].abs().max()
    su, sf = fill.clone(), fill.clone()
    unf, fus = _unfused(d, sink=su), _fused(d, sink=sf)
    want = fill.view(CO, CI) + ref["dw"]
    eu, ef = _err(unf["dw"], want), _err(fus["dw"], want)
    print(f"conv3_bwd fp32 sink: unfused err {eu:.3e} fused err {ef:.3e}")
    assert fus["dw"].dtype == torch.float32 and ef <= 2 * eu, (eu, ef)
    assert torch.equal(fus["dz2"], unf["dz2"])


def test_without_a_relu_mask():
    d = _inputs(MS[1])
    unf, fus = _unfused(d, mask=False), _fused(d, mask=False)
    want = _reference(dict(d, bits=torch.ones_like(d["bits"])))
    assert torch.equal(fus["dz2"], unf["dz2"]) and torch.equal(fus["rows"], unf["rows"])
    assert _err(fus["dz2"], want["dz2"]) <= 2 * _err(unf["dz2"], want["dz2"])
    assert _err(fus["dw"], want["dw"]) <= 2 * _err(unf["dw"], want["dw"])


# ---------------------------------------------------------------------------------- module level
class _Counter:
    def __init__(self, fn):
        self.fn, self.n, self.hits = fn, 0, 0

    def __call__(self, *a, **k):
        self.n += 1
        out = self.fn(*a, **k)
        self.hits += out is not None
        return out


def _blocks():
    from databricks_distributed_deep_learning_amd.models.resnet import Bottleneck
    torch.manual_seed(7)
    net = torch.nn.Sequential(Bottleneck(256, 64), Bottleneck(256, 64)).cuda().bfloat16().train()
    with torch.no_grad():
        for m in net.modules():
            if hasattr(m, "running_mean"):
                m.weight.copy_(torch.rand_like(m.weight) + 0.5)
                m.bias.copy_(torch.randn_like(m.bias) * 0.1)
    return net


def _step(net, x, gout, tap=None):
    """One forward / backward -> (input gradient, parameter gradients); ``tap``: a second consumer of
    the first block's conv3 output."""
    for p_ in net.parameters():
        p_.grad = None
    x = x.clone().requires_grad_(True)
    seen = []
    if tap is not None:
        h = net[0].conv3.register_forward_hook(lambda m, i, o: seen.append(o))
    out = net(x)
    loss = (out.float() * gout).sum()
    if tap is not None:
        h.remove()
        loss = loss + (seen[0].float() * tap).sum()
    loss.backward()
    torch.cuda.synchronize()
    return [x.grad.clone()] + [p_.grad.clone() for p_ in net.parameters()]


def _names(net):
    return ["input"] + [n for n, _ in net.named_parameters()]


def _compare(net, got, want, loose, bound, why):
    """Bitwise equality for every gradient except those named by ``loose`` (prefixes), which get
    ``bound`` x the tensor's largest element."""
    for n, g_, w_ in zip(_names(net), got, want):
        diff = (g_.float() - w_.float()).abs().max().item()
        if any(n.startswith(p_) for p_ in loose):
            top = w_.float().abs().max().item()
            print(f"conv3_bwd module {why}: {n} max|diff| / max|ref| = {diff / max(top, 1e-30):.3e} (bound {bound:.3e})")
            assert diff <= bound * top, (n, diff, top)
        else:
            assert diff == 0.0, (why, n, diff)


@pytest.fixture()
def _counted(monkeypatch):
    from databricks_distributed_deep_learning_amd.ops import _native_conv as NC
    fused, mat = _Counter(NC._conv3_bwd_fused), _Counter(NC._conv3_materialise)
    monkeypatch.setattr(NC, "_conv3_bwd_fused", fused)
    monkeypatch.setattr(NC, "_conv3_materialise", mat)
    return fused, mat


def _data():
    g = torch.Generator(device="cuda").manual_seed(99)
    x = torch.randn(2, 8, 8, 256, device="cuda", generator=g).bfloat16()
    gout = torch.randn(2, 8, 8, 256, device="cuda", generator=g)
    tap = torch.randn(2, 8, 8, 256, device="cuda", generator=g) * 0.5
    return x, gout, tap


def test_bottleneck_blocks_fused_against_switch_off(monkeypatch, _counted):
    fused, mat = _counted
    net = _blocks()
    x, gout, _ = _data()
    monkeypatch.setattr(B, "CONV3_FUSED", False)
    want = _step(net, x, gout)
    assert fused.n == 0 and mat.n == 0
    monkeypatch.setattr(B, "CONV3_FUSED", True)
    got = _step(net, x, gout)
    assert fused.hits >= 1 and mat.n == 0, "the first block's conv3 / bn3 backward must run fused"
    # dz2 and the statistics rows are bitwise the unfused kernels', so every gradient is bitwise equal
    # except the fused conv's own dW: both paths sum bf16-rounded per-workgroup partials (2^-9 of a
    # partial each, a partial is at most the size of the largest sum) over different row chunks, and
    # round the result to bf16 (2^-9): 2^-8 of the largest element covers both paths' rounding
    _compare(net, got, want, ["0.conv3.weight"], 2.0 ** -8, "fused")


def test_second_consumer_takes_the_correction_path(monkeypatch, _counted):
    fused, mat = _counted
    net = _blocks()
    x, gout, tap = _data()
    monkeypatch.setattr(B, "CONV3_FUSED", False)
    want = _step(net, x, gout, tap)
    monkeypatch.setattr(B, "CONV3_FUSED", True)
    got = _step(net, x, gout, tap)
    assert mat.n >= 1, "the summed gradient is a new tensor: dx3 must be materialised"
    # the second block and the first block's bn3 run before the correction: bitwise.  Below it the
    # switch-off path feeds conv3 bf16(dx3 + tap); the correction feeds bf16(bf16(bf16(dz + tap) - dz)
    # + dx3): up to three more bf16 roundings (2^-9 each) at the magnitudes of dz + tap, tap and the
    # result, i.e. an element-wise perturbation of up to ~4 x 2^-9 of the gradient's own scale, which
    # the GEMMs and BatchNorm sums below carry on without growing in norm: 2^-6 of the largest element
    exact = ["1.", "0.bn3."]
    loose = [n for n in _names(net) if not any(n.startswith(p_) for p_ in exact)]
    _compare(net, got, want, loose, 2.0 ** -6, "correction")


def test_two_consecutive_steps_leave_nothing_parked(monkeypatch, _counted):
    fused, _ = _counted
    monkeypatch.setattr(B, "CONV3_FUSED", True)
    net = _blocks()
    x, gout, _ = _data()
    hints = []
    real = B.Conv3Fold.__init__

    def spy(self):
        real(self)
        hints.append(self)

    monkeypatch.setattr(B.Conv3Fold, "__init__", spy)
    first = _step(net, x, gout)
    assert hints and all(h.parked is None for h in hints)
    n1 = fused.hits
    second = _step(net, x, gout)
    assert all(h.parked is None for h in hints) and fused.hits == 2 * n1
    # BatchNorm running statistics do not enter the training-mode gradients: the steps are the same
    _compare(net, second, first, [], 0.0, "second step")
