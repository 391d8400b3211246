"""Linear layers at M <= 16 rows (GPU only; csrc/kernels/linear_decode.hip through ops.linear_small_m).

Cases: M in {1, 2, 3, 8, 16} x (N, K) in {(1, 8), (7, 64), (8, 72), (257, 768), (768, 3072), (3072, 768)},
plus the vocabulary head (50257, 768) at M = 2, each with no epilogue, bias, bias + GELU and bias +
residual.  They cover an N below one 16-row tile, N tails (7, 257, 50257 = 16 * 3141 + 1), a K below and
not a multiple of the 64-deep k step (8, 72), the 4-tile-per-wave kernel (N > 4096) and K splits over
gridDim.y with the second, combining launch ((257, 768), (768, 3072), (3072, 768) on a 256-CU part).

Tolerance: the form of tests/test_attention_edges_gpu.py (`check`, M = 2): against fp64 from the bf16
inputs, bounded by twice the error of an fp32 emulation with a bf16 output plus half a bf16 ulp.  Every
case prints its ratios.  The exact-selection cases (one-hot weight rows with power-of-two values, so
y[m, n] = c x[m, k(n)] exactly, k(n) running over the first and last element of every wave's k range)
and the repeatability case compare bits.

Measured on an MI355X: 124 comparisons.  With the ulp term subtracted the largest ratios are
-0.000 (max form, e.g. M = 2, N = 50257, bias + residual) and 0.062 (rms form; M = 8, N = 1, K = 8, where the
whole output is 8 numbers), at most -0.012 otherwise; as plain kernel error / emulation error the largest is 1.00.
K splits taken on the 256-CU part: (257, 768) and (3072, 768) 3, (768, 3072) 12, the other shapes 1.  So
M = 2 holds as it stands.
"""
import pytest
import torch

from conftest import gpu_device
from test_attention_edges_gpu import M as MARGIN, check  # noqa: F401

from databricks_distributed_deep_learning_amd import ops

pytestmark = pytest.mark.gpu

MS = [1, 2, 3, 8, 16]
SHAPES = [(1, 8), (7, 64), (8, 72), (257, 768), (768, 3072), (3072, 768)]
EPIS = ["none", "bias", "bias_gelu", "bias_res"]


def _inputs(m, n, k, dev, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    x = torch.randn(m, k, generator=g).bfloat16().to(dev)
    w = (torch.randn(n, k, generator=g) * k ** -0.5).bfloat16().to(dev)
    b = torch.randn(n, generator=g).bfloat16().to(dev)
    r = torch.randn(m, n, generator=g).bfloat16().to(dev)
    return x, w, b, r


def _ref(x, w, b, r, epi, dt):
    y = x.to(dt) @ w.to(dt).t()
    if epi != "none":
        y = y + b.to(dt)
    if epi == "bias_gelu":
        y = torch.nn.functional.gelu(y)
    if epi == "bias_res":
        y = y + r.to(dt)
    return y


def _run(x, w, b, r, epi):
    y = ops.linear_small_m(x, w, None if epi == "none" else b, "gelu" if epi == "bias_gelu" else None,
                           r if epi == "bias_res" else None)
    torch.cuda.synchronize()
    return y


def _parity(fails, m, n, k, dev):
    x, w, b, r = _inputs(m, n, k, dev, 1000 * m + n + k)
    w64, w32 = w.double(), w.float()
    for epi in EPIS:
        r64 = _ref(x, w64, b, r, epi, torch.float64)
        em = _ref(x, w32, b, r, epi, torch.float32).bfloat16()
        y = _run(x, w, b, r, epi)
        assert y.shape == (m, n) and y.dtype == torch.bfloat16
        check(fails, f"M={m} N={n} K={k} {epi}", y, r64, em)


@pytest.mark.parametrize("n,k", SHAPES, ids=[f"{n}x{k}" for n, k in SHAPES])
def test_parity(n, k):
    dev = gpu_device()
    fails = []
    for m in MS:
        _parity(fails, m, n, k, dev)
    assert not fails, "\n".join(fails)


def test_parity_vocabulary_head():
    dev = gpu_device()
    fails = []
    _parity(fails, 2, 50257, 768, dev)
    assert not fails, "\n".join(fails)


def _k_edges(n, k):
    """First and last element of every wave's k range, of every 64-deep step's, and of K."""
    from databricks_distributed_deep_learning_amd.ops import _native_linear_decode as NL
    _, _, ksplit, per = NL.plan(n, k)
    edges = {0, k - 1}
    for step in (64, 64 * per):
        for a in range(0, k, step):
            edges |= {a, min(a + step, k) - 1}
    return sorted(edges), ksplit


@pytest.mark.parametrize("n,k", SHAPES + [(50257, 768)], ids=[f"{n}x{k}" for n, k in SHAPES + [(50257, 768)]])
def test_exact_selection(n, k):
    """A mis-indexed row, a lost or doubled K slice and an N tail all change bits here."""
    dev = gpu_device()
    edges, ksplit = _k_edges(n, k)
    print(f"N={n} K={k}: ksplit {ksplit}, {len(edges)} edges")
    ar = torch.arange(n, device=dev)
    c = torch.pow(2.0, (ar % 5 - 2).float())
    et = torch.tensor(edges, device=dev)
    for m in ([2] if n > 4096 else MS):
        x = torch.randn(m, k, device=dev).bfloat16()
        for rot in range(-(-len(edges) // n)):
            kn = et[(ar + rot * n) % len(edges)]
            w = torch.zeros(n, k, device=dev)
            w[ar, kn] = c
            y = _run(x, w.bfloat16(), None, None, "none")
            want = (x.float()[:, kn] * c).bfloat16()
            assert torch.equal(y.view(torch.int16), want.view(torch.int16)), (m, rot)


def test_repeatable_with_k_split():
    from databricks_distributed_deep_learning_amd.ops import _native_linear_decode as NL
    dev = gpu_device()
    assert NL.plan(768, 3072)[2] > 1
    x, w, b, r = _inputs(3, 768, 3072, dev, 5)
    a, c = _run(x, w, b, r, "bias_res"), _run(x, w, b, r, "bias_res")
    assert torch.equal(a.view(torch.int16), c.view(torch.int16))


def test_m17_goes_to_ops_linear():
    dev = gpu_device()
    x, w, b, r = _inputs(17, 768, 768, dev, 9)
    for epi in EPIS:
        bias, act, res = (None if epi == "none" else b), ("gelu" if epi == "bias_gelu" else None), \
            (r if epi == "bias_res" else None)
        want = ops.linear(x, w, bias, act, residual=res)
        assert torch.equal(_run(x, w, b, r, epi).view(torch.int16), want.view(torch.int16))


def test_batched_leading_dims_and_no_autograd():
    dev = gpu_device()
    x, w, b, _ = _inputs(4, 64, 32, dev, 2)
    y = ops.linear_small_m(x.view(2, 2, 32), w, b)
    assert y.shape == (2, 2, 64) and torch.equal(y.view(4, 64), ops.linear_small_m(x, w, b))
    with pytest.raises(RuntimeError, match="autograd"):
        ops.linear_small_m(x.clone().requires_grad_(True), w, b)
