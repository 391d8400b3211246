"""The convolution oracle (tests/conv_oracle.py) against fp64 ``F.conv2d`` + autograd, its absolute-sum
companions against the same ops on absolute values, and the exact tier's conditions on every case the
GPU file runs (built from the same case tables and seeds): A <= 256 everywhere, statistics sums below
2^24, at least 90 % of the oracle's output elements nonzero.  The last is taken over the elements that
have a term at all: pixels of empty stride-2 parity classes, masked elements of the BatchNorm-backward
epilogue and taps that only ever meet padding are zero by construction, and must be.
"""
import pytest
import torch
import torch.nn.functional as F

import conv_oracle as O

REL = 1e-12

# N, H, W, C, K, R, S, stride, pad: strided, padded, non-square, kernel larger than the image
CONFIGS = [(2, 6, 7, 3, 5, 3, 3, 1, 1), (2, 9, 8, 4, 6, 3, 3, 2, 1), (1, 7, 9, 5, 4, 5, 3, 2, 2),
           (2, 8, 8, 4, 8, 1, 1, 2, 0), (1, 4, 4, 2, 3, 7, 7, 2, 3), (1, 6, 9, 3, 4, 3, 1, 1, 0),
           (2, 7, 7, 3, 4, 2, 2, 1, 1), (1, 10, 11, 2, 3, 4, 2, 3, 1)]


def _close(a, b):
    scale = float(b.abs().max()) or 1.0
    assert a.shape == b.shape
    assert float((a - b).abs().max()) <= REL * scale, float((a - b).abs().max()) / scale


def _torch_conv(x, w, stride, pad):
    y = F.conv2d(x.permute(0, 3, 1, 2), w.permute(0, 3, 1, 2), stride=stride, padding=pad)
    return y.permute(0, 2, 3, 1)


@pytest.mark.parametrize("cfg", CONFIGS)
@pytest.mark.parametrize("absolute", [False, True])
def test_conv_references_match_autograd(cfg, absolute):
    N, H, W, C, K, R, S, stride, pad = cfg
    torch.manual_seed(sum(cfg))
    x = torch.randn(N, H, W, C, dtype=torch.float64)
    w = torch.randn(K, R, S, C, dtype=torch.float64)
    P, Q = O.out_hw(H, W, R, S, stride, pad)
    dy = torch.randn(N, P, Q, K, dtype=torch.float64)
    res = torch.randn(N, P, Q, K, dtype=torch.float64)
    bx, bw = torch.randn_like(x), torch.randn_like(w)
    ab = (lambda t: t.abs()) if absolute else (lambda t: t)
    xr, wr = ab(x).clone().requires_grad_(), ab(w).clone().requires_grad_()
    yr = _torch_conv(xr, wr, stride, pad)
    yr.backward(ab(dy))
    _close(O.conv_fwd(x, w, stride, pad, absolute=absolute), yr.detach())
    _close(O.conv_fwd(x, w, stride, pad, res=res, absolute=absolute), yr.detach() + ab(res))
    _close(O.conv_dgrad(dy, w, x.shape, stride, pad, absolute=absolute), xr.grad)
    _close(O.conv_dgrad(dy, w, x.shape, stride, pad, base=bx, absolute=absolute), xr.grad + ab(bx))
    _close(O.conv_wgrad(dy, x, w.shape, stride, pad, absolute=absolute), wr.grad)
    _close(O.conv_wgrad(dy, x, w.shape, stride, pad, base=bw, absolute=absolute), wr.grad + ab(bw))
    # the term count: the same computation on ones
    n = O.conv_fwd(O.ones(x), O.ones(w), stride, pad)
    _close(n, _torch_conv(torch.ones_like(x), torch.ones_like(w), stride, pad))


@pytest.mark.parametrize("absolute", [False, True])
def test_statistics_and_bn_backward_epilogue(absolute):
    torch.manual_seed(3)
    C = 8
    v = torch.randn(2, 5, 6, C, dtype=torch.float64)
    aux = torch.randn(2, 5, 6, C, dtype=torch.float64)
    mean, istd = torch.randn(C, dtype=torch.float64), torch.rand(C, dtype=torch.float64) + 0.5
    bits = torch.rand(2, 5, 6, C) > 0.4
    dz = O.bnb_epilogue(v, bits)
    assert torch.equal(dz, torch.where(bits, v, torch.zeros_like(v)))
    assert O.bnb_epilogue(v, None) is v
    s0, s1 = O.bn_stats_rows(v, absolute=absolute)
    va = v.abs() if absolute else v
    _close(s0, va.reshape(-1, C).sum(0))
    _close(s1, (v * v).reshape(-1, C).sum(0))
    b0, b1 = O.bnb_sums(dz, aux, mean, istd, absolute=absolute)
    if absolute:
        _close(b0, dz.abs().reshape(-1, C).sum(0))
        _close(b1, (dz.abs() * (aux.abs() + mean.abs())).reshape(-1, C).sum(0) * istd.abs())
    else:
        xhat = ((aux - mean) * istd).reshape(-1, C)
        _close(b0, dz.reshape(-1, C).sum(0))
        _close(b1, (dz.reshape(-1, C) * xhat).sum(0))
    # the packed mask: bit i of byte b is element 8 b + i
    packed = O.pack_mask(bits)
    flat = bits.reshape(-1)
    for e in (0, 1, 7, 8, 13, flat.numel() - 1):
        assert bool((packed[e // 8] >> (e % 8)) & 1) == bool(flat[e])


@pytest.mark.parametrize("H,W", [(32, 32), (13, 37), (12, 15)])
@pytest.mark.parametrize("absolute", [False, True])
def test_stem_references(H, W, absolute):
    """The original 7x7 stride-2 stem against F.conv2d + autograd, and the space-to-depth identities the
    direct-kernel references rely on: the stride-1 4x4 conv of the transformed operands is the stem,
    and the un-space-to-depth of its weight gradient is the stem's."""
    torch.manual_seed(H + W)
    x = torch.randn(2, H, W, 3, dtype=torch.float64)
    w = torch.randn(64, 7, 7, 3, dtype=torch.float64)
    P, Q = O.out_hw(H, W, 7, 7, 2, 3)
    dy = torch.randn(2, P, Q, 64, dtype=torch.float64)
    ab = (lambda t: t.abs()) if absolute else (lambda t: t)
    wr = ab(w).clone().requires_grad_()
    yr = _torch_conv(ab(x), wr, 2, 3)
    yr.backward(ab(dy))
    _close(O.stem_fwd(x, w, absolute=absolute), yr.detach())
    _close(O.stem_wgrad(dy, x, absolute=absolute), wr.grad)
    xs, ws = O.s2d_input(x, 3), O.s2d_weight(w)
    assert ws.shape == (64, 4, 4, 16)
    ys = O.conv_fwd(xs, ws, 1, 0, absolute=absolute)
    _close(ys[:, :P, :Q], yr.detach())
    dws = O.conv_wgrad(dy, xs[:, :P + 3, :Q + 3], ws.shape, 1, 0, absolute=absolute)
    _close(O.un_s2d_weight_grad(dws, w.shape), wr.grad)


@pytest.mark.parametrize("absolute", [False, True])
def test_patch_embedding_reference(absolute):
    B, H, W, C, P, D = O.PATCH_SHAPE
    torch.manual_seed(5)
    x = torch.randn(B, H, W, C, dtype=torch.float64)
    w = torch.randn(D, P * P * C, dtype=torch.float64)
    b = torch.randn(D, dtype=torch.float64)
    dy = torch.randn(B, (H // P) * (W // P), D, dtype=torch.float64)
    ab = (lambda t: t.abs()) if absolute else (lambda t: t)
    wr, br = ab(w).clone().requires_grad_(), ab(b).clone().requires_grad_()
    t = ab(x).view(B, H // P, P, W // P, P, C).permute(0, 1, 3, 2, 4, 5).reshape(B, -1, P * P * C)
    yr = F.linear(t, wr, br)
    yr.backward(ab(dy))
    _close(O.patch_embed_fwd(x, w, b, P, absolute=absolute), yr.detach())
    dw, db = O.patch_embed_grads(dy, x, P, absolute=absolute)
    _close(dw, wr.grad)
    _close(db, br.grad)


def test_half_ulp_and_tolerance():
    vals = [0.0, 1.0, 1.5, 2.0, 3.999, 255.0, 256.0, 1e-3, 7.3e4, 2.0 ** -20]
    for dt in (torch.bfloat16, torch.float32):
        got = O.half_ulp_t(torch.tensor(vals, dtype=torch.float64), dt)
        assert got.tolist() == [O.half_ulp(v, dt) for v in vals]
    ref, A, n = torch.tensor([3.0, 0.0]), torch.tensor([5.0, 0.0]), torch.tensor([10.0, 0.0])
    a = 2 * 10 * 2.0 ** -24 * 5.0
    t = O.tol(ref, A, n, torch.bfloat16)
    assert t.tolist() == [a + O.half_ulp(3.0 + a, torch.bfloat16), 0.0]
    tb = O.tol(ref, A, n, torch.bfloat16, bf16_partials=True)
    ab_ = a + 2.0 ** -8 * 5.0
    assert tb.tolist() == [ab_ + O.half_ulp(3.0 + ab_, torch.bfloat16), 0.0]
    # an element without terms must be exactly zero; a NaN anywhere is an infinite ratio
    assert O.ratio(torch.tensor([3.0, 0.0]), ref, A, n, torch.bfloat16) == 0.0
    assert O.ratio(torch.tensor([3.0, 1e-30]), ref, A, n, torch.bfloat16) == float("inf")
    assert O.ratio(torch.tensor([float("nan"), 0.0]), ref, A, n, torch.bfloat16) == float("inf")


_EXACT = list(O.all_exact_refs())


def test_exact_cases_cover_every_family():
    labels = [lb for lb, _ in _EXACT]
    assert len(labels) == len(set(labels))
    for shape, _ in O.DIRECT_SHAPES:
        assert sum(lb.startswith(f"direct{shape}:") for lb in labels) == 8
    for case in O.IGEMM_SHAPES:
        assert sum(lb.startswith(f"igemm{case}:") for lb in labels) == (5 if case[7] > 1 else 4)
    assert sum(lb.startswith(f"igemm{O.WG_SHAPE}:") for lb in labels) == 2
    for shape, _ in O.STEM_FWD_SHAPES + O.STEM_WGRAD_SHAPES:
        assert f"stem{shape}:fwd" in labels and f"stem{shape}:wgrad_acc" in labels
    for shape in O.STEM_PATH_SHAPES:
        assert f"stem_path{shape}:wgrad" in labels
    assert "patch:db" in labels


@pytest.mark.parametrize("label,r", _EXACT, ids=[lb for lb, _ in _EXACT])
def test_exact_case_conditions(label, r):
    assert r.ref.shape == r.A.shape == r.n.shape
    assert float(r.A.max()) <= O.EXACT_A_MAX, f"{label}: max A = {float(r.A.max())}"
    assert bool((r.ref == r.ref.round()).all()), f"{label}: the oracle is not integer-valued"
    has = r.n > 0
    assert bool((r.ref[~has] == 0).all()) and bool((r.A[~has] == 0).all())
    assert float(has.double().mean()) >= 0.2, f"{label}: hardly any element has a term"
    nz = float((r.ref[has] != 0).double().mean())
    assert nz >= 0.9, f"{label}: only {nz:.3f} of the elements with a term are nonzero"
    if r.stats is not None:
        for s in r.stats[1]:
            assert float(s.max()) < O.EXACT_STAT_MAX, f"{label}: statistics sum {float(s.max())}"
        for s in r.stats[0]:
            assert bool((s * 2 == (s * 2).round()).all())      # istd in {0.5, 1, 2}: halves at the worst
