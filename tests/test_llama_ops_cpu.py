"""RMSNorm, RoPE + GQA pack and SwiGLU on the CPU: the ``ops.*_reference`` functions against the fp64 oracle
of ``llama_oracle.py``, their autograd against finite differences, the rotation's invariants, the grouped-
query head mapping, the rotary table and the dispatch of CPU tensors.

Tolerances: fp32 references against the fp64 oracle, ``atol = rtol = 1e-5`` -- sums of at most 960 fp32
products (relative 960 * 2^-24 = 6e-5 in the worst case, sqrt of that typically) on O(1) values; the rotation
and SwiGLU are a handful of fp32 operations per element (a few 2^-24).
"""
import math

import pytest
import torch

import llama_oracle as LO
from databricks_distributed_deep_learning_amd import ops
from databricks_distributed_deep_learning_amd.ops import llama as L
from databricks_distributed_deep_learning_amd.ops.bridge import GradBridge

F64 = torch.float64
TOL = dict(atol=1e-5, rtol=1e-5)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# ------------------------------------------------------------------ references against the oracle
@pytest.mark.parametrize("H", [64, 576, 960])
def test_rms_norm_reference_matches_oracle(H):
    g = _gen(H)
    x = torch.randn(3, 5, H, generator=g)
    w = torch.rand(H, generator=g) + 0.5
    dy = torch.randn(3, 5, H, generator=g)
    add = torch.randn(3, 5, H, generator=g)
    ref = LO.rms_ref(x, w, 1e-5, dy, add, F64)
    xp, wp = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    bridge = GradBridge()
    y = ops.rms_norm(xp, wp, 1e-5, grad_from=bridge)       # CPU: the reference, the bridge joined
    assert torch.equal(y, L.rms_norm_reference(x, w, 1e-5))
    bridge.put(add.clone())
    y.backward(dy)
    torch.testing.assert_close(y.double(), ref.y, **TOL)
    torch.testing.assert_close(xp.grad.double(), ref.dx, **TOL)
    torch.testing.assert_close(wp.grad.double(), ref.dw, atol=1e-4, rtol=1e-5)   # 15-row sums of O(1) terms
    # without the bridge: the same gradient less `add`
    xq = x.clone().requires_grad_(True)
    ops.rms_norm(xq, w, 1e-5).backward(dy)
    torch.testing.assert_close(xq.grad.double(), LO.rms_ref(x, w, 1e-5, dy, None, F64).dx, **TOL)


@pytest.mark.parametrize("H,Hkv", [(2, 2), (2, 1), (3, 1), (9, 3)])
def test_rope_qkv_reference_matches_oracle(H, Hkv):
    B, S = 2, 7
    g = _gen(10 * H + Hkv)
    qkv = torch.randn(B, S, (H + 2 * Hkv) * 64, generator=g)
    dout = torch.randn(B, S, 3 * H * 64, generator=g)
    table = ops.rope_table(16, 1e4)
    ref = LO.rope_ref(qkv, table, H, Hkv, dout, F64)
    qp = qkv.clone().requires_grad_(True)
    out = ops.rope_qkv(qp, table, H, Hkv)
    assert torch.equal(out, L.rope_qkv_reference(qkv, table, H, Hkv))
    out.backward(dout)
    torch.testing.assert_close(out.double(), ref.out, **TOL)
    torch.testing.assert_close(qp.grad.double(), ref.din, **TOL)


@pytest.mark.parametrize("I", [8, 352])
def test_swiglu_reference_matches_oracle(I):
    g = _gen(I)
    gu = torch.randn(5, 2 * I, generator=g)
    gu[:, :I] *= 4
    dz = torch.randn(5, I, generator=g)
    ref = LO.swiglu_ref(gu, dz, F64)
    gp = gu.clone().requires_grad_(True)
    z = ops.swiglu(gp)
    assert torch.equal(z, L.swiglu_reference(gu))
    z.backward(dz)
    torch.testing.assert_close(z.double(), ref.z, **TOL)
    torch.testing.assert_close(gp.grad.double(), ref.dgu, **TOL)


def test_swiglu_reference_finite_at_the_ends_of_the_range():
    gu = torch.tensor([[80.0, -80.0, 3e38, -3e38, 0.5, 0.5, 0.5, 0.5]], requires_grad=True)
    z = L.swiglu_reference(gu)
    z.backward(torch.full_like(z, 0.5))
    assert torch.isfinite(z).all() and torch.isfinite(gu.grad).all()


# ------------------------------------------------------------------ gradcheck
def test_references_gradcheck_fp64():
    g = _gen(0)
    x = torch.randn(3, 16, dtype=F64, generator=g, requires_grad=True)
    w = (torch.rand(16, dtype=F64, generator=g) + 0.5).requires_grad_(True)
    assert torch.autograd.gradcheck(lambda a, b: L.rms_norm_reference(a, b, 1e-5), (x, w))
    table = ops.rope_table(8, 1e4, head_dim=8).double()
    qkv = torch.randn(2, 3, (4 + 2 * 2) * 8, dtype=F64, generator=g, requires_grad=True)
    assert torch.autograd.gradcheck(lambda a: L.rope_qkv_reference(a, table, 4, 2), (qkv,))
    gu = torch.randn(3, 12, dtype=F64, generator=g, requires_grad=True)
    assert torch.autograd.gradcheck(L.swiglu_reference, (gu,))


# ------------------------------------------------------------------ rotation invariants, head mapping
@pytest.mark.parametrize("G", [1, 2, 3])
def test_rope_norms_position_zero_and_gqa_mapping(G):
    Hkv, B, S = 2, 2, 9
    H = Hkv * G
    g = _gen(G)
    qkv = torch.randn(B, S, (H + 2 * Hkv) * 64, generator=g)
    table = ops.rope_table(S, 1e4)
    out = ops.rope_qkv(qkv, table, H, Hkv).view(B, S, 3, H, 64)
    x = qkv.view(B, S, H + 2 * Hkv, 64)
    # a rotation: every head keeps its norm
    torch.testing.assert_close(out[:, :, 0].norm(dim=-1), x[:, :, :H].norm(dim=-1), **TOL)
    # position 0 is the identity, exactly (cos 1, sin 0)
    assert torch.equal(out[:, 0, 0], x[:, 0, :H])
    # later positions are not
    assert not torch.allclose(out[:, 1:, 0], x[:, 1:, :H], atol=1e-2)
    for kv in range(Hkv):
        for r in range(G):
            assert torch.equal(out[:, :, 2, kv * G + r], x[:, :, H + Hkv + kv])          # v: a copy
            assert torch.equal(out[:, :, 1, kv * G + r], out[:, :, 1, kv * G])            # k: one rotation, G slots
        torch.testing.assert_close(out[:, :, 1, kv * G].norm(dim=-1), x[:, :, H + kv].norm(dim=-1), **TOL)
        assert torch.equal(out[:, 0, 1, kv * G], x[:, 0, H + kv])
    # the backward sums each group's slots: a gradient of ones on v slots gives G per v element, and a
    # gradient on ONE slot reaches only its own group's head
    qp = qkv.clone().requires_grad_(True)
    o = ops.rope_qkv(qp, table, H, Hkv).view(B, S, 3, H, 64)
    o[:, :, 2].sum().backward()
    gr = qp.grad.view(B, S, H + 2 * Hkv, 64)
    assert torch.equal(gr[:, :, H + Hkv:], torch.full_like(gr[:, :, H + Hkv:], float(G)))
    assert not gr[:, :, :H + Hkv].any()
    qp.grad = None
    slot = H - 1                                             # the last slot: group Hkv - 1
    d = torch.randn(B, S, 64, generator=g)
    o = ops.rope_qkv(qp, table, H, Hkv).view(B, S, 3, H, 64)
    (o[:, :, 1, slot] * d).sum().backward()
    gr = qp.grad.view(B, S, H + 2 * Hkv, 64)
    assert gr[:, :, H + Hkv - 1].abs().sum() > 0
    gr[:, :, H + Hkv - 1] = 0
    assert not gr.any()


def test_rope_half_split_convention():
    """out[i] = x[i] cos_i - x[i+32] sin_i, out[i+32] = x[i+32] cos_i + x[i] sin_i, written out by index"""
    table = ops.rope_table(4, 1e4)
    x = torch.randn(1, 4, 3 * 64, generator=_gen(5))
    out = ops.rope_qkv(x, table, 1, 1).view(4, 3, 64)
    xv = x.view(4, 3, 64)
    for s in (1, 3):
        for i in (0, 7, 31):
            c, sn = table[s, i], table[s, 32 + i]
            for part in (0, 1):
                assert out[s, part, i].item() == pytest.approx((xv[s, part, i] * c - xv[s, part, i + 32] * sn).item(),
                                                               abs=1e-6)
                assert out[s, part, i + 32].item() == pytest.approx(
                    (xv[s, part, i + 32] * c + xv[s, part, i] * sn).item(), abs=1e-6)


# ------------------------------------------------------------------ the table
@pytest.mark.parametrize("theta", [1e4, 5e5])
def test_rope_table_against_fp64(theta):
    n = 2048
    t = ops.rope_table(n, theta)
    assert t.shape == (n, 64) and t.dtype == torch.float32
    want = LO.table_ref(n, theta)
    # the angle is one fp32 product (half an ulp of the angle, at most 2^-24 * 2048 rounded up to its
    # binade: 2^-13 at the largest angles), sin / cos are 1-Lipschitz and then rounded to fp32 themselves
    inv = (1.0 / (theta ** (torch.arange(0, 64, 2).float() / 64))).double()
    ang = torch.arange(n, dtype=F64)[:, None] * inv[None, :]
    tol = torch.where(ang > 0, 2.0 ** (torch.floor(torch.log2(ang.clamp_min(1e-30))) - 24), torch.zeros_like(ang))
    tol = torch.cat([tol, tol], 1) + 2e-7
    assert bool(((t.double() - want).abs() <= tol).all())
    assert torch.equal(t[0], torch.cat([torch.ones(32), torch.zeros(32)]))
    # and the frequencies: theta^(-2i/64)
    assert t[1, 31].item() == pytest.approx(math.cos(theta ** (-62 / 64)), abs=1e-6)


def test_rope_qkv_raises_past_the_table():
    table = ops.rope_table(8, 1e4)
    qkv = torch.randn(1, 9, 3 * 64)
    with pytest.raises(ValueError, match="exceeds the rotary table"):
        ops.rope_qkv(qkv, table, 1, 1)
    with pytest.raises(ValueError, match="exceeds the rotary table"):
        L.rope_qkv_reference(qkv, table, 1, 1)
    assert ops.rope_qkv(qkv[:, :8], table, 1, 1).shape == (1, 8, 3 * 64)
    with pytest.raises(ValueError):
        ops.rope_qkv(qkv[:, :8], table, 3, 2)


# ------------------------------------------------------------------ dispatch
def test_cpu_tensors_route_to_the_references(monkeypatch):
    from databricks_distributed_deep_learning_amd.ops import _lib

    def boom(*a, **k):
        raise AssertionError("the native library was asked for on CPU tensors")
    monkeypatch.setattr(_lib, "load", boom)
    x, w = torch.randn(4, 64).bfloat16(), torch.ones(64).bfloat16()
    assert torch.equal(ops.rms_norm(x, w, 1e-5), L.rms_norm_reference(x, w, 1e-5))
    table = ops.rope_table(4, 1e4)
    qkv = torch.randn(1, 4, 4 * 64).bfloat16()
    assert torch.equal(ops.rope_qkv(qkv, table, 2, 1), L.rope_qkv_reference(qkv, table, 2, 1))
    gu = torch.randn(4, 16).bfloat16()
    assert torch.equal(ops.swiglu(gu), L.swiglu_reference(gu))
    assert ops.swiglu(gu).dtype == torch.bfloat16 and ops.rope_qkv(qkv, table, 2, 1).dtype == torch.bfloat16
