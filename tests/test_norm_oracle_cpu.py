"""The normalisation oracle itself (``norm_oracle.py``), checked without a GPU: its fp64 run agrees
with autograd through ``torch.nn.functional``, its fp32 emulation is a yardstick that is neither
degenerate nor loose, and no BatchNorm case of the GPU file hides more than ``BAND_CAP`` of its
elements in the ReLU band."""
import pytest
import torch
import torch.nn.functional as F

import norm_oracle as NO
import test_norm_oracle_gpu as G

F64 = torch.float64
REL = 1e-12


def _agree(got, want, what):
    got, want = got.double(), want.double()
    assert got.shape == want.shape, f"{what}: {tuple(got.shape)} vs {tuple(want.shape)}"
    err, scale = float((got - want).abs().max()), float(want.abs().max())
    assert err <= REL * max(scale, 1e-300), f"{what}: {err:.3e} against {scale:.3e}"


def _ln_case(res, drop, add, dtype=F64, lead=(3, 5), H=64, key=0):
    gen = torch.Generator().manual_seed(key)
    mk = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float32).to(dtype)  # noqa: E731
    x, dy = mk(*lead, H), mk(*lead, H)
    g = (torch.rand(H, generator=gen) + 0.5).to(dtype)
    b = (torch.randn(H, generator=gen) * 0.3).to(dtype)
    r = {None: None, "full": mk(*lead, H), "bcast": mk(1, *lead[1:], H)}[res]
    keep = (torch.rand(*lead, H, generator=gen) >= 0.1) if drop else None
    a = mk(*lead, H) if add else None
    return x, g, b, r, keep, dy, a


@pytest.mark.parametrize("res", [None, "full", "bcast"])
@pytest.mark.parametrize("drop", [False, True])
@pytest.mark.parametrize("add", [False, True])
def test_ln_ref_matches_autograd(res, drop, add):
    x, g, b, r, keep, dy, a = _ln_case(res, drop, add)
    p, eps = 0.1, 1e-5
    o = NO.ln_ref(x, g, b, eps, r, keep, p if drop else 0.0, dy, a, F64)
    lx, lg, lb = (t.clone().requires_grad_(True) for t in (x, g, b))
    lr = None if r is None else r.clone().requires_grad_(True)
    xd = lx * keep.double() / (1 - p) if drop else lx
    h = xd if lr is None else xd + lr
    h.retain_grad()
    y = F.layer_norm(h, (h.shape[-1],), lg, lb, eps)
    y.backward(dy)
    dx = lx.grad if a is None else lx.grad + a
    _agree(o.y, y.detach(), "y")
    _agree(o.mean, h.detach().mean(-1).reshape(-1), "mean")
    _agree(o.rstd, (h.detach().var(-1, unbiased=False) + eps).rsqrt().reshape(-1), "rstd")
    _agree(o.dx, dx, "dx")
    _agree(o.dgamma, lg.grad, "dgamma")
    _agree(o.dbeta, lb.grad, "dbeta")
    _agree(o.dgamma_raw, lg.grad, "dgamma_raw")
    _agree(o.dxsum, dx.reshape(-1, dx.shape[-1]).sum(0), "dxsum")
    if r is None:
        assert o.dres is None
    else:
        _agree(o.dres, lr.grad, "dres")
        if drop and res == "full":        # the residual's gradient is not masked, the input's is
            assert bool(o.dres[~keep].ne(0).any())
            assert add or not bool(o.dx[~keep].ne(0).any())


@pytest.mark.parametrize("relu,res", G.BN_VARIANTS)
@pytest.mark.parametrize("shape", [(1, 1, 3), (2, 3, 5)])   # (two rows: dx cancels to ~eps, no relative figure)
def test_bn_ref_matches_autograd(relu, res, shape):
    gen = torch.Generator().manual_seed(1)
    C, eps = 16, 1e-5
    x = torch.randn(*shape, C, generator=gen, dtype=F64) * 2 + 0.5
    dy = torch.randn(*shape, C, generator=gen, dtype=F64)
    g = torch.rand(C, generator=gen, dtype=F64) + 0.5
    b = torch.randn(C, generator=gen, dtype=F64) * 0.3
    r = torch.randn(*shape, C, generator=gen, dtype=F64) if res else None
    o = NO.bn_ref(x, g, b, eps, relu, r, dy, F64)
    lx, lg, lb = (t.clone().requires_grad_(True) for t in (x, g, b))
    lr = None if r is None else r.clone().requires_grad_(True)
    rm, rv = torch.zeros(C, dtype=F64), torch.ones(C, dtype=F64)
    z = F.batch_norm(lx.reshape(-1, C), rm, rv, lg, lb, True, 0.1, eps).view_as(lx)
    if lr is not None:
        z = z + lr
    y = torch.relu(z) if relu else z
    y.backward(dy)
    _agree(o.y, y.detach(), "y")
    _agree(o.z, z.detach(), "z")
    _agree(o.mean, x.reshape(-1, C).mean(0), "mean")
    _agree(o.var, x.reshape(-1, C).var(0, unbiased=False), "var")
    _agree(o.dx, lx.grad, "dx")
    _agree(o.dgamma, lg.grad, "dgamma")
    _agree(o.dbeta, lb.grad, "dbeta")
    if res:
        _agree(o.dres, lr.grad, "dres")
    else:
        assert o.dres is None
    orm, orv = NO.bn_running(o.mean, o.var_unbiased, 0.1, F64)
    m32 = float(torch.tensor(0.1, dtype=torch.float32))      # the kernels take a float momentum
    rm2, rv2 = torch.zeros(C, dtype=F64), torch.ones(C, dtype=F64)
    F.batch_norm(x.reshape(-1, C), rm2, rv2, None, None, True, m32, eps)
    _agree(orm, rm2, "running_mean")
    _agree(orv, rv2, "running_var")
    # an explicit mask replaces the reference's own
    mask = torch.rand(*shape, C, generator=gen) > 0.5
    om = NO.bn_ref(x, g, b, eps, mask, r, dy, F64)
    z.grad = None
    lx.grad = lg.grad = lb.grad = None
    z2 = F.batch_norm(lx.reshape(-1, C), rm, rv, lg, lb, True, 0.1, eps).view_as(lx)
    z2.backward(dy * mask)
    _agree(om.dx, lx.grad, "dx under a given mask")
    _agree(om.dgamma, lg.grad, "dgamma under a given mask")


@pytest.mark.parametrize("relu,res", G.BN_VARIANTS)
def test_bn_eval_ref_matches_functional(relu, res):
    gen = torch.Generator().manual_seed(2)
    C, eps = 16, 1e-5
    x = torch.randn(4, 3, 3, C, generator=gen, dtype=F64)
    g = torch.rand(C, generator=gen, dtype=F64) + 0.5
    b = torch.randn(C, generator=gen, dtype=F64) * 0.3
    rm = torch.randn(C, generator=gen, dtype=F64)
    rv = torch.rand(C, generator=gen, dtype=F64) + 0.5
    rv[0] = 1e-5
    r = torch.randn(4, 3, 3, C, generator=gen, dtype=F64) if res else None
    o = NO.bn_eval_ref(x, g, b, rm, rv, eps, relu, r, F64)
    z = F.batch_norm(x.reshape(-1, C), rm.clone(), rv.clone(), g, b, False, 0.1, eps).view_as(x)
    if r is not None:
        z = z + r
    _agree(o.z, z, "z")
    _agree(o.y, torch.relu(z) if relu else z, "y")


def _ulps(em, ref, dtype):
    """max |em - ref| in units of the spacing of ``dtype`` at the largest reference value (the unit of
    ``bound``'s ulp term: y near zero carries the absolute error of its row's statistics)."""
    ref = ref.double()
    return float((em.double() - ref).abs().max()) / (2 * NO.half_ulp(float(ref.abs().max()), dtype))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_emulation_is_a_yardstick(dtype):
    """On y the emulation differs from the oracle, and by less than 2 ulp of its dtype."""
    x, g, b, r, keep, dy, a = _ln_case("full", True, True, dtype=dtype, lead=(3, 7), H=256, key=3)
    ref, em = (NO.ln_ref(x, g, b, 1e-5, r, keep, 0.1, dy, a, dt) for dt in (F64, torch.float32))
    assert em.y.dtype == dtype and em.dx.dtype == dtype and em.mean.dtype == torch.float32
    worst = _ulps(em.y, ref.y, dtype)
    assert 0.0 < worst < 2.0, worst
    C = 16
    case = (C, (4, 7, 9), True, True, 0.0, 0, 1.0)
    bx, bg, bb, br, bdy = (t if t is None or dtype == torch.bfloat16 else t.float() for t in G.bn_inputs(case, "cpu"))
    ref, em = (NO.bn_ref(bx, bg, bb, 1e-5, False, br, bdy, dt) for dt in (F64, torch.float32))
    assert em.y.dtype == dtype
    worst = _ulps(em.y, ref.y, dtype)
    assert 0.0 < worst < 2.0, worst


def test_half_ulp():
    assert NO.half_ulp(1.0, torch.bfloat16) == 2.0 ** -8
    assert NO.half_ulp(7.9, torch.bfloat16) == 2.0 ** -6
    assert NO.half_ulp(1.0, torch.float32) == 2.0 ** -24
    assert NO.half_ulp(0.0, torch.float32) == 0.0
    one = torch.tensor(1.0, dtype=torch.float32)
    assert 2 * NO.half_ulp(1.0, torch.float32) == float(torch.nextafter(one, one + 1) - one)


def test_bound_rejects_and_accepts():
    ref = torch.linspace(-4, 4, 1024, dtype=F64)
    em = ref.to(torch.bfloat16)
    NO.bound(em, ref, em, torch.bfloat16, 2.0, "emulation itself")
    off = (ref + 0.1).to(torch.bfloat16)
    with pytest.raises(AssertionError):
        NO.bound(off, ref, em, torch.bfloat16, 2.0, "shifted by 0.1")
    fails = []
    NO.bound(off, ref, em, torch.bfloat16, 2.0, "shifted by 0.1", fails)
    assert len(fails) == 2


@pytest.mark.parametrize("case", [c for c in G.BN_TRAIN_CASES + G.BN_OFFSET_CASES if c[2]], ids=G._bn_id)
def test_relu_band_stays_under_its_cap(case):
    """On the oracle alone: the band |z| <= t of a GPU case hides at most BAND_CAP of its elements."""
    x, g, b, r, dy = G.bn_inputs(case, "cpu")
    _, _, t, inside, share = G.bn_band(case, x, g, b, r, dy)
    print(f"BAND {G._bn_id(case)} t={t:.4e} share={share:.4f}")
    assert t > 0
    assert share <= G.BAND_CAP, f"{share:.4f} of the elements lie within {t:.3e} of zero"


def test_bn_case_table():
    """The GPU file's shapes do what their comments say."""
    for C, shape in G.BN_ODD_SHAPE.items():
        rows, per_iter = shape[0] * shape[1] * shape[2], 256 // (C // 8)
        assert rows > 8 * per_iter, (C, rows)                    # more than one statistics block
        assert per_iter == 1 or rows % per_iter, (C, rows)
    big = [c for c in G.BN_OFFSET_CASES if c[0] == 64 and c[1][0] * c[1][1] * c[1][2] >= 100_000]
    assert big and all(c[4] == 8.0 and not c[2] for c in G.BN_OFFSET_CASES)
