"""The elementwise oracle itself (``elementwise_oracle.py``), checked without a GPU: its fp64 run agrees
with torch's own fp64 ops where both are defined alike (tie-free inputs for top-k and max-pool), and
the inputs of every GPU case -- rebuilt here from the same generator functions and seeds -- have the
properties the GPU file relies on (ties, NaN and all ``-inf`` windows where they are meant to be,
finite oracle losses, and at most ``BAND_CAP`` undecided mask bits and windows in every BN-pool case)."""
import math

import pytest
import torch
import torch.nn.functional as F

import elementwise_oracle as EO
import test_elementwise_oracle_gpu as G

F64 = torch.float64
REL = 1e-12


def _agree(got, want, what, rel=REL):
    got, want = got.double(), want.double()
    assert got.shape == want.shape, f"{what}: {tuple(got.shape)} vs {tuple(want.shape)}"
    err, scale = float((got - want).abs().max()), float(want.abs().max())
    assert err <= rel * max(scale, 1e-300), f"{what}: {err:.3e} against {scale:.3e}"


def _r(key, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(key), dtype=F64)


# ---------------------------------------------------------------------------- references against torch
def test_gelu_tanh_refs_match_autograd():
    z = torch.cat([_r(0, 500) * 3, G.gelu_fixed(torch.float32)[0].double()]).requires_grad_(True)
    dy = _r(1, z.numel())
    y = F.gelu(z)
    y.backward(dy)
    _agree(EO.gelu_ref(z.detach(), F64), y.detach(), "gelu", 1e-10)
    _agree(EO.gelu_bwd_ref(dy, z.detach(), F64).dz, z.grad, "gelu dz", 1e-10)
    _agree(EO.gelu_grad_ref(z.detach(), F64) * dy, z.grad, "gelu grad", 1e-10)
    x = _r(2, 300).requires_grad_(True)
    t = torch.tanh(x)
    t.backward(dy[:300])
    _agree(EO.tanh_bwd_ref(dy[:300], t.detach(), F64), x.grad, "tanh_bwd")
    z2, dy2 = _r(3, 9, 16), _r(4, 9, 16)
    o = EO.gelu_bwd_ref(dy2, z2, F64, _r(5, 16), F64, True)
    _agree(o.colsum, o.dz.sum(0) + _r(5, 16), "gelu colsum")


def test_dropout_ref():
    x = _r(0, 4096)
    for p in G.DROP_PS:
        p = G._p32(p)
        o = EO.dropout_ref(x, G.SEEDS[1], p, F64)
        assert torch.equal(o.keep, EO._hash_keep(G.SEEDS[1], 4096, p))
        _agree(o.y, x * o.keep / (1 - p), f"dropout p={p}")
    assert abs(float(EO.keep_bits(x, 7, 0.5).double().mean()) - 0.5) < 0.05
    assert bool(EO.keep_bits(x, 7, 0.0).all())
    assert not torch.equal(EO.keep_bits(x, G.SEEDS[0], 0.5), EO.keep_bits(x, G.SEEDS[1], 0.5))
    assert G.SEEDS[0] & 0xFFFFFFFF == G.SEEDS[1] & 0xFFFFFFFF and G.SEEDS[1] < 2 ** 62
    assert G._p32(G.P_LAST) == G.P_LAST and int(G.P_LAST * 65536.0) == 65535


def test_colsum_and_glue_refs():
    x, out = _r(0, 33, 24), _r(1, 24)
    _agree(EO.colsum_ref(x, F64), x.sum(0), "colsum")
    _agree(EO.colsum_ref(x, F64, out, F64, True), x.sum(0) + out, "colsum acc")
    emu = EO.colsum_ref(x.float(), torch.float32, out.bfloat16(), torch.bfloat16, True)
    assert emu.dtype == torch.bfloat16
    _agree(EO.acc_ref(out, x[0], True, F64), x[0], "acc first")
    _agree(EO.acc_ref(out, x[0], False, F64), out + x[0], "acc")
    _agree(EO.acc_f32_ref(out, x[0], F64), out + x[0], "acc_f32")
    _agree(EO.rows_add_row_ref(x, out, F64), x + out, "rows_add_row")


@pytest.mark.parametrize("B,C", [(1, 1), (3, 2), (7, 257), (5, 1000)])
def test_ce_ref_matches_autograd(B, C):
    x = (_r(B + C, B, C) * 3).requires_grad_(True)
    lab = torch.randint(0, C, (B,), generator=torch.Generator().manual_seed(C))
    loss = F.cross_entropy(x, lab)
    (loss * 2.5).backward()
    o = EO.ce_ref(x.detach(), lab, 2.5, F64)
    _agree(o.loss, loss.detach(), "loss")
    _agree(o.row_loss, F.cross_entropy(x.detach(), lab, reduction="none"), "row loss")
    _agree(o.dscaled, x.grad, "dlogits")
    _agree(o.dlogits * 2.5, x.grad, "unscaled dlogits")


@pytest.mark.parametrize("B,C,k", G.TOPK_CASES)
def test_topk_ref_matches_torch(B, C, k):
    x = _r(C, B, C) * 3                                   # tie-free
    o = EO.topk_ref(x, k, F64)
    p = torch.softmax(x, -1)
    v, i = torch.topk(p, k, dim=-1)
    _agree(o.probs, p, "probs")
    assert torch.equal(o.indices, i)
    _agree(o.values, v, "values")
    # the documented rule on ties: by value, then by lower index
    t = EO.topk_ref(torch.tensor([[1.0, 3.0, 3.0, -math.inf, 3.0, 2.0]], dtype=F64), 5, F64)
    assert t.indices.tolist() == [[1, 2, 4, 5, 0]]


def _torch_pool(x, K, S, pad, dy):
    xr = x.clone().requires_grad_(True)
    y, flat = F.max_pool2d(xr.permute(0, 3, 1, 2), K, S, pad, return_indices=True)
    y.backward(dy.permute(0, 3, 1, 2))
    N, H, W, C = x.shape
    P, Q = y.shape[2:]
    h, w = flat // W, flat % W                               # [N, C, P, Q]
    p0 = (torch.arange(P) * S - pad).view(1, 1, P, 1)
    q0 = (torch.arange(Q) * S - pad).view(1, 1, 1, Q)
    tap = (h - p0) * K + (w - q0)
    return y.detach().permute(0, 2, 3, 1), tap.permute(0, 2, 3, 1), xr.grad


@pytest.mark.parametrize("shape", G.POOL_SHAPES, ids=str)
@pytest.mark.parametrize("K,S,pad", G.POOL_KSP)
def test_maxpool_ref_matches_torch(shape, K, S, pad):
    N, H, W, C = shape
    x = _r(K + C, N, H, W, C)                              # tie-free
    x[N - 1, :2, :2, :] = -math.inf                        # torch routes an all -inf window's gradient to
    P, Q = EO.pool_shape(H, W, K, S, pad)                  # its first in-bounds tap: the rule of the oracle
    dy = _r(1, N, P, Q, C)
    o = EO.maxpool_ref(x, K, S, pad, dy, F64)
    y, tap, dx = _torch_pool(x, K, S, pad, dy)
    assert torch.equal(o.y, y)
    assert torch.equal(o.idx, tap)
    _agree(o.dx, dx, "dx")
    if pad and K == 3:                                     # the corner window's in-bounds taps: all -inf
        assert int(o.idx[N - 1, 0, 0, 0]) == pad * K + pad and float(dx[N - 1, 1, 1, 0]) == 0
        assert float((dx[N - 1, 0, 0] - dy[N - 1, 0, 0]).abs().max()) == 0


def test_maxpool_ref_tie_and_nan_rules():
    x = torch.zeros(1, 3, 3, 8, dtype=F64)
    o = EO.maxpool_ref(x, 3, 1, 1, torch.ones(1, 3, 3, 8, dtype=F64), F64)
    assert o.idx[0, :, :, 0].tolist() == [[4, 3, 3], [1, 0, 0], [1, 0, 0]]       # the first in-bounds tap
    x[0, 1, 1, 0], x[0, 2, 2, 0] = math.nan, math.nan
    o = EO.maxpool_ref(x, 3, 1, 1, torch.ones(1, 3, 3, 8, dtype=F64), F64)
    assert int(o.idx[0, 1, 1, 0]) == 8 and math.isnan(float(o.y[0, 1, 1, 0]))     # the last NaN tap
    assert int(o.idx[0, 0, 0, 0]) == 8 and int(o.idx[0, 0, 0, 1]) == 4 and int(o.idx[0, 1, 1, 1]) == 0


@pytest.mark.parametrize("shape", G.BNPOOL_SHAPES, ids=str)
def test_bn_relu_maxpool_ref_matches_torch(shape):
    x, scale, shift = (t.double() for t in G.bnpool_inputs(torch.float32, shape))
    shift = shift + 2.0                                    # half the activations positive: tie-free maxima
    o = EO.bn_relu_maxpool_ref(x, scale, shift, F64)
    a = torch.relu(x * scale + shift)
    _agree(o.y, F.max_pool2d(a.permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1), "y")
    _agree(o.best, o.y, "best")
    assert torch.equal(o.mask, a > 0)
    assert torch.equal(EO.unpack_mask(EO.pack_mask(o.mask), o.mask.shape), o.mask)
    assert EO.pack_mask(torch.tensor([True] + [False] * 6 + [True] * 2 + [False] * 7)).tolist() == [129, 1]
    _agree(o.win.gather(0, o.idx.unsqueeze(0)).squeeze(0), o.y, "value at the recorded tap")
    assert bool((o.second <= o.best).all())


@pytest.mark.parametrize("N,HW,C", G.AVG_SHAPES)
def test_avgpool_ref_matches_autograd(N, HW, C):
    x, dy = (t.double() for t in G.avgpool_inputs(torch.float32, N, HW, C))
    xr = x.clone().requires_grad_(True)
    y = xr.mean(dim=(1, 2))
    y.backward(dy)
    o = EO.avgpool_ref(x, dy, F64)
    _agree(o.y, y.detach(), "y")
    _agree(o.dx, xr.grad, "dx")


@pytest.mark.parametrize("kind,V,D,lead", G.EMB_CASES)
def test_embedding_ref_matches_autograd(kind, V, D, lead):
    ids, w, dy, sink = G.embedding_inputs(torch.float32, kind, V, D, lead)
    w, dy, sink = w.double(), dy.double(), sink.double()
    wr = w.clone().requires_grad_(True)
    y = F.embedding(ids, wr)
    y.backward(dy)
    o = EO.embedding_ref(ids, w, dy, F64, sink)
    assert torch.equal(o.y, y.detach())
    _agree(o.dw, wr.grad + sink, "dw + sink")
    _agree(EO.embedding_ref(ids, w, dy, F64).dw, wr.grad, "dw")
    assert D % 8 == 0 and (D == 8 or D % 64)
    if kind == "same":
        assert ids.unique().numel() == 1
    if kind == "ends":
        assert int(ids.min()) == 0 and int(ids.max()) == V - 1


def test_shrink():
    ref = torch.tensor([1.0, 1.0, 1.0], dtype=F64)
    got = torch.tensor([1.5, 0.9, 1.01], dtype=F64)
    _agree(EO.shrink(got, ref, torch.tensor([0.2, 0.2, 0.2], dtype=F64)), torch.tensor([1.3, 1.0, 1.0], dtype=F64), "s")


# ---------------------------------------------------------------------------- the GPU cases' inputs
@pytest.mark.parametrize("dtype", G.DTYPES, ids=G._name)
def test_flat_inputs(dtype):
    assert G.BIG_N // 8 > 8192 * 256 and (G.BIG_N - 2056) // 8 == 8192 * 256 and G.BIG_N % 8 == 0
    assert G.BIG_N // 8 > 4096 * 256                       # ddl_acc_grad / ddl_drain_acc: grid of 4096
    z, dy, y, acc, n_fix = G.flat_inputs(dtype, 2056)
    assert n_fix == 22 and z.dtype == dtype
    fi = torch.finfo(dtype)
    assert z[-2].item() == fi.max and z[-1].item() == -fi.max
    fixed = set(z[-n_fix:-2].double().abs().tolist())
    assert {0.0, float(fi.tiny), 0.5, 1.0, 3.0, 5.0, 8.0, 13.0, 40.0} <= fixed and len(fixed) == 10
    assert bool(torch.signbit(z[-n_fix + 1])) and z[-n_fix + 1] == 0          # -0
    assert float(y.float().abs().max()) <= 1.0
    assert G.flat_inputs(dtype, 8)[4] == 0
    # the oracle at the fixed vector: finite, slopes 1 and 0 at the two large ends
    g = EO.gelu_grad_ref(z, F64)
    assert bool(torch.isfinite(g).all()) and g[-2].item() == 1.0 and g[-1].item() == 0.0
    r = EO.gelu_ref(z, F64)
    assert r[-2].item() == fi.max and r[-1].item() == 0.0


def test_colsum_inputs():
    rows, C = G.COLSUM_SHAPES[-1]
    nblk = max(1, min(1024, (rows + 15) // 16))
    rpb = -(-rows // nblk)
    assert nblk == 1024 and (nblk - 1) * rpb >= rows and C // 8 > 256        # empty trailing blocks, blockIdx.y = 1
    x, z, dy, old = G.colsum_inputs(torch.float32, 17, 72)
    assert abs(float(x.mean(0)[71] - x.mean(0)[0]) - 0.71) < 1.0 and x.shape == (17, 72)


@pytest.mark.parametrize("dtype", G.DTYPES, ids=G._name)
@pytest.mark.parametrize("B", G.CE_BS)
def test_ce_inputs(dtype, B):
    assert any(c > 256 for c in G.CE_CS) and B in (1, 3, 300) and max(G.CE_BS) > 256
    for C in G.CE_CS:
        seen_inf = seen_spread = False
        for special in (("spread", "ninf") if B == 1 else ("both",)):
            x, lab = G.ce_inputs(dtype, B, C, special)
            assert x.dtype == dtype and int(lab[0]) == 0 and (B == 1 or int(lab[1]) == C - 1)
            S = 80.0 if dtype == torch.bfloat16 else 1e4
            seen_spread |= bool((x.float().abs().max(-1).values >= S * 0.99).any())
            ninf = torch.isinf(x.float()).sum(-1)
            seen_inf |= bool((ninf == C - 2).any())
            assert bool(((ninf == 0) | (ninf == C - 2)).all())
            assert not bool(torch.isinf(x.float().gather(1, lab.view(-1, 1))).any())
            for up in G.CE_UPSTREAM:
                o = EO.ce_ref(x, lab, up, F64)
                assert bool(torch.isfinite(o.loss)) and bool(torch.isfinite(o.dscaled).all())
        assert seen_spread and (seen_inf or C <= 2)


@pytest.mark.parametrize("dtype", G.DTYPES, ids=G._name)
@pytest.mark.parametrize("B,C,k", G.TOPK_CASES)
def test_topk_inputs(dtype, B, C, k):
    x = G.topk_inputs(dtype, B, C, k)
    assert torch.equal(x.bfloat16().to(dtype), x)          # bf16 values in either dtype
    finite = x[torch.isfinite(x.float())].double()
    assert finite.unique().numel() <= 64
    d = finite.unique().diff()
    assert d.numel() == 0 or float(d.min()) >= 0.125       # distinct logits: distinct fp32 probabilities
    if C >= 4:
        o = EO.topk_ref(x, k, F64)
        for b in range(B):                                 # ties inside the top k of every row
            assert x[b, o.indices[b]].double().unique().numel() < k
        assert bool(torch.isinf(x[B - 1].float()).any())


@pytest.mark.parametrize("dtype", G.DTYPES, ids=G._name)
@pytest.mark.parametrize("shape", G.POOL_SHAPES, ids=str)
@pytest.mark.parametrize("K,S,pad", G.POOL_KSP)
def test_maxpool_inputs(dtype, shape, K, S, pad):
    N, H, W, C = shape
    assert (N * H) % 8 and C % 8 == 0
    x, dy = G.maxpool_inputs(dtype, shape, K, S, pad)
    o = EO.maxpool_ref(x, K, S, pad, dy, F64)
    assert bool(torch.isnan(o.y.float()).any()) and bool(torch.isfinite(o.dx).all())
    if (K, S, pad) != (5, 3, 2):                           # the corner window's in-bounds taps: all -inf
        assert bool(torch.isinf(o.y[N - 1, 0, 0].float()).all())
        assert int(o.idx[N - 1, 0, 0, 0]) == pad * K + pad
    # natural ties: some window holds its maximum twice
    win = torch.stack([torch.where(valid, v, torch.full((), -math.inf, dtype=F64))
                       for _, v, valid, _, _ in EO._taps(x.double(), K, S, pad)])
    top2 = torch.sort(win, dim=0, descending=True).values[:2]
    assert bool(((top2[0] == top2[1]) & torch.isfinite(top2[0])).any())


@pytest.mark.parametrize("dtype", G.DTYPES, ids=G._name)
@pytest.mark.parametrize("shape", G.BNPOOL_SHAPES, ids=str)
def test_bnpool_band_cap(dtype, shape):
    """At most BAND_CAP of a case's mask bits and of its windows are left to the kernel's rounding."""
    x, scale, shift = G.bnpool_inputs(dtype, shape)
    assert shape[1] % 2 == 0 and shape[2] % 2 == 0 and shape[3] % 8 == 0
    r64, e32 = EO.bn_relu_maxpool_ref(x, scale, shift, F64), EO.bn_relu_maxpool_ref(x, scale, shift, torch.float32)
    t, bit_decided, win_decided = G.bnpool_bands(r64, e32, dtype)
    bits, wins = 1 - float(bit_decided.double().mean()), 1 - float(win_decided.double().mean())
    print(f"BAND {G._name(dtype)} {shape} t={t:.3e} mask {bits:.4f} windows {wins:.4f} "
          f"positive {float(r64.mask.double().mean()):.3f}")
    assert bits <= G.BAND_CAP and wins <= G.BAND_CAP
    assert bool(r64.mask.any()) and bool((r64.best > 0).any())
