"""Causal fused attention (GPU only): the tiled kernels' CAUSAL instances, which every sequence length
takes (ddl_attn_causal_fwd / ddl_attn_causal_bwd), against an fp64 reference with the same mask.

References and tolerance are those of test_attention_edges_gpu.py (`check`, M = 2, M_LSE = 2): the
local `ref64_causal` / `emu_causal` are its `ref64` / `emu` with -inf added above the diagonal.  The
emulation applies the same mask, so the margin over its error carries over unchanged.

Lengths: one either side of the 64-key tile and of the 128-query forward workgroup, odd lengths, and
513 (9 diagonal tiles).  Cases: parity on random inputs (mask x dropout), routing (a dropped key or
an off-by-one on the diagonal moves the output by O(1)), prefix invariance (no future key leaks:
exact equality, no oracle), the bias-gradient column sums, repeatability, and causal=False unchanged.

Measured on an MI355X (113 cases, all passing): with the ulp term subtracted the largest ratios are 1.35
(max form; dQ, S = 129, no mask, p = 0.25) and 1.00 (rms form; dQ / dK at S = 1); dK reaches 1.00, out 0.61,
dV 0.38; as plain kernel error / emulation error the largest are 2.23 (dQ, the same case), 1.95 (out), 1.38
(dK) and 1.00 (dV).  The log-sum-exp reaches 1.29 (max; S = 191, suffix mask) and 1.03 (rms) of torch's fp32
error.  At S = 1 the "suffix" mask of `random_inputs` hides the only key, so that row's log-sum-exp is
score - 10000, where one fp32 rounding is up to 4.9e-4: the causal forward keeps its running max in natural
units for that reason and measures 1.00 there (with the mask pre-multiplied by log2 e it took three such
roundings, 2.15).
"""
import math

import pytest
import torch

from conftest import gpu_device
from test_attention_edges_gpu import (D, M_LSE, _bf, _heads, _merge, _split, check, check_all, keep_bits,
                                      random_inputs)

pytestmark = pytest.mark.gpu

S_CAUSAL = [1, 17, 63, 64, 65, 127, 128, 129, 191, 192, 193, 257, 321, 513]
B, H = 2, 2


# ------------------------------------------------------------------ references
def _tri(S, dev, dtype):
    ar = torch.arange(S, device=dev)
    return torch.zeros(S, S, device=dev, dtype=dtype).masked_fill(ar[None, :] > ar[:, None], -math.inf)


def ref64_causal(qkv, H, mask, keep, p, g):
    """test_attention_edges_gpu.ref64 with the triangular -inf on the scores: out, dqkv, P, lse."""
    Bq, S, _ = qkv.shape
    x = qkv.detach().double().requires_grad_(True)
    q, k, v = _split(x, H)
    s = q @ k.transpose(-1, -2) / math.sqrt(D) + _tri(S, qkv.device, torch.float64)
    if mask is not None:
        s = s + mask.double().view(Bq, 1, 1, S)
    P = torch.softmax(s, -1)
    Pd = P if keep is None else P * keep.double() / (1.0 - p)
    out = _merge(Pd @ v)
    out.backward(g.double())
    return out.detach(), x.grad, P.detach(), torch.logsumexp(s.detach(), -1)


def emu_causal(qkv, H, mask, keep, p, g):
    """test_attention_edges_gpu.emu with the triangular -inf on the scores: out, dqkv (both bf16)."""
    Bq, S, _ = qkv.shape
    q, k, v = _split(qkv.detach().float(), H)
    scale = 1.0 / math.sqrt(D)
    s = (q @ k.transpose(-1, -2)) * scale + _tri(S, qkv.device, torch.float32)
    if mask is not None:
        s = s + mask.float().view(Bq, 1, 1, S)
    P = torch.softmax(s, -1)
    kf = 1.0 if keep is None else keep.float() / (1.0 - p)
    Pd = _bf(P * kf)
    out = (Pd @ v).bfloat16()
    do = _heads(g.float(), H)
    delta = (do * out.float()).sum(-1, keepdim=True)
    dS = _bf(P * ((do @ v.transpose(-1, -2)) * kf - delta))
    dq = (dS @ k) * scale
    dk = (dS.transpose(-1, -2) @ q) * scale
    dv = Pd.transpose(-1, -2) @ do
    grad = torch.stack([dq, dk, dv], 0).permute(1, 3, 0, 2, 4).reshape(Bq, S, 3 * H * D)
    return _merge(out), grad.bfloat16()


def run_causal(qkv, H, mask, p, g, key=123, causal=True):
    """out, dqkv (the tensor the backward returned, with its column-sum rows) and the keep bits."""
    from databricks_distributed_deep_learning_amd.ops import _native_attention as NA
    Bq, S, _ = qkv.shape
    x = qkv.detach().clone().requires_grad_(True)
    got = []
    x.register_hook(got.append)
    torch.manual_seed(key)
    out = NA.attention(x, H, mask, p, causal=causal)
    keep = None
    if p > 0:
        torch.manual_seed(key)
        keep = keep_bits(NA.new_seed(), Bq, S, H, p, qkv.device)
    out.backward(g)
    return out.detach(), got[0], keep


def lse_causal(qkv, H, mask):
    """the forward's log-sum-exp [B, H, S] through the new entry point (p = 0)"""
    from databricks_distributed_deep_learning_amd.ops import _lib, _native_attention  # noqa: F401 (signatures)
    Bq, S, _ = qkv.shape
    out = torch.empty(Bq, S, H * D, dtype=torch.bfloat16, device=qkv.device)
    lse = torch.full((Bq, H, S), float("nan"), dtype=torch.float32, device=qkv.device)
    _lib.call("ddl_attn_causal_fwd", qkv.data_ptr(), _lib.p(mask), out.data_ptr(), lse.data_ptr(), Bq, S, H,
              1.0 / math.sqrt(D), 0.0, 0, 0)
    torch.cuda.synchronize()
    return lse, out


# ------------------------------------------------------------------ 1. parity
@pytest.mark.parametrize("p", [0.0, 0.25])
@pytest.mark.parametrize("kind", [None, "suffix"])
@pytest.mark.parametrize("S", S_CAUSAL)
def test_parity(S, kind, p):
    dev = gpu_device()
    qkv, g, mask = random_inputs(B, S, H, kind, dev, 3 + S)
    out, grad, keep = run_causal(qkv, H, mask, p, g)
    r_out, r_grad, _, lse64 = ref64_causal(qkv, H, mask, keep, p, g)
    e_out, e_grad = emu_causal(qkv, H, mask, keep, p, g)
    fails = []
    check_all(fails, f"causal S={S} mask={kind} p={p}", out, grad, r_out, r_grad, e_out, e_grad, H)
    if p == 0.0:
        lse, out2 = lse_causal(qkv, H, mask)
        assert torch.equal(out2, out)
        q, k, _ = _split(qkv.float(), H)
        s32 = (q @ k.transpose(-1, -2)) * (1.0 / math.sqrt(D)) + _tri(S, dev, torch.float32)
        if mask is not None:
            s32 = s32 + mask.view(B, 1, 1, S)
        check(fails, f"causal lse S={S} mask={kind}", lse, lse64, torch.logsumexp(s32, -1), m=M_LSE, ulp_term=False)
    assert not fails, "\n".join(fails)


# ------------------------------------------------------------------ 2. routing
def causal_routing_inputs(Bq, S, Hq, c=4.0, seed=0):
    """As test_attention_edges_gpu.routing_inputs (K a +-1 code, Q = c * code[t(i)], V randn), with the
    target t(i) <= i cycling through: the diagonal itself, key 0, the first key of the diagonal tile,
    the last key of the tile before it, and a uniform draw from 0..i."""
    q, k, v = (torch.empty(Bq, Hq, S, D) for _ in range(3))
    tgt = torch.empty(Bq, Hq, S, dtype=torch.long)
    ar = torch.arange(S)
    for b in range(Bq):
        for h in range(Hq):
            gen = torch.Generator().manual_seed(seed * 7919 + 1000 * b + h + 1)
            code = (torch.randint(0, 2, (S, D), generator=gen) * 2 - 1).float()
            vv = torch.randn(S, D, generator=gen).bfloat16().float()
            tile0 = ar // 64 * 64
            rnd = (torch.rand(S, generator=gen) * (ar + 1).float()).long().clamp_max(ar)
            kind = (ar + b + 2 * h) % 5
            t = torch.where(kind == 0, ar, torch.where(kind == 1, torch.zeros_like(ar), torch.where(
                kind == 2, tile0, torch.where(kind == 3, torch.where(tile0 > 0, tile0 - 1, ar), rnd))))
            assert (t <= ar).all() and (t >= 0).all()
            q[b, h], k[b, h], v[b, h], tgt[b, h] = c * code[t], code, vv, t
    qkv = torch.stack([q, k, v], 0).permute(1, 3, 0, 2, 4).reshape(Bq, S, 3 * Hq * D)
    assert (qkv.bfloat16().float() == qkv).all()
    return qkv.bfloat16(), tgt


@pytest.mark.parametrize("S", S_CAUSAL)
def test_causal_routing(S):
    dev = gpu_device()
    qkv, tgt = causal_routing_inputs(B, S, H, seed=S)
    ar = torch.arange(S)
    if S > 1:       # every kind of target is present
        assert (tgt == ar).any() and (tgt[..., 1:] == 0).any()
    if S > 65:
        assert ((tgt == ar // 64 * 64) & (ar % 64 != 0)).any() and ((tgt == ar // 64 * 64 - 1) & (ar >= 64)).any()
    qkv, tgt = qkv.to(dev), tgt.to(dev)
    g = torch.randn(B, S, H * D, generator=torch.Generator().manual_seed(S + 5)).bfloat16().to(dev)
    out, grad, _ = run_causal(qkv, H, None, 0.0, g)
    r_out, r_grad, P, _ = ref64_causal(qkv, H, None, None, 0.0, g)
    e_out, e_grad = emu_causal(qkv, H, None, None, 0.0, g)
    # conditions on the inputs alone
    wt = P.gather(-1, tgt.unsqueeze(-1)).squeeze(-1)
    assert wt.min().item() >= 0.999, f"target weight {wt.min().item()}"
    v = _split(qkv.double(), H)[2]
    do = _heads(g.double(), H)
    ti = tgt.unsqueeze(-1).expand(-1, -1, -1, D)
    want_out = _merge(v.gather(2, ti))
    want_dv = _merge(torch.zeros_like(v).scatter_add_(2, ti, do))
    assert (r_out - want_out).abs().max().item() < 1e-2 and (r_grad[..., 2 * H * D:] - want_dv).abs().max().item() < 1e-2
    fails = []
    label = f"causal routing S={S}"
    check_all(fails, label, out, grad, r_out, r_grad, e_out, e_grad, H, thirds=(2,))
    check(fails, f"{label} dV-routed", grad[..., 2 * H * D:], want_dv, e_grad[..., 2 * H * D:])
    assert not fails, "\n".join(fails)


# ------------------------------------------------------------------ 3. prefix invariance
@pytest.mark.parametrize("p", [0.0, 0.25])
@pytest.mark.parametrize("S", S_CAUSAL[1:])
def test_prefix_invariance(S, p):
    """Keys and values at positions >= n replaced by decoys (K = 2 * the code of a live target, V = 8)
    and dout zeroed there: rows < n of out, the log-sum-exp, dQ, dK and dV do not change by one bit, and
    dK / dV rows >= n are exactly zero.  A masked score contributes exp2(-inf) = 0 exactly and the tile
    order of rows < n does not depend on later rows, so this needs no tolerance."""
    dev = gpu_device()
    hd = H * D
    qkv, tgt = causal_routing_inputs(B, S, H, c=0.5, seed=S + 1)      # soft: dS, dQ, dK carry something
    g0 = torch.randn(B, S, hd, generator=torch.Generator().manual_seed(S + 9)).bfloat16()
    for n in sorted({n for n in (1, 63, 64, 65, 128, S - 1) if 1 <= n < S}):
        decoy = qkv.clone()
        live_k = qkv[:, :n, hd:2 * hd]                      # codes of keys below n (targets of live queries)
        idx = torch.arange(S - n) % n
        decoy[:, n:, hd:2 * hd] = 2.0 * live_k[:, idx]
        decoy[:, n:, 2 * hd:] = 8.0
        g = g0.clone()
        g[:, n:] = 0
        g = g.to(dev)
        res = []
        for x in (qkv.to(dev), decoy.to(dev)):
            out, grad, _ = run_causal(x, H, None, p, g, key=77)
            lse, _ = lse_causal(x, H, None)
            res.append((out, lse, grad))
        (o1, l1, g1), (o2, l2, g2) = res
        assert torch.equal(o1[:, :n], o2[:, :n]), f"n={n}: out rows < n differ"
        assert torch.equal(l1[:, :, :n], l2[:, :, :n]), f"n={n}: lse rows < n differ"
        for i, name in enumerate("QKV"):
            sl = slice(i * hd, (i + 1) * hd)
            assert torch.equal(g1[:, :n, sl], g2[:, :n, sl]), f"n={n}: d{name} rows < n differ"
        for gr in (g1, g2):
            assert (gr[:, n:, hd:] == 0).all(), f"n={n}: dK / dV rows >= n not zero"
        assert o1[:, :n].float().abs().max() > 0 and g1[:, :n].float().abs().max() > 0


# ------------------------------------------------------------------ 4. bias-gradient column sums
@pytest.mark.parametrize("p", [0.0, 0.25])
@pytest.mark.parametrize("S", [1, 65, 129, 193, 513])
def test_colsum_rows(S, p):
    """The rows attached to dQKV (the QKV Linear's bias gradient) sum to the column sums of dQKV.  The
    kernels sum their fp32 results before rounding them to bf16, so per column the two differ by at most
    sum|x| * (2^-8 [each element's bf16 rounding: 8 significand bits] + N * 2^-24 [fp32 summation of
    N = B * S terms]).  Measured: at most 0.98 of that bound (S = 1, two rows), 0.14 .. 0.47 beyond."""
    dev = gpu_device()
    qkv, g, mask = random_inputs(B, S, H, "suffix", dev, 21 + S)
    _, grad, _ = run_causal(qkv, H, mask, p, g)
    rows, ver = grad._ddl_colsum_rows
    assert ver == grad._version and rows.shape == (B * 4 * -(-S // 64), 3 * H * D)
    got = rows.double().sum(0)
    x = grad.double().reshape(-1, 3 * H * D)
    want, mag = x.sum(0), x.abs().sum(0)
    bound = mag * (2.0 ** -8 + x.shape[0] * 2.0 ** -24) + 1e-30
    worst = ((got - want).abs() / bound).max().item()
    print(f"COLSUM S={S} p={p} worst error / bound = {worst:.3f}")
    assert worst <= 1.0


# ------------------------------------------------------------------ 5. repeatability, 6. defaults
@pytest.mark.parametrize("S", [65, 193, 513])
def test_repeatable(S):
    dev = gpu_device()
    qkv, g, mask = random_inputs(B, S, H, "suffix", dev, 31 + S)
    a = run_causal(qkv, H, mask, 0.25, g, key=5)
    b = run_causal(qkv, H, mask, 0.25, g, key=5)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.parametrize("S", [17, 129, 200, 513])
def test_causal_false_is_the_default(S):
    from databricks_distributed_deep_learning_amd import ops
    dev = gpu_device()
    qkv, g, mask = random_inputs(B, S, H, "suffix", dev, 41 + S)
    res = []
    for kw in ({}, {"causal": False}):
        x = qkv.detach().clone().requires_grad_(True)
        torch.manual_seed(9)
        out = ops.attention(x, H, mask, 0.25, True, **kw)
        out.backward(g)
        res.append((out.detach(), x.grad))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    x = qkv.detach().clone().requires_grad_(True)
    torch.manual_seed(9)
    assert not torch.equal(ops.attention(x, H, mask, 0.25, True, causal=True), res[0][0])
