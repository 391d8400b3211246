"""Fused attention at its edges (GPU only): a dropped, leaked or unmasked key, the mask + dropout
paths, S < 64 and S > 512, the saved log-sum-exp and the switch-selected kernel paths.

Inputs.  The *routing* inputs make every key count: per (batch, head) a +-1 code matrix and a
permutation, K = code, Q = c * code[perm], V = randn, so query i puts its whole weight on key perm[i]
(c = 4: target weight >= 0.999, asserted on the reference) and out[i] = V[perm[i]]: one key dropped,
read from another batch / head, or unmasked moves the output by O(1).  Masked keys are decoys (K of a
live key times 2, V = 8) that would win without the bias.  The *shifted* variant moves every real
score below zero (a shared component: K[:, 63] = 1, Q[:, 63] = -512), so a zero-padded key past S
that is counted in a softmax wins as well.  The *soft* variant lowers c until the median target weight
is 0.4 .. 0.8, which gives dS, hence dQ and dK, something to carry.

Tolerance.  Every comparison is against an fp64 reference computed from the bf16 inputs (`ref64`) and
bounded by what a plain-torch emulation of the kernels' precision (`emu`: fp32 scores and softmax, P
and dS rounded to bf16 before their matmuls, fp32 accumulation, bf16 outputs) loses against it:
    max|kernel - ref64| <= M * max|emu - ref64| + 1/2 ulp_bf16(max|ref64|)
    rms(kernel - ref64) <= M * rms(emu - ref64) + 1/2 ulp_bf16(rms(ref64))
per tensor (out, dQ, dK, dV each on their own).  The log-sum-exp (fp32) is bounded by M_LSE times the
error of torch's fp32 logsumexp of fp32 scores against fp64.  Every case prints its ratios
((kernel error - ulp term) / emu error) before it asserts.

Measured on an MI355X (507 comparisons, all cases of this file): with the ulp term subtracted the
largest ratios are 0.62 (max form; dK, random inputs, S = 128, suffix mask, p = 0.1) and 0.35 (rms
form; soft routing dQ, S = 257); as plain kernel error / emu error the largest are 1.73 (dK), 1.46
(out), 1.40 (dQ), 1.00 (dV) and 0.86 .. 1.00 in the routing cases.  The log-sum-exp reaches 1.27 (max)
and 1.16 (rms) of torch's fp32 error (S = 255, no mask).  So M = 2 holds as it stands, for both.

Two limits of the cases: the sharp routing cases compare out and dV only (dS vanishes there, dQ and dK
are rounding noise), and in the shifted soft cases the shared component makes column 63 of dK large,
so dK is checked tightly by the plain soft cases only.
"""
import math
import os
import subprocess
import sys

import pytest
import torch

from conftest import gpu_device
from test_attention_gpu import attn_keep

pytestmark = pytest.mark.gpu

D = 64
# margin over the emulation's own error: a different summation order, v_exp_f32 in place of exp
M = 2.0
M_LSE = 2.0

S_SHORT = [1, 7, 16, 17, 63, 64, 65, 127, 128]
S_MED = [129, 191, 255, 256]
S_TILED = [257, 321, 511, 512, 513, 577, 641, 769]
S_MASKED = [7, 16, 17, 63, 64, 65, 127, 128, 129, 197, 256, 257, 321, 512, 513, 577]
S_RAGGED = [1, 7, 17, 63, 65, 127, 129, 191, 255, 257, 511, 513, 577]
# soft routing scale per S (bf16-exact), chosen on the CPU for a median target weight of 0.4 .. 0.8
# (plain, shifted); about ln(1.65 S) / 8
C_SOFT = {17: (0.40625, 0.40625), 63: (0.59375, 0.59375), 128: (0.6875, 0.703125), 197: (0.75, 0.765625),
          255: (0.78125, 0.796875), 257: (0.78125, 0.796875), 511: (0.875, 0.890625), 577: (0.890625, 0.90625)}


# ------------------------------------------------------------------ references
def _split(x, H):
    B, S, _ = x.shape
    return x.view(B, S, 3, H, D).permute(2, 0, 3, 1, 4).unbind(0)


def _merge(o):
    B, H, S, _ = o.shape
    return o.permute(0, 2, 1, 3).reshape(B, S, H * D)


def _heads(g, H):
    B, S, _ = g.shape
    return g.view(B, S, H, D).permute(0, 2, 1, 3)


def ref64(qkv, H, mask, keep, p, g):
    """fp64 forward and autograd backward from the bf16 inputs: out, dqkv, P, lse."""
    B, S, _ = qkv.shape
    x = qkv.detach().double().requires_grad_(True)
    q, k, v = _split(x, H)
    s = q @ k.transpose(-1, -2) / math.sqrt(D)
    if mask is not None:
        s = s + mask.double().view(B, 1, 1, S)
    P = torch.softmax(s, -1)
    Pd = P if keep is None else P * keep.double() / (1.0 - p)
    out = _merge(Pd @ v)
    out.backward(g.double())
    return out.detach(), x.grad, P.detach(), torch.logsumexp(s.detach(), -1)


def _bf(t):
    return t.bfloat16().float()


def emu(qkv, H, mask, keep, p, g):
    """The precision the kernels are entitled to, in plain torch: out, dqkv (both bf16)."""
    B, S, _ = qkv.shape
    q, k, v = _split(qkv.detach().float(), H)
    scale = 1.0 / math.sqrt(D)
    s = (q @ k.transpose(-1, -2)) * scale
    if mask is not None:
        s = s + mask.float().view(B, 1, 1, S)
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
    grad = torch.stack([dq, dk, dv], 0).permute(1, 3, 0, 2, 4).reshape(B, S, 3 * H * D)
    return _merge(out), grad.bfloat16()


def keep_bits(seed, B, S, H, p, dev):
    bh = torch.arange(B * H, device=dev).view(B, H, 1, 1)
    qi = torch.arange(S, device=dev).view(1, 1, S, 1)
    ki = torch.arange(S, device=dev).view(1, 1, 1, S)
    return attn_keep(seed, (bh * S + qi) * S + ki, p)


def run_kernel(qkv, H, mask, p, g, key=123):
    """out, dqkv and (p > 0) the keep bits the kernels drew, rebuilt from the same host seed."""
    from databricks_distributed_deep_learning_amd.ops import _native_attention as NA
    B, S, _ = qkv.shape
    x = qkv.detach().clone().requires_grad_(True)
    torch.manual_seed(key)
    out = NA.attention(x, H, mask, p)
    keep = None
    if p > 0:
        torch.manual_seed(key)
        keep = keep_bits(NA.new_seed(), B, S, H, p, qkv.device)
    out.backward(g)
    return out.detach(), x.grad, keep


# ------------------------------------------------------------------ tolerance
def _half_ulp_bf16(x):
    return 0.0 if not x > 0 else 2.0 ** (math.floor(math.log2(x)) - 8)


def _rms(t):
    return t.pow(2).mean().sqrt().item()


def check(fails, label, got, ref, em, m=None, ulp_term=True):
    """The two bounds of the module docstring; prints the figures, appends what fails."""
    m = M if m is None else m
    ref = ref.double()
    d, e = (got.double() - ref).abs(), (em.double() - ref).abs()
    kmax, emax, krms, erms = d.max().item(), e.max().item(), _rms(d), _rms(e)
    hmax = _half_ulp_bf16(ref.abs().max().item()) if ulp_term else 0.0
    hrms = _half_ulp_bf16(_rms(ref)) if ulp_term else 0.0

    def ratio(kk, h, ee):
        return (kk - h) / ee if ee > 0 else (0.0 if kk <= h else float("inf"))
    print(f"RATIO {label} max={ratio(kmax, hmax, emax):.3f} rms={ratio(krms, hrms, erms):.3f} "
          f"kmax={kmax:.3e} emax={emax:.3e} hmax={hmax:.3e} krms={krms:.3e} erms={erms:.3e} hrms={hrms:.3e}")
    if not kmax <= m * emax + hmax:
        worst = int(d.flatten(1).max(1).values.argmax()) if d.dim() > 1 else -1
        fails.append(f"{label}: max err {kmax:.3e} > {m} * {emax:.3e} + {hmax:.3e} (worst batch row {worst})")
    if not krms <= m * erms + hrms:
        fails.append(f"{label}: rms err {krms:.3e} > {m} * {erms:.3e} + {hrms:.3e}")


def check_all(fails, label, out, grad, r_out, r_grad, e_out, e_grad, H, thirds=(0, 1, 2)):
    check(fails, f"{label} out", out, r_out, e_out)
    hd = H * D
    for i in thirds:
        sl = slice(i * hd, (i + 1) * hd)
        check(fails, f"{label} d{'QKV'[i]}", grad[..., sl], r_grad[..., sl], e_grad[..., sl])


# ------------------------------------------------------------------ inputs
def mask_patterns(S):
    """(name, masked keys, bias) per batch row: suffixes pinned to the 4-key group, 16-key block and
    64-key tile edges and to S - 1, a prefix past the first tile, every third key, the last key
    alone, and two rows with -inf in place of -10000."""
    ar = torch.arange(S)
    pats = [(f"suffix{L}", ar >= L, -10000.0)
            for L in sorted({1, 3, 4, 5, 15, 16, 17, 63, 64, 65, S - 1}) if 1 <= L <= S - 1]
    pats.append(("prefix", ar < min(65, S - 1), -10000.0))
    pats.append(("third", ar % 3 == 0, -10000.0))
    pats.append(("last", ar == S - 1, -10000.0))
    pats.append(("suffix-inf", ar >= (S + 1) // 2, -math.inf))
    pats.append(("third-inf", ar % 3 == 0, -math.inf))
    return pats


def routing_inputs(B, S, H, c, dead=None, shift=False, seed=0):
    """qkv [B, S, 3 H D] bf16 (exactly representable) and the target key of every query [B, H, S].
    dead: [B, S] bool, keys that a mask hides; they become decoys."""
    q, k, v = (torch.empty(B, H, S, D) for _ in range(3))
    tgt = torch.empty(B, H, S, dtype=torch.long)
    ar = torch.arange(S)
    for b in range(B):
        for h in range(H):
            gen = torch.Generator().manual_seed(seed * 7919 + 1000 * b + h + 1)
            code = (torch.randint(0, 2, (S, D), generator=gen) * 2 - 1).float()
            vv = torch.randn(S, D, generator=gen).bfloat16().float()
            dd = torch.zeros(S, dtype=torch.bool) if dead is None else dead[b]
            live = (~dd).nonzero().flatten()
            t = live[torch.randperm(len(live), generator=gen)][ar % len(live)]
            kk = code.clone()
            di = dd.nonzero().flatten()
            if len(di):
                kk[di] = 2.0 * code[live[di % len(live)]]
                vv[di] = 8.0
            qq = c * code[t]
            if shift:
                kk[:, D - 1] = 1.0
                qq[:, D - 1] = -512.0
            q[b, h], k[b, h], v[b, h], tgt[b, h] = qq, kk, vv, t
    qkv = torch.stack([q, k, v], 0).permute(1, 3, 0, 2, 4).reshape(B, S, 3 * H * D)
    assert (qkv.bfloat16().float() == qkv).all()
    return qkv.bfloat16(), tgt


def masked_routing_inputs(S, H, c, shift, seed=0):
    pats = mask_patterns(S)
    dead = torch.stack([p[1] for p in pats])
    mask = torch.stack([p[1].float() * 0.0 for p in pats])
    for i, (_, dd, val) in enumerate(pats):
        mask[i][dd] = val
    qkv, tgt = routing_inputs(len(pats), S, H, c, dead, shift, seed)
    return qkv, tgt, mask, [p[0] for p in pats]


def routing_case(dev, B, S, H, masked=False, p=0.0, shift=False, c=4.0, run=run_kernel):
    """Sharp routing: out and dV against the fp64 reference, dV against dO routed through perm."""
    names = None
    if masked:
        qkv, tgt, mask, names = masked_routing_inputs(S, H, c, shift, seed=S)
        B = len(names)
        mask = mask.to(dev)
    else:
        qkv, tgt = routing_inputs(B, S, H, c, None, shift, seed=S)
        mask = None
    qkv, tgt = qkv.to(dev), tgt.to(dev)
    g = torch.randn(B, S, H * D, generator=torch.Generator().manual_seed(S + 5)).bfloat16().to(dev)
    out, grad, keep = run(qkv, H, mask, p, g)
    r_out, r_grad, P, _ = ref64(qkv, H, mask, keep, p, g)
    e_out, e_grad = emu(qkv, H, mask, keep, p, g)
    # conditions on the inputs alone
    wt = P.gather(-1, tgt.unsqueeze(-1)).squeeze(-1)
    assert wt.min().item() >= 0.999, f"target weight {wt.min().item()}"
    v = _split(qkv.double(), H)[2]
    do = _heads(g.double(), H)
    ti = tgt.unsqueeze(-1).expand(-1, -1, -1, D)
    kt = torch.ones_like(wt) if keep is None else keep.gather(-1, tgt.unsqueeze(-1)).squeeze(-1).double() / (1.0 - p)
    if keep is not None:
        assert abs(keep.double().mean().item() - (1.0 - p)) < 0.02
    want_out = _merge(v.gather(2, ti) * kt.unsqueeze(-1))
    want_dv = _merge(torch.zeros_like(v).scatter_add_(2, ti, do * kt.unsqueeze(-1)))
    assert (r_out - want_out).abs().max().item() < 1e-2 and (r_grad[..., 2 * H * D:] - want_dv).abs().max().item() < 1e-2
    fails = []
    label = f"routing S={S} masked={masked} p={p} shift={shift}"
    check_all(fails, label, out, grad, r_out, r_grad, e_out, e_grad, H, thirds=(2,))
    check(fails, f"{label} dV-routed", grad[..., 2 * H * D:], want_dv, e_grad[..., 2 * H * D:])
    if names is not None:
        fails = [f + f" rows={names}" for f in fails]
    return fails


def random_inputs(B, S, H, kind, dev, seed):
    gen = torch.Generator().manual_seed(seed)
    qkv = torch.randn(B, S, 3 * H * D, generator=gen).bfloat16().to(dev)
    g = torch.randn(B, S, H * D, generator=gen).bfloat16().to(dev)
    ar = torch.arange(S)
    mask = None
    if kind == "suffix":       # per-batch length; row 0 hides the last key alone
        lens = torch.tensor([max(S // 2, S - 1 - 37 * b) for b in range(B)])
        mask = ((ar[None] >= lens[:, None]).float() * -10000.0).to(dev)
    elif kind == "holes":
        mask = (torch.stack([((ar * 7 + 3 * b) % 5 == 0) | (ar == S - 1) for b in range(B)]).float() * -10000.0).to(dev)
    return qkv, g, mask


def random_case(dev, B, S, H, kind, p, seed=0):
    qkv, g, mask = random_inputs(B, S, H, kind, dev, seed + S)
    out, grad, keep = run_kernel(qkv, H, mask, p, g)
    if keep is not None:
        assert abs(keep.double().mean().item() - (1.0 - p)) < 0.02
    r_out, r_grad, _, _ = ref64(qkv, H, mask, keep, p, g)
    e_out, e_grad = emu(qkv, H, mask, keep, p, g)
    fails = []
    check_all(fails, f"random B={B} S={S} H={H} mask={kind} p={p}", out, grad, r_out, r_grad, e_out, e_grad, H)
    return fails


# ------------------------------------------------------------------ 1. routing
@pytest.mark.parametrize("S", S_SHORT + S_MED + S_TILED)
def test_routing(S):
    fails = routing_case(gpu_device(), 2, S, 2)
    assert not fails, "\n".join(fails)


def test_routing_s1024():
    fails = routing_case(gpu_device(), 1, 1024, 1)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("S", S_RAGGED)
def test_routing_shifted(S):
    """every real score below zero: a zero-padded key past S that is counted wins the softmax"""
    fails = routing_case(gpu_device(), 2, S, 2, shift=True)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("shift", [False, True])
@pytest.mark.parametrize("S", S_MASKED)
def test_routing_masked(S, shift):
    fails = routing_case(gpu_device(), 0, S, 2, masked=True, shift=shift)
    assert not fails, "\n".join(fails)


# ------------------------------------------------------------------ 2. soft routing: dQ, dK
@pytest.mark.parametrize("shift", [False, True])
@pytest.mark.parametrize("S", sorted(C_SOFT))
def test_routing_soft(S, shift):
    dev = gpu_device()
    B, H = 2, 2
    qkv, tgt = routing_inputs(B, S, H, C_SOFT[S][int(shift)], None, shift, seed=S)
    qkv, tgt = qkv.to(dev), tgt.to(dev)
    g = torch.randn(B, S, H * D, generator=torch.Generator().manual_seed(S + 5)).bfloat16().to(dev)
    out, grad, _ = run_kernel(qkv, H, None, 0.0, g)
    r_out, r_grad, P, _ = ref64(qkv, H, None, None, 0.0, g)
    med = P.gather(-1, tgt.unsqueeze(-1)).median().item()
    assert 0.4 <= med <= 0.8, med
    e_out, e_grad = emu(qkv, H, None, None, 0.0, g)
    fails = []
    check_all(fails, f"soft S={S} shift={shift}", out, grad, r_out, r_grad, e_out, e_grad, H)
    assert not fails, "\n".join(fails)


# ------------------------------------------------------------------ 3. dropout
@pytest.mark.parametrize("S", [384, 512, 513, 577, 641, 769])   # 3, 4, 5, 5, 6, 7 keep words of 128 keys
def test_dropout_parity_long(S):
    fails = random_case(gpu_device(), 2, S, 2, None, 0.25)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("kind", ["suffix", "holes"])
@pytest.mark.parametrize("p", [0.1, 0.25])
@pytest.mark.parametrize("S", [100, 128, 197, 256, 300, 577])
def test_mask_and_dropout(S, p, kind):
    fails = random_case(gpu_device(), 2, S, 2, kind, p)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("S", [197, 577])
def test_routing_dropout(S, masked):
    """a dropped target key leaves its row near 0, a kept one near V[perm[i]] / (1 - p): each keep bit
    is tied to its (query, key) pair, in the forward and through dV in the backward"""
    fails = routing_case(gpu_device(), 2, S, 2, masked=masked, p=0.25)
    assert not fails, "\n".join(fails)


# ------------------------------------------------------------------ 4. the random-input shapes, tight
@pytest.mark.parametrize("kind", [None, "suffix"])
@pytest.mark.parametrize("B,S,H", [(2, 128, 12), (3, 197, 2), (1, 129, 2), (1, 257, 2), (1, 512, 2)])
def test_random_shapes(B, S, H, kind):
    fails = random_case(gpu_device(), B, S, H, kind, 0.0)
    assert not fails, "\n".join(fails)


# ------------------------------------------------------------------ 5. lse
@pytest.mark.parametrize("kind", [None, "suffix", "holes"])
@pytest.mark.parametrize("S", [17, 63, 127, 128, 197, 255, 511, 577])
def test_lse(S, kind):
    dev = gpu_device()
    from databricks_distributed_deep_learning_amd.ops import _lib, _native_attention  # noqa: F401 (signatures)
    B, H = 2, 2
    qkv, _, mask = random_inputs(B, S, H, kind, dev, 11 + S)
    out = torch.empty(B, S, H * D, dtype=torch.bfloat16, device=dev)
    lse = torch.full((B, H, S), float("nan"), dtype=torch.float32, device=dev)
    _lib.call("ddl_attn_fwd", qkv.data_ptr(), _lib.p(mask), out.data_ptr(), lse.data_ptr(), B, S, H,
              1.0 / math.sqrt(D), 0.0, 0, 0)
    torch.cuda.synchronize()
    g = torch.zeros_like(out)
    _, _, _, lse64 = ref64(qkv, H, mask, None, 0.0, g)
    q, k, _ = _split(qkv.float(), H)
    s32 = (q @ k.transpose(-1, -2)) * (1.0 / math.sqrt(D))
    if mask is not None:
        s32 = s32 + mask.view(B, 1, 1, S)
    fails = []
    check(fails, f"lse S={S} mask={kind}", lse, lse64, torch.logsumexp(s32, -1), m=M_LSE, ulp_term=False)
    assert not fails, "\n".join(fails)


# ------------------------------------------------------------------ 6. the switch-selected paths
CHILD_S = [17, 100, 128, 197, 256]


def _child():
    dev = torch.device("cuda", 0)
    fails = []
    for S in CHILD_S:
        for masked in (False, True):
            for p in (0.0, 0.25):
                fails += routing_case(dev, 2, S, 2, masked=masked, p=p)
    print("\n".join(fails))
    return 1 if fails else 0


def test_switch_selected_paths():
    """DDL_ATTN_FUSED_BWD=0 / DDL_ATTN_MED=0 send S <= 128 / 128 < S <= 256 to the tiled kernels; the
    switches are read once per process, so each setting gets a fresh child that runs the routing test."""
    gpu_device()
    bad = []
    for var in ("DDL_ATTN_FUSED_BWD", "DDL_ATTN_MED"):
        env = {k: v for k, v in os.environ.items() if k not in ("DDL_ATTN_FUSED_BWD", "DDL_ATTN_MED")}
        env[var] = "0"
        cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.abspath(__file__), "--child"]
        try:
            r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=240)
        except subprocess.TimeoutExpired:
            pytest.fail(f"{var}=0: child timed out; no further child started")
        print(r.stdout[-4000:])
        if r.returncode < 0:
            pytest.fail(f"{var}=0: child ended by signal {-r.returncode}; no further child started\n{r.stderr[-2000:]}")
        if r.returncode != 0:
            bad.append(f"{var}=0: exit {r.returncode}\n{r.stdout[-3000:]}\n{r.stderr[-2000:]}")
    assert not bad, "\n".join(bad)


if __name__ == "__main__":
    if sys.argv[1:] == ["--child"]:
        sys.exit(_child())
