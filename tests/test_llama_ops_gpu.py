"""RMSNorm, RoPE + GQA pack and SwiGLU kernels against an fp64 oracle (GPU only).

Every case draws its inputs once in bf16 and hands the same values to the kernels (through ``ops.*``, so the
dispatch is under test: each case asserts that the native autograd Function ran), to the oracle
(``llama_oracle.*_ref`` in fp64) and to the emulation (the same code in fp32 with every stored tensor rounded
once to bf16).  Inputs are ``randn``, weights ``rand + 0.5``: a column, row, pair-partner, sign, head or
position mix-up moves a result by O(0.1 .. 1) while the bf16 yardstick is about 1e-2.  Per tensor
(``norm_oracle.bound``)
    max|kernel - ref64| <= M * max|emu - ref64| + 1/2 ulp(max|ref64|)
    rms(kernel - ref64) <= M * rms(emu - ref64) + 1/2 ulp(rms(ref64))
with ``M_STORE = 2`` for the bf16 tensors and ``M_F32 = 4`` for the fp32 side output (``rstd``), the margins
``tests/test_norm_oracle_gpu.py`` derived for this class of kernel.  Every comparison prints its ratios
((kernel error - ulp term) / emulation error) before it asserts; a ratio above M / 1.5 would be a finding.

Bit-exact checks ride along: two runs of every kernel give the same bits; RoPE copies v, is the identity at
position 0 and, with one query head per key / value head, hands dv through unchanged.  SwiGLU is also run
with gate entries of +-80 and +-3e38 planted (``up`` and ``dz`` are 0.5 there, so that the exact results are
representable): everything stays finite, the planted results are within 2^-7 relative (twice bf16's half
ulp) of the oracle and every other element keeps its bits.

Measured on an MI355X (268 comparisons, all cases of this file), largest (error - ulp term) / emulation error
per tensor kind, max form / rms form (<= 0: the kernel's error is within the half-ulp term alone):
  RMSNorm   y <= 0 / <= 0, dx <= 0 / <= 0, dw <= 0 / <= 0 (bf16); rstd 0.62 / 0.33 (fp32; H = 576, 4100 rows:
            ``rsqrtf`` and the DPP summation order against torch's)
  RoPE      out <= 0 / <= 0, din <= 0 / <= 0 (0 where the emulation is exact: S = 1 is position 0 alone)
  SwiGLU    z <= 0 / <= 0, dgate <= 0 / <= 0, dup <= 0 / 0.17 (I = 8, 3 rows: 24 elements)
all far below M / 1.5; nothing to explain.  The planted gates: z and dup at -80 came out as -7.2222e-34 against
-7.2194e-34 (3.9e-4 relative, one bf16 rounding), dgate -3.5660e-34 against -3.5646e-34; +-3e38 gave 1.502e38 /
-0.0 and 0.25 / -0.0, as the oracle.
"""
import pytest
import torch

import llama_oracle as LO
import norm_oracle as NO
from conftest import gpu_device

pytestmark = pytest.mark.gpu

M_STORE = 2.0
M_F32 = 4.0
BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
EPS = 1e-5


def _ops():
    from databricks_distributed_deep_learning_amd import ops
    from databricks_distributed_deep_learning_amd.ops import _lib
    assert _lib.available(), _lib.load_error()
    return ops


def _native(t, name):
    assert t.grad_fn is not None and name in type(t.grad_fn).__name__, type(t.grad_fn).__name__


# ================================================================== RMSNorm
def rms_run(x, w, dy, add):
    from databricks_distributed_deep_learning_amd.ops.bridge import GradBridge
    ops = _ops()
    xp, wp = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    bridge = GradBridge() if add is not None else None
    y = ops.rms_norm(xp, wp, EPS, grad_from=bridge)
    _native(y, "_RMSNorm")
    rstd = y.grad_fn.saved_tensors[2]
    if bridge is not None:
        bridge.put(add.clone())
    y.backward(dy)
    return dict(y=y.detach(), rstd=rstd, dx=xp.grad, dw=wp.grad)


RMS_WIDTHS = [64, 128, 576, 960, 2048, 4096]
RMS_CASES = [(H, r) for H in RMS_WIDTHS for r in (1, 3, 67)] + [(576, 4100), (2048, 4100)]


@pytest.mark.parametrize("H,rows", RMS_CASES)
def test_rmsnorm_against_oracle(H, rows):
    dev = gpu_device()
    torch.manual_seed(H * 7 + rows)
    lead = (4, rows // 4) if rows % 4 == 0 else (rows,)
    mk = lambda *s: torch.randn(*s, device=dev).to(BF16)  # noqa: E731
    x, dy, add = mk(*lead, H), mk(*lead, H), mk(*lead, H)
    w = (torch.rand(H, device=dev) + 0.5).to(BF16)
    from databricks_distributed_deep_learning_amd.ops import _lib
    from databricks_distributed_deep_learning_amd.ops import _native_llama  # noqa: F401  (registers the signatures)
    nblk = _lib.fn("ddl_rmsnorm_bwd_nblk")(rows)
    assert (nblk > 1) == (rows > 8)          # 67 and 4100 rows: dw over more than one partial block
    fails = []
    for a in (None, add):
        tag = f"rms H={H} rows={rows} add={a is not None}"
        got = rms_run(x, w, dy, a)
        ref, em = (LO.rms_ref(x, w, EPS, dy, a, dt) for dt in (F64, F32))
        assert got["rstd"].dtype == F32 and got["y"].dtype == BF16 and got["dw"].dtype == BF16
        NO.bound(got["y"], ref.y, em.y, BF16, M_STORE, f"{tag} y", fails)
        NO.bound(got["rstd"], ref.rstd, em.rstd, F32, M_F32, f"{tag} rstd", fails)
        NO.bound(got["dx"], ref.dx, em.dx, BF16, M_STORE, f"{tag} dx", fails)
        NO.bound(got["dw"], ref.dw, em.dw, BF16, M_STORE, f"{tag} dw", fails)
        again = rms_run(x, w, dy, a)
        for k in got:
            assert torch.equal(got[k], again[k]), f"{tag} {k}: two runs differ"
    assert not fails, "\n".join(fails)


def test_rmsnorm_unsupported_widths_fall_back():
    dev = gpu_device()
    ops = _ops()
    for H in (60, 8200):
        x = torch.randn(3, H, device=dev).to(BF16).requires_grad_(True)
        w = torch.ones(H, device=dev, dtype=BF16)
        y = ops.rms_norm(x, w, EPS)
        assert "_RMSNorm" not in type(y.grad_fn).__name__
        ref = LO.rms_ref(x.detach(), w, EPS, torch.zeros_like(x), None, F32)
        torch.testing.assert_close(y.float(), ref.y.float(), atol=2e-2, rtol=2e-2)


# ================================================================== RoPE + GQA pack
def rope_run(qkv, table, H, Hkv, dout):
    ops = _ops()
    qp = qkv.clone().requires_grad_(True)
    out = ops.rope_qkv(qp, table, H, Hkv)
    _native(out, "_RopeQKV")
    out.backward(dout)
    return out.detach(), qp.grad


_TABLES = {}


def _table(theta, dev):
    if theta not in _TABLES:
        _TABLES[theta] = _ops().rope_table(256, theta).to(dev)
    return _TABLES[theta]


@pytest.mark.parametrize("theta", [1e4, 5e5])
@pytest.mark.parametrize("S", [1, 5, 130])
@pytest.mark.parametrize("H,Hkv", [(2, 2), (2, 1), (4, 1), (9, 3), (32, 8)])
def test_rope_qkv_against_oracle(H, Hkv, S, theta):
    dev = gpu_device()
    B, G = 2, H // Hkv
    torch.manual_seed(H * 100 + Hkv * 10 + S)
    qkv = torch.randn(B, S, (H + 2 * Hkv) * 64, device=dev).to(BF16)
    dout = torch.randn(B, S, 3 * H * 64, device=dev).to(BF16)
    table = _table(theta, dev)
    tag = f"rope H={H} Hkv={Hkv} S={S} theta={theta:g}"
    out, din = rope_run(qkv, table, H, Hkv, dout)
    ref, em = (LO.rope_ref(qkv, table, H, Hkv, dout, dt) for dt in (F64, F32))
    fails = []
    NO.bound(out, ref.out, em.out, BF16, M_STORE, f"{tag} out", fails)
    NO.bound(din, ref.din, em.din, BF16, M_STORE, f"{tag} din", fails)
    assert not fails, "\n".join(fails)
    o5 = out.view(B, S, 3, H, 64)
    x4 = qkv.view(B, S, H + 2 * Hkv, 64)
    # v: the input's bits, in every slot of its group
    assert torch.equal(o5[:, :, 2], x4[:, :, H + Hkv:].repeat_interleave(G, 2))
    # k: every slot of a group holds the same bits
    assert torch.equal(o5[:, :, 1], o5[:, :, 1, ::G].repeat_interleave(G, 2))
    # position 0: the identity, in bits
    assert torch.equal(o5[:, 0, 0], x4[:, 0, :H])
    assert torch.equal(o5[:, 0, 1, ::G], x4[:, 0, H:H + Hkv])
    if G == 1:      # dv is the incoming gradient's bits
        assert torch.equal(din.view(B, S, H + 2 * Hkv, 64)[:, :, H + Hkv:], dout.view(B, S, 3, H, 64)[:, :, 2])
    out2, din2 = rope_run(qkv, table, H, Hkv, dout)
    assert torch.equal(out, out2) and torch.equal(din, din2), f"{tag}: two runs differ"


def test_rope_qkv_raises_past_the_table_on_the_gpu():
    dev = gpu_device()
    ops = _ops()
    table = ops.rope_table(8, 1e4).to(dev)
    qkv = torch.randn(1, 9, 3 * 64, device=dev).to(BF16)
    with pytest.raises(ValueError, match="exceeds the rotary table"):
        ops.rope_qkv(qkv, table, 1, 1)
    # the C entry point refuses on its own too: nothing is launched
    from databricks_distributed_deep_learning_amd.ops import _lib
    from databricks_distributed_deep_learning_amd.ops import _native_llama  # noqa: F401  (registers the signatures)
    out = torch.zeros(1, 9, 3 * 64, device=dev, dtype=BF16)
    rc = _lib.fn("ddl_rope_qkv_fwd")(_lib.p(qkv), _lib.p(table), _lib.p(out), 1, 9, 1, 1, 8, _lib.stream())
    torch.cuda.synchronize()
    assert rc == -2 and not out.any()


# ================================================================== SwiGLU
def swiglu_run(gu, dz):
    ops = _ops()
    gp = gu.clone().requires_grad_(True)
    z = ops.swiglu(gp)
    _native(z, "_SwiGLU")
    z.backward(dz)
    return z.detach(), gp.grad


@pytest.mark.parametrize("rows", [1, 3, 67, 1030])
@pytest.mark.parametrize("I", [8, 352, 1536, 8192])
def test_swiglu_against_oracle(I, rows):
    dev = gpu_device()
    torch.manual_seed(I + rows)
    gu = torch.randn(rows, 2 * I, device=dev)
    gu[:, :I] *= 4
    gu = gu.to(BF16)
    dz = torch.randn(rows, I, device=dev).to(BF16)
    tag = f"swiglu I={I} rows={rows}"
    z, dgu = swiglu_run(gu, dz)
    ref, em = (LO.swiglu_ref(gu, dz, dt) for dt in (F64, F32))
    fails = []
    NO.bound(z, ref.z, em.z, BF16, M_STORE, f"{tag} z", fails)
    NO.bound(dgu[:, :I], ref.dgu[:, :I], em.dgu[:, :I], BF16, M_STORE, f"{tag} dgate", fails)
    NO.bound(dgu[:, I:], ref.dgu[:, I:], em.dgu[:, I:], BF16, M_STORE, f"{tag} dup", fails)
    assert not fails, "\n".join(fails)
    z2, dgu2 = swiglu_run(gu, dz)
    assert torch.equal(z, z2) and torch.equal(dgu, dgu2), f"{tag}: two runs differ"

    # the ends of the range: +-80 and +-3e38 planted in the last row's gate (up = dz = 0.5 at those columns)
    cols = torch.tensor([0, 2, 5, 7], device=dev)
    gp, dp = gu.clone(), dz.clone()
    gp[-1, cols] = torch.tensor([80.0, -80.0, 3e38, -3e38], device=dev).to(BF16)
    gp[-1, I + cols] = 0.5
    dp[-1, cols] = 0.5
    zp, dgp = swiglu_run(gp, dp)
    assert torch.isfinite(zp).all() and torch.isfinite(dgp).all(), f"{tag}: non-finite with planted gates"
    rp = LO.swiglu_ref(gp, dp, F64)
    for name, got, want in (("z", zp[-1, cols], rp.z[-1, cols]), ("dgate", dgp[-1, cols], rp.dgu[-1, cols]),
                            ("dup", dgp[-1, I + cols], rp.dgu[-1, I + cols])):
        print(f"PLANTED {tag} {name} got={got.tolist()} want={want.tolist()}")
        assert bool(((got.double() - want).abs() <= 2.0 ** -7 * want.abs() + 1e-37).all()), f"{tag} planted {name}"
    # elementwise kernels: nothing else moved
    keep = torch.ones(rows, I, dtype=torch.bool, device=dev)
    keep[-1, cols] = False
    assert torch.equal(zp[keep], z[keep])
    assert torch.equal(dgp[:, :I][keep], dgu[:, :I][keep]) and torch.equal(dgp[:, I:][keep], dgu[:, I:][keep])


def test_swiglu_odd_width_falls_back():
    dev = gpu_device()
    ops = _ops()
    gu = torch.randn(3, 2 * 12, device=dev).to(BF16).requires_grad_(True)       # I = 12: no multiple of 8
    z = ops.swiglu(gu)
    assert "_SwiGLU" not in type(z.grad_fn).__name__
    torch.testing.assert_close(z.float(), LO.swiglu_ref(gu.detach(), None, F32).z.float(), atol=2e-2, rtol=2e-2)
