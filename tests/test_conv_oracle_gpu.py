"""The convolution kernels against the fp64 oracle of tests/conv_oracle.py, in two tiers.

exact   small-integer operands (every element's absolute sum A <= 256, statistics sums < 2^24; the CPU
        file checks that for every case here): ``torch.equal`` with the oracle, no tolerance.
real    randn operands rounded to bf16: per element |err| <= a + half_ulp_out(|r| + a) with
        a = 2 n 2^-24 A (conv_oracle.tol).  The only cases that carry the extra 2^-8 A term of bf16
        split-K partials are the implicit-GEMM weight gradients on kernel "wg" with a bf16 output
        (``ddl_gemm_wgrad``: bf16 slabs whenever the output is bf16, one split included); the other
        conv weight-gradient kernels ("small", "narrow", "tnarrow": gemm.hip) keep fp32 slabs, and
        "big" / "duo" have no CONVW variant and run "small".  Statistics rows are compared with the fp64
        sums of the kernel's own stored output within n 2^-24 sum |term| (n = pixels; n + 3 for the
        centred BatchNorm-backward row, which the kernels form as (sum dz x - mean sum dz) istd: three more
        roundings, and |term| = |dz| (|x| + |mean|) istd).

Guards: every tensor handed to a kernel, and every tensor the wrappers allocate themselves (outputs,
statistics rows, split-K workspaces, re-laid-out weights: ``torch.empty`` / ``torch.zeros`` of
ops/_native_conv.py and ops/_native_gemm.py are routed through the arena), is a 16-byte-aligned view
into a buffer with 64 KiB of 0xFF bytes on each side -- NaN in bf16 and fp32.  Fresh outputs are NaN
before the call.  After the call every guard byte must still be 0xFF (nothing writes outside its
output), and a result that depended on memory outside its inputs would be NaN.

Largest max(|err| / tol) of the real tier per kernel (MI355X; all 440 cases pass, the file takes 7 s):
  direct 3x3   forward 0.964, BatchNorm-backward epilogue 0.973, dgrad 0.967, wgrad 0.994;
               statistics rows 0.026
  implicit GEMM forward 0.997 and dgrad 0.995 under every forced kind, stride-2 dgrad 0.991 on each of
               serial / multi / multi_narrow, in-place residual 0.993; wgrad 1.000 on small / narrow /
               tnarrow (and big / duo, which run small), 0.604 on wg (its bound carries 2^-8 A)
  stem         direct forward 0.970 (statistics rows 0.028), direct wgrad 0.998, whole path forward
               0.992, whole path wgrad 0.967
  patch embed  forward 0.930, dW 0.999, db 0.999
A ratio just below 1 is one correct rounding: with short reductions a ~ 1e-5 |r| and the bound is the
output format's half ulp, which a round-to-nearest store reaches.  The 1.000 of the weight gradients is
a tie: a sum of a few bf16 products that lies exactly between two bf16 numbers.
Kernels that ran where a forced kind was not eligible (these shapes have C < 32 or K not a multiple of
128, and a reduction under 64 in places): "duo" always ran ddl_gemm (128x128); "big" ran ddl_gemm_big2
where the reduction is a multiple of 8 and at least 64 and ddl_gemm otherwise, and ddl_gemm for every
weight gradient (no CONVW variant); "narrow" and "tnarrow" ran ddl_gemm_n64; the tuner (None) picked
among ddl_gemm, ddl_gemm_n64, ddl_gemm_big2 and, for the wg shape, ddl_gemm_wgrad.
"""
from types import SimpleNamespace

import pytest
import torch

import conv_oracle as O
from conftest import gpu_device

pytestmark = pytest.mark.gpu

GUARD = 65536
BF, F32 = torch.bfloat16, torch.float32


# ---------------------------------------------------------------------------- guards
class Arena:
    """Tensors as views into 0xFF-filled buffers; ``check`` asserts every guard byte is untouched."""

    def __init__(self, dev):
        self.dev, self.bufs = dev, []

    def _raw(self, nbytes):
        buf = torch.full((2 * GUARD + (nbytes + 15) // 16 * 16,), 0xFF, dtype=torch.uint8, device=self.dev)
        self.bufs.append((buf, nbytes))
        return buf[GUARD:GUARD + nbytes]

    def new(self, shape, dtype, zero=False):
        """A NaN-filled (0xFF bytes; ``zero``: zero-filled) tensor between two guards."""
        shape = tuple(int(s) for s in shape)
        n = 1
        for s in shape:
            n *= s
        v = self._raw(n * torch.empty((), dtype=dtype).element_size()).view(dtype).view(shape)
        if zero:
            v.zero_()
        return v

    def put(self, t):
        """A copy of ``t`` inside a NaN arena (None stays None)."""
        if t is None:
            return None
        v = self.new(t.shape, t.dtype)
        v.copy_(t)
        return v

    def check(self):
        torch.cuda.synchronize()
        for i, (buf, nbytes) in enumerate(self.bufs):
            ok = bool((buf[:GUARD] == 0xFF).all()) and bool((buf[GUARD + nbytes:] == 0xFF).all())
            assert ok, f"buffer {i} ({nbytes} bytes): a kernel wrote outside its tensor"


class _GuardedTorch:
    """``torch`` as ops/_native_conv.py and ops/_native_gemm.py see it: allocations come from the arena."""

    def __init__(self, arena):
        self._arena = arena

    def __getattr__(self, name):
        return getattr(torch, name)

    def _alloc(self, size, dtype, device, zero):
        if len(size) == 1 and isinstance(size[0], (tuple, list, torch.Size)):
            size = tuple(size[0])
        if device is None or torch.device(device).type != "cuda":
            return (torch.zeros if zero else torch.empty)(*size, dtype=dtype, device=device)
        return self._arena.new(size, dtype or F32, zero)

    def empty(self, *size, dtype=None, device=None):
        return self._alloc(size, dtype, device, False)

    def zeros(self, *size, dtype=None, device=None):
        return self._alloc(size, dtype, device, True)


@pytest.fixture
def env(monkeypatch):
    dev = gpu_device()
    from databricks_distributed_deep_learning_amd.ops import _lib
    from databricks_distributed_deep_learning_amd.ops import _native_conv as NC
    from databricks_distributed_deep_learning_amd.ops import _native_gemm as NG
    arena = Arena(dev)
    proxy = _GuardedTorch(arena)
    monkeypatch.setattr(NC, "torch", proxy)
    monkeypatch.setattr(NG, "torch", proxy)
    calls, real_fn = [], _lib.fn

    def fn(name):
        calls.append(name)
        return real_fn(name)
    monkeypatch.setattr(_lib, "fn", fn)
    e = SimpleNamespace(dev=dev, arena=arena, calls=calls, NC=NC, NG=NG, put=arena.put, new=arena.new)
    yield e
    arena.check()


def _ran(env):
    """The native entry points called since the last look (which kernel a forced kind really ran)."""
    names = [c for c in env.calls if c not in ("ddl_conv_w_dgrad", "ddl_gemm_bnb")]
    del env.calls[:]
    return "+".join(sorted(set(names)))


# ---------------------------------------------------------------------------- the two checks
def _check(tier, label, got, r, out_dtype, fails, bf16_partials=False):
    """Exact tier: bit equality with the oracle.  Real tier: prints max(|err| / tol), must be <= 1."""
    dev = got.device
    ref = r.ref.to(dev)
    assert got.shape == ref.shape, f"{label}: shape {tuple(got.shape)} vs {tuple(ref.shape)}"
    if tier == "exact":
        if not torch.equal(got.double(), ref):
            bad = (got.double() != ref) | torch.isnan(got.double())
            idx = bad.nonzero()[0].tolist()
            fails.append(f"{label}: {int(bad.sum())} of {bad.numel()} elements differ, first at {idx}: "
                         f"{float(got[tuple(idx)])} vs {float(ref[tuple(idx)])}")
        return
    q = O.ratio(got, ref, r.A.to(dev), r.n.to(dev), out_dtype, bf16_partials)
    print(f"RATIO {label} {q:.4f}")
    if not q <= 1.0:
        fails.append(f"{label}: max |err| / tol = {q:.4f}")


def _check_rows(tier, label, rows, want, absum, n, fails):
    """Statistics rows (summed in fp64): exact tier bit equality with ``want``; real tier within
    n 2^-24 absum of ``want`` (the fp64 sums of the kernel's own stored output)."""
    for i, (g, w_, a) in enumerate(zip(rows, want, absum)):
        g, w_, a = g.double(), w_.double().to(g.device), a.double().to(g.device)
        if tier == "exact":
            if not torch.equal(g, w_):
                fails.append(f"{label} row {i}: {int((g != w_).sum())} of {g.numel()} columns differ")
            continue
        t = n * 2.0 ** -24 * a
        err = (g - w_).abs()
        q = float(torch.where(err > 0, err / t, torch.zeros_like(err)).max()) if bool(torch.isfinite(g).all()) \
            else float("inf")
        print(f"RATIO {label}.row{i} {q:.4f}")
        if not q <= 1.0:
            fails.append(f"{label} row {i}: max |err| / tol = {q:.4f}")


def _done(fails):
    assert not fails, "\n".join(fails)


# ---------------------------------------------------------------------------- direct 3x3
DIRECT_IDS = [f"{n}x{h}x{w}-g{g}" for (n, h, w), g in O.DIRECT_SHAPES]


@pytest.mark.parametrize("tier", O.TIERS)
@pytest.mark.parametrize("shape,grid", O.DIRECT_SHAPES, ids=DIRECT_IDS)
def test_direct3x3_forward_stats(env, tier, shape, grid):
    """conv3x3_k<false>: the output and its BatchNorm statistics rows (one per workgroup)."""
    o, refs = O.direct_refs(tier, shape)
    N, H, W = shape
    x, w = env.put(o["x"].to(env.dev)), env.put(o["w"].to(env.dev))
    y = env.new((N, H, W, 64), BF)
    part = env.new((env.NC._direct3x3_rows(N * H * W) * 128,), F32)
    rows = env.NC._direct3x3(x, w, y, part, grid=grid)
    fails = []
    _check(tier, f"direct3x3.fwd {shape}", y, refs["fwd"], BF, fails)
    st = part[:rows * 128].view(rows, 2, 64).double().sum(0)
    _check_rows(tier, f"direct3x3.fwd.stats {shape}", (st[0], st[1]), O.bn_stats_rows(y),
                O.bn_stats_rows(y, absolute=True), N * H * W, fails)
    _done(fails)


@pytest.mark.parametrize("tier", O.TIERS)
@pytest.mark.parametrize("with_res", [False, True])
@pytest.mark.parametrize("with_mask", [False, True])
@pytest.mark.parametrize("shape,grid", O.DIRECT_SHAPES, ids=DIRECT_IDS)
def test_direct3x3_bn_backward_epilogue(env, tier, shape, grid, with_res, with_mask):
    """conv3x3_k<true>: dz = (conv + res) * mask and the rows sum dz, sum dz (x - mean) istd."""
    o, refs = O.direct_refs(tier, shape)
    N, H, W = shape
    dev = env.dev
    x, w = env.put(o["x"].to(dev)), env.put(o["w"].to(dev))
    res = env.put(o["res"].to(dev)) if with_res else None
    aux, mean, istd = env.put(o["aux"].to(dev)), env.put(o["mean"].to(dev)), env.put(o["istd"].to(dev))
    mask = env.put(O.pack_mask(o["bits"]).to(dev)) if with_mask else None
    hint = SimpleNamespace(x=aux, mask=mask, mean=mean, istd=istd)
    dz = env.new((N, H, W, 64), BF)
    part = env.new((env.NC._direct3x3_rows(N * H * W) * 128,), F32)
    rows = env.NC._direct3x3(x, w, dz, part, res=res, bnb=hint, grid=grid)
    fails = []
    label = f"direct3x3.bnb res{int(with_res)} mask{int(with_mask)} {shape}"
    _check(tier, label, dz, refs[f"bnb_res{int(with_res)}_mask{int(with_mask)}"], BF, fails)
    st = part[:rows * 128].view(rows, 2, 64).double().sum(0)
    _check_rows(tier, label + " stats", (st[0], st[1]), O.bnb_sums(dz, aux, mean, istd),
                O.bnb_sums(dz, aux, mean, istd, absolute=True), N * H * W + 3, fails)
    _done(fails)


@pytest.mark.parametrize("tier", O.TIERS)
@pytest.mark.parametrize("shape,grid", O.DIRECT_SHAPES, ids=DIRECT_IDS)
def test_direct3x3_dgrad(env, tier, shape, grid):
    """The input gradient through ``_dgrad`` (flipped, transposed weight layout + the direct kernel)."""
    o, refs = O.direct_refs(tier, shape)
    N, H, W = shape
    dy, w = env.put(o["x"].to(env.dev)), env.put(o["w"].to(env.dev))
    dx = env.NC._dgrad(dy, w, (N, H, W, 64), 1, 1)
    assert "ddl_conv3x3" in env.calls
    fails = []
    _check(tier, f"direct3x3.dgrad {shape}", dx, refs["dgrad"], BF, fails)
    _done(fails)


@pytest.mark.parametrize("tier", O.TIERS)
@pytest.mark.parametrize("out", ["fresh_bf16", "acc_bf16", "acc_f32"])
@pytest.mark.parametrize("shape,grid", O.DIRECT_SHAPES, ids=DIRECT_IDS)
def test_direct3x3_wgrad(env, tier, shape, grid, out):
    """conv3x3_wgrad_k + conv3x3_wgrad_reduce_k: into a fresh bf16 tensor, += a bf16 and an fp32 base."""
    o, refs = O.direct_refs(tier, shape)
    dy, x = env.put(o["dyg"].to(env.dev)), env.put(o["xg"].to(env.dev))
    dt = F32 if out == "acc_f32" else BF
    acc = out != "fresh_bf16"
    dw = env.put(o["base"].to(env.dev).to(dt)) if acc else env.new((64, 3, 3, 64), dt)
    env.NC._direct3x3_wgrad(dy, x, dw, acc, grid=grid)
    fails = []
    _check(tier, f"direct3x3.wgrad {out} {shape}", dw, refs["wgrad_acc" if acc else "wgrad"], dt, fails)
    _done(fails)


# ---------------------------------------------------------------------------- implicit GEMM
def _cid(c):
    return "x".join(str(v) for v in c)


STRIDED = [c for c in O.IGEMM_SHAPES if c[7] > 1]


@pytest.mark.parametrize("tier", O.TIERS)
@pytest.mark.parametrize("kind", O.FWD_KINDS, ids=str)
@pytest.mark.parametrize("case", O.IGEMM_SHAPES, ids=_cid)
def test_igemm_forward(env, tier, case, kind):
    """MODE_CONV through ``_fwd`` with each kernel kind forced (an ineligible kind runs another
    kernel: the entry point that ran is printed)."""
    o, refs = O.igemm_refs(tier, case)
    x, w = env.put(o["x"].to(env.dev)), env.put(o["w"].to(env.dev))
    with env.NG.force_kernel(kind):
        y = env.NC._fwd(x, w, case[7], case[8])
    print(f"RAN igemm.fwd {_cid(case)} forced={kind}: {_ran(env)}")
    fails = []
    _check(tier, f"igemm.fwd[{kind}] {_cid(case)}", y, refs["fwd"], BF, fails)
    _done(fails)


@pytest.mark.parametrize("tier", O.TIERS)
@pytest.mark.parametrize("kind", O.FWD_KINDS, ids=str)
@pytest.mark.parametrize("case", O.IGEMM_SHAPES, ids=_cid)
def test_igemm_dgrad(env, tier, case, kind):
    """``_dgrad`` with each kernel kind forced; stride 2 takes the per-class launches here (the other
    paths: test_igemm_strided_dgrad_paths).  Pixels of empty parity classes must be exactly zero (the
    oracle's are, and the real tier's tolerance is 0 where an element has no term)."""
    N, H, W, C, K, R, S, stride, pad = case
    o, refs = O.igemm_refs(tier, case)
    dy, w = env.put(o["dy"].to(env.dev)), env.put(o["wd"].to(env.dev))
    key = (tuple(dy.shape), tuple(w.shape), stride, pad)
    env.NC._MULTI_CHOICE[key] = "serial"
    try:
        with env.NG.force_kernel(kind):
            dx = env.NC._dgrad(dy, w, (N, H, W, C), stride, pad)
    finally:
        env.NC._MULTI_CHOICE.pop(key, None)
    print(f"RAN igemm.dgrad {_cid(case)} forced={kind}: {_ran(env)}")
    fails = []
    _check(tier, f"igemm.dgrad[{kind}] {_cid(case)}", dx, refs["dgrad"], BF, fails)
    _done(fails)


@pytest.mark.parametrize("tier", O.TIERS)
@pytest.mark.parametrize("path", O.DGRAD_PATHS)
@pytest.mark.parametrize("case", STRIDED, ids=_cid)
def test_igemm_strided_dgrad_paths(env, tier, case, path):
    """Stride-2 dgrad: per-class launches against the single multi-class launch (ddl_gemm_conv_multi,
    both tile widths); a shape with one non-empty class always takes the per-class launch."""
    N, H, W, C, K, R, S, stride, pad = case
    o, refs = O.igemm_refs(tier, case)
    dy, w = env.put(o["dy"].to(env.dev)), env.put(o["wd"].to(env.dev))
    key = (tuple(dy.shape), tuple(w.shape), stride, pad)
    env.NC._MULTI_CHOICE[key] = path
    try:
        dx = env.NC._dgrad(dy, w, (N, H, W, C), stride, pad)
    finally:
        env.NC._MULTI_CHOICE.pop(key, None)
    ran = _ran(env)
    print(f"RAN igemm.dgrad {_cid(case)} path={path}: {ran}")
    if path != "serial" and not (R == 1 and S == 1):
        assert "ddl_gemm_conv_multi" in ran
    fails = []
    _check(tier, f"igemm.dgrad[{path}] {_cid(case)}", dx, refs["dgrad"], BF, fails)
    _done(fails)


@pytest.mark.parametrize("tier", O.TIERS)
@pytest.mark.parametrize("case", STRIDED, ids=_cid)
def test_igemm_strided_dgrad_residual_in_place(env, tier, case):
    """The in-place ``serial(dx, dx)`` path: every class adds the residual where it writes, and pixels
    of empty classes keep the residual exactly."""
    N, H, W, C, K, R, S, stride, pad = case
    o, refs = O.igemm_refs(tier, case)
    dy, w = env.put(o["dy"].to(env.dev)), env.put(o["wd"].to(env.dev))
    res = env.put(o["res"].to(env.dev))
    dx = env.NC._dgrad(dy, w, (N, H, W, C), stride, pad, residual=res)
    assert dx.data_ptr() == res.data_ptr()
    fails = []
    _check(tier, f"igemm.dgrad[residual] {_cid(case)}", dx, refs["dgrad_res"], BF, fails)
    none = (O.conv_dgrad(O.ones(o["dy"]), O.ones(o["wd"]), (N, H, W, C), stride, pad) == 0).to(env.dev)
    if not torch.equal(dx[none], o["res"].to(env.dev)[none]):
        fails.append("pixels of empty classes lost the residual")
    _done(fails)


def _convw(env, dy, x, w_shape, stride, pad, dw, acc, kind, splits):
    N, H, W, C = x.shape
    K, R, S, _ = w_shape
    _, P, Q, _ = dy.shape
    NG = env.NG
    NG.gemm(NG.MODE_CONVW, dy, K, x, 0, dw, R * S * C, K, R * S * C, N * P * Q, accumulate=acc, kernel=kind,
            splits=splits, conv=env.NC._desc(N, H, W, C, P, Q, stride, -pad, -pad, 1, 1, R, S, P, Q))


@pytest.mark.parametrize("tier", O.TIERS)
@pytest.mark.parametrize("kind", O.WGRAD_KINDS, ids=str)
@pytest.mark.parametrize("case", O.IGEMM_SHAPES + [O.WG_SHAPE], ids=_cid)
def test_igemm_wgrad(env, tier, case, kind):
    """MODE_CONVW: ``_wgrad`` (kind None: the tuner's choice) or ``gemm(MODE_CONVW, splits=1 | 3)`` with
    the kind forced; into a fresh bf16 tensor, += a bf16 and an fp32 base."""
    _run_wgrad(env, tier, case, kind)


@pytest.mark.parametrize("tier", O.TIERS)
def test_igemm_wgrad_wg(env, tier):
    """The 4-wave weight-gradient kernel at the smallest shape of its contract (``wg_ok``); with a bf16
    output its partials are bf16 (the 2^-8 A term)."""
    N, H, W, C, K, R, S, stride, pad = O.WG_SHAPE
    P, Q = O.out_hw(H, W, R, S, stride, pad)
    assert env.NG.wg_ok(K, R * S * C, N * P * Q, K, 0)
    assert not env.NG.wg_ok(K, R * S * C, N * P * Q - 128, K, 0) and not env.NG.wg_ok(K - 128, R * S * C, 128, K, 0)
    _run_wgrad(env, tier, O.WG_SHAPE, "wg")


def _run_wgrad(env, tier, case, kind):
    N, H, W, C, K, R, S, stride, pad = case
    o, refs = O.igemm_refs(tier, case)
    dy, x = env.put(o["dyg"].to(env.dev)), env.put(o["xg"].to(env.dev))
    fails = []
    for splits in ((None,) if kind is None else (1, 3)):
        for out in ("fresh_bf16", "acc_bf16", "acc_f32"):
            dt = F32 if out == "acc_f32" else BF
            acc = out != "fresh_bf16"
            dw = env.put(o["base"].to(env.dev).to(dt)) if acc else env.new((K, R, S, C), dt)
            if kind is None:
                got = env.NC._wgrad(dy, x, (K, R, S, C), stride, pad, out=dw if acc else None)
            else:
                _convw(env, dy, x, (K, R, S, C), stride, pad, dw, acc, kind, splits)
                got = dw
            ran = _ran(env)
            print(f"RAN igemm.wgrad {_cid(case)} forced={kind} splits={splits} {out}: {ran}")
            if kind == "wg":
                assert ran == "ddl_gemm_wgrad"
            _check(tier, f"igemm.wgrad[{kind}] s{splits} {out} {_cid(case)}", got,
                   refs["wgrad_acc" if acc else "wgrad"], dt, fails,
                   bf16_partials=(kind == "wg" and dt == BF))
    _done(fails)


# ---------------------------------------------------------------------------- stem
class _Rec:
    def set(self, y, part, rows):
        self.part, self.rows = part, rows


@pytest.mark.parametrize("tier", O.TIERS)
@pytest.mark.parametrize("with_stats", [False, True])
@pytest.mark.parametrize("shape,grid", O.STEM_FWD_SHAPES, ids=lambda v: str(v).replace(" ", ""))
def test_stem_forward_kernel(env, tier, shape, grid, with_stats):
    """stem_conv.hip forward on space-to-depth operands that are dense in all 16 channels and taps."""
    o, refs = O.stem_refs(tier, shape)
    N, P, Q = shape
    xs, ws = env.put(o["xs"].to(env.dev)), env.put(o["ws"].to(env.dev))
    assert env.NC._stem_fwd_ok(xs, ws)
    rec = _Rec() if with_stats else None
    y = env.NC._stem_fwd(xs, ws, rec, grid=grid)
    fails = []
    _check(tier, f"stem.fwd {shape}", y, refs["fwd"], BF, fails)
    if with_stats:
        st = rec.part[:rec.rows * 128].view(rec.rows, 2, 64).double().sum(0)
        _check_rows(tier, f"stem.fwd.stats {shape}", (st[0], st[1]), O.bn_stats_rows(y),
                    O.bn_stats_rows(y, absolute=True), N * P * Q, fails)
    _done(fails)


@pytest.mark.parametrize("tier", O.TIERS)
@pytest.mark.parametrize("out", ["fresh_bf16", "acc_f32"])
@pytest.mark.parametrize("shape,grid", O.STEM_WGRAD_SHAPES, ids=lambda v: str(v).replace(" ", ""))
def test_stem_wgrad_kernel(env, tier, shape, grid, out):
    """stem_conv.hip weight gradient, written in the original [64,7,7,3] layout: the eighth tap row /
    column and the fourth channel of the (dense) space-to-depth operands must drop out."""
    o, refs = O.stem_refs(tier, shape)
    xs, dy = env.put(o["xg"].to(env.dev)), env.put(o["dyg"].to(env.dev))
    assert env.NC._stem_wgrad_ok(xs, dy, (64, 4, 4, 16), (64, 7, 7, 3))
    acc = out == "acc_f32"
    dw = env.put(o["base"].to(env.dev)) if acc else env.new((64, 7, 7, 3), BF)
    env.NC._stem_wgrad(xs, dy, dw, acc, grid=grid)
    fails = []
    _check(tier, f"stem.wgrad {out} {shape}", dw, refs["wgrad_acc" if acc else "wgrad"], F32 if acc else BF, fails)
    _done(fails)


@pytest.mark.parametrize("tier", O.TIERS)
@pytest.mark.parametrize("shape", O.STEM_PATH_SHAPES, ids=lambda v: "x".join(map(str, v)))
def test_stem_whole_path(env, tier, shape):
    """``ops.conv2d(x[N,H,W,3], w[64,7,7,3], 2, 3)`` and its weight gradient against the original 7x7
    stride-2 convolution: 32x32 runs the direct kernels, 13x37 the general fallback.  Equality in the
    exact tier shows that the taps past 7 and the fourth channel contribute nothing."""
    from databricks_distributed_deep_learning_amd.ops.conv import conv2d
    o, refs = O.stem_path_refs(tier, shape)
    fails = []
    x, w = env.put(o["x"].to(env.dev)), env.put(o["w"].to(env.dev)).requires_grad_()
    y = conv2d(x, w, 2, 3)
    ran = _ran(env)
    print(f"RAN stem.path.fwd {shape}: {ran}")
    assert ("ddl_stem_fwd" in ran) == (shape[1] == 32)
    _check(tier, f"stem.path.fwd {shape}", y.detach(), refs["fwd"], BF, fails)
    xg, dy = env.put(o["xg"].to(env.dev)), env.put(o["dyg"].to(env.dev))
    conv2d(xg, w, 2, 3).backward(dy)
    ran = _ran(env)
    print(f"RAN stem.path.wgrad {shape}: {ran}")
    assert ("ddl_stem_wgrad" in ran) == (shape[1] == 32)
    _check(tier, f"stem.path.wgrad {shape}", w.grad, refs["wgrad"], BF, fails)
    _done(fails)


# ---------------------------------------------------------------------------- patch embedding
@pytest.mark.parametrize("tier", O.TIERS)
def test_patch_embedding(env, tier):
    """``patch_embed`` with a bias: the forward, dW and db."""
    from databricks_distributed_deep_learning_amd.ops.conv import patch_embed
    o, refs = O.patch_refs(tier)
    P = O.PATCH_SHAPE[4]
    fails = []
    x = env.put(o["x"].to(env.dev))
    w, b = env.put(o["w"].to(env.dev)).requires_grad_(), env.put(o["b"].to(env.dev)).requires_grad_()
    y = patch_embed(x, w, b, P)
    print(f"RAN patch.fwd: {_ran(env)}")
    _check(tier, "patch.fwd", y.detach(), refs["fwd"], BF, fails)
    xg, dy = env.put(o["xg"].to(env.dev)), env.put(o["dy"].to(env.dev))
    patch_embed(xg, w, b, P).backward(dy)
    print(f"RAN patch.bwd: {_ran(env)}")
    _check(tier, "patch.dw", w.grad, refs["dw"], BF, fails)
    _check(tier, "patch.db", b.grad, refs["db"], BF, fails)
    _done(fails)
