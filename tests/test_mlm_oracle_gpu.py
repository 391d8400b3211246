"""The kernels of ``csrc/kernels/mlm_loss.hip`` against an fp64 oracle (GPU only): ``ddl_ce_lse`` /
``ddl_ce_bwd`` (cross-entropy with ignored targets), the fused vocabulary head around them
(``ops.linear_cross_entropy``) and ``ddl_gather_rows`` / ``ddl_scatter_rows``.

Every case draws its inputs once on the CPU (``*_inputs``: a seeded generator, so that
``test_mlm_oracle_cpu.py`` rebuilds the very same tensors), rounds them to the case dtype and hands the
rounded values to the kernel, to the oracle (``mlm_oracle`` in fp64) and to the emulation (the same code
in fp32, every stored tensor rounded once); the references run on the CPU.  Per tensor
    max|kernel - ref64| <= M * max|emu - ref64| + 1/2 ulp(max|ref64|)
    rms(kernel - ref64) <= M * rms(emu - ref64) + 1/2 ulp(rms(ref64))
(``norm_oracle.bound``; ``M_STORE`` for tensors stored in the case dtype, ``M_F32`` for the fp32 side
outputs lse, row loss, loss and 1 / n_valid).  Gather and scatter move bits and are compared bit for bit.
Every output buffer lies between two runs of sentinel bytes that must survive (``Guard`` of
``test_elementwise_oracle_gpu.py``: the test's own buffers and, under ``G.ops()``, the ones the bindings
allocate); the logits' pad columns [C, ld) hold 0xFF bytes (NaN) on input.

Measured on an MI355X (4473 comparisons, 90 tests, the whole file in 5.7 s), largest (error - ulp term) /
emulation error per tensor kind, the larger of the max and rms forms:
  stored tensors, fp32:  dlogits 1.48 (M = 3, C = 9, one valid row) and 1.42 (M = 255, C = 1000); every other
      case <= 1.33.  Both are above M_STORE / 1.5 and below M_STORE; they sit on ``ce_bwd_k``'s
      ``__expf(v[j] - l)``: the emulation already carries that intrinsic's named product rounding
      (``mlm_oracle._exp_bwd``), what is left is the hardware exp2's own last bit.
  stored tensors, bf16:  dlogits 0.05, head dx 0.43, dW 0.38, db 0.43, logits <= 0 (one rounding of an fp32 result;
      no split-K plan with bf16 partials was met at K = 128, M <= 130).
  fp32 side outputs:     lse 0.53, row losses (lse - x[label], formed by the test) 1.00, loss 0.40 in fp32 and 1.00
      in bf16 (the head, M = 10, V = 1000), the head's loss against the oracle of its own returned logits <= 0,
      1 / n_valid exact.
Margins in force: M_STORE = 2, M_F32 = 4, the project's figures for this class of kernel (one rounding of an fp32
result; ``__expf`` / ``logf`` against torch's, measured 2.45 by the elementwise CE cases).  Nothing was raised.

A second finding, in the row losses the mean is taken over.  With suspect 1 fixed, the loss of bf16 M = 3,
C = 8191 and C = 32769 (every row valid) was still 4.241e-06 and 3.633e-06 from fp64 where the emulation is
4.266e-07 and 1.813e-07 off (+ half ulp 1.907e-06: ratios 5.47 and 9.52).  Traced to ``row_loss[row] = l -
to_f(x[lab])`` of the two lse kernels: the +-80 row's loss is 164, so that fp32 subtraction (after the fp32 ``m +
logf(s)``) leaves it 6.3e-06 off, a third of which reaches a mean of ~56 (ulp 3.8e-06) and, next to a rounding
midpoint, costs it a whole ulp.  The row losses are now formed and kept in fp64, ``(m + log(s)) - x[label]`` from
the fp32 m, s and x[label] (``lse`` itself keeps its bits): both cases <= 0, no loss above 1.00.

The five suspects:
  1. fp32 sum in ``ce_finish_k``: CONFIRMED and fixed (fp64 partials and tree, one conversion, as ``mean_k``).
     Loss ratio before / after, fp32, C = 1000, every row valid, one row spread over +-1e4:
     M = 300 (``test_ce_saturated_mean``) 3.24 / -1.24 -- above M_F32 / 1.5, yet it did not fail as predicted;
     M = 257 3.10 / -1.10; M = 1025 4.54 / -2.54 and M = 300 with every third row ignored 7.89 / <= 0: without
     the fix ``test_ce_rows[1025-fp32]`` and ``test_ce_rows[300-fp32]`` fail.  (The "before" figures are the
     parent's kernel; the saturated case is still at -1.24 with the fp64 row losses of the second finding.)
  2. loader switches: REFUTED.  8191 / 8192 / 8193 and 32767 / 32768 / 32769 with both layouts meet the bounds.
  3. out-of-range labels: REFUTED.  -1, C, ld - 1, 2^31 + 1 and 2^32 + 3 all count as ignored at every C.
  4. n_valid through the shuffles and the LDS counts: REFUTED (M up to 1025, one wave holding every count, a
     single valid row first or last): 1 / n_valid is exact everywhere.
  5. gather / scatter: REFUTED.  D = 8 / 136 / 1024, both index forms, out-of-range positions, ``labels=None`` and
     the second grid trip (16400 x 1024) are bit-exact and stay inside their buffers.
"""
import functools
import math

import pytest
import torch

import mlm_oracle as MO
from conftest import gpu_device
from test_elementwise_oracle_gpu import Guard

pytestmark = pytest.mark.gpu

M_STORE = 2.0
M_F32 = 4.0
IGN = -100
BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
DTYPES = [F32, BF16]
UPSTREAMS = [1.0, 2.0, 65536.0]

# 8192 and 32768 are launch_lse's switches (register form with 4 vectors per thread, with 16, streaming)
CE_CS = [1, 2, 7, 8, 9, 255, 257, 1000, 2047, 2048, 2049, 8191, 8192, 8193, 30522, 32767, 32768, 32769]
OOR = ["oor_neg1", "oor_C", "oor_ldm1", "oor_2p31", "oor_2p32"]
IGNORE_PATTERNS = ["none", "third", "all", "one"]
CE_PATTERNS = IGNORE_PATTERNS + OOR
ROWS_C = 1000
ROWS_MS = [1, 255, 256, 257, 300, 1025]
SAT_M = 300
PUBLIC_CS = [1000, 1002, 8193]

HEAD_K = 128
HEAD_MS = [10, 130]
HEAD_VS = [1000, 1002, 8200]          # no pad, a pad of 6, the 16-vector loader behind the GEMM

GS_DS = [8, 136, 1024]
BIG_N, BIG_D = 16400, 1024            # 16400 * 128 vectors > 8192 * 256: the grid makes a second trip


def _lib():
    from databricks_distributed_deep_learning_amd.ops import _lib
    assert _lib.available(), _lib.load_error()
    return _lib


def _name(dt):
    return "bf16" if dt == BF16 else "fp32"


def _gen(key):
    return torch.Generator().manual_seed(key)


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF16 else torch.int32)


def check(got, ref64, emu, dtype, M, label, fails):
    MO.bound(got.detach().cpu(), ref64, emu, dtype, M, label, fails)


def finish(fails):
    assert not fails, "; ".join(fails)


def roundup8(n):
    return (n + 7) // 8 * 8


# ================================================================== cross-entropy inputs
def ce_inputs(dtype, M, C, key=0):
    """Logits randn * 3 and the labels of the pattern "none".  M >= 3: row 0 is -inf everywhere but at its
    label (column 0) and one other column (C > 2), row 1 has the label C - 1, row 2 is spread over
    +-80 (bf16) / +-1e4 (fp32) with its lowest value at its label, which lies in the last partial
    vector [C - C % 8, C) when there is one.  M < 3: every label is C - 1 and row 0 is the spread one."""
    gen = _gen(5000 + 31 * M + C + key)
    x = torch.randn(M, C, generator=gen, dtype=F32) * 3
    lab = torch.randint(0, C, (M,), generator=gen)
    r_inf, r_spread = (0, 2) if M >= 3 else (None, 0)
    if M >= 3:
        lab[0], lab[1] = 0, C - 1
        if C % 8:
            lab[2] = C - C % 8
    else:
        lab[:] = C - 1
    if C > 1:
        S = 80.0 if dtype == BF16 else 1e4
        row = torch.linspace(-S, S, C)[torch.randperm(C, generator=gen)]
        lo, at = int(row.argmin()), int(lab[r_spread])
        row[lo], row[at] = row[at].clone(), row[lo].clone()
        x[r_spread] = row
    if r_inf is not None and C > 2:
        keep = torch.zeros(C, dtype=torch.bool)
        keep[lab[r_inf]] = True
        keep[(int(lab[r_inf]) + 1 + int(torch.randint(0, C - 1, (1,), generator=gen))) % C] = True
        x[r_inf, ~keep] = -math.inf
    return x.to(dtype), lab


def ce_labels(base, pattern, C, ld):
    """The labels of a pattern, or None where the pattern does not exist (``oor_ldm1`` at ld = C)."""
    y = base.clone()
    M = y.numel()
    rows = torch.arange(M)
    if pattern == "third":
        y[::3] = IGN
    elif pattern == "all":
        y[:] = IGN
    elif pattern == "one":                       # exactly one valid row
        y[rows != min(1, M - 1)] = IGN
    elif pattern == "last":                      # the only valid row is the last one
        y[:M - 1] = IGN
    elif pattern == "wave3":                     # one wave of ce_finish_k holds every count
        y[rows % 256 < 192] = IGN
    elif pattern in OOR:                         # row 0: a label outside [0, C), not the ignore index
        if pattern == "oor_ldm1" and ld - 1 < C:
            return None
        y[0] = {"oor_neg1": -1, "oor_C": C, "oor_ldm1": ld - 1, "oor_2p31": 2 ** 31 + 1,
                "oor_2p32": 2 ** 32 + 3}[pattern]
    else:
        assert pattern == "none", pattern
    return y


def pad_nan(x, ld):
    """[M, ld] storage whose columns [C, ld) hold 0xFF bytes (a NaN in either dtype)."""
    M, C = x.shape
    size = torch.empty((), dtype=x.dtype).element_size()
    out = torch.full((M, ld * size), 0xFF, dtype=torch.uint8).view(x.dtype)
    out[:, :C] = x
    return out


@functools.lru_cache(maxsize=None)
def _ce_case(dtype, M, C):
    return ce_inputs(dtype, M, C)


_REFS = {}


def ce_refs(dtype, M, C, y, up):
    """(oracle, emulation) of a case: computed once per label vector and upstream, never changed."""
    key = (dtype, M, C, tuple(y.tolist()) if M <= 16 else hash(tuple(y.tolist())), up)
    if key not in _REFS:
        if len(_REFS) > 64:
            _REFS.clear()
        x, _ = _ce_case(dtype, M, C)
        _REFS[key] = (MO.ce_ignore_ref(x, y, IGN, up, F64), MO.ce_ignore_ref(x, y, IGN, up, F32))
    return _REFS[key]


def run_ce(xp, C, y, ups):
    """The entry points on ``xp [M, ld]`` (device): (loss, lse, inv_n, [dlogits per upstream]).  Outputs
    are guarded; the fresh-buffer backward must leave its source alone and agree bitwise with the
    in-place one."""
    from databricks_distributed_deep_learning_amd.ops import _native_mlm as N
    M, ld = xp.shape
    G = Guard()
    with G.ops():
        loss, lse, inv_n = N._lse(xp, M, ld, C, y, IGN)
    G.check()
    keep = _bits(xp).clone()
    dls = []
    for up in ups:
        g = torch.full((), up, dtype=F32, device=xp.device)
        G = Guard()
        dl = G.alloc((M, ld), xp.dtype, xp.device)
        N._bwd(xp, M, ld, C, y, IGN, lse, g, inv_n, dl)
        inplace = G.like(xp, fill=xp)
        N._bwd(inplace, M, ld, C, y, IGN, lse, g, inv_n, inplace)
        torch.cuda.synchronize()
        G.check()
        assert torch.equal(_bits(xp), keep), "the fresh-buffer backward wrote to its source"
        assert torch.equal(_bits(dl), _bits(inplace)), "in-place backward differs"
        dls.append(dl)
    return loss, lse, inv_n, dls


def check_ce(dtype, x, xp, C, y, ups, label, fails, out=None):
    """Runs the entry points and compares every output with the oracle of ``x [M, C]``."""
    M, ld = xp.shape
    dev = xp.device
    loss, lse, inv_n, dls = run_ce(xp, C, y.to(dev), ups)
    assert loss.dtype == F32 and lse.dtype == F32 and inv_n.dtype == F32
    r64, e32 = ce_refs(dtype, M, C, y, ups[0])
    v, n = r64.valid, r64.n_valid
    assert n == int(MO.valid_rows(y, IGN, C).sum())
    want_inv = float(torch.ones((), dtype=F32) / n) if n else 0.0
    assert inv_n.item() == want_inv, f"{label}: 1 / n_valid = {inv_n.item()!r}, n_valid = {n}"
    check(inv_n.reshape(()), r64.inv_n, e32.inv_n, F32, M_F32, f"{label} inv_n", fails)
    assert math.isfinite(loss.item()), f"{label}: loss {loss.item()}"
    if n:
        lse_k = lse.cpu()[v]
        row_k = lse_k - x.float()[v].gather(1, y[v].view(-1, 1)).squeeze(1)     # the kernel's own subtraction
        check(lse_k, r64.lse[v], e32.lse[v], F32, M_F32, f"{label} lse", fails)
        check(row_k, r64.row_loss[v], e32.row_loss[v], F32, M_F32, f"{label} row loss", fails)
    else:
        assert loss.item() == 0.0, f"{label}: loss {loss.item()} with no valid row"
    check(loss, r64.loss, e32.loss, F32, M_F32, f"{label} loss", fails)
    for up, dl in zip(ups, dls):
        r64, e32 = ce_refs(dtype, M, C, y, up)
        d = dl.cpu()
        assert bool(torch.isfinite(d.float()).all()), f"{label}: gradient not finite"
        if ld > C:
            assert bool((_bits(d[:, C:]) == 0).all()), f"{label}: pad columns of the gradient are not exact zeros"
        if n < M:
            assert bool((d[~v] == 0).all()), f"{label}: rows without a valid label are not exact zeros"
        check(d[:, :C], r64.dlogits, e32.dlogits, dtype, M_STORE, f"{label} dlogits x{up:g}", fails)
    if out is not None:
        out.append((loss.clone(), lse.cpu()[v], inv_n.clone(), [d.clone() for d in dls]))


# ================================================================== cross-entropy: columns, layouts, labels
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("C", CE_CS)
def test_ce_columns(dtype, C):
    """M = 3 rows of C columns in both layouts, every pattern of ignored rows, every upstream factor."""
    dev = gpu_device()
    _lib()
    M = 3
    x, base = _ce_case(dtype, M, C)
    fails = []
    for ld in (roundup8(C), roundup8(C) + 8):
        xp = pad_nan(x, ld).to(dev)
        for pattern in IGNORE_PATTERNS:
            y = ce_labels(base, pattern, C, ld)
            check_ce(dtype, x, xp, C, y, UPSTREAMS, f"{_name(dtype)} M={M} C={C} ld={ld} {pattern}", fails)
    finish(fails)


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("pattern", OOR)
def test_ce_out_of_range_labels(dtype, pattern):
    """Row 0 carries a label outside [0, C) that is not the ignore index: by ``row_valid``'s documented
    contract the row counts as ignored -- not in n_valid, an exact-zero gradient row, a finite loss.
    (``oor_C`` / ``oor_ldm1`` name a NaN pad column of the row when ld > C; 2^32 + 3 is column 3 once
    truncated to 32 bits.)"""
    dev = gpu_device()
    _lib()
    M = 3
    fails = []
    for C in CE_CS:
        x, base = _ce_case(dtype, M, C)
        for ld in (roundup8(C), roundup8(C) + 8):
            y = ce_labels(base, pattern, C, ld)
            if y is None:
                continue
            check_ce(dtype, x, pad_nan(x, ld).to(dev), C, y, [2.0], f"{_name(dtype)} M={M} C={C} ld={ld} {pattern}",
                     fails)
    finish(fails)


# ================================================================== cross-entropy: rows and the reduction
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("M", ROWS_MS)
def test_ce_rows(dtype, M):
    """n_valid and the mean where they depend on ce_finish_k's strided loop, shuffles and LDS counts."""
    dev = gpu_device()
    _lib()
    C = ROWS_C
    x, base = _ce_case(dtype, M, C)
    fails = []
    patterns = ["none", "third", "one", "last"] + (["wave3"] if M == 1025 else [])
    for ld in (C, C + 8):
        xp = pad_nan(x, ld).to(dev)
        for pattern in patterns:
            y = ce_labels(base, pattern, C, ld)
            if pattern == "wave3":
                assert int(MO.valid_rows(y, IGN, C).sum()) == 256
            runs = []
            check_ce(dtype, x, xp, C, y, [2.0], f"{_name(dtype)} M={M} C={C} ld={ld} {pattern}", fails, runs)
            if ld == C:                                            # twice: the same bits
                check_ce(dtype, x, xp, C, y, [2.0], f"{_name(dtype)} M={M} C={C} ld={ld} {pattern} again", [], runs)
                a, b = runs
                assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
                assert torch.equal(_bits(a[3][0]), _bits(b[3][0])), "not repeatable"
    finish(fails)


def test_ce_saturated_mean():
    """One row with a loss of ~2e4 among 299 of ~8 (fp32, M = 300, C = 1000, every row valid): the mean
    of the row losses must stay as close to fp64 as an fp32 emulation's."""
    dev = gpu_device()
    _lib()
    M, C = SAT_M, ROWS_C
    x, base = _ce_case(F32, M, C)
    fails = []
    check_ce(F32, x, pad_nan(x, C).to(dev), C, base, [1.0], f"saturated fp32 M={M} C={C}", fails)
    finish(fails)


# ================================================================== cross-entropy: the public op
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("C", PUBLIC_CS)
def test_ce_public_op(dtype, C):
    """``ops.cross_entropy(ignore_index=...)`` on unpadded logits (through the ``copy2d`` pad when C % 8):
    the bits of the entry points, in the loss and in autograd's gradient; twice."""
    from databricks_distributed_deep_learning_amd import ops
    dev = gpu_device()
    _lib()
    M = 3
    x, base = _ce_case(dtype, M, C)
    ld = roundup8(C)
    xp = pad_nan(x, ld).to(dev)
    for pattern in ("none", "third", "oor_C"):
        y = ce_labels(base, pattern, C, ld).to(dev)
        loss, _, _, (dl,) = run_ce(xp, C, y, [2.0])
        for _ in range(2):
            xc = x.to(dev).requires_grad_(True)
            G = Guard()
            with G.ops():
                l2 = ops.cross_entropy(xc, y, ignore_index=IGN)
                assert type(l2.grad_fn).__name__ == "_CEIgnoreBackward", l2.grad_fn
                (l2 * 2).backward()
            G.check()
            assert torch.equal(l2.detach(), loss), f"{pattern}: public loss {l2.item()!r} != {loss.item()!r}"
            assert torch.equal(_bits(xc.grad), _bits(dl[:, :C])), f"{pattern}: public gradient differs"


# ================================================================== fused head
def head_inputs(M, K, V, key=0):
    """x, W (* 0.1), b (* 0.1) in bf16 and labels: every third row ignored, row 1 on V - 1, row 4 on 0,
    row 2 out of range (the label V: a pad column of the padded logits, or the next row's column 0)."""
    gen = _gen(7000 + M * 31 + V + key)
    x = torch.randn(M, K, generator=gen).bfloat16()
    w = (torch.randn(V, K, generator=gen) * 0.1).bfloat16()
    b = (torch.randn(V, generator=gen) * 0.1).bfloat16()
    y = torch.randint(0, V, (M,), generator=gen)
    y[::3] = IGN
    y[1], y[4], y[2] = V - 1, 0, V
    return x, w, b, y


@functools.lru_cache(maxsize=None)
def _head_refs(M, V, bias, up):
    x, w, b, y = head_inputs(M, HEAD_K, V)
    b = b if bias else None
    return MO.head_ref(x, w, b, y, IGN, up, F64), MO.head_ref(x, w, b, y, IGN, up, F32)


@pytest.mark.parametrize("bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("M", HEAD_MS)
@pytest.mark.parametrize("V", HEAD_VS)
def test_linear_cross_entropy_oracle(V, M, bias):
    from databricks_distributed_deep_learning_amd import ops
    dev = gpu_device()
    _lib()
    x, w, b, y = head_inputs(M, HEAD_K, V)
    yd = y.to(dev)
    fails = []
    for up in (1.0, 65536.0):
        label = f"head M={M} K={HEAD_K} V={V} {'bias' if bias else 'nobias'} x{up:g}"
        runs = []
        for _ in range(2):
            xg, wg = (t.to(dev).requires_grad_(True) for t in (x, w))
            bg = b.to(dev).requires_grad_(True) if bias else None
            G = Guard()
            with G.ops():
                loss = ops.linear_cross_entropy(xg, wg, bg, yd, IGN)
                assert type(loss.grad_fn).__name__ == "_LinearCEBackward", loss.grad_fn
                (loss * up).backward()
            G.check()
            runs.append([loss.detach(), xg.grad, wg.grad] + ([bg.grad] if bias else []))
        for a, c in zip(*runs):
            assert torch.equal(a, c), f"{label}: not repeatable"
        r64, e32 = _head_refs(M, V, bias, up)
        got = runs[0]
        assert got[0].dtype == F32
        check(got[0], r64.loss, e32.loss, F32, M_F32, f"{label} loss", fails)
        check(got[1], r64.dx, e32.dx, BF16, M_STORE, f"{label} dx", fails)
        check(got[2], r64.dW, e32.dW, BF16, M_STORE, f"{label} dW", fails)
        if bias:
            check(got[3], r64.db, e32.db, BF16, M_STORE, f"{label} db", fails)
    # the CE kernels alone, at the head's real layout: the loss against the oracle of the returned logits
    label = f"head M={M} K={HEAD_K} V={V} {'bias' if bias else 'nobias'}"
    G = Guard()
    with G.ops():
        loss, logits = ops.linear_cross_entropy(x.to(dev), w.to(dev), b.to(dev) if bias else None, yd, IGN,
                                                return_logits=True)
    G.check()
    assert logits.shape == (M, V) and logits.dtype == BF16
    assert torch.equal(loss, runs[0][0]), f"{label}: the loss changes with return_logits"
    lg = logits.cpu()
    check(loss, MO.ce_ignore_ref(lg, y, IGN, 1.0, F64).loss, MO.ce_ignore_ref(lg, y, IGN, 1.0, F32).loss, F32, M_F32,
          f"{label} loss of the returned logits", fails)
    check(lg, _head_refs(M, V, bias, 1.0)[0].logits, _head_refs(M, V, bias, 1.0)[1].logits, BF16, M_STORE,
          f"{label} logits", fails)
    finish(fails)


# ================================================================== gather / scatter
GS_R, GS_B, GS_S, GS_P = 96, 4, 24, 5


def gs_inputs(dtype, D, form, key=0):
    """h [R, D], positions, labels and dy for ``form``:
    "flat"  positions [n] into h [R, D]: unique valid positions that include rows 0 and R - 1, ignored
            slots on row 0 and on another valid slot's row, and three out-of-range positions (-1, R,
            R + 5) whose labels are valid;
    "seq"   positions [B, P] into h [B, S, D]: unique per sequence, rows 0 and S - 1 used, ignored slots
            on position 0."""
    gen = _gen(9000 + D + key)
    R = GS_R
    h = torch.randn(R, D, generator=gen).to(dtype)
    if form == "flat":
        pos = torch.tensor([0, R - 1, 17, 33, 64, 1, 50, 80, 0, 33, 0, -1, R, R + 5, 2])
        lab = torch.tensor([4, 9, 2, 7, 7, 1, 3, 8, IGN, IGN, IGN, 5, 6, 7, 0])
    else:
        pos = torch.stack([torch.randperm(GS_S, generator=gen)[:GS_P] for _ in range(GS_B)])
        lab = torch.randint(0, 50, (GS_B, GS_P), generator=gen)
        pos[0, 0], pos[GS_B - 1, 1] = 0, GS_S - 1
        pos[0, 1:] = torch.tensor([5, 9, 0, 0])
        pos[GS_B - 1, 0], pos[GS_B - 1, 2:] = 3, torch.tensor([7, 11, 0])
        lab[0, 3:], lab[GS_B - 1, 4] = IGN, IGN
        pos[1, 4], lab[1, 4] = pos[1, 0], IGN              # an ignored slot on a valid slot's row
    dy = torch.randn(pos.numel(), D, generator=gen).to(dtype)
    # the labels=None arm scatters every slot: positions that are unique over all slots
    if form == "flat":
        pos_u = torch.randperm(R, generator=gen)[:pos.numel()]
        pos_u[11:14] = torch.tensor([-1, R, R + 5])
    else:
        pos_u = torch.stack([torch.randperm(GS_S, generator=gen)[:GS_P] for _ in range(GS_B)])
    return h, pos, lab, dy, pos_u


def _gather_scatter(h, pos, lab, dy, dev):
    """``ops.gather_rows`` forward and backward under sentinels: (out, dh) on the CPU."""
    from databricks_distributed_deep_learning_amd import ops
    hd = h.to(dev).requires_grad_(True)
    G = Guard()
    with G.ops():
        out = ops.gather_rows(hd, pos.to(dev), None if lab is None else lab.to(dev), IGN)
        assert type(out.grad_fn).__name__ == "_GatherRowsBackward", out.grad_fn
        out.backward(dy.to(dev))
    G.check()
    return out.detach().cpu(), hd.grad.cpu()


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("form", ["flat", "seq"])
@pytest.mark.parametrize("D", GS_DS)
def test_gather_scatter_oracle(D, form, dtype):
    dev = gpu_device()
    _lib()
    h, pos_l, lab, dy, pos_u = gs_inputs(dtype, D, form)
    R = h.shape[0]
    P, S = (GS_P, GS_S) if form == "seq" else (0, 0)
    h_in = h.reshape(GS_B, GS_S, D) if form == "seq" else h
    for pos, labels in ((pos_l, lab), (pos_u, None)):
        for _ in range(2):                                        # twice: the same bits
            out, dh = _gather_scatter(h_in, pos, labels, dy, dev)
            want = MO.gather_ref(h, pos, P, S)
            assert torch.equal(_bits(out), _bits(want)), f"gather {form} D={D}"
            rows = MO.slot_rows(pos, P, S)
            oob = (rows < 0) | (rows >= R)
            assert bool((_bits(out[oob]) == 0).all()), "an out-of-range position did not give exact zeros"
            want_dh = MO.scatter_ref(dy, pos, labels, IGN, R, P, S).reshape(h_in.shape)
            assert torch.equal(_bits(dh), _bits(want_dh)), f"scatter {form} D={D} labels={labels is not None}"


def big_inputs():
    gen = _gen(9999)
    h = torch.randn(BIG_N, BIG_D, generator=gen).bfloat16()
    pos = torch.randperm(BIG_N, generator=gen)
    return h, pos


def test_gather_scatter_second_grid_trip():
    """n * D / 8 = 16400 * 128 vectors on a grid capped at 8192 * 256 threads: the slots past 2^21
    vectors are gathered and scattered too (a permutation: dh = scatter(gather(h)) is h again)."""
    dev = gpu_device()
    _lib()
    h, pos = big_inputs()
    assert BIG_N * (BIG_D // 8) > 8192 * 256
    lab = torch.zeros(BIG_N, dtype=torch.int64)
    lab[5::1000] = IGN
    out, dh = _gather_scatter(h, pos, lab, h[pos], dev)
    assert torch.equal(_bits(out), _bits(MO.gather_ref(h, pos))), "gather: second grid trip"
    assert torch.equal(_bits(dh), _bits(MO.scatter_ref(out, pos, lab, IGN, BIG_N))), "scatter: second grid trip"
    assert bool((_bits(dh[pos[lab == IGN]]) == 0).all()) and torch.equal(_bits(dh[pos[-1]]), _bits(h[pos[-1]]))
