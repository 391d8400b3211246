"""LayerNorm and BatchNorm kernels against an fp64 oracle (GPU only).

Every case draws its inputs once, rounds them to the case dtype and hands the rounded values to the
kernels, to the oracle (``norm_oracle.*_ref`` in fp64) and to the emulation (the same code in fp32
with every stored tensor rounded once).  gamma is ``rand + 0.5`` and beta ``randn * 0.3`` per column,
x, res, dy and add are independent ``randn``: a column, row or operand mix-up moves a result by
O(0.1 .. 1) while the bf16 yardstick is about 1e-2.  Per tensor
    max|kernel - ref64| <= M * max|emu - ref64| + 1/2 ulp(max|ref64|)
    rms(kernel - ref64) <= M * rms(emu - ref64) + 1/2 ulp(rms(ref64))
with ulp of the tensor's own format (``M_STORE`` for tensors stored in the case dtype, ``M_F32`` for
the fp32 side outputs: saved mean / rstd, running statistics, column sums).  Every comparison prints
its ratios ((kernel error - ulp term) / emulation error) before it asserts.

LayerNorm goes through ``ops.norm.layer_norm`` (so the Python dispatch is under test): every width
with every residual variant, the row-count edges (1, 3, 9, 4100 and 16400 rows), fused dropout,
``grad_from`` (fused ``ADD`` kernels and the late add), the gradient-arena sinks and the saved
statistics.  The column sums of dx that ride on the gradient are bounded twice: against the
oracle's, and against the fp64 column sums of the kernel's own stored dx with torch's fp32
``sum(0)`` of that same tensor as the yardstick.

BatchNorm (bf16, the training dtype) goes through ``ops.norm.batch_norm``: C = 8 .. 2048, two rows,
252 rows and a row count per C that is no multiple of the rows a block covers per iteration and
gives more than one statistics block; inputs with mean / std = 8; the inference path.  With a ReLU
the kernel's zero pattern must equal ``z > 0`` wherever the oracle's pre-activation has ``|z| > t``
(t: the right-hand side of the forward max inequality); inside that band, which may hold at most
3 % of a case's elements (``BAND_CAP``; ``test_norm_oracle_cpu.py`` checks every case on the oracle
alone), the gradients are compared under the kernel's own pattern.

Measured on an MI355X (1080 comparisons, all cases of this file), largest (error - ulp term) /
emulation error per tensor kind, max form (the rms form is never larger except where noted):
  stored tensors, bf16:  LN y <= 0, dx 0.99 (grad_from, H = 1280: the late add rounds twice), dres 0.46
      (H = 1536, broadcast), dgamma / dbeta <= 0, arena slots 0.36 (bias slot, H = 768); BatchNorm y, dx,
      dres, dgamma, dbeta <= 0 in the max form and 0.20 in the rms form (dx, C = 512, two rows);
      inference y <= 0.
  stored tensors, fp32:  LN dx 1.08 (H = 256, broadcast residual), dgamma 1.04 (H = 256, full residual),
      dres 0.97 (1 row, H = 768), dbeta 0.81, y 0.81 (H = 2048), arena slots 0.80.
  fp32 side outputs:     dx column sums 1.45 against the oracle (fp32, dropout, H = 256; bf16: 1.00, rms
      1.00) and 1.01 against the kernel's own dx; saved mean 1.16 (fp32, H = 2048), rstd 0.67; the sunk
      column sums 1.00; running_mean 0.72, running_var 1.18 -- after the fix below.
So M_STORE = 2 (1.08 * 1.5 < 2) and M_F32 = 4 (1.45 * 1.5 > 2).

running_var at mean / std = 8 was the finding of this file, in the statistics pass of ``ddl_bn_fwd_train``.
Its finalize summed the blocks' [sum | sumsq] partial rows in fp32 (ratio 22.6 at C = 64 with 100352 rows,
11.6 at C = 2048 with 3200 rows); it now sums them in fp64 (0.30 and 0.27).  That left one statistics
block of 252 rows at C = 64 at 5.47: the block's own fp32 sum of squares (about 16400) is one rounding of
2^-24 relative, which E[x^2] - mean^2 multiplies by mean^2 / var = 64.  The squares are now taken about a
pivot k, the mean of the first (up to 8) rows, and var = E[(x - k)^2] - (mean - k)^2: 0.20 in that case,
and 1.18 at most over all cases of this file (C = 8, 2697 rows, centred data, where the pivot is a little
worse than 0).  A single-row pivot was tried and is not enough: for centred data it costs (x0 - mean)^2 /
var, which reached 4.6 at C = 8.
"""
import pytest
import torch

import norm_oracle as NO
from conftest import gpu_device

pytestmark = pytest.mark.gpu

# margins over the emulation's own error: a different summation order, rsqrtf and DPP reductions in
# place of torch's (figures in the module docstring)
M_STORE = 2.0
M_F32 = 4.0
BAND_CAP = 0.03
BF16, F32 = torch.bfloat16, torch.float32
DTYPES = [F32, BF16]
LN_EPS = 1e-12
BN_EPS = 1e-5
MOMENTUM = 0.1


def _lib():
    from databricks_distributed_deep_learning_amd.ops import _lib
    assert _lib.available(), _lib.load_error()
    return _lib


def _name(dt):
    return "bf16" if dt == BF16 else "fp32"


# ================================================================== LayerNorm
class _Tap(torch.autograd.Function):
    """Stands where the producing Linear stands: its backward sees the very dx tensor the LayerNorm
    returned (and what rides on it)."""

    @staticmethod
    def forward(ctx, x, box):
        ctx.box = box
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        ctx.box.append(g)
        return g, None


def _draw_seed(key=123):
    """The seed the op will draw (``new_seed``), as ``test_layernorm_fused_dropout`` obtains it."""
    torch.manual_seed(key)
    seed = int(torch.randint(0, 2 ** 62, (1,)).item())
    torch.manual_seed(key)
    return seed


def ln_inputs(dev, dtype, lead, H, res, add, key):
    """x, g, b, res, dy, add of one case, rounded to ``dtype``.  ``lead``: the leading shape."""
    torch.manual_seed(key)
    mk = lambda *s: torch.randn(*s, device=dev).to(dtype)  # noqa: E731
    x = mk(*lead, H)
    g = (torch.rand(H, device=dev) + 0.5).to(dtype)
    b = (torch.randn(H, device=dev) * 0.3).to(dtype)
    r = None
    if res == "full":
        r = mk(*lead, H)
    elif res == "bcast":
        r = mk(1, *lead[1:], H)
    dy = mk(*lead, H)
    a = mk(*lead, H) if add else None
    return x, g, b, r, dy, a


def ln_run(x, g, b, r, dy, add, p=0.0, sinks=None):
    """One forward + backward through ``ops.norm.layer_norm``.  ``sinks``: None, or a dict that
    receives the arena slots and the ready counts (gamma / beta / producing-bias sinks armed)."""
    from databricks_distributed_deep_learning_amd.ops import norm
    from databricks_distributed_deep_learning_amd.ops.bridge import GradBridge
    _lib()
    dev, dtype, H = x.device, x.dtype, x.shape[-1]
    x0 = x.clone().requires_grad_(True)
    gp, bp = g.clone().requires_grad_(True), b.clone().requires_grad_(True)
    rp = None if r is None else r.clone().requires_grad_(True)
    box = []
    xin = _Tap.apply(x0, box)
    if sinks is not None:
        sinks["fired"] = {"g": 0, "b": 0}
        for name, prm in (("g", gp), ("b", bp)):
            prm._ddl_main_grad = torch.randn(H, device=dev).to(dtype)
            sinks[name + "_old"] = prm._ddl_main_grad.clone()
            prm._ddl_grad_ready = (lambda n: (lambda: sinks["fired"].__setitem__(n, sinks["fired"][n] + 1)))(name)
        lin_bias = torch.nn.Parameter(torch.zeros(H, device=dev, dtype=dtype))
        lin_bias._ddl_main_grad = torch.randn(H, device=dev).to(dtype)
        lin_bias._ddl_sunk = None
        sinks["bias_old"] = lin_bias._ddl_main_grad.clone()
        sinks["bias"] = lin_bias
        xin._ddl_bias_param = lin_bias
    bridge = GradBridge() if add is not None else None
    seed = _draw_seed() if p > 0 else None
    y = norm.layer_norm(xin, gp, bp, LN_EPS, rp, dropout=p, grad_from=bridge)
    if bridge is not None:
        bridge.put(add.clone())
    y.backward(dy)
    keep = None
    if p > 0:
        keep = NO.keep_mask(seed, x.shape, p, dev)
        assert 0.85 < keep.float().mean().item() < 0.95
    dxt = box[0]
    return dict(y=y.detach(), dx=x0.grad, dxt=dxt, colsum=getattr(dxt, "_ddl_colsum", None),
                dres=None if rp is None else rp.grad, dgamma=gp.grad, dbeta=bp.grad, keep=keep, gp=gp, bp=bp)


def ln_pair(x, g, b, r, dy, add, keep, p):
    return tuple(NO.ln_ref(x, g, b, LN_EPS, r, keep, p, dy, add, dt) for dt in (torch.float64, torch.float32))


def check_colsum(fails, label, got, ref, em):
    """The fp32 column sums riding on dx: against the oracle's, and against the kernel's own dx."""
    colsum, version = got["colsum"]
    dx = got["dxt"]
    assert version == dx._version
    assert colsum.dtype == F32
    assert torch.equal(dx, got["dx"])
    NO.bound(colsum, ref.dxsum, em.dxsum, F32, M_F32, f"{label} dxsum", fails)
    flat = dx.reshape(-1, dx.shape[-1])
    NO.bound(colsum, flat.double().sum(0), flat.float().sum(0), F32, M_F32, f"{label} dxsum-vs-own-dx", fails)


def check_ln(label, got, ref, em, dtype, colsum=True, params=True):
    fails = []
    NO.bound(got["y"], ref.y, em.y, dtype, M_STORE, f"{label} y", fails)
    NO.bound(got["dx"], ref.dx, em.dx, dtype, M_STORE, f"{label} dx", fails)
    if ref.dres is not None:
        assert got["dres"].shape == ref.dres.shape
        NO.bound(got["dres"], ref.dres, em.dres, dtype, M_STORE, f"{label} dres", fails)
    if params:
        NO.bound(got["dgamma"], ref.dgamma, em.dgamma, dtype, M_STORE, f"{label} dgamma", fails)
        NO.bound(got["dbeta"], ref.dbeta, em.dbeta, dtype, M_STORE, f"{label} dbeta", fails)
    if colsum:
        check_colsum(fails, label, got, ref, em)
    assert not fails, "\n".join(fails)


LN_WIDTHS = [256, 512, 768, 1024, 1280, 1536, 2048]


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("res", [None, "full", "bcast"])
@pytest.mark.parametrize("H", LN_WIDTHS)
def test_ln_every_width(H, res, dtype):
    dev = gpu_device()
    x, g, b, r, dy, _ = ln_inputs(dev, dtype, (3, 37), H, res, False, key=H + 1)
    got = ln_run(x, g, b, r, dy, None)
    ref, em = ln_pair(x, g, b, r, dy, None, None, 0.0)
    check_ln(f"ln H={H} res={res} {_name(dtype)}", got, ref, em, dtype)


# 9 rows: the half-wave tail of ln_fwd8_k and a partly filled block of ln_fwd_k; 4100 rows: 129 partial
# rows, so the merged column sum's last slice holds one; 16400 rows: 513 blocks, rounded up to 1024
LN_ROW_CASES = [(H, rows, dt) for H in (256, 768, 1024, 2048) for rows in (1, 3, 9, 4100) for dt in DTYPES] + \
               [(H, 16400, BF16) for H in (256, 768)]


@pytest.mark.parametrize("H,rows,dtype", LN_ROW_CASES, ids=lambda v: _name(v) if isinstance(v, torch.dtype) else str(v))
def test_ln_row_edges(H, rows, dtype):
    dev = gpu_device()
    x, g, b, r, dy, _ = ln_inputs(dev, dtype, (rows,), H, "full", False, key=H + rows)
    got = ln_run(x, g, b, r, dy, None)
    ref, em = ln_pair(x, g, b, r, dy, None, None, 0.0)
    check_ln(f"ln rows={rows} H={H} {_name(dtype)}", got, ref, em, dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("H", [256, 768, 1280, 2048])      # 768: the compiled KNOWN case
def test_ln_fused_dropout(H, dtype):
    """dx is the gradient through the mask, dres the unmasked one."""
    dev = gpu_device()
    p = 0.1
    x, g, b, r, dy, _ = ln_inputs(dev, dtype, (3, 37), H, "full", False, key=H + 7)
    got = ln_run(x, g, b, r, dy, None, p=p)
    ref, em = ln_pair(x, g, b, r, dy, None, got["keep"], p)
    check_ln(f"ln dropout H={H} {_name(dtype)}", got, ref, em, dtype)
    dropped = ~got["keep"]
    assert not bool(got["dx"][dropped].any()), "a dropped element has a gradient"
    assert bool(got["dres"][dropped].any()), "the residual gradient is masked"


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("H", [256, 512, 768, 1024, 1280, 2048])
def test_ln_grad_from(H, dtype):
    """A bridged gradient of x: added before the column sums (H <= 1024), or afterwards with the
    column sums withdrawn (wider rows)."""
    dev = gpu_device()
    x, g, b, _, dy, add = ln_inputs(dev, dtype, (3, 37), H, None, True, key=H + 13)
    got = ln_run(x, g, b, None, dy, add)
    ref, em = ln_pair(x, g, b, None, dy, add, None, 0.0)
    fused = H <= 1024
    if not fused:
        assert got["colsum"] is None, "column sums of an incomplete dx ride on the gradient"
    check_ln(f"ln grad_from H={H} {_name(dtype)}", got, ref, em, dtype, colsum=fused)


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("H", [256, 768, 2048])
def test_ln_arena_sinks(H, dtype):
    """gamma / beta and the producing Linear's bias own gradient-arena slots: the kernels add into
    them (old + gradient, rounded once) and autograd receives nothing."""
    dev = gpu_device()
    x, g, b, r, dy, _ = ln_inputs(dev, dtype, (3, 37), H, "full", False, key=H + 17)
    sinks = {}
    got = ln_run(x, g, b, r, dy, None, sinks=sinks)
    ref, em = ln_pair(x, g, b, r, dy, None, None, 0.0)
    label = f"ln sinks H={H} {_name(dtype)}"
    check_ln(label, got, ref, em, dtype, params=False)
    assert got["dgamma"] is None and got["dbeta"] is None
    assert sinks["fired"] == {"g": 1, "b": 1}
    fails = []
    for name, prm, raw in (("dgamma", got["gp"], "dgamma_raw"), ("dbeta", got["bp"], "dbeta_raw")):
        old = sinks[name[1] + "_old"]
        NO.bound(prm._ddl_main_grad, old.double() + getattr(ref, raw), (old.float() + getattr(em, raw)).to(dtype),
                 dtype, M_STORE, f"{label} slot {name}", fails)
    bias = sinks["bias"]
    old = sinks["bias_old"]
    NO.bound(bias._ddl_main_grad, old.double() + ref.dxsum, (old.float() + em.dxsum).to(dtype), dtype, M_STORE,
             f"{label} slot bias", fails)
    assert bias._ddl_sunk is not None and bias._ddl_sunk.dtype == F32
    NO.bound(bias._ddl_sunk, ref.dxsum, em.dxsum, F32, M_F32, f"{label} sunk", fails)
    assert bias.grad is None
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("H", LN_WIDTHS)
def test_ln_saved_statistics(H, dtype):
    """The per-row mean and rstd ``ddl_ln_fwd`` saves for the backward."""
    dev = gpu_device()
    L = _lib()
    eps = 1e-5
    x, g, b, r, dy, _ = ln_inputs(dev, dtype, (41,), H, "full", False, key=H + 19)
    y = torch.empty_like(x)
    stats = torch.empty(2, 41, dtype=F32, device=dev)
    L.call("ddl_ln_fwd", L.dcode(x), L.p(x), L.p(r), 41, L.p(g), L.p(b), L.p(y), L.p(stats[0]), L.p(stats[1]),
           41, H, eps, 0, 0.0)
    ref, em = (NO.ln_ref(x, g, b, eps, r, None, 0.0, dy, None, dt) for dt in (torch.float64, torch.float32))
    label = f"ln stats H={H} {_name(dtype)}"
    fails = []
    NO.bound(y, ref.y, em.y, dtype, M_STORE, f"{label} y", fails)
    NO.bound(stats[0], ref.mean, em.mean, F32, M_F32, f"{label} mean", fails)
    NO.bound(stats[1], ref.rstd, em.rstd, F32, M_F32, f"{label} rstd", fails)
    assert not fails, "\n".join(fails)


# ================================================================== BatchNorm
# per C: (N, H, W) whose row count is no multiple of the 256 / (C / 8) rows a block covers per
# iteration (C = 2048: one row, so any count) and exceeds the 8 iterations of one statistics block
BN_ODD_SHAPE = {8: (3, 29, 31), 16: (3, 19, 23), 32: (3, 13, 17), 64: (3, 11, 13), 128: (3, 7, 11),
                512: (3, 5, 7), 1024: (3, 3, 5), 2048: (3, 3, 5)}
BN_VARIANTS = [(False, False), (True, False), (True, True)]
# (seed, scale) of the ReLU cases; scale multiplies gamma, beta and the residual, hence the whole
# pre-activation.  t is about (M_STORE + 1) half ulps of the largest |y|, so the band's share follows
# where that maximum falls within its binade: 2 % just under a power of two, 4 % just above, and with
# the default draw (seed 0, scale 1) most cases exceed BAND_CAP.  Chosen on the CPU, on the oracle
# alone, as the first of a fixed list of scales and seeds with a share under 2.75 %.
_T, _F = True, False
BN_OVERRIDES = {
    (8, (4, 7, 9), _T, _F): (1, 0.9), (8, (4, 7, 9), _T, _T): (1, 1.0), (8, (3, 29, 31), _T, _F): (0, 0.62),
    (8, (3, 29, 31), _T, _T): (2, 1.0), (16, (1, 1, 2), _T, _T): (1, 1.0), (16, (4, 7, 9), _T, _F): (1, 1.0),
    (16, (4, 7, 9), _T, _T): (2, 1.0), (16, (3, 19, 23), _T, _F): (1, 0.8), (16, (3, 19, 23), _T, _T): (2, 0.7),
    (32, (4, 7, 9), _T, _F): (3, 0.9), (32, (4, 7, 9), _T, _T): (2, 1.0), (32, (3, 13, 17), _T, _F): (1, 0.8),
    (32, (3, 13, 17), _T, _T): (0, 0.62), (64, (4, 7, 9), _T, _F): (1, 0.8), (64, (4, 7, 9), _T, _T): (2, 0.7),
    (64, (3, 11, 13), _T, _F): (0, 0.8), (64, (3, 11, 13), _T, _T): (2, 0.62), (128, (4, 7, 9), _T, _F): (2, 0.7),
    (128, (4, 7, 9), _T, _T): (0, 0.62), (128, (3, 7, 11), _T, _F): (1, 0.8), (128, (3, 7, 11), _T, _T): (0, 0.62),
    (512, (4, 7, 9), _T, _F): (1, 0.7), (512, (4, 7, 9), _T, _T): (0, 0.55), (512, (3, 5, 7), _T, _F): (0, 0.7),
    (512, (3, 5, 7), _T, _T): (1, 0.62), (1024, (1, 1, 2), _T, _T): (1, 1.0), (1024, (4, 7, 9), _T, _F): (8, 0.74),
    (1024, (4, 7, 9), _T, _T): (1, 0.55), (1024, (3, 3, 5), _T, _F): (3, 0.7), (1024, (3, 3, 5), _T, _T): (0, 0.62),
    (2048, (4, 7, 9), _T, _F): (2, 0.7), (2048, (4, 7, 9), _T, _T): (2, 0.55), (2048, (3, 3, 5), _T, _F): (1, 0.8),
    (2048, (3, 3, 5), _T, _T): (2, 0.62),
}


def _bn_case(C, shape, relu, res, offset=0.0):
    seed, scale = BN_OVERRIDES.get((C, shape, relu, res), (0, 1.0))
    return (C, shape, relu, res, offset, seed, scale)


BN_TRAIN_CASES = [_bn_case(C, shape, relu, res)
                  for C in (8, 16, 32, 64, 128, 512, 1024, 2048)
                  for shape in ((1, 1, 2), (4, 7, 9), BN_ODD_SHAPE[C])
                  for relu, res in BN_VARIANTS]
# mean / std = 8: E[x^2] - mean^2 over fp32 partial sums; one small and one large row count
BN_OFFSET_CASES = [_bn_case(C, shape, False, False, 8.0)
                   for C, shapes in ((64, ((4, 7, 9), (8, 112, 112))), (2048, ((4, 7, 9), (2, 40, 40))))
                   for shape in shapes]
BN_EVAL_CASES = [(C, (4, 7, 9), relu, res) for C in (8, 64, 2048) for relu, res in BN_VARIANTS]


def _bn_id(case):
    C, shape, relu, res = case[:4]
    return f"C{C}-{'x'.join(map(str, shape))}-relu{int(relu)}-res{int(res)}" + ("-offset" if len(case) > 4 and case[4] else "")


def bn_inputs(case, device):
    """x, g, b, res, dy of one case in bf16, drawn on the CPU (so that the CPU test sees the same)."""
    C, shape, relu, res, offset, seed, scale = case
    gen = torch.Generator().manual_seed(seed)
    full = (*shape, C)
    x = (torch.randn(full, generator=gen) + offset).to(BF16)
    g = ((torch.rand(C, generator=gen) + 0.5) * scale).to(BF16)
    b = (torch.randn(C, generator=gen) * 0.3 * scale).to(BF16)
    r = (torch.randn(full, generator=gen) * scale).to(BF16) if res else None
    dy = torch.randn(full, generator=gen).to(BF16)
    return tuple(None if t is None else t.to(device) for t in (x, g, b, r, dy))


def bn_band(case, x, g, b, r, dy):
    """(ref64, emu, t, inside, share) under the oracle's own ReLU mask."""
    relu = case[2]
    ref, em = (NO.bn_ref(x, g, b, BN_EPS, relu, r, dy, dt) for dt in (torch.float64, torch.float32))
    if not relu:
        return ref, em, 0.0, None, 0.0
    t = NO.forward_tol(ref.y, em.y, BF16, M_STORE)
    inside, share = NO.relu_band(ref.z, t)
    return ref, em, t, inside, share


def _bn_train(case):
    from databricks_distributed_deep_learning_amd.ops import norm
    dev = gpu_device()
    _lib()
    C, shape, relu, res = case[:4]
    label = "bn " + _bn_id(case)
    x, g, b, r, dy = bn_inputs(case, dev)
    leaves = [None if t is None else t.clone().requires_grad_(True) for t in (x, g, b, r)]
    rm, rv = torch.zeros(C, device=dev), torch.ones(C, device=dev)
    y = norm.batch_norm(leaves[0], leaves[1], leaves[2], rm, rv, True, MOMENTUM, BN_EPS, relu, leaves[3])
    y.backward(dy)
    y = y.detach()
    ref, em, t, inside, share = bn_band(case, x, g, b, r, dy)
    fails = []
    if relu:
        print(f"BAND {label} t={t:.4e} share={share:.4f}")
        if not share <= BAND_CAP:
            fails.append(f"{label}: the ReLU band hides {share:.4f} of the elements")
        pos = ref.z > 0
        wrong = ((y > 0) != pos) & ~inside
        if bool(wrong.any()):
            fails.append(f"{label}: {int(wrong.sum())} elements outside the band on the wrong side of the ReLU")
        mask = torch.where(inside, y > 0, pos)
        ref, em = (NO.bn_ref(x, g, b, BN_EPS, mask, r, dy, dt) for dt in (torch.float64, torch.float32))
    NO.bound(y, ref.y, em.y, BF16, M_STORE, f"{label} y", fails)
    NO.bound(leaves[0].grad, ref.dx, em.dx, BF16, M_STORE, f"{label} dx", fails)
    if res:
        NO.bound(leaves[3].grad, ref.dres, em.dres, BF16, M_STORE, f"{label} dres", fails)
    NO.bound(leaves[1].grad, ref.dgamma, em.dgamma, BF16, M_STORE, f"{label} dgamma", fails)
    NO.bound(leaves[2].grad, ref.dbeta, em.dbeta, BF16, M_STORE, f"{label} dbeta", fails)
    (rm64, rv64), (rm32, rv32) = (NO.bn_running(o.mean, o.var_unbiased, MOMENTUM, dt)
                                  for o, dt in ((ref, torch.float64), (em, torch.float32)))
    NO.bound(rm, rm64, rm32, F32, M_F32, f"{label} running_mean", fails)
    NO.bound(rv, rv64, rv32, F32, M_F32, f"{label} running_var", fails)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("case", BN_TRAIN_CASES, ids=_bn_id)
def test_bn_train(case):
    _bn_train(case)


@pytest.mark.parametrize("case", BN_OFFSET_CASES, ids=_bn_id)
def test_bn_offset_statistics(case):
    _bn_train(case)


@pytest.mark.parametrize("case", BN_EVAL_CASES, ids=_bn_id)
def test_bn_inference(case):
    """``ddl_bn_eval_coeffs`` + the mask-less ``ddl_bn_apply``.  Channel 0 has a running variance of
    1e-5 (= eps), so it is bounded on its own: its outputs are two orders of magnitude larger."""
    from databricks_distributed_deep_learning_amd.ops import norm
    dev = gpu_device()
    _lib()
    C, shape, relu, res = case
    label = "bn eval " + _bn_id(case)
    x, g, b, r, _ = bn_inputs(_bn_case(C, shape, relu, res), dev)
    gen = torch.Generator().manual_seed(5)
    rm = torch.randn(C, generator=gen).to(dev)
    rv = (torch.rand(C, generator=gen) + 0.5).to(dev)
    rv[0] = 1e-5
    rm0, rv0 = rm.clone(), rv.clone()
    with torch.no_grad():
        y = norm.batch_norm(x, g, b, rm, rv, False, MOMENTUM, BN_EPS, relu, r)
    assert torch.equal(rm.view(torch.int32), rm0.view(torch.int32)), "running_mean changed in inference"
    assert torch.equal(rv.view(torch.int32), rv0.view(torch.int32)), "running_var changed in inference"
    ref, em = (NO.bn_eval_ref(x, g, b, rm, rv, BN_EPS, relu, r, dt) for dt in (torch.float64, torch.float32))
    fails = []
    NO.bound(y[..., 1:], ref.y[..., 1:], em.y[..., 1:], BF16, M_STORE, f"{label} y", fails)
    NO.bound(y[..., :1], ref.y[..., :1], em.y[..., :1], BF16, M_STORE, f"{label} y[small-variance channel]", fails)
    assert not fails, "\n".join(fails)
