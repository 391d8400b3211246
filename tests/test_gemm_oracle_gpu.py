"""The GEMM kernels against the fp64 oracle of tests/gemm_oracle.py, in two tiers.

exact   small-integer operands (every element's absolute sum A <= 256, statistics sums < 2^24; the CPU
        file checks that for every case here): ``torch.equal`` with the oracle for C, the stored
        pre-activation ``aux``, relu outputs, BatchNorm-backward ``dz`` and statistics rows.
real    randn operands rounded to bf16: per element |err| <= a + half_ulp_out(|r| + a) with
        a = 2 n 2^-24 A (conv_oracle.tol), plus 2^-8 A where the kernel stores bf16 split-K partials.
        gelu / dgelu / tanh outputs take ``gemm_oracle.act_tol`` in both tiers (a = 0 in the exact one).
        Statistics rows are compared with the fp64 sums of the kernel's own stored output within
        n 2^-24 sum |term| (n = rows; n + 3 for the centred BatchNorm-backward row).

Every case asserts the native entry point that ran (a forced kind that falls back is a failure), and for
"big192" / "hybrid" the kind ``_choose`` returns.  Nothing is tuned or timed: every ``gemm`` call forces its
kind, and the autograd cases run with the tuner off.

Guards: the arena and the ``env`` fixture of tests/test_conv_oracle_gpu.py (64 KiB of 0xFF on both sides
of every tensor, including the split-K workspaces, the zero page and the statistics rows that
``_native_gemm.py`` allocates itself).  Every kernel that takes leading dimensions runs each shape twice:
tight, and with ``ld = extent + 8`` on all three, the gaps filled with 0xFF (NaN) and checked afterwards
(``residual`` and ``aux`` share ``ldc``).

Measured on an MI355X: all 273 cases pass with 1358 printed ratios; the file takes 11 s, the slowest case --
the 65537-row shape in the exact tier, tight and ld + 8 -- 1.7 s.  Every exact-tier comparison was bitwise,
every guard byte and every ld gap (A, B, C, aux, residual) intact, every case ran the entry point it names.
Largest max(|err| / tol) per kernel and tier.  The exact tier is bitwise for C, aux, relu, dz and the
statistics rows and prints a ratio only for gelu / dgelu / tanh outputs (a = 0); "rows" = statistics rows.
  kernel                      real tier                                   exact tier (gelu / dgelu / tanh)
  ddl_gemm                    NT 0.996  NN 0.994  TN 0.999   rows 0.015   0.925
  ddl_gemm_n64 "narrow"       NT 0.994  NN 0.992  TN 0.993   rows 0.033   0.925
  ddl_gemm_n64 "tnarrow"      TN 0.972                                    (bitwise only)
  ddl_gemm_big2 "big"         NT 0.996  NN 0.996  TN 0.995   rows 0.007   0.995 (dgelu rows 0.006)
  ddl_gemm_big2 "big192"      NT 0.996  NN 0.996             rows 0.007   0.995 (dgelu rows 0.005)
  65537 x 256 x 512 "big"     NT 0.951  NN 0.954, the same tight and ld + 8   0.995
  65537 x 256 x 512 "hybrid"  NT 0.951  NN 0.954, the same tight and ld + 8   0.995
  ddl_gemm_duo                NT 0.998  NN 0.998             rows 0.016   0.995 (rows 0.017)
  ddl_gemm_duo_tn 0.998   ddl_gemm_wgrad 0.454   ddl_stream_wgrad 0.081   (bitwise only)
  ddl_skinny_gemm 0.995 (rows 0.347)   ddl_stream_gemm 0.991 (rows 0.407)  (bitwise only)
  ops.linear      forward 0.995, stored dZ against its formula 0.9999, dx 0.9998 (the 2-wide head: a sum of two
                  bf16 products next to the middle of two bf16 numbers), dW 0.993, db 0.972; its exact-tier
                  cases (no activation, relu) are bitwise in every tensor
  FFN handoff     h 0.993, z 0.995, y 0.981, dZ (dgelu epilogue) 0.995, dW2 0.954, db2 0.837, dx 0.982,
                  dW1 0.960, db1 0.916
A ratio just below 1 is one correct rounding: with these short reductions a ~ 1e-5 |r| and the bound is the
output format's half ulp.  No bound needed a term beyond those of gemm_oracle's docstring.
Kernels whose bound carries the 2^-8 A term: ddl_gemm_duo_tn with splits > 1, ddl_gemm_wgrad with a bf16
output, ddl_stream_wgrad, and ddl_gemm_big2 in TN mode with splits > 1 and a bf16 output (each read in the
kernel source: gemm_oracle's docstring).  Extra rounding term: ddl_gemm_duo_tn with one split and
``accumulate`` rounds the product sum to bf16 before it adds the base (``gemm_oracle.tol_twice``).
"""
from types import SimpleNamespace

import pytest
import torch

import gemm_oracle as O
from test_conv_oracle_gpu import BF, F32, _check, _check_rows, _done, env  # noqa: F401  (the guard arena + fixture)

pytestmark = pytest.mark.gpu

ENTRY = {"small": "ddl_gemm", "narrow": "ddl_gemm_n64", "tnarrow": "ddl_gemm_n64", "big": "ddl_gemm_big2",
         "big192": "ddl_gemm_big2", "hybrid": "ddl_gemm_big2", "wg": "ddl_gemm_wgrad"}
PADS = (0, 8)


def _ran(env):
    names = [c for c in env.calls if c not in ("ddl_gemm_bnb", "ddl_stream_wgrad_ws")]
    del env.calls[:]
    return "+".join(sorted(set(names)))


def _store(env, t, ld, dtype=None):
    """``t`` [rows, cols] on the device inside guarded [rows, ld] storage whose gaps stay 0xFF."""
    dtype = dtype or t.dtype
    s = env.new((t.shape[0], ld), dtype)
    s[:, :t.shape[1]].copy_(t.to(env.dev))
    return s


def _fresh(env, rows, cols, ld, dtype=BF):
    return env.new((rows, ld), dtype)


def _gaps(label, fails, **stores):
    for name, (s, cols) in stores.items():
        if s is not None and s.shape[1] > cols and not O.gaps_intact(s, cols):
            fails.append(f"{label}: the ld gap of {name} was written")


def _check_act(tier, label, got, act, r, fails, aux=None):
    dev = got.device
    rr = SimpleNamespace(ref=r.ref.to(dev), A=r.A.to(dev), n=r.n.to(dev))
    q = O.act_ratio(got, act, rr, BF, tier == "exact", None if aux is None else aux.to(dev))
    print(f"RATIO {label} {q:.4f}")
    if not q <= 1.0:
        fails.append(f"{label}: max |err| / tol = {q:.4f}")


def _relu_ref(r):
    return SimpleNamespace(ref=torch.clamp_min(r.ref, 0.0), A=r.A, n=r.n)


def _eff_splits(K, s, bk=64):
    nk = -(-K // bk)
    s = max(1, min(s or 1, nk))
    per = -(-nk // s)
    return -(-nk // per)


def _gemm(env, tier, kind, mode, shape, epi, fails, out="fresh_bf16", splits=None, pad=0, expect=None,
          bf16_partials=False, twice=False, cr=None):
    """One ``gemm`` call with the kind forced, checked against the oracle; returns the label."""
    NG = env.NG
    M, N, K = shape
    o, R = cr if cr is not None else O.case_refs(tier, mode, M, N, K)
    (ar, ac), (br, bc), _ = O.extents(mode, M, N, K)
    lda, ldb, ldc = ac + pad, bc + pad, N + pad
    label = f"{tier} {kind}.{mode} {shape} {epi} {out} s{splits} ld+{pad}"
    A, B = _store(env, o["a"], lda), _store(env, o["b"], ldb)
    dt = F32 if out == "acc_f32" else BF
    acc = out != "fresh_bf16"
    C = _store(env, o["base"], ldc, dt) if acc else _fresh(env, M, N, ldc, dt)
    kw, aux, part, ref, res = {}, None, None, None, None
    if epi in ("bias", "bias_res", "relu", "tanh", "gelu"):
        kw["bias"] = env.put(o["bias"].to(env.dev))
    if epi == "bias32":
        kw["bias"] = env.put(o["bias32"].to(env.dev))
    if epi in ("res", "bias_res") or epi.startswith("bnb_res1"):
        res = _store(env, o["res"], ldc)
        kw["residual"] = res
    if epi in ("relu", "tanh", "gelu"):
        kw["act"] = epi
    if epi == "gelu":
        aux = _fresh(env, M, N, ldc)
        kw["aux"] = aux
    if epi.startswith("dgelu"):
        aux = _store(env, o["aux"], ldc)
        kw.update(act="dgelu", aux=aux)
    if epi in ("colstats", "dgelu_stats") or epi.startswith("bnb"):
        part = env.new((NG.stats_rows_max(M) * 2 * N,), F32)
        kw["colstats"] = part
    if epi.startswith("bnb"):
        aux = _store(env, o["aux"], ldc)
        mean, istd = env.put(o["mean"].to(env.dev)), env.put(o["istd"].to(env.dev))
        mask = env.put(O.pack_mask(o["bits"]).to(env.dev)) if epi.endswith("mask1") else None
        kw.update(act="bnb", aux=aux, bnb=(mask, mean, istd))
    if kind in ("big192", "hybrid"):
        ch = NG._choose(O.MODE_ID[mode], A, lda, B, ldb, C, ldc, M, N, K, kw.get("bias"), kw.get("act"), kw.get("aux"),
                        splits, None, None, False, kw.get("residual"), kind, kw.get("colstats"))
        if ch[0] != kind:
            fails.append(f"{label}: _choose gave {ch}")
    rows = NG.gemm(O.MODE_ID[mode], A, lda, B, ldb, C, ldc, M, N, K, splits=splits, kernel=kind, accumulate=acc, **kw)
    ran = _ran(env)
    if ran != expect:
        fails.append(f"{label}: ran {ran}, not {expect}")
    got = C[:, :N]
    if epi in ("plain", "colstats"):
        ref = R["acc" if acc else "plain"]
    elif epi in ("bias", "bias32"):
        ref = R["bias"]
    elif epi in ("res", "bias_res"):
        ref = R[epi]
    elif epi == "relu":
        ref = _relu_ref(R["bias"])
    elif epi.startswith("bnb"):
        ref = R[epi]
    if ref is not None:
        if twice and tier == "real":
            dev = got.device
            rr = SimpleNamespace(ref=ref.ref.to(dev), A=ref.A.to(dev), n=ref.n.to(dev))
            q = O.ratio_twice(got, rr, o["base"].to(dev), dt, bf16_partials)
            print(f"RATIO {label} {q:.4f}")
            if not q <= 1.0:
                fails.append(f"{label}: max |err| / tol = {q:.4f}")
        else:
            _check(tier, label, got, ref, dt, fails, bf16_partials=bf16_partials)
    elif epi in ("tanh", "gelu"):
        _check_act(tier, label, got, epi, R["bias"], fails)
        if epi == "gelu":
            _check(tier, label + " aux", aux[:, :N], R["bias"], BF, fails)
    else:   # dgelu
        _check_act(tier, label, got, "dgelu", R["plain"], fails, aux=o["aux"])
    if part is not None:
        st = part[:rows * 2 * N].view(rows, 2, N).double().sum(0)
        if epi.startswith("bnb"):
            x = aux[:, :N]
            mean, istd = kw["bnb"][1], kw["bnb"][2]
            want = ref.stats[0] if tier == "exact" else O.bnb_sums(got, x, mean, istd)
            _check_rows(tier, label + " stats", (st[0], st[1]), want, O.bnb_sums(got, x, mean, istd, absolute=True),
                        M + 3, fails)
        elif epi == "dgelu_stats":      # sums of a rounded nonlinear output: against the stored tensor in both tiers
            _check_rows("real", label + " stats", (st[0], st[1]), O.bn_stats_rows(got),
                        O.bn_stats_rows(got, absolute=True), M, fails)
        else:
            want = ref.stats[0] if tier == "exact" else O.bn_stats_rows(got)
            _check_rows(tier, label + " stats", (st[0], st[1]), want, O.bn_stats_rows(got, absolute=True), M, fails)
    _gaps(label, fails, C=(C, N), aux=(aux, N), A=(A, ac), B=(B, bc), residual=(res, N))
    return label


def _sid(s):
    return "x".join(str(v) for v in s)


# ---------------------------------------------------------------------------- gemm.hip: 128x128, 128x64
SMALL_EPIS = ("plain", "bias", "bias32", "relu", "tanh", "gelu", "res", "colstats")


@pytest.mark.parametrize("tier", O.TIERS)
@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("mode", ("NT", "NN"))
@pytest.mark.parametrize("shape", O.SMALL_SHAPES, ids=_sid)
def test_small_nt_nn(env, tier, shape, mode, pad):
    """ddl_gemm (128x128x64) with every epilogue of gemm_k, and += a bf16 / an fp32 base."""
    fails = []
    for epi in SMALL_EPIS:
        _gemm(env, tier, "small", mode, shape, epi, fails, pad=pad, expect="ddl_gemm")
    for out in ("acc_bf16", "acc_f32"):
        _gemm(env, tier, "small", mode, shape, "plain", fails, out=out, pad=pad, expect="ddl_gemm")
    _gemm(env, tier, "small", mode, shape, "bias_res", fails, splits=3, pad=pad, expect="ddl_gemm")
    _done(fails)


@pytest.mark.parametrize("tier", O.TIERS)
@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("kind,shape", [("small", s) for s in O.SMALL_SHAPES] + [("narrow", s) for s in O.NARROW_SHAPES]
                         + [("tnarrow", s) for s in O.TNARROW_SHAPES], ids=lambda v: v if isinstance(v, str) else _sid(v))
def test_gemm_hip_tn(env, tier, kind, shape, pad):
    """TN on the 128x128, 128x64 and transposed 128x64 kernels: splits 1 and 3 (fp32 slabs +
    gemm_reduce), into a fresh bf16 tensor, += a bf16 and an fp32 base."""
    fails = []
    shape = O.mode_shape("TN", shape)
    for splits in (1, 3):
        for out in O.OUTS:
            _gemm(env, tier, kind, "TN", shape, "plain", fails, out=out, splits=splits, pad=pad, expect=ENTRY[kind])
    _done(fails)


@pytest.mark.parametrize("tier", O.TIERS)
@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("mode", ("NT", "NN"))
@pytest.mark.parametrize("shape", O.NARROW_SHAPES, ids=_sid)
def test_narrow_nt_nn(env, tier, shape, mode, pad):
    """ddl_gemm_n64 (128x64 tiles): the knobs of the 128x128 kernel, one per kind."""
    fails = []
    for epi in ("plain", "bias", "gelu", "res", "colstats"):
        _gemm(env, tier, "narrow", mode, shape, epi, fails, pad=pad, expect="ddl_gemm_n64")
    _gemm(env, tier, "narrow", mode, shape, "plain", fails, out="acc_f32", pad=pad, expect="ddl_gemm_n64")
    _done(fails)


# ---------------------------------------------------------------------------- gemm_big.hip: 256x256, 256x192
BIG_EPIS = ("plain", "bias", "bias32", "relu", "gelu", "dgelu_stats", "res", "colstats")


@pytest.mark.parametrize("tier", O.TIERS)
@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("mode", ("NT", "NN"))
@pytest.mark.parametrize("shape", O.BIG_SHAPES, ids=_sid)
def test_big_nt_nn(env, tier, shape, mode, pad):
    """ddl_gemm_big2: every register epilogue, accumulate, and one fp32 split-K launch with its reduce."""
    fails = []
    for epi in BIG_EPIS:
        _gemm(env, tier, "big", mode, shape, epi, fails, pad=pad, expect="ddl_gemm_big2")
    for out in ("acc_bf16", "acc_f32"):
        _gemm(env, tier, "big", mode, shape, "plain", fails, out=out, pad=pad, expect="ddl_gemm_big2")
    _gemm(env, tier, "big", mode, shape, "bias_res", fails, splits=2, pad=pad, expect="ddl_gemm_big2")
    _done(fails)


@pytest.mark.parametrize("tier", O.TIERS)
@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("shape", O.BIG_SHAPES, ids=_sid)
def test_big_tn(env, tier, shape, pad):
    """ddl_gemm_big2 TN: splits 1 and 2 (bf16 slabs when split and the output is bf16; an fp32 output
    runs unsplit), fresh and accumulating."""
    fails = []
    shape = O.mode_shape("TN", shape)
    for splits in (1, 2):
        for out in O.OUTS:
            pb = out != "acc_f32" and _eff_splits(shape[2], splits) > 1
            _gemm(env, tier, "big", "TN", shape, "plain", fails, out=out, splits=splits, pad=pad,
                  expect="ddl_gemm_big2", bf16_partials=pb)
    _done(fails)


@pytest.mark.parametrize("tier", O.TIERS)
@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("mode", ("NT", "NN"))
@pytest.mark.parametrize("shape", O.BIG192_SHAPES, ids=_sid)
def test_big192(env, tier, shape, mode, pad):
    """256x192 tiles of the 256x256 kernel (register epilogues only)."""
    fails = []
    for epi in ("plain", "bias", "bias_res", "relu", "gelu", "dgelu_stats"):
        _gemm(env, tier, "big192", mode, shape, epi, fails, pad=pad, expect="ddl_gemm_big2")
    _done(fails)


@pytest.mark.parametrize("tier", O.TIERS)
@pytest.mark.parametrize("mode", ("NT", "NN"))
def test_big_persistent_and_hybrid(env, tier, mode):
    """65537 x 256 x 512: 257 tiles on 256 CUs, so one block of the persistent grid walks a second tile,
    and ``hybrid_rows`` gives (65536, 2): 256 tiles unsplit plus a one-row tail split 2 (launched at
    ``_at`` offsets), tight and with ``ld = extent + 8`` (so that ``M1 * ld`` differs from ``M1 * extent``).  The
    oracle of this one shape is computed in fp64 on the device."""
    M, N, K = O.HUGE_SHAPE
    assert env.NG.hybrid_rows(M, N, K) == (65536, 2)
    cr = O.case_refs.__wrapped__(tier, mode, M, N, K, str(env.dev), O.HUGE_VMAX, O.HUGE_EPIS)
    fails = []
    for pad in PADS:            # ld + 8: the ``_at`` offsets M1 * ld and the tile walker's row strides
        for kind, splits in (("big", None), ("hybrid", 2)):
            for epi in ("plain", "bias_res", "gelu", "dgelu"):
                _gemm(env, tier, kind, mode, O.HUGE_SHAPE, epi, fails, splits=splits, pad=pad, expect="ddl_gemm_big2",
                      cr=cr)
    _done(fails)


# ---------------------------------------------------------------------------- gemm_duo.hip
@pytest.mark.parametrize("tier", O.TIERS)
@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("mode", ("NT", "NN"))
@pytest.mark.parametrize("shape", O.DUO_SHAPES, ids=_sid)
def test_duo_nt_nn(env, tier, shape, mode, pad):
    """ddl_gemm_duo (256x128 tiles, 32-deep stages): its epilogues."""
    fails = []
    for epi in ("plain", "bias", "bias_res", "gelu", "dgelu_stats", "colstats"):
        _gemm(env, tier, "duo", mode, shape, epi, fails, pad=pad, expect="ddl_gemm_duo")
    _done(fails)


@pytest.mark.parametrize("tier", O.TIERS)
@pytest.mark.parametrize("mode", ("NT", "NN"))
@pytest.mark.parametrize("with_res", (0, 1))
@pytest.mark.parametrize("with_mask", (0, 1))
def test_duo_bn_backward_epilogue(env, tier, mode, with_res, with_mask):
    """ddl_gemm_duo's BatchNorm-backward epilogue (dense output: ldc == N)."""
    fails = []
    _gemm(env, tier, "duo", mode, O.DUO_BNB_SHAPE, f"bnb_res{with_res}_mask{with_mask}", fails, expect="ddl_gemm_duo")
    _done(fails)


@pytest.mark.parametrize("tier", O.TIERS)
@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("shape,splits", O.DUO_TN_CASES, ids=lambda v: _sid(v))
def test_duo_tn(env, tier, shape, splits, pad):
    """ddl_gemm_duo_tn: bf16 partial tiles + duo_reduce_k when split; one split stores straight into C
    (and with ``accumulate`` rounds twice: gemm_oracle.tol_twice)."""
    fails = []
    for s in splits:
        for out in ("fresh_bf16", "acc_bf16"):
            pb = _eff_splits(shape[2], s, 32) > 1
            _gemm(env, tier, "duo", "TN", shape, "plain", fails, out=out, splits=s, pad=pad, expect="ddl_gemm_duo_tn",
                  bf16_partials=pb, twice=(not pb and out == "acc_bf16"))
    _done(fails)


# ---------------------------------------------------------------------------- the weight-gradient kernels
@pytest.mark.parametrize("tier", O.TIERS)
@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("shape,splits", O.WG_CASES, ids=lambda v: _sid(v))
def test_wgrad_kernel_plain_tn(env, tier, shape, splits, pad):
    """ddl_gemm_wgrad without a conv descriptor: bf16 slabs whenever the output is bf16."""
    fails = []
    for s in splits:
        for out in O.OUTS:
            _gemm(env, tier, "wg", "TN", shape, "plain", fails, out=out, splits=s, pad=pad, expect="ddl_gemm_wgrad",
                  bf16_partials=(out != "acc_f32"))
    _done(fails)


@pytest.mark.parametrize("tier", O.TIERS)
@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("grid", O.SWG_GRIDS)
@pytest.mark.parametrize("shape", O.SWG_SHAPES, ids=_sid)
def test_stream_wgrad(env, tier, shape, grid, pad):
    """ddl_stream_wgrad through its entry point (``grid`` is not exposed through ``gemm``): all 256
    workgroups and 3, K not a multiple of the 32-row slot; bf16 workgroup partials + reduce."""
    from databricks_distributed_deep_learning_amd.ops import _lib
    M, N, K = shape
    o, R = O.case_refs(tier, "TN", M, N, K)
    lda, ldb, ldc = M + pad, N + pad, N + pad
    assert env.NG.swg_ok(M, N, K, lda, ldb)
    A, B = _store(env, o["a"], lda), _store(env, o["b"], ldb)
    zero = env.NG._zero_page(env.dev)
    fails = []
    for out in ("fresh_bf16", "acc_bf16"):
        acc = out == "acc_bf16"
        C = _store(env, o["base"], ldc, BF) if acc else _fresh(env, M, N, ldc)
        ws = env.new(((grid or 256) * M * N,), BF)
        assert ws.numel() <= int(_lib.fn("ddl_stream_wgrad_ws")(M, N))
        rc = _lib.fn("ddl_stream_wgrad")(A.data_ptr(), lda, B.data_ptr(), ldb, C.data_ptr(), ldc, M, N, K, int(acc),
                                         ws.data_ptr(), ws.numel(), zero.data_ptr(), grid, _lib.stream())
        assert rc == 0, rc
        assert _ran(env) == "ddl_stream_wgrad"
        label = f"{tier} swg {shape} g{grid} {out} ld+{pad}"
        _check(tier, label, C[:, :N], R["acc" if acc else "plain"], BF, fails, bf16_partials=True)
        _gaps(label, fails, C=(C, N), A=(A, M), B=(B, N))
    _done(fails)


# ---------------------------------------------------------------------------- skinny_gemm.hip, stream_gemm.hip
def _streaming(env, tier, name, M, N, K, grid, epi, fails, nrows):
    """One ddl_skinny_gemm / ddl_stream_gemm call: epi in plain_stats, res, bnb_res{0,1}_mask{0,1}."""
    from databricks_distributed_deep_learning_amd.ops import _lib
    o, R = O.case_refs(tier, "NT", M, N, K)
    dev = env.dev
    a, w = env.put(o["a"].to(dev)), env.put(o["b"].to(dev))
    c = env.new((M, N), BF)
    bnb = epi.startswith("bnb")
    res = env.put(o["res"].to(dev)) if (epi == "res" or epi.startswith("bnb_res1")) else None
    part = env.new((nrows * 2 * N,), F32) if epi != "res" else None
    aux = mean = istd = mask = None
    if bnb:
        aux, mean, istd = env.put(o["aux"].to(dev)), env.put(o["mean"].to(dev)), env.put(o["istd"].to(dev))
        mask = env.put(O.pack_mask(o["bits"]).to(dev)) if epi.endswith("mask1") else None
    rows = _lib.fn(name)(a.data_ptr(), w.data_ptr(), c.data_ptr(), M, N, K, _lib.p(part), _lib.p(res), _lib.p(aux),
                         _lib.p(mask), _lib.p(mean), _lib.p(istd), grid, _lib.stream())
    label = f"{tier} {name} {(M, N, K)} g{grid} {epi}"
    assert rows >= 0, f"{label}: {rows}"
    assert _ran(env) == name
    ref = R["plain"] if epi == "plain_stats" else R[epi]
    _check(tier, label, c, ref, BF, fails)
    if part is None:
        return
    assert 0 < rows <= nrows, f"{label}: {rows} statistics rows"
    st = part[:rows * 2 * N].view(rows, 2, N).double().sum(0)
    if bnb:
        want = ref.stats[0] if tier == "exact" else O.bnb_sums(c, aux, mean, istd)
        _check_rows(tier, label + " stats", (st[0], st[1]), want, O.bnb_sums(c, aux, mean, istd, absolute=True), M + 3,
                    fails)
    else:
        want = ref.stats[0] if tier == "exact" else O.bn_stats_rows(c)
        _check_rows(tier, label + " stats", (st[0], st[1]), want, O.bn_stats_rows(c, absolute=True), M, fails)


@pytest.mark.parametrize("tier", O.TIERS)
@pytest.mark.parametrize("M,grid", O.SKINNY_MG)
@pytest.mark.parametrize("N,K", O.SKINNY_NK)
def test_skinny_gemm(env, tier, N, K, M, grid):
    """ddl_skinny_gemm: plain + statistics; residual (N = 256); the BatchNorm-backward epilogue with and
    without a mask (N = 64), and with the residual (N = 256)."""
    epis = ["plain_stats"] + (["res", "bnb_res1_mask0", "bnb_res1_mask1"] if N == 256 else
                              ["bnb_res0_mask0", "bnb_res0_mask1"])
    fails = []
    for epi in epis:
        _streaming(env, tier, "ddl_skinny_gemm", M, N, K, grid, epi, fails, -(-M // 64))
    _done(fails)


@pytest.mark.parametrize("tier", O.TIERS)
@pytest.mark.parametrize("M,grid", O.STREAM_MG)
@pytest.mark.parametrize("N,K", O.STREAM_NK)
def test_stream_gemm(env, tier, N, K, M, grid):
    """ddl_stream_gemm: plain + statistics; the BatchNorm-backward epilogue with and without a mask, and
    with the residual where the kernel has it (N = 512 and 1024)."""
    epis = ["plain_stats", "bnb_res0_mask0", "bnb_res0_mask1"] + (["bnb_res1_mask1"] if N in (512, 1024) else [])
    fails = []
    for epi in epis:
        _streaming(env, tier, "ddl_stream_gemm", M, N, K, grid, epi, fails, 256)
    _done(fails)


# ---------------------------------------------------------------------------- the autograd path
@pytest.fixture
def rec(env, monkeypatch):
    """``ops.linear`` with the tuner off, every GEMM it issues recorded with its operand tensors: the
    gradients' operand dZ is a stored bf16 tensor that only autograd sees, and each check below bounds the
    one kernel that read it."""
    from databricks_distributed_deep_learning_amd.ops import _native_linear as NL
    monkeypatch.setattr(env.NG, "_TUNE", False)
    calls, real = [], NL.gemm

    def gemm(mode, A, lda, B, ldb, C, ldc, M, N, K, **kw):
        out = real(mode, A, lda, B, ldb, C, ldc, M, N, K, **kw)
        calls.append(SimpleNamespace(mode=O.MODES[mode], A=A.detach(), B=B.detach(), C=C.detach(), kw=kw))
        return out
    monkeypatch.setattr(NL, "gemm", gemm)
    return calls


def _gemm_entries(env):
    return {n for n in _ran(env).split("+") if n.startswith("ddl_gemm") or n.startswith("ddl_stream")}


def _check_call(tier, label, c, fails):
    """One recorded GEMM against the oracle run on the very tensors it read."""
    kw = {k2: c.kw[k1].detach() for k1, k2 in (("bias", "bias"), ("residual", "residual")) if c.kw.get(k1) is not None}
    assert not c.kw.get("accumulate"), label
    r = O.ref_of(c.mode, c.A, c.B, **kw)
    act = c.kw.get("act")
    if act in ("gelu", "tanh", "dgelu"):
        _check_act(tier, label, c.C, act, r, fails, aux=c.kw["aux"].detach() if act == "dgelu" else None)
        if act == "gelu" and c.kw.get("aux") is not None:
            _check(tier, label + " aux", c.kw["aux"].detach(), r, BF, fails)
    else:
        _check(tier, label, c.C, _relu_ref(r) if act == "relu" else r, BF, fails)


def _colsum_ref(dz):
    d = dz.double()
    return SimpleNamespace(ref=d.sum(0), A=d.abs().sum(0),
                           n=torch.full((d.shape[1],), float(d.shape[0]), dtype=O.F64, device=d.device))


def _verdict(label, got, ref, t, fails):
    err = (got.double() - ref).abs()
    q = float(torch.where(err > 0, err / t, torch.zeros_like(err)).max()) if bool(torch.isfinite(got.double()).all()) \
        else float("inf")
    print(f"RATIO {label} {q:.4f}")
    if not q <= 1.0:
        fails.append(f"{label}: max |err| / tol = {q:.4f}")


def _dz_of(act, dy, y, zs):
    """(dZ in fp64, its bound) of the elementwise backward in front of the gradient GEMMs: exact (bound 0)
    for no activation and relu; one fp32 evaluation and one bf16 rounding for tanh (from the stored output)
    and gelu (from the stored pre-activation, with the erf allowance of the elementwise oracle)."""
    dyd = dy.double()
    if act is None:
        return dyd, torch.zeros_like(dyd)
    if act == "relu":
        return dyd * (y.double() > 0), torch.zeros_like(dyd)
    if act == "tanh":
        yd = y.double()
        dz = dyd * (1.0 - yd * yd)
        t = 4.0 * 2.0 ** -24 * dyd.abs() * (1.0 + yd * yd)
    else:
        dz = dyd * O.gelu_grad_ref(zs.double(), O.F64)
        t = (0.5 * O.ERF_ABS_ERR + O.EVAL_ROUNDINGS * O.GELU_LIP) * dyd.abs()
    return dz, t + O.half_ulp_t(dz.abs() + t, BF)


@pytest.mark.parametrize("tier,shape,act,bias", O.LINEAR_CASES,
                         ids=[f"{t}-{_sid(s)}-{a}-bias{int(b)}" for t, s, a, b in O.LINEAR_CASES])
def test_linear_autograd(env, rec, tier, shape, act, bias):
    """``ops.linear`` forward, dx, dW and db.  Each recorded GEMM is checked against the oracle on the stored
    tensors it read (dZ included), dZ itself against the formula on the stored output / pre-activation,
    and db against the column sums of the stored dZ: one kernel per check.  The exact tier runs the cases
    whose dZ is exact (no activation, relu) and is bitwise throughout.  out = 2 and 5 take the N-padded-to-8
    path (no GELU there; one of its cases runs without a bias)."""
    from databricks_distributed_deep_learning_amd import ops
    M, K, N = shape
    Np = -(-N // 8) * 8
    o = {k: v.to(env.dev) for k, v in O.linear_case(tier, M, K, N).items()}
    x, w = env.put(o["x"]).requires_grad_(), env.put(o["w"]).requires_grad_()
    b = env.put(o["b"]).requires_grad_() if bias else None
    tag = f"{tier} linear {shape} {act} bias{int(bias)}"
    y = ops.linear(x, w, b, act)
    assert _gemm_entries(env) == {"ddl_gemm"}
    fails = []
    assert len(rec) == 1 and rec[0].mode == "NT"
    _check_call(tier, tag + " fwd", rec[0], fails)
    assert torch.equal(y.detach(), rec[0].C[:, :N])
    z = O.ref_of("NT", o["x"], o["w"], **({"bias": o["b"]} if bias else {}))      # the unpadded problem
    if act in ("gelu", "tanh"):
        _check_act(tier, tag + " y", y.detach(), act, z, fails)
    else:
        _check(tier, tag + " y", y.detach(), _relu_ref(z) if act == "relu" else z, BF, fails)
    zs = getattr(y, "_ddl_gelu_pre")[0].detach() if act == "gelu" else None
    y.backward(o["dy"])
    torch.cuda.synchronize()
    assert _gemm_entries(env) == {"ddl_gemm"}
    assert [c.mode for c in rec[1:]] == ["NN", "TN"]
    dgrad, wgrad = rec[1], rec[2]
    dzs = dgrad.A
    assert wgrad.A.data_ptr() == dzs.data_ptr() and tuple(dzs.shape) == (M, Np)
    dz, tol_dz = _dz_of(act, o["dy"], y.detach(), zs)
    _verdict(tag + " dz", dzs[:, :N], dz, tol_dz, fails)
    assert not bool(dzs[:, N:].any())
    _check_call(tier, tag + " dx", dgrad, fails)
    _check_call(tier, tag + " dw", wgrad, fails)
    assert torch.equal(x.grad, dgrad.C) and torch.equal(w.grad, wgrad.C[:N])
    if bias:
        _check(tier, tag + " db", b.grad, _colsum_ref(dzs[:, :N]), BF, fails)
    _done(fails)


def test_ffn_dgelu_handoff(env, rec):
    """Linear(gelu) -> Linear(fuse_dgelu=True) at (M, H, I) = (300, 64, 192): the second layer's dgrad applies
    the first layer's dGELU and column-sums its bias gradient (the 256x256 kernel's register epilogue).
    All five gradients, each against the stored tensors its kernel read (the stored dZ is the dgrad's
    recorded output)."""
    from databricks_distributed_deep_learning_amd import ops
    M, H, I = O.FFN_SHAPE
    o = {k: v.to(env.dev) for k, v in O.ffn_case().items()}
    x, w1, b1, w2, b2 = (env.put(o[k]).requires_grad_() for k in ("x", "w1", "b1", "w2", "b2"))
    h = ops.linear(x, w1, b1, "gelu")
    y = ops.linear(h, w2, b2, None, fuse_dgelu=True)
    assert _gemm_entries(env) == {"ddl_gemm"}
    fails = []
    assert [c.mode for c in rec] == ["NT", "NT"]
    _check_call("real", "real ffn h", rec[0], fails)
    _check_call("real", "real ffn y", rec[1], fails)
    zs = rec[0].kw["aux"].detach()
    y.backward(o["dy"])
    torch.cuda.synchronize()
    assert _gemm_entries(env) == {"ddl_gemm", "ddl_gemm_big2"}      # big2: the dGELU + column-sum epilogue
    assert [c.mode for c in rec[2:]] == ["NN", "TN", "NN", "TN"]
    dz_call, dw2, dx, dw1 = rec[2:]
    assert dz_call.kw.get("act") == "dgelu" and dz_call.kw["aux"].data_ptr() == zs.data_ptr() \
        and dz_call.kw.get("colstats") is not None
    dZ = dz_call.C
    assert dx.A.data_ptr() == dZ.data_ptr() and dw1.A.data_ptr() == dZ.data_ptr()
    for name, c in (("dZ", dz_call), ("dw2", dw2), ("dx", dx), ("dw1", dw1)):
        _check_call("real", f"real ffn {name}", c, fails)
    assert torch.equal(w2.grad, dw2.C) and torch.equal(w1.grad, dw1.C) and torch.equal(x.grad, dx.C)
    _check("real", "real ffn db2", b2.grad, _colsum_ref(o["dy"]), BF, fails)
    _check("real", "real ffn db1", b1.grad, _colsum_ref(dZ), BF, fails)
    _done(fails)
