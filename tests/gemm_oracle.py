"""An independent reference for the GEMM kernels (gemm.hip, gemm_big.hip, gemm_duo.hip, skinny_gemm.hip,
stream_gemm.hip and the ``_native_gemm.py`` dispatch), the bounds the oracle tests share, and the case
tables both test files build their operands from.

Everything here is device-agnostic torch written out from the formulas: nothing from ``ops/``, no
autograd.  The bound, the operand generators and the BatchNorm epilogue references are those of
``conv_oracle`` (imported, not copied); GELU and its slope are those of ``elementwise_oracle``.

``gemm_ref(mode, A, B, ...)`` covers NT (``A[M,K] B[N,K]^T``), NN (``A[M,K] B[K,N]``) and TN
(``A[K,M]^T B[K,N]``).  Operands may sit in padded ``[rows, ld]`` storage whose gap columns hold NaN: the
reference slices ``shape = (M, N, K)`` out before any arithmetic.  ``absolute=True`` gives the
absolute-sum companion ``A = sum |term|`` (bias, residual and accumulate base count as one term each);
the term count ``n`` is the same computation on all-ones operands (``_triple``).

Epilogues on top of the pre-activation ``z`` (``z = acc + bias + residual``):
  relu      exact (a selection).
  gelu      ``gelu(z)`` with ``aux = z`` stored next to it.  Every kernel of the family (gemm_k's
            ``apply_act``, ``direct4`` / ``epi_direct<EK_GELU>`` of gemm_big.hip, ``E_GELU`` of
            gemm_duo.hip, and the split-K reduce kernels) applies GELU to the **fp32** pre-activation and
            rounds ``aux`` and the output separately, once each; the oracle models exactly that: the
            output is compared with ``gelu(z_ref)``, not with ``gelu(bf16(z))``.
  dgelu     ``C = acc * gelu'(aux)`` (aux: a stored bf16 pre-activation, an input).
  tanh      ``tanh(z)``.
  bnb       the BatchNorm-backward epilogue ``dz = (acc + res) * mask`` with rows
            ``[sum dz | sum dz xhat]`` (``conv_oracle.bnb_sums``).
  colstats  ``[sum C | sum C^2]`` of the *stored* output (``conv_oracle.bn_stats_rows``).

Two tiers, as for the convolutions:
exact   small-integer operands at ``density(K)``: every element has ``A <= 256`` and every statistics sum
        stays below 2^24, so every product, every partial sum in any order and every bf16 or fp32 split-K
        partial is exact: C, the stored ``aux``, relu outputs, bnb ``dz`` and statistics rows must equal
        the oracle bit for bit.  gelu / dgelu / tanh outputs take the real tier's bound with ``a = 0``.
real    randn operands rounded to bf16, weights scaled by K^-0.5: ``conv_oracle.tol`` per element,
            a   = 2 n 2^-24 A (+ 2^-8 A where split-K partials are stored in bf16)
            tol = a + half_ulp_out(|r| + a).
        bf16 partials are stored by (read in the kernel sources):
          ddl_gemm_duo_tn with splits > 1   (gemm_duo.hip ``store_image(p.ws ...)``: bf16 partial tiles)
          ddl_gemm_wgrad with a bf16 output (gemm_big.hip ``p.part_bf16 = !out_f32``, one split included)
          ddl_stream_wgrad                  (stream_gemm.hip: bf16 workgroup partials, always)
          ddl_gemm_big2 in TN mode with splits > 1 (gemm_big.hip ``launch_big``: ``p.part_bf16 = LA == KO
                                            && LB == KO && splits > 1``; an fp32 output runs unsplit)
        The 128x128 / 128x64 kernels of gemm.hip keep fp32 slabs.
        One rounding the plain model lacks, added for the kernel that performs it only (``twice=True``):
          ddl_gemm_duo_tn with one split and ``accumulate``: the tile is packed to bf16 in the LDS image
          (``pack2bf``) *before* ``store_image`` adds the base and rounds again, so the product sum is
          rounded once more: + half_ulp_bf16(|r - base| + a), the first of the two roundings.
        Nonlinear epilogues f (``act_tol``): with L the Lipschitz bound of f at z (gelu 1.13, tanh 1;
        dgelu: the accumulator's ``a`` scaled by ``|gelu'(aux)|``),
            t   = L a + allowance_f
            tol = t + half_ulp_out(|f(z)| + t)
        allowance_f is what tests/test_elementwise_oracle_gpu.py grants the device erf: half of
        ``ERF_ABS_ERR`` times |z| for GELU and times |acc| for its slope -- plus the fp32 evaluation of f
        itself, which that file covers with its emulation multiplier and this per-element bound has to
        name: ``EVAL_ROUNDINGS`` = 8 roundings of 2^-24 (the scaled argument, the polynomial's last
        steps, 1 + erf, the products) on max(|z|, |f|) resp. |acc| L, and for tanh the 5 ulp the OpenCL C
        specification (whose accuracy table the device math library follows) allows ``tanh``:
        5 * 2^-23 |tanh z|.  All of these are ~1e-6 relative, 1/2000 of a bf16 half ulp.
        Statistics rows go against fp64 sums of the kernel's own stored output within
        ``n 2^-24 sum |term|`` (``n + 3`` for the centred bnb row).

Shapes that the issue's tables list and a contract excludes (replaced by the nearest inside):
  * reduction-outer operands (B of NN, both of TN) are loaded in 16-byte chunks along the output side
    (``Loader<KO>``: ``col < rows_total`` is tested per chunk, not per element), so that side must be a
    multiple of 8, as ``_native_linear._ok`` guarantees for every caller.  TN cases therefore use M rounded
    up to 8: (1, 8, 8) -> (8, 8, 8), (129, 136, 72) -> (136, 136, 72), (130, 72, 200) -> (136, 72, 200),
    (129, 64, 72) -> (136, 64, 72), (70, 192, 136) -> (72, 192, 136), (257, 264, 72) -> (264, 264, 72),
    (300, 520, 136) -> (304, 520, 136).  NT / NN keep the odd M.
"""
from __future__ import annotations

import functools
from types import SimpleNamespace

import torch

from conv_oracle import (EXACT_A_MAX, EXACT_STAT_MAX, _triple, bn_stats_rows, bnb_sums, density, gen,  # noqa: F401
                         half_ulp_t, int_tensor, ones, operand, pack_mask, ratio, real_tensor, tol)
from elementwise_oracle import ERF_ABS_ERR, gelu_grad_ref, gelu_ref

F64 = torch.float64
BF, F32 = torch.bfloat16, torch.float32
TIERS = ("exact", "real")
MODES = ("NT", "NN", "TN")
MODE_ID = {"NT": 0, "NN": 1, "TN": 2}
GELU_LIP = 1.13                   # max |gelu'| = 1.1290 (at z = sqrt(2))
EVAL_ROUNDINGS = 8.0 * 2.0 ** -24
TANH_ULPS = 5.0 * 2.0 ** -23


# ---------------------------------------------------------------------------- reference
def extents(mode, M, N, K):
    """((rows, cols) of A, of B, of C) in storage order."""
    if mode == "NT":
        return (M, K), (N, K), (M, N)
    if mode == "NN":
        return (M, K), (K, N), (M, N)
    return (K, M), (K, N), (M, N)


def _infer(mode, A, B):
    if mode == "NT":
        return A.shape[0], B.shape[0], A.shape[1]
    if mode == "NN":
        return A.shape[0], B.shape[1], A.shape[1]
    return A.shape[1], B.shape[1], A.shape[0]


def _cut(t, rows, cols, dtype, absolute):
    t = t[:rows, :cols].to(dtype)
    return t.abs() if absolute else t


def gemm_ref(mode, A, B, dtype=F64, bias=None, residual=None, base=None, absolute=False, shape=None):
    """C[M, N] = op(A) op(B) (+ bias[n]) (+ residual) (+ base).  ``shape`` = (M, N, K) when the operands
    (and residual / base, rows of ``ldc``) sit in padded storage; inferred from tight operands otherwise."""
    M, N, K = shape if shape is not None else _infer(mode, A, B)
    (ar, ac), (br, bc), _ = extents(mode, M, N, K)
    a, b = _cut(A, ar, ac, dtype, absolute), _cut(B, br, bc, dtype, absolute)
    if mode == "NT":
        c = a @ b.t()
    elif mode == "NN":
        c = a @ b
    else:
        c = a.t() @ b
    if bias is not None:
        bv = bias[:N].to(dtype)
        c = c + (bv.abs() if absolute else bv)
    if residual is not None:
        c = c + _cut(residual, M, N, dtype, absolute)
    if base is not None:
        c = c + _cut(base, M, N, dtype, absolute)
    return c


def ref_of(mode, A, B, shape=None, **kw):
    """(ref, A, n) of one GEMM (+ linear epilogue terms) as a ``conv_oracle._triple``."""
    return _triple(lambda T, a: gemm_ref(mode, T(A), T(B), absolute=a, shape=shape,
                                         **{k: T(v) for k, v in kw.items()}))


# ---------------------------------------------------------------------------- nonlinear epilogues
def _acc_a(r, exact, bf16_partials=False):
    if exact:
        return torch.zeros_like(r.A)
    a = 2.0 * r.n.double() * 2.0 ** -24 * r.A.double()
    return a + 2.0 ** -8 * r.A.double() if bf16_partials else a


def act_ref(act, r, aux=None):
    """The oracle value of an activation epilogue: f(z) for z = r.ref, or acc * gelu'(aux) for dgelu."""
    if act == "gelu":
        return gelu_ref(r.ref, F64)
    if act == "tanh":
        return torch.tanh(r.ref)
    if act == "relu":
        return torch.clamp_min(r.ref, 0.0)
    if act == "dgelu":
        return r.ref * gelu_grad_ref(aux.double(), F64)
    raise ValueError(act)


def act_tol(act, r, out_dtype, exact, aux=None):
    """Per-element bound of a nonlinear epilogue (module docstring); ``r``: the pre-activation's triple
    (dgelu: the accumulator's)."""
    a = _acc_a(r, exact)
    f = act_ref(act, r, aux)
    z = r.ref.abs()
    if act == "gelu":
        t = GELU_LIP * a + (0.5 * ERF_ABS_ERR) * z + EVAL_ROUNDINGS * torch.maximum(z, f.abs())
    elif act == "tanh":
        t = a + TANH_ULPS * f.abs()
    elif act == "dgelu":
        g = gelu_grad_ref(aux.double(), F64).abs()
        t = g * a + (0.5 * ERF_ABS_ERR + EVAL_ROUNDINGS * GELU_LIP) * z
    else:
        raise ValueError(act)
    return t + half_ulp_t(f.abs() + t, out_dtype)


def act_ratio(got, act, r, out_dtype, exact, aux=None) -> float:
    if not bool(torch.isfinite(got.double()).all()):
        return float("inf")
    err = (got.double() - act_ref(act, r, aux)).abs()
    t = act_tol(act, r, out_dtype, exact, aux)
    q = torch.where(err > 0, err / t, torch.zeros_like(err))
    return float(q.max()) if q.numel() else 0.0


def tol_twice(r, base, out_dtype, bf16_partials=False):
    """``conv_oracle.tol`` plus the first of two roundings of a kernel that rounds the product sum to
    bf16 before it adds the base (ddl_gemm_duo_tn, one split, accumulate)."""
    a = _acc_a(r, False, bf16_partials)
    first = half_ulp_t((r.ref - base.double()).abs() + a, BF)
    return tol(r.ref, r.A, r.n, out_dtype, bf16_partials) + first


def ratio_twice(got, r, base, out_dtype, bf16_partials=False) -> float:
    if not bool(torch.isfinite(got.double()).all()):
        return float("inf")
    err = (got.double() - r.ref).abs()
    t = tol_twice(r, base, out_dtype, bf16_partials)
    q = torch.where(err > 0, err / t, torch.zeros_like(err))
    return float(q.max()) if q.numel() else 0.0


# ---------------------------------------------------------------------------- operands
def _vmax(K):
    """Magnitudes of the exact tier's operands: short reductions get larger integers so that a sum of
    K products is rarely 0 (K = 8: |a b| <= 20, A <= 160)."""
    return (5, 4) if K <= 8 else (3, 2)


# cases whose default seed gives a zero among very few outputs (8 elements: one zero is 12 %)
SEEDS = {("NN", 1, 8, 8): 1}


def gemm_case(tier, mode, M, N, K, seed=0, vmax=None):
    """Every operand of one case from one seeded CPU generator: a, b (tight, storage order), bias (bf16;
    ``bias32`` the same values in fp32), res, aux (a stored pre-activation for dgelu / the BatchNorm
    input for bnb), base (bf16-representable fp32), mask bits, mean, istd."""
    seed += SEEDS.get((mode, M, N, K), 0)
    g = gen(7000 + seed + MODE_ID[mode] * 1000003 + M * 10007 + N * 101 + K)
    (ar, ac), (br, bc), _ = extents(mode, M, N, K)
    va, vb = vmax or _vmax(K)
    d = density(K)
    o = {"a": operand(tier, g, (ar, ac), va, d), "b": operand(tier, g, (br, bc), vb, d, K ** -0.5),
         "bias": operand(tier, g, (N,), 3, 1.0), "res": operand(tier, g, (M, N), 3, 1.0),
         "aux": operand(tier, g, (M, N), 3, 1.0), "base": operand(tier, g, (M, N), 3, 1.0).float(),
         "bits": torch.rand((M, N), generator=g) > 0.3}
    o["bias32"] = o["bias"].float()
    if tier == "exact":
        o["mean"] = torch.randint(-2, 3, (N,), generator=g).float()
        o["istd"] = torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (N,), generator=g)]
    else:
        o["mean"] = torch.randn(N, generator=g) * 0.1
        o["istd"] = torch.rand(N, generator=g) + 0.5
    return o


LINEAR_EPIS = {"plain": (), "bias": ("bias",), "res": ("res",), "bias_res": ("bias", "res"), "acc": ("base",)}
_KW = {"bias": "bias", "res": "residual", "base": "base"}


@functools.lru_cache(maxsize=None)
def case_refs(tier, mode, M, N, K, device="cpu", vmax=None, epis=None):
    """(operands, {epilogue: Ref}) of one case: the linear epilogues (``LINEAR_EPIS``), the masked
    BatchNorm-backward values ``bnb_res{0,1}_mask{0,1}`` and, in ``Ref.stats``, the oracle's statistics
    rows with their absolute sums.  Computed once (fp64, on ``device``) and shared, never modified."""
    o = {k: v.to(device) for k, v in gemm_case(tier, mode, M, N, K, vmax=vmax).items()}
    refs = {}
    for name, terms in LINEAR_EPIS.items():
        if epis is not None and name not in epis:
            continue
        refs[name] = ref_of(mode, o["a"], o["b"], **{_KW[t]: o[t] for t in terms})
    if epis is None:        # (no column statistics at the 65537-row shape: the sums would pass 2^24)
        refs["plain"].stats = (bn_stats_rows(refs["plain"].ref), bn_stats_rows(refs["plain"].ref, absolute=True))
    if mode != "TN" and epis is None:
        for with_res in (0, 1):
            for with_mask in (0, 1):
                src = refs["res" if with_res else "plain"]
                m = o["bits"].to(F64) if with_mask else torch.ones_like(src.ref)
                r = SimpleNamespace(ref=src.ref * m, A=src.A * m, n=src.n * m)
                r.stats = (bnb_sums(r.ref, o["aux"], o["mean"], o["istd"]),
                           bnb_sums(r.ref, o["aux"], o["mean"], o["istd"], absolute=True))
                refs[f"bnb_res{with_res}_mask{with_mask}"] = r
    return o, refs


def pad_ld(t, ld):
    """``t`` [rows, cols] inside [rows, ld] storage whose gaps hold 0xFF bytes (NaN in bf16 and fp32)."""
    nbytes = t.shape[0] * ld * t.element_size()
    out = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=t.device).view(t.dtype).view(t.shape[0], ld)
    out[:, :t.shape[1]] = t
    return out


# ---------------------------------------------------------------------------- case tables
def _tn(shape):
    """The TN version of a listed shape: M rounded up to 8 (module docstring)."""
    M, N, K = shape
    return (-(-M // 8) * 8, N, K)


SMALL_SHAPES = [(1, 8, 8), (129, 136, 72), (130, 72, 200)]
NARROW_SHAPES = [(129, 64, 72), (70, 192, 136)]
TNARROW_SHAPES = [(64, 72, 200), (40, 136, 520)]
BIG_SHAPES = [(256, 256, 64), (257, 264, 72), (300, 520, 136)]
HUGE_SHAPE = (65537, 256, 512)          # 257 tiles of 256 x 256; hybrid_rows -> (65536, 2)
HUGE_EPIS = ("plain", "bias", "bias_res")
HUGE_VMAX = (2, 2)                      # 16.8 M outputs: A <= 256 needs a 10-sigma margin (E[A] = 90, sigma = 16)
BIG192_SHAPES = [(257, 192, 72), (300, 384, 136)]
DUO_SHAPES = [(257, 128, 32), (130, 128, 160), (300, 256, 96)]
DUO_BNB_SHAPE = (257, 128, 96)
DUO_TN_CASES = [((256, 128, 32), (1,)), ((256, 128, 160), (1, 5)), ((512, 256, 96), (1, 2, 3))]
WG_CASES = [((256, 128, 128), (1,)), ((256, 128, 384), (1, 3)), ((512, 256, 256), (2,))]
SWG_SHAPES = [(64, 64, 8192), (512, 128, 8192 + 17), (256, 256, 8200)]
SWG_GRIDS = (0, 3)
SKINNY_NK = [(256, 64), (64, 256)]
SKINNY_MG = [(1, 0), (64, 0), (64 * 3 + 5, 2), (64 * 5, 3)]
STREAM_NK = [(512, 128), (128, 512), (1024, 256), (256, 1024)]
STREAM_MG = [(1, 0), (32 * 3 + 5, 2), (32 * 9, 3)]
OUTS = ("fresh_bf16", "acc_bf16", "acc_f32")
LINEAR_SHAPES = [(130, 72, 136), (128, 64, 2), (128, 64, 5)]      # (tokens, in, out); out = 2, 5: the N-padded path
LINEAR_ACTS = (None, "gelu", "tanh", "relu")


def _linear_cases():
    """(tier, shape, act, bias): every act where ``ops.linear`` has it (the padded heads have no GELU and
    run once without a bias instead); the exact tier where dZ is exact (no activation, relu)."""
    out = []
    for shape in LINEAR_SHAPES:
        acts = [(a, True) for a in LINEAR_ACTS if not (shape[2] % 8 and a == "gelu")]
        if shape[2] % 8:
            acts.append((None, False))
        out += [(t, shape, a, b) for a, b in acts for t in TIERS if t == "real" or a in (None, "relu")]
    return out


LINEAR_CASES = _linear_cases()
FFN_SHAPE = (300, 64, 192)                                        # (M, H, I)


def mode_shape(mode, shape):
    return _tn(shape) if mode == "TN" else shape


def gemm_cases():
    """(mode, (M, N, K), vmax) of every case the GPU file builds through ``case_refs``."""
    seen = []

    def add(mode, shape, vmax=None):
        c = (mode, mode_shape(mode, shape), vmax)
        if c not in seen:
            seen.append(c)
    for shapes, modes in ((SMALL_SHAPES, MODES), (NARROW_SHAPES, MODES), (TNARROW_SHAPES, ("TN",)),
                          (BIG_SHAPES, MODES), (BIG192_SHAPES, ("NT", "NN")), (DUO_SHAPES + [DUO_BNB_SHAPE], ("NT", "NN")),
                          ([s for s, _ in DUO_TN_CASES], ("TN",)), ([s for s, _ in WG_CASES], ("TN",)),
                          (SWG_SHAPES, ("TN",))):
        for mode in modes:
            for s in shapes:
                add(mode, s)
    for N, K in SKINNY_NK:
        for M, _ in SKINNY_MG:
            add("NT", (M, N, K))
    for N, K in STREAM_NK:
        for M, _ in STREAM_MG:
            add("NT", (M, N, K))
    return seen


def exact_keys():
    """(label, mode, shape, vmax, epilogue name) of every exact-tier check the GPU file compares bit for
    bit -- names only, nothing computed (``exact_ref`` builds one)."""
    for mode, shape, vmax in gemm_cases() + [("NT", HUGE_SHAPE, HUGE_VMAX), ("NN", HUGE_SHAPE, HUGE_VMAX)]:
        names = list(HUGE_EPIS) if shape == HUGE_SHAPE else list(LINEAR_EPIS)
        if mode != "TN" and shape != HUGE_SHAPE:
            names += [f"bnb_res{r}_mask{m}" for r in (0, 1) for m in (0, 1)]
        for k in names:
            yield f"{mode}{shape}:{k}", mode, shape, vmax, k


_huge = {}      # the refs of the last 65537-row case asked for (1.3 GB: never more than one alive)


def exact_ref(mode, shape, vmax, name):
    M, N, K = shape
    if shape != HUGE_SHAPE:
        return case_refs("exact", mode, M, N, K, "cpu", vmax)[1][name]
    if mode not in _huge:
        _huge.clear()
        _huge[mode] = case_refs.__wrapped__("exact", mode, M, N, K, "cpu", vmax, HUGE_EPIS)[1]
    return _huge[mode][name]


# ---------------------------------------------------------------------------- verdicts (CPU self-test)
def passes(tier, got, r, out_dtype, bf16_partials=False) -> bool:
    """The GPU file's verdict on one output: bit equality (exact) or max |err| / tol <= 1 (real)."""
    if tier == "exact":
        return torch.equal(got.double(), r.ref)
    return ratio(got, r.ref, r.A, r.n, out_dtype, bf16_partials) <= 1.0


def rows_pass(tier, rows, want, absum, n) -> bool:
    """Statistics rows: bit equality (exact) or within n 2^-24 sum |term| of ``want`` (real)."""
    for g, w_, a in zip(rows, want, absum):
        g, w_, a = g.double(), w_.double(), a.double()
        if tier == "exact":
            if not torch.equal(g, w_):
                return False
            continue
        err = (g - w_).abs()
        if not bool(torch.isfinite(g).all()) or bool((err > n * 2.0 ** -24 * a).any()):
            return False
    return True


def gaps_intact(storage, cols) -> bool:
    """Every gap element of NaN-padded [rows, ld] storage still holds its 0xFF bytes."""
    gap = storage[:, cols:].contiguous()
    return bool((gap.view(torch.uint8) == 0xFF).all())


# ---------------------------------------------------------------------------- the autograd path
def linear_case(tier, M, K, N, seed=0):
    """x [M, K], w [N, K], b [N], dy [M, N] of one ``ops.linear`` case (K: in, N: out features)."""
    g = gen(9000 + seed + M * 10007 + K * 101 + N)
    va, vb = _vmax(K)
    return {"x": operand(tier, g, (M, K), va, density(K)), "w": operand(tier, g, (N, K), vb, 1.0 if N % 8 else density(K), K ** -0.5),     # (heads: no zero column of dx)
            "b": operand(tier, g, (N,), 3, 1.0),
            # dy: sparse for the reduction over M (dW); the 2- / 5-wide heads get a dense +-1 dy, so that no
            # row of dx (a sum of 2 or 5 terms) is entirely 0
            "dy": operand(tier, g, (M, N), 1 if N % 8 else 2, 1.0 if N % 8 else density(M))}


def ffn_case(seed=0):
    """The FFN handoff's operands (real tier: its dZ is a rounded nonlinear output, never exact)."""
    tier = "real"
    M, H, I = FFN_SHAPE
    g = gen(9500 + seed)
    return {"x": operand(tier, g, (M, H), 3, density(H)), "w1": operand(tier, g, (I, H), 2, density(H), H ** -0.5),
            "b1": operand(tier, g, (I,), 3, 1.0), "w2": operand(tier, g, (H, I), 2, density(I), I ** -0.5),
            "b2": operand(tier, g, (H,), 3, 1.0), "dy": operand(tier, g, (M, H), 2, density(M))}
