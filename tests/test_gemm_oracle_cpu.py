"""The GEMM oracle (tests/gemm_oracle.py) checked on the CPU: its three modes against each other and
against ``conv_oracle.conv_fwd`` for a 1x1 convolution; the exact tier's conditions on every case the GPU
file runs (built from the same case tables and seeds): A <= 256 everywhere, statistics sums below 2^24
term-wise, at most 5 % of the elements that have a term are 0 and no row or column with a term is
entirely 0 (a kernel that leaves a tile unwritten or zero cannot pass; masked elements of the
BatchNorm-backward epilogue have no term and must be 0; a row or column of a single element is an element
and falls under the 5 % rule); and a mutation self-test: a torch emulation of the kernel contract (fp32
products accumulated in K-steps of 64, optional bf16 split-K partials, one round-to-nearest store) passes
both tiers, and each subtly wrong variant of it fails the tier the GPU file would catch it in.
"""
from types import SimpleNamespace

import pytest
import torch

import conv_oracle as CO
import gemm_oracle as O

BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
REL = 1e-12


def _close(a, b):
    scale = float(b.abs().max()) or 1.0
    assert a.shape == b.shape
    assert float((a - b).abs().max()) <= REL * scale, float((a - b).abs().max()) / scale


# ---------------------------------------------------------------------------- self-consistency
@pytest.mark.parametrize("absolute", [False, True])
def test_modes_agree_on_transposed_operands(absolute):
    torch.manual_seed(1)
    M, N, K = 13, 24, 40
    a, b = torch.randn(M, K, dtype=F64), torch.randn(N, K, dtype=F64)
    bias, res, base = torch.randn(N, dtype=F64), torch.randn(M, N, dtype=F64), torch.randn(M, N, dtype=F64)
    kw = dict(bias=bias, residual=res, base=base, absolute=absolute)
    nt = O.gemm_ref("NT", a, b, **kw)
    _close(O.gemm_ref("NN", a, b.t().contiguous(), **kw), nt)
    _close(O.gemm_ref("TN", a.t().contiguous(), b.t().contiguous(), **kw), nt)
    ab = (lambda t: t.abs()) if absolute else (lambda t: t)
    _close(nt, torch.einsum("mk,nk->mn", ab(a), ab(b)) + ab(bias) + ab(res) + ab(base))
    # padded storage: the gaps (NaN) are never read
    ap, bp, rp = O.pad_ld(a, K + 8), O.pad_ld(b, K + 8), O.pad_ld(res, N + 8)
    _close(O.gemm_ref("NT", ap, bp, bias=bias, residual=rp, base=O.pad_ld(base, N + 8), absolute=absolute,
                      shape=(M, N, K)), nt)
    r = O.ref_of("NT", a, b, bias=bias, residual=res)
    assert bool((r.n == K + 2).all())


@pytest.mark.parametrize("absolute", [False, True])
def test_nt_is_a_1x1_convolution(absolute):
    torch.manual_seed(2)
    M, N, K = 21, 16, 24
    a, b = torch.randn(M, K, dtype=F64), torch.randn(N, K, dtype=F64)
    bias, res = torch.randn(N, dtype=F64), torch.randn(M, N, dtype=F64)
    y = CO.conv_fwd(a.view(1, M, 1, K), b.view(N, 1, 1, K), 1, 0, res=res.view(1, M, 1, N), bias=bias,
                    absolute=absolute)
    _close(O.gemm_ref("NT", a, b, bias=bias, residual=res, absolute=absolute), y.view(M, N))


def _one_term(ref):
    return SimpleNamespace(ref=ref, A=ref.abs(), n=torch.ones_like(ref))


def test_activation_bounds():
    z = _one_term(torch.tensor([[0.0, 1.5, -3.0]], dtype=F64))
    for act in ("gelu", "tanh"):
        f = O.act_ref(act, z)
        assert O.act_ratio(f.to(BF), act, z, BF, True) <= 1.0            # one correct rounding passes
        assert O.act_ratio((f * 1.01).to(BF), act, z, BF, True) > 1.0    # a percent off does not
    aux = torch.tensor([[0.5, -1.0, 2.0]], dtype=BF)
    f = O.act_ref("dgelu", z, aux)
    assert O.act_ratio(f.to(BF), "dgelu", z, BF, True, aux) <= 1.0
    assert O.act_ratio((f * 1.01).to(BF), "dgelu", z, BF, True, aux) > 1.0


# ---------------------------------------------------------------------------- exact-tier conditions
_KEYS = list(O.exact_keys())      # names only: every reference is built inside its test


def test_exact_cases_cover_every_family():
    labels = [k[0] for k in _KEYS]
    assert len(labels) == len(set(labels))
    for mode in O.MODES:
        for s in O.SMALL_SHAPES + O.NARROW_SHAPES + O.BIG_SHAPES:
            assert f"{mode}{O.mode_shape(mode, s)}:acc" in labels
    for s in O.DUO_SHAPES + O.BIG192_SHAPES:
        assert f"NN{s}:bias_res" in labels
    for s in O.SWG_SHAPES + [c for c, _ in O.WG_CASES + O.DUO_TN_CASES] + O.TNARROW_SHAPES:
        assert f"TN{s}:acc" in labels
    for N, K in O.SKINNY_NK + O.STREAM_NK:
        assert f"NT{(1, N, K)}:bnb_res0_mask1" in labels
    assert f"NT{O.HUGE_SHAPE}:bias_res" in labels and f"NN{O.HUGE_SHAPE}:plain" in labels


def _conditions(label, r, nz_min=0.95):
    assert r.ref.shape == r.A.shape == r.n.shape
    assert float(r.A.max()) <= O.EXACT_A_MAX, f"{label}: max A = {float(r.A.max())}"
    assert bool((r.ref == r.ref.round()).all()), f"{label}: the oracle is not integer-valued"
    has = r.n > 0
    assert bool((r.ref[~has] == 0).all()) and bool((r.A[~has] == 0).all())
    assert float(has.double().mean()) >= 0.5, f"{label}: hardly any element has a term"
    nonzero = r.ref != 0
    nz = float(nonzero[has].double().mean())
    assert nz >= nz_min, f"{label}: only {nz:.3f} of the elements with a term are nonzero"
    if r.ref.dim() == 2:
        M, N = r.ref.shape
        if N > 1:
            assert bool(nonzero.any(1)[has.any(1)].all()), f"{label}: an output row is entirely 0"
        if M > 1:
            assert bool(nonzero.any(0)[has.any(0)].all()), f"{label}: an output column is entirely 0"


@pytest.mark.parametrize("label,mode,shape,vmax,name", _KEYS, ids=[k[0] for k in _KEYS])
def test_exact_case_conditions(label, mode, shape, vmax, name):
    r = O.exact_ref(mode, shape, vmax, name)
    _conditions(label, r)
    if getattr(r, "stats", None) is not None:
        for s in r.stats[1]:
            assert float(s.max()) < O.EXACT_STAT_MAX, f"{label}: statistics sum {float(s.max())}"
        for s in r.stats[0]:
            assert bool((s * 2 == (s * 2).round()).all())      # istd in {0.5, 1, 2}: halves at the worst


@pytest.mark.parametrize("shape", O.LINEAR_SHAPES, ids=str)
def test_autograd_exact_cases(shape):
    """The exact-tier ``ops.linear`` cases (no activation, relu): the forward, dx, dW and db references
    meet the exact tier's conditions.  (dx and dW of the relu case use a masked dy: fewer terms, A no larger.)"""
    M, K, N = shape
    o = O.linear_case("exact", M, K, N)
    _conditions(f"linear{shape}:fwd", O.ref_of("NT", o["x"], o["w"], bias=o["b"]))
    _conditions(f"linear{shape}:fwd nobias", O.ref_of("NT", o["x"], o["w"]))
    # dx of the 2- / 5-wide heads is a sum of 2 / 5 products: zeros are frequent, whole rows of them are not
    _conditions(f"linear{shape}:dx", O.ref_of("NN", o["dy"], o["w"]), nz_min=0.7 if N % 8 else 0.95)
    _conditions(f"linear{shape}:dw", O.ref_of("TN", o["dy"], o["x"]))
    assert float(o["dy"].double().abs().sum(0).max()) <= O.EXACT_A_MAX
    assert ("exact", shape, "relu", True) in O.LINEAR_CASES and ("exact", shape, "gelu", True) not in O.LINEAR_CASES


# ---------------------------------------------------------------------------- emulation and mutants
def _rn(v, dtype):
    return v.to(dtype)


def _trunc_bf16(v):
    """fp32 -> bf16 by dropping the low 16 bits (no rounding)."""
    return (v.float().contiguous().view(torch.int32) & -65536).view(F32).to(BF)


def emulate(mode, o, shape, epi="plain", out_dtype=BF, splits=1, bf16_partials=False, ldc=None, stats=False,
            mutant=None):
    """The kernel contract in torch: fp32 products accumulated in K-steps of 64, split-K slabs (rounded to
    bf16 where the kernel stores bf16 partials) summed in fp32 with the epilogue terms, one
    round-to-nearest store into [M, ldc] storage whose gaps keep their 0xFF bytes.  Returns the storage
    and, with ``stats``, the rows [sum C | sum C^2] of the stored output.  ``mutant`` names one error."""
    M, N, K = shape
    a, b = o["a"].float(), o["b"].float()
    if mode == "TN":
        a = a.t()
    if mode != "NT":
        b = b.t()                                      # a [M, K], b [N, K]
    a, b = a.contiguous(), b.contiguous()
    if mutant == "tail_row":
        a = a.clone()
        a[M - 1] = a[M - 2]
    kend = K - 8 if mutant == "drop_k" else K
    steps = list(range(0, kend, 64))
    per = -(-len(steps) // splits)
    slabs = []
    for s in range(splits):
        acc = torch.zeros(M, N, dtype=F32)
        for k0 in steps[s * per:(s + 1) * per]:
            k1 = min(k0 + 64, kend)
            acc = acc + a[:, k0:k1] @ b[:, k0:k1].t()
        slabs.append(acc.to(BF).float() if (bf16_partials and (splits > 1 or bf16_partials == "always")) else acc)
    if mutant == "slab_twice":
        slabs.append(slabs[min(1, len(slabs) - 1)])
    v = slabs[0]
    for s in slabs[1:]:
        v = v + s
    raw = v.clone()
    terms = O.LINEAR_EPIS[epi]
    if "bias" in terms:
        bias = o["bias"].float()
        v = v + (torch.roll(bias, 1) if mutant == "bias_shift" else bias)
    if "res" in terms:
        v = v + o["res"].float()
    if "base" in terms and mutant != "overwrite":
        v = v + o["base"].to(out_dtype).float()
    if mutant == "transpose_block":
        v = v.clone()
        v[:16, :16] = v[:16, :16].t().clone()
    c = _trunc_bf16(v) if (mutant == "trunc" and out_dtype == BF) else _rn(v, out_dtype)
    ldc = N if ldc is None else ldc
    store = O.pad_ld(c, ldc)
    if mutant == "gap_write":
        store[M // 2, N:N + 8] = 1.0
    if not stats:
        return store
    src = raw if mutant == "stats_from_acc" else c.float()
    return store, (src.sum(0), (src * src).sum(0))


EMU_CASES = [("NT", (130, 72, 200)), ("NN", (129, 136, 72)), ("TN", (136, 72, 200))]
_IDS = [m for m, _ in EMU_CASES]


def _verdict(tier, mode, shape, epi="plain", out_dtype=BF, splits=1, bf16_partials=False, mutant=None):
    M, N, K = shape
    o, refs = O.case_refs(tier, mode, M, N, K)
    store = emulate(mode, o, shape, epi, out_dtype, splits, bf16_partials, ldc=N + 8, mutant=mutant)
    return O.passes(tier, store[:, :N], refs[epi], out_dtype, bool(bf16_partials)) and O.gaps_intact(store, N)


@pytest.mark.parametrize("tier", O.TIERS)
@pytest.mark.parametrize("mode,shape", EMU_CASES, ids=_IDS)
def test_emulation_is_accepted(tier, mode, shape):
    for epi in O.LINEAR_EPIS:
        for dt in ((BF, F32) if epi in ("plain", "acc") else (BF,)):
            assert _verdict(tier, mode, shape, epi, dt), (epi, dt)
            assert _verdict(tier, mode, shape, epi, dt, splits=3), (epi, dt, "split 3")
    assert _verdict(tier, mode, shape, "acc", BF, splits=3, bf16_partials=True)
    assert _verdict(tier, mode, shape, "plain", BF, splits=1, bf16_partials="always")
    M, N, K = shape
    o, refs = O.case_refs(tier, mode, M, N, K)
    store, rows = emulate(mode, o, shape, stats=True)
    c = store[:, :N]
    assert O.rows_pass(tier, rows, refs["plain"].stats[0] if tier == "exact" else O.bn_stats_rows(c),
                       O.bn_stats_rows(c, absolute=True), M)


BOTH = [("drop_k", "plain", 1), ("tail_row", "plain", 1), ("transpose_block", "plain", 1), ("bias_shift", "bias", 1),
        ("slab_twice", "plain", 3), ("overwrite", "acc", 1)]


@pytest.mark.parametrize("tier", O.TIERS)
@pytest.mark.parametrize("mutant,epi,splits", BOTH, ids=[m for m, _, _ in BOTH])
@pytest.mark.parametrize("mode,shape", EMU_CASES, ids=_IDS)
def test_mutants_are_rejected_in_both_tiers(tier, mode, shape, mutant, epi, splits):
    assert _verdict(tier, mode, shape, epi, BF, splits)
    assert not _verdict(tier, mode, shape, epi, BF, splits, mutant=mutant)
    if mutant in ("drop_k", "slab_twice", "overwrite"):
        assert not _verdict(tier, mode, shape, epi, F32 if epi != "bias" else BF, splits, mutant=mutant)


@pytest.mark.parametrize("mode,shape", EMU_CASES, ids=_IDS)
def test_truncating_store_is_rejected_in_the_real_tier(mode, shape):
    assert not _verdict("real", mode, shape, mutant="trunc")
    assert _verdict("exact", mode, shape, mutant="trunc")       # integers up to 256: nothing to truncate


@pytest.mark.parametrize("mode,shape", EMU_CASES, ids=_IDS)
def test_statistics_of_the_accumulator_are_rejected(mode, shape):
    """Rows summed from the fp32 accumulator instead of the stored bf16: caught in the real tier; in the
    exact tier the accumulator *is* the stored value (an integer of at most 256), so the two cannot differ
    there and the rows pass -- which is why the exact tier compares them with the oracle's, bit for bit."""
    M, N, K = shape
    o, refs = O.case_refs("real", mode, M, N, K)
    store, rows = emulate(mode, o, shape, stats=True, mutant="stats_from_acc")
    c = store[:, :N]
    assert not O.rows_pass("real", rows, O.bn_stats_rows(c), O.bn_stats_rows(c, absolute=True), M)
    o, refs = O.case_refs("exact", mode, M, N, K)
    store, rows = emulate(mode, o, shape, stats=True, mutant="stats_from_acc")
    assert O.rows_pass("exact", rows, refs["plain"].stats[0], refs["plain"].stats[1], M)
    bad = (rows[0] + 1.0, rows[1])
    assert not O.rows_pass("exact", bad, refs["plain"].stats[0], refs["plain"].stats[1], M)


@pytest.mark.parametrize("tier", O.TIERS)
@pytest.mark.parametrize("mode,shape", EMU_CASES, ids=_IDS)
def test_write_into_the_ldc_gap_is_rejected(tier, mode, shape):
    M, N, K = shape
    o, refs = O.case_refs(tier, mode, M, N, K)
    store = emulate(mode, o, shape, ldc=N + 16, mutant="gap_write")
    assert O.passes(tier, store[:, :N], refs["plain"], BF)      # the result itself is right ...
    assert not O.gaps_intact(store, N)                          # ... the guard check is what fails
    assert O.gaps_intact(emulate(mode, o, shape, ldc=N + 16), N)
