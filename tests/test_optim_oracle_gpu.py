"""The fused optimizer kernels (``csrc/kernels/optim.hip``) against the independent fp64 oracle.

Same oracle, fixture and per-step checks as ``test_optim_oracle_cpu.py`` (all in
``tests/optim_oracle.py``), with the kernels in place of the torch path: after EVERY step the
fp32 master and each state tensor lie within ``4 * yard + ulp32(max|oracle|)`` of the float64
oracle, where ``yard`` is the float32 oracle's own distance from it on the same inputs; the
bf16 copy is bit-for-bit the rounded master; alignment pads stay zero.  ``global_norm`` /
``ddl_sumsq`` is checked bit for bit on 0/1 vectors past its grid cap.
"""
import math

import pytest
import torch

import optim_oracle as O
from conftest import gpu_device

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
DTYPES = [(F32, F32), (BF16, BF16), (BF16, F32)]          # (params, gradients)
DTYPE_IDS = ["f32-f32", "bf16-bf16", "bf16-f32grad"]


@pytest.fixture(autouse=True)
def _native():
    from databricks_distributed_deep_learning_amd.ops import _lib
    assert _lib.available(), _lib.load_error()
    _lib.set_mode("auto")


def _run(kind, pdtype, gdtype, hp, **kw):
    dev = gpu_device()
    run = O.FlatRun(kind, dev, pdtype, gdtype, hp, nan_buffer=(hp.get("momentum") == 0.0), **kw)
    assert run.opt._native()
    if hp["max_grad_norm"]:
        on, off = run.clip_activity()
        assert on > 0 and off > 0, (on, off)
    return run


@pytest.mark.parametrize("clip", [0.0, 1.0], ids=["noclip", "clip"])
@pytest.mark.parametrize("pdtype,gdtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("kind", ["sgd", "adamw", "lamb"])
def test_kernels_match_oracle(kind, pdtype, gdtype, clip):
    run = _run(kind, pdtype, gdtype, O.default_hp(kind, max_grad_norm=clip))
    try:
        run.run()
    finally:
        print(run.report())


@pytest.mark.parametrize("kind,over,pdtype,gdtype,clip", [
    ("sgd", {"nesterov": True}, F32, F32, 0.0),
    ("sgd", {"nesterov": True}, BF16, BF16, 1.0),
    ("sgd", {"momentum": 0.0}, F32, F32, 0.0),
    ("sgd", {"momentum": 0.0}, BF16, F32, 1.0),
    ("lamb", {"bias_correction": False}, F32, F32, 0.0),
    ("lamb", {"bias_correction": False}, BF16, BF16, 1.0),
], ids=["nesterov-f32", "nesterov-bf16-clip", "momentum0-f32", "momentum0-bf16-f32grad-clip",
        "lamb-nobias-f32", "lamb-nobias-bf16-clip"])
def test_kernel_variants_match_oracle(kind, over, pdtype, gdtype, clip):
    """Nesterov, momentum 0 (the NaN-filled buffer is neither read nor written) and LAMB without
    bias correction."""
    run = _run(kind, pdtype, gdtype, O.default_hp(kind, max_grad_norm=clip, **over))
    try:
        run.run()
    finally:
        print(run.report())


@pytest.mark.parametrize("kind,pdtype", [("sgd", BF16), ("adamw", BF16), ("lamb", BF16), ("lamb", F32)],
                         ids=["sgd-bf16", "adamw-bf16", "lamb-bf16", "lamb-f32"])
def test_kernel_range_steps_match_oracle(kind, pdtype):
    """Native begin_step / step_range / end_step, last bucket first: row subsets of the block
    table, and LAMB's per-step norm scratch shared by all ranges."""
    run = _run(kind, pdtype, pdtype, O.default_hp(kind))
    try:
        run.run(ranges=True)
    finally:
        print(run.report())


@pytest.mark.parametrize("kind,pdtype", [("sgd", BF16), ("adamw", BF16), ("lamb", BF16), ("sgd", F32)],
                         ids=["sgd-bf16", "adamw-bf16", "lamb-bf16", "sgd-f32"])
def test_kernel_resume_is_bitwise(kind, pdtype):
    """state_dict() after step 2 -> fresh arena and optimizer -> load_state_dict(): the resumed
    run follows the oracle and repeats the bits of the uninterrupted native run.  Only what the
    kernels compute in a fixed order can repeat bit for bit, so the clip is off (``ddl_sumsq``
    adds its block partials with ``atomicAdd``, and two uninterrupted clipped runs already differ
    in the last bit), and LAMB's master is exempt from the bit comparison: its trust ratios sum
    up to four block partials per tensor the same way.  LAMB's moments are elementwise and are
    compared bit for bit; its master is held to the oracle after every step."""
    hp = O.default_hp(kind)
    whole = _run(kind, pdtype, pdtype, hp).run()
    resumed = _run(kind, pdtype, pdtype, hp).run(resume_at=2)
    for s, (a, b) in enumerate(zip(whole.snaps, resumed.snaps)):
        for k in a:
            if kind == "lamb" and k in ("master", "flat"):
                continue
            assert O.same_bits(a[k], b[k]), f"{kind} step {s + 1}: {k} differs after the resume"


@pytest.mark.parametrize("kind", ["sgd", "adamw"])
def test_sharded_kernels_match_oracle(kind, monkeypatch):
    """ZeRO-1 rank 0 of 2 owning chunk 0 of two buckets (collectives stubbed): the owned elements
    follow the oracle, the unowned arena elements stay untouched."""
    from databricks_distributed_deep_learning_amd.optim import flat as F_
    monkeypatch.setattr(F_, "_sum_over_ranks", lambda t: None)
    run = _run(kind, BF16, BF16, O.default_hp(kind), shard=True)
    assert run.opt.shard == (0, 2) and run.opt.state_numel == run.arena.numel // 2
    try:
        run.run()
    finally:
        print(run.report())


@pytest.mark.parametrize("pdtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("nesterov", [False, True], ids=["plain", "nesterov"])
def test_sgd_kernel_exact(nesterov, pdtype):
    """lr=0.5, momentum=0.5, weight_decay=0.25, grad_scale=0.5 on integers in [-4, 4] for three
    steps: every intermediate is a short dyadic rational, exact in fp32 whatever the operation
    order or contraction, so a wrong formula shows as a bit difference.  Master, buffer and (for
    an fp32 model) the parameters must equal the fp64 oracle; ``FlatRun`` asserts first that the
    fp32 oracle equals the fp64 one, the condition that makes the test valid."""
    hp = O.default_hp("sgd", lr=0.5, momentum=0.5, weight_decay=0.25, nesterov=nesterov)
    _run("sgd", pdtype, pdtype, hp, integers=True, steps=3, exact=True).run()


# ---------------------------------------------------------------------------- global_norm / ddl_sumsq
GRID_CAP, LANES, VEC = 2048, 256, 8
PASS = GRID_CAP * LANES * VEC                      # elements one grid-stride pass covers
BIG = 2 * PASS + VEC * 77 + 5                      # two full passes, a ragged third, a torch-side tail


def _ones_vector(n: int) -> torch.Tensor:
    """0/1 values, ones at about a quarter of the positions and forced where a dropped element
    would otherwise go unnoticed.  The sum of squares is an integer below 2**24: every fp32
    summation order is exact."""
    g = torch.Generator().manual_seed(5)
    x = (torch.rand(n, generator=g) < 0.25).float()
    n8 = n // VEC * VEC
    x[0] = x[n - 1] = 1
    x[torch.arange(0, n, PASS)] = 1                # first element of each grid-stride pass
    x[n8 - VEC:n8] = 1                             # the last full group of 8
    x[n8:] = 1                                     # the tail
    return x


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("n", [BIG, 40, 8])
def test_global_norm_counts_every_element(n, dtype):
    dev = gpu_device()
    from databricks_distributed_deep_learning_amd.ops import _native_optim
    x = _ones_vector(n)
    count = int(x.to(torch.int64).sum())
    assert count < 2 ** 24
    want = torch.tensor(count, dtype=torch.float32).sqrt()
    got = _native_optim.global_norm(x.to(dtype).to(dev)).cpu()
    assert O.same_bits(got, want), f"global_norm = {got.item()!r}, sqrt({count}) = {want.item()!r}"


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_global_norm_randn_within_chain_bound(dtype):
    """A normal vector past the grid cap against the fp64 norm of the same (rounded) values.
    All addends are positive, so the relative error of the sum is at most the length of the
    longest addition chain times 2**-24: 3 groups x 8 squares per thread (each fused or rounded
    once more: +1), 6 wave shuffle levels, 4 wave partials, ``gridDim`` = 2048 atomics, and the
    tail's 5 squares plus its one add.  The square root halves it and rounds once."""
    dev = gpu_device()
    from databricks_distributed_deep_learning_amd.ops import _native_optim
    chain = 3 * VEC + 1 + 6 + 4 + GRID_CAP + 5 + 1
    rel_bound = chain * 2.0 ** -24 / 2 + 2.0 ** -24
    x = torch.randn(BIG, generator=torch.Generator().manual_seed(9)).to(dtype)
    want = math.sqrt(float(x.double().pow(2).sum()))
    got = float(_native_optim.global_norm(x.to(dev)))
    rel = abs(got - want) / want
    print(f"SUMSQ-ERROR {dtype} measured {rel:.3e} bound {rel_bound:.3e}")
    assert rel <= rel_bound, f"relative error {rel:.3e} > {rel_bound:.3e}"
