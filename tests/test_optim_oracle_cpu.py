"""The flat optimizers' torch path against the independent fp64 oracle (no GPU needed).

``tests/optim_oracle.py`` holds the oracle (``torch.optim`` / a written-out LAMB, per tensor,
float64), the fixture (seven tensors around the 8192-element table split, five steps with one
10x gradient, an lr change and an always-zero gradient) and the per-step checks.  The kernels
run the same cases in ``test_optim_oracle_gpu.py``.
"""
import pytest
import torch

import optim_oracle as O

F32, BF16 = torch.float32, torch.bfloat16
CPU = torch.device("cpu")

# (optimizer, hyper-parameter overrides)
VARIANTS = [
    ("sgd", {}),
    ("sgd", {"nesterov": True}),
    ("sgd", {"momentum": 0.0}),
    ("adamw", {}),
    ("lamb", {}),
    ("lamb", {"bias_correction": False}),
]


@pytest.fixture(autouse=True)
def _torch_path():
    from databricks_distributed_deep_learning_amd.ops import _lib
    _lib.set_mode("off")


def _ids(v):
    return "-".join([v[0]] + [f"{k}={x}" for k, x in v[1].items()]) if isinstance(v, tuple) else None


@pytest.mark.parametrize("clip", [0.0, 1.0], ids=["noclip", "clip"])
@pytest.mark.parametrize("variant", VARIANTS, ids=_ids)
def test_torch_path_matches_oracle(variant, clip):
    kind, over = variant
    hp = O.default_hp(kind, max_grad_norm=clip, **over)
    run = O.FlatRun(kind, CPU, F32, F32, hp, nan_buffer=(hp.get("momentum") == 0.0))
    if clip:
        on, off = run.clip_activity()
        assert on > 0 and off > 0, (on, off)
    run.run()
    print(run.report())


@pytest.mark.parametrize("pdtype,gdtype", [(BF16, BF16), (BF16, F32)], ids=["bf16-bf16", "bf16-f32grad"])
@pytest.mark.parametrize("kind", ["sgd", "adamw", "lamb"])
def test_torch_path_bf16_model_matches_oracle(kind, pdtype, gdtype):
    run = O.FlatRun(kind, CPU, pdtype, gdtype, O.default_hp(kind, max_grad_norm=1.0)).run()
    print(run.report())


@pytest.mark.parametrize("kind", ["sgd", "adamw", "lamb"])
def test_torch_path_range_steps_match_oracle(kind):
    """begin_step / step_range / end_step with the ranges handed over last bucket first."""
    run = O.FlatRun(kind, CPU, BF16, BF16, O.default_hp(kind)).run(ranges=True)
    print(run.report())


@pytest.mark.parametrize("pdtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("kind", ["sgd", "adamw", "lamb"])
def test_torch_path_resume_is_bitwise(kind, pdtype):
    """state_dict() after step 2 -> fresh arena and optimizer -> load_state_dict(): steps 3..5
    give the bits of the uninterrupted run (SGD's first-step rule and both bias corrections
    hang on the restored step count)."""
    hp = O.default_hp(kind, max_grad_norm=1.0)
    whole = O.FlatRun(kind, CPU, pdtype, pdtype, hp).run()
    resumed = O.FlatRun(kind, CPU, pdtype, pdtype, hp).run(resume_at=2)
    for s, (a, b) in enumerate(zip(whole.snaps, resumed.snaps)):
        for k in a:
            assert O.same_bits(a[k], b[k]), f"{kind} step {s + 1}: {k} differs after the resume"


@pytest.mark.parametrize("kind", ["sgd", "adamw"])
def test_torch_path_sharded_matches_oracle(kind, monkeypatch):
    """ZeRO-1 rank 0 of 2, two buckets, collectives stubbed: owned elements follow the oracle."""
    from databricks_distributed_deep_learning_amd.optim import flat as F_
    monkeypatch.setattr(F_, "_sum_over_ranks", lambda t: None)
    run = O.FlatRun(kind, CPU, BF16, BF16, O.default_hp(kind), shard=True).run()
    print(run.report())


@pytest.mark.parametrize("nesterov", [False, True], ids=["plain", "nesterov"])
def test_torch_path_sgd_exact(nesterov):
    """Small-integer inputs and dyadic hyper-parameters: every intermediate is exact in fp32, so
    the result must EQUAL the fp64 oracle (and the fp32 oracle must, which makes the test valid)."""
    hp = O.default_hp("sgd", lr=0.5, momentum=0.5, weight_decay=0.25, nesterov=nesterov)
    O.FlatRun("sgd", CPU, F32, F32, hp, integers=True, steps=3, exact=True).run()


def test_oracle_sees_both_decay_kinds_and_the_table_edges():
    """The fixture is what the issue asks for: both decay kinds, the sizes around the 8192 split."""
    arena = O.make_arena(CPU, F32)
    by = {e.name: e for e in arena.entries}
    assert sorted(e.numel for e in arena.entries) == [5, 21, 129, 8192, 8193, 8643, 24616]
    assert {n for n, e in by.items() if e.decay} == {"fc1.weight", "fc2.weight", "big.weight"}
    assert not by["norm.weight"].decay and len(by["norm.weight"].shape) == 2
    assert not bool(by["head.bias"].param.any())
    grads = O.make_grads(arena, F32)
    z = by[O.ZERO_GRAD]
    assert all(not bool(g[z.offset:z.offset + z.numel].any()) and not bool(g[O.pad_mask(arena)].any()) for g in grads)
