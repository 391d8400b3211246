"""bench.py's command line: what a plain run measures, ``--full``, and ``--dump-outputs``."""
import os

import numpy as np
import torch

import bench


def test_plain_run_measures_the_headline_model_only():
    assert bench.parse_args([]).model == "resnet50"
    assert bench.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "2"]).steps == 7
    assert bench.parse_args(["--full"]).model == "both"
    assert bench.parse_args(["--model", "both"]).model == "both"
    assert bench.parse_args(["--full", "--model", "vit_b16"]).model == "vit_b16"
    assert bench.parse_args(["--warmup", "0"]).warmup == 1      # tuning never lands in the timed steps


def test_dump_outputs_small_arena_is_written_whole(tmp_path):
    flat = torch.arange(1000, dtype=torch.float32).to(torch.bfloat16)
    bench.dump_outputs(str(tmp_path / "d"), "m", 2.5, flat)
    loss = np.load(tmp_path / "d" / "m_loss.npy")
    params = np.load(tmp_path / "d" / "m_params.npy")
    assert loss.dtype == np.float64 and loss.tolist() == [2.5]
    assert params.dtype == np.float32 and np.array_equal(params, flat.float().numpy())


def test_dump_outputs_samples_a_large_arena_at_fixed_positions(tmp_path):
    n = bench.DUMP_MAX_ELEMS + 12345
    flat = torch.arange(n, dtype=torch.float32)                 # value == position (exact below 2^24)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), "m", 0.0, flat)
    a, b = (np.load(tmp_path / d / "m_params.npy") for d in ("a", "b"))
    assert a.dtype == np.float32 and a.shape == (bench.DUMP_MAX_ELEMS,)
    assert np.array_equal(a, b)                                 # the same positions in every run
    assert np.all(np.diff(a) >= 0) and a.max() > 0.99 * n       # spread over the whole arena
    # the pair of models of a --full run stays below 64 MB
    assert 2 * sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")) < 64 * 2 ** 20
