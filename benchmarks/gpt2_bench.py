#!/usr/bin/env python3
"""GPT-2 causal-LM pretraining throughput on one GPU (the ``gpt2_pretrain`` preset).

    python benchmarks/gpt2_bench.py [--steps 20] [--warmup 8] [--batch-size 16] [--seq-len 1024] [--model gpt2]

Prints the training summary's headline figures and tokens/s (= samples/s * seq_len) as one JSON line.
The warm-up steps also pick the GEMM kernels of shapes the committed plan table does not hold.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--batch-size", type=int, default=16)
    ap.add_argument("--seq-len", type=int, default=1024)
    ap.add_argument("--model", default="gpt2")
    args = ap.parse_args()
    from databricks_distributed_deep_learning_amd.config import get_preset
    from databricks_distributed_deep_learning_amd.training.loop import train
    out = train(get_preset("gpt2_pretrain", model=args.model, steps=args.steps, warmup_steps=args.warmup,
                           batch_size=args.batch_size, seq_len=args.seq_len, log_every=0))
    print(json.dumps({"model": out["model"], "per_rank_batch": out["per_rank_batch"], "seq_len": out["seq_len"],
                      "params": out["params"], "ms_per_step": round(out["ms_per_step"], 2),
                      "samples_per_sec": round(out["samples_per_sec"], 2),
                      "tokens_per_sec": round(out["samples_per_sec"] * out["seq_len"], 1),
                      "final_loss": out["final_loss"], "phases_ms": out["phases_ms"],
                      "peak_mem_gb": out.get("max_allocated_gb")}))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
