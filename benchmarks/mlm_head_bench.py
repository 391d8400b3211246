#!/usr/bin/env python3
"""MLM vocabulary head, forward + backward: the fused native head against the stock arm.

    python benchmarks/mlm_head_bench.py [--rows 9728] [--hidden 1024] [--vocab 30522] [--iters 30] [--out FILE]

native : ops.linear_cross_entropy (NT GEMM into one 8-padded logits buffer, ddl_ce_lse, ddl_ce_bwd in
         place, NN dgrad, TN wgrad, column sums)
stock  : F.linear in bf16, .float(), F.cross_entropy(ignore_index=-100), autograd

Both arms run in this one process on the same inputs (a third of the labels ignored), interleaved
round by round after a warm-up; the time is the median of per-iteration HIP-event times, the memory
is the peak allocated above the inputs.  Default rows = 128 sequences x 76 predictions.
"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from databricks_distributed_deep_learning_amd import ops  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=128 * 76)
    ap.add_argument("--hidden", type=int, default=1024)
    ap.add_argument("--vocab", type=int, default=30522)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    x = torch.randn(a.rows, a.hidden, device=dev).bfloat16().requires_grad_(True)
    w = (torch.randn(a.vocab, a.hidden, device=dev) * 0.02).bfloat16().requires_grad_(True)
    b = torch.zeros(a.vocab, device=dev, dtype=torch.bfloat16, requires_grad=True)
    y = torch.randint(0, a.vocab, (a.rows,), device=dev)
    y[::3] = -100

    def native():
        return ops.linear_cross_entropy(x, w, b, y, -100)

    def stock():
        return F.cross_entropy(F.linear(x, w, b).float(), y, ignore_index=-100)

    arms = {"native": native, "stock": stock}

    def once(fn):
        x.grad = w.grad = b.grad = None
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        loss = fn()
        loss.backward()
        e1.record()
        return e0, e1, loss

    times = {k: [] for k in arms}
    peak, losses = {}, {}
    for k, fn in arms.items():
        for _ in range(a.warmup):
            once(fn)
        torch.cuda.synchronize()
        x.grad = w.grad = b.grad = None
        base = torch.cuda.memory_allocated(dev)
        torch.cuda.reset_peak_memory_stats(dev)
        losses[k] = once(fn)[2].item()
        torch.cuda.synchronize()
        peak[k] = (torch.cuda.max_memory_allocated(dev) - base) / 2 ** 20
    for _ in range(a.iters):
        for k, fn in arms.items():
            e0, e1, _ = once(fn)
            torch.cuda.synchronize()
            times[k].append(e0.elapsed_time(e1))
    res = {"bench": "mlm_head", "rows": a.rows, "hidden": a.hidden, "vocab": a.vocab, "iters": a.iters,
           "device": torch.cuda.get_device_name(dev)}
    for k in arms:
        t = sorted(times[k])
        res[k] = {"ms_median": round(statistics.median(t), 4), "ms_min": round(t[0], 4), "ms_max": round(t[-1], 4),
                  "peak_mb": round(peak[k], 1), "loss": losses[k]}
    res["stock_over_native_time"] = round(res["stock"]["ms_median"] / res["native"]["ms_median"], 3)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
