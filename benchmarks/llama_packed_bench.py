#!/usr/bin/env python3
"""Packed-row pretraining on one GPU: the document-masked attention kernels against the plain causal ones.

    python benchmarks/llama_packed_bench.py [--reps 3] [--steps 10] [--warmup 6] [--skip-calls] [--skip-train]

SmolLM-135M at 8 x 2048 tokens (the ``llama_pretrain`` shape: 9 heads of 64), ``docs_per_row`` in {1, 4, 16},
the document cuts those of the synthetic loader.
(a) Per-call times of ``ops.attention(causal=True, doc_start=...)``, forward (no graph) and backward (the graph
    built once and kept), against the plain ``causal=True`` call on the same tensor, without dropout and
    with p = 0.1 (GPT-2's ``attn_pdrop``: the ``DROP`` instances).  Device events around
    back-to-back calls, the arms alternating, best of ``--reps``.  ``tiles`` is the share of the plain call's
    key tiles that the document form still visits (counted from the layout, 128-row forward workgroups).  A
    call at or below ~30 us sits on the enqueue floor and says nothing about the kernel.
(b) Step time of the ``llama_pretrain`` preset, plain and packed on the same ids (the loader draws its cuts
    from a generator of their own).  A fresh Trainer per run, the arms alternating in this one process, best
    of ``--reps``.  The packed steps include ``ops.doc_bounds``' check of every batch (a host synchronisation).
One JSON line per result.  Expectations the lines record and do not enforce: no slower than plain causal at
one document per row, and less time as the documents get shorter.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

DOCS = (1, 4, 16)
B, S, H = 8, 2048, 9
FLOOR_US = 30.0


def _events(fn, iters):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / iters      # us per call


def _tile_share(doc_start):
    """key tiles (64 keys) the forward's 128-row workgroups visit, over those of the plain causal call"""
    plain = doc = 0
    for q0 in range(0, S, 128):
        diag = min(q0 + 127, S - 1) // 64
        plain += (diag + 1) * doc_start.shape[0]
        doc += int((diag + 1 - doc_start[:, q0] // 64).sum())
    return doc / plain


def bench_calls(dev, reps, iters=30):
    import torch
    from databricks_distributed_deep_learning_amd import ops
    from databricks_distributed_deep_learning_amd.data import SyntheticTokens
    qkv = torch.randn(B, S, 3 * H * 64, device=dev).bfloat16().requires_grad_(True)
    dout = torch.randn(B, S, H * 64, device=dev).bfloat16()
    arms = {"plain": None}
    for k in DOCS:
        pos = SyntheticTokens(B, S, 1000, device=dev, pool=1, causal_lm=True, docs_per_row=k).pool[0]["position_ids"]
        arms[k] = ops.doc_bounds(pos)

    def call(doc, p):
        if doc is None:
            return ops.attention(qkv, H, None, p, True, causal=True)
        return ops.attention(qkv, H, None, p, True, causal=True, doc_start=doc)

    def fwd(doc, p):
        def run():
            with torch.no_grad():
                call(doc, p)
        return run

    def bwd(doc, p):
        out = call(doc, p)
        return lambda: torch.autograd.grad(out, qkv, dout, retain_graph=True)

    for p, phase, make in ((p, ph, mk) for p in (0.0, 0.1) for ph, mk in (("fwd", fwd), ("bwd", bwd))):
        fns = {name: make(doc, p) for name, doc in arms.items()}
        for fn in fns.values():
            fn()
            _events(fn, 5)
        best = {name: float("inf") for name in fns}
        for _ in range(reps):
            for name, fn in fns.items():
                best[name] = min(best[name], _events(fn, iters))
        for k in DOCS:
            print(json.dumps({"call": f"attention_doc_{phase}", "shape": f"[{B}, {S}, 3*{H}*64]", "p_drop": p,
                              "docs_per_row": k,
                              "us": round(best[k], 1), "plain_causal_us": round(best["plain"], 1),
                              "ratio_to_plain": round(best[k] / best["plain"], 3),
                              "tiles": round(_tile_share(arms[k][0].cpu()), 3),
                              "on_enqueue_floor": bool(best[k] <= FLOOR_US),
                              "no_slower_than_plain": bool(best[k] <= best["plain"])}), flush=True)


def bench_train(reps, steps, warmup):
    import torch
    from databricks_distributed_deep_learning_amd.config import get_preset
    from databricks_distributed_deep_learning_amd.training.loop import Trainer
    arms = (0,) + DOCS
    ms = {k: [] for k in arms}
    last = {}
    for _ in range(reps):
        for k in arms:
            t = Trainer(get_preset("llama_pretrain", docs_per_row=k, steps=steps, warmup_steps=warmup, log_every=0))
            out = t.run()
            t.close()
            del t
            torch.cuda.empty_cache()
            ms[k].append(1e3 * out["per_rank_batch"] / out["samples_per_sec"])
            last[k] = out
    plain = min(ms[0])
    for k in DOCS:
        best = min(ms[k])
        print(json.dumps({"train": last[k]["model"], "per_rank_batch": last[k]["per_rank_batch"],
                          "seq_len": last[k]["seq_len"], "docs_per_row": k, "step_ms": round(best, 2),
                          "plain_causal_step_ms": round(plain, 2), "ratio_to_plain": round(best / plain, 4),
                          "no_slower_than_plain": bool(best <= plain), "final_loss": last[k]["final_loss"],
                          "plain_final_loss": last[0]["final_loss"],
                          "step_ms_all": [round(v, 2) for v in ms[k]],
                          "plain_step_ms_all": [round(v, 2) for v in ms[0]],
                          "phases_ms": last[k].get("phases_ms"), "plain_phases_ms": last[0].get("phases_ms")}),
              flush=True)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--skip-calls", action="store_true")
    ap.add_argument("--skip-train", action="store_true")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("llama_packed_bench needs a GPU: times are not measured without one")
    dev = torch.device("cuda", 0)
    if not args.skip_calls:
        bench_calls(dev, args.reps)
    if not args.skip_train:
        bench_train(args.reps, args.steps, args.warmup)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
