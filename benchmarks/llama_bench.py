#!/usr/bin/env python3
"""Llama-family kernels and pretraining throughput on one GPU.

    python benchmarks/llama_bench.py [--reps 3] [--skip-ops] [--skip-train] [--steps 10] [--warmup 6]

(a) Per-op times.  Each of the six kernels of ``csrc/kernels/llama.hip`` -- RMSNorm, RoPE + GQA pack and SwiGLU,
    forward and backward (RMSNorm's without the bridged residual
    gradient) -- at SmolLM-135M and SmolLM-1.7B row shapes (B S = 16384 rows), bf16, against its torch
    reference composition (``ops.llama.*_reference`` and its autograd backward) on the same tensors.  Call times
    from device events around back-to-back calls (launch overhead and the output allocation included), every
    call on another copy of the inputs (copies totalling >= 512 MB, beyond what the caches hold); the arms
    alternate, best of ``--reps``.  GB/s counts the bytes the op has to move (its bf16 inputs once, its bf16
    outputs once), next to the 6.3 TB/s streaming rate.
(b) Training tokens/s of the ``llama_pretrain`` preset with the native ops (``auto``) against ``off``: the same
    model through the reference ops on the GPU.  A fresh Trainer per run, the arms alternating in this one
    process, best of ``--reps``.
One JSON line per result.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ROTATE_BYTES = 512 << 20
STREAM_GBS = 6300.0
ROWS = 16384
SHAPES = {"smollm_135m": dict(E=576, H=9, Hkv=3, I=1536), "smollm_1p7b": dict(E=2048, H=32, Hkv=32, I=8192)}


def _events(fn, iters):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for i in range(iters):
        fn(i)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / iters      # us per call


def _copies(nbytes):
    return max(2, min(16, -(-ROTATE_BYTES // nbytes)))


def _ab(name, shape, ours, ref, nbytes, reps, iters=40):
    for fn in (ours, ref):
        fn(0)
        _events(fn, 5)
    t_o, t_r = [], []
    for _ in range(reps):
        t_o.append(_events(ours, iters))
        t_r.append(_events(ref, iters))
    o, r = min(t_o), min(t_r)
    print(json.dumps({"kernel": name, "shape": shape, "us": round(o, 1), "reference_us": round(r, 1),
                      "GBps": round(nbytes / o / 1e3, 1), "reference_GBps": round(nbytes / r / 1e3, 1),
                      "share_of_stream": round(nbytes / o / 1e3 / STREAM_GBS, 3), "speedup": round(r / o, 2),
                      "faster_than_reference": bool(o < r)}), flush=True)


def bench_ops(dev, reps):
    import torch
    from databricks_distributed_deep_learning_amd import ops
    from databricks_distributed_deep_learning_amd.ops import llama as L
    bf = torch.bfloat16
    table = ops.rope_table(2048, 1e4).to(dev)
    B, S = ROWS // 2048, 2048

    def backward_arms(outs_n, outs_r, leaves_n, leaves_r, grads):
        """Backward alone: the graph is built once per copy and kept."""
        def nat(i):
            k = i % len(outs_n)
            torch.autograd.grad(outs_n[k], leaves_n[k], grads[k], retain_graph=True)

        def ref(i):
            k = i % len(outs_r)
            torch.autograd.grad(outs_r[k], leaves_r[k], grads[k], retain_graph=True)
        return nat, ref

    for model, d in SHAPES.items():
        E, H, Hkv, I = d["E"], d["H"], d["Hkv"], d["I"]
        # ---------------- RMSNorm
        n = _copies(ROWS * E * 2)
        xs = [torch.randn(ROWS, E, device=dev).to(bf).requires_grad_(True) for _ in range(n)]
        w = (torch.rand(E, device=dev) + 0.5).to(bf).requires_grad_(True)
        shape = f"{model} [{ROWS}, {E}]"
        with torch.no_grad():
            _ab("rmsnorm_fwd", shape, lambda i: ops.rms_norm(xs[i % n], w, 1e-5),
                lambda i: L.rms_norm_reference(xs[i % n], w, 1e-5), 2 * ROWS * E * 2, reps)
        dys = [torch.randn(ROWS, E, device=dev).to(bf) for _ in range(n)]
        yn = [ops.rms_norm(x, w, 1e-5) for x in xs]
        yr = [L.rms_norm_reference(x, w, 1e-5) for x in xs]
        nat, ref = backward_arms(yn, yr, [(x, w) for x in xs], [(x, w) for x in xs], dys)
        _ab("rmsnorm_bwd", shape, nat, ref, 3 * ROWS * E * 2, reps)
        del xs, dys, yn, yr
        # ---------------- RoPE + GQA pack
        win, wout = (H + 2 * Hkv) * 64, 3 * H * 64
        n = _copies(ROWS * win * 2)
        qs = [torch.randn(B, S, win, device=dev).to(bf).requires_grad_(True) for _ in range(n)]
        shape = f"{model} [{B}, {S}, ({H}+2*{Hkv})*64]"
        with torch.no_grad():
            _ab("rope_qkv_fwd", shape, lambda i: ops.rope_qkv(qs[i % n], table, H, Hkv),
                lambda i: L.rope_qkv_reference(qs[i % n], table, H, Hkv), ROWS * (win + wout) * 2, reps)
        dos = [torch.randn(B, S, wout, device=dev).to(bf) for _ in range(n)]
        on = [ops.rope_qkv(q, table, H, Hkv) for q in qs]
        orf = [L.rope_qkv_reference(q, table, H, Hkv) for q in qs]
        nat, ref = backward_arms(on, orf, [(q,) for q in qs], [(q,) for q in qs], dos)
        _ab("rope_qkv_bwd", shape, nat, ref, ROWS * (win + wout) * 2, reps)
        del qs, dos, on, orf
        # ---------------- SwiGLU
        n = _copies(ROWS * 2 * I * 2)
        gs = [torch.randn(ROWS, 2 * I, device=dev).to(bf).requires_grad_(True) for _ in range(n)]
        shape = f"{model} [{ROWS}, 2*{I}]"
        with torch.no_grad():
            _ab("swiglu_fwd", shape, lambda i: ops.swiglu(gs[i % n]), lambda i: L.swiglu_reference(gs[i % n]),
                ROWS * 3 * I * 2, reps)
        dz = torch.randn(ROWS, I, device=dev).to(bf)
        zn = [ops.swiglu(g) for g in gs]
        zr = [L.swiglu_reference(g) for g in gs]
        nat, ref = backward_arms(zn, zr, [(g,) for g in gs], [(g,) for g in gs], [dz] * n)
        _ab("swiglu_bwd", shape, nat, ref, ROWS * 5 * I * 2, reps)
        del gs, zn, zr
        torch.cuda.empty_cache()


def bench_train(reps, steps, warmup):
    import torch
    from databricks_distributed_deep_learning_amd import ops
    from databricks_distributed_deep_learning_amd.config import get_preset
    from databricks_distributed_deep_learning_amd.training.loop import Trainer
    runs = {"auto": [], "off": []}
    last = {}
    for _ in range(reps):
        for arm in ("auto", "off"):
            ops.set_native_mode(arm)     # a Trainer only ever switches the mode away from "auto"
            t = Trainer(get_preset("llama_pretrain", native=arm, steps=steps, warmup_steps=warmup, log_every=0))
            out = t.run()
            t.close()
            del t
            torch.cuda.empty_cache()
            assert out["native"] == arm, (out["native"], arm)
            runs[arm].append(out["samples_per_sec"] * out["seq_len"])
            last[arm] = out
    ops.set_native_mode("auto")
    a, o = max(runs["auto"]), max(runs["off"])
    out = last["auto"]
    print(json.dumps({"train": out["model"], "per_rank_batch": out["per_rank_batch"], "seq_len": out["seq_len"],
                      "params": out["params"], "native_tokens_per_sec": round(a, 1),
                      "reference_ops_tokens_per_sec": round(o, 1), "speedup": round(a / o, 3),
                      "native_faster": bool(a > o), "native_final_loss": last["auto"]["final_loss"],
                      "reference_final_loss": last["off"]["final_loss"],
                      "native_tokens_per_sec_all": [round(v, 1) for v in runs["auto"]],
                      "reference_tokens_per_sec_all": [round(v, 1) for v in runs["off"]],
                      "plan_source": out.get("plan_source"), "phases_ms": out.get("phases_ms"),
                      "peak_mem_gb": out.get("max_allocated_gb")}), flush=True)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--skip-ops", action="store_true")
    ap.add_argument("--skip-train", action="store_true")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("llama_bench needs a GPU: times are not measured without one")
    dev = torch.device("cuda", 0)
    if not args.skip_ops:
        bench_ops(dev, args.reps)
    if not args.skip_train:
        bench_train(args.reps, args.steps, args.warmup)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
